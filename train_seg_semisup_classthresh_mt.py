"""`python train_seg_semisup_classthresh_mt.py --flags...`: the class-threshold CutMix trainer, a script beside the reference's four;
it lives in cutmix-semisup-seg_amd/train_seg_semisup_classthresh_mt.py."""
from cutmix_semisup_seg_amd.train_seg_semisup_classthresh_mt import train_seg_semisup_classthresh_mt, experiment  # noqa: F401

if __name__ == '__main__':
    experiment()
