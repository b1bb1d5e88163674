"""`python train_seg_semisup_classmix_mt.py --flags...`: the ClassMix trainer, a script beside the reference's four; it lives in
cutmix-semisup-seg_amd/train_seg_semisup_classmix_mt.py."""
from cutmix_semisup_seg_amd.train_seg_semisup_classmix_mt import train_seg_semisup_classmix_mt, experiment  # noqa: F401

if __name__ == '__main__':
    experiment()
