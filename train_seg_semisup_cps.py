"""`python train_seg_semisup_cps.py --flags...`: the cross-pseudo-supervision trainer, a script beside the reference's four; it lives in
cutmix-semisup-seg_amd/train_seg_semisup_cps.py."""
from cutmix_semisup_seg_amd.train_seg_semisup_cps import train_seg_semisup_cps, experiment  # noqa: F401

if __name__ == '__main__':
    experiment()
