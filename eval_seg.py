"""Drop-in script name (`python eval_seg.py MODEL.pth --dataset pascal_aug [--scales 0.5,0.75,1 --flip]`); the program lives in
cutmix-semisup-seg_amd/eval_seg.py."""
from cutmix_semisup_seg_amd.eval_seg import experiment, evaluate  # noqa: F401

if __name__ == '__main__':
    experiment()
