"""Drop-in script name of the reference (`python intra_inter_class_patch_dist.py OUT_PATH --flags...`); the program lives in
cutmix-semisup-seg_amd/intra_inter_class_patch_dist.py."""
from cutmix_semisup_seg_amd.intra_inter_class_patch_dist import intra_inter_class_patch_dist, class_distances  # noqa: F401

if __name__ == '__main__':
    intra_inter_class_patch_dist()
