"""Drop-in script name of the reference (`python convert_isic.py ISIC_ZIPS_DIR [--out_size 248,248]`); the program lives in
cutmix-semisup-seg_amd/convert_isic.py."""
from cutmix_semisup_seg_amd.convert_isic import convert_isic, convert_archives  # noqa: F401

if __name__ == '__main__':
    convert_isic()
