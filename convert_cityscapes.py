"""Drop-in script name of the reference (`python convert_cityscapes.py LEFTIMG8BIT_ZIP GTFINE_ZIP [--downsample 2]`); the program
lives in cutmix-semisup-seg_amd/convert_cityscapes.py."""
from cutmix_semisup_seg_amd.convert_cityscapes import convert, convert_archives  # noqa: F401

if __name__ == '__main__':
    convert()
