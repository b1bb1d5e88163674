"""Drop-in module name of the reference (`patch_dist.py`); the implementation lives in cutmix-semisup-seg_amd/patch_dist.py."""
from cutmix_semisup_seg_amd import patch_dist as _impl

globals().update({_k: _v for _k, _v in vars(_impl).items() if not _k.startswith('__')})
