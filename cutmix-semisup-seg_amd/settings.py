"""
Mirror of the reference's settings.py: where the data sets live. The location of a data set is read from
`./semantic_segmentation.cfg` (the working directory the trainer is started from), section `[paths]`:

    [paths]
    pascal_voc=/data/VOCdevkit/VOC2012

(settings.py:16-49 of the reference; its dnnlib branch -- a cluster submission library -- is not reproduced.)
Host-side plumbing only.
"""
import os
from configparser import RawConfigParser, NoOptionError, NoSectionError

_CONFIG_PATH = './semantic_segmentation.cfg'


class DataPathError(RuntimeError):
    """The configuration names no location for a data set, or the location does not exist (the reference raises a plain
    RuntimeError for the second and a configparser error for the first)."""

_config__ = None
_config_key__ = None


def get_config():
    """The parsed configuration file of the current working directory (cached per file and modification time: the reference
    caches for the life of the process, which never changes its directory)."""
    global _config__, _config_key__
    path = os.path.abspath(_CONFIG_PATH)
    key = (path, os.path.getmtime(path) if os.path.exists(path) else None)
    if _config__ is None or key != _config_key__:
        _config__ = RawConfigParser()
        _config_key__ = key
        if key[1] is not None:
            try:
                _config__.read(path)
            except Exception as e:
                print('WARNING: error {} trying to open config file from {}'.format(e, _CONFIG_PATH))
                _config__ = RawConfigParser()
    return _config__


def get_config_dir(name, exists=True):
    try:
        dir_path = get_config().get('paths', name)
    except (NoSectionError, NoOptionError):
        raise DataPathError('semantic_segmentation.settings: no path `{}` in section [paths] of {} (the file holds the data set '
                           'locations; see README)'.format(name, _CONFIG_PATH))
    if exists:
        if not os.path.exists(dir_path):
            raise DataPathError(
                'semantic_segmentation.settings: the directory path {} does not exist'.format(dir_path))
    return dir_path


def get_data_path(config_name, dnnlib_template=None, exists=True):
    return get_config_dir(config_name, exists=exists)
