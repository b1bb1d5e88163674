#!/usr/bin/env python
"""
Generate tests/golden/trainer_cli_full.json: the COMPLETE command-line surface of this build's four trainers -- every option of
`experiment.params` in order, this build's additions and their positions included (the reference goldens cli_options.json,
cli_options_vat.json, ict_cli.json and aug_cli.json pin the reference's options only).

    python tests/golden/make_trainer_cli_golden.py

Run it on the commit whose surface is to be pinned (it was written from the last commit with one option table per trainer file);
its output, a small JSON file holding only settings, is committed and is all tests/test_trainer_common_cpu.py reads.
"""
import importlib
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TRAINERS = ('train_seg_semisup_mask_mt', 'train_seg_semisup_vat_mt', 'train_seg_semisup_ict', 'train_seg_semisup_aug_mt')


def surface(experiment):
    """The ordered option records of a click command (shared with the test that compares against the file)."""
    import click
    opts = []
    for prm in experiment.params:
        choices = list(prm.type.choices) if isinstance(prm.type, click.Choice) else None
        opts.append(dict(name=prm.name, opts=list(prm.opts), type=type(prm.type).__name__,
                         # an option without a default is None here, whatever this click version calls "unset"
                         default=prm.default if isinstance(prm.default, (bool, int, float, str)) else None,
                         is_flag=bool(getattr(prm, 'is_flag', False)), choices=choices))
    return opts


def main():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    out = {name: surface(importlib.import_module('cutmix_semisup_seg_amd.' + name).experiment) for name in TRAINERS}
    with open(os.path.join(HERE, 'trainer_cli_full.json'), 'w') as f:
        json.dump(out, f, indent=0)
    print('wrote trainer_cli_full.json ({})'.format(', '.join('{}: {}'.format(k, len(v)) for k, v in out.items())))


if __name__ == '__main__':
    main()
