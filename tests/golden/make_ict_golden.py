#!/usr/bin/env python
"""
Generate tests/golden/ict_cli.json: the command-line surface of the reference's ICT trainer (train_seg_semisup_ict.py:508-559),
read off the click command of the reference's own module -- names, option strings, flags, defaults, types, choices.

    python tests/golden/make_ict_golden.py <path of a checkout of the reference>

Needs the reference's sources; its output (a small JSON file holding only settings) is committed and is all the tests read.
"""
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main(ref):
    ref = os.path.abspath(ref)
    # keep the repository root (which holds a same-named drop-in script) OFF the path; the reference goes first
    sys.path = [p for p in sys.path if os.path.abspath(p or '.') not in (REPO, HERE)]
    sys.path.insert(0, ref)
    import click
    import train_seg_semisup_ict as ref_trainer      # reference (the module body only defines the job and the click command)
    assert os.path.abspath(ref_trainer.__file__).startswith(ref)
    opts = []
    for prm in ref_trainer.experiment.params:
        kind = type(prm.type).__name__
        choices = list(prm.type.choices) if isinstance(prm.type, click.Choice) else None
        opts.append(dict(name=prm.name, opts=list(prm.opts), is_flag=bool(getattr(prm, 'is_flag', False)),
                         default=prm.default if not callable(prm.default) else None, type=kind, choices=choices))
    with open(os.path.join(HERE, 'ict_cli.json'), 'w') as f:
        json.dump(opts, f, indent=0, default=str)
    print('wrote ict_cli.json ({} options)'.format(len(opts)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
