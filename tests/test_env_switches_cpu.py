"""
CPU-only: the "Environment switches" table of INTEGRATION.md lists exactly the `CMS_*` environment variables the package
reads -- every name that is an argument of `os.environ.get(...)` / `os.environ[...]` in its Python sources or of `getenv(...)`
(or of a `*_env("...")` wrapper around it, csrc/wgrad8.hip) in its HIP sources. A new switch, or a retired one, shows up here
as a decision somebody has to write down. Reads text only.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(REPO, 'cutmix-semisup-seg_amd')
DOC = os.path.join(REPO, 'INTEGRATION.md')

_READ = re.compile(r"""(?:environ\.get\(|environ\[|getenv\(|_env\()\s*['"](CMS_[A-Z0-9_]+)['"]""")
_ROW = re.compile(r'^\|\s*`(CMS_[A-Z0-9_]+)`\s*\|')


def _names_read():
    names = {}
    for root, dirs, files in os.walk(PACKAGE):
        dirs[:] = [d for d in dirs if d != '__pycache__']
        for f in files:
            if not f.endswith(('.py', '.hip', '.hpp', '.h', '.cpp')):
                continue
            path = os.path.join(root, f)
            with open(path, encoding='utf-8') as fh:
                for name in _READ.findall(fh.read()):
                    names.setdefault(name, os.path.relpath(path, REPO))
    return names


def _names_documented():
    with open(DOC, encoding='utf-8') as fh:
        lines = fh.read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith('#') and l.rstrip().endswith('Environment switches'))
    rows = []
    for l in lines[start + 1:]:
        if l.startswith('#'):
            break
        m = _ROW.match(l)
        if m:
            rows.append(m.group(1))
    return rows


def test_switch_table_matches_the_sources():
    read = _names_read()
    rows = _names_documented()
    assert read, 'no environment switch found under {}: the collector is broken'.format(PACKAGE)
    assert len(rows) == len(set(rows)), 'duplicate rows: {}'.format(sorted(r for r in set(rows) if rows.count(r) > 1))
    missing = {n: read[n] for n in set(read) - set(rows)}
    stale = sorted(set(rows) - set(read))
    assert not missing and not stale, ('INTEGRATION.md "Environment switches" is out of date -- read but not listed: {}; '
                                       'listed but no longer read: {}'.format(missing, stale))
