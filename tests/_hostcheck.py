"""
The one place that compiles and runs host programs for the tests.

A host checker is a small C++ file under tests/hostcheck*/ that drives one csrc/*_math.hpp header on the CPU. Two kinds:

  'program'  its own main: reads a request file, writes a result file, exit code 0 / 2 (refused) / other (broken);
  'library'  extern "C" entry points loaded with ctypes; a define turns on a stand-alone main of the same entry points.

build() compiles into one temporary directory per process, outside the repository, at most once per (name, sanitize).
build(name, sanitize=True) ALWAYS yields a stand-alone executable -- the program itself, or a library's -D..._MAIN driver -- and never
a shared object: a sanitizer does not check code loaded into the Python interpreter (its runtime would have to be loaded before
everything else, which no test here does), so a sanitized library would load, run and prove nothing. The sanitized executables run as
processes of their own.

By hand:  python tests/_hostcheck.py NAME [--sanitize]   builds one checker and prints its path.
"""
import atexit
import collections
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)

LIBRARY = ['-O1', '-ffp-contract=off', '-std=c++17']                       # + -shared -fPIC, or + -D<main> for the stand-alone driver
PROGRAM = ['-O1', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas']       # `#pragma unroll` / `clang fp` are hipcc's
SANITIZE = ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']

Checker = collections.namedtuple('Checker', 'name source kind flags main')


def _entry(name, kind, flags, main=None):
    return Checker(name, os.path.join(TESTS, name, name + '.cpp'), kind, flags, main)


REGISTRY = {c.name: c for c in (
    _entry('hostcheck', 'library', LIBRARY),                                    # no stand-alone main
    _entry('hostcheck_aug', 'library', LIBRARY, 'HC_AUG_MAIN'),
    _entry('hostcheck_ict', 'library', LIBRARY, 'HC_ICT_MAIN'),
    _entry('hostcheck_stage', 'library', LIBRARY, 'HC_STAGE_MAIN'),
    _entry('hostcheck_stage_pair', 'library', LIBRARY, 'HC_STAGE_PAIR_MAIN'),
    _entry('hostcheck_tta', 'program', PROGRAM),
    _entry('hostcheck_classmix', 'program', PROGRAM),
    _entry('hostcheck_boundary', 'program', PROGRAM),
    _entry('hostcheck_surface', 'program', PROGRAM),
    _entry('hostcheck_cowmask', 'program', PROGRAM),
    _entry('hostcheck_convert', 'program', PROGRAM),
    _entry('hostcheck_resize', 'program', PROGRAM),
    _entry('hostcheck_cps', 'program', PROGRAM),
    _entry('hostcheck_crf', 'program', PROGRAM),
    _entry('hostcheck_calib', 'program', PROGRAM),
    _entry('hostcheck_window', 'program', PROGRAM),
    # its own flags: the driver includes "cthresh_math.hpp" by name (-I), and its tests have only ever run at -O2 without -Wall
    _entry('hostcheck_cthresh', 'program', ['-O2', '-std=c++17', '-I', os.path.join(REPO, 'cutmix-semisup-seg_amd', 'csrc')]),
)}

_dir = []
_built = {}
_requests = [0]


def directory():
    """the process's temporary directory, made on first use and removed at exit"""
    if not _dir:
        _dir.append(tempfile.mkdtemp(prefix='hostcheck_'))
        atexit.register(shutil.rmtree, _dir[0], ignore_errors=True)
    return _dir[0]


def _compile(cmd):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if p.returncode != 0:
        raise RuntimeError('{}\nexit code {}:\n{}'.format(' '.join(cmd), p.returncode, p.stdout.decode(errors='replace')))


def build(name, sanitize=False):
    """compile the checker `name` -> the path of its executable (a program; anything with sanitize=True) or shared object (a library)"""
    if (name, sanitize) not in _built:
        c = REGISTRY[name]
        flags = list(c.flags)
        if sanitize:
            if c.kind == 'library' and c.main is None:
                raise ValueError('{} has no stand-alone main to run under the sanitizers'.format(name))
            out = name + '_asan'
            flags += SANITIZE + (['-D' + c.main] if c.kind == 'library' else [])
        elif c.kind == 'library':
            out = 'lib{}.so'.format(name)
            flags += ['-shared', '-fPIC']
        else:
            out = name
        out = os.path.join(directory(), out)
        _compile(['g++'] + flags + [c.source, '-o', out])
        _built[(name, sanitize)] = out
    return _built[(name, sanitize)]


def load(name):
    """the library-kind checker `name`, loaded with ctypes"""
    assert REGISTRY[name].kind == 'library', name
    return ctypes.CDLL(build(name))


def run(exe, header, blocks=(), expect_code=0, args=()):
    """One request through a program: `header` (packed bytes), then every (array, dtype) of `blocks` written contiguously. The
    program runs as a child process, `exe [args...] REQUEST RESULT`, and must end with `expect_code`.
    -> the result file's bytes, or None for a non-zero expected code."""
    _requests[0] += 1
    req, res = (os.path.join(directory(), '{}{}.bin'.format(k, _requests[0])) for k in ('req', 'res'))
    try:
        with open(req, 'wb') as f:
            f.write(header)
            for a, dtype in blocks:
                f.write(np.ascontiguousarray(a, dtype=dtype).tobytes())
        code = subprocess.call([exe] + list(args) + [req, res])
        assert code == expect_code, code
        if code != 0:
            return None
        with open(res, 'rb') as f:
            return f.read()
    finally:
        for p in (req, res):
            if os.path.exists(p):
                os.remove(p)


def split(raw, fields):
    """`raw` cut into the ordered `fields` [(name, dtype, shape)] -> {name: read-only array}. The length must be exactly theirs."""
    sizes = [np.dtype(dtype).itemsize * int(np.prod(shape, dtype=np.int64)) for _, dtype, shape in fields]
    assert len(raw) == sum(sizes), (len(raw), sizes)
    out, at = {}, 0
    for (name, dtype, shape), size in zip(fields, sizes):
        out[name] = np.frombuffer(raw[at:at + size], dtype=dtype).reshape(shape)
        at += size
    return out


def compile_against_header(c_source, directory):
    """a C snippet compiled against include/cutmixseg.h with the host C compiler, into `directory` -> the executable"""
    src, exe = os.path.join(str(directory), 't.c'), os.path.join(str(directory), 't')
    with open(src, 'w') as f:
        f.write(c_source)
    _compile(['gcc', '-I', os.path.join(REPO, 'include'), src, '-o', exe])
    return exe


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description='build one host checker and print its path')
    ap.add_argument('name', choices=sorted(REGISTRY))
    ap.add_argument('--sanitize', action='store_true', help='the stand-alone executable under the address and UB sanitizers')
    a = ap.parse_args()
    _dir.append(tempfile.mkdtemp(prefix='hostcheck_'))   # built by hand, the product is the point: this directory stays
    print(build(a.name, a.sanitize))
