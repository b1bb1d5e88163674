"""
CPU-only: tests/_hostcheck.py, the one place that compiles and runs the host checkers -- its registry against the directories, the
one-compile-per-process rule, what `sanitize=True` yields for a library, a compiler error's message, and split()'s length check.
"""
import glob
import os

import numpy as np
import pytest

import _hostcheck as H


def test_every_checker_directory_is_registered_and_every_source_exists():
    with_cpp = {os.path.basename(d) for d in glob.glob(os.path.join(H.TESTS, 'hostcheck*')) if glob.glob(os.path.join(d, '*.cpp'))}
    assert with_cpp == set(H.REGISTRY)
    for c in H.REGISTRY.values():
        assert os.path.isfile(c.source), c.source
        assert c.kind in ('program', 'library') and (c.main is None or c.kind == 'library')
    assert not glob.glob(os.path.join(H.TESTS, '**', 'Makefile'), recursive=True)


def test_the_same_build_twice_compiles_once(monkeypatch):
    compiles = []
    compile_ = H._compile
    monkeypatch.setattr(H, '_compile', lambda cmd: (compiles.append(cmd), compile_(cmd)))
    monkeypatch.setattr(H, '_built', {})                              # whatever other tests of this process have built already
    first = H.build('hostcheck_convert')
    assert H.build('hostcheck_convert') == first and len(compiles) == 1
    assert os.access(first, os.X_OK) and not first.startswith(H.REPO + os.sep)


def test_a_sanitized_library_is_a_stand_alone_executable():
    exe = H.build('hostcheck_stage_pair', sanitize=True)
    assert H.REGISTRY['hostcheck_stage_pair'].kind == 'library' and not exe.endswith('.so')
    with open(exe, 'rb') as f:
        head = f.read(4)
    assert head == b'\x7fELF' and os.access(exe, os.X_OK)
    assert exe != H.build('hostcheck_stage_pair') and H.build('hostcheck_stage_pair').endswith('.so')
    with pytest.raises(ValueError, match='no stand-alone main'):
        H.build('hostcheck', sanitize=True)


def test_a_source_that_does_not_compile_raises_with_the_compilers_output(tmp_path, monkeypatch):
    src = tmp_path / 'broken.cpp'
    src.write_text('int main() {\n    return no_such_name; }\n')
    monkeypatch.setitem(H.REGISTRY, 'broken', H.Checker('broken', str(src), 'program', H.PROGRAM, None))
    with pytest.raises(RuntimeError, match='no_such_name'):
        H.build('broken')
    assert ('broken', False) not in H._built


def test_split_refuses_a_result_of_another_length():
    fields = [('a', np.uint8, (3,)), ('b', np.int32, (2, 2)), ('c', np.float64, (1,))]
    raw = bytes(range(27))
    out = H.split(raw, fields)
    assert out['a'].tolist() == [0, 1, 2] and out['b'].shape == (2, 2) and out['b'].dtype == np.int32 and out['c'].shape == (1,)
    assert out['b'].tobytes() == raw[3:19]
    for bad in (raw[:-1], raw + b'\0'):
        with pytest.raises(AssertionError):
            H.split(bad, fields)
