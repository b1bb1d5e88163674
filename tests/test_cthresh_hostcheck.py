"""
CPU-only: csrc/cthresh_math.hpp -- the per-pixel pieces and the update arithmetic the kernels of csrc/cthresh.hip are made of -- driven on
the host by a small stand-alone program of its own (tests/hostcheck_cthresh), over every pixel of the GPU test's cases
against the fp64 restatement (tests/_cthresh_refs.py): k*, the pass bit, N_pred / N_pass exactly, S_conf / S_c within the bound; the
update on hand-made integer tables; then what a margin cannot hold -- equal logits, a confidence exactly at its threshold, NaN logits,
one class -- and the same program once more under the host's address and undefined-behaviour sanitizers. Nothing is loaded into Python.
"""
import struct

import numpy as np
import pytest

import _cthresh_refs as R
import _hostcheck

def run_pixels(exe, l0, l1, thr, size, align, mode, ranges=None, mask=None, um0=None, um1=None, expect_code=0):
    n, c, h, w = l0.shape
    H, W = size
    nb = 0 if ranges is None else int(np.asarray(ranges).shape[1])
    flags = (1 if l1 is not None else 0) | (2 if mask is not None else 0) | (4 if um0 is not None else 0) | (8 if um1 is not None else 0)
    header = struct.pack('<10i', n, c, h, w, H, W, int(align), 0 if mode == 'mix' else 1, nb, flags)
    blocks = [(l0, np.float32)] + ([(l1, np.float32)] if l1 is not None else []) + [(thr, np.float32)]
    blocks += [(ranges, np.int32)] if ranges is not None else []
    blocks += [(m, np.float32) for m in (mask, um0, um1) if m is not None]
    raw = _hostcheck.run(exe, header, blocks, expect_code, args=['pixels'])
    if raw is None:
        return None
    out = _hostcheck.split(raw, [('kstar', np.int32, (n, H, W)), ('passed', np.uint8, (n, H, W)), ('table', np.uint64, (2 + 3 * c,))])
    return dict(kstar=out['kstar'], passed=out['passed'] > 0, table=[int(v) for v in out['table']])


def run_update(exe, C, adaptive, lam, floor, ceil, state, thr, table, epoch, expect_code=0):
    header = struct.pack('<2i3d', C, int(adaptive), lam, floor, ceil)
    blocks = [(state, np.float64), (thr, np.float32), (table, np.uint64), (epoch, np.uint64)]
    raw = _hostcheck.run(exe, header, blocks, expect_code, args=['update'])
    if raw is None:
        return None
    out = _hostcheck.split(raw, [('state', np.float64, (1 + C,)), ('thr', np.float32, (C,)), ('table', np.uint64, (2 + 3 * C,)),
                                 ('epoch', np.uint64, (1 + 2 * C,))])
    return list(out['state']), list(out['thr']), [int(v) for v in out['table']], [int(v) for v in out['epoch']]


@pytest.fixture(scope='module')
def host():
    return _hostcheck.build('hostcheck_cthresh')


def _check_case(exe, case, vec):
    name, mode, fn, pp, given = case
    N, C, h, w, H, W, ac = R.geometry(name)
    i, ref, rows = R.inputs(case), R.reference(case, vec), R.rows_of(case)
    assert ref['gap'] >= R.GAP and ref['conf_margin'] >= R.CONF
    got = run_pixels(exe, i['l0'], i['l1'], ref['thr'], (H, W), ac, mode, i['ranges'], i['mask'], i['um0'], i.get('um1'))
    assert np.array_equal(got['kstar'], rows['kstar'])
    want_pass = rows['conf'] >= ref['thr'].astype(np.float64)[rows['kstar']]
    assert np.array_equal(got['passed'], want_pass)
    t, b = ref['table'], ref['table_bound']
    assert got['table'][0] == t[0] and got['table'][2 + C:] == t[2 + C:]          # n_valid, N_pred, N_pass: equal
    for k in range(1, 2 + C):
        assert abs(got['table'][k] - t[k]) <= b[k], (k, got['table'][k], t[k], b[k])


@pytest.mark.parametrize('case', R.CASES + [R.REFUSED], ids=R.case_id)
def test_header_on_the_host_vs_restatement_every_pixel(host, case):
    for vec in R.VECTORS:
        _check_case(host, case, vec)


# ------------------------------------------------------------------------------------------------------------ the update
def _tables():
    """hand-made integer tables: (C, table) with n_valid pixels whose fixed-point sums are consistent (sum_c S_c ~ n_valid 2^24)"""
    one = 1 << 24
    return {
        'first': (3, [10, 8 * one, 5 * one, 3 * one, 2 * one, 6, 3, 1, 4, 1, 0]),
        'empty': (3, [0] * 11),
        'twice': (4, [8, 6 * one, 3 * one, 3 * one, one, one, 4, 4, 0, 0, 2, 1, 0, 0]),         # max_j p~_j attained twice
        'low': (2, [5, one // 2, 4 * one, one, 5, 0, 0, 0]),                                   # a tiny mean confidence: the floor
        'high': (2, [5, 5 * one, 5 * one, 0, 5, 0, 5, 0]),                                     # confidence 1 everywhere: the ceiling
    }


def _same_update(got, want, C):
    gs, gt, gtab, gep = got
    ws, wt, wtab, wep = want
    assert gs == ws, (gs, ws)                                                  # fp64, no contraction: bit for bit
    assert [np.float32(v) for v in gt] == [np.float32(v) for v in wt]
    assert gtab == wtab and gep == wep


@pytest.mark.parametrize('lam,floor,ceil', [(0.999, 0.0, 0.97), (0.5, 0.0, 0.97), (0.0, 0.3, 0.6), (0.5, 0.25, 1.0)])
def test_update_on_hand_made_tables(host, lam, floor, ceil):
    for name, (C, table) in _tables().items():
        state, thr = R.initial(C, floor, ceil)
        epoch = [7] + [3] * (2 * C)
        want = R.update(state, thr, table, epoch, C, True, lam, floor, ceil)
        got = run_update(host, C, True, lam, floor, ceil, state, thr, table, epoch)
        _same_update(got, want, C)
        assert got[2] == [0] * (2 + 3 * C) and got[3][0] == 7 + table[0]
        if name == 'empty':
            assert got[0] == state and [float(v) for v in got[1]] == [float(v) for v in thr]          # n_valid = 0: as it was
        if name == 'twice':
            assert got[0][1] == got[0][2] == max(got[0][1:]) and got[1][0] == got[1][1]
        assert all(np.float32(floor) <= v <= np.float32(ceil) for v in got[1])
        # static mode: only the counters move
        gs = run_update(host, C, False, lam, floor, ceil, state, thr, table, epoch)
        _same_update(gs, R.update(state, thr, table, epoch, C, False, lam, floor, ceil), C)
        assert gs[0] == state and [float(v) for v in gs[1]] == [float(v) for v in thr] and gs[3] == got[3]
    # three updates in a row
    C, table = _tables()['first']
    st, th = R.initial(C, floor, ceil)
    gs, gt, ep, gep = st, th, [0] * (1 + 2 * C), [0] * (1 + 2 * C)
    for k in range(3):
        tab = [v + k * (1 << 20) if 1 <= j < 2 + C else v for j, v in enumerate(table)]
        st, th, _, ep = R.update(st, th, tab, ep, C, True, lam, floor, ceil)
        gs, gt, _, gep = run_update(host, C, True, lam, floor, ceil, gs, gt, tab, gep)
        _same_update((gs, gt, [], gep), (st, th, [], ep), C)


def test_update_refusals(host):
    C, table = _tables()['first']
    st, th = R.initial(C)
    ep = [0] * (1 + 2 * C)
    for lam, floor, ceil in ((1.0, 0.0, 0.97), (-0.1, 0.0, 0.97), (0.5, 0.98, 0.97), (float('nan'), 0.0, 1.0)):
        run_update(host, C, True, lam, floor, ceil, st, th, table, ep, expect_code=2)


# ------------------------------------------------------------------------------------------------------------ what no margin holds
def test_equal_logits_lowest_index_wins_and_a_threshold_exactly_reached_passes(host):
    for C in (2, 4, 5):
        l0 = np.full((1, C, 2, 3), 1.5, dtype=np.float32)                       # uniform: conf = 1 / C exactly for powers of two
        l0[0, :, 1, 2] = np.arange(C)[::-1] * 0.0 + 1.5
        conf = np.float32(1.0) / np.float32(C)                                   # z = C exactly (C ones), one reciprocal
        for thr0, passes in ((conf, True), (np.nextafter(conf, np.float32(1)), False)):
            thr = np.full(C, 0.0, dtype=np.float32)
            thr[0] = thr0
            thr[1:] = 0.0                                                       # the other classes would always pass
            got = run_pixels(host, l0, None, thr, (5, 6), True, 'cut', mask=np.ones((1, 5, 6), np.float32))
            assert not got['kstar'].any()                                       # a tie of ALL classes: index 0
            assert got['passed'].all() == passes and got['passed'].any() == passes
            assert got['table'][0] == 30 and got['table'][2 + C] == 30 and got['table'][2 + 2 * C] == (30 if passes else 0)
            assert got['table'][1] == 30 * int(np.rint(float(conf) * 2 ** 24))
    # a tie of two classes above a third
    l0 = np.zeros((1, 3, 1, 1), dtype=np.float32)
    l0[0, :, 0, 0] = (-1.0, 2.0, 2.0)
    got = run_pixels(host, l0, None, np.zeros(3, np.float32), (2, 2), True, 'cut', mask=np.ones((1, 2, 2), np.float32))
    assert (got['kstar'] == 1).all()


def test_nan_logits_fail_and_corrupt_no_sum(host):
    g = np.random.RandomState(7)
    l0 = (g.standard_normal((1, 3, 4, 4)) * 3).astype(np.float32)
    clean = run_pixels(host, l0, None, np.zeros(3, np.float32), (4, 4), True, 'cut', mask=np.ones((1, 4, 4), np.float32))
    bad = l0.copy()
    bad[0, 1, 0, 0] = np.nan                                  # one class of one pixel
    bad[0, :, 3, 3] = np.nan                                  # a whole row of NaNs: no logit equals the maximum, k* = 0
    got = run_pixels(host, bad, None, np.zeros(3, np.float32), (4, 4), True, 'cut', mask=np.ones((1, 4, 4), np.float32))
    assert not got['passed'][0, 0, 0] and not got['passed'][0, 3, 3] and got['kstar'][0, 3, 3] == 0      # even against a threshold of 0
    keep = np.ones((4, 4), dtype=bool)
    keep[0, 0] = keep[3, 3] = False
    assert np.array_equal(got['passed'][0][keep], clean['passed'][0][keep]) and got['passed'][0][keep].all()
    assert got['table'][0] == 16 and sum(got['table'][5:8]) == 16 and sum(got['table'][8:11]) == 14
    # the two NaN pixels add nothing to S_conf / S_c: the sums are those of the other fourteen
    only = run_pixels(host, l0, None, np.zeros(3, np.float32), (4, 4), True, 'cut', mask=np.ones((1, 4, 4), np.float32),
                      um0=keep.astype(np.float32)[None])
    assert got['table'][1:5] == only['table'][1:5] and all(v < 16 << 24 for v in got['table'][1:5])


def test_one_class(host):
    g = np.random.RandomState(3)
    l0 = (g.standard_normal((2, 1, 3, 3)) * 3).astype(np.float32)
    for thr, n_pass in ((1.0, 70), (0.5, 70)):               # the confidence is exactly 1 and reaches a threshold of 1
        got = run_pixels(host, l0, None, np.full(1, thr, np.float32), (5, 7), False, 'cut', mask=np.zeros((2, 5, 7), np.float32))
        assert not got['kstar'].any() and got['passed'].all()
        assert got['table'] == [70, 70 << 24, 70 << 24, 70, n_pass]


def test_host_driver_refuses_bad_arguments(host):
    l0 = np.zeros((1, 3, 2, 2), np.float32)
    ok = dict(mask=np.ones((1, 4, 4), np.float32))
    run_pixels(host, l0, None, np.zeros(3, np.float32), (4, 4), True, 'mix', expect_code=2, **ok)       # mix needs l1
    run_pixels(host, l0, None, np.zeros(3, np.float32), (1, 4), True, 'cut', expect_code=2, **ok)       # logits larger
    run_pixels(host, l0, None, np.zeros(3, np.float32), (4, 4), True, 'cut', expect_code=2)             # no mask at all


def test_stand_alone_under_the_host_sanitizers(host):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_cthresh', sanitize=True)
    for case in (R.CASES[0], R.CASES[1], R.CASES[2], R.CASES[5], R.CASES[8], R.CASES[10]):
        _check_case(exe, case, 'ascending')
    C, table = _tables()['twice']
    st, th = R.initial(C)
    ep = [0] * (1 + 2 * C)
    _same_update(run_update(exe, C, True, 0.5, 0.0, 0.97, st, th, table, ep), R.update(st, th, table, ep, C, True, 0.5, 0.0, 0.97), C)
