"""
CPU-only: calibration and pseudo-label quality without a GPU.

  * the new ABI symbol: declared, exported, prototyped, its descriptor laid out as the C compiler lays it out; every CMS_EINVAL case
    (decided before any HIP call)
  * the fp64 restatement (tests/_calib_refs.py) against hand-worked tiny examples, and the conditions on the cases the GPU test shares:
    at most 1 % ambiguous pixels in every case, the top bins reached once per class count
  * the edge union, ECE by merging sub-bins against ECE on equal-width bins directly, suffix sums against direct threshold counts,
    every derived score of evaluation.EvaluatorCalibration from injected integer tables
  * every refusal of eval_seg.prepare / the command line with torch's GPU never touched, and the command-line surface
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
import _hostcheck
import _calib_refs as R
import _pascal_tree


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_symbol_is_declared_exported_and_prototyped():
    from cutmix_semisup_seg_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'cutmixseg.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+cms_calib_accumulate\s*\(const cms_calib_desc\* d, void\* stream\);', header)
    assert '#define CMS_CALIB_MAX_BINS 48' in header and '#define CMS_CALIB_MAX_TEMPS 8' in header
    assert hasattr(_lib.lib, 'cms_calib_accumulate')
    assert _lib.PROTOTYPES['cms_calib_accumulate'] == (ctypes.c_int, [ctypes.POINTER(_lib.CalibDesc), ctypes.c_void_p])
    assert (_lib.CALIB_MAX_BINS, _lib.CALIB_MAX_TEMPS) == (48, 8)


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from cutmix_semisup_seg_amd import _lib
    fields = ('h', 'n', 'labels', 'pred_out', 'nb', 'edges', 'nt', 'temps', 'hist', 'scores')
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cutmixseg.h"\nint main(void) { printf("%zu' + ' %zu' * len(fields) +
            '\\n", sizeof(cms_calib_desc)' + ''.join(', offsetof(cms_calib_desc, {})'.format(f) for f in fields) + '); return 0; }\n')
    sizes = [int(v) for v in subprocess.check_output([_hostcheck.compile_against_header(prog, tmp_path)]).decode().split()]
    D = _lib.CalibDesc
    assert sizes == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields]


def test_bad_descriptors_return_einval_before_any_hip_call():
    """No GPU here: a call that got past its argument checks would fail in the HIP runtime with another code."""
    from cutmix_semisup_seg_amd import _lib
    f, err = _lib.fn['cms_calib_accumulate'], _lib.fn['cms_last_error']
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value                       # host memory: never dereferenced before the launch
    edges = np.asarray([0.25, 0.5, 0.75], dtype=np.float32)
    temps = np.asarray([1.0, 2.0], dtype=np.float32)
    keep = []

    def desc(**over):
        d = _lib.CalibDesc()
        d.logits[0], d.h[0], d.w[0] = p, 3, 4
        d.logits[1], d.h[1], d.w[1] = p, 5, 6
        d.n, d.c, d.H, d.W, d.k, d.align_corners = 2, 3, 6, 7, 2, 1
        d.labels, d.label_dtype, d.ignore_index, d.cm, d.pred_out = p, _lib.LABEL_U8, 255, p, p
        d.nb, d.edges, d.nt, d.temps, d.hist, d.scores = 4, edges.ctypes.data, 2, temps.ctypes.data, p, p
        for key, val in over.items():
            if isinstance(val, np.ndarray):
                keep.append(val)
                val = val.ctypes.data
            setattr(d, key, val)
        return d
    assert f(None, None) == -1 and b'NULL descriptor' in err()
    f32 = lambda *v: np.asarray(v, dtype=np.float32)
    for what, over in (('views', dict(k=0)), ('views', dict(k=17)), ('num_classes', dict(c=0)), ('num_classes', dict(c=65)),
                       ('geometry', dict(n=0)), ('geometry', dict(H=0)), ('geometry', dict(W=-1)), ('label dtype', dict(label_dtype=5)),
                       ('2^31', dict(H=2 ** 16, W=2 ** 16)), ('labels', dict(labels=None)), ('labels NULL', dict(labels=None, cm=None)),
                       ('nothing to produce', dict(cm=None, pred_out=None)), ('hist NULL', dict(hist=None)),
                       ('scores NULL', dict(scores=None)), ('nb', dict(nb=0)), ('nb', dict(nb=49)), ('edges NULL', dict(edges=None)),
                       ('ascending', dict(edges=f32(0.5, 0.25, 0.75))), ('ascending', dict(edges=f32(0.25, 0.25, 0.75))),
                       ('(0, 1)', dict(edges=f32(0.0, 0.5, 0.75))), ('(0, 1)', dict(edges=f32(0.25, 0.5, 1.0))),
                       ('(0, 1)', dict(edges=f32(0.25, np.nan, 0.75))), ('(0, 1)', dict(edges=f32(-0.5, 0.5, 0.75))),
                       ('nt', dict(nt=0)), ('nt', dict(nt=9)), ('temps NULL', dict(temps=None)),
                       ('temperature', dict(temps=f32(0.0, 1.0))), ('temperature', dict(temps=f32(1.0, -2.0))),
                       ('temperature', dict(temps=f32(np.nan, 1.0))), ('temperature', dict(temps=f32(1.0, np.inf)))):
        assert f(ctypes.byref(desc(**over)), None) == -1, (what, over)
        assert what in err().decode(), (what, over, err())
    d = desc()
    d.logits[1] = None
    assert f(ctypes.byref(d), None) == -1 and b'logits NULL' in err()
    d = desc()
    d.h[1] = 0
    assert f(ctypes.byref(d), None) == -1 and b'below 1 x 1' in err()


def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


def test_op_refusals(monkeypatch):
    import torch
    from cutmix_semisup_seg_amd import ops
    _no_gpu(monkeypatch)
    lg = torch.zeros(2, 3, 4, 5)
    ok = dict(logits_list=[lg], flips=[False], num_classes=3, out_size=(8, 9), labels=torch.zeros(2, 8, 9, dtype=torch.uint8),
              edges=[0.5, 0.9], temps=[1.0], hist=torch.zeros(3, 3, 3, dtype=torch.int64), scores=torch.zeros(3, dtype=torch.int64))

    def refused(exc, what, **over):
        with pytest.raises(exc, match=what):
            ops.calibration_accumulate(**dict(ok, **over))
    refused(RuntimeError, 'GPU only')                                                  # CPU tensors, everything else in order
    refused(ValueError, 'views', logits_list=[])
    refused(ValueError, 'flips', flips=[False, True])
    refused(TypeError, r'\(N,C,h,w\)', logits_list=[lg[0]])
    refused(ValueError, 'num_classes', num_classes=65)
    refused(ValueError, 'a view of shape', num_classes=4)
    refused(TypeError, 'labels', labels=None)
    refused(TypeError, 'labels', labels=torch.zeros(2, 8, 9))
    refused(ValueError, 'labels of shape', labels=torch.zeros(2, 8, 8, dtype=torch.uint8))
    refused(ValueError, 'bins', edges=np.arange(1, 49) / 49.0, hist=torch.zeros(3, 49, 3, dtype=torch.int64))
    refused(ValueError, 'ascending', edges=[0.9, 0.5])
    refused(ValueError, 'ascending', edges=[0.5, 1.0])
    refused(ValueError, 'temperatures', temps=[])
    refused(ValueError, 'temperatures', temps=[1.0] * 9, scores=torch.zeros(11, dtype=torch.int64))
    refused(ValueError, 'temperature', temps=[0.0])
    refused(ValueError, 'temperature', temps=[float('nan')])
    refused(TypeError, 'hist must be', hist=torch.zeros(3, 3, 2, dtype=torch.int64))
    refused(TypeError, 'hist must be', hist=torch.zeros(3, 3, 3))
    refused(TypeError, 'scores must be', scores=torch.zeros(4, dtype=torch.int64))
    refused(TypeError, 'cm must be', cm=torch.zeros(3, 3))
    refused(TypeError, 'pred must be', pred=torch.zeros(2, 8, 9))
    refused(ValueError, '2\\^31', out_size=(2 ** 15, 2 ** 15))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_a_hand_worked_single_view():
    """two classes, one 1 x 2 view of the output's size: softmax(log 3, 0) = (0.75, 0.25), softmax(0, log 9) = (0.1, 0.9)"""
    lg = np.array([[[[math.log(3.0), 0.0]], [[0.0, math.log(9.0)]]]], dtype=np.float64)          # (1, 2, 1, 2)
    labels = np.array([[[0, 0]]], dtype=np.uint8)
    edges = np.array([0.5, 0.8], dtype=np.float32)
    ref = R.report([lg], [False], labels, (1, 2), True, edges, np.array([1.0, 2.0], dtype=np.float32))
    assert ref['pred'].tolist() == [[[0, 1]]] and ref['ambiguous'] == 0
    assert np.allclose(ref['conf'], [[[0.75, 0.9]]], atol=1e-12)
    want = np.zeros((2, 3, 3), dtype=np.int64)
    want[0, 1] = (1, 1, round(0.75 * 2 ** 24))
    want[1, 2] = (1, 0, round(0.9 * 2 ** 24))
    assert np.array_equal(ref['hist'], want) and np.array_equal(ref['cm'], [[1, 1], [0, 0]])
    brier = (0.25 ** 2 * 2) + (0.9 ** 2 * 2)
    nll1 = -math.log(0.75) - math.log(0.1)
    # T = 2 halves the logits: softmax(log 3 / 2, 0) = sqrt 3 / (1 + sqrt 3), softmax(0, log 9 / 2) = (1 / 4, 3 / 4)
    nll2 = -math.log(math.sqrt(3.0) / (1.0 + math.sqrt(3.0))) - math.log(0.25)
    assert ref['scores'].tolist() == [2, int(np.rint(0.125 * 2 ** 24) + np.rint(1.62 * 2 ** 24)),
                                      int(np.rint(-math.log(0.75) * 2 ** 20) + np.rint(-math.log(0.1) * 2 ** 20)),
                                      int(np.rint(-math.log(math.sqrt(3.0) / (1.0 + math.sqrt(3.0))) * 2 ** 20) + np.rint(-math.log(0.25) * 2 ** 20))]
    assert abs(ref['brier'].sum() - brier) < 1e-12 and abs(ref['nll'][0].sum() - nll1) < 1e-12 and abs(ref['nll'][1].sum() - nll2) < 1e-12


def test_restatement_on_a_hand_worked_vote_with_a_flip_and_an_ignored_pixel():
    """two views of a 1 x 2 output; the second is flipped, so its columns are read mirrored"""
    a = np.log(np.array([[[[3.0, 1.0]], [[1.0, 1.0]]]]))               # softmax -> (0.75, 0.25) | (0.5, 0.5)
    b = np.log(np.array([[[[1.0, 1.0]], [[1.0, 3.0]]]]))               # mirrored -> (0.5, 0.5) | (0.25, 0.75)... read as columns 1, 0
    labels = np.array([[[0, 255]]], dtype=np.uint8)
    ref = R.report([a, b], [False, True], labels, (1, 2), False, np.array([0.5], dtype=np.float32), np.array([1.0], dtype=np.float32))
    # pixel 0: view a (0.75, 0.25), view b's column 1 (0.25, 0.75) -> mean (0.5, 0.5): a tie, ambiguous between the two classes
    assert ref['scores'][0] == 1 and ref['ambiguous'] == 1 and ref['hist'].sum() == 0
    assert ref['maybe'][:, :, 0].sum() >= 2 and ref['maybe'][0, :, 1].sum() >= 1 and ref['maybe'][1, :, 1].sum() == 0
    assert abs(ref['nll'][0][0, 0, 0] - math.log(2.0)) < 1e-12 and abs(ref['brier'][0, 0, 0] - 0.5) < 1e-12
    # the ignored pixel 1: view a (0.5, 0.5), view b's column 0 (0.5, 0.5); it is predicted but not scored
    labels[0, 0, 1] = 1
    both = R.report([a, b], [False, True], labels, (1, 2), False, np.array([0.5], dtype=np.float32), np.array([1.0], dtype=np.float32))
    assert both['scores'][0] == 2


def test_bin_rule_puts_a_confidence_equal_to_an_edge_into_the_upper_bin():
    edges = R.make_edges(4, (0.97,))
    assert edges.dtype == np.float32 and edges.tolist() == [0.25, 0.5, 0.75, float(np.float32(0.97))]
    assert R.bin_of(np.array([0.0, 0.2499, 0.25, 0.75, float(np.float32(0.97)), 1.0]), edges).tolist() == [0, 0, 1, 3, 4, 4]


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_ambiguous_pixels_are_at_most_one_per_cent_in_every_case(name):
    inp, ref = R.case(name)
    scored = int(ref['scores'][0])
    print(name, 'ambiguous', ref['ambiguous'], '(edge', ref['edge_ambiguous'], 'tie', ref['tie_ambiguous'], ') of', scored)
    assert ref['ambiguous'] <= R.MAX_AMBIGUOUS * scored
    assert np.diff(inp['edges'].astype(np.float64)).min(initial=1.0) > 8 * R.B_CONF          # a pixel is near one edge at most
    if R.CASES[name]['ignore_all']:
        assert scored == 0 and not ref['hist'].any() and not ref['maybe'].any()
    elif inp['shape'] != (1, 1, 1):
        assert scored > 3000 and (~ref['valid']).sum() > 100                               # ignored pixels are among them


def test_cases_cover_what_they_should():
    cs = R.CASES
    grid = {(c['k'], c['c'], c['temps'][0]) for c in cs.values() if len(c['temps']) == 1 and not c['hot']}
    for kc in ((1, 2), (1, 21), (1, 19), (2, 19), (5, 64), (16, 2)):
        for t in (1.0, 0.5, 2.0):
            assert kc + (t,) in grid
    sizes = {n: [l.shape[2:] for l in R.case_inputs(n)['logits']] for n in ('k1_c21_T1', 'k1_c19_T1', 'k1_c2_T1')}
    assert sizes['k1_c21_T1'] == [R.OUT[1:]] and sizes['k1_c19_T1'] != [R.OUT[1:]] and sizes['k1_c2_T1'] != [R.OUT[1:]]
    assert any(len(c['temps']) == 8 for c in cs.values())
    assert {c['dtype'] for c in cs.values()} == {np.uint8, np.int64} and {c['align'] for c in cs.values()} == {True, False}
    assert {(c['k'] == 1, c['align']) for c in cs.values()} == {(True, True), (True, False), (False, True), (False, False)}
    worst = R.case_inputs('lds_worst_k16_c64_nb48')
    assert (worst['k'], worst['c'], len(worst['edges']) + 1) == (16, 64, 48)
    assert len(R.case_inputs('nb1_k2_c19')['edges']) == 0 and R.case_inputs('one_pixel_k1')['shape'] == (1, 1, 1)
    assert R.OUT[0] * R.OUT[1] * R.OUT[2] % 256 != 0 and R.OUT[0] * R.OUT[1] * R.OUT[2] > 256
    assert {cs[n]['c'] for n in R.HOT} == {c['c'] for c in cs.values()}                    # one hot case per class count


@pytest.mark.parametrize('name', R.HOT)
def test_hot_cases_occupy_eight_bins_and_the_one_above_the_highest_threshold(name):
    inp, ref = R.case(name)
    per_bin = ref['hist'][:, :, 0].sum(axis=0)
    assert (per_bin > 0).sum() >= 8 and per_bin[-1] > 0
    assert inp['edges'][-1] == np.float32(0.99)


# ------------------------------------------------------------------------------------------------------------------ the evaluator
def test_edge_union():
    from cutmix_semisup_seg_amd import evaluation as E
    edges, eq_bin, thr_bin = E.calibration_edges(15, E.CALIB_DEFAULT_THRESHOLDS)
    assert np.array_equal(edges, R.make_edges(15, R.DEFAULT_THRESHOLDS)) and edges.dtype == np.float32 and len(edges) == 19
    assert np.all(np.diff(edges) > 0) and eq_bin.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11, 12, 13, 13, 14, 14, 14, 14]
    for t, b in zip(E.CALIB_DEFAULT_THRESHOLDS, thr_bin):
        assert edges[b - 1] == np.float32(t)                           # the sub-bin whose lower edge is the threshold
    # a threshold that IS an equal-width edge is merged with it
    edges, eq_bin, thr_bin = E.calibration_edges(4, (0.5, 0.75))
    assert edges.tolist() == [0.25, 0.5, 0.75] and eq_bin.tolist() == [0, 1, 2, 3] and thr_bin.tolist() == [2, 3]
    edges, eq_bin, thr_bin = E.calibration_edges(1, ())
    assert len(edges) == 0 and eq_bin.tolist() == [0] and len(thr_bin) == 0
    assert len(E.calibration_edges(48, ())[0]) == 47 and len(E.calibration_edges(43, E.CALIB_DEFAULT_THRESHOLDS)[0]) == 47
    for bins, thr in ((0, ()), (49, ()), (2.5, ()), (True, ()), (45, E.CALIB_DEFAULT_THRESHOLDS), (15, (0.0,)), (15, (1.0,)),
                      (15, (float('nan'),)), (15, (0.5, 0.5)), (15, (1.0 - 1e-12,))):
        with pytest.raises(ValueError):
            E.calibration_edges(bins, thr)
    assert E.parse_calibration_thresholds(' 0.5, 0.97 ') == (0.5, 0.97) and E.parse_calibration_thresholds('') == ()
    assert E.parse_calibration_temperatures('0.5,2') == (0.5, 2.0) and E.parse_calibration_temperatures('') == ()
    for bad in ('0.5,,0.9', 'high', '0.5;0.9', '1.5'):
        with pytest.raises(ValueError):
            E.parse_calibration_thresholds(bad)
    for bad in ('0', '-1', 'nan', 'inf', '1e39', 'warm', '1,,2'):
        with pytest.raises(ValueError):
            E.parse_calibration_temperatures(bad)


def _pixels(seed, n, c):
    """random (pred, label, conf) with confidences on a grid of fp32 numbers, some exactly on edges"""
    rng = np.random.RandomState(seed)
    conf = rng.randint(1, 2 ** 12 + 1, size=n).astype(np.float64) / 2 ** 12
    conf[:5] = [float(np.float32(t)) for t in R.DEFAULT_THRESHOLDS]
    pred = rng.randint(0, c - 1, size=n)                               # class c - 1 is never predicted
    label = np.where(rng.uniform(size=n) < conf, pred, rng.randint(0, c, size=n))
    label[label == 1] = 0                                              # ... and class 1 never the truth
    return pred, label, conf


def _tables(pred, label, conf, edges, c, nll, brier):
    hist = np.zeros((c, len(edges) + 1, 3), dtype=np.int64)
    b = R.bin_of(conf, edges)
    np.add.at(hist[:, :, 0], (pred, b), 1)
    np.add.at(hist[:, :, 1], (pred, b), (pred == label).astype(np.int64))
    np.add.at(hist[:, :, 2], (pred, b), np.rint(conf * 2 ** 24).astype(np.int64))
    cm = np.zeros((c, c), dtype=np.int64)
    np.add.at(cm, (label, pred), 1)
    scores = np.array([len(pred), int(np.rint(brier * 2 ** 24).sum())] + [int(np.rint(v * 2 ** 20).sum()) for v in nll], dtype=np.int64)
    return hist, scores, cm


def test_derived_scores_from_injected_tables(monkeypatch):
    from cutmix_semisup_seg_amd import evaluation as E
    _no_gpu(monkeypatch)
    c, n, n_bins = 5, 4000, 15
    pred, label, conf = _pixels(3, n, c)
    rng = np.random.RandomState(4)
    nll, brier = rng.uniform(0, 5, size=(3, n)), rng.uniform(0, 2, size=n)
    ev = E.EvaluatorCalibration(c, n_bins, R.DEFAULT_THRESHOLDS, 1.0, (0.5, 2.0))
    assert ev.scored_pixels() == 0 and math.isnan(ev.ece()) and math.isnan(ev.mce()) and np.isnan(ev.nll()).all()      # nothing yet
    ev.load_tables(*_tables(pred, label, conf, ev.edges, c, nll, brier))
    assert ev.scored_pixels() == n
    # ECE by merging sub-bins equals ECE computed directly on the equal-width bins
    eq = R.bin_of(conf, (np.arange(1, n_bins) / n_bins).astype(np.float32))
    hit = (pred == label).astype(np.float64)
    conf_q = np.rint(conf * 2 ** 24) / 2 ** 24

    def ece_direct(mask):
        tot, worst = 0.0, 0.0
        for b in range(n_bins):
            m = mask & (eq == b)
            if m.any():
                gap = abs(hit[m].mean() - conf_q[m].mean())
                tot, worst = tot + m.sum() * gap, max(worst, gap)
        return tot / mask.sum(), worst
    want, worst = ece_direct(np.ones(n, dtype=bool))
    assert abs(ev.ece() - want) < 1e-12 and abs(ev.mce() - worst) < 1e-12
    per = ev.ece_per_class()
    for k in range(c - 1):
        assert abs(per[k] - ece_direct(pred == k)[0]) < 1e-12
    assert math.isnan(per[c - 1])                                      # never predicted
    rows = ev.reliability()
    assert len(rows) == n_bins and sum(r['n'] for r in rows) == n and rows[3]['lo'] == 3 / 15 and rows[3]['hi'] == 4 / 15
    for b, r in enumerate(rows):
        m = eq == b
        assert r['n'] == m.sum() and abs(r['acc'] - hit[m].mean()) < 1e-12 and abs(r['conf'] - conf_q[m].mean()) < 1e-12
    assert np.allclose(ev.nll(), np.rint(nll * 2 ** 20).sum(axis=1) / 2 ** 20 / n, rtol=0, atol=1e-12)
    assert abs(ev.brier() - np.rint(brier * 2 ** 24).sum() / 2 ** 24 / n) < 1e-12
    # suffix sums equal a direct threshold count, the trainers' `conf >= conf_thresh` in fp32
    for t, rep in zip(R.DEFAULT_THRESHOLDS, ev.threshold_report()):
        ok = conf.astype(np.float32) >= np.float32(t)
        assert rep['threshold'] == t and abs(rep['pass_rate'] - ok.mean()) < 1e-15 and abs(rep['acc'] - hit[ok].mean()) < 1e-15
        for k in range(c):
            m, truth = ok & (pred == k), label == k
            assert (math.isnan(rep['acc_per_class'][k]) and not m.any()) or abs(rep['acc_per_class'][k] - hit[m].mean()) < 1e-15
            want = (ok & truth & (pred == k)).sum() / truth.sum() if truth.any() else float('nan')
            assert (math.isnan(want) and math.isnan(rep['recall_per_class'][k])) or abs(rep['recall_per_class'][k] - want) < 1e-15
        assert math.isnan(rep['recall_per_class'][1]) and math.isnan(rep['acc_per_class'][c - 1])
    # as_dict is JSON and round-trips
    import json
    d = json.loads(json.dumps(ev.as_dict()))
    again = E.EvaluatorCalibration(c, d['n_bins'], d['thresholds'], d['temperatures'][0], d['temperatures'][1:])
    again.load_tables(d['hist'], d['scores'], d['cm'])
    assert again.as_dict() == d and d['ece_per_class'][c - 1] is None and d['scored_pixels'] == n
    with pytest.raises(ValueError):
        ev.load_tables(d['hist'], d['scores'][:-1], d['cm'])
    for kw in (dict(n_classes=0), dict(n_classes=65), dict(n_classes=3, temperature=0.0), dict(n_classes=3, nll_temperatures=(1.0,) * 8),
               dict(n_classes=3, n_bins=45), dict(n_classes=3, thresholds=(1.5,))):
        with pytest.raises(ValueError):
            E.EvaluatorCalibration(**kw)


def test_report_lines(monkeypatch):
    from cutmix_semisup_seg_amd import evaluation as E
    from cutmix_semisup_seg_amd.eval_seg import calibration_lines
    _no_gpu(monkeypatch)
    c, n = 3, 500
    pred, label, conf = _pixels(5, n, c)
    ev = E.EvaluatorCalibration(c, 4, (0.5, 0.97), 2.0, (1.0,))
    ev.load_tables(*_tables(pred, label, conf, ev.edges, c, np.stack([np.full(n, 0.75), np.full(n, 0.5)]), np.full(n, 0.25)))
    lines = calibration_lines('VAL', ev, ['0.5', '0.97'], n_views=4)
    assert lines[0] == '-- calibration at T=2: the vote over the 4 views is taken at T'
    assert re.match(r'VAL ECE=\d+\.\d{3}%$', lines[1]) and re.match(r'-- ECE \d+\.\d{3}%, \d+\.\d{3}%, -$', lines[2])
    assert re.match(r'-- MCE=\d+\.\d{3}% NLL=0\.7500 Brier=0\.2500$', lines[3])
    assert [l[:14] for l in lines[4:8]] == ['-- bin [0.000,', '-- bin [0.250,', '-- bin [0.500,', '-- bin [0.750,']
    assert re.match(r'-- bin \[0\.750,1\.000\) n=\d+ acc=\d+\.\d{3}% conf=\d+\.\d{3}%$', lines[7])
    assert re.match(r'VAL pseudo@0\.5 pass=\d+\.\d{3}% acc=\d+\.\d{3}%$', lines[8])
    assert lines[9].startswith('-- pseudo@0.5 acc ') and lines[9].endswith(', -') and lines[10].startswith('-- pseudo@0.5 recall ')
    assert lines[11].startswith('VAL pseudo@0.97 ') and lines[14] == '-- NLL@T 2=0.7500, 1=0.5000; lowest at T=1' and len(lines) == 15
    assert calibration_lines('TEST', E.EvaluatorCalibration(c, 1, ()), [])[:2] == ['TEST ECE=-', '-- ECE -, -, -']


# ------------------------------------------------------------------------------------------------------------------ eval_seg
BAD_OPTIONS = [(['--calib_bins', '0'], '--calib_bins'), (['--calib_bins', '49'], '--calib_bins'), (['--calib_bins', 'many'], '--calib_bins'),
               (['--calib_bins', '2.5'], '--calib_bins'), (['--calib_bins', '45'], '--calib_bins'),
               (['--calib_thresh', '0.5,,0.9'], '--calib_thresh'), (['--calib_thresh', '1'], '--calib_thresh'),
               (['--calib_thresh', '0'], '--calib_thresh'), (['--calib_thresh', 'high'], '--calib_thresh'),
               (['--calib_thresh', '0.9,0.9'], '--calib_thresh'), (['--calib_thresh', 'nan'], '--calib_thresh'),
               (['--calib_bins', '40', '--calib_thresh', '0.11,0.12,0.13,0.14,0.16,0.17,0.18,0.19,0.21'], '--calib_bins / --calib_thresh'),
               (['--calib_temperature', '0'], '--calib_temperature'), (['--calib_temperature', '-1'], '--calib_temperature'),
               (['--calib_temperature', 'inf'], '--calib_temperature'), (['--calib_temperature', '1,2'], '--calib_temperature'),
               (['--calib_temperature', 'warm'], '--calib_temperature'), (['--calib_nll_temps', '0.5,0'], '--calib_nll_temps'),
               (['--calib_nll_temps', '1,2,3,4,5,6,7,8'], '--calib_nll_temps'), (['--calib_nll_temps', 'nan'], '--calib_nll_temps'),
               (['--crf'], '--crf')]


def test_eval_seg_refusals_come_before_the_model_and_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import eval_seg
    from cutmix_semisup_seg_amd import checkpoint, eval_seg as es
    _no_gpu(monkeypatch)
    root = _pascal_tree.write_tree(str(tmp_path / 'VOC2012'), {'a': (20, 24), 'b': (22, 20), 'c': (20, 20)}, ['a', 'b'], ['c'])
    _pascal_tree.write_config(str(tmp_path), root)
    monkeypatch.chdir(tmp_path)
    opened = []
    monkeypatch.setattr(checkpoint, 'load_model', lambda path: opened.append(path) or (_ for _ in ()).throw(IOError('not a model')))
    ok = ['no_such_model.pth', '--dataset', 'pascal']

    def refused(args, what):
        res = CliRunner().invoke(eval_seg.experiment, ok + args)
        assert res.exit_code != 0, res.output
        assert not isinstance(res.exception, AssertionError), res.exception
        assert what in res.output, (args, res.output)
        assert not opened                                                             # said before the model file is opened
    for args, what in BAD_OPTIONS:
        refused(['--calibration'] + args, what)
    for opt, val in (('calib_bins', '15'), ('calib_thresh', '0.9'), ('calib_temperature', '2'), ('calib_nll_temps', '2'),
                     ('calib_out', 'x.json')):
        refused(['--' + opt, val], '--{} is given without --calibration'.format(opt))
    # prepare() itself refuses the same, as EvalNotRun naming the option, before it opens the model
    common = ('no_such_model.pth', 'pascal', 'val', '1', False, -1, 131, None, False)
    for over, what in ((dict(calib_bins='0'), '--calib_bins'), (dict(calib_thresh='2'), '--calib_thresh'),
                       (dict(calib_temperature='0'), '--calib_temperature'), (dict(calib_nll_temps='x'), '--calib_nll_temps'),
                       (dict(calib_bins='48', calib_thresh='0.97'), '--calib_bins / --calib_thresh')):
        with pytest.raises(es.EvalNotRun, match=what):
            es.prepare(*common, calibration=(True, over))
    with pytest.raises(es.EvalNotRun, match='--calib_out is given without --calibration'):
        es.prepare(*common, calibration=(False, dict(calib_out='x.json')))
    with pytest.raises(es.EvalNotRun, match='--crf'):
        es.prepare(*common, calibration=(True, {}), crf=True)
    with pytest.raises(es.EvalNotRun, match='--crf'):
        es.prepare(*common, calibration=es.calibration_spec(True), crf=object())
    assert not opened
    # with everything in order the program gets as far as the model file
    res = CliRunner().invoke(eval_seg.experiment, ok + ['--calibration', '--calib_bins', '10', '--calib_thresh', '0.9,0.97',
                                                        '--calib_temperature', '1.5', '--calib_nll_temps', '1,2'])
    assert res.exit_code != 0 and opened and 'does not load' in res.output


def test_command_line_surface():
    from click.testing import CliRunner
    import eval_seg
    from cutmix_semisup_seg_amd import eval_seg as es
    names = {o.name for o in eval_seg.experiment.params}
    assert {'calibration', 'calib_bins', 'calib_thresh', 'calib_temperature', 'calib_nll_temps', 'calib_out'} <= names
    assert set(es.CALIB_OPTIONS) == {n for n in names if n.startswith('calib_')}
    out = CliRunner().invoke(eval_seg.experiment, ['--help']).output
    for opt in ('--calibration', '--calib_bins', '--calib_thresh', '--calib_temperature', '--calib_nll_temps', '--calib_out'):
        assert opt in out
    spec = es.calibration_spec(True)
    assert spec == dict(n_bins=15, thresholds=(0.5, 0.9, 0.95, 0.97, 0.99), labels=['0.5', '0.9', '0.95', '0.97', '0.99'],
                        temperature=1.0, nll_temperatures=(), out=None)
    spec = es.calibration_spec(True, calib_bins='10', calib_thresh='0.9, 0.970', calib_temperature='1.5', calib_nll_temps='1,2',
                               calib_out='r.json')
    assert spec == dict(n_bins=10, thresholds=(0.9, 0.97), labels=['0.9', '0.970'], temperature=1.5, nll_temperatures=(1.0, 2.0),
                        out='r.json')
    assert es.calibration_spec(True, calib_thresh='')['thresholds'] == () and es.calibration_spec(False) is None
    for doc in (es.__doc__, open(os.path.join(REPO, 'README.md')).read()):
        for opt in ('--calibration', '--calib_bins', '--calib_thresh', '--calib_temperature', '--calib_nll_temps', '--calib_out'):
            assert opt in doc


def test_the_trainers_never_pass_calibration():
    import inspect
    from cutmix_semisup_seg_amd import trainer_common as tc, tta
    assert inspect.signature(tc.DatasetRun.staged_eval).parameters['calibration'].default is None
    assert inspect.signature(tta.TTA.predict).parameters['calibration'].default is None
    pkg = os.path.join(REPO, 'cutmix-semisup-seg_amd')
    for f in os.listdir(pkg):
        if f.startswith('train_seg_'):
            assert 'calibration' not in open(os.path.join(pkg, f)).read(), f
