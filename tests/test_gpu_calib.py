"""
GPU: the calibration launch (csrc/calib.hip through ops.calibration_accumulate, evaluation.EvaluatorCalibration, tta.TTA.predict and
DatasetRun.staged_eval with `calibration=`, eval_seg --calibration) against the fp64 restatement of tests/_calib_refs.py under its
acceptance rule, against the vote kernel it takes the place of, and end to end on the fabricated Pascal VOC tree. Every output sits
between guard bytes that must survive the launch.
"""
import json

import numpy as np
import pytest
import torch

import _calib_refs as R
import _pascal_tree

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256
EINVAL = -1                                          # CMS_EINVAL


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded(object):
    """An output tensor of `shape`, filled with `fill`, inside a buffer with GUARD bytes of 0xA5 on both sides"""

    def __init__(self, shape, dtype, fill=0):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + nbytes] = fill
        self.t = self.buf[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[-GUARD:] == 0xA5).all())


def launch(inp, tables=None, want_pred=True, **over):
    """ops.calibration_accumulate on a case's inputs into guarded tables (new and zeroed unless given) -> dict on the host"""
    from cutmix_semisup_seg_amd import ops
    n, H, W = inp['shape']
    c, nb, nt = inp['c'], len(inp['edges']) + 1, len(inp['temps'])
    if tables is None:
        tables = (Guarded((c, nb, 3), torch.int64), Guarded((2 + nt,), torch.int64), Guarded((c, c), torch.int64))
    gh, gs, gc = tables
    gp = Guarded((n, H, W), torch.uint8, 0xFF)
    cm, pred = ops.calibration_accumulate([cu(l) for l in inp['logits']], inp['flips'], c, (H, W), cu(inp['labels']), inp['edges'],
                                          inp['temps'], gh.t, gs.t, align_corners=inp['align'], cm=gc.t,
                                          pred=gp.t if want_pred else None, **over)
    torch.cuda.synchronize()
    assert gh.intact() and gs.intact() and gc.intact() and gp.intact() and cm is gc.t
    return dict(hist=gh.t.cpu().numpy(), scores=gs.t.cpu().numpy(), cm=gc.t.cpu().numpy(),
                pred=gp.t.cpu().numpy() if want_pred else None, tables=tables)


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_kernel_vs_restatement(name):
    inp, ref = R.case(name)
    n_scored = int(ref['scores'][0])
    assert ref['ambiguous'] <= R.MAX_AMBIGUOUS * max(n_scored, 1)                        # a condition on the case
    got = launch(inp)
    mean = lambda a, b, scale: abs(int(a) - int(b)) / scale / max(n_scored, 1)
    print(name, 'mean error on the GPU: conf {:.3g} squared error {:.3g} nll {}; ambiguous {} of {}'.format(
        mean(got['hist'][:, :, 2].sum(), ref['conf_fx_all'], R.CONF_SCALE), mean(got['scores'][1], ref['scores'][1], R.BRIER_SCALE),
        ['{:.3g}'.format(mean(a, b, R.NLL_SCALE)) for a, b in zip(got['scores'][2:], ref['scores'][2:])], ref['ambiguous'], n_scored))
    R.accept(got, ref)
    if R.CASES[name]['ignore_all']:
        assert not got['hist'].any() and not got['scores'].any() and not got['cm'].any()


@pytest.mark.parametrize('name', R.HOT)
def test_the_hot_cases_reach_the_top_bins(name):
    inp, _ = R.case(name)
    got = launch(inp)
    per_bin = got['hist'][:, :, 0].sum(axis=0)
    assert (per_bin > 0).sum() >= 8 and per_bin[-1] > 0


@pytest.mark.parametrize('name', ['k1_c2_T1', 'k1_c21_T1', 'k1_c19_T1', 'k1_c21_ident_align_i64', 'k2_c19_T1', 'k5_c64_T1',
                                  'k16_c2_T1', 'lds_worst_k16_c64_nb48', 'k1_c19_T2', 'k1_c21_T0.5', 'hot_k2_c19'])
def test_prediction_and_matrix_are_the_votes_bit_for_bit(name):
    """T == 1, and one view at any temperature"""
    from cutmix_semisup_seg_amd import ops
    inp, _ = R.case(name)
    assert inp['k'] == 1 or float(inp['temps'][0]) == 1.0
    n, H, W = inp['shape']
    cm, pred = ops.tta_vote([cu(l) for l in inp['logits']], inp['flips'], inp['c'], (H, W), labels=cu(inp['labels']),
                            align_corners=inp['align'], want_pred=True)
    got = launch(inp)
    assert np.array_equal(got['pred'], pred.cpu().numpy()) and np.array_equal(got['cm'], cm.cpu().numpy())


@pytest.mark.parametrize('name,other', [('k2_c19_nt8', 'hot_k2_c19'), ('k1_c19_nt8_i64', 'k1_c19_T1'), ('hot_k5_c64', 'k5_c64_T1')])
def test_two_launches_add_and_a_repeated_call_gives_the_same_bits(name, other):
    inp, _ = R.case(name)
    a, b = launch(inp), launch(inp)
    for key in ('hist', 'scores', 'cm', 'pred'):
        assert np.array_equal(a[key], b[key]), key
    twice = launch(inp, tables=a['tables'])
    for key in ('hist', 'scores', 'cm'):
        assert np.array_equal(twice[key], 2 * b[key]), key
    # another batch into the same tables: the entrywise sum of the two launched alone
    inp2 = dict(R.case(other)[0], edges=inp['edges'], temps=inp['temps'])
    alone = launch(inp2)
    both = launch(inp2, tables=b['tables'])
    for key in ('hist', 'scores', 'cm'):
        assert np.array_equal(both[key], b[key] + alone[key]) and alone[key].any(), key


def test_without_pred_and_on_a_side_stream():
    inp, ref = R.case('k5_c64_i64')
    want = launch(inp)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = launch(inp, want_pred=False)
    side.synchronize()
    assert got['pred'] is None
    for key in ('hist', 'scores', 'cm'):
        assert np.array_equal(got[key], want[key]), key
    R.accept(got, ref)


def test_the_library_refuses_without_launching():
    import ctypes as C
    from cutmix_semisup_seg_amd import _lib
    inp, _ = R.case('k2_c19_T1')
    n, H, W = inp['shape']
    c, nb = inp['c'], len(inp['edges']) + 1
    views = [cu(l) for l in inp['logits']]
    labels = cu(inp['labels'])
    gh, gs, gc = Guarded((c, nb, 3), torch.int64), Guarded((3,), torch.int64), Guarded((c, c), torch.int64)
    edges, temps = np.ascontiguousarray(inp['edges']), np.ones(1, dtype=np.float32)

    def desc(**over):
        d = _lib.CalibDesc()
        for i, t in enumerate(views):
            d.logits[i], d.h[i], d.w[i], d.flip[i] = t.data_ptr(), int(t.shape[2]), int(t.shape[3]), int(inp['flips'][i])
        d.n, d.c, d.H, d.W, d.k, d.align_corners = n, c, H, W, len(views), int(inp['align'])
        d.labels, d.label_dtype, d.ignore_index = labels.data_ptr(), _lib.LABEL_U8, 255
        d.cm, d.pred_out = gc.t.data_ptr(), None
        d.nb, d.edges, d.nt, d.temps = nb, edges.ctypes.data, 1, temps.ctypes.data
        d.hist, d.scores = gh.t.data_ptr(), gs.t.data_ptr()
        for key, val in over.items():
            setattr(d, key, val)
        return d
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad_edges = [np.ascontiguousarray(e, dtype=np.float32) for e in (edges[::-1], np.r_[0.0, edges[1:]], np.r_[edges[:-1], 1.0],
                                                                     np.r_[edges[:3], edges[2:-1]])]
    bad_temps = [np.asarray([v], dtype=np.float32) for v in (0.0, -1.0, np.nan, np.inf)]
    refused = [dict(nb=0), dict(nb=49), dict(nt=0), dict(nt=9), dict(hist=None), dict(scores=None), dict(labels=None),
               dict(labels=None, cm=None, pred_out=gc.t.data_ptr()), dict(edges=None), dict(temps=None), dict(k=0), dict(k=17),
               dict(c=0), dict(c=65), dict(n=0), dict(H=0), dict(W=-1), dict(label_dtype=9), dict(cm=None)]
    refused += [dict(edges=e.ctypes.data) for e in bad_edges] + [dict(temps=t.ctypes.data) for t in bad_temps]
    for over in refused:
        assert _lib.fn['cms_calib_accumulate'](C.byref(desc(**over)), stream) == EINVAL, over
    assert _lib.fn['cms_calib_accumulate'](None, stream) == EINVAL
    torch.cuda.synchronize()
    assert not gh.t.any() and not gs.t.any() and not gc.t.any() and gh.intact() and gs.intact() and gc.intact()
    assert _lib.fn['cms_calib_accumulate'](C.byref(desc()), stream) == 0
    torch.cuda.synchronize()
    assert int(gs.t[0]) == int(gh.t[:, :, 0].sum()) > 0


def test_ops_refuses_bad_arguments():
    from cutmix_semisup_seg_amd import ops
    inp, _ = R.case('k2_c19_T1')
    n, H, W = inp['shape']
    c, nb = inp['c'], len(inp['edges']) + 1
    views, labels = [cu(l) for l in inp['logits']], cu(inp['labels'])
    hist, scores = torch.zeros((c, nb, 3), dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)

    def call(**over):
        kw = dict(logits_list=views, flips=inp['flips'], num_classes=c, out_size=(H, W), labels=labels, edges=inp['edges'],
                  temps=[1.0], hist=hist, scores=scores)
        kw.update(over)
        return ops.calibration_accumulate(**kw)
    for over, err in ((dict(edges=inp['edges'][::-1]), ValueError), (dict(edges=np.arange(1, 49) / 49.0), ValueError),
                      (dict(temps=[]), ValueError), (dict(temps=[1.0] * 9), ValueError), (dict(temps=[0.0]), ValueError),
                      (dict(labels=None), TypeError), (dict(hist=hist[:, :, :2]), TypeError), (dict(scores=scores[:2]), TypeError),
                      (dict(hist=hist.cpu()), RuntimeError), (dict(flips=[False]), ValueError)):
        with pytest.raises(err):
            call(**over)
    assert not hist.any() and not scores.any()


# ------------------------------------------------------------------------------------------------------------------ the evaluator
def test_evaluator_accumulates_batches_and_feeds_the_iou_evaluator():
    from cutmix_semisup_seg_amd import evaluation, ops
    inp, ref = R.case('hot_k2_c19')
    n, H, W = inp['shape']
    cal = evaluation.EvaluatorCalibration(19)
    assert np.array_equal(cal.edges, inp['edges'])
    views, labels = [cu(l) for l in inp['logits']], cu(inp['labels'])
    for _ in range(2):
        batch_cm, pred = cal.sample_views(views, inp['flips'], labels, (H, W), align_corners=inp['align'], want_pred=True)
    hist, scores, cm = cal.tables()
    one = launch(inp)
    assert np.array_equal(hist, 2 * one['hist']) and np.array_equal(scores, 2 * one['scores']) and np.array_equal(cm, 2 * one['cm'])
    assert np.array_equal(batch_cm.cpu().numpy(), one['cm']) and np.array_equal(pred.cpu().numpy(), one['pred'])
    assert cal.scored_pixels() == 2 * int(ref['scores'][0]) == int(cm.sum())
    # the derived scores against the fp64 per-pixel values of the restatement
    v = ref['valid']
    assert abs(cal.nll()[0] - ref['nll'][0][v].mean()) <= R.B_NLL + 1 / R.NLL_SCALE
    assert abs(cal.brier() - ref['brier'][v].mean()) <= R.B_BRIER + 1 / R.BRIER_SCALE
    assert 0.0 <= cal.ece() <= cal.mce() <= 1.0
    rep = cal.threshold_report()
    assert [r['threshold'] for r in rep] == list(R.DEFAULT_THRESHOLDS)
    rates = [r['pass_rate'] for r in rep]
    assert rates == sorted(rates, reverse=True) and rates[-1] > 0


# ------------------------------------------------------------------------------------------------------------------ end to end
SIZES = {'img_a': (40, 50), 'img_b': (44, 38), 'img_c': (36, 52), 'img_d': (41, 47), 'img_e': (40, 40)}
TRAIN, VAL = ['img_e'], ['img_a', 'img_b', 'img_c', 'img_d']


@pytest.fixture(scope='module')
def pascal(tmp_path_factory):
    """-> (working directory with the tree and its configuration, model.pth of a small DeepLab v2)"""
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    from oracle import deeplab2 as odl
    cwd = tmp_path_factory.mktemp('calib_pascal')
    root = _pascal_tree.write_tree(str(cwd / 'VOC2012'), SIZES, TRAIN, VAL)
    _pascal_tree.write_config(str(cwd), root)
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 21, np.zeros(3), np.ones(3))
    net.load_state_dict(odl.closed_form_state(21, [1, 1, 1, 1]))      # weights under which the classes are not tied
    model_path = str(cwd / 'model.pth')
    checkpoint.save_model(net, model_path)
    return cwd, root, model_path


@pytest.mark.parametrize('views', [[], ['--scales', '0.75,1', '--flip']], ids=['one_view', 'four_views'])
def test_eval_seg_with_calibration_end_to_end(pascal, monkeypatch, tmp_path, views):
    from click.testing import CliRunner
    from PIL import Image
    import eval_seg
    cwd, root, model_path = pascal
    monkeypatch.chdir(cwd)
    base = [model_path, '--dataset', 'pascal', '--batch_size', '3', '--compute_dtype', 'fp32'] + views
    out = str(tmp_path / 'calib.json')
    res = CliRunner().invoke(eval_seg.experiment, base + ['--calibration', '--calib_nll_temps', '0.5,2', '--calib_out', out,
                                                          '--save_preds', str(tmp_path / 'cal')], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    plain = CliRunner().invoke(eval_seg.experiment, base + ['--save_preds', str(tmp_path / 'plain')], catch_exceptions=False)
    assert plain.exit_code == 0, plain.output
    got, want = res.output.splitlines(), plain.output.splitlines()
    assert got[:len(want)] == want                                    # every existing line, unchanged and first
    new = got[len(want):]
    print('\n'.join(new))
    assert new[0].startswith('VAL ECE=') and new[1].startswith('-- ECE ') and new[2].startswith('-- MCE=')
    assert [l.split()[1] for l in new if l.startswith('VAL pseudo@')] == ['pseudo@' + t for t in ('0.5', '0.9', '0.95', '0.97', '0.99')]
    assert sum(l.startswith('-- bin [') for l in new) == 15 and new[-1].startswith('-- NLL@T 1=') and '; lowest at T=' in new[-1]
    assert len(new) == 3 + 15 + 3 * 5 + 1
    for name in VAL:                                                  # the saved predictions are the plain run's
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'cal' / (name + '.png'))),
                              np.asarray(Image.open(tmp_path / 'plain' / (name + '.png'))))
    rep = json.load(open(out))
    hist, cm = np.asarray(rep['hist']), np.asarray(rep['cm'])
    labelled = sum(int((np.asarray(Image.open('{}/SegmentationClass/{}.png'.format(root, n))) < 21).sum()) for n in VAL)
    assert hist[:, :, 0].sum() == cm.sum() == rep['scores'][0] == rep['scored_pixels'] == labelled
    assert np.array_equal(hist[:, :, 0].sum(axis=1), cm.sum(axis=0))              # keyed by predicted class
    # the file round-trips into an evaluator that derives the same scores without a GPU
    from cutmix_semisup_seg_amd import evaluation
    again = evaluation.EvaluatorCalibration(21, rep['n_bins'], rep['thresholds'], rep['temperatures'][0], rep['temperatures'][1:])
    again.load_tables(rep['hist'], rep['scores'], rep['cm'])
    assert again.as_dict() == rep
    assert new[0] == 'VAL ECE={:.3%}'.format(again.ece())


def test_evaluate_returns_the_same_iou_with_and_without_calibration(pascal, monkeypatch, capsys):
    import eval_seg
    cwd, _, model_path = pascal
    monkeypatch.chdir(cwd)
    kw = dict(batch_size=2, compute_dtype='fp32', scales='0.75,1')
    a = eval_seg.evaluate(model_path, 'pascal', **kw)
    b = eval_seg.evaluate(model_path, 'pascal', calibration=True, **kw)
    assert np.array_equal(a, b)
    from cutmix_semisup_seg_amd.eval_seg import calibration_spec
    c = eval_seg.evaluate(model_path, 'pascal', calibration=calibration_spec(True, calib_temperature='2'), **kw)
    assert 'the vote over the 2 views is taken at T' in capsys.readouterr().out and c.shape == a.shape
