"""
GPU: test-time augmentation (csrc/tta.hip through ops.tta_resize / ops.tta_vote, tta.TTA, EvaluatorIoU.sample_logits_tta,
DatasetRun.staged_eval(tta=...), eval_seg) against the fp64 restatement of tests/_tta_refs.py, against ops.argmax_confusion (one view:
bit for bit), and end to end on a fabricated Pascal VOC tree with a small DeepLab v2. Every output is poisoned before the launch and
sits between guard bytes that must survive it.
"""
import os

import numpy as np
import pytest
import torch

import _pascal_tree
import _tta_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded(object):
    """A poisoned output tensor of `shape` inside a buffer with GUARD bytes of 0xA5 on both sides"""

    def __init__(self, shape, dtype, poison=0xFF):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + nbytes] = poison
        self.t = self.buf[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[-GUARD:] == 0xA5).all())


def vote(logits, flips, c, size, labels=None, align=True, cm=None, want_pred=True, ignore_index=255):
    """ops.tta_vote with a poisoned, guarded prediction buffer (and a fresh zero cm) -> (cm | None, pred | None) on the host"""
    from cutmix_semisup_seg_amd import ops
    n = int(logits[0].shape[0])
    g = Guarded((n, size[0], size[1]), torch.uint8) if want_pred else None
    cm_out, pred = ops.tta_vote(logits, flips, c, size, labels=labels, ignore_index=ignore_index, align_corners=align, cm=cm,
                                pred=g.t if g is not None else None)
    torch.cuda.synchronize()
    assert g is None or (g.intact() and pred is g.t)
    return (None if cm_out is None else cm_out.cpu().numpy()), (None if pred is None else pred.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ resize
def _resize(x, size, flip):
    from cutmix_semisup_seg_amd import ops
    g = Guarded(tuple(x.shape[:2]) + tuple(size), x.dtype)               # 0xFF bytes: NaN in fp32 and in bf16
    out = ops.tta_resize(x, size, flip=flip, out=g.t)
    torch.cuda.synchronize()
    assert out is g.t and g.intact()
    return out


@pytest.mark.parametrize('shape,size,flip', R.RESIZE_CASES)
def test_resize_fp32_vs_fp64(shape, size, flip):
    x = R.resize_input(shape)
    got = _resize(cu(x), size, flip).cpu().numpy()
    want = R.resize(x, size, flip)
    print(shape, size, flip, 'max |got - fp64| =', np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('shape,size,flip', R.RESIZE_CASES)
def test_resize_bf16_within_one_ulp(shape, size, flip):
    xb = cu(R.resize_input(shape)).bfloat16()
    got = _resize(xb, size, flip)
    assert got.dtype == torch.bfloat16
    want = R.resize(xb.float().cpu().numpy(), size, flip)
    got = got.float().cpu().numpy().astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -126))) - 7)       # bf16: 8 significant bits
    assert np.isfinite(got).all() and (np.abs(got - want) <= ulp).all()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_resize_flip_is_the_mirrored_resize(dtype):
    x = cu(R.resize_input((2, 3, 33, 47))).to(dtype)
    for size in ((17, 24), (50, 71), (33, 47), (1, 1)):
        assert torch.equal(_resize(x, size, True), _resize(x, size, False).flip(-1))
    assert torch.equal(_resize(x, (33, 47), False), x)                               # the identity size copies


# ------------------------------------------------------------------------------------------------------------------ one view
def _labels(shape, c, dtype, seed=0):
    lab = R.make_labels(shape, c, seed)
    return cu(lab.astype(np.int64) if dtype == torch.int64 else lab)


@pytest.mark.parametrize('c', [2, 21, 64])
@pytest.mark.parametrize('align', [True, False])
@pytest.mark.parametrize('view', [(9, 13), (37, 53)], ids=['lowres', 'identity'])
@pytest.mark.parametrize('ldt', [torch.uint8, torch.int64], ids=['u8', 'i64'])
def test_one_view_is_argmax_confusion_bit_for_bit(c, align, view, ldt):
    from cutmix_semisup_seg_amd import ops
    n, H, W = R.OUT
    lg = cu(R.make_views(1, c, n, seed=c, sizes=[view])[0][0])
    labels = _labels((n, H, W), c, ldt)
    want_cm, want_pred = ops.argmax_confusion(lg, labels, c, (H, W), align_corners=align, want_pred=True)
    cm, pred = vote([lg], [False], c, (H, W), labels=labels, align=align)
    assert np.array_equal(pred, want_pred.cpu().numpy()) and np.array_equal(cm, want_cm.cpu().numpy())
    assert cm.sum() == int((labels != 255).sum())
    # ... its NaN rule included: a NaN counts as maximal, the first one wins
    lg2 = lg.clone()
    lg2[:, c - 1, 2:5, 1:6] = float('nan')
    lg2[0, 0, 3, 3] = float('nan')
    want_cm, want_pred = ops.argmax_confusion(lg2, labels, c, (H, W), align_corners=align, want_pred=True)
    cm, pred = vote([lg2], [False], c, (H, W), labels=labels, align=align)
    assert np.array_equal(pred, want_pred.cpu().numpy()) and np.array_equal(cm, want_cm.cpu().numpy())
    # a mirrored view, flipped: the same prediction
    _, pred_f = vote([lg.flip(-1).contiguous()], [True], c, (H, W), align=align)
    _, pred_u = vote([lg], [False], c, (H, W), align=align)
    assert np.array_equal(pred_f, pred_u)


# ------------------------------------------------------------------------------------------------------------------ the vote
@pytest.mark.parametrize('k,c', sorted(R.VOTE_CASES))
def test_vote_vs_fp64(k, c):
    case = R.vote_case(k, c)
    n, H, W = R.OUT
    # a condition on the INPUTS, not a tolerance: the reference decides every pixel by more than fp32 can move the scores
    assert case['gap'].min() >= R.gap_bound(k)
    logits = [cu(l) for l in case['logits']]
    cm, pred = vote(logits, case['flips'], c, (H, W), labels=cu(case['labels']), align=case['align'])
    print('k', k, 'C', c, 'pixels that differ:', int((pred != case['pred']).sum()), 'min gap', case['gap'].min())
    assert np.array_equal(pred, case['pred'])
    assert np.array_equal(cm, case['cm'])
    # int64 labels, accumulation into a given matrix
    from cutmix_semisup_seg_amd import ops
    acc = cu(case['cm'].astype(np.int64))
    ops.tta_vote(logits, case['flips'], c, (H, W), labels=cu(case['labels'].astype(np.int64)), align_corners=case['align'], cm=acc)
    assert np.array_equal(acc.cpu().numpy(), 2 * case['cm'])


def test_determinism_and_batch_independence():
    case = R.vote_case(5, 19)
    n, H, W = R.OUT
    logits, labels = [cu(l) for l in case['logits']], cu(case['labels'])
    a = vote(logits, case['flips'], 19, (H, W), labels=labels, align=case['align'])
    b = vote(logits, case['flips'], 19, (H, W), labels=labels, align=case['align'])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    total = np.zeros_like(a[0])
    for i in range(n):
        cm, pred = vote([l[i:i + 1].contiguous() for l in logits], case['flips'], 19, (H, W), labels=labels[i:i + 1].contiguous(),
                        align=case['align'])
        assert np.array_equal(pred[0], a[1][i])
        total += cm
    assert np.array_equal(total, a[0])


def test_degenerate_inputs():
    case = R.vote_case(2, 19)
    n, H, W = R.OUT
    logits = [cu(l) for l in case['logits']]
    cm, pred = vote(logits, case['flips'], 19, (H, W), labels=torch.full((n, H, W), 255, dtype=torch.uint8, device=DEV),
                    align=case['align'])
    assert cm.shape == (19, 19) and not cm.any() and np.array_equal(pred, case['pred'])
    cm, pred = vote(logits, case['flips'], 19, (H, W), align=case['align'])                      # prediction only
    assert cm is None and np.array_equal(pred, case['pred'])
    cm, pred = vote(logits, case['flips'], 19, (H, W), labels=cu(case['labels']), align=case['align'], want_pred=False)
    assert pred is None and np.array_equal(cm, case['cm'])                                       # histogram only
    cm, _ = vote(logits, case['flips'], 19, (H, W), labels=cu(case['labels']), align=case['align'], ignore_index=None)
    assert cm.sum() == int((case['labels'] < 19).sum())                                          # 255 is out of range, not ignored
    # one output pixel
    for k in (1, 3):
        lg, flips = R.make_views(k, 4, 1, seed=9)
        want = R.vote(lg, flips, (1, 1), True)
        assert want[2].min() >= R.gap_bound(k)
        cm, pred = vote([cu(l) for l in lg], flips, 4, (1, 1), labels=torch.zeros((1, 1, 1), dtype=torch.uint8, device=DEV))
        assert pred.shape == (1, 1, 1) and np.array_equal(pred, want[1]) and cm.sum() == 1 and cm[0, want[1][0, 0, 0]] == 1


def test_sample_logits_tta_with_fill_holes():
    from cutmix_semisup_seg_amd import evaluation, ops
    case = R.vote_case(5, 2)
    n, H, W = R.OUT
    logits = [cu(l) for l in case['logits']]
    truth = cu(np.where(case['labels'] == 255, 255, case['labels'] % 2).astype(np.uint8))
    ev = evaluation.EvaluatorIoU(2, fill_holes=True)
    ev.sample_logits_tta(logits, case['flips'], truth[:, None], (H, W), ignore_value=255, align_corners=case['align'])
    filled, want_cm = ops.fill_holes(cu(case['pred']), truth=truth, ignore_index=255)
    assert np.array_equal(ev.cm, want_cm.cpu().numpy().astype(np.float64))
    assert not torch.equal(filled, cu(case['pred']))                                             # the case has holes to fill
    plain = evaluation.EvaluatorIoU(2)
    plain.sample_logits_tta(logits, case['flips'], truth, (H, W), ignore_value=255, align_corners=case['align'])
    assert np.array_equal(plain.cm, R.confusion(truth.cpu().numpy(), case['pred'], 2).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ end to end
SIZES = {'img_a': (40, 50), 'img_b': (44, 38), 'img_c': (36, 52), 'img_d': (41, 47), 'img_e': (40, 40)}
TRAIN, VAL = ['img_e'], ['img_a', 'img_b', 'img_c', 'img_d']


@pytest.fixture(scope='module')
def pascal(tmp_path_factory):
    """-> (working directory with the tree and its configuration, model.pth of a small DeepLab v2)"""
    from architectures import deeplab2
    from cutmix_semisup_seg_amd import checkpoint
    cwd = tmp_path_factory.mktemp('tta_pascal')
    root = _pascal_tree.write_tree(str(cwd / 'VOC2012'), SIZES, TRAIN, VAL)
    _pascal_tree.write_config(str(cwd), root)
    from oracle import deeplab2 as odl
    net = deeplab2.ResNetDeepLab(deeplab2.Bottleneck, [1, 1, 1, 1], 21, np.zeros(3), np.ones(3))
    net.load_state_dict(odl.closed_form_state(21, [1, 1, 1, 1]))      # weights under which the classes are not tied
    model_path = str(cwd / 'model.pth')
    checkpoint.save_model(net, model_path)
    return cwd, model_path


def _run(cwd, model_path, monkeypatch, batch_size=3):
    from cutmix_semisup_seg_amd import checkpoint, trainer_common as tc
    from cutmix_semisup_seg_amd.datapipe import datasets
    import types
    monkeypatch.chdir(cwd)
    ds = datasets.load_dataset('pascal', -1, 131, -1, -1, 12345, None)
    net = checkpoint.load_model(model_path).to(DEV)
    net.compute_dtype = torch.float32
    net.eval()
    run = tc.DatasetRun.for_evaluation(ds, ds['val_ndx_tgt'], net, torch.device(DEV), batch_size, torch.float32)
    assert len(run.pool) == len(VAL)                   # the chosen subset only
    return run, net, ds, types.SimpleNamespace(align_corners=net.upsample_align_corners)


def test_staged_eval_with_tta(pascal, monkeypatch, tmp_path):
    from cutmix_semisup_seg_amd import evaluation, ops
    from cutmix_semisup_seg_amd.datapipe import seg_data
    from cutmix_semisup_seg_amd.tta import TTA
    from PIL import Image
    run, net, ds, step = _run(*pascal, monkeypatch)

    def cm_of(tta, preds_dir=None):
        ev = evaluation.EvaluatorIoU(21)
        run.staged_eval(net, step, run.val_ndx, ev, preds_dir, **({} if tta == 'none' else dict(tta=tta)))
        return ev.cm
    plain = cm_of('none', str(tmp_path / 'plain'))
    assert plain.sum() > 0 and np.count_nonzero(plain.sum(axis=0)) > 1            # the network predicts more than one class
    assert np.array_equal(cm_of(None), plain)
    assert np.array_equal(cm_of(TTA((1,), False), str(tmp_path / 'one')), plain)   # one view: today's evaluation, bit for bit
    names = sorted(os.listdir(tmp_path / 'plain'))
    assert names == sorted(n + '.png' for n in VAL) == sorted(os.listdir(tmp_path / 'one'))
    for n in names:
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'plain' / n)), np.asarray(Image.open(tmp_path / 'one' / n)))

    tta = TTA((0.75, 1, 1.25), True)
    got = cm_of(tta, str(tmp_path / 'six'))
    flips = [f for _, f in tta.views()]
    assert flips == [False, True] * 3
    want = torch.zeros((21, 21), dtype=torch.int64, device=DEV)
    differs = 0
    with torch.no_grad():
        for batch in seg_data.eval_batches(run.val_ndx, run.batch_size):
            ev = run.augment.stage_eval(run.pool, batch, net.BLOCK_SIZE)
            inputs = tta.make_inputs(ev['image'], net.BLOCK_SIZE)
            assert inputs[2] is ev['image'] and len(inputs) == 6
            hc, wc = ev['canvas']
            assert [tuple(x.shape[2:]) for x in inputs[::2]] == [tta.view_size((hc, wc), net.BLOCK_SIZE, s) for s in (0.75, 1, 1.25)]
            assert torch.equal(inputs[3], ev['image'].flip(-1))                    # the canvas' own size, flipped: a mirror copy
            logits = [net.forward_lowres(x) for x in inputs]
            _, pred = ops.tta_vote(logits, flips, 21, ev['canvas'], labels=ev['labels'], align_corners=step.align_corners, cm=want,
                                   want_pred=True)
            _, pred1 = ops.argmax_confusion(logits[2], None, 21, ev['canvas'], align_corners=step.align_corners, want_pred=True)
            differs += int((pred != pred1).sum())
            for k, i in enumerate(batch):
                saved = np.asarray(Image.open(tmp_path / 'six' / (ds['ds_src'].sample_names[i] + '.png')))
                assert np.array_equal(saved, pred[k].cpu().numpy())
    assert np.array_equal(got, want.cpu().numpy().astype(np.float64))
    assert got.sum() == plain.sum()                                                # the same pixels counted
    print('pixels the six-view vote decides otherwise than the single view:', differs)


def test_eval_seg_end_to_end(pascal, monkeypatch, tmp_path):
    from click.testing import CliRunner
    from PIL import Image
    from cutmix_semisup_seg_amd import evaluation
    from cutmix_semisup_seg_amd.tta import TTA
    import eval_seg
    cwd, model_path = pascal
    run, net, ds, step = _run(cwd, model_path, monkeypatch, batch_size=2)

    def lines(tta, preds_dir):
        ev = evaluation.EvaluatorIoU(21)
        run.staged_eval(net, step, run.val_ndx, ev, preds_dir, tta=tta)
        iou = ev.score()
        return ['VAL mIoU={:.3%}'.format(iou.mean()), '-- {}'.format(', '.join(['{:.3%}'.format(x) for x in iou]))]

    for name, extra, tta in (('plain', [], None), ('tta', ['--scales', '0.75,1,1.25', '--flip'], TTA((0.75, 1, 1.25), True))):
        want = lines(tta, str(tmp_path / (name + '_want')))
        res = CliRunner().invoke(eval_seg.experiment, [model_path, '--dataset', 'pascal', '--batch_size', '2', '--compute_dtype', 'fp32',
                                                       '--save_preds', str(tmp_path / name)] + extra, catch_exceptions=False)
        assert res.exit_code == 0, res.output
        out = [l for l in res.output.splitlines() if l.startswith('VAL mIoU=') or l.startswith('-- ')]
        assert out == want, (out, want)
        assert sorted(os.listdir(tmp_path / name)) == sorted(n + '.png' for n in VAL)
        for n in VAL:
            assert np.array_equal(np.asarray(Image.open(tmp_path / name / (n + '.png'))),
                                  np.asarray(Image.open(tmp_path / (name + '_want') / (n + '.png'))))
    # a held-out set: the official validation list becomes the test set
    res = CliRunner().invoke(eval_seg.experiment, [model_path, '--dataset', 'pascal', '--n_val', '1', '--subset', 'test',
                                                   '--compute_dtype', 'fp32'], catch_exceptions=False)
    assert res.exit_code == 0 and 'TEST mIoU=' in res.output and 'VAL mIoU' not in res.output
