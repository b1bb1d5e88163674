"""
CPU-only: sliding-window evaluation off the GPU -- the grid arithmetic of tta.Windows against the restatement (tests/_window_refs.py),
the coverage of every pixel of every shared case, the margins the cases are drawn for, `parse_window` and what eval_seg refuses
(without torch being imported), and the argument checks of ops.window_crop / ops.window_vote.
"""
import subprocess
import sys

import numpy as np
import pytest

import _window_refs as R
from conftest import REPO

VIEWS = [R.CANVAS, R.HALF, R.SMALL, R.LARGE, (12, 53), (37, 20), (16, 24), (17, 25), (1, 1), (1024, 2048), (1792, 3584)]
GRIDS = [(R.WIN, R.STRIDE), (R.WIN, R.WIN), (R.WIN, (4, 6)), ((40, 56), (27, 38)), ((512, 1024), (342, 683)), ((513, 513), (342, 342)),
         ((1, 1), (1, 1)), ((5, 3), (2, 1))]


def test_windows_agree_with_the_restatement():
    from cutmix_semisup_seg_amd.tta import Windows
    for window, stride in GRIDS:
        w = Windows(window, stride)
        assert (w.window, w.stride) == (window, stride)
        for view in VIEWS:
            (eh, ys), (ew, xs) = R.axis_grid(view[0], window[0], stride[0]), R.axis_grid(view[1], window[1], stride[1])
            assert w.extent(view) == (eh, ew) and w.grid(view) == (len(ys), len(xs)) and w.count(view) == len(ys) * len(xs)
            assert w.origins(view) == (ys, xs)
            assert w.max_cover(view) == R.max_cover_axis(view[0], window[0], stride[0]) * R.max_cover_axis(view[1], window[1], stride[1])
            # the definition's words: the last window is flush with the edge, the first at 0, steps of the stride in between
            for origins, e, v, s in ((ys, eh, view[0], stride[0]), (xs, ew, view[1], stride[1])):
                assert origins[0] == 0 and origins[-1] == v - e and all(b - a <= s for a, b in zip(origins, origins[1:]))
                assert origins[:-1] == [j * s for j in range(len(origins) - 1)]


def test_the_issues_examples():
    from cutmix_semisup_seg_amd.tta import Windows
    w = Windows(R.WIN, R.STRIDE)
    assert w.grid(R.CANVAS) == (3, 3) and w.origins(R.CANVAS) == ([0, 11, 21], [0, 16, 29])         # overlaps 5 / 6 rows, 8 / 11 columns
    assert w.grid(R.HALF) == (2, 2) and w.origins(R.HALF) == ([0, 3], [0, 3])
    assert w.grid(R.SMALL) == (1, 1) and w.extent(R.SMALL) == R.SMALL
    big = Windows((512, 1024))
    assert big.stride == (342, 683) and big.count((1024, 2048)) == 9                                # 4500 windows over 500 images


def test_default_stride_and_refusals():
    from cutmix_semisup_seg_amd.tta import Windows
    for window in ((16, 24), (512, 1024), (513, 513), (1, 1), (2, 3), (321, 321)):
        assert Windows(window).stride == tuple(-(-2 * v // 3) for v in window)
    assert Windows(513).window == (513, 513) and Windows(16, 4).stride == (4, 4)
    Windows((16, 24), (4, 6))                                                                       # ceil(window / 4): still taken
    Windows((17, 25), (5, 7))
    for window, stride in (((16, 24), (3, 6)), ((16, 24), (4, 5)), ((17, 25), (4, 7)), ((16, 24), (17, 24)), ((16, 24), (16, 25)),
                           ((0, 24), None), ((16, -1), None), ((16, 24), (0, 6)), ((16, 24, 3), None), ('a', None)):
        with pytest.raises(ValueError):
            Windows(window, stride)
    w = Windows((16, 24))
    w.check_block((8, 8))
    w.check_block((16, 24))
    with pytest.raises(ValueError, match='16 and 32'):
        Windows((20, 24)).check_block((16, 8))
    with pytest.raises(ValueError, match='multiples are 32'):
        Windows((16, 24)).check_block((8, 32))


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_every_pixel_is_covered(name):
    spec = R.CASES[name]
    for v in R.layout(name):
        cnt = R.cover_count((v['Hv'], v['Wv']), spec['window'], spec['stride'])
        most = R.max_cover_axis(v['Hv'], spec['window'][0], spec['stride'][0]) * R.max_cover_axis(v['Wv'], spec['window'][1],
                                                                                                    spec['stride'][1])
        assert cnt.min() >= 1 and cnt.max() <= most <= 25               # at most 4 regular windows and the flush one per axis


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_case_margins(name):
    """the condition the exact comparisons stand on: the fp64 reference decides EVERY pixel by more than the gap bound"""
    cs = R.case(name)
    print(name, 'min gap', cs['gap'].min())
    assert cs['gap'].min() > R.GAP_BOUND
    assert cs['cm'].sum() == int((cs['labels'] != 255).sum()) and (cs['labels'] == 255).any()


def test_the_case_table_covers_what_it_should():
    specs = R.CASES.values()
    assert {s['c'] for s in specs} >= {2, 21, 64} and {s['align'] for s in specs} == {True, False}
    assert {len(s['views']) for s in specs} >= {1, 2, 5} and {bool(s.get('i64')) for s in specs} == {True, False}
    assert any(s['stride'] == s['window'] for s in specs) and any(s['stride'] == (4, 6) for s in specs)
    lays = [v for n in R.CASES for v in R.layout(n)]
    assert any(v['flip'] and v['gy'] * v['gx'] > 1 for v in lays) and any(v['flip'] and v['gy'] * v['gx'] == 1 for v in lays)
    assert any((v['hl'], v['wl']) == (v['eh'], v['ew']) for v in lays) and any((v['hl'], v['wl']) == (5, 7) for v in lays)
    assert any((v['gy'], v['gx']) == (2, 2) for v in lays) and any((v['gy'], v['gx']) == (1, 3) for v in lays)
    mixed = [n for n in R.CASES if len({v['gy'] * v['gx'] == 1 for v in R.layout(n)}) == 2]
    assert len(mixed) >= 3 and sum(R.case(n)['all_single'] for n in R.CASES) == 3


def test_restatement_with_one_window_per_view_is_the_vote():
    import _tta_refs as T
    cs = R.case('single_k2_c19')
    n, H, W = R.OUT
    want = T.vote(cs['logits'], cs['flips'], (H, W), cs['align'])
    assert np.array_equal(cs['pred'], want[1]) and np.array_equal(cs['score'], want[0])
    # a view of one window beside a stitched one: its share of the score is the vote's probabilities
    cs = R.case('small_first_c2_k2_a0_i64')
    alone = R.stitch(cs['logits'][1:], cs['flips'][1:], cs['view_sizes'][1:], cs['window'], cs['stride'], (H, W), cs['align'])[0]
    p = T.softmax(T.upsample(cs['logits'][0], (H, W), cs['align'], cs['flips'][0]), 1)
    assert np.abs(cs['score'] - (p + alone)).max() <= 1e-15


def test_parse_window():
    from cutmix_semisup_seg_amd.tta import parse_window
    assert parse_window('512,1024') == (512, 1024) and parse_window('513') == (513, 513) and parse_window(' 16 , 24 ') == (16, 24)
    for bad in ('', ',', '16,', '16,24,3', 'a', '16.5', '0', '16,0', '-3', '16x24'):
        with pytest.raises(ValueError):
            parse_window(bad)


REFUSALS = r'''
import sys
from cutmix_semisup_seg_amd import eval_seg as E
from cutmix_semisup_seg_amd.tta import Windows

def refused(what, **kw):
    try:
        E.window_spec(**kw)
    except E.EvalNotRun as e:
        assert what in e.message, (what, e.message)
    else:
        raise AssertionError('not refused: {}'.format(kw))

assert E.window_spec(None) is None
w, b = E.window_spec('512,1024')
assert (w.window, w.stride, b) == ((512, 1024), (342, 683), None)
w, b = E.window_spec('513', '171', '4')
assert (w.window, w.stride, b) == ((513, 513), (171, 171), 4)
w, b = E.window_spec((16, 24), (11, 16), 2)
assert (w.window, w.stride, b) == ((16, 24), (11, 16), 2)
for bad in ('', 'a', '16,', '1,2,3', '0', '16.5'):
    refused('--window', window=bad)
    refused('--window_stride', window='16,24', window_stride=bad)
refused('without --window', window=None, window_stride='8')
refused('without --window', window=None, window_batch='2')
refused('[4, 16]', window='16,24', window_stride='3,6')
refused('[6, 24]', window='16,24', window_stride='4,5')
refused('[4, 16]', window='16,24', window_stride='17,24')
refused('--window_batch', window='16,24', window_batch='0')
refused('--window_batch', window='16,24', window_batch='-1')
refused('--window_batch', window='16,24', window_batch='two')
refused('--crf', window='16,24', crf=True)
refused('--calibration', window='16,24', calibration=True)
try:
    E.check_window_block(Windows((20, 24)), (8, 8))
except E.EvalNotRun as e:
    assert '16 and 24' in e.message and 'block size 8' in e.message, e.message
else:
    raise AssertionError('a window off the block size was taken')
E.check_window_block(Windows((16, 24)), (8, 8))
assert 'torch' not in sys.modules, 'torch was imported'
print('refusals ok')
'''


def test_eval_seg_window_refusals_need_no_torch():
    out = subprocess.run([sys.executable, '-c', REFUSALS], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and 'refusals ok' in out.stdout, out.stderr


def test_eval_seg_refuses_on_the_command_line_before_the_model_is_opened(tmp_path):
    from click.testing import CliRunner
    import eval_seg
    missing = str(tmp_path / 'missing.pth')
    for args, what in ((['--window', '16x24'], '--window'), (['--window_stride', '8'], 'without --window'),
                       (['--window_batch', '2'], 'without --window'), (['--window', '16,24', '--window_stride', '3,6'], '[4, 16]'),
                       (['--window', '16,24', '--window_batch', '0'], '--window_batch'), (['--window', '16,24', '--crf'], '--crf'),
                       (['--window', '16,24', '--calibration'], '--calibration')):
        res = CliRunner().invoke(eval_seg.experiment, [missing, '--dataset', 'pascal'] + args)
        assert res.exit_code != 0 and what in res.output and 'does not load' not in res.output, (args, res.output)
    res = CliRunner().invoke(eval_seg.experiment, [missing, '--dataset', 'pascal', '--window', '16,24'])
    assert res.exit_code != 0 and 'does not load' in res.output


def test_ops_check_their_arguments_before_the_library():
    import torch
    from cutmix_semisup_seg_amd import ops
    img = torch.zeros(1, 3, 8, 8)
    lg = [torch.zeros(4, 3, 2, 2)]
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.window_crop(img, (8, 8), False, (4, 4), (3, 3))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.window_vote(lg, [False], [(6, 6)], (4, 4), (2, 2), 3, (8, 8), want_pred=True)
    for exc, call in (
            (ValueError, lambda: ops.window_crop(img, (8, 8), False, (4, 4), (5, 3))),
            (ValueError, lambda: ops.window_crop(img, (8, 8), False, (8, 8), (1, 2))),
            (ValueError, lambda: ops.window_crop(img, (0, 8), False, (4, 4), (3, 3))),
            (TypeError, lambda: ops.window_crop(img[0], (8, 8), False, (4, 4), (3, 3))),
            (TypeError, lambda: ops.window_crop(img.double(), (8, 8), False, (4, 4), (3, 3))),
            (TypeError, lambda: ops.window_crop(img, 8, False, (4, 4), (3, 3))),
            (ValueError, lambda: ops.window_vote([], [], [], (4, 4), (2, 2), 3, (8, 8), want_pred=True)),
            (ValueError, lambda: ops.window_vote(lg, [False], [(6, 6)], (4, 4), (2, 2), 3, (8, 8))),
            (ValueError, lambda: ops.window_vote(lg, [False, True], [(6, 6)], (4, 4), (2, 2), 3, (8, 8), want_pred=True)),
            (ValueError, lambda: ops.window_vote(lg, [False], [(6, 6)], (4, 4), (5, 2), 3, (8, 8), want_pred=True)),
            (ValueError, lambda: ops.window_vote(lg, [False], [(6, 6)], (4, 4), (2, 2), 4, (8, 8), want_pred=True)),
            (ValueError, lambda: ops.window_vote(lg, [False], [(7, 6)], (4, 4), (2, 2), 3, (8, 8), want_pred=True)),     # 3 x 2 windows
            (ValueError, lambda: ops.window_vote([torch.zeros(4, 3, 5, 2)], [False], [(6, 6)], (4, 4), (2, 2), 3, (8, 8), want_pred=True)),
            (ValueError, lambda: ops.window_vote(lg, [False], [(6, 6)], (4, 4), (2, 2), 3, (8, 8), labels=torch.zeros(1, 8, 7, dtype=torch.uint8))),
            (ValueError, lambda: ops.window_vote(lg, [False], [(6, 6)], (4, 4), (2, 2), 3, (8, 8), cm=torch.zeros(3, 3, dtype=torch.int64))),
            (TypeError, lambda: ops.window_vote(lg, [False], [(6, 6)], (4, 4), (2, 2), 3, (8, 8), labels=torch.zeros(1, 8, 8))),
            (TypeError, lambda: ops.window_vote([lg[0][0]], [False], [(6, 6)], (4, 4), (2, 2), 3, (8, 8), want_pred=True))):
        with pytest.raises(exc):
            call()
