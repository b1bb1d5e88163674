"""
CPU-only: csrc/crf_math.hpp -- the functions the kernels of csrc/crf.hip are made of -- driven on the host by a small program of its
own (tests/hostcheck_crf) over every case of the GPU test, against the fp64 restatement (tests/_crf_refs.py): Q within B
at every element, labels and both counts equal, no pixel left out. Then the refusals, sizes at which the launch's tiles end, and the
same stand-alone program once more under the host's address and undefined-behaviour sanitizers.
"""
import numpy as np
import pytest

import _hostcheck
import _crf_refs as R


@pytest.fixture(scope='module')
def host():
    exe = _hostcheck.build('hostcheck_crf')

    def run(inp, program=exe, **kw):
        return R.hostcheck_run(program, inp, **kw)
    return run


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_header_on_the_host_vs_reference_every_pixel(host, name):
    inp, ref = R.case(name)
    assert ref['gap'] >= 4 * R.B and ref['changed'] >= R.MIN_CHANGED
    err = R.compare(host(inp), ref)
    print(name, 'max |Q - Q_fp64| on the host =', err)


def test_one_iteration_of_a_five_iteration_case(host):
    inp, _ = R.case('c5_r2s3_t5_k3')
    one, ref = R.case('c5_r2s3_t5_k3', iters=1)
    got = host(one)
    assert np.abs(got['q'] - ref['q']).max() <= R.B and np.array_equal(got['unary_pred'], ref['unary_pred'])
    assert np.array_equal(got['unary_pred'], host(inp)['unary_pred'])


def test_without_weights_the_unary_prediction_comes_back(host):
    inp, ref = R.case('c21_r5s3_t5_k1')
    got = host(inp, bi_w=0.0, pos_w=0.0)
    assert np.array_equal(got['pred'], got['unary_pred']) and np.array_equal(got['pred'], ref['unary_pred'])
    assert got['stats'].tolist() == [int(ref['stats'][0]), 0]


# rectangles at which the 32 x 8 tiles of a residue class end: one short of / exactly / one past a tile in either direction, at
# dilation 1 and 3, inside a canvas with padding on every side
EDGES = [(1, 31, 7), (1, 32, 8), (1, 33, 9), (3, 94, 22), (3, 97, 25), (2, 1, 70), (1, 40, 1)]


@pytest.mark.parametrize('dilation,w,h', EDGES, ids=lambda v: str(v))
def test_tile_edges(host, dilation, w, h):
    """No seed search here: one class outweighs the others by far more than a message can move (|message| <= bi_w + pos_w = 7)."""
    rng = np.random.RandomState(w + h)
    H, W, c = h + 3, w + 2, 3
    best = rng.randint(0, c, size=(1, 1, H, W))
    logits = (np.arange(c).reshape(1, c, 1, 1) == best) * 40.0 - 20.0 + rng.standard_normal((1, c, H, W))
    inp = dict(logits=[logits.astype(np.float32)], flips=[False], rgb=R.make_image(1, H, W, w), rects=np.array([[2, 1, h, w]], dtype=np.int32),
               size=(H, W), align=True, radius=2, dilation=dilation, iters=2, prm=R.PARAMS)
    ref = R.refine(inp['logits'], inp['flips'], inp['rgb'], inp['rects'], inp['size'], True, 2, dilation, 2)
    assert ref['gap'] >= 0.5 and np.array_equal(ref['pred'], best[:, 0])
    R.compare(host(inp), ref)


def test_host_driver_refuses_what_the_library_refuses(host):
    inp, _ = R.case('tiny_5x7')
    for over in (dict(n=0), dict(c=0), dict(c=65), dict(H=0), dict(W=-1), dict(k=0), dict(k=17), dict(radius=0), dict(radius=6),
                 dict(dilation=0), dict(dilation=17), dict(iters=0), dict(iters=33), dict(bi_w=-1.0), dict(pos_w=float('nan')),
                 dict(bi_xy=0.0), dict(bi_rgb=-2.0), dict(pos_xy=float('inf')), dict(rects=[[0, 0, 6, 7]]), dict(rects=[[0, 1, 5, 7]]),
                 dict(rects=[[-1, 0, 5, 7]]), dict(rects=[[0, 0, 0, 7]])):
        host(inp, expect_code=2, **over)


def test_stand_alone_under_the_host_sanitizers(host):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_crf', sanitize=True)
    for name in ('c5_r2s3_t5_k3', 'c64_r5s3_t1_k3', 'c21_r5s16_t5_k3', 'tiny_5x7', 'one_pixel', 'full_canvas'):
        inp, ref = R.case(name)
        R.compare(host(inp, program=exe), ref)
