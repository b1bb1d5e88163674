"""
CPU-only: csrc/window_math.hpp -- the functions the kernels of csrc/window.hip are made of -- driven on the host by a small program
of its own (tests/hostcheck_window) over every case of the GPU test, against the fp64 restatement
(tests/_window_refs.py): exact predictions and confusion matrices, the score errors the gap bound is derived from, the bit-for-bit
claims of the definition (one window per view: the vote of csrc/tta_math.hpp; the crop: the resize plus slicing), every descriptor
refusal, and the same stand-alone program once more under the host's address and undefined-behaviour sanitizers.
"""
import numpy as np
import pytest

import _hostcheck
import _tta_refs as T
import _window_refs as R


@pytest.fixture(scope='module')
def host():
    exe = _hostcheck.build('hostcheck_window')

    def run(cs, program=exe, **kw):
        return R.hostcheck_run(program, cs, **kw)
    run.exe = exe
    return run


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_header_on_the_host_vs_restatement(host, name):
    cs = R.case(name)
    got = host(cs)
    err = float(np.abs(got['score'].astype(np.float64) - cs['score']).max())
    print(name, 'max |fp32 - fp64| of a score on the host: {:.3g}; min gap {:.3g}'.format(err, cs['gap'].min()))
    # the bound is twice the largest figure printed here (the record is in _window_refs.py): every score is well inside it
    assert 2.0 * err <= R.GAP_BOUND
    assert np.array_equal(got['pred'], cs['pred'])                       # every pixel: the case's margins allow no exception
    assert np.array_equal(got['cm'], cs['cm'])


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_one_window_per_view_is_the_vote_bit_for_bit(host, name):
    """all views of one window, k >= 2: win_vote_pixel's scores and prediction are tta_vote_pixel's bits at every pixel"""
    cs = R.case(name)
    claims = host(cs)['claims']
    assert claims == (0 if cs['all_single'] and len(cs['logits']) >= 2 else -1)


def test_crop_is_resize_plus_slicing_bit_for_bit(host):
    """against the restatement of the resize (fp64: close) and against the crop of the view of the canvas' own size (exact)"""
    x = T.resize_input((2, 3, 37, 53))
    for view, flip, window, stride in ((R.CANVAS, False, R.WIN, R.STRIDE), (R.CANVAS, True, R.WIN, R.STRIDE),
                                       (R.HALF, True, R.WIN, R.STRIDE), (R.LARGE, False, R.WIN, R.WIN), (R.SMALL, True, R.WIN, (4, 6)),
                                       ((12, 53), False, R.WIN, R.STRIDE)):
        got = R.hostcheck_crop(host.exe, x, view, flip, window, stride)
        full = T.resize(x, view, flip)
        # one window that holds the whole view: the resize itself, in fp32 -- what the other windows must be slices of, bit for bit
        whole = R.hostcheck_crop(host.exe, x, view, flip, (64, 96), (43, 64))
        assert whole.shape == (2, 3) + tuple(view)
        (eh, ys), (ew, xs) = R.axis_grid(view[0], window[0], stride[0]), R.axis_grid(view[1], window[1], stride[1])
        assert got.shape == (2 * len(ys) * len(xs), 3, eh, ew) and np.isfinite(got).all()
        for n in range(2):
            for j, y1 in enumerate(ys):
                for i, x1 in enumerate(xs):
                    item = (n * len(ys) + j) * len(xs) + i
                    assert np.array_equal(got[item], whole[n, :, y1:y1 + eh, x1:x1 + ew])
        np.testing.assert_allclose(whole, full, rtol=1e-5, atol=1e-6)
        if view == R.CANVAS:
            assert np.array_equal(whole, x[..., ::-1] if flip else x)


def test_host_driver_refuses_what_the_library_refuses(host):
    cs = R.case('half_c21_k2_a1')
    for over in (dict(n=0), dict(c=0), dict(c=65), dict(H=0), dict(W=-1), dict(k=0), dict(k=17), dict(label_dtype=7),
                 dict(wh=0), dict(ww=-3), dict(null=('labels',)), dict(null=('cm', 'pred_out')), dict(null=('logits',)),
                 dict(views={1: dict(sh=0)}), dict(views={0: dict(sw=-1)}),
                 dict(views={0: dict(sh=17)}), dict(views={1: dict(sw=25)}),                      # above the window
                 dict(views={0: dict(sh=3)}), dict(views={1: dict(sw=5)}),                        # below ceil(window / 4)
                 dict(views={0: dict(eh=15)}), dict(views={1: dict(ew=27)}), dict(views={0: dict(gy=2)}), dict(views={1: dict(gx=3)}),
                 dict(views={0: dict(gy=4)}), dict(views={0: dict(Hv=0)}), dict(views={1: dict(Wv=-5)}),
                 dict(views={0: dict(Hv=49)}), dict(views={1: dict(Wv=24)}),                      # the view no longer gives gy / gx
                 dict(views={0: dict(hl=17)}), dict(views={1: dict(wl=25)}), dict(views={0: dict(hl=0)}),
                 dict(wh=17), dict(ww=23),                                                        # the grid no longer follows
                 dict(n=2 ** 20, views={0: dict(hl=16, wl=24)})):                                 # more than 2^31 - 1 logits / pixels
        host(cs, expect_code=2, **over)
    # and accepts what it should: no cm, no pred_out, the smallest and the largest stride
    got = host(cs, null=('cm',))
    assert not got['cm'].any()
    host(cs, null=('pred_out',))


def test_stride_limits_are_taken(host):
    for name in ('dense_c21_k1_a0_i64', 'nooverlap_c21_k1_a1'):
        cs = R.case(name)
        assert np.array_equal(host(cs)['pred'], cs['pred'])


def test_stand_alone_under_the_host_sanitizers(host):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_window', sanitize=True)
    for name in ('w3x3_c2_k1_a0_low', 'w3x3_c64_k2_a0_flip', 'dense_c2_k2_a1', 'large_c21_k2_a0', 'mixed_c21_k5_a0',
                 'mixed_c64_k5_a1', 'one_axis_c21_k2_a1', 'single_k1_c21', 'single_k1_c21_ident', 'single_k2_c19'):
        cs = R.case(name)
        got = host(cs, program=exe)
        assert np.array_equal(got['pred'], cs['pred']) and np.array_equal(got['cm'], cs['cm'])
    cs = R.case('half_c21_k2_a1')
    host(cs, program=exe, expect_code=2, views={0: dict(gy=4)})
    host(cs, program=exe, expect_code=2, null=('labels',))
    x = T.resize_input((1, 3, 9, 11))
    for view, flip in (((9, 11), False), ((13, 17), True), ((4, 5), True)):
        got = R.hostcheck_crop(exe, x, view, flip, (6, 8), (4, 5))
        assert np.isfinite(got).all()
