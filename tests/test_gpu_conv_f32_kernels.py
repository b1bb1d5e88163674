"""
GPU: the fp32 convolution family of csrc/conv_f32.hip -- conv_f32_kernel<2,2,2> / <2,1,2> / <1,1,1> in forward and data-gradient mode,
conv_wgrad_f32_kernel<2,2> / <2,1> / <1,2> / <1,1>, pack_transpose_f32_kernel -- through `ops.conv_igemm`, `ops.conv_wgrad` and
`ops.conv_pack_transpose`, against the plain fp64 references of tests/_conv_f32_refs.py (pinned against torch fp64 on the CPU by
tests/test_conv_f32_refs_cpu.py, which also asserts where each case lands and that the bounds below notice five mutations), on every
element, none excluded.

  forward   k1_m35 (one K stage, 32-tile, M = 35), cin96_t32 (three stages per tap, three 32-tiles, 2 x 128 + 14 pixels), t64_exact
            (64-tile, M = 256), t64_m129 (64-tile, a tail of one pixel), t128_s2 (128-tile, stride 2, M = 84), head18 (18 taps mostly
            outside the map, NCHW output with 21 of 32 channels, ksplit 1 / 4 / 5 / 7 / 18)
  epilogue  each of plain, scale, bias, scale + bias, relu, res, res + relu, all four; data gradient with neither, mask, res, both
  scatter   the four phases of the stride-2 data gradient: out_stride 2, out_pixel_offset 0, 1, W, W + 1, caller-owned pre-filled output
  wgrad     the four tile pairs and the padded class axis x ksplit 0 / 1 / 3 / 1000 x scale given / None, into a pre-filled buffer
  re-pack   channel counts that are no multiples of 32, flip, scale None: bit for bit
  refusals  Cin 48, Cout 40, ksplit above the taps, ksplit with an NHWC output, weight gradient with Cin 32: ValueError, output untouched

Tolerances are derived (tests/_conv_f32_refs.py: forward_bound, wgrad_bound); each check prints
`RATIO <what> <largest |got - ref| / bound>` before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import _conv_f32_refs as C
import _stream_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_id = lambda c: c.name


@pytest.fixture(scope='module')
def ops():
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


# ---- inputs and references: computed once and shared; nothing below writes to them
_finputs = functools.lru_cache(maxsize=None)(C.forward_inputs)
_winputs = functools.lru_cache(maxsize=None)(C.wgrad_inputs)
_sinputs = functools.lru_cache(maxsize=None)(C.scatter_inputs)


@functools.lru_cache(maxsize=None)
def _acc(case):
    """the bare sums (value, on absolute values) every epilogue of a case shares"""
    i = _finputs(case)
    taps, hw = C.case_taps(case), C.case_out_hw(case)
    return C.conv(i.x, i.w, taps, case.stride, hw), C.conv(np.abs(i.x), np.abs(i.w), taps, case.stride, hw)


@functools.lru_cache(maxsize=None)
def _wgrad_sums(case):
    """(ref, A) without scale and prefill: rescaled per variant below"""
    i = _winputs(case)
    return C.wgrad(i.du, i.x, C.case_taps(case), case.stride, None, None, None, 0.0)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _plan(case, ksplit=1):
    return C.fwd_plan(case.cin, case.cout, C.case_m(case), len(C.case_taps(case)), ksplit)


# ====================================================================================================== forward
def _run_forward(ops, case, s, b, r, relu):
    i = _finputs(case)
    hw = C.case_out_hw(case)
    y = ops.conv_igemm(_dev(i.x), _dev(i.w), C.case_taps(case), stride=case.stride, out_hw=hw, scale=_dev(i.scale) if s else None,
                       bias=_dev(i.bias) if b else None, res=_dev(i.res) if r else None, relu=bool(relu))
    assert y.dtype == torch.float32 and tuple(y.shape) == (case.n,) + hw + (case.cout,)
    ref, A = C.epilogue(*_acc(case), scale=i.scale if s else None, bias=i.bias if b else None, res=i.res if r else None, relu=bool(relu))
    return _np(y), ref, C.forward_bound(A, _plan(case), case.cin, s + b + r)


@pytest.mark.parametrize('epi', ['plain', 'scale_bias_res_relu'])
@pytest.mark.parametrize('case', [c for c in C.FORWARD if not c.cout_real], ids=_id)
def test_forward_every_tile_with_tails_and_odd_stage_counts(ops, case, epi):
    """NHWC output of every tile size at the smallest shapes that have one K stage, an odd number of stages per tap, a partial pixel
    tile of 1 / 14 / 35 / 84 pixels, none, and a strided input walk. d = taps x Cin + operands."""
    got, ref, bnd = _run_forward(ops, case, *C.EPILOGUES[epi])
    R.assert_within(got, ref, bnd, 'conv_f32 fwd {} {}'.format(case.name, epi))


@pytest.mark.parametrize('epi', list(C.EPILOGUES))
@pytest.mark.parametrize('case', C.EPILOGUE_CASES, ids=_id)
def test_forward_epilogue_operands_one_at_a_time(ops, case, epi):
    got, ref, bnd = _run_forward(ops, case, *C.EPILOGUES[epi])
    R.assert_within(got, ref, bnd, 'conv_f32 fwd {} {}'.format(case.name, epi))
    if C.EPILOGUES[epi][3]:
        assert (got >= 0).all()


@pytest.mark.parametrize('gate', list(C.GATES))
@pytest.mark.parametrize('case', C.EPILOGUE_CASES, ids=_id)
def test_data_gradient_every_gating_combination(ops, case, gate):
    """mode 1 on the same operands (x as the gradient, w as the transposed weights): (acc + res) * [mask > 0]. The mask holds exact
    +0.0 and -0.0 (gated); a gated element has bound 0: it must be an exact zero."""
    m, r = C.GATES[gate]
    i = _finputs(case)
    taps, hw = C.case_taps(case), C.case_out_hw(case)
    y = ops.conv_igemm(_dev(i.x), _dev(i.w), taps, out_hw=hw, mode=1, res=_dev(i.res) if r else None, mask_src=_dev(i.mask) if m else None)
    acc, Aacc = _acc(case)
    ref, A = C.epilogue(acc, Aacc, res=i.res if r else None)
    if m:
        ref, A = np.where(i.mask > 0, ref, 0.0), np.where(i.mask > 0, A, 0.0)
    R.assert_within(_np(y), ref, C.forward_bound(A, _plan(case), case.cin, r), 'conv_f32 dgrad {} {}'.format(case.name, gate))


@pytest.mark.parametrize('ksplit', C.HEAD_KSPLITS)
def test_head_nchw_output_with_every_kind_of_split(ops, ksplit):
    """fp32 NCHW output with 21 of 32 channels, pre-zeroed as the entry requires: ksplit 1 stores, 4 and 5 end in a ragged split, 7 in
    an EMPTY one (3 taps each for six splits), 18 has one tap per split; the bias is added once. d = taps per split x Cin + splits + 1."""
    case = C.F['head18']
    i = _finputs(case)
    taps, hw = C.case_taps(case), C.case_out_hw(case)
    plan = _plan(case, ksplit)
    x, w, bias = _dev(i.x), _dev(i.w), _dev(i.bias)
    run = lambda: ops.conv_igemm(x, w, taps, bias=bias, out_f32_nchw=torch.zeros((case.n, case.cout_real) + hw, device=DEV),
                                 cout_real=case.cout_real, ksplit=ksplit)
    out = run()
    ref, A = C.epilogue(*_acc(case), bias=i.bias)
    R.assert_within(_np(out), C.nchw(ref, case.cout_real), C.nchw(C.forward_bound(A, plan, case.cin, 1), case.cout_real),
                    'conv_f32 head18 ksplit {} (taps per split {})'.format(ksplit, plan.split_taps))
    if ksplit == 1:
        assert torch.equal(out, run()), 'the plain-store branch does not repeat bit for bit'


@pytest.mark.parametrize('phase', C.PHASES, ids=lambda p: 'phase{}{}'.format(*p))
def test_strided_scatter_into_a_caller_owned_output(ops, phase):
    """the stride-2 data gradient of t128_s2 as the phases of a transposed convolution: out_stride 2, out_pixel_offset py * W + px, 1 /
    2 / 2 / 4 taps, residual and mask read at the shifted positions. Visited positions within the bound, every other position the
    fill, bit for bit."""
    c, s = C.SCATTER, _sinputs()
    idx, taps, hw, off = C.scatter_phase(*phase)
    C.scatter_pixels(c.n, hw, (c.h, c.w), 2, off)                   # asserts that the launch stays inside the output tensor
    out = torch.full((c.n, c.h, c.w, c.cin), C.FILL, device=DEV)
    got = ops.conv_igemm(_dev(s.du), _dev(s.wT[idx]), taps, mode=1, res=_dev(s.res), mask_src=_dev(s.mask), out=out, out_hw=hw,
                         out_stride=2, out_full_hw=(c.h, c.w), out_pixel_offset=off)
    assert got is out
    ref, A = C.dgrad(s.du, s.wT[idx], taps, C.gathered(s.res, hw, 2, off), C.gathered(s.mask, hw, 2, off), hw)
    plan = C.fwd_plan(c.cout, c.cin, c.n * hw[0] * hw[1], len(taps))
    fill = np.full(out.shape, C.FILL)
    want, visited = C.scattered(ref, fill, 2, off)
    bnd, _ = C.scattered(C.forward_bound(A, plan, c.cout, 1), np.zeros(out.shape), 2, off)         # bound 0 outside: exact
    R.assert_within(_np(out), want, bnd, 'conv_f32 scatter phase {} offset {}'.format(phase, off))
    assert visited.sum() == c.n * hw[0] * hw[1] and np.array_equal(_np(out)[~visited], fill[~visited]), 'the launch wrote beside its phase'


# ====================================================================================================== weight gradient
@pytest.mark.parametrize('with_scale', [True, False], ids=['scale', 'noscale'])
@pytest.mark.parametrize('ksplit', C.WGRAD_KSPLITS)
@pytest.mark.parametrize('case', C.WGRAD, ids=_id)
def test_weight_gradient_every_tile_and_split(ops, case, ksplit, with_scale):
    """into a buffer pre-filled with 0.25; ksplit 0 = automatic, 1 = one slice (one atomic per element: repeats bit for bit), 3 = slices
    of 96 / 32 pixels with a partial last stage, 1000 = clamped to M / 32 slices. d = pixels per slice + slices. Rows cout_real ..
    dw_cout - 1 of the padded class axis have bound 0 and are checked bit for bit as well."""
    i = _winputs(case)
    taps = C.case_taps(case)
    plan = C.wgrad_plan(case.cin, case.cout, C.case_m(case), len(taps), ksplit)
    cr, dc = case.cout_real or case.cout, case.dw_cout or case.cout
    du, x, scale = _dev(i.du), _dev(i.x), _dev(i.scale) if with_scale else None

    def run():
        dw = torch.full((len(taps), dc, case.cin), C.PREFILL, device=DEV)
        ops.conv_wgrad(du, x, taps, dw, stride=case.stride, scale=scale, cout_real=case.cout_real, ksplit=ksplit, dw_cout=case.dw_cout)
        return dw
    dw = run()
    s = (i.scale.astype(np.float64) if with_scale else np.ones(case.cout))[None, :cr, None]
    part, Apart = _wgrad_sums(case)
    ref, A = np.full(dw.shape, C.PREFILL), np.zeros(dw.shape)
    ref[:, :cr] += part[:, :cr] * s
    A[:, :cr] = C.PREFILL + Apart[:, :cr] * s
    R.assert_within(_np(dw), ref, C.wgrad_bound(A, plan),
                    'conv_wgrad_f32 {} ksplit {} ({} x {} px) {}'.format(case.name, ksplit, plan.ksplit, plan.per, 'scale' if with_scale else 'noscale'))
    if dc > cr:
        assert torch.equal(dw[:, cr:], torch.full_like(dw[:, cr:], C.PREFILL)), 'rows beyond cout_real were written'
    if plan.ksplit == 1:
        assert torch.equal(dw, run()), 'one slice = one atomic per element, yet two launches differ'


# ====================================================================================================== re-pack
@pytest.mark.parametrize('with_scale', [True, False], ids=['scale', 'noscale'])
@pytest.mark.parametrize('flip', [True, False], ids=['flip', 'noflip'])
@pytest.mark.parametrize('shape', C.PACK_SHAPES, ids=str)
def test_pack_transpose_fp32_bit_for_bit(ops, shape, flip, with_scale):
    rng = np.random.RandomState(sum(shape))
    w = rng.randn(*shape).astype(np.float32)
    scale = (rng.rand(shape[1]) + 0.5).astype(np.float32) if with_scale else None
    out = torch.full((shape[0], shape[2], shape[1]), 7.0, device=DEV)
    got = ops.conv_pack_transpose(_dev(w), scale=_dev(scale), flip=flip, out=out, out_dtype=torch.float32)
    assert got is out and torch.equal(out.cpu(), torch.from_numpy(C.pack_transpose(w, scale, flip)))


# ====================================================================================================== refusals
def _untouched(t, fill):
    torch.cuda.synchronize()
    return torch.equal(t, torch.full_like(t, fill))


def test_host_refuses_unsupported_shapes_before_any_launch(ops):
    """CMS_REQUIRE return codes (ValueError through `check`): nothing is launched, the pre-filled output keeps its content"""
    z = lambda *s: torch.zeros(s, device=DEV)
    out = torch.full((1, 4, 4, 32), 2.5, device=DEV)
    with pytest.raises(ValueError, match='Cin'):
        ops.conv_igemm(z(1, 4, 4, 48), z(1, 32, 48), [(0, 0)], out=out)
    assert _untouched(out, 2.5)
    out = torch.full((1, 4, 4, 40), 2.5, device=DEV)
    with pytest.raises(ValueError, match='Cout'):
        ops.conv_igemm(z(1, 4, 4, 32), z(1, 40, 32), [(0, 0)], out=out)
    assert _untouched(out, 2.5)
    case = C.F['head18']
    i, taps, hw = _finputs(case), C.case_taps(case), C.case_out_hw(case)
    logits = torch.full((case.n, case.cout_real) + hw, 2.5, device=DEV)
    with pytest.raises(ValueError, match='ksplit'):
        ops.conv_igemm(_dev(i.x), _dev(i.w), taps, out_f32_nchw=logits, cout_real=case.cout_real, ksplit=19)
    assert _untouched(logits, 2.5)
    out = torch.full((case.n,) + hw + (case.cout,), 2.5, device=DEV)
    with pytest.raises(ValueError, match='ksplit'):
        ops.conv_igemm(_dev(i.x), _dev(i.w), taps, out=out, ksplit=2)
    assert _untouched(out, 2.5)
    dw = torch.full((1, 64, 32), 2.5, device=DEV)
    with pytest.raises(ValueError, match='Cin'):
        ops.conv_wgrad(z(1, 4, 4, 64), z(1, 4, 4, 32), [(0, 0)], dw)
    assert _untouched(dw, 2.5)
