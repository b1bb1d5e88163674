"""
GPU: the stem convolution kernels of csrc/stem.hip -- stem_fwd_kernel (all four type pairs but bf16 -> bf16), stem_fwd_mfma_kernel,
stem_wgrad_kernel, stem_wgrad_mfma_kernel, stem_wgrad_reduce_kernel, stem_dgrad_kernel -- through `ops.*`, against the plain fp64
references of tests/_stem_refs.py (pinned against torch fp64 on the CPU by tests/test_stem_refs_cpu.py, which also shows that the
bounds below notice one dropped or one stale tile), on every element, at

  persistent (66, 49, 97)   528 forward / matrix-core weight-gradient tiles for 512 / 256 workgroups, 1056 VALU weight-gradient tiles
                            for 768: every persistent loop takes a second trip (the matrix-core weight gradient a third), through
                            the barrier at its head, and a block accumulates over tiles of two images; ragged in both directions
                            (25 = 16 + 9 rows, 49 = 3 x 16 + 1 columns)
  edges                     images smaller than the 7 x 7 kernel (Ho, Wo of 1..3), a one-pixel ragged tile (16 x 34 -> 8 x 17), 33 x 47
  reduce                    N images of 9 x 9 = N one-tile blocks, N in {1, 3, 5, 13, 17}: the guards of the ordered combine

Tolerances are derived (tests/_stem_refs.py: forward_bound, wgrad_bound / wgrad_depth, dgrad_bound), d stated
there; each check prints `RATIO <what> <largest |got - ref| / bound>` before it asserts.

Not covered: CMS_STEM_MFMA=0 forces the VALU kernels for bf16 x bf16 (stem_fwd_kernel<uint16_t, uint16_t>,
stem_wgrad_kernel<uint16_t, uint16_t>); the library reads it once per process, so these two instances are left out.
"""
import functools

import numpy as np
import pytest
import torch

import _stem_refs as S
import _stream_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)]
_dn = lambda d: 'bf16' if d == BF16 else 'fp32'
_pid = lambda p: '{}x{}'.format(_dn(p[0]), _dn(p[1]))
_cid = lambda c: c.name
SLAB = 49 * 64 * 3 * 4


@pytest.fixture(scope='module')
def ops():
    from cutmix_semisup_seg_amd import ops as _ops
    return _ops


# ---- inputs and references: computed once per (case, types) and shared; nothing below writes to them
_inputs = functools.lru_cache(maxsize=None)(S.case_inputs)


@functools.lru_cache(maxsize=None)
def _forward_ref(case, x_bf16):
    i = _inputs(case)
    return S.stem_forward(S.typed(i.x, x_bf16), i.w, i.scale, i.bias)


@functools.lru_cache(maxsize=None)
def _wgrad_ref(case, x_bf16, ds_bf16):
    i = _inputs(case)
    return S.stem_wgrad(S.typed(i.x, x_bf16), S.typed(i.ds, ds_bf16), None)


@functools.lru_cache(maxsize=None)
def _dgrad_ref(case, ds_bf16):
    i = _inputs(case)
    return S.stem_dgrad(S.typed(i.ds, ds_bf16), i.w, i.scale, (case.h, case.w))


def _dev(a, dtype=F32):
    """fp32 numpy -> device tensor; `a` is bf16-exact where dtype is bf16 (S.typed), so the cast does not round"""
    return torch.from_numpy(a).to(dtype).to(DEV)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _w147(ops, case):
    return ops.stem_pack_weights(_dev(_inputs(case).w))          # fp32 weights that bf16 cannot hold


# ====================================================================================================== forward
@pytest.mark.parametrize('pair', PAIRS, ids=_pid)
@pytest.mark.parametrize('case', S.CASES, ids=_cid)
def test_stem_forward_every_type_pair(ops, case, pair):
    """image type -> output type. bf16 -> bf16 runs stem_fwd_mfma_kernel (persistent, at most 512 workgroups), the other three
    stem_fwd_kernel<TX, TY>. Bounds: S.forward_bound (d = 147; the matrix-core one adds 2^-16 A for the bf16 weight pair)."""
    xt, yt = pair
    mfma = xt == BF16 and yt == BF16
    i = _inputs(case)
    ho, wo, _, _ = ops.stem_out_hw(case.h, case.w)
    assert (ho, wo) == S.stem_out_hw(case.h, case.w)
    if case is S.PERSISTENT:
        # the reason this case exists: more tiles than persistent workgroups, so some take a second tile (of another image)
        ntiles = case.n * (-(-ho // 16)) * (-(-wo // 16))
        assert ntiles == 528 and ntiles > S.FWD_CAP and ho % 16 == 9 and wo % 16 == 1
    x = _dev(S.typed(i.x, xt == BF16), xt)
    y = ops.stem_forward(x, _w147(ops, case), _dev(i.scale), _dev(i.bias), yt)
    assert y.dtype == yt and tuple(y.shape) == (case.n, ho, wo, 64)
    ref, A = _forward_ref(case, xt == BF16)
    R.assert_within(_np(y), ref, S.forward_bound(A, ref, yt == BF16, mfma),
                    'stem_fwd{} {}->{} {}'.format('_mfma' if mfma else '', _dn(xt), _dn(yt), case.name))


# ====================================================================================================== weight gradient
def _blocks(ops, x, ds, case):
    nbytes = int(ops.fn['cms_stem_wgrad_workspace_bytes'](ops._dtype_code(x), ops._dtype_code(ds), case.n, case.h, case.w))
    assert nbytes % SLAB == 0
    return nbytes // SLAB


def _check_wgrad(ops, case, pair, with_scale, paths):
    xt, dt = pair
    i = _inputs(case)
    x, ds = _dev(S.typed(i.x, xt == BF16), xt), _dev(S.typed(i.ds, dt == BF16), dt)
    scale = _dev(i.scale) if with_scale else None
    plan = S.wgrad_plan(xt == BF16, dt == BF16, case.n, case.h, case.w)
    assert _blocks(ops, x, ds, case) == plan.nblocks                # the launch is the one the bound's d was read from
    if case is S.PERSISTENT:
        assert plan.nblocks == (256 if plan.mfma else 768) and plan.ntiles > plan.nblocks
    ref, A = S.scaled(*_wgrad_ref(case, xt == BF16, dt == BF16), i.scale if with_scale else None)
    what = 'stem_wgrad{} {}x{} {} {}'.format('_mfma' if plan.mfma else '', _dn(xt), _dn(dt), 'scale' if with_scale else 'noscale', case.name)
    fill = lambda: torch.full((49, 64, 3), S.PREFILL, device=DEV)
    was = ops.deterministic_wgrad()
    try:
        if 'atomics' in paths:
            # d = ceil(tiles / blocks) x pixels per tile (128 VALU, 256 matrix cores) + one addition per block (S.wgrad_depth)
            ops.set_deterministic_wgrad(False)
            dw = fill()
            ops.stem_wgrad(x, ds, dw, scale)
            R.assert_within(_np(dw), S.PREFILL + ref, S.wgrad_bound(A, S.PREFILL, plan), what + ' atomics')
            # the += contract: a second launch into the same buffer; the chain on the element is twice as long (calls = 2)
            ops.stem_wgrad(x, ds, dw, scale)
            R.assert_within(_np(dw), S.PREFILL + 2.0 * ref, S.wgrad_bound(A, S.PREFILL, plan, calls=2), what + ' atomics, twice')
        if 'slabs' in paths:
            # per-block slabs + stem_wgrad_reduce_kernel: the same d bounds its (shorter) ordered chain; and it repeats bit for bit
            ops.set_deterministic_wgrad(True)
            dw1, dw2 = fill(), fill()
            ops.stem_wgrad(x, ds, dw1, scale)
            ops.stem_wgrad(x, ds, dw2, scale)
            R.assert_within(_np(dw1), S.PREFILL + ref, S.wgrad_bound(A, S.PREFILL, plan), what + ' slabs')
            assert torch.equal(dw1, dw2), what + ': the deterministic path does not repeat'
    finally:
        ops.set_deterministic_wgrad(was)


@pytest.mark.parametrize('with_scale', [True, False], ids=['scale', 'noscale'])
@pytest.mark.parametrize('pair', PAIRS, ids=_pid)
@pytest.mark.parametrize('case', [S.PERSISTENT] + S.EDGES, ids=_cid)
def test_stem_wgrad_every_type_pair_both_combines(ops, case, pair, with_scale):
    """image type x dS type. bf16 x bf16 runs stem_wgrad_mfma_kernel (16 x 16 tiles, at most 256 workgroups), the other three
    stem_wgrad_kernel<TX, TS> (8 x 16 tiles, at most 768); scale None is the bn_trainable path. Both accumulate into a pre-filled
    buffer, through fp32 atomics or through slabs and the ordered reduce."""
    _check_wgrad(ops, case, pair, with_scale, ('atomics', 'slabs'))


@pytest.mark.parametrize('pair', PAIRS[:2], ids=_pid)
@pytest.mark.parametrize('case', S.REDUCE, ids=_cid)
def test_stem_wgrad_reduce_guards(ops, case, pair):
    """stem_wgrad_reduce_kernel deals slabs b, b + 4, b + 8, b + 12 over four thread groups, b = group + 16 k; with N one-tile
    images the block count is N: fewer than the 4 groups (1, 3), fewer than 16 (5, 13: the `b + 4 / 8 / 12 < nblocks` guards cut
    inside the first deal), 16 + 1 (a second deal for group 0 alone). The 17-block launch first leaves NON-ZERO partial sums in
    slabs 0..16 of the workspace the launches share, so a guard that lets a slab >= N through adds something."""
    big = S.REDUCE[-1]
    assert big.n == 17 and case.n <= big.n
    _check_wgrad(ops, big, pair, True, ('slabs',))
    _check_wgrad(ops, case, pair, True, ('slabs',))


# ====================================================================================================== data gradient
@pytest.mark.parametrize('dt', [F32, BF16], ids=_dn)
@pytest.mark.parametrize('case', [S.PERSISTENT] + S.EDGES, ids=_cid)
def test_stem_dgrad_both_types(ops, case, dt):
    """stem_dgrad_kernel<float> / <uint16_t> (bf16 dS: what the bf16 engine passes when the image needs a gradient).
    Bound: S.dgrad_bound, d = 64 x contributing taps of the pixel (1..16, from the reference) + 2."""
    i = _inputs(case)
    ds = _dev(S.typed(i.ds, dt == BF16), dt)
    dx = ops.stem_dgrad(ds, _w147(ops, case), _dev(i.scale), (case.n, 3, case.h, case.w))
    ref, A, taps = _dgrad_ref(case, dt == BF16)
    assert dx.dtype == F32
    R.assert_within(_np(dx), ref, S.dgrad_bound(A, taps), 'stem_dgrad {} {}'.format(_dn(dt), case.name))
