"""
GPU: one descriptor entry point for the batch-statistics BatchNorm launches (cms_bn_run, csrc/bn.hip; the reference's
nn.BatchNorm2d in training mode, architectures/deeplab2.py:72-84, deeplab3plus.py:40-64).

Every path to a BatchNorm kernel -- ops.bn_op issued eagerly, ops.bn_op recorded into an ops.Program and replayed, and the
autograd functions behind ops.batch_norm_act / ops.frozen_bn_act -- fills a cms_bn_op and runs the same C function, so they
must agree BIT FOR BIT:
  (a) every kind (and every variant the selection rule distinguishes), eager against recorded + replayed;
  (b) batch_norm_act forward + backward against the explicit sequence stats -> apply, reduce_bwd -> bwd_apply with y as the
      mask; frozen_bn_act against 'apply';
  (c) the autograd path launches at once while a program is being recorded, and records nothing.
Shapes: 2 x 17 x 17 pixel rows -- 289 rows per group with two sample groups = 3 pixel splits of the tiled reduction; C = 72 = a
second, partial 64-channel tile; two groups = the group stride.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, H, W = 2, 17, 17
P = N * H * W
EPS, MOM = 1e-5, 0.1
SHAPES = [(C, G, dt) for C in (64, 72) for G in (1, 2) for dt in (torch.bfloat16, torch.float32)]
_sid = lambda s: 'C{}-G{}-{}'.format(s[0], s[1], 'bf16' if s[2] == torch.bfloat16 else 'fp32')


@functools.lru_cache(maxsize=None)
def _data(C, G, dtype):
    """Inputs of every kind, consistent with each other (real statistics, the real output and its mask bits, real backward
    sums). Built once per shape and never written again."""
    from cutmix_semisup_seg_amd import ops
    g = torch.Generator().manual_seed(1000 * C + 10 * G + int(dtype == torch.float32))
    act = lambda s, m=0.0: (torch.randn(N, H, W, C, generator=g) * s + m).to(dtype).to(DEV)
    d = dict(x=act(1.7, 0.3), res=act(1.0), dy=act(1.0), gamma=(torch.rand(C, generator=g) + 0.5).to(DEV),
             beta=(torch.randn(C, generator=g) * 0.2).to(DEV))
    flat = d['x'].double().view(G, P // G, C)
    d['fsums'] = torch.stack([flat.sum(1), (flat * flat).sum(1)], 1).reshape(-1).contiguous()          # [G][2][C]
    d['mean'] = flat.mean(1).float().reshape(-1).contiguous()
    d['rstd'] = (1.0 / torch.sqrt(flat.var(1, unbiased=False) + EPS)).float().reshape(-1).contiguous()
    d['scale'] = (d['gamma'] * d['rstd'].view(G, C)).reshape(-1).contiguous()
    d['shift'] = (d['beta'] - d['mean'].view(G, C) * d['scale'].view(G, C)).reshape(-1).contiguous()
    kw = dict(c=C, dtype=dtype, n_pixels=P, groups=G)
    d['y'], d['bits'] = torch.empty_like(d['x']), torch.empty(P * C // 8, dtype=torch.uint8, device=DEV)
    ops.bn_op('apply', relu=True, x=d['x'], res=d['res'], y=d['y'], scale=d['scale'], shift=d['shift'], mask_bits=d['bits'], **kw)
    d['bsums'] = torch.empty(G * 2 * C, dtype=torch.float64, device=DEV)
    ops.bn_op('reduce_bwd', x=d['x'], dy=d['dy'], y=d['y'], mean=d['mean'], rstd=d['rstd'], sums=d['bsums'],
              ws=ops.bn_workspace(P, C, DEV, G), **kw)
    torch.cuda.synchronize()
    return d


def _fresh(ops, d, C, G):
    """Output buffers with a defined start (the atomics-based reductions ADD to `sums`; running statistics and counters move)."""
    f32 = lambda n, v=0.0: torch.full((n,), v, device=DEV)
    return dict(y=torch.zeros_like(d['x']), dx=torch.zeros_like(d['x']), dres=torch.zeros_like(d['x']),
                bits=torch.zeros(d['x'].numel() // 8, dtype=torch.uint8, device=DEV),
                sums=torch.zeros(G * 2 * C, dtype=torch.float64, device=DEV),
                mean=f32(G * C), rstd=f32(G * C), scale=f32(G * C), shift=f32(G * C),
                running_mean=f32(C, 0.25), running_var=f32(C, 1.5), counter=torch.full((), 3, dtype=torch.int64, device=DEV),
                clear_a=torch.ones(2 * C, dtype=torch.float64, device=DEV), clear_b=torch.ones(2 * C, dtype=torch.float64, device=DEV),
                ws=ops.bn_workspace(d['x'].numel() // C, C, DEV, G))


def _finalize(ops, kw, d, o):          # one launch per sample group on slices, as the data-parallel callers issue it
    C, G = kw['c'], kw['groups']
    for g in range(G):
        sl = slice(g * C, (g + 1) * C)
        ops.bn_op('finalize', c=C, count=float(kw['n_pixels'] // G), eps=EPS, momentum=MOM, sums=d['fsums'][g * 2 * C:(g + 1) * 2 * C],
                  gamma=d['gamma'], beta=d['beta'], mean=o['mean'][sl], rstd=o['rstd'][sl], scale=o['scale'][sl], shift=o['shift'][sl],
                  running_mean=o['running_mean'], running_var=o['running_var'], counter=o['counter'], clear_a=o['clear_a'],
                  clear_b=o['clear_b'])


def _norm_outputs(o):
    return dict(mean=o['mean'], rstd=o['rstd'], scale=o['scale'], shift=o['shift'], running_mean=o['running_mean'],
                running_var=o['running_var'], counter=o['counter'])


# kind / variant -> (its launches through ops.bn_op, an output it must have written, one sample group only)
VARIANTS = {
    'reduce_ws': (lambda ops, kw, d, o: ops.bn_op('reduce', x=d['x'], sums=o['sums'], ws=o['ws'], **kw), 'sums', False),
    'reduce_atomics': (lambda ops, kw, d, o: ops.bn_op('reduce', x=d['x'], sums=o['sums'], **kw), 'sums', True),
    'finalize': (_finalize, 'mean', False),
    'apply': (lambda ops, kw, d, o: ops.bn_op('apply', relu=True, x=d['x'], res=d['res'], y=o['y'], scale=d['scale'],
                                              shift=d['shift'], **kw), 'y', False),
    'apply_bits': (lambda ops, kw, d, o: ops.bn_op('apply', relu=True, x=d['x'], res=d['res'], y=o['y'], scale=d['scale'],
                                                   shift=d['shift'], mask_bits=o['bits'], **kw), 'y', False),
    'reduce_bwd_y': (lambda ops, kw, d, o: ops.bn_op('reduce_bwd', x=d['x'], dy=d['dy'], y=d['y'], mean=d['mean'], rstd=d['rstd'],
                                                     sums=o['sums'], ws=o['ws'], **kw), 'sums', False),
    'reduce_bwd_bits': (lambda ops, kw, d, o: ops.bn_op('reduce_bwd', x=d['x'], dy=d['dy'], mean=d['mean'], rstd=d['rstd'],
                                                        sums=o['sums'], ws=o['ws'], mask_bits=d['bits'], **kw), 'sums', False),
    'reduce_bwd_atomics': (lambda ops, kw, d, o: ops.bn_op('reduce_bwd', x=d['x'], dy=d['dy'], y=d['y'], mean=d['mean'],
                                                           rstd=d['rstd'], sums=o['sums'], **kw), 'sums', True),
    'bwd_apply_y': (lambda ops, kw, d, o: ops.bn_op('bwd_apply', count=float(kw['n_pixels'] // kw['groups']), x=d['x'], dy=d['dy'],
                                                    y=d['y'], dx=o['dx'], dres=o['dres'], mean=d['mean'], rstd=d['rstd'],
                                                    gamma=d['gamma'], sums=d['bsums'], **kw), 'dx', False),
    'bwd_apply_bits': (lambda ops, kw, d, o: ops.bn_op('bwd_apply', count=float(kw['n_pixels'] // kw['groups']), x=d['x'], dy=d['dy'],
                                                       dx=o['dx'], dres=o['dres'], mean=d['mean'], rstd=d['rstd'], gamma=d['gamma'],
                                                       sums=d['bsums'], mask_bits=d['bits'], **kw), 'dx', False),
    'count': (lambda ops, kw, d, o: ops.bn_op('count', counter=o['counter']), 'counter', False),
    'stats': (lambda ops, kw, d, o: ops.bn_op('stats', eps=EPS, momentum=MOM, x=d['x'], ws=o['ws'], gamma=d['gamma'], beta=d['beta'],
                                              sums=o['sums'], **_norm_outputs(o), **kw), 'rstd', False),
}


def _eager_and_replayed(ops, launch, kw, d, fresh):
    """`launch` issued now into one set of output buffers, recorded + replayed into another: every buffer bit-identical."""
    a, b = fresh(), fresh()
    launch(ops, kw, d, a)
    prog = ops.Program()
    st = torch.cuda.current_stream()
    with ops.recording(prog, [st]):
        launch(ops, kw, d, b)
    assert prog.size() >= 1                      # recorded, not launched ...
    prog.run([st])
    torch.cuda.synchronize()
    for k in a:
        if k != 'ws':                            # (partial sums: scratch, never read by a caller)
            assert torch.equal(a[k], b[k]), k
    return a


# (the workspace-free reductions have no sample groups: bn_op refuses them)
CASES = [(v, s) for v in sorted(VARIANTS) for s in SHAPES if not (VARIANTS[v][2] and s[1] != 1)]
START = dict(sums=0.0, mean=0.0, rstd=0.0, y=0.0, dx=0.0, counter=3)          # what _fresh puts there


@pytest.mark.parametrize('variant,shape', CASES, ids=['{}-{}'.format(v, _sid(s)) for v, s in CASES])
def test_eager_and_recorded_launches_are_bit_identical(variant, shape):
    """(The atomics-based reductions add fp32 block sums into fp64 words. A block sum s is a multiple of its ulp, at least
    2^-23 |s|, and the totals stay below 2^11 (sum of squares: 578 rows x about 3): with every block sum above 2^-19 in
    magnitude -- they are sums of some 30 rows -- the running total always fits the 53 bits, every add is exact, and the
    order of the atomics cannot show in the bits.)"""
    from cutmix_semisup_seg_amd import ops
    C, G, dtype = shape
    launch, written, _ = VARIANTS[variant]
    d = _data(C, G, dtype)
    kw = dict(c=C, dtype=dtype, n_pixels=P, groups=G)
    a = _eager_and_replayed(ops, launch, kw, d, lambda: _fresh(ops, d, C, G))
    assert bool((a[written] != START[written]).any()), written          # (two untouched buffers would compare equal, too)
    if variant == 'apply_bits':
        assert torch.equal(a['bits'], d['bits']) and torch.equal(a['y'], d['y'])
    if variant == 'finalize':
        assert int(a['counter']) == 3 + G and float(a['clear_a'].abs().sum()) == 0.0 and float(a['clear_b'].abs().sum()) == 0.0


@functools.lru_cache(maxsize=None)
def _tile_data(G):
    """Tile sums of a real convolution launch: the smallest geometry of tests/test_gpu_conv_stats.py whose launch writes them
    (2 x 21 x 17 pixels, 64 -> 32 channels, 1 x 1: 128-row tiles, the last one partial, one straddling the group boundary)."""
    from cutmix_semisup_seg_amd import ops
    g = torch.Generator().manual_seed(77 + G)
    n, h, w, cin, cout = 2, 21, 17, 64, 32
    x = (torch.randn(n, h, w, cin, generator=g) * 0.8 + 0.1).to(torch.bfloat16).to(DEV)
    wt = (torch.randn(1, cout, cin, generator=g) * (1.5 / np.sqrt(cin))).to(torch.bfloat16).to(DEV)
    st = {'groups': G}
    ops.conv_igemm(x, wt, [(0, 0)], stats=st)
    torch.cuda.synchronize()
    return dict(x=x, tile_sums=st['tile_sums'], tile_rows=st['tile_rows'], gamma=(torch.rand(cout, generator=g) + 0.5).to(DEV),
                beta=(torch.randn(cout, generator=g) * 0.2).to(DEV)), n * h * w, cout


@pytest.mark.parametrize('G', [1, 2])
@pytest.mark.parametrize('kind', ['finalize_tiles', 'sums_tiles'])
def test_eager_and_recorded_tile_sum_launches_are_bit_identical(kind, G):
    from cutmix_semisup_seg_amd import ops
    d, M, C = _tile_data(G)
    if d['tile_rows'] == 0:
        pytest.skip('the library reports that this convolution launch cannot write tile sums')
    kw = dict(c=C, dtype=torch.bfloat16, n_pixels=M, groups=G, tile_rows=d['tile_rows'], ws=d['tile_sums'])
    if kind == 'finalize_tiles':
        launch = lambda ops, kw, d, o: ops.bn_op('finalize_tiles', eps=EPS, momentum=MOM, gamma=d['gamma'], beta=d['beta'],
                                                 **_norm_outputs(o), **kw)
    else:                                        # (the launch only adds tile sums: any launch's serve)
        launch = lambda ops, kw, d, o: ops.bn_op('sums_tiles', sums=o['sums'], **kw)
    a = _eager_and_replayed(ops, launch, kw, d, lambda: {k: v for k, v in _fresh(ops, d, C, G).items() if k != 'ws'})
    if kind == 'finalize_tiles':
        assert int(a['counter']) == 3 + G and bool((a['rstd'] > 0).all())
    else:
        assert bool((a['sums'].view(G, 2, C)[:, 1] > 0).all())          # sums of squares


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
def test_batch_norm_act_is_the_explicit_launch_sequence(with_res, relu, shape):
    from cutmix_semisup_seg_amd import ops
    C, G, dtype = shape
    d = _data(C, G, dtype)
    kw = dict(c=C, dtype=dtype, n_pixels=P, groups=G)
    # autograd
    x = d['x'].clone().requires_grad_(True)
    res = d['res'].clone().requires_grad_(True) if with_res else None
    gamma, beta = d['gamma'].clone().requires_grad_(True), d['beta'].clone().requires_grad_(True)
    a = _fresh(ops, d, C, G)
    y = ops.batch_norm_act(x, gamma, beta, a['running_mean'], a['running_var'], MOM, EPS, relu=relu, res=res, groups=G)
    y.backward(d['dy'])
    # the same launches by hand: y is the ReLU mask, no mask bits, no counter, no copy of the sums
    b = _fresh(ops, d, C, G)
    ops.bn_op('stats', eps=EPS, momentum=MOM, x=d['x'], ws=b['ws'], gamma=d['gamma'], beta=d['beta'], mean=b['mean'], rstd=b['rstd'],
              scale=b['scale'], shift=b['shift'], running_mean=b['running_mean'], running_var=b['running_var'], **kw)
    ops.bn_op('apply', relu=relu, x=d['x'], res=d['res'] if with_res else None, y=b['y'], scale=b['scale'], shift=b['shift'], **kw)
    mask = b['y'] if relu else None
    ops.bn_op('reduce_bwd', x=d['x'], dy=d['dy'], y=mask, mean=b['mean'], rstd=b['rstd'], sums=b['sums'], ws=b['ws'], **kw)
    ops.bn_op('bwd_apply', count=float(P // G), x=d['x'], dy=d['dy'], y=mask, dx=b['dx'], dres=b['dres'] if with_res else None,
              mean=b['mean'], rstd=b['rstd'], gamma=d['gamma'], sums=b['sums'], **kw)
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), b['y'])
    assert torch.equal(x.grad, b['dx'])
    if with_res:
        assert torch.equal(res.grad, b['dres'])
    local = b['sums'].view(G, 2, C).sum(0)       # the groups' passes add into the same parameter gradients
    assert torch.equal(gamma.grad, local[1].float()) and torch.equal(beta.grad, local[0].float())
    assert torch.equal(a['running_mean'], b['running_mean']) and torch.equal(a['running_var'], b['running_var'])
    assert bool((a['running_mean'] != 0.25).any())


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[1] == 1], ids=_sid)
@pytest.mark.parametrize('relu,with_res', [(False, False), (True, True)], ids=['linear', 'relu_res'])
def test_frozen_bn_act_forward_is_the_apply_kind(relu, with_res, shape):
    from cutmix_semisup_seg_amd import ops
    C, G, dtype = shape
    d = _data(C, G, dtype)
    res = d['res'] if with_res else None
    y = ops.frozen_bn_act(d['x'], d['scale'], d['shift'], relu=relu, res=res)
    want = torch.zeros_like(d['x'])
    ops.bn_op('apply', c=C, dtype=dtype, n_pixels=P, groups=1, relu=relu, x=d['x'], res=res, y=want, scale=d['scale'], shift=d['shift'])
    torch.cuda.synchronize()
    assert torch.equal(y, want)


def test_recording_does_not_capture_the_autograd_path():
    """ops.batch_norm_act / ops.frozen_bn_act launch at once while a program is being recorded: the U-Nets and the DeepLab v3+
    head run them eagerly beside recorded passes."""
    from cutmix_semisup_seg_amd import ops
    C, G, dtype = 72, 2, torch.bfloat16
    d = _data(C, G, dtype)

    def run():
        x = d['x'].clone().requires_grad_(True)
        o = _fresh(ops, d, C, G)
        y = ops.batch_norm_act(x, d['gamma'], d['beta'], o['running_mean'], o['running_var'], MOM, EPS, relu=True, res=d['res'], groups=G)
        y.backward(d['dy'])
        z = ops.frozen_bn_act(d['x'], d['scale'][:C].contiguous(), d['shift'][:C].contiguous(), relu=True)
        torch.cuda.synchronize()
        return y.detach(), x.grad, o['running_mean'], o['running_var'], z
    want = run()
    prog = ops.Program()
    with ops.recording(prog, [torch.cuda.current_stream()]):
        size = prog.size()
        got = run()                              # results are there without any replay
        assert prog.size() == size == 0
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_)
    assert bool((got[0] != 0).any()) and bool((got[2] != 0.25).any())
