"""
GPU: the NHWC data-movement kernels of the DeepLab v3+ head (csrc/nhwc.hip) against their PyTorch formulations in fp32 on the
host -- values and every gradient: concat with a broadcast (N,1,1,C) input, bilinear upsample (align_corners False / True) into
a channel slice, global average pool, k-way gradient fan-in.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stream_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _tol(dtype):
    return dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_concat_with_broadcast_input(dtype):
    from cutmix_semisup_seg_amd import ops
    g = torch.Generator().manual_seed(0)
    N, H, W = 3, 9, 11
    xs = [torch.randn(N, H, W, c, generator=g).to(dtype) for c in (16, 48, 256)] + [torch.randn(N, 1, 1, 24, generator=g).to(dtype)]
    dy = torch.randn(N, H, W, 16 + 48 + 256 + 24, generator=g).to(dtype)
    ref_in = [x.float().clone().requires_grad_(True) for x in xs]
    ref = torch.cat(ref_in[:3] + [ref_in[3].expand(N, H, W, 24)], dim=3)
    ref.backward(dy.float())
    dev_in = [x.to(DEV).requires_grad_(True) for x in xs]
    out = ops.concat_channels(dev_in)
    out.backward(dy.to(DEV))
    assert torch.equal(out.detach().float().cpu(), ref.detach())                 # bit copies
    for a, b in zip(dev_in, ref_in):
        torch.testing.assert_close(a.grad.float().cpu(), b.grad, **_tol(dtype))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('geo', [(2, 9, 9, 17, 17), (2, 65 // 4, 65 // 4, 33, 33), (1, 5, 7, 20, 13), (2, 17, 17, 9, 9)],
                         ids=lambda g: 'x'.join(map(str, g)))
def test_upsample_concat_vs_interpolate(dtype, align, geo):
    from cutmix_semisup_seg_amd import ops
    N, h, w, H, W = geo
    g = torch.Generator().manual_seed(1)
    low = torch.randn(N, H, W, 48, generator=g).to(dtype)
    x = torch.randn(N, h, w, 32, generator=g).to(dtype)
    dy = torch.randn(N, H, W, 80, generator=g).to(dtype)
    lr, xr = low.float().clone().requires_grad_(True), x.float().clone().requires_grad_(True)
    up = F.interpolate(xr.permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=align).permute(0, 2, 3, 1)
    ref = torch.cat([lr, up], dim=3)
    ref.backward(dy.float())
    ld, xd = low.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    out = ops.upsample_concat(ld, xd, align_corners=align)
    out.backward(dy.to(DEV))
    torch.testing.assert_close(out.detach().float().cpu(), ref.detach(), **_tol(dtype))
    torch.testing.assert_close(ld.grad.float().cpu(), lr.grad, **_tol(dtype))
    if dtype == torch.bfloat16:
        # the derived bound on every element (tests/_stream_refs.py): fp32 accumulation of d products -- d = the number of output
        # pixels whose taps touch the source pixel -- then one bf16 rounding
        adj, A, d = R.upsample_bilinear_adjoint(dy[..., 48:].double().numpy(), (h, w), align, 'nhwc', np.float32)
        R.assert_within(xd.grad.double().cpu().numpy(), adj, R.bound(A, d, adj, bf16_out=True), 'upsample_nhwc_adjoint bf16 (test_gpu_nhwc)')
    else:
        torch.testing.assert_close(xd.grad.float().cpu(), xr.grad, **_tol(dtype))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_global_avg_pool_and_fanout(dtype):
    from cutmix_semisup_seg_amd import ops
    g = torch.Generator().manual_seed(2)
    N, H, W, C = 3, 13, 7, 72
    x = torch.randn(N, H, W, C, generator=g).to(dtype)
    dp = torch.randn(N, 1, 1, C, generator=g).to(dtype)
    xr = x.float().clone().requires_grad_(True)
    ref = xr.mean(dim=(1, 2), keepdim=True)
    ref.backward(dp.float())
    xd = x.to(DEV).requires_grad_(True)
    out = ops.global_avg_pool(xd)
    out.backward(dp.to(DEV))
    torch.testing.assert_close(out.detach().float().cpu(), ref.detach(), **_tol(dtype))
    torch.testing.assert_close(xd.grad.float().cpu(), xr.grad, **_tol(dtype))
    # fan-out: five consumers, one of them unused
    ws = [torch.randn(N, H, W, C, generator=g) for _ in range(4)]
    xr = x.float().clone().requires_grad_(True)
    sum((xr * w).sum() for w in ws).backward()
    xd = x.to(DEV).requires_grad_(True)
    al = ops.fanout(xd, 5)
    sum((a.float() * w.to(DEV)).sum() for a, w in zip(al[:4], ws)).backward()
    torch.testing.assert_close(xd.grad.float().cpu(), xr.grad, **_tol(dtype))
