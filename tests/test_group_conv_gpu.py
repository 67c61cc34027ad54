"""Grouped 3x3 convolution kernels (csrc/kernels/conv_group.hip) against an fp64 CPU reference.

`int` data (x, dy in [-2, 2], w in [-1, 1]): every partial sum is an integer below 2^24, exact in
fp32 in any order, so forward and data gradient must equal bf16(reference) bit for bit and the fp32
weight gradient the reference exactly. `randn` data: with e = L * 2^-24 * sum(|a||b|) over the L
products of an element (L = 9 cg forward / data gradient, N P Q weight gradient), bf16 outputs
must lie within 2^-8 (|ref| + e) + e and fp32 outputs within e. Outputs are prefilled with NaN.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from distributed_resnet_tensorflow_amd.ops import _lib
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# (cg, stride, N, H = W, C = K): 9 px = every border + the stride-2 remainder, 96 = a 64-channel slab
# with a tail; 17 px x 128 ch = several spatial tiles per image and several weight-gradient splits
SHAPES = [(cg, s, 2, 9, 96) for cg in (4, 8, 16, 32) for s in (1, 2)] + \
         [(cg, s, 3, 17, 128) for cg in (4, 32) for s in (1, 2)]
CASES = [sh + (kind,) for sh in SHAPES for kind in ("int", "randn")]


@functools.lru_cache(maxsize=None)
def _case(cg, stride, N, H, C, kind):
    """bf16 inputs, their fp64 references (y, dx, dw) and the error terms e of each."""
    g = torch.Generator().manual_seed(1000 * cg + 10 * H + stride)
    P = (H - 1) // stride + 1
    if kind == "int":
        draw = lambda shape, m: torch.randint(-m, m + 1, shape, generator=g).double()
    else:
        draw = lambda shape, m: torch.randn(shape, generator=g).bfloat16().double()
    x, w, dy = draw((N, H, H, C), 2), draw((C, 3, 3, cg), 1), draw((N, P, P, C), 2)

    def grads(x, w, dy):   # NHWC x, [K,3,3,cg] w, the project's padding (leading pad 1)
        x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
        end = (P - 1) * stride + 2 - H
        y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (1, end, 1, end)), w.permute(0, 3, 1, 2), stride=stride,
                     groups=C // cg).permute(0, 2, 3, 1)
        dx, dw = torch.autograd.grad(y, (x, w), dy)
        return y.detach(), dx, dw
    ref = grads(x, w, dy)
    mag = grads(x.abs(), w.abs(), dy.abs())
    err = [L * 2.0 ** -24 * m for L, m in zip((9 * cg, 9 * cg, N * P * P), mag)]
    return (x.bfloat16(), w.bfloat16(), dy.bfloat16()), ref, err


def _check(out, ref, e, kind):
    out = out.cpu()
    assert not torch.isnan(out.float()).any(), "unwritten elements"
    if kind == "int":
        assert torch.equal(out, ref.to(out.dtype))
        return
    bound = 2.0 ** -8 * (ref.abs() + e) + e if out.dtype == torch.bfloat16 else e
    worst = ((out.double() - ref).abs() - bound).max().item()
    assert worst <= 0, worst


@pytest.mark.parametrize("cg,stride,N,H,C,kind", CASES)
def test_forward_and_statistics(cg, stride, N, H, C, kind):
    (x, w, _), ref, err = _case(cg, stride, N, H, C, kind)
    y = torch.full(ref[0].shape, float("nan"), dtype=torch.bfloat16, device="cuda")
    stats = torch.zeros(8, 2, C, device="cuda")
    HipBackend().gconv_fwd(x.cuda(), w.cuda(), y, stride, stats=stats)
    _check(y, ref[0], err[0], kind)
    # the replicas sum to sum(y), sum(y^2) of the STORED values, to fp32 accumulation of M terms
    ys = y.double().cpu().reshape(-1, C)
    got = stats.double().sum(0).cpu()
    for which, terms in enumerate((ys, ys * ys)):
        assert ((got[which] - terms.sum(0)).abs() <= ys.shape[0] * 2.0 ** -24 * terms.abs().sum(0)).all(), which


@pytest.mark.parametrize("cg,stride,N,H,C,kind", CASES)
def test_data_gradient(cg, stride, N, H, C, kind):
    (x, w, dy), ref, err = _case(cg, stride, N, H, C, kind)
    dx = torch.full(x.shape, float("nan"), dtype=torch.bfloat16, device="cuda")
    HipBackend().gconv_dgrad(dy.cuda(), w.cuda(), dx, stride)
    _check(dx, ref[1], err[1], kind)


@pytest.mark.parametrize("cg,stride,N,H,C,kind", CASES)
def test_weight_gradient(cg, stride, N, H, C, kind):
    (x, w, dy), ref, err = _case(cg, stride, N, H, C, kind)
    be = HipBackend()
    dw = torch.full(w.shape, float("nan"), device="cuda")
    ws = torch.full((max(1, be.gconv_wgrad_ws_elems(x.shape, dy.shape, w.shape, stride)),), float("nan"), device="cuda")
    be.gconv_wgrad(x.cuda(), dy.cuda(), dw, stride, ws=ws)
    _check(dw, ref[2], err[2], kind)


def test_refusals():
    be = HipBackend()
    z = lambda *shape: torch.zeros(shape, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):   # 64-wide groups
        be.gconv_fwd(z(1, 8, 8, 128), z(128, 3, 3, 64), z(1, 8, 8, 128), 1)
    with pytest.raises(ValueError):   # C != K
        be.gconv_fwd(z(1, 8, 8, 64), z(96, 3, 3, 4), z(1, 8, 8, 96), 1)
    # the entry points refuse on their own (an error code, which the Python side raises), launching nothing
    x, w = z(1, 8, 8, 128), z(128, 3, 3, 64)
    for entry, cg, stride in ((be.L.drn_gconv_fwd, 64, 1), (be.L.drn_gconv_dgrad, 32, 3), (be.L.drn_gconv_wgrad, 12, 1)):
        a = _lib.DrnGconvArgs()
        a.x = a.dy = x.data_ptr()
        a.w, a.y, a.dx, a.dw = w.data_ptr(), x.data_ptr(), x.data_ptr(), w.data_ptr()
        a.N, a.H, a.W, a.P, a.Q, a.C, a.cg, a.stride = 1, 8, 8, 8, 8, 128, cg, stride
        with pytest.raises(_lib.KernelLibraryError):
            _lib.check(entry(ctypes.byref(a), be.stream()), "grouped conv")
