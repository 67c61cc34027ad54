"""Pooled projection kernels (csrc/kernels/pool_proj.hip) against an fp64 CPU reference.

`int` data (x, d_out in [-2, 2], w in [-1, 1], scale 1, shift 0): every quantity is exact, so ap, sc
and da must equal bf16(reference) bit for bit. `randn` data, from bf16 and fp32 rounding alone:
  ap: 2^-8 |ref| + 4 * 2^-24 * sum|terms|     (one bf16 rounding of an fp32 sum of four terms)
  sc: 2^-8 (|ref| + e) + e, e = (Cin 2^-24 + 2^-8) sum|a_pool||w|   (2^-8: the stash rounding of A)
  da: 2^-8 (|ref| + e) + e, e = Cout 2^-24 * 0.25 * sum|d_out||w|
The reference pools in fp64 from the bf16-rounded terms (raw input: bf16(relu(fp32(scale * x + shift))), the
fp32 value rounded once like the kernel's fma). Outputs are prefilled with NaN; two launches must agree bitwise.
"""
import ctypes

import pytest
import torch

from distributed_resnet_tensorflow_amd.ops import _lib
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# (N, H = W, Cin, Cout): M = 18, a partial M tile; a reduction tail and a column tail; several M tiles and
# column blocks (one stash writer per tile). WIDE: the smallest grids that take the 128-column tile (512
# workgroups), forward and data gradient, on exact data.
SHAPES = [(2, 6, 64, 128), (2, 6, 96, 72), (3, 18, 256, 512)]
WIDE = [(1, 128, 72, 1024), (1, 128, 1024, 72)]
FWD = [sh + (raw, kind) for sh in SHAPES for raw in (False, True) for kind in ("int", "randn")] + \
      [WIDE[0] + (raw, "int") for raw in (False, True)]
BWD = [sh + (kind,) for sh in SHAPES for kind in ("int", "randn")] + [WIDE[1] + ("int",)]


def _draw(g, kind, shape, m):
    if kind == "int":
        return torch.randint(-m, m + 1, shape, generator=g).double()
    return torch.randn(shape, generator=g).bfloat16().double()


def _run_twice(shapes, launch):
    """Two launches into NaN-prefilled bf16 outputs of `shapes`; asserts equal bits, returns the first."""
    runs = []
    for _ in range(2):
        outs = [torch.full(s, float("nan"), dtype=torch.bfloat16, device="cuda") for s in shapes]
        launch(*outs)
        runs.append(outs)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    return runs[0]


def _check(out, ref, bound, kind, what):
    out = out.cpu()
    assert not torch.isnan(out.float()).any(), f"{what}: unwritten elements"
    if kind == "int":
        assert torch.equal(out, ref.bfloat16()), what
        return
    worst = ((out.double() - ref).abs() - bound).max().item()
    print(f"{what}: worst error - bound = {worst:.3e}")
    assert worst <= 0, (what, worst)


@pytest.mark.parametrize("N,H,C,K,raw,kind", FWD)
def test_forward_and_stash(N, H, C, K, raw, kind):
    g = torch.Generator().manual_seed(100 * H + C + raw)
    x, w = _draw(g, kind, (N, H, H, C), 2), _draw(g, kind, (K, C), 1)
    scale, shift = torch.ones(C), torch.zeros(C)
    if raw and kind == "randn":
        scale, shift = torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
        assert (scale < 0).any()
    t = torch.relu((x * scale.double() + shift.double()).float().bfloat16().double()) if raw else x
    terms = [t[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    ap_ref = 0.25 * (terms[0] + terms[1] + terms[2] + terms[3])
    sc_ref = ap_ref @ w.t()
    e = (C * 2.0 ** -24 + 2.0 ** -8) * (ap_ref.abs() @ w.abs().t())
    xd, wd, bn = x.bfloat16().cuda(), w.bfloat16().view(K, 1, 1, C).cuda(), (scale.cuda(), shift.cuda()) if raw else None
    ap, sc = _run_twice((ap_ref.shape, sc_ref.shape), lambda ap, sc: HipBackend().pool_proj_fwd(xd, wd, sc, ap, in_bn=bn))
    _check(ap, ap_ref, 2.0 ** -8 * ap_ref.abs() + 4 * 2.0 ** -24 * sum(v.abs() for v in terms), kind, "ap")
    _check(sc, sc_ref, 2.0 ** -8 * (sc_ref.abs() + e) + e, kind, "sc")


@pytest.mark.parametrize("N,H,C,K,kind", BWD)
def test_data_gradient_writes_every_phase(N, H, C, K, kind):
    g = torch.Generator().manual_seed(100 * H + C + 7)
    dy, w = _draw(g, kind, (N, H // 2, H // 2, K), 2), _draw(g, kind, (K, C), 1)
    up = lambda v: v.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)   # noqa: E731
    ref, e = up(0.25 * (dy @ w)), up(K * 2.0 ** -24 * 0.25 * (dy.abs() @ w.abs()))
    dyd, wt = dy.bfloat16().cuda(), w.t().contiguous().bfloat16().view(C, 1, 1, K).cuda()
    da, = _run_twice((ref.shape,), lambda da: HipBackend().pool_proj_dgrad(dyd, wt, da))
    _check(da, ref, 2.0 ** -8 * (ref.abs() + e) + e, kind, "da")


def test_refusals():
    be = HipBackend()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.bfloat16, device="cuda")   # noqa: E731
    for H, C in ((7, 64), (6, 60)):   # an odd H; Cin % 8 != 0
        x, w, sc, ap = nan(1, H, 6, C), nan(128, 1, 1, C), nan(1, H // 2, 3, 128), nan(1, H // 2, 3, C)
        with pytest.raises(ValueError):
            be.pool_proj_fwd(x, w, sc, ap)
        with pytest.raises(ValueError):
            be.pool_proj_dgrad(sc, w.view(C, 1, 1, 128), x)
        # the entry points refuse on their own (an error code, which the Python side raises), launching nothing
        a = _lib.DrnPoolProjArgs()
        a.x = a.da = x.data_ptr()
        a.w, a.sc, a.dy, a.ap = w.data_ptr(), sc.data_ptr(), sc.data_ptr(), ap.data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout = 1, H, 6, C, 128
        for entry in (be.L.drn_pool_proj_fwd, be.L.drn_pool_proj_dgrad):
            with pytest.raises(_lib.KernelLibraryError):
                _lib.check(entry(ctypes.byref(a), be.stream()), "pooled projection")
        torch.cuda.synchronize()
        assert all(torch.isnan(t.float()).all() for t in (x, sc, ap))
