"""Deep-stem kernels (csrc/kernels/stem_deep.hip) against RefBackend in fp64, and the deep-stem step.

Continuous random bf16 data. With mag = the same conv over |a|, |w| and L = 9 C products per element,
e = L * 2^-24 * mag (fp32 accumulation, as tests/test_group_conv_gpu.py); with the BN + ReLU prologue the
kernel rounds every activation to bf16 once (relative 2^-9) where the fp64 reference does not, which adds
2^-9 * mag. bf16 outputs must lie within 2^-8 (|ref| + e) + e; statistics within M * 2^-24 * sum|terms| of
the sums of the STORED values. The pooled kernel stores no conv output, so its maxima are checked against
the fp64 pool with the window's largest bound, and its values and argmax bytes EXACTLY against the
reference max-pool of the plain kernel's stored output (the same MFMA sequence per pixel, so the same
bf16 values: rounding makes near-equal taps tie, which an unrounded reference would order differently).
Outputs are prefilled with NaN. Shifts are positive for every other channel (padding that passed through
the affine map would show), scales have mixed signs.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from distributed_resnet_tensorflow_amd.models.spec import imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops import _lib
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# (C, K, stride, pool, prologue) x H = W. The planner fits its tiles to the image, so per conv size P: 3, 6,
# 10, 17, 20 are one tile (34: 2 x 2 whole tiles of 17 x 17); P = 35 (H = 35, or 70 at stride 2) is 2 x 2 tiles
# of 18 x 18 with a partial last tile in both directions. Pooled: 10 -> 2 x 1 tiles, 17 -> 3 x 2 tiles with
# partial last ones, and the odd 35 -> 18 with the 'SAME' leading pad 1
KINDS = [(8, 32, 2, False, False), (32, 32, 1, False, False), (32, 32, 1, False, True),
         (32, 64, 1, True, False), (32, 64, 1, True, True)]
CASES = [k + (hw,) for k in KINDS for hw in (6, 20, 34, 70 if k[2] == 2 else 35)]
N = 2


@functools.lru_cache(maxsize=None)
def _case(C, K, stride, pro, H):
    """bf16 inputs, (scale, shift) or None, the fp64 conv reference and its bound's error term e."""
    g = torch.Generator().manual_seed(100 * C + 10 * H + K + pro)
    x = torch.randn((N, H, H, C), generator=g).bfloat16()
    w = (torch.randn((K, 3, 3, C), generator=g) / 8).bfloat16()
    bn = None
    if pro:
        sign = torch.where(torch.arange(C) % 4 < 2, 1.0, -1.0)
        scale = sign * (0.5 + torch.rand(C, generator=g))
        shift = torch.where(torch.arange(C) % 2 == 0, 0.5 + torch.rand(C, generator=g), -torch.rand(C, generator=g))
        bn = (scale.float(), shift.float())
    ref = RefBackend(dtype=torch.float64)
    P = (H - 1) // stride + 1
    y = torch.empty(N, P, P, K, dtype=torch.float64)
    ref.stem_deep_conv(x.double(), w.double(), y, stride, in_bn=None if bn is None else tuple(t.double() for t in bn))
    a = x.double() if bn is None else torch.relu(x.double() * bn[0].double() + bn[1].double())
    mag = torch.empty_like(y)
    ref.stem_deep_conv(a.abs(), w.double().abs(), mag, stride)
    e = (9 * C * 2.0 ** -24 + (2.0 ** -9 if pro else 0.0)) * mag
    return x, w, bn, y, e


def _stats_ok(stats, y, K):
    ys = y.double().cpu().reshape(-1, K)
    got = stats.double().sum(0).cpu()
    for which, terms in enumerate((ys, ys * ys)):
        assert ((got[which] - terms.sum(0)).abs() <= ys.shape[0] * 2.0 ** -24 * terms.abs().sum(0)).all(), which


@pytest.mark.parametrize("C,K,stride,pool,pro,H", CASES)
def test_kernel_against_fp64(C, K, stride, pool, pro, H):
    x, w, bn, ref, e = _case(C, K, stride, pro, H)
    be = HipBackend()
    in_bn = None if bn is None else tuple(t.cuda() for t in bn)
    y = torch.full(ref.shape, float("nan"), dtype=torch.bfloat16, device="cuda")
    stats = torch.zeros(8, 2, K, device="cuda")
    be.stem_deep_conv(x.cuda(), w.cuda(), y, stride, in_bn=in_bn, stats=stats)
    assert not torch.isnan(y.float()).any(), "unwritten elements"
    bound = 2.0 ** -8 * (ref.abs() + e) + e
    worst = ((y.double().cpu() - ref).abs() - bound).max().item()
    assert worst <= 0, worst
    _stats_ok(stats, y, K)
    if not pool:
        return
    PP = (ref.shape[1] + 1) // 2
    py = torch.full((N, PP, PP, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    parg = torch.full((N, PP, PP, K), 255, dtype=torch.uint8, device="cuda")
    pstats = torch.zeros(8, 2, K, device="cuda")
    be.stem_deep_conv_pool(x.cuda(), w.cuda(), py, parg, stride, in_bn=in_bn, stats=pstats)
    rb = RefBackend(dtype=torch.float64)
    want, want_arg = torch.empty(N, PP, PP, K, dtype=torch.float64), torch.empty(N, PP, PP, K, dtype=torch.uint8)
    total = (PP - 1) * 2 + 3 - ref.shape[1]                   # 'SAME': the smaller half of the padding leads
    pad = total // 2
    rb.maxpool_fwd(ref, want, want_arg, 3, 2, pad, pad)
    pb = F.max_pool2d(F.pad(bound.permute(0, 3, 1, 2), (pad, total - pad) * 2), 3, 2).permute(0, 2, 3, 1)
    assert ((py.double().cpu() - want).abs() <= pb).all()
    rb.maxpool_fwd(y.double().cpu(), want, want_arg, 3, 2, pad, pad)
    assert torch.equal(py.double().cpu(), want) and torch.equal(parg.cpu(), want_arg)
    _stats_ok(pstats, py, K)


def test_refusals():
    be = HipBackend()
    z = lambda *shape: torch.zeros(shape, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):   # 16 input channels
        be.stem_deep_conv(z(1, 8, 8, 16), z(32, 3, 3, 16), z(1, 8, 8, 32), 1)
    # the entry points refuse on their own (an error code, which the Python side raises), launching nothing
    for entry, C, K, stride in ((be.L.drn_stem_deep_conv, 16, 32, 1), (be.L.drn_stem_deep_conv, 32, 48, 1),
                                (be.L.drn_stem_deep_conv_pool, 32, 64, 3)):
        a = _lib.DrnStemDeepArgs()
        a.x, a.w, a.y, a.arg = (z(1, 8, 8, 64).data_ptr() for _ in range(4))
        a.N, a.H, a.W, a.C, a.K, a.stride = 1, 8, 8, C, K, stride
        with pytest.raises(_lib.KernelLibraryError):
            _lib.check(entry(ctypes.byref(a), be.stream()), "deep stem")


def _spec():
    return imagenet_resnet_v2(50, num_classes=7, image_size=64, deep_stem=True)


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


def test_fused_forward_equals_composed(monkeypatch):
    """pool_out of the fused forward against the composed one's (DRN_DEEP_STEM_FUSED=0), same weights and
    images: within one bf16 ulp (2^-7 relative to the larger magnitude)."""
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("DRN_DEEP_STEM_FUSED", fused)
        be = HipBackend()
        ex = Executor(_spec(), 4, be, "cuda", seed=1)
        assert ex.deep_fused == (fused == "1")
        be.synthetic_images(ex.images, seed=9)
        ex.be.zero_(ex.stats_arena)
        ex._deep_stem_fwd(True)
        if not ex.deep_fused:
            be.maxpool_fwd(ex.stem_out, ex.pool_out, ex.pool_arg, 3, 2, 0, 0)
        torch.cuda.synchronize()
        outs.append(ex.pool_out.float().cpu())
    a, b = outs
    diff, ulp = (a - b).abs(), 2.0 ** -7 * torch.maximum(a.abs(), b.abs())
    assert (diff <= ulp).all(), (int((diff > ulp).sum()), a.numel())


def test_stem_step_teacher_forced():
    """The procedure and tolerances of tests/test_resnext_gpu.py::test_every_block_teacher_forced for the stem:
    forward and backward from the SAME bf16 images and pool_out gradient as the fp32 reference executor."""
    torch.manual_seed(0)
    h = Executor(_spec(), 4, HipBackend(), "cuda", seed=5)
    r = Executor(_spec(), 4, RefBackend(), "cpu", seed=5)
    images = torch.zeros(h.images.shape)
    images[..., :3] = torch.randn(4, 64, 64, 3)
    dout = (torch.randn(h.pool_out.shape) * 0.1).bfloat16()
    for ex in (h, r):
        ex.P.master.copy_(h.P.master.cpu().bfloat16().float().to(ex.device))
        ex.sync_weights()
        ex.images.copy_(images.bfloat16().to(ex.device, ex.images.dtype))
        ex.be.zero_(ex.stats_arena)
        ex._deep_stem_fwd(True)
    # bf16 rounding makes near-equal taps tie, which the unrounded fp32 pool orders differently: the gradient
    # is routed by the SAME argmax bytes (tested exactly above), like every other input of the backward
    r.pool_arg.copy_(h.pool_arg.cpu())
    for ex in (h, r):
        bufs = [ex.g_a, ex.g_b, ex.g_c]
        ex._view(bufs[0], ex.pool_out).copy_(dout.to(ex.device, ex.pool_out.dtype))
        ex._deep_stem_bwd(bufs, 0)
        ex._join()
    torch.cuda.synchronize()
    errs = [("pool_out", _rel(h.pool_out, r.pool_out), 2e-2),
            ("pool_stats", _rel(h.pool_stats.sum(0), r.pool_stats.sum(0)), 2e-2)]
    for op in h.stem_pre_ops + [h.stem_op]:
        n = f"{op.conv.name}/kernel"
        errs.append((n, _rel(h.P.g(n), r.P.g(n)), 1e-1))
    for b in h.stem_bn:  # sums with cancellation: compare by direction
        for v in ("gamma", "beta"):
            n = f"{b.bn.name}/{v}"
            cos = torch.nn.functional.cosine_similarity(h.P.g(n).cpu(), r.P.g(n), dim=0).item()
            errs.append((n, 1 - cos, 5e-3))
    bad =[e for e in errs if not e[1] < e[2]]
    assert not bad, bad


def test_plan_replay_is_bitwise_the_eager_step(monkeypatch):
    """As tests/test_resnext_gpu.py: DRN_DETERMINISTIC=1, one eager step + two replays of the native plan
    leave the bits of three eager steps."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan

    def make():
        be = HipBackend()
        ex = Executor(_spec(), 4, be, "cuda", seed=3, weight_decay=1e-4)
        be.synthetic_images(ex.images, seed=9)
        ex.labels.copy_(torch.arange(4, dtype=torch.int32))
        ex.set_lr(0.02)
        return ex

    def state(ex):
        torch.cuda.synchronize()
        return [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.bn_state, ex.P.wbf16)]
    a = make()
    for _ in range(3):
        a.forward(train=True), a.backward(defer_tail=True), a.apply_gradients()
    want = state(a)
    b = make()
    plan = StepPlan(b, warmup=1)
    for _ in range(2):
        plan.replay()
    for name, x, y in zip(("master", "momentum", "bn_state", "wbf16"), state(b), want):
        assert torch.equal(x, y), name
