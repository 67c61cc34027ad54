"""tests/test_aux_kernels_gpu.py's cases at its bounds with RefBackend (the CPU training path) in
place of the HIP kernels, against the fp64 references of tests/kernel_refs.py: the case lists and
bounds are satisfiable by an fp32 implementation, and the CPU path is pinned to the same definitions.
Left out: the 21 M-element optimizer case, the NaN-poisoned split-K workspace (the CPU path has none)
and the entry points' argument checks."""
import numpy as np
import pytest
import torch

import kernel_cases as kc
from distributed_resnet_tensorflow_amd.ops import backend as backend_mod
from distributed_resnet_tensorflow_amd.ops.backend import RefBackend

DEV = "cpu"


@pytest.fixture(scope="module")
def be():
    """RefBackend(dtype=...) writes the module global _DT: put it back afterwards."""
    saved = backend_mod._DT[0]
    yield RefBackend("cpu", dtype=torch.float32)
    backend_mod._DT[0] = saved


@pytest.mark.parametrize("name", list(kc.SGEMM_CASES))
def test_sgemm(be, name):
    kc.run_sgemm(be, DEV, name)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("cols", kc.COLSUM_COLS)
@pytest.mark.parametrize("rows", kc.COLSUM_ROWS)
def test_colsum(be, rows, cols, scale, accumulate):
    kc.run_colsum(be, DEV, rows, cols, scale, accumulate)


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", kc.POOL_BNRELU_SHAPES)
def test_pool_bnrelu(be, shape, relu, bn):
    kc.run_pool_bnrelu(be, DEV, shape, relu, bn)


@pytest.mark.parametrize("kind", kc.MAXPOOL_KINDS)
@pytest.mark.parametrize("name", list(kc.MAXPOOL_GEOMS))
def test_maxpool_fwd(be, name, kind):
    kc.run_maxpool_fwd(be, DEV, name, kind)


@pytest.mark.parametrize("kind", kc.MAXPOOL_KINDS)
@pytest.mark.parametrize("name", list(kc.MAXPOOL_GEOMS))
def test_maxpool_bwd(be, name, kind):
    kc.run_maxpool_bwd(be, DEV, name, kind)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("with_wb", [True, False])
@pytest.mark.parametrize("g_bf16", [False, True])
@pytest.mark.parametrize("size", ["n4", "n1020"])
def test_sgd_momentum(be, size, g_bf16, with_wb, skip):
    kc.run_sgd(be, DEV, kc.SGD_N[size], g_bf16, with_wb, skip)


@pytest.mark.parametrize("size,g_bf16,with_wb,skip", [
    ("pair-first", False, True, 0), ("pair-first", True, False, 0), ("pair-first", True, True, 0),
    ("pair-first", False, False, 0), ("pair-first", False, True, 1)])
def test_sgd_momentum_capped_grid(be, size, g_bf16, with_wb, skip):
    kc.run_sgd(be, DEV, kc.SGD_N[size], g_bf16, with_wb, skip)


@pytest.mark.parametrize("size", list(kc.CAST_N))
def test_cast_bf16(be, size):
    kc.run_cast_bf16(be, DEV, kc.CAST_N[size])


@pytest.mark.parametrize("n", kc.FILL_N)
def test_fill(be, n):
    kc.run_fill(be, DEV, n)


@pytest.mark.parametrize("name", list(kc.ZERO_CASES))
def test_zero(be, name):
    kc.run_zero(be, DEV, name)


@pytest.mark.parametrize("name", kc.CIFAR_CASES)
def test_cifar_augment(be, name):
    kc.run_cifar_augment(be, DEV, name)


def test_cifar_augment_constant_image_is_exactly_zero(be):
    kc.run_cifar_constant(be, DEV)


@pytest.mark.parametrize("seed", kc.SYNTH_SEEDS)
@pytest.mark.parametrize("shape", list(kc.SYNTH_SHAPES))
def test_synthetic_images(be, shape, seed):
    kc.run_synthetic_images(be, DEV, shape, seed)


# =====================================================================================================
# Convolution and BatchNorm: tests/test_conv_bn_elementwise_gpu.py's cases that RefBackend can express
# (no kernel configurations, no split-K), then the new references themselves against fp64 autograd.
# =====================================================================================================
import torch.nn.functional as F  # noqa: E402

import kernel_refs as kr  # noqa: E402

CONV_ALL = kc.GLDS_CONV_CASES + kc.KS_CONV_CASES + ["nk-1x1", "nk-3x3-k32", "nk-s2-k32"]


@pytest.mark.parametrize("cls,pro", [("int", False), ("int", True), ("randn", False), ("randn", True), ("zeros", True)])
@pytest.mark.parametrize("name", CONV_ALL)
def test_conv_fwd(be, name, cls, pro):
    assert kc.run_conv_fwd(be, DEV, name, cls, pro)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("name", ["bwd-3x3", "bwd-nk"])
def test_conv_bn_bwd_epilogue(be, name, residual, cls):
    assert kc.run_conv_fwd(be, DEV, name, cls, False, residual=residual, bwd=True)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("size,oh,ow", [(s, oh, ow) for s in (9, 8) for oh in (0, 1) for ow in (0, 1)])
def test_conv_out_map(be, size, oh, ow, fill, cls):
    kc.run_conv_out_map(be, DEV, size, oh, ow, fill, cls)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("name", list(kc.DGRAD_CASES))
def test_conv_dgrad(be, name, cls):
    kc.run_dgrad(be, DEV, name, cls)


@pytest.mark.parametrize("cls,pro", [("int", False), ("int", True), ("randn", False), ("randn", True), ("zeros", True)])
@pytest.mark.parametrize("name", list(kc.WGRAD_CASES))
def test_conv_wgrad(be, name, cls, pro):
    assert kc.run_wgrad(be, DEV, name, cls, pro)


@pytest.mark.parametrize("M,C", kc.BN_RED_SHAPES)
def test_bn_stats(be, M, C):
    kc.run_bn_stats(be, DEV, M, C, 1)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("M,C", kc.BN_RED_SHAPES)
def test_bn_bwd_reduce(be, M, C, pool):
    kc.run_bn_bwd_reduce(be, DEV, M, C, 1, pool)


@pytest.mark.parametrize("running", [True, False])
@pytest.mark.parametrize("count", kc.FIN_COUNTS)
@pytest.mark.parametrize("G", kc.FIN_G)
def test_bn_finalize(be, G, count, running):
    kc.run_bn_finalize(be, DEV, 24, G, count, running)


@pytest.mark.parametrize("count", kc.FIN_COUNTS)
@pytest.mark.parametrize("G", kc.FIN_G)
def test_bn_finalize_bwd(be, G, count):
    kc.run_bn_finalize_bwd(be, DEV, 24, G, count)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", list(kc.BN_APPLY_SHAPES))
def test_bn_apply(be, shape, relu):
    kc.run_bn_apply(be, DEV, *kc.BN_APPLY_SHAPES[shape], relu)


@pytest.mark.parametrize("G", [1, 3, 8])
def test_bn_apply_fin(be, G):
    kc.run_bn_apply(be, DEV, *kc.BN_APPLY_SHAPES["c16"], True, fin=G)


@pytest.mark.parametrize("fin,add,pool", [(f, a, p) for f in (False, True) for a in (False, True) for p in (False, True)])
@pytest.mark.parametrize("name", ["small-c16", "mid-c64"])
def test_bn_bwd_apply(be, name, fin, add, pool):
    kc.run_bn_bwd_apply(be, DEV, name, fin, add, pool)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("name", ["3x3s2", "1x1s2", "nk-3x3s2"])
def test_conv_dgrad_stride2_phases(be, name, cls):
    kc.run_dgrad_phases(be, DEV, name, cls)


@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("name", ["3x3-m162", "1x1"])
def test_conv_bn_fin(be, name, bwd):
    kc.run_conv_bn_fin(be, DEV, "bwd-3x3" if bwd else name, bwd)


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("name", ["1x1", "3x3-m162"])
def test_conv_in_fin(be, name, G):
    kc.run_conv_in_fin(be, DEV, name, G)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("M,C", [(101, 16), (19, 256)])
def test_bn_apply_stats(be, M, C, relu):
    kc.run_bn_apply_stats(be, DEV, M, C, relu)


@pytest.mark.parametrize("add,pool", [(a, p) for a in (False, True) for p in (False, True)])
@pytest.mark.parametrize("M,C", [(203, 16), (3001, 64)])
def test_bn_bwd_apply_stats(be, M, C, add, pool):
    kc.run_bn_bwd_apply_stats(be, DEV, M, C, add, pool)


# -- the references against fp64 autograd ---------------------------------------------------------------
def _autograd_conv(x, w, P, Q, s, p, in_bn=None):
    """F.conv2d in fp64 with the explicit leading / trailing padding of the layer."""
    N, H, W, C = x.shape
    R = w.shape[1]
    op = x if in_bn is None else torch.relu(x * in_bn[0] + in_bn[1])
    xc = F.pad(op.permute(0, 3, 1, 2), (p, (Q - 1) * s + R - p - W, p, (P - 1) * s + R - p - H))
    return F.conv2d(xc, w.permute(0, 3, 1, 2), stride=s).permute(0, 2, 3, 1)


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("name", ["3x3-m162", "3x3s2-odd", "1x1s2", "c8-7x7s2"])
def test_reference_conv_and_gradients_match_autograd(name, pro):
    """kernel_refs.conv_fwd, kernel_cases.dgrad_ref and kernel_refs.conv_wgrad against fp64 autograd
    of F.conv2d (1e-12 of sum |terms|: both sides are fp64)."""
    N, H, W, C, K, R, s, p = kc.CONV_CASES[name]
    d = kc.conv_inputs(kc.CONV_CASES[name], "zeros" if pro else "randn", pro)
    x = d["x"].double().requires_grad_(True)
    w = d["w"].double().requires_grad_(True)
    in_bn = None if d["in_bn"] is None else tuple(t.double() for t in d["in_bn"])
    y = _autograd_conv(x, w, d["P"], d["Q"], s, p, in_bn) + d["res"].double()
    ref, bound, _ = kr.conv_fwd(d["x"], d["w"], d["P"], d["Q"], s, p, p, in_bn=d["in_bn"], residual=d["res"])
    assert bool(((ref - y.detach()).abs() <= 1e-12 * (1 + ref.abs())).all())
    assert bool((bound > 0).all())
    dy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    y.backward(dy)
    dw_ref, _ = kr.conv_wgrad(d["x"], dy, R, R, s, p, p, in_bn=d["in_bn"])
    assert bool(((dw_ref - w.grad).abs() <= 1e-11 * (1 + dw_ref.abs())).all())
    if not pro:   # (the data gradient is of the conv's own input)
        dx_ref, _ = kc.dgrad_ref(dy, d["w"], H, W, s, p)
        assert bool(((dx_ref - x.grad).abs() <= 1e-11 * (1 + dx_ref.abs())).all())
        # ... and the dgrad-as-forward-conv form the kernels run equals it too
        wt = d["w"].flip(1, 2).permute(3, 1, 2, 0).contiguous()
        as_fwd, _, _ = kr.conv_fwd(dy, wt, H, W, 1, R - 1 - p, R - 1 - p, dil=s)
        assert bool(((as_fwd - x.grad).abs() <= 1e-11 * (1 + as_fwd.abs())).all())


def test_reference_bn_relu_backward_matches_autograd():
    """bn_finalize_fwd -> bn_apply forward, relu_mask + bn_bwd_sums -> bn_finalize_bwd -> bn_bwd_apply
    backward against fp64 autograd of batch-norm + ReLU (+ the shortcut gradient)."""
    g = torch.Generator().manual_seed(5)
    M, C = 48, 16
    x = kc.bf_round(torch.randn(M, C, generator=g) * 2 + 0.5).double().requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).double().requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.1).double().requires_grad_(True)
    y = torch.relu(F.batch_norm(x, None, None, gamma, beta, training=True, eps=float(np.float32(1e-5))))
    dy = torch.randn(M, C, generator=g).double()
    y.backward(dy)
    xd = x.detach()
    parts = torch.stack([xd.sum(0), (xd * xd).sum(0)]).unsqueeze(0)
    fin = kr.bn_finalize_fwd(parts, M, gamma.detach(), beta.detach(), 1e-5, 0.997, None, None, fp32_math=False)
    sc, sh, mu, isd = (fin[k][0] for k in ("scale", "shift", "mean", "invstd"))
    yr, _ = kr.bn_apply(xd, sc, sh, True)
    assert torch.allclose(yr, y.detach(), rtol=1e-9, atol=1e-9)    # (parts is fp64 here, never rounded)
    mask, amb = kr.relu_mask(xd, sc, sh)
    assert amb == 0
    gm = torch.where(mask, dy, torch.zeros_like(dy))
    sums, _ = kr.bn_bwd_sums(gm, xd, mu, isd, 1)
    b = kr.bn_finalize_bwd(sums.unsqueeze(0), M, gamma.detach(), isd)
    k1, k2, k3 = b["coef"][0]
    dx, _ = kr.bn_bwd_apply(gm, xd, k1, k2, k3, mu, isd, None, (0, 2, 2, 4))
    assert torch.allclose(dx, x.grad, rtol=1e-8, atol=1e-9)
    assert torch.allclose(b["dgamma"][0], gamma.grad, rtol=1e-8, atol=1e-9)
    assert torch.allclose(b["dbeta"][0], beta.grad, rtol=1e-8, atol=1e-9)
