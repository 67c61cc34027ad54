"""The head, pooling, optimizer and input HIP kernels (sgemm, colsum, bnrelu_pool, maxpool_fwd /
maxpool_bwd, sgd_momentum, cast_bf16, fill_f32, cifar_augment, synthetic_images) element by element
against the fp64 references of tests/kernel_refs.py, at the shapes where each kernel takes another
path. The cases and drivers are tests/kernel_cases.py's, shared with tests/test_kernel_refs.py."""
import pytest
import torch

import kernel_cases as kc
import kernel_refs as kr
from distributed_resnet_tensorflow_amd.ops import _lib
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend

pytestmark = pytest.mark.gpu
DEV = "cuda"


# -- sgemm --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kc.SGEMM_CASES))
def test_sgemm(hip, name):
    ta, tb, M, N, K = kc.SGEMM_CASES[name][:5]
    # the path the case is for (a retune of SGEMM_TARGET_WG must not silently empty it)
    assert kr.sgemm_splits(M, N, K, HipBackend.SGEMM_TARGET_WG) == kc.SGEMM_CASES[name][-1]
    kc.run_sgemm(hip, DEV, name)


@pytest.mark.parametrize("name", ["empty-slice", "splitk-beta-bias-ldc", "imagenet-logits"])
def test_sgemm_splitk_writes_every_partial_tile(hip, name):
    """The split-K workspace is uninitialised memory shared across calls: after a first call it is
    overwritten with NaN, and the second call's output must be finite and within the bound -- every
    slice, the empty one included, wrote its own partial tile."""
    kc.run_sgemm(hip, DEV, name)
    assert HipBackend._sgemm_ws
    for ws in HipBackend._sgemm_ws.values():
        ws.fill_(float("nan"))
    kc.run_sgemm(hip, DEV, name)


# -- colsum -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("cols", kc.COLSUM_COLS)
@pytest.mark.parametrize("rows", kc.COLSUM_ROWS)
def test_colsum(hip, rows, cols, scale, accumulate):
    kc.run_colsum(hip, DEV, rows, cols, scale, accumulate)


# -- pool_bnrelu --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", kc.POOL_BNRELU_SHAPES)
def test_pool_bnrelu(hip, shape, relu, bn):
    kc.run_pool_bnrelu(hip, DEV, shape, relu, bn)


def test_pool_bnrelu_rejects_channels_not_a_multiple_of_8(hip):
    x = torch.zeros(2, 2, 2, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.KernelLibraryError):
        hip.pool_bnrelu(x, None, None, torch.zeros(2, 12, device=DEV))


# -- max-pool -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", kc.MAXPOOL_KINDS)
@pytest.mark.parametrize("name", list(kc.MAXPOOL_GEOMS))
def test_maxpool_fwd(hip, name, kind):
    kc.run_maxpool_fwd(hip, DEV, name, kind)


@pytest.mark.parametrize("kind", kc.MAXPOOL_KINDS)
@pytest.mark.parametrize("name", list(kc.MAXPOOL_GEOMS))
def test_maxpool_bwd(hip, name, kind):
    kc.run_maxpool_bwd(hip, DEV, name, kind)


def test_maxpool_rejects_more_than_2048_channels(hip):
    x = torch.zeros(1, 4, 4, 2056, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(1, 2, 2, 2056, dtype=torch.bfloat16, device=DEV)
    arg = torch.zeros(1, 2, 2, 2056, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.KernelLibraryError):
        hip.maxpool_fwd(x, y, arg, 3, 2, 0, 0)


# -- sgd_momentum (the plain kernel) ------------------------------------------------------------------
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("with_wb", [True, False])
@pytest.mark.parametrize("g_bf16", [False, True])
@pytest.mark.parametrize("size", ["n4", "n1020"])
def test_sgd_momentum(hip, size, g_bf16, with_wb, skip):
    kc.run_sgd(hip, DEV, kc.SGD_N[size], g_bf16, with_wb, skip)


# the capped grid (8192 x 256 threads): "pair-first" is the first size whose first thread enters the
# two-groups-in-flight loop, "pair-tail" (21 M elements, the one large case) runs the loop and the tail
@pytest.mark.parametrize("size,g_bf16,with_wb,skip", [
    ("pair-first", False, True, 0), ("pair-first", True, False, 0), ("pair-first", True, True, 0),
    ("pair-first", False, False, 0), ("pair-first", False, True, 1),
    ("pair-tail", False, True, 0), ("pair-tail", True, False, 0)])
def test_sgd_momentum_capped_grid(hip, size, g_bf16, with_wb, skip):
    kc.run_sgd(hip, DEV, kc.SGD_N[size], g_bf16, with_wb, skip)


def test_sgd_momentum_rejects_a_length_not_a_multiple_of_4(hip):
    w, m, g = (torch.zeros(6, device=DEV) for _ in range(3))
    with pytest.raises(_lib.KernelLibraryError):
        hip.sgd_momentum(w, m, g, None, torch.tensor([0.1], device=DEV), 0.9, 0.0, 1.0)


# -- cast_bf16 / fill_ / zero_ ------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(kc.CAST_N))
def test_cast_bf16(hip, size):
    kc.run_cast_bf16(hip, DEV, kc.CAST_N[size])


def test_cast_bf16_rejects_a_length_not_a_multiple_of_4(hip):
    with pytest.raises(_lib.KernelLibraryError):
        hip.cast_bf16(torch.zeros(6, device=DEV), torch.zeros(6, dtype=torch.bfloat16, device=DEV))


@pytest.mark.parametrize("n", kc.FILL_N)
def test_fill(hip, n):
    kc.run_fill(hip, DEV, n)


@pytest.mark.parametrize("name", list(kc.ZERO_CASES))
def test_zero(hip, name):
    kc.run_zero(hip, DEV, name)


# -- cifar_augment ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.CIFAR_CASES)
def test_cifar_augment(hip, name):
    kc.run_cifar_augment(hip, DEV, name)


def test_cifar_augment_constant_image_is_exactly_zero(hip):
    kc.run_cifar_constant(hip, DEV)


def test_cifar_augment_rejects_more_than_2048_pixels(hip):
    raw = torch.zeros(1, 33, 64, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, 33, 64, 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.KernelLibraryError):
        hip.cifar_augment(raw, torch.zeros(1, 3, dtype=torch.int32, device=DEV), out, 0)


# -- synthetic_images ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", kc.SYNTH_SEEDS)
@pytest.mark.parametrize("shape", list(kc.SYNTH_SHAPES))
def test_synthetic_images(hip, shape, seed):
    kc.run_synthetic_images(hip, DEV, shape, seed)
