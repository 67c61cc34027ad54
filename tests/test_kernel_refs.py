"""tests/test_aux_kernels_gpu.py's cases at its bounds with RefBackend (the CPU training path) in
place of the HIP kernels, against the fp64 references of tests/kernel_refs.py: the case lists and
bounds are satisfiable by an fp32 implementation, and the CPU path is pinned to the same definitions.
Left out: the 21 M-element optimizer case, the NaN-poisoned split-K workspace (the CPU path has none)
and the entry points' argument checks."""
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
