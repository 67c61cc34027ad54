"""The kernels that carry the training step -- conv_fwd.hip (register-staged, the LDS-DMA configurations,
split-K, stream-K, narrow-output), conv_wgrad.hip, the shared epilogue of drn_conv_epi.h and bn.hip --
element by element against the fp64 references of tests/kernel_refs.py, on sentinel-prefilled outputs
with guard rows. Two data classes per conv case: `int` (every partial sum exact in fp32, so the output
must equal bf16(ref) bit for bit in every configuration) and `randn` / `zeros` under derived bounds;
statistics are checked as pure reductions of the values the kernel stored. The cases and drivers are
tests/kernel_cases.py's, shared with tests/test_kernel_refs.py (RefBackend, no GPU)."""
import pytest

import kernel_cases as kc

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the configuration id sets, checked against the library's own table by test_conv_cfg_table_matches_literals
from test_ops_gpu import BIG, BK32, IL, KS, N_GLDS  # noqa: E402
# (data class, fused prologue): zeros is about the prologue (a zero input is not padding)
DATA_PRO = [("int", False), ("int", True), ("randn", False), ("randn", True), ("zeros", True)]


def _refused(name, cfg):
    """tests/test_ops_gpu.py asserts these refusals; here they only select the applicable cases."""
    C = kc.CONV_CASES[name][3]
    narrow = C in (8, 16)
    return (C % 64 and not narrow and cfg not in BK32) or (narrow and (cfg in BK32 or cfg in BIG or cfg in IL))


@pytest.fixture(scope="module")
def nk0(hip):
    return hip.L.drn_conv_nk_cfg0()


# -- forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,pro", DATA_PRO)
@pytest.mark.parametrize("name,cfg", [(n, c) for n in kc.GLDS_CONV_CASES for c in range(N_GLDS) if not _refused(n, c)])
def test_conv_fwd_glds(hip, name, cfg, cls, pro):
    assert kc.run_conv_fwd(hip, DEV, name, cls, pro, cfg=cfg)


@pytest.mark.parametrize("cls,pro", DATA_PRO)
@pytest.mark.parametrize("name", kc.REG_CONV_CASES)
def test_conv_fwd_register_staged(hip, name, cls, pro):
    assert kc.run_conv_fwd(hip, DEV, name, cls, pro, cfg=100)


@pytest.mark.parametrize("cls,pro", DATA_PRO)
@pytest.mark.parametrize("name,i", [(n, i) for n in kc.NK_CONV_CASES for i in range(5)
                                    if kc.CONV_CASES[n][4] == 16 * (1, 1, 2, 2, 2)[i]])
def test_conv_fwd_narrow(hip, nk0, name, i, cls, pro):
    """(the refusal of the other channel count is test_conv_fwd_nk's)"""
    assert kc.run_conv_fwd(hip, DEV, name, cls, pro, cfg=nk0 + i)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("ks", [2, 3, 4, -3, -7, -16])
@pytest.mark.parametrize("cfg", KS)
@pytest.mark.parametrize("name", kc.KS_CONV_CASES)
def test_conv_fwd_splitk_streamk(hip, name, cfg, ks, cls):
    """ks > 1: split-K factor; ks < 0: stream-K over -ks workgroups. A launch is refused only with fewer
    k-stages than splits, or more workgroups than units (asserted in tests/test_ops_gpu.py)."""
    import ctypes
    ran = kc.run_conv_fwd(hip, DEV, name, cls, True, cfg=cfg, ks=ks)
    if not ran:
        N, H, W, C, K, R, s, p = kc.CONV_CASES[name]
        stages = R * R * C // (32 if cfg in BK32 else 64)
        if ks > 0:
            assert stages < ks, (cfg, ks)
        else:
            d = kc.conv_case(name, cls, True)
            import torch
            a = hip.conv_args(torch.zeros(N, H, W, C, dtype=torch.bfloat16, device=DEV),
                              torch.zeros(K, R, R, C, dtype=torch.bfloat16, device=DEV),
                              torch.zeros(N, d["P"], d["Q"], K, dtype=torch.bfloat16, device=DEV), d["geom"])
            assert hip.L.drn_conv_sk_slots_cfg(ctypes.byref(a), cfg, -ks) == 0, (cfg, ks)


# -- epilogue variants --------------------------------------------------------------------------------
EPI_CFGS = [3, 25, 100, "nk"]


def _epi_cfg(hip, cfg):
    return (hip.L.drn_conv_nk_cfg0() + 1, 16) if cfg == "nk" else (cfg, 64)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("size,oh,ow", [(s, oh, ow) for s in (9, 8) for oh in (0, 1) for ow in (0, 1)])
@pytest.mark.parametrize("cfg", EPI_CFGS)
def test_conv_out_map(hip, cfg, size, oh, ow, fill, cls):
    cfg, K = _epi_cfg(hip, cfg)
    kc.run_conv_out_map(hip, DEV, size, oh, ow, fill, cls, cfg=cfg, K=K)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("cfg", [0, 3, 6, 25, 28, 100, "nk"])
def test_conv_bn_bwd_epilogue(hip, cfg, residual, cls):
    name = "bwd-nk" if cfg == "nk" else "bwd-3x3"
    cfg = _epi_cfg(hip, cfg)[0]
    assert kc.run_conv_fwd(hip, DEV, name, cls, False, cfg=cfg, residual=residual, bwd=True)


# -- data gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("name,cfg", [("3x3", 100), ("3x3", 0), ("3x3", 25), ("1x1", 100), ("1x1", 13), ("3x3s2", 100),
                                      ("1x1s2", 100), ("nk-3x3", "nk"), ("nk-3x3", 100), ("nk-3x3", 23)])
def test_conv_dgrad(hip, name, cfg, cls):
    """Stride 2 runs on the register-staged kernel only (the zero-dilated input, dil = 2)."""
    kc.run_dgrad(hip, DEV, name, cls, cfg=_epi_cfg(hip, cfg)[0])


# -- weight gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,pro", [("int", False), ("int", True), ("randn", False), ("randn", True), ("zeros", True)])
@pytest.mark.parametrize("split", ["none", "slabs", "atomic"])
@pytest.mark.parametrize("ns", kc.WGRAD_NS)
@pytest.mark.parametrize("name", list(kc.WGRAD_CASES))
def test_conv_wgrad(hip, name, ns, split, cls, pro):
    ran = kc.run_wgrad(hip, DEV, name, cls, pro, ns=ns, split=split)
    if not ran:   # the narrow 32-channel dY tile needs 64-pixel stages (asserted in tests/test_ops_gpu.py)
        assert kc.WGRAD_CASES[name][4] <= 32 and ns in (4, 5, 6), (name, ns)


# -- bn_stats / bn_bwd_reduce -------------------------------------------------------------------------
@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("M,C", kc.BN_RED_SHAPES)
def test_bn_stats(hip, M, C, reps):
    kc.run_bn_stats(hip, DEV, M, C, reps)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("M,C", kc.BN_RED_SHAPES)
def test_bn_bwd_reduce(hip, M, C, reps, pool):
    kc.run_bn_bwd_reduce(hip, DEV, M, C, reps, pool)


# -- finalize -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("running", [True, False])
@pytest.mark.parametrize("count", kc.FIN_COUNTS)
@pytest.mark.parametrize("G", kc.FIN_G)
@pytest.mark.parametrize("C", [24, 200])
def test_bn_finalize(hip, C, G, count, running):
    kc.run_bn_finalize(hip, DEV, C, G, count, running)


@pytest.mark.parametrize("count", kc.FIN_COUNTS)
@pytest.mark.parametrize("G", kc.FIN_G)
@pytest.mark.parametrize("C", [24, 200])
def test_bn_finalize_bwd(hip, C, G, count):
    kc.run_bn_finalize_bwd(hip, DEV, C, G, count)


# -- applies ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", list(kc.BN_APPLY_SHAPES))
def test_bn_apply(hip, shape, relu):
    kc.run_bn_apply(hip, DEV, *kc.BN_APPLY_SHAPES[shape], relu)


def test_bn_apply_capped_grid(hip):
    """More vectors than two per thread of the capped grid: the two-in-flight loop runs twice for some
    threads, the single-vector tail for the others."""
    kc.run_bn_apply(hip, DEV, *kc.BN_APPLY_CAPPED, True)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("G", [1, 3, 5, 8])
@pytest.mark.parametrize("shape", ["c16", "c256"])
def test_bn_apply_fin(hip, shape, G, relu):
    kc.run_bn_apply(hip, DEV, *kc.BN_APPLY_SHAPES[shape], relu, fin=G)


def test_bn_apply_fin_split_finalize(hip):
    """At BN_FIN_SPLIT_C channels the publishing apply is the standalone finalize + the plain apply."""
    kc.run_bn_apply(hip, DEV, 37, 1024, True, fin=4)


@pytest.mark.parametrize("fin,add,pool", [(f, a, p) for f in (False, True) for a in (False, True) for p in (False, True)])
@pytest.mark.parametrize("name", ["small-c16", "mid-c64"])
def test_bn_bwd_apply(hip, name, fin, add, pool):
    kc.run_bn_bwd_apply(hip, DEV, name, fin, add, pool)


@pytest.mark.parametrize("fin,add,pool", [(False, False, False), (False, True, False), (True, True, False),
                                          (True, False, True)])
@pytest.mark.parametrize("name", ["c128", "c1024"])
def test_bn_bwd_apply_batches(hip, name, fin, add, pool):
    """Several 4-vector batches per thread of the capped grid with a partial last batch, below and at
    BN_FIN_SPLIT_C, on NaN-prefilled output."""
    kc.run_bn_bwd_apply(hip, DEV, name, fin, add, pool)


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("name,cfg", [("3x3s2", 0), ("3x3s2", 25), ("3x3s2", 100), ("1x1s2", 13), ("nk-3x3s2", "nk"),
                                      ("nk-3x3s2", 18)])
def test_conv_dgrad_stride2_phases(hip, name, cfg, cls):
    """The stride-2 data gradient as the step plan runs it: one launch per output parity through out_map."""
    kc.run_dgrad_phases(hip, DEV, name, cls, cfg=_epi_cfg(hip, cfg)[0])


@pytest.mark.parametrize("cls", ["int", "randn"])
@pytest.mark.parametrize("ns", kc.STEM_WGRAD_NS)
def test_conv_wgrad_packed_stem(hip, ns, cls):
    kc.run_stem_wgrad(hip, DEV, cls, ns)


# -- the finalize fused into other kernels ------------------------------------------------------------
@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("name,cfg", [("3x3-m162", 3), ("3x3-m162", 10), ("1x1", 0), ("1x1", 15), ("1x1", 25), ("1x1", 100),
                                      ("bwd-3x3", 6), ("bwd-nk", "nk")])
def test_conv_bn_fin(hip, name, cfg, bwd):
    if bwd:
        name = "bwd-nk" if cfg == "nk" else "bwd-3x3"
    kc.run_conv_bn_fin(hip, DEV, name, bwd, cfg=_epi_cfg(hip, cfg)[0])


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("name,cfg", [("1x1", 0), ("1x1", 25), ("1x1", 100), ("3x3-m162", 3), ("nk-1x1", "nk")])
def test_conv_in_fin(hip, name, cfg, G):
    kc.run_conv_in_fin(hip, DEV, name, G, cfg=_epi_cfg(hip, cfg)[0])


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("M,C", [(101, 16), (19, 256), (4099, 64)])
def test_bn_apply_stats(hip, M, C, relu):
    kc.run_bn_apply_stats(hip, DEV, M, C, relu)


@pytest.mark.parametrize("add,pool", [(a, p) for a in (False, True) for p in (False, True)])
@pytest.mark.parametrize("M,C", [(203, 16), (3001, 64), (37, 2048)])
def test_bn_bwd_apply_stats(hip, M, C, add, pool):
    kc.run_bn_bwd_apply_stats(hip, DEV, M, C, add, pool)
