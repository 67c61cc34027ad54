"""The case lists of the auxiliary-kernel tests and one driver per operation. A driver takes a
backend and its device, builds the inputs, calls the backend's entry point on sentinel-prefilled
output buffers with guard elements, and checks the result element by element against
tests/kernel_refs.py. tests/test_aux_kernels_gpu.py runs them on HipBackend (the HIP kernels),
tests/test_kernel_refs.py on RefBackend (the CPU training path): the same cases, the same bounds.
The second half holds the convolution and BatchNorm cases of tests/test_conv_bn_elementwise_gpu.py.
"""
import numpy as np
import torch

import kernel_refs as kr
from kernel_refs import S, assert_within

SENT = -7.0      # prefill of float outputs (exact in bf16)
SENT_U8 = 0xAB   # prefill of the argmax record
GUARD = 64       # elements past the logical end of every output buffer


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def bf_round(t):
    return t.to(torch.bfloat16).float()


class Out:
    """An output buffer: `pre` guard elements, the logical tensor, GUARD guard elements; `init` (a
    CPU tensor of the logical size) or the sentinel everywhere."""

    def __init__(self, shape, dtype, dev, init=None, pre=0, sentinel=None):
        n = int(np.prod(shape))
        if sentinel is None:
            sentinel = SENT_U8 if dtype == torch.uint8 else SENT
        full = torch.full((pre + n + GUARD,), sentinel, dtype=dtype)
        if init is not None:
            full[pre:pre + n] = init.reshape(-1).to(dtype)
        self.before = full.clone()
        self.buf = full.to(dev)
        self.t = self.buf[pre:pre + n].view(shape)
        self.pre, self.n = pre, n

    def result(self):
        """The logical tensor (CPU) after checking that the guards kept their bits."""
        after = self.buf.cpu()
        assert _same_bits(after[:self.pre], self.before[:self.pre]), "guard before the buffer was written"
        assert _same_bits(after[self.pre + self.n:], self.before[self.pre + self.n:]), "guard past the end was written"
        return after[self.pre:self.pre + self.n].view(self.t.shape)

    def untouched(self):
        return _same_bits(self.buf.cpu(), self.before)


def _same_bits(a, b):
    if a.dtype.is_floating_point:
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
    return torch.equal(a, b)


def sync(dev):
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()


# -- sgemm --------------------------------------------------------------------------------------------
# name: (ta, tb, M, N, K, alpha, beta, bias, extra leading-dimension elements, expected split-K factor)
SGEMM_CASES = {
    # the three head calls (logits, dW, dpool) at the CIFAR head: batch 32, 10 classes, 64 channels
    "cifar-logits": (0, 1, 32, 10, 64, 1.0, 0.0, True, 0, 1),
    "cifar-dW": (1, 0, 10, 64, 32, 1.0, 0.0, False, 0, 1),
    "cifar-dpool": (0, 0, 32, 64, 10, 1.0, 0.0, False, 0, 1),
    # ... and at the ImageNet head: batch 8, 1001 classes, 2048 channels
    "imagenet-logits": (0, 1, 8, 1001, 2048, 1.0, 0.0, True, 0, 16),
    "imagenet-dW": (1, 0, 1001, 2048, 8, 1.0, 0.0, False, 0, 1),
    "imagenet-dpool": (0, 0, 8, 2048, 1001, 1.0, 0.0, False, 0, 7),
    # partial tiles on every axis, wide leading dimensions, alpha / beta / bias
    "odd-nn": (0, 0, 65, 129, 33, 0.5, -2.0, True, 3, 1),
    "odd-nt": (0, 1, 65, 129, 33, 0.5, -2.0, True, 3, 1),
    "odd-tn": (1, 0, 65, 129, 33, 0.5, -2.0, True, 3, 1),
    "odd-tt": (1, 1, 65, 129, 33, 0.5, -2.0, True, 3, 1),
    # 8 splits of 160: slice 7 starts past K and must still write its (zero) partial tile
    "empty-slice": (0, 1, 8, 8, 1025, 1.0, 0.0, False, 0, 8),
    # split-K with beta, bias and padding columns
    "splitk-beta-bias-ldc": (0, 0, 8, 70, 1001, 0.5, -2.0, True, 3, 7),
}


def run_sgemm(be, dev, name):
    ta, tb, M, N, K, alpha, beta, has_bias, extra, splits = SGEMM_CASES[name]
    g = _gen(M, N, K, ta, tb)
    ar, ac = (K, M) if ta else (M, K)
    br, bc = (N, K) if tb else (K, N)
    lda, ldb, ldc = ac + extra, bc + extra, N + extra
    A = torch.randn(ar, lda, generator=g)        # (the padding columns hold data too: a wrong stride shows)
    B = torch.randn(br, ldb, generator=g) * 0.5
    bias = torch.randn(N, generator=g) if has_bias else None
    C0 = torch.randn(M, ldc, generator=g) if beta != 0 else torch.full((M, ldc), SENT)
    out = Out((M, ldc), torch.float32, dev, init=C0)
    be.sgemm(ta, tb, M, N, K, alpha, A.to(dev), lda, B.to(dev), ldb, beta, out.t, ldc,
             bias=None if bias is None else bias.to(dev))
    sync(dev)
    got = out.result()
    ref, bound = kr.sgemm(ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C0, ldc, bias, splits)
    assert bool(torch.isfinite(got[:, :N]).all()), name
    assert_within(got[:, :N], ref, bound, f"sgemm: {name}")
    assert _same_bits(got[:, N:], C0[:, N:]), "padding columns (ldc > N) were written"


# -- colsum -------------------------------------------------------------------------------------------
COLSUM_ROWS = [1, 7, 8, 24, 25, 32, 33, 57, 128]   # around the 32-row unrolled loop and the 8-row tail
COLSUM_COLS = [1, 31, 32, 33, 1001]


def run_colsum(be, dev, rows, cols, scale, accumulate):
    g = _gen(rows, cols)
    x = torch.randn(rows, cols, generator=g)
    # (one more row of large values behind the input: a loop that runs one row too far sums it)
    xbuf = torch.cat([x, torch.full((1, cols), 1000.0)]).to(dev)
    out0 = torch.randn(cols, generator=g) if accumulate else None
    out = Out((cols,), torch.float32, dev, init=out0)
    be.colsum(xbuf[:rows], out.t, scale=scale, accumulate=bool(accumulate))
    sync(dev)
    ref, bound = kr.colsum(x, scale, accumulate, out0)
    assert_within(out.result(), ref, bound, f"colsum: {rows}x{cols} scale {scale} accumulate {accumulate}")


# -- pool_bnrelu --------------------------------------------------------------------------------------
POOL_BNRELU_SHAPES = [(3, 1, 1, 8), (2, 8, 8, 64), (2, 7, 5, 2048), (2, 3, 2, 2056)]


def run_pool_bnrelu(be, dev, shape, relu, bn):
    N, H, W, C = shape
    g = _gen(N, H, W, C)
    x = bf_round(torch.randn(N, H, W, C, generator=g))
    scale = torch.rand(C, generator=g) + 0.5 if bn else None
    shift = torch.randn(C, generator=g) * 0.3 if bn else None
    out = Out((N, C), torch.float32, dev)
    be.pool_bnrelu(x.to(dev, torch.bfloat16), None if scale is None else scale.to(dev),
                   None if shift is None else shift.to(dev), out.t, relu=relu)
    sync(dev)
    ref, bound = kr.pool_bnrelu(x, scale, shift, relu)
    assert_within(out.result(), ref, bound, f"pool_bnrelu: {shape} relu {relu} bn {bn}")


# -- max-pool -----------------------------------------------------------------------------------------
# (N, H, W, C, k, stride, pad_h, pad_w)
MAXPOOL_GEOMS = {
    "same-9x14-c24": (2, 9, 14, 24, 3, 2, 0, 0),        # TF 'SAME', H != W, C / 8 = 3 does not divide 256
    "pad1-5x7-c8": (1, 5, 7, 8, 3, 2, 1, 1),
    "c2048": (2, 12, 10, 2048, 3, 2, 0, 0),             # one output column per pass
    "rows4097": (241, 33, 4, 8, 3, 2, 0, 0),            # N * P = 4097: 4 rows per block, ragged last block
    # outside what the executor calls, accepted by the entry points
    "k2s2": (2, 7, 6, 16, 2, 2, 0, 0),
    "k4s2p1": (2, 8, 7, 16, 4, 2, 1, 1),                # three windows per dimension over a 2x2 block
    "k3s1p1": (2, 5, 6, 16, 3, 1, 1, 1),                # generic backward kernel
    "k3s3": (2, 8, 7, 16, 3, 3, 0, 0),
}
MAXPOOL_KINDS = ["randn", "ints"]


def maxpool_inputs(geom, kind):
    N, H, W, C, k, s, ph, pw = geom
    g = _gen(N, H, W, C, k, s, ph, len(kind))
    x = torch.randn(N, H, W, C, generator=g)
    if kind == "ints":   # ties in most windows: three levels for 9 or 16 taps, two for the 4 taps of k = 2
        x = x.round().clamp_(-1, 1) if k > 2 else torch.where(x > 0, 1.0, -1.0)
    else:
        x = bf_round(x)
    P, Q = kr.pool_out(H, k, s, ph), kr.pool_out(W, k, s, pw)
    dy = bf_round(torch.randn(N, P, Q, C, generator=g))
    return x, dy, P, Q


def run_maxpool_fwd(be, dev, name, kind):
    geom = MAXPOOL_GEOMS[name]
    N, H, W, C, k, s, ph, pw = geom
    x, _, P, Q = maxpool_inputs(geom, kind)
    y = Out((N, P, Q, C), torch.bfloat16, dev)
    arg = Out((N, P, Q, C), torch.uint8, dev)
    st = Out((3, 2, C), torch.float32, dev, init=torch.zeros(3, 2, C))   # 3 replicas, accumulated into
    be.maxpool_fwd(x.to(dev, torch.bfloat16), y.t, arg.t, k, s, ph, pw, stats=st.t)
    sync(dev)
    y_ref, arg_ref, nmax = kr.maxpool_fwd(x, k, s, ph, pw)
    if kind == "ints":
        assert float((nmax > 1).double().mean()) > 0.5, "the tie case has too few ties"
    assert torch.equal(y.result().double(), y_ref), f"maxpool_fwd y {name} {kind}"
    got = arg.result()
    ne = got != arg_ref
    assert not bool(ne.any()), (f"maxpool_fwd arg {name} {kind}: {int(ne.sum())} differ, first at "
                                f"{ne.nonzero()[0].tolist()}: {int(got[ne][0])} != {int(arg_ref[ne][0])}")
    ref, bound = kr.pool_stats(y_ref)
    assert_within(st.result().double().sum(0), ref, bound, f"maxpool_fwd stats: {name} {kind}")


def run_maxpool_bwd(be, dev, name, kind):
    geom = MAXPOOL_GEOMS[name]
    N, H, W, C, k, s, ph, pw = geom
    x, dy, P, Q = maxpool_inputs(geom, kind)
    _, arg_ref, _ = kr.maxpool_fwd(x, k, s, ph, pw)
    dx = Out((N, H, W, C), torch.bfloat16, dev)
    be.maxpool_bwd(dy.to(dev, torch.bfloat16), arg_ref.to(dev), dx.t, k, s, ph, pw)
    sync(dev)
    ref, bound = kr.maxpool_bwd(dy, arg_ref, k, s, ph, pw, H, W)
    got = dx.result()
    assert_within(got, ref, bound, f"maxpool_bwd: {name} {kind}")
    none = bound == 0   # pixels no window selected
    assert bool(none.any()) and bool((got[none] == 0).all())


# -- sgd_momentum -------------------------------------------------------------------------------------
SGD_N = {"n4": 4, "n1020": 1020, "pair-first": 4 * (S + 1), "pair-tail": 4 * (2 * S + S // 2 + 3)}
LR, MU, WD, GS = 0.1, 0.9, 2e-4, 0.5
_sgd_cache: dict = {}


def sgd_inputs(n):
    """w0, m0, g (bf16-representable, so one reference serves both gradient types) and the fp64
    results with their bounds; the latest size only is kept."""
    if n not in _sgd_cache:
        _sgd_cache.clear()
        g = _gen(n)
        w0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
        gr = bf_round(torch.randn(n, generator=g))
        _sgd_cache[n] = (w0, m0, gr) + kr.sgd_momentum(w0, m0, gr, LR, MU, WD, GS)
    return _sgd_cache[n]


def run_sgd(be, dev, n, g_bf16, with_wb, skip):
    w0, m0, gr, w_ref, m_ref, w_bound, m_bound = sgd_inputs(n)
    w, m = Out((n,), torch.float32, dev, init=w0), Out((n,), torch.float32, dev, init=m0)
    wb = Out((n,), torch.bfloat16, dev) if with_wb else None
    gd = gr.to(dev, torch.bfloat16 if g_bf16 else torch.float32)
    be.sgd_momentum(w.t, m.t, gd, wb.t if with_wb else None, torch.tensor([LR], device=dev), MU, WD, GS,
                    skip=torch.tensor([skip], dtype=torch.int32, device=dev))
    sync(dev)
    what = f"n {n} bf16 grad {g_bf16} wb {with_wb}"
    if skip:
        assert w.untouched() and m.untouched() and (wb is None or wb.untouched())
        return
    w_got = w.result()
    assert_within(w_got, w_ref, w_bound, f"sgd_momentum w: {what}")
    assert_within(m.result(), m_ref, m_bound, f"sgd_momentum m: {what}")
    if with_wb:
        assert _same_bits(wb.result(), w_got.to(torch.bfloat16)), "wb is not the bf16 rounding of w"


# -- cast_bf16 / fill_ / zero_ ------------------------------------------------------------------------
def _cast_specials():
    tie_down, tie_up = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8   # exact ties: to the even 1.0 / up to 1.015625
    vals = [tie_down, tie_up, -tie_down, -tie_up, 0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38,
            float("inf"), float("-inf"), 2.0 ** -127, -(2.0 ** -127), 2.0 ** -149, 2.0 ** -133 + 2.0 ** -141,
            float("nan"), 2.0 ** -126]
    return torch.tensor(vals, dtype=torch.float32)


CAST_N = {"n4": 4, "capped-grid": 4 * (S + 5)}


def run_cast_bf16(be, dev, n):
    sp = _cast_specials()
    assert sp.numel() % 4 == 0
    if n == 4:
        xs = [sp[i:i + 4].clone() for i in range(0, sp.numel(), 4)] + [torch.randn(4, generator=_gen(4))]
    else:
        x = torch.randn(n, generator=_gen(n))
        x[:sp.numel()] = sp
        x[-sp.numel():] = sp.flip(0)
        xs = [x]
    for x in xs:
        y = Out((x.numel(),), torch.bfloat16, dev)
        be.cast_bf16(x.to(dev), y.t)
        sync(dev)
        got, want = y.result(), x.to(torch.bfloat16)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), "NaN must stay NaN (and nothing else become one)"
        ne = (got.view(torch.int16) != want.view(torch.int16)) & ~nan
        assert not bool(ne.any()), (f"cast_bf16: {int(ne.sum())} differ, first at {ne.nonzero()[0].tolist()}: "
                                    f"{x[ne][0].item()!r} -> {got[ne][0].item()!r}, want {want[ne][0].item()!r}")


FILL_N = [1, 1023, S + 1]


def run_fill(be, dev, n):
    t = Out((n,), torch.float32, dev, pre=3)
    be.fill_(t.t, 1.25)
    sync(dev)
    assert torch.equal(t.result(), torch.full((n,), 1.25))


# name: (dtype, elements, guard elements in front)
ZERO_CASES = {"f32": (torch.float32, 1023, 3), "bf16-even": (torch.bfloat16, 1022, 6),
              "bf16-odd": (torch.bfloat16, 1023, 6), "bf16-2-bytes-in": (torch.bfloat16, 1022, 7)}


def run_zero(be, dev, name):
    dtype, n, pre = ZERO_CASES[name]
    t = Out((n,), dtype, dev, pre=pre)
    if name == "bf16-2-bytes-in":
        assert t.t.data_ptr() % 4 == 2
    be.zero_(t.t)
    sync(dev)
    assert _same_bits(t.result(), torch.zeros(n, dtype=dtype))


# -- cifar_augment ------------------------------------------------------------------------------------
def cifar_case(name):
    """raw uint8 [N, H, W, 3], params int32 [N, 3] = (oy, ox, flip), pad."""
    g = _gen(len(name), ord(name[0]))
    if name == "corners":       # the four corner crops of the 4-pixel padding x flip
        params = [(oy, ox, f) for oy in (0, 8) for ox in (0, 8) for f in (0, 1)]
        return torch.randint(0, 256, (8, 32, 32, 3), generator=g, dtype=torch.uint8), params, 4
    if name == "eval":          # the evaluation path: standardization only
        return torch.randint(0, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8), [(0, 0, 0)] * 2, 0
    if name == "32x64":         # the 2048-pixel limit
        return torch.randint(0, 256, (2, 32, 64, 3), generator=g, dtype=torch.uint8), [(3, 5, 1), (8, 0, 0)], 4
    if name == "low-contrast":  # bright, standard deviation 0.5: E[x^2] - mean^2 cancels in fp32
        return torch.randint(254, 256, (2, 32, 32, 3), generator=g, dtype=torch.uint8), [(0, 0, 0), (0, 0, 1)], 0
    raise KeyError(name)


CIFAR_CASES = ["corners", "eval", "32x64", "low-contrast"]


def _cifar_call(be, dev, raw, params, pad):
    N, H, W, _ = raw.shape
    out = Out((N, H, W, 8), torch.bfloat16, dev)
    be.cifar_augment(raw.to(dev), torch.tensor(params, dtype=torch.int32, device=dev), out.t, pad)
    sync(dev)
    return out.result()


def run_cifar_augment(be, dev, name):
    raw, params, pad = cifar_case(name)
    got = _cifar_call(be, dev, raw, params, pad)
    ref, bound = kr.cifar_augment(raw, torch.tensor(params), pad)
    assert bool((got[..., 3:] == 0).all()), "channels 3..7 must be exactly 0"
    assert_within(got[..., :3], ref, bound, f"cifar_augment: {name}")


def run_cifar_constant(be, dev):
    for H, W in ((32, 32), (32, 64)):
        raw = torch.tensor([0, 77, 255], dtype=torch.uint8)[:, None, None, None].expand(3, H, W, 3).contiguous()
        got = _cifar_call(be, dev, raw, [(0, 0, 0), (0, 0, 1), (0, 0, 0)], 0)
        assert bool((got == 0).all()), "a constant image standardizes to exactly 0"


# -- synthetic_images ---------------------------------------------------------------------------------
SYNTH_SHAPES = {"npix7": (1, 1, 7, 8), "capped-grid": (2, 1024, 1025, 8)}   # 2.1 M pixels > 8192 x 256
SYNTH_SEEDS = [17, 0x9E3779B9]                                             # the second is >= 2^31


def run_synthetic_images(be, dev, shape_name, seed):
    shape = SYNTH_SHAPES[shape_name]
    out = Out(shape, torch.bfloat16, dev)
    be.synthetic_images(out.t, seed)
    sync(dev)
    want = kr.synthetic_images(shape[0] * shape[1] * shape[2], seed).view(shape)
    assert _same_bits(out.result(), want)


# =====================================================================================================
# Convolution and BatchNorm kernels (conv_fwd.hip, conv_wgrad.hip, drn_conv_epi.h, bn.hip)
# =====================================================================================================
import ctypes  # noqa: E402

from distributed_resnet_tensorflow_amd.ops.backend import BnCfin, BnFin, ConvGeom, OutMap, dgrad_geom  # noqa: E402

BF16 = torch.bfloat16
NREP = 3         # statistics replicas the tests allocate (block b adds into replica b % 3)


def is_hip(be):
    return be.name == "hip"


def bfx(t):
    """A CPU tensor as the exact bf16 tensor both backends read."""
    return t.to(BF16)


def out_size(H, R, stride):
    return H if stride == 1 else (H - 1) // stride + 1


def _seed(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# name: (N, H, W, C, K, R, stride, pad)
CONV_CASES = {
    "3x3-m162": (2, 9, 9, 64, 64, 3, 1, 1),          # M = 162: not a multiple of 16, partial pixel tiles for every BP
    "3x3s2-odd": (2, 13, 13, 64, 128, 3, 2, 1),      # stride 2, odd size: M = 98
    "1x1": (3, 7, 7, 128, 256, 1, 1, 0),             # M = 147
    "1x1s2": (2, 8, 8, 256, 64, 1, 2, 0),
    "k72": (1, 6, 6, 192, 72, 3, 1, 1),              # K % BC != 0 (zero-page weight rows)
    "c96": (2, 9, 9, 96, 64, 3, 1, 1),               # C % 64 != 0: the 32-deep-stage configurations only
    "c8-7x7s2": (2, 16, 16, 8, 64, 7, 2, 3),         # row-staged stem
    "c8-3x3": (2, 9, 9, 8, 16, 3, 1, 1),             # row-staged, taps 3..7 of each stage zero pieces
    "c16": (2, 10, 10, 16, 16, 3, 1, 1),             # row-staged, 2 chunks per tap
    # the split-K / stream-K shapes (tests/test_ops_gpu.py SPLITK_CASES)
    "ks-3x3": (2, 9, 9, 64, 128, 3, 1, 1),
    "ks-k72": (1, 7, 7, 256, 72, 3, 1, 1),
    "ks-1x1": (3, 8, 8, 128, 256, 1, 1, 0),
    # narrow-output kernels (K = 16 / 32; C a power of two, at most 9 32-deep k-steps)
    "nk-1x1": (2, 9, 9, 64, 16, 1, 1, 0),
    "nk-3x3-k32": (3, 8, 8, 16, 32, 3, 1, 1),
    "nk-s2-k32": (1, 9, 9, 32, 32, 3, 2, 1),
    # the BN-backward epilogue / data-gradient shapes
    "bwd-3x3": (2, 10, 10, 128, 64, 3, 1, 1),
    "bwd-nk": (2, 10, 10, 16, 16, 3, 1, 1),
}
GLDS_CONV_CASES = ["3x3-m162", "3x3s2-odd", "1x1", "1x1s2", "k72", "c96", "c8-7x7s2", "c8-3x3", "c16"]
REG_CONV_CASES = ["3x3-m162", "3x3s2-odd", "1x1s2", "k72", "c8-7x7s2", "c16"]
NK_CONV_CASES = ["nk-1x1", "c16", "nk-3x3-k32", "nk-s2-k32", "c8-3x3"]
KS_CONV_CASES = ["ks-3x3", "ks-k72", "ks-1x1"]
CONV_DATA = ["int", "randn", "zeros"]   # zeros: randn with whole 8-channel chunks and whole pixels exactly 0
_conv_cache: dict = {}


def conv_inputs(shape, cls, pro, bwd=False, tag=0):
    """The inputs of one conv case (bf16-exact CPU tensors) drawn from a seed of the shape and the data
    class, never of the kernel configuration. int: small integers, weights in {-1, 0, 1}, prologue
    scale in {0.5, 1, 2} and shift in multiples of 0.5, so every operand is exact in bf16 and every
    partial sum a multiple of 0.5 below 2^23: fp32 accumulation is exact in any order (asserted)."""
    N, H, W, C, K, R, s, p = shape
    P, Q = out_size(H, R, s), out_size(W, R, s)
    g = _seed(N, H, W, C, K, R, s, p, CONV_DATA.index(cls), tag)
    d = {"P": P, "Q": Q}
    if cls == "int":
        d["x"] = torch.randint(-3, 4, (N, H, W, C), generator=g).float()
        d["w"] = torch.randint(-1, 2, (K, R, R, C), generator=g).float()
        d["res"] = torch.randint(-8, 9, (N, P, Q, K), generator=g).float()
        d["in_bn"] = (torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)],
                      torch.randint(-3, 4, (C,), generator=g).float() * 0.5) if pro else None
        if bwd:   # the mask input: x scale + shift is a multiple of 0.5 plus 0.25, never 0
            d["bn_bwd"] = (torch.randint(-3, 4, (N, P, Q, K), generator=g).float(),
                           torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (K,), generator=g)],
                           torch.randint(-3, 4, (K,), generator=g).float() * 0.5 + 0.25,
                           torch.randint(-2, 3, (K,), generator=g).float(),
                           torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (K,), generator=g)])
        op, _ = kr.conv_operand(d["x"], d["in_bn"])
        assert torch.equal(op, op.to(BF16).double()), "int class: a prologue value is not exact in bf16"
        big = float(op.abs().max()) * R * R * C + 8
        assert big < 2 ** 23 and bool((op * 2 == (op * 2).round()).all()), "int class: partial sums are not exact"
    else:
        d["x"] = bf_round(torch.randn(N, H, W, C, generator=g))
        d["w"] = bf_round(torch.randn(K, R, R, C, generator=g) * (2.0 / (R * R * C)) ** 0.5)
        d["res"] = bf_round(torch.randn(N, P, Q, K, generator=g))
        d["in_bn"] = (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5) if pro else None
        if cls == "zeros":   # a zero input is not padding: it becomes relu(shift) > 0
            d["x"].view(N, H, W, C // 8, 8)[:, ::2, :, ::2] = 0
            d["x"][:, ::3, 1::2] = 0
            d["x"][:, 0, 0] = 0
            d["x"][:, H - 1, W - 1] = 0
            if pro:
                d["in_bn"] = (d["in_bn"][0], torch.rand(C, generator=g) + 0.25)
        if bwd:
            d["bn_bwd"] = (bf_round(torch.randn(N, P, Q, K, generator=g)), torch.rand(K, generator=g) + 0.5,
                           torch.randn(K, generator=g) * 0.3, torch.randn(K, generator=g) * 0.1,
                           torch.rand(K, generator=g) + 0.5)
    return d


def conv_case(name, cls, pro, residual=True, bwd=False):
    """conv_inputs + the fp64 reference, cached per (case, data class, prologue, epilogue): every
    configuration shares one reference. The bound is affine in the number of extra partial
    combinations: bound(s) = b0 + s db."""
    key = (name, cls, pro, residual, bwd)
    if key not in _conv_cache:
        if len(_conv_cache) > 24:
            _conv_cache.clear()
        shape = CONV_CASES[name]
        N, H, W, C, K, R, s, p = shape
        d = conv_inputs(shape, cls, pro, bwd)
        kw = dict(in_bn=d["in_bn"], residual=d["res"] if residual else None, bn_bwd=d.get("bn_bwd"))
        ref, b0, amb = kr.conv_fwd(d["x"], d["w"], d["P"], d["Q"], s, p, p, **kw)
        _, b1, _ = kr.conv_fwd(d["x"], d["w"], d["P"], d["Q"], s, p, p, partials=1, **kw)
        assert amb == 0, f"{key}: {amb} elements with a ReLU mask that is ambiguous in fp32 (choose another seed)"
        d.update(ref=ref, b0=b0, db=b1 - b0, geom=ConvGeom(stride=s, pad_h=p, pad_w=p))
        _conv_cache[key] = d
    return _conv_cache[key]


def launch_conv(be, dev, x, w, y, g, cfg=None, ks=1, out_fill=False, **kw):
    """One conv launch: HipBackend with the configuration id and split forced (returns the library's
    status: nonzero = refused), RefBackend through conv_fwd."""
    if not is_hip(be):
        be.conv_fwd(x, w, y, g, out_fill=out_fill, **kw)
        return 0
    a = be.conv_args(x, w, y, g, **kw)
    if cfg is not None:
        a.cfg = cfg
    a.out_fill = 1 if out_fill else 0
    be._set_ksplit(a, ks)
    rc = be.L.drn_conv_fwd2(ctypes.byref(a), be.zero_page.data_ptr(), be.stream())
    sync(dev)
    return rc


def check_conv_out(got, d, cls, partials, what):
    """The stored output against the reference: bitwise bf16(ref) for the int class, the bound otherwise."""
    if cls == "int":
        want = d["ref"].float().to(BF16)
        ne = got.view(torch.int16) != want.view(torch.int16)
        ne &= ~((got == 0) & (want == 0))    # (-0 == +0)
        assert not bool(ne.any()), (f"{what}: {int(ne.sum())} of {ne.numel()} elements differ from bf16(ref), first at "
                                    f"{ne.nonzero()[0].tolist()}: {got[ne][0].item()!r} != {want[ne][0].item()!r}")
    else:
        assert_within(got, d["ref"], d["b0"] + partials * d["db"], what)


def check_conv_stats(st, got, d, bwd, what):
    """The statistics as a pure reduction of the values the kernel stored."""
    if bwd:
        xb, _, _, mu, isd = d["bn_bwd"]
        ref, bound = kr.bn_bwd_sums(got, xb, mu, isd, NREP)
    else:
        ref, bound = kr.conv_stats(got, NREP)
    assert_within(st.result().double().sum(0), ref, bound, what)


def run_conv_fwd(be, dev, name, cls, pro, cfg=None, ks=1, residual=True, bwd=False):
    """y (sentinel-prefilled, guards on both sides) and the statistics (zeroed, guards on both sides) of
    one conv launch. Returns False when the library refused the launch (the caller knows whether it may)."""
    d = conv_case(name, cls, pro, residual, bwd)
    N, H, W, C, K, R, s, p = CONV_CASES[name]
    y = Out((N, d["P"], d["Q"], K), BF16, dev, pre=GUARD)
    st = Out((NREP, 2, K), torch.float32, dev, init=torch.zeros(NREP, 2, K), pre=GUARD)
    kw = dict(residual=bfx(d["res"]).to(dev) if residual else None, stats=st.t,
              in_bn=None if d["in_bn"] is None else tuple(t.to(dev) for t in d["in_bn"]))
    if bwd:
        xb, sc, sh, mu, isd = d["bn_bwd"]
        kw["bn_bwd"] = (bfx(xb).to(dev),) + tuple(t.to(dev) for t in (sc, sh, mu, isd))
    rc = launch_conv(be, dev, bfx(d["x"]).to(dev), bfx(d["w"]).to(dev), y.t, d["geom"], cfg=cfg, ks=ks, **kw)
    if rc != 0:
        assert y.untouched() and st.untouched(), "a refused launch wrote memory"
        return False
    partials = 0 if ks == 1 else abs(ks)
    what = f"{name} {cls} pro {pro} cfg {cfg} ks {ks}"
    got = y.result()
    check_conv_out(got, d, cls, partials, f"conv_fwd{' bn_bwd' if bwd else ''} y: {what}")
    check_conv_stats(st, got, d, bwd, f"conv_fwd{' bn_bwd' if bwd else ''} stats: {what}")
    # (the split-K workspace and tickets are the backend's own buffers, sized by _set_ksplit: no guards there)
    if is_hip(be) and ks != 1:
        assert int(be.ks_tickets.abs().sum()) == 0, "a split-K ticket was not re-armed"
    return True


_map_cache: dict = {}


# -- strided output map (phases of a stride-2 data gradient), out_fill ---------------------------------
def run_conv_out_map(be, dev, size, oh, ow, fill, cls, cfg=None, K=64):
    """A 1x1 conv whose P x Q grid lands at y[:, 2i + oh, 2j + ow] of a size x size output. Without
    out_fill every other position keeps the sentinel; with it they are exactly 0. The residual
    (read through the same map) rides along where the entry point allows it (no out_fill)."""
    N, C = 2, 64
    Pp, Qp = (size - oh + 1) // 2, (size - ow + 1) // 2
    key = (size, oh, ow, fill, cls, K)
    if key not in _map_cache:
        if len(_map_cache) > 16:
            _map_cache.clear()
        d = conv_inputs((N, Pp, Qp, C, K, 1, 1, 0), cls, False, tag=1)
        d["ref"], d["b0"], _ = kr.conv_fwd(d["x"], d["w"], Pp, Qp, 1, 0, 0, residual=None if fill else d["res"])
        d["db"] = 0
        _map_cache[key] = d
    d = _map_cache[key]
    res_full = torch.full((N, size, size, K), 5.0)     # (the residual is read through the same map)
    sl = (slice(None), slice(oh, oh + 2 * (Pp - 1) + 1, 2), slice(ow, ow + 2 * (Qp - 1) + 1, 2))
    res_full[sl] = d["res"]
    y = Out((N, size, size, K), BF16, dev, pre=GUARD)
    om = OutMap(P=Pp, Q=Qp, stride=2, oh=oh, ow=ow)
    if fill and (2 * Pp < size or 2 * Qp < size):
        # an odd size with a phase other than 0: the last row / column is no sibling position of any pixel
        # of the phase grid, so the epilogue's zero stores cannot reach it -- both entry points refuse
        import pytest
        with pytest.raises(AssertionError, match="out_fill"):
            be.conv_fwd(bfx(d["x"]).to(dev), bfx(d["w"]).to(dev), y.t, ConvGeom(1, 0, 0), out_map=om, out_fill=True)
        assert y.untouched()
        return
    rc = launch_conv(be, dev, bfx(d["x"]).to(dev), bfx(d["w"]).to(dev), y.t, ConvGeom(1, 0, 0), cfg=cfg, out_fill=fill,
                     out_map=om, residual=None if fill else bfx(res_full).to(dev))
    assert rc == 0
    what = f"size {size} phase ({oh}, {ow}) fill {fill} {cls} cfg {cfg}"
    full = y.result()
    check_conv_out(full[sl].contiguous(), d, cls, 0, f"conv_fwd out_map y: {what}")
    rest = torch.ones(N, size, size, dtype=torch.bool)
    rest[sl] = False
    other = full[rest]
    want = torch.zeros_like(other) if fill else torch.full_like(other, SENT)
    assert _same_bits(other, want), f"conv_fwd out_map: {what}: the other phase positions were not left " \
                                    f"{'exactly 0' if fill else 'untouched'}"


# -- data gradient -------------------------------------------------------------------------------------
# name: (N, H, W, C, K, R, stride, pad) of the FORWARD conv whose input gradient is computed
DGRAD_CASES = {"3x3": (2, 9, 9, 64, 64, 3, 1, 1), "1x1": (2, 7, 7, 64, 128, 1, 1, 0),
               "3x3s2": (3, 9, 9, 32, 64, 3, 2, 1), "1x1s2": (2, 6, 6, 64, 64, 1, 2, 0),
               "nk-3x3": (2, 9, 9, 16, 16, 3, 1, 1), "nk-3x3s2": (2, 9, 9, 16, 32, 3, 2, 1)}


def dgrad_ref(dy, w, H, W, stride, pad):
    """dx[n,h,w,c] = sum_{p,q,k,r,s : p stride - pad + r = h, q stride - pad + s = w} dy[n,p,q,k] w[k,r,s,c],
    scattered term by term from the definition (no flipped weights, no dilation), and sum |terms|."""
    N, P, Q, K = dy.shape
    _, R, S, C = w.shape
    d, wd = dy.double().reshape(-1, K), w.double()
    ref = torch.zeros(N, H + 2 * R * stride, W + 2 * S * stride, C, dtype=torch.float64)   # (margins: cropped below)
    mag = torch.zeros_like(ref)
    o = R * stride
    for r in range(R):
        for s in range(S):
            h0, w0 = o - pad + r, o - pad + s
            sl = (slice(None), slice(h0, h0 + (P - 1) * stride + 1, stride), slice(w0, w0 + (Q - 1) * stride + 1, stride))
            ref[sl] += (d @ wd[:, r, s, :]).view(N, P, Q, C)
            mag[sl] += (d.abs() @ wd[:, r, s, :].abs()).view(N, P, Q, C)
    return ref[:, o:o + H, o:o + W], mag[:, o:o + H, o:o + W]


def run_dgrad(be, dev, name, cls, cfg=None):
    """dx = conv_fwd(dy, flipped and channel-transposed weights, dgrad_geom) against the gradient's
    own definition. Bound: at most R S K accumulation steps + 2, then the bf16 rounding."""
    N, H, W, C, K, R, s, p = DGRAD_CASES[name]
    P, Q = out_size(H, R, s), out_size(W, R, s)
    g = _seed(N, H, C, K, R, s, CONV_DATA.index(cls), 2)
    if cls == "int":
        dy = torch.randint(-3, 4, (N, P, Q, K), generator=g).float()
        w = torch.randint(-1, 2, (K, R, R, C), generator=g).float()
    else:
        dy = bf_round(torch.randn(N, P, Q, K, generator=g))
        w = bf_round(torch.randn(K, R, R, C, generator=g) * 0.1)
    ref, mag = dgrad_ref(dy, w, H, W, s, p)
    e = (R * R * K + 2) * kr.A23 * mag
    d = {"ref": ref, "b0": (1 + kr.BF) * e + kr.BF * ref.abs(), "db": 0}
    wt = w.flip(1, 2).permute(3, 1, 2, 0).contiguous()   # [C][R][S][K]
    dx = Out((N, H, W, C), BF16, dev, pre=GUARD)
    rc = launch_conv(be, dev, bfx(dy).to(dev), bfx(wt).to(dev), dx.t, dgrad_geom(ConvGeom(s, p, p), R, R), cfg=cfg)
    assert rc == 0
    check_conv_out(dx.result(), d, cls, 0, f"conv dgrad: {name} {cls} cfg {cfg}")


# -- weight gradient -----------------------------------------------------------------------------------
WGRAD_CASES = {
    "3x3": (2, 9, 9, 64, 64, 3, 1, 1),              # 162 pixels: partial pixel stage
    "3x3s2-odd": (3, 13, 13, 64, 128, 3, 2, 1),
    "1x1-c72-k200": (2, 9, 9, 72, 200, 1, 1, 0),    # 1x1 stride 1, partial k and output-channel tiles
    "k16": (2, 16, 16, 16, 16, 3, 1, 1),
    "k24": (2, 8, 8, 64, 24, 3, 1, 1),
    "stem-c8": (2, 16, 16, 8, 64, 7, 2, 3),
}
WGRAD_NS = [0, 2, 3, 4, 5, 6, 7, 8]
_wgrad_cache: dict = {}


def wgrad_case(name, cls, pro):
    key = (name, cls, pro)
    if key not in _wgrad_cache:
        if len(_wgrad_cache) > 8:
            _wgrad_cache.clear()
        N, H, W, C, K, R, s, p = WGRAD_CASES[name]
        d = conv_inputs((N, H, W, C, K, R, s, p), cls, pro, tag=3)
        g = _seed(N, H, C, K, R, 5, CONV_DATA.index(cls))
        d["dy"] = torch.randint(-3, 4, (N, d["P"], d["Q"], K), generator=g).float() if cls == "int" else \
            bf_round(torch.randn(N, d["P"], d["Q"], K, generator=g))
        if cls == "int":   # sums of M products of operands <= 7.5 and |dy| <= 3, multiples of 0.5
            assert 7.5 * 3 * N * d["P"] * d["Q"] < 2 ** 23
        d["ref"], b0 = kr.conv_wgrad(d["x"], d["dy"], R, R, s, p, p, in_bn=d["in_bn"])
        _, b1 = kr.conv_wgrad(d["x"], d["dy"], R, R, s, p, p, in_bn=d["in_bn"], partials=1)
        d["b0"], d["db"] = b0, b1 - b0
        d["geom"] = ConvGeom(s, p, p)
        _wgrad_cache[key] = d
    return _wgrad_cache[key]


def run_wgrad(be, dev, name, cls, pro, ns=None, split="slabs"):
    """dw (fp32, sentinel-prefilled; pre-zeroed for the atomic split-K) of one weight-gradient pipeline;
    split: "none" (the default split count: one split at these sizes), "slabs" (one split per 64-pixel step,
    partial slabs + drn_splitk_reduce), "atomic" (the same splits added into dw with fp32 atomics).
    Returns False when the library refuses the pipeline for this geometry."""
    d = wgrad_case(name, cls, pro)
    N, H, W, C, K, R, s, p = WGRAD_CASES[name]
    splits, atomic = 1, split == "atomic"
    dw = Out((K, R, R, C), torch.float32, dev, pre=GUARD, init=torch.zeros(K, R, R, C) if atomic else None)
    x, dy = bfx(d["x"]).to(dev), bfx(d["dy"]).to(dev)
    in_bn = None if d["in_bn"] is None else tuple(t.to(dev) for t in d["in_bn"])
    if not is_hip(be):
        be.conv_wgrad(x, dy, dw.t, d["geom"], in_bn=in_bn)
    else:
        tb, ms = (0, 0) if split == "none" else (4096, 1)
        nsp, _ = be.wgrad_splits(N * d["P"] * d["Q"], R * R * C, K, tb, ms)
        ws = Out((max(1, nsp * K * R * R * C),), torch.float32, dev, pre=GUARD)
        a = be.wgrad_args(x, dy, dw.t, d["geom"], in_bn=in_bn, ws=ws.t, target_blocks=tb, atomic=atomic, min_steps=ms)
        splits = a.splits
        assert a.splits == nsp and (split == "none" or a.splits > 1) and a.atomic_out == int(atomic)
        if be.L.drn_conv_wgrad2(ctypes.byref(a), be.zero_page.data_ptr(), ns, be.stream()) != 0:
            sync(dev)
            assert dw.untouched() and ws.untouched(), "a refused launch wrote memory"
            return False
        if a.splits > 1 and not a.atomic_out:
            from distributed_resnet_tensorflow_amd.ops import _lib
            _lib.check(be.L.drn_splitk_reduce(a.out, dw.t.data_ptr(), dw.t.numel(), a.splits, 1.0, 0, be.stream()),
                       "drn_splitk_reduce")
        sync(dev)
        ws.result()    # (guards of the slab workspace)
    got = dw.result()
    what = f"conv_wgrad: {name} {cls} pro {pro} ns {ns} split {split}"
    if cls == "int":
        ne = got != d["ref"].float()
        assert not bool(ne.any()), (f"{what}: {int(ne.sum())} of {ne.numel()} elements differ from the exact sum, "
                                    f"first at {ne.nonzero()[0].tolist()}")
    else:
        assert_within(got, d["ref"], d["b0"] + splits * d["db"], what)
    return True


# -- bn_stats / bn_bwd_reduce --------------------------------------------------------------------------
BN_RED_SHAPES = [(37, 8), (1000, 8), (131, 16), (77, 24), (301, 64), (600, 64), (53, 2048)]   # (M, C)


def _bn_params(C, g):
    return (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1,
            torch.rand(C, generator=g) + 0.5)


def run_bn_stats(be, dev, M, C, reps):
    g = _seed(M, C, 11)
    x = bf_round(torch.randn(M, C, generator=g) * 2 + 0.5)
    # (one more row of large values behind the input: a loop that runs one row too far sums it)
    xbuf = torch.cat([x, torch.full((1, C), 1000.0)]).to(dev, BF16)
    part = Out((reps, 2, C), torch.float32, dev, init=torch.zeros(reps, 2, C), pre=GUARD)
    be.bn_stats(xbuf[:M], part.t)
    sync(dev)
    v = x.double()
    ref, bound = kr.channel_sums(v, v * v, reps, 4)
    assert_within(part.result().double().sum(0), ref, bound, f"bn_stats: M {M} C {C} replicas {reps}")


def run_bn_bwd_reduce(be, dev, M, C, reps, pool, relu=True):
    """pool: dy is dpool[n][c] / HW broadcast over HW = 7 rows (M a multiple of 7 is not required of
    the kernel's row loop: the last image is then partial, so M is rounded up here)."""
    hw = 7
    if pool:
        M = -(-M // hw) * hw
    g = _seed(M, C, 12, int(pool))
    x = bf_round(torch.randn(M, C, generator=g))
    sc, sh, mu, isd = _bn_params(C, g)
    if pool:
        dpool = torch.randn(M // hw, C, generator=g)
        inv = float(np.float32(1.0) / np.float32(hw))
        dy = (dpool.double() * inv).repeat_interleave(hw, 0)      # (one more rounding: c + 2)
    else:
        dyb = bf_round(torch.randn(M, C, generator=g))
        dy = dyb.double()
    mask, amb = kr.relu_mask(x, sc, sh)
    assert amb == 0, "a ReLU mask is ambiguous in fp32 (choose another seed)"
    gm = torch.where(mask, dy, torch.zeros_like(dy)) if relu else dy
    part = Out((reps, 2, C), torch.float32, dev, init=torch.zeros(reps, 2, C), pre=GUARD)
    xs = x.view(M // hw, hw, 1, C) if pool else x
    be.bn_bwd_reduce(None if pool else dyb.to(dev, BF16), dpool.to(dev) if pool else None, hw if pool else 0,
                     xs.to(dev, BF16), sc.to(dev), sh.to(dev), mu.to(dev), isd.to(dev), part.t, relu=relu)
    sync(dev)
    ref, bound = kr.bn_bwd_sums(gm, x, mu, isd, reps, c=10 if pool else 8)
    assert_within(part.result().double().sum(0), ref, bound, f"bn_bwd_reduce: M {M} C {C} replicas {reps} pool {pool}")


# -- finalize ------------------------------------------------------------------------------------------
FIN_G = [1, 3, 4, 5, 8]
FIN_COUNTS = [1, 2, 98]


def fin_parts(C, G, count, g):
    """[G][2][C] statistics of `count` rows whose channel means / deviations reach 4, split UNEQUALLY over
    the replicas (some negative); channel 0 is constant (variance exactly 0), channel 1 is constant at a
    value whose fp32 sums make q / n - mean^2 come out negative (the clamp)."""
    rows = torch.randn(count, C, generator=g) * (torch.rand(C, generator=g) * 4) + torch.randn(C, generator=g) * 4
    rows[:, 0] = 3.0
    rows[:, 1] = 1.1
    rows = bf_round(rows).double()
    tot = torch.stack([rows.sum(0), (rows * rows).sum(0)])
    wgt = torch.randn(G, 1, 1, generator=g).double()
    wgt[-1] += 1 - wgt.sum()
    return (tot.unsqueeze(0) * wgt).float().contiguous()


def _check_named(outs, refs, names, what):
    for k in names:
        assert_within(outs[k].result() if isinstance(outs[k], Out) else outs[k], refs[k][0], refs[k][1], f"{what} {k}")


def run_bn_finalize(be, dev, C, G, count, running):
    g = _seed(C, G, count, 13)
    parts = fin_parts(C, G, count, g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    o = {k: Out((C,), torch.float32, dev, pre=GUARD) for k in ("scale", "shift", "mean", "invstd")}
    o["run_mean"], o["run_var"] = Out((C,), torch.float32, dev, init=rm0, pre=GUARD), Out((C,), torch.float32, dev, init=rv0, pre=GUARD)
    be.bn_finalize(parts.to(dev).clone(), G, count, gamma.to(dev), beta.to(dev), o["run_mean"].t, o["run_var"].t, o["scale"].t,
                   o["shift"].t, o["mean"].t, o["invstd"].t, 0.997, 1e-5, update_running=running)
    sync(dev)
    refs = kr.bn_finalize_fwd(parts, count, gamma, beta, 1e-5, 0.997, rm0, rv0, fp32_math=False)
    names = ["scale", "shift", "mean", "invstd"] + (["run_mean", "run_var"] if running else [])
    _check_named(o, refs, names, f"bn_finalize: C {C} G {G} count {count}")
    if not running:
        assert o["run_mean"].untouched() and o["run_var"].untouched()


def run_bn_finalize_bwd(be, dev, C, G, count):
    g = _seed(C, G, count, 14)
    parts = (torch.randn(G, 2, C, generator=g) * count ** 0.5).contiguous()
    gamma, isd = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    o = {"dgamma": Out((C,), torch.float32, dev, pre=GUARD), "dbeta": Out((C,), torch.float32, dev, pre=GUARD),
         "coef": Out((3, C), torch.float32, dev, pre=GUARD)}
    be.bn_finalize_bwd(parts.to(dev).clone(), G, count, gamma.to(dev), isd.to(dev), o["dgamma"].t, o["dbeta"].t, o["coef"].t)
    sync(dev)
    refs = kr.bn_finalize_bwd(parts, count, gamma, isd)
    _check_named(o, refs, ["dgamma", "dbeta", "coef"], f"bn_finalize_bwd: C {C} G {G} count {count}")


# -- bn_apply / bn_apply_fin ---------------------------------------------------------------------------
# (M, C): C / 8 = 3 and 9 take the generic path
BN_APPLY_SHAPES = {"c16": (101, 16), "c24": (101, 24), "c72": (35, 72), "c256": (19, 256)}
BN_APPLY_CAPPED = (6145, 2048)     # nvec = 3 * (2048 * 256) + 256: 256 threads run the two-in-flight loop twice, the rest the tail


def run_bn_apply(be, dev, M, C, relu, fin=None):
    """fin: None = bn_apply with given scale / shift; G = bn_apply_fin deriving them from G replicas,
    publishing: the published values against fp64 first, then y from the published fp32 values."""
    g = _seed(M, C, 15)
    x = bf_round(torch.randn(M, C, generator=g) * 1.5 + 0.3)
    x[::5, : 8] = 0
    y = Out((M, C), BF16, dev, pre=GUARD)
    what = f"M {M} C {C} relu {relu} fin {fin}"
    if fin is None:
        sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        be.bn_apply(x.to(dev, BF16), y.t, sc.to(dev), sh.to(dev), relu=relu)
        sync(dev)
    else:
        parts = fin_parts(C, fin, M, g)
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
        rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        o = {k: Out((C,), torch.float32, dev, pre=GUARD) for k in ("scale", "shift", "mean", "invstd")}
        o["run_mean"], o["run_var"] = Out((C,), torch.float32, dev, init=rm0, pre=GUARD), Out((C,), torch.float32, dev, init=rv0, pre=GUARD)
        f = BnCfin(parts.to(dev).clone(), float(M), gamma.to(dev), beta=beta.to(dev), run_mean=o["run_mean"].t, run_var=o["run_var"].t,
                   scale=o["scale"].t, shift=o["shift"].t, mean=o["mean"].t, invstd=o["invstd"].t, publish=True)
        be.bn_apply_fin(x.to(dev, BF16), y.t, f, relu=relu)
        sync(dev)
        fp32 = is_hip(be) and C < be.BN_FIN_SPLIT_C     # (at and above it: the standalone double-precision finalize)
        refs = kr.bn_finalize_fwd(parts, M, gamma, beta, 1e-5, 0.997, rm0, rv0, fp32_math=fp32)
        _check_named(o, refs, ["scale", "shift", "mean", "invstd", "run_mean", "run_var"], f"bn_apply_fin: {what}")
        sc, sh = o["scale"].result(), o["shift"].result()
    ref, bound = kr.bn_apply(x, sc, sh, relu)
    assert_within(y.result(), ref, bound, f"bn_apply{'_fin' if fin else ''} y: {what}")


# -- bn_bwd_apply / bn_bwd_apply_fin --------------------------------------------------------------------
# (M, C): 1024 workgroups x 256 threads x 4 vectors = 1048576 vectors per round of batches; the smallest M with
# a second batch per thread that is partial (most of its slots clamped): nvec = M C / 8 a little above one round
BN_BWD_APPLY_SHAPES = {"c128": (73745, 128), "c1024": (9001, 1024), "small-c16": (203, 16), "mid-c64": (3001, 64)}


def run_bn_bwd_apply(be, dev, name, fin, add, pool):
    M, C = BN_BWD_APPLY_SHAPES[name]
    hw = 7
    if pool:
        M = -(-M // hw) * hw
    g = _seed(M, C, 16, int(pool))
    x = bf_round(torch.randn(M, C, generator=g) * 1.5 + 0.2)
    sc, sh, mu, isd = _bn_params(C, g)
    gamma = torch.rand(C, generator=g) + 0.5
    bst = (torch.randn(3, 2, C, generator=g) * M ** 0.5).contiguous()
    addt = bf_round(torch.randn(M, C, generator=g)) if add else None
    if pool:
        dpool = torch.randn(M // hw, C, generator=g)
        dy = (dpool.double() * float(np.float32(1.0) / np.float32(hw))).repeat_interleave(hw, 0)
    else:
        dyb = bf_round(torch.randn(M, C, generator=g))
        dy = dyb.double()
    mask, amb = kr.relu_mask(x, sc, sh)
    assert amb == 0, "a ReLU mask is ambiguous in fp32 (choose another seed)"
    gm = torch.where(mask, dy, torch.zeros_like(dy))
    dx = Out((M, C), BF16, dev, pre=GUARD, sentinel=float("nan"))
    xs = (x.view(M // hw, hw, 1, C) if pool else x).to(dev, BF16)
    dxs = dx.t.view(xs.shape)
    args = (None if pool else dyb.to(dev, BF16), dpool.to(dev) if pool else None, hw if pool else 0, xs, sc.to(dev), sh.to(dev))
    addd = None if addt is None else addt.to(dev, BF16).view(xs.shape)
    what = f"{name} fin {fin} add {add} pool {pool}"
    if fin:
        dg, db = Out((C,), torch.float32, dev, pre=GUARD), Out((C,), torch.float32, dev, pre=GUARD)
        f = BnCfin(bst.to(dev).clone(), float(M), gamma.to(dev), mean=mu.to(dev), invstd=isd.to(dev), dgamma=dg.t, dbeta=db.t, publish=True)
        be.bn_bwd_apply_fin(*args, f, addd, dxs, relu=True)
        sync(dev)
        refs = kr.bn_finalize_bwd(bst, M, gamma, isd)
        _check_named({"dgamma": dg, "dbeta": db}, refs, ["dgamma", "dbeta"], f"bn_bwd_apply_fin: {what}")
        n = float(np.float32(M))
        k1, k2, k3 = gamma.double() * isd.double(), db.result().double() / n, dg.result().double() / n
        cr = (1, 4, 4, 6)
    else:
        k1, k2, k3 = gamma * isd, bst[:, 0].sum(0) / M, bst[:, 1].sum(0) / M
        be.bn_bwd_apply(*args, mu.to(dev), isd.to(dev), torch.cat([k1, k2, k3]).to(dev), addd, dxs, relu=True)
        sync(dev)
        cr = (0, 2, 2, 4)
    ref, bound = kr.bn_bwd_apply(gm, x, k1, k2, k3, mu, isd, addt, cr)
    if pool:   # dpool * fl(1 / HW): one more rounding of g
        bound = bound + (1 + kr.BF) * kr.U * (k1.double() * gm).abs()
    got = dx.result()
    assert bool(torch.isfinite(got.float()).all()), f"bn_bwd_apply: {what}: an element was not written"
    assert_within(got, ref, bound, f"bn_bwd_apply{'_fin' if fin else ''} dx: {what}")


# -- bn_apply_stats / bn_bwd_apply_stats (the finalize fused into the apply, one [2][C] accumulator) --------------
def run_bn_apply_stats(be, dev, M, C, relu):
    """Published scale / shift / mean / invstd / moving averages against fp64 (fp32 math on the HIP side:
    bn_stats_to_affine), then y from the published fp32 values; the accumulator is left unchanged."""
    g = _seed(M, C, 17)
    x = bf_round(torch.randn(M, C, generator=g) * 1.5 + 0.3)
    parts = fin_parts(C, 1, M, g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    o = {k: Out((C,), torch.float32, dev, pre=GUARD) for k in ("scale", "shift", "mean", "invstd")}
    o["run_mean"] = Out((C,), torch.float32, dev, init=rm0, pre=GUARD)
    o["run_var"] = Out((C,), torch.float32, dev, init=rv0, pre=GUARD)
    acc = Out((2, C), torch.float32, dev, init=parts[0], pre=GUARD)
    y = Out((M, C), BF16, dev, pre=GUARD)
    be.bn_apply_stats(x.to(dev, BF16), y.t, acc.t, M, gamma.to(dev), beta.to(dev), o["run_mean"].t, o["run_var"].t,
                      o["scale"].t, o["shift"].t, o["mean"].t, o["invstd"].t, 0.997, 1e-5, relu=relu)
    sync(dev)
    what = f"M {M} C {C} relu {relu}"
    assert acc.untouched(), "the accumulator must be left unchanged"
    refs = kr.bn_finalize_fwd(parts, M, gamma, beta, 1e-5, 0.997, rm0, rv0, fp32_math=is_hip(be))
    _check_named(o, refs, ["scale", "shift", "mean", "invstd", "run_mean", "run_var"], f"bn_apply_stats: {what}")
    ref, bound = kr.bn_apply(x, o["scale"].result(), o["shift"].result(), relu)
    assert_within(y.result(), ref, bound, f"bn_apply_stats y: {what}")


def run_bn_bwd_apply_stats(be, dev, M, C, add, pool):
    hw = 7
    if pool:
        M = -(-M // hw) * hw
    g = _seed(M, C, 18, int(pool))
    x = bf_round(torch.randn(M, C, generator=g) * 1.5 + 0.2)
    sc, sh, mu, isd = _bn_params(C, g)
    gamma = torch.rand(C, generator=g) + 0.5
    accv = torch.randn(2, C, generator=g) * M ** 0.5
    addt = bf_round(torch.randn(M, C, generator=g)) if add else None
    if pool:
        dpool = torch.randn(M // hw, C, generator=g)
        dy = (dpool.double() * float(np.float32(1.0) / np.float32(hw))).repeat_interleave(hw, 0)
    else:
        dyb = bf_round(torch.randn(M, C, generator=g))
        dy = dyb.double()
    mask, amb = kr.relu_mask(x, sc, sh)
    assert amb == 0, "a ReLU mask is ambiguous in fp32 (choose another seed)"
    gm = torch.where(mask, dy, torch.zeros_like(dy))
    acc = Out((2, C), torch.float32, dev, init=accv, pre=GUARD)
    dg, db = Out((C,), torch.float32, dev, pre=GUARD), Out((C,), torch.float32, dev, pre=GUARD)
    coef = Out((3 * C,), torch.float32, dev, pre=GUARD)
    dx = Out((M, C), BF16, dev, pre=GUARD, sentinel=float("nan"))
    xs = (x.view(M // hw, hw, 1, C) if pool else x).to(dev, BF16)
    be.bn_bwd_apply_stats(None if pool else dyb.to(dev, BF16), dpool.to(dev) if pool else None, hw if pool else 0, xs,
                          sc.to(dev), sh.to(dev), mu.to(dev), isd.to(dev), acc.t, M, gamma.to(dev), dg.t, db.t,
                          None if addt is None else addt.to(dev, BF16).view(xs.shape), dx.t.view(xs.shape), coef.t,
                          relu=True)
    sync(dev)
    what = f"M {M} C {C} add {add} pool {pool}"
    assert acc.untouched(), "the accumulator must be left unchanged"
    assert _same_bits(db.result(), accv[0]) and _same_bits(dg.result(), accv[1]), "dbeta / dgamma are the sums themselves"
    ref, bound = kr.bn_bwd_apply_nested(gm, x, gamma, isd, mu, accv[0], accv[1], M, addt)
    if pool:   # dpool * fl(1 / HW): one more rounding of g
        bound = bound + (1 + kr.BF) * kr.U * (gamma.double() * isd.double() * gm).abs()
    got = dx.result()
    assert bool(torch.isfinite(got.float()).all()), f"bn_bwd_apply_stats: {what}: an element was not written"
    assert_within(got, ref, bound, f"bn_bwd_apply_stats dx: {what}")


# -- the finalize inside the conv: epilogue (bn_fin, bn_fin_column) and prologue (in_fin) ----------------------------
def run_conv_bn_fin(be, dev, name, bwd, cfg=None):
    """The last-arriving workgroup of each channel column finalizes the BN of the conv's output (forward) or
    its backward sums (with the BN-backward epilogue). y and the statistics are checked as in run_conv_fwd; the
    published values against fp64 from the replicas the kernel left; the arrival counters are re-armed."""
    d = conv_case(name, "randn", False, True, bwd)
    N, H, W, C, K, R, s, p = CONV_CASES[name]
    M = N * d["P"] * d["Q"]
    g = _seed(K, M, 19, int(bwd))
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2
    rm0, rv0 = torch.randn(K, generator=g) * 0.1, torch.rand(K, generator=g) + 0.5
    y = Out((N, d["P"], d["Q"], K), BF16, dev, pre=GUARD)
    st = Out((NREP, 2, K), torch.float32, dev, init=torch.zeros(NREP, 2, K), pre=GUARD)
    cnt = Out((64,), torch.int32, dev, init=torch.zeros(64, dtype=torch.int32), pre=GUARD, sentinel=77)
    names = ["dgamma", "dbeta"] if bwd else ["scale", "shift", "mean", "invstd", "run_mean", "run_var"]
    o = {k: Out((K,), torch.float32, dev, pre=GUARD) for k in names}
    kw = dict(residual=bfx(d["res"]).to(dev), stats=st.t)
    if bwd:
        o["coef"] = Out((3, K), torch.float32, dev, pre=GUARD)
        xb, sc, sh, mu, isd = d["bn_bwd"]
        kw["bn_bwd"] = (bfx(xb).to(dev),) + tuple(t.to(dev) for t in (sc, sh, mu, isd))
        kw["bn_fin"] = BnFin(cnt.t, float(M), gamma.to(dev), dgamma=o["dgamma"].t, dbeta=o["dbeta"].t, coef=o["coef"].t.view(-1))
    else:
        o["run_mean"], o["run_var"] = (Out((K,), torch.float32, dev, init=t, pre=GUARD) for t in (rm0, rv0))
        kw["bn_fin"] = BnFin(cnt.t, float(M), gamma.to(dev), beta=beta.to(dev), run_mean=o["run_mean"].t,
                             run_var=o["run_var"].t, scale=o["scale"].t, shift=o["shift"].t, mean=o["mean"].t,
                             invstd=o["invstd"].t)
    rc = launch_conv(be, dev, bfx(d["x"]).to(dev), bfx(d["w"]).to(dev), y.t, d["geom"], cfg=cfg, **kw)
    assert rc == 0
    what = f"{name} bwd {bwd} cfg {cfg}"
    got = y.result()
    check_conv_out(got, d, "randn", 0, f"conv_fwd bn_fin y: {what}")
    assert _same_bits(cnt.result(), torch.zeros(64, dtype=torch.int32)), "an arrival counter was not re-armed"
    if is_hip(be):
        check_conv_stats(st, got, d, bwd, f"conv_fwd bn_fin stats: {what}")
        parts, e_parts = st.result(), None
    else:   # (the CPU finalize clears its accumulator: the sums are those of the stored output, with their bound)
        sums, e_parts = kr.bn_bwd_sums(got, d["bn_bwd"][0], d["bn_bwd"][3], d["bn_bwd"][4], 1) if bwd else kr.conv_stats(got, 1)
        parts = sums.unsqueeze(0)
    if bwd:
        refs = kr.bn_finalize_bwd(parts, M, gamma, d["bn_bwd"][4], e_parts=e_parts)
        _check_named(o, refs, ["dgamma", "dbeta", "coef"], f"conv bn_fin bwd: {what}")
    else:
        refs = kr.bn_finalize_fwd(parts, M, gamma, beta, 1e-5, 0.997, rm0, rv0, fp32_math=False, e_parts=e_parts)
        _check_named(o, refs, names, f"conv bn_fin fwd: {what}")


def run_conv_in_fin(be, dev, name, G, cfg=None):
    """The fused prologue finalizes its input BN from G statistics replicas (BnCfin). Publishing: the published
    values against fp64, y against the conv of the PUBLISHED scale / shift. Not publishing (a second launch
    reading the published scale / shift where the kernel does not derive them): nothing but y is written,
    and y is the same bits."""
    N, H, W, C, K, R, s, p = CONV_CASES[name]
    d = conv_inputs(CONV_CASES[name], "randn", False, tag=4)
    g = _seed(C, G, 20)
    M_in = N * H * W
    parts = fin_parts(C, G, M_in, g)
    parts[:, :, :2] = parts[:, :, 2:4]      # (no constant channel here: its scale of ~300 only inflates the bound)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    names = ["scale", "shift", "mean", "invstd", "run_mean", "run_var"]
    x, w = bfx(d["x"]).to(dev), bfx(d["w"]).to(dev)
    ys = []
    pub_vals = None
    for publish in (True, False):
        o = {k: Out((C,), torch.float32, dev, pre=GUARD, init=None if pub_vals is None else pub_vals[k]) for k in names}
        if publish:
            o["run_mean"], o["run_var"] = (Out((C,), torch.float32, dev, init=t, pre=GUARD) for t in (rm0, rv0))
        fin = BnCfin(parts.to(dev).clone(), float(M_in), gamma.to(dev), beta=beta.to(dev), run_mean=o["run_mean"].t,
                     run_var=o["run_var"].t, scale=o["scale"].t, shift=o["shift"].t, mean=o["mean"].t,
                     invstd=o["invstd"].t, publish=publish)
        y = Out((N, d["P"], d["Q"], K), BF16, dev, pre=GUARD)
        rc = launch_conv(be, dev, x, w, y.t, ConvGeom(s, p, p), cfg=cfg, in_bn=(o["scale"].t, o["shift"].t), in_fin=fin)
        assert rc == 0
        what = f"{name} G {G} cfg {cfg} publish {publish}"
        if publish:
            refs = kr.bn_finalize_fwd(parts, M_in, gamma, beta, 1e-5, 0.997, rm0, rv0, fp32_math=is_hip(be))
            _check_named(o, refs, names, f"conv in_fin: {what}")
            pub_vals = {k: o[k].result().clone() for k in names}
            ref, bound, _ = kr.conv_fwd(d["x"], d["w"], d["P"], d["Q"], s, p, p, in_bn=(pub_vals["scale"], pub_vals["shift"]))
        else:
            assert all(o[k].untouched() for k in names), "a non-publishing launch wrote BN parameters"
        got = y.result()
        assert_within(got, ref, bound, f"conv in_fin y: {what}")
        ys.append(got)
    assert _same_bits(ys[0], ys[1]), "publishing and non-publishing launches differ"


# -- packed stem weight gradient -------------------------------------------------------------------------------
STEM_WGRAD_NS = [2, 3, 4, 5, 6, 9, 10]


def run_stem_wgrad(be, dev, cls, ns):
    """The 7x7 / 2 stem's weight gradient on the packed layout (4-channel, column-padded images, tap-pair
    weights), mapped back by stem_unpack_grad to [K][7][7][8]: channels 0..3 against the definition (bitwise
    in the int class), the padding channels 4..7 exactly 0. HIP only: the packed layout is the kernels' own."""
    N, H, K, R = 2, 16, 64, 7
    P = out_size(H, R, 2)
    assert P % 2 == 0     # (the input-halo kernels 9 / 10 take half output rows)
    g = _seed(N, H, K, 21, CONV_DATA.index(cls))
    x = torch.zeros(N, H, H, 8)
    if cls == "int":
        x[..., :3] = torch.randint(-3, 4, (N, H, H, 3), generator=g).float()
        dy = torch.randint(-3, 4, (N, P, P, K), generator=g).float()
    else:
        x[..., :3] = bf_round(torch.randn(N, H, H, 3, generator=g))
        dy = bf_round(torch.randn(N, P, P, K, generator=g))
    ref, bound = kr.conv_wgrad(x, dy, R, R, 2, 3, 3, partials=8)
    n_xp = N * H * (H + 2) * 4
    buf = torch.zeros(n_xp + 64, dtype=BF16, device=dev)
    xp = buf[:n_xp].view(N, H, H + 2, 4)
    be.stem_pack_input(bfx(x).to(dev), xp)
    ws = Out((max(1, be.wgrad_ws_elems(N * P * P, K, R, 8, 4)),), torch.float32, dev, pre=GUARD)
    dw4 = Out((K, R, 8, 4), torch.float32, dev, pre=GUARD)
    dw = Out((K, R, R, 8), torch.float32, dev, pre=GUARD)
    old = be.forced_wgrad_ns
    be.forced_wgrad_ns = ns
    try:
        be.conv_wgrad(xp, bfx(dy).to(dev), dw4.t, ConvGeom(stride=2, pad_h=3, pad_w=2), ws=ws.t)
    finally:
        be.forced_wgrad_ns = old
    be.stem_unpack_grad(dw4.t, dw.t)
    sync(dev)
    ws.result(), dw4.result()
    got = dw.result()
    assert bool((got[..., 4:] == 0).all()), "padding channels must be exactly 0"
    what = f"conv_wgrad packed stem: {cls} ns {ns}"
    if cls == "int":
        ne = got[..., :4] != ref[..., :4].float()
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} elements differ from the exact sum, first at {ne.nonzero()[0].tolist()}"
    else:
        assert_within(got[..., :4], ref[..., :4], bound[..., :4], what)


# -- stride-2 data gradient by phases ----------------------------------------------------------------------------
def dgrad_phases(w, in_hw, stride, pad):
    """The phase decomposition of a stride-`stride` data gradient as the step plan builds it (runtime/executor.py
    _conv_op): output parity (ph, pw) sees the taps r = ph + pad (mod stride) only. Yields
    (weights [C][Ru][Sv][K], geometry, out_map)."""
    K, R, _, C = w.shape
    for ph in range(stride):
        rs = [r for r in range(R) if (r - ph - pad) % stride == 0]
        for pw in range(stride):
            ss = [q for q in range(R) if (q - pw - pad) % stride == 0]
            Hph, Wph = (in_hw - ph + stride - 1) // stride, (in_hw - pw + stride - 1) // stride
            if not rs or not ss or Hph <= 0 or Wph <= 0:
                continue
            r0, s0 = max(rs), max(ss)
            rsel, ssel = [r0 - stride * u for u in range(len(rs))], [s0 - stride * v for v in range(len(ss))]
            wt = w[:, rsel][:, :, ssel].permute(3, 1, 2, 0).contiguous()
            yield wt, ConvGeom(1, -((ph + pad - r0) // stride), -((pw + pad - s0) // stride), 1), OutMap(Hph, Wph, stride, ph, pw)


def run_dgrad_phases(be, dev, name, cls, cfg=None):
    """The assembled dx of the phase launches against the gradient's own definition (dgrad_ref); positions no
    phase writes (1x1 stride 2: the odd ones) keep the sentinel here -- the executor clears or out_fills them."""
    N, H, W, C, K, R, s, p = DGRAD_CASES[name]
    P = out_size(H, R, s)
    g = _seed(N, H, C, K, R, s, CONV_DATA.index(cls), 2)
    if cls == "int":
        dy = torch.randint(-3, 4, (N, P, P, K), generator=g).float()
        w = torch.randint(-1, 2, (K, R, R, C), generator=g).float()
    else:
        dy = bf_round(torch.randn(N, P, P, K, generator=g))
        w = bf_round(torch.randn(K, R, R, C, generator=g) * 0.1)
    ref, mag = dgrad_ref(dy, w, H, W, s, p)
    e = (R * R * K + 2) * kr.A23 * mag
    d = {"ref": ref, "b0": (1 + kr.BF) * e + kr.BF * ref.abs(), "db": 0}
    dx = Out((N, H, W, C), BF16, dev, pre=GUARD)
    written = torch.zeros(H, W, dtype=torch.bool)
    for wt, geom, om in dgrad_phases(w, H, s, p):
        assert launch_conv(be, dev, bfx(dy).to(dev), bfx(wt).to(dev), dx.t, geom, cfg=cfg, out_map=om) == 0
        written[om.oh::s, om.ow::s] = True
    got = dx.result()
    what = f"conv dgrad phases: {name} {cls} cfg {cfg}"
    assert bool(written.any()) and _same_bits(got[:, ~written], torch.full_like(got[:, ~written], SENT)), what
    assert float(ref[:, ~written].abs().max()) == 0 if bool((~written).any()) else True
    sub = {k: (v[:, written] if torch.is_tensor(v) else v) for k, v in d.items()}
    check_conv_out(got[:, written], sub, cls, 0, what)
