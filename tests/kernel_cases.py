"""The case lists of the auxiliary-kernel tests and one driver per operation. A driver takes a
backend and its device, builds the inputs, calls the backend's entry point on sentinel-prefilled
output buffers with guard elements, and checks the result element by element against
tests/kernel_refs.py. tests/test_aux_kernels_gpu.py runs them on HipBackend (the HIP kernels),
tests/test_kernel_refs.py on RefBackend (the CPU training path): the same cases, the same bounds.
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
