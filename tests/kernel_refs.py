"""Independent fp64 references of the head, pooling, optimizer and input kernels and (second half) of the
convolution and BatchNorm kernels, written directly
with torch and numpy from each operation's definition (RefBackend is not used here: it is one of
the two implementations under test), and the one comparison helper, assert_within.

Every reference returns the exact result in fp64 together with a per-element bound that is derived
from the operation and computed in fp64 from the inputs:

  * an fp32 sum of n terms / a length-K dot product, in ANY summation order:
        (n + c) * 2^-24 * sum |terms|        (c: the roundings outside the sum, counted per op below)
  * a value rounded to bf16 at the end:  + 2^-8 * |ref|   (half a bf16 ulp plus the double rounding)
  * integers, maxima of bf16 values, hashes, casts, fills and untouched memory: torch.equal.
  * an MFMA-accumulated dot product: 2^-23 per step (the matrix unit's adder may truncate), see conv_fwd.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24      # fp32 unit roundoff
BF = 2.0 ** -8      # bf16 unit roundoff (half an ulp, relative)
S = 8192 * 256      # threads of the capped grid of the flat element-wise kernels (8192 blocks x 256)

# worst error / bound seen per label prefix (the text before ':' of `what`), for the record
RATIOS: dict = {}


def assert_within(actual, ref64, bound64, what):
    """|actual - ref| <= bound element by element (a NaN or inf in `actual` is an offender)."""
    a = actual.detach().cpu().to(torch.float64)
    r = torch.as_tensor(ref64, dtype=torch.float64)
    b = torch.as_tensor(bound64, dtype=torch.float64).expand_as(r)
    assert a.shape == r.shape, (what, tuple(a.shape), tuple(r.shape))
    err = (a - r).abs()
    bad = ~(err <= b)
    ratio = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, np.inf)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = what.split(":")[0]
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst if worst == worst else np.inf)
    print(f"[within] {what}: worst error / bound = {worst:.3e} over {a.numel()} elements")
    if bool(bad.any()):
        over = torch.where(bad, torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, np.inf)),
                           torch.full_like(ratio, -1.0))
        idx = np.unravel_index(int(over.argmax()), tuple(a.shape)) if a.dim() else ()
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.numel()} elements outside the bound; worst at "
                             f"{tuple(int(i) for i in idx)}: actual {a[idx].item()!r}, reference {r[idx].item()!r}, "
                             f"error {err[idx].item():.6e}, bound {b[idx].item():.6e}")


def f32(v: float) -> float:
    """The fp32 value a float kernel argument arrives as."""
    return float(np.float32(v))


# -- dense layer --------------------------------------------------------------------------------------
def sgemm_splits(M, N, K, target_wg):
    """HipBackend.sgemm's split-K factor."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    return max(1, min(K // 128, target_wg // max(tiles, 1)))


def sgemm(ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C0, ldc, bias, splits):
    """C = alpha op(A) op(B) + beta C0 + bias on flat row-major buffers with leading dimensions."""
    a = A.double().reshape(-1)[: (K if ta else M) * lda].view(-1, lda)
    a = a[:, :M].t() if ta else a[:, :K]
    b = B.double().reshape(-1)[: (N if tb else K) * ldb].view(-1, ldb)
    b = b[:, :K].t() if tb else b[:, :N]
    c0 = C0.double().reshape(-1)[: M * ldc].view(M, ldc)[:, :N]
    al, be = f32(alpha), f32(beta)
    ref = al * (a @ b)
    mag = abs(al) * (a.abs() @ b.abs())
    if beta != 0:
        ref = ref + be * c0
        mag = mag + (be * c0).abs()
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    return ref, (K + splits + 4) * U * mag


def colsum(x, scale, accumulate, out0):
    """out = [out0 +] scale * sum_rows x: rows terms, then the scaling and the accumulate (c = 4)."""
    sc = f32(scale)
    ref = sc * x.double().sum(0)
    mag = abs(sc) * x.double().abs().sum(0)
    if accumulate:
        ref = ref + out0.double()
        mag = mag + out0.double().abs()
    return ref, (x.shape[0] + 4) * U * mag


def pool_bnrelu(x, scale, shift, relu):
    """pooled[n][c] = mean_hw act(x * scale + shift): HW terms of two roundings each, the rounded
    1 / HW and the final product (c = 6); |act(v)| <= |x scale| + |shift|."""
    N, H, W, C = x.shape
    v = x.double()
    mag = v.abs()
    if scale is not None:
        v = v * scale.double() + shift.double()
        mag = mag * scale.double().abs() + shift.double().abs()
    if relu:
        v = v.clamp_min(0)
    return v.mean(dim=(1, 2)), (H * W + 6) * U * mag.sum(dim=(1, 2)) / (H * W)


# -- max-pool -----------------------------------------------------------------------------------------
def pool_out(H, k, stride, pad):
    """Output size: TF 'SAME' (ceil(H / stride), the window may hang over the far edge) when pad == 0,
    else the symmetric-pad floor rule."""
    return -(-H // stride) if pad == 0 else (H + 2 * pad - k) // stride + 1


def _windows(x, k, stride, pad_h, pad_w, P, Q):
    """x [N,H,W,C] -> the explicit -inf padded taps [k*k][N,P,Q,C] in row-major tap order."""
    N, H, W, C = x.shape
    xc = x.double().permute(0, 3, 1, 2)
    pb, pr = (P - 1) * stride + k - pad_h - H, (Q - 1) * stride + k - pad_w - W
    xp = F.pad(xc, (pad_w, max(pr, 0), pad_h, max(pb, 0)), value=float("-inf"))
    taps = []
    for r in range(k):
        for t in range(k):
            taps.append(xp[:, :, r:r + (P - 1) * stride + 1:stride, t:t + (Q - 1) * stride + 1:stride]
                        .permute(0, 2, 3, 1))
    return xp, taps


def maxpool_fwd(x, k, stride, pad_h, pad_w):
    """y = F.max_pool2d of the explicitly -inf padded input; arg = the FIRST tap (row-major) holding
    the maximum, found by a strict-greater scan (no argmax); nmax = how many taps hold it."""
    N, H, W, C = x.shape
    P, Q = pool_out(H, k, stride, pad_h), pool_out(W, k, stride, pad_w)
    xp, taps = _windows(x, k, stride, pad_h, pad_w, P, Q)
    y = F.max_pool2d(xp, k, stride)[:, :, :P, :Q].permute(0, 2, 3, 1).contiguous()
    best = torch.full_like(taps[0], float("-inf"))
    arg = torch.zeros(taps[0].shape, dtype=torch.uint8)
    for i, t in enumerate(taps):
        win = t > best
        best = torch.where(win, t, best)
        arg = torch.where(win, torch.full_like(arg, i), arg)
    assert torch.equal(best, y)
    nmax = sum((t == y).to(torch.int32) for t in taps)
    return y, arg, nmax


def pool_stats(y):
    """Per-channel (sum, sum of squares) of y [.., C] over n rows: n terms, the squares rounded once,
    the partial sums combined by atomics and over the replicas (c = 4)."""
    C = y.shape[-1]
    v = y.double().reshape(-1, C)
    n = v.shape[0]
    ref = torch.stack([v.sum(0), (v * v).sum(0)])
    return ref, (n + 4) * U * torch.stack([v.abs().sum(0), (v * v).sum(0)])


def maxpool_bwd(dy, arg, k, stride, pad_h, pad_w, H, W):
    """dx = scatter-add of dy to the recorded tap of each window (fp64), and sum |contributions|.
    Bound: at most k*k fp32 additions, then the bf16 rounding; exactly 0 where nothing arrives."""
    N, P, Q, C = dy.shape
    n, p, q, c = torch.meshgrid(torch.arange(N), torch.arange(P), torch.arange(Q), torch.arange(C), indexing="ij")
    a = arg.long()
    h = p * stride - pad_h + a // k
    w = q * stride - pad_w + a % k
    ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
    flat = (((n * H + h) * W + w) * C + c)[ok]
    d = dy.double()[ok]
    ref = torch.zeros(N * H * W * C, dtype=torch.float64).index_add_(0, flat, d).view(N, H, W, C)
    mag = torch.zeros(N * H * W * C, dtype=torch.float64).index_add_(0, flat, d.abs()).view(N, H, W, C)
    return ref, (BF + (k * k + 2) * U) * mag


# -- optimizer ----------------------------------------------------------------------------------------
def sgd_momentum(w0, m0, g, lr, mu, wd, gs):
    """g' = gs g + wd w0; m = mu m0 + g'; w = w0 - lr m, with the scalars as their fp32 values.
    Bounds (the issue's): 8 * 2^-24 * the sum of the magnitudes entering each result."""
    lr, mu, wd, gs = f32(lr), f32(mu), f32(wd), f32(gs)
    w0, m0, g = w0.double(), m0.double(), g.double()
    m = mu * m0 + (gs * g + wd * w0)
    w = w0 - lr * m
    mag_m = mu * m0.abs() + gs * g.abs() + wd * w0.abs()
    return w, m, 8 * U * (w0.abs() + lr * mag_m), 8 * U * mag_m


# -- input --------------------------------------------------------------------------------------------
def cifar_augment(raw, params, pad):
    """Zero-pad by `pad`, crop H x W at (oy, ox), flip, (x - mean) / max(std, 1 / sqrt(3 H W)).
    fp32 error of (v - mean) / adj: the sums of 3HW terms behind mean and the variance
    ((3HW + 8) * 2^-24 relative to the result), the rounded mean against v (2 * 2^-24 |mean| / adj),
    then the bf16 rounding."""
    N, H, W, _ = raw.shape
    ref = torch.zeros(N, H, W, 3, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    cnt = 3 * H * W
    for n in range(N):
        oy, ox, flip = (int(v) for v in params[n].tolist())
        big = torch.zeros(H + 2 * pad, W + 2 * pad, 3, dtype=torch.float64)
        big[pad:pad + H, pad:pad + W] = raw[n].double()
        crop = big[oy:oy + H, ox:ox + W]
        if flip:
            crop = crop.flip(1)
        mean = crop.sum() / cnt
        var = ((crop - mean) ** 2).sum() / cnt
        adj = max(float(var.sqrt()), cnt ** -0.5)
        ref[n] = (crop - mean) / adj
        bound[n] = BF * ref[n].abs() + U * ((cnt + 8) * ref[n].abs() + 2 * abs(float(mean)) / adj)
    return ref, bound


def synthetic_images(npix, seed):
    """The hash of csrc/kernels/augment.hip synthetic_images_kernel in numpy uint32 arithmetic:
    [npix, 8] bf16, channels 3..7 zero. (h >> 8) * 2^-23 - 1 is exact in fp32."""
    with np.errstate(over="ignore"):
        idx = np.arange(npix * 3, dtype=np.uint64).astype(np.uint32)
        h = idx * np.uint32(2654435761) ^ np.uint32(seed & 0xFFFFFFFF)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    f = ((h >> np.uint32(8)).astype(np.float64) * (2.0 / 16777216.0) - 1.0).astype(np.float32)
    out = torch.zeros(npix, 8, dtype=torch.bfloat16)
    out[:, :3] = torch.from_numpy(f).view(npix, 3).to(torch.bfloat16)
    return out


# -- convolution --------------------------------------------------------------------------------------
# The references below are the definitions of conv_fwd.hip / conv_wgrad.hip / bn.hip's operations.
A23 = 2.0 ** -23    # one MFMA accumulation step: the matrix unit's adder may truncate (one fp32 ulp)


def conv_operand(x, in_bn, relu_in=True):
    """The conv's input operand and its error: x itself (exact), or the fused BN prologue
    bf16(act(fl(x scale + shift))). Reference: the unrounded fp64 act(x scale + shift); error of the
    kernel's operand (two fp32 roundings, ReLU is 1-Lipschitz, then the bf16 rounding):
    (BF + 2U) (|x scale| + |shift|)."""
    v = x.double()
    if in_bn is None:
        return v, torch.zeros_like(v)
    sc, sh = in_bn[0].double(), in_bn[1].double()
    err = (BF + 2 * U) * ((v * sc).abs() + sh.abs())
    v = v * sc + sh
    return (v.clamp_min(0) if relu_in else v), err


def _im2col(t, R, S, P, Q, stride, pad_h, pad_w, dil=1):
    """t [N,H,W,C] fp64 -> {(r, s): [N*P*Q, C]} with rows t_v[n, p stride - pad_h + r, q stride - pad_w + s]
    of the virtual input t_v (t with dil - 1 zeros between its pixels), exact zeros outside it."""
    N, H, W, C = t.shape
    Hv, Wv = (H - 1) * dil + 1, (W - 1) * dil + 1
    big = torch.zeros(N, max(pad_h + Hv, (P - 1) * stride + R), max(pad_w + Wv, (Q - 1) * stride + S), C,
                      dtype=torch.float64)
    big[:, pad_h:pad_h + Hv:dil, pad_w:pad_w + Wv:dil] = t
    return {(r, s): big[:, r:r + (P - 1) * stride + 1:stride, s:s + (Q - 1) * stride + 1:stride].reshape(-1, C)
            for r in range(R) for s in range(S)}


def conv_fwd(x, w, P, Q, stride, pad_h, pad_w, dil=1, in_bn=None, relu_in=True, residual=None, bn_bwd=None,
             partials=0):
    """y[n,p,q,k] = sum_{r,s,c} op[n, p stride - pad_h + r, q stride - pad_w + s, c] w[k,r,s,c] (+ residual),
    op = conv_operand(x) zero-dilated by dil, zero outside; with bn_bwd = (xb, scale, shift) the
    stored value is the sum where xb scale + shift > 0 and exactly 0 elsewhere.
    Returns (ref [N,P,Q,K], bound, number of elements whose mask is ambiguous in fp32).
    Bound: n = R S C MFMA accumulation steps + `partials` extra combinations (split-K partials,
    stream-K slots) + the residual add (c = 2 with the hand-off of the tile), each 2^-23 of
    sum |terms| + |residual|; the prologue's operand error sum_k |w_k| err_k; the whole carried
    through the bf16 rounding ((1 + BF) e + BF |ref|). Where the mask is off the bound is 0."""
    K, R, S, C = w.shape
    N = x.shape[0]
    op, operr = conv_operand(x, in_bn, relu_in)
    cols, ecols = _im2col(op, R, S, P, Q, stride, pad_h, pad_w, dil), None
    if in_bn is not None:
        ecols = _im2col(operr, R, S, P, Q, stride, pad_h, pad_w, dil)
    wd = w.double()
    ref = torch.zeros(N * P * Q, K, dtype=torch.float64)
    mag, perr = torch.zeros_like(ref), torch.zeros_like(ref)
    for (r, s), a in cols.items():
        wt = wd[:, r, s, :].t()
        ref += a @ wt
        mag += a.abs() @ wt.abs()
        if ecols is not None:
            perr += ecols[(r, s)] @ wt.abs()
    if residual is not None:
        ref += residual.double().reshape(-1, K)
        mag += residual.double().abs().reshape(-1, K)
    e = (R * S * C + partials + 2) * A23 * mag + perr
    bound = (1 + BF) * e + BF * ref.abs()
    amb = 0
    if bn_bwd is not None:
        xb, sc, sh = (t.double() for t in bn_bwd[:3])
        pre = xb.reshape(-1, K) * sc
        amb = int(((pre + sh).abs() <= 2 * U * (pre.abs() + sh.abs())).sum())
        on = (pre + sh) > 0
        ref, bound = torch.where(on, ref, torch.zeros_like(ref)), torch.where(on, bound, torch.zeros_like(bound))
    return ref.view(N, P, Q, K), bound.view(N, P, Q, K), amb


def conv_wgrad(x, dy, R, S, stride, pad_h, pad_w, in_bn=None, relu_in=True, partials=0):
    """dw[k,r,s,c] = sum_{n,p,q} dy[n,p,q,k] op[n, p stride - pad_h + r, q stride - pad_w + s, c].
    Bound: M = N P Q accumulation steps + `partials` (slabs summed by drn_splitk_reduce, or atomics)
    + 2, each 2^-23 of sum |terms|, + the prologue's operand error sum_m |dy_m| err_m. fp32 output."""
    N, P, Q, K = dy.shape
    C = x.shape[-1]
    op, operr = conv_operand(x, in_bn, relu_in)
    cols = _im2col(op, R, S, P, Q, stride, pad_h, pad_w)
    ecols = _im2col(operr, R, S, P, Q, stride, pad_h, pad_w) if in_bn is not None else None
    d = dy.double().reshape(-1, K).t()
    ref = torch.zeros(K, R, S, C, dtype=torch.float64)
    mag, perr = torch.zeros_like(ref), torch.zeros_like(ref)
    for (r, s), a in cols.items():
        ref[:, r, s] = d @ a
        mag[:, r, s] = d.abs() @ a.abs()
        if ecols is not None:
            perr[:, r, s] = d.abs() @ ecols[(r, s)]
    return ref, (N * P * Q + partials + 2) * A23 * mag + perr


def channel_sums(t1, t2, reps, c):
    """Per-channel (sum t1, sum t2) of [M][C] fp64 terms: a pure fp32 reduction of M terms in any
    order over `reps` replicas, c roundings per term outside the sum: (M + reps + c) U sum |terms|."""
    ref = torch.stack([t1.sum(0), t2.sum(0)])
    return ref, (t1.shape[0] + reps + c) * U * torch.stack([t1.abs().sum(0), t2.abs().sum(0)])


def conv_stats(y_stored, reps):
    """The conv epilogue's next-BN statistics (sum, sum of squares) of the values it STORED (the
    bf16 y read back, checked per element separately); the squares are rounded once (c = 4)."""
    v = y_stored.double().reshape(-1, y_stored.shape[-1])
    return channel_sums(v, v * v, reps, 4)


def bn_bwd_sums(g, xb, mean, invstd, reps, c=8):
    """(sum g, sum g xhat), xhat = (xb - mean) invstd, of the masked gradient g the kernel stored (conv
    epilogue) or read (bn_bwd_reduce): fl(xb - mean), the two products and the accumulation's own
    step are 3 roundings per term (c = 8 with the cross-wave / atomic combination; + 2 for the
    pool-broadcast source's dpool * fl(1 / HW))."""
    C = g.shape[-1]
    gg = g.double().reshape(-1, C)
    xh = (xb.double().reshape(-1, C) - mean.double()) * invstd.double()
    return channel_sums(gg, gg * xh, reps, c)


def relu_mask(x, scale, shift):
    """(x scale + shift > 0, number of elements ambiguous in fp32: |x scale + shift| <= 2U(|x scale| + |shift|))."""
    pre = x.double() * scale.double()
    v = pre + shift.double()
    return v > 0, int((v.abs() <= 2 * U * (pre.abs() + shift.double().abs())).sum())


# -- batch norm ---------------------------------------------------------------------------------------
def bn_finalize_fwd(parts, count, gamma, beta, eps, momentum, run_mean0, run_var0, fp32_math, e_parts=None):
    """parts [G][2][C] fp32 -> dict name: (ref, bound) of scale, shift, mean, invstd, run_mean, run_var,
    in fp64 from the given sums. The replicas are summed in fp32: e_s = G U sum_r |s_r|, e_q alike.
      mean = s / n:            e_m = e_s / n + cm U |mean|
      var = max(q / n - mean^2, 0): e_v = e_q / n + 2 |mean| e_m + e_m^2 + cv U q / n   (relative to q / n:
                               the subtraction cancels; the clamp is 1-Lipschitz)
      invstd = (var + eps)^-1/2: e_i = e_v / (2 (max(var - e_v, 0) + eps)^1.5) + ci U invstd
      scale = gamma invstd:    e_sc = |gamma| e_i + U |scale|
      shift = beta - mean scale: e_sh = |mean| e_sc + |scale| e_m + e_m e_sc + 3 U (|beta| + |mean scale|)
                               (fl(mean), the product, the subtraction: 3 roundings)
      run_mean = mo rm0 + (1 - mo) mean: (1 - mo) e_m + 4 U (|mo rm0| + |(1 - mo) mean|)  (fl(mean), two products,
                               the add; 1 - mo is exact in fp32, Sterbenz)
      run_var = mo rv0 + (1 - mo) var k, k = n / (n - 1) (count == 1: k = 1): (1 - mo) k e_v + 6 U (|mo rv0| +
                               |(1 - mo) var k|)  (var n, the division or fl(n / (n - 1)), fl(unbiased), two products,
                               the add)
    e_parts [2][C]: an error the sums themselves already carry (a backend that hands over no replicas).
    Rounding counts: the standalone bn_finalize_kernel and the conv's bn_fin_column work in double
    from the fp32 sums and round once (cm = 1, cv = 0, ci = 1); the consumer-side drn_bn_fin_fwd and
    bn_stats_to_affine work in fp32 (cm = 2: 1 / n and the product; cv = 4; ci = 4: the add, sqrtf, the
    division, correctly rounded in this build)."""
    cm, cv, ci = (2, 4, 4) if fp32_math else (1, 0, 1)
    p = parts.double()
    G = p.shape[0]
    n = float(np.float32(count))
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    e_s, e_q = G * U * p[:, 0].abs().sum(0), G * U * p[:, 1].abs().sum(0)
    if e_parts is not None:
        e_s, e_q = e_s + e_parts[0], e_q + e_parts[1]
    mean = s / n
    e_m = e_s / n + cm * U * mean.abs()
    var = (q / n - mean * mean).clamp_min(0)
    e_v = e_q / n + 2 * mean.abs() * e_m + e_m * e_m + cv * U * (q / n).abs()
    ep = float(np.float32(eps))
    invstd = (var + ep) ** -0.5
    e_i = e_v / (2 * ((var - e_v).clamp_min(0) + ep) ** 1.5) + ci * U * invstd
    ga, be = gamma.double(), beta.double()
    scale = ga * invstd
    e_sc = ga.abs() * e_i + U * scale.abs()
    shift = be - mean * scale
    e_sh = mean.abs() * e_sc + scale.abs() * e_m + e_m * e_sc + 3 * U * (be.abs() + (mean * scale).abs())
    out = {"scale": (scale, e_sc), "shift": (shift, e_sh), "mean": (mean, e_m), "invstd": (invstd, e_i)}
    if run_mean0 is not None:
        mo = float(np.float32(momentum))
        om = float(np.float32(1) - np.float32(momentum))
        k = n / (n - 1) if n > 1 else 1.0
        a, b = mo * run_mean0.double(), om * mean
        out["run_mean"] = (a + b, om * e_m + 4 * U * (a.abs() + b.abs()))
        a, b = mo * run_var0.double(), om * var * k
        out["run_var"] = (a + b, om * k * e_v + 6 * U * (a.abs() + b.abs()))
    return out


def bn_finalize_bwd(parts, count, gamma, invstd, e_parts=None):
    """parts [G][2][C] (sum g, sum g xhat) -> dbeta, dgamma, coef [3][C] = (gamma invstd, sum g / n,
    sum g xhat / n): the fp32 replica sum (G U sum_r |.|), one rounding for each quotient / product."""
    p = parts.double()
    G = p.shape[0]
    n = float(np.float32(count))
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    e_s, e_q = G * U * p[:, 0].abs().sum(0), G * U * p[:, 1].abs().sum(0)
    if e_parts is not None:
        e_s, e_q = e_s + e_parts[0], e_q + e_parts[1]
    k1 = gamma.double() * invstd.double()
    coef = torch.stack([k1, s / n, q / n])
    e_c = torch.stack([U * k1.abs(), e_s / n + U * (s / n).abs(), e_q / n + U * (q / n).abs()])
    return {"dbeta": (s, e_s), "dgamma": (q, e_q), "coef": (coef, e_c)}


def bn_apply(x, scale, shift, relu):
    """y = bf16(act(fl(x scale + shift))): BF |ref| + 2U (|x scale| + |shift|)."""
    pre = x.double() * scale.double()
    v = pre + shift.double()
    ref = v.clamp_min(0) if relu else v
    return ref, BF * ref.abs() + (1 + BF) * 2 * U * (pre.abs() + shift.double().abs())


def bn_bwd_apply(g, x, k1, k2, k3, mean, invstd, add, coef_roundings):
    """dx = bf16(A g + B x + D (+ add)), A = k1, B = -k1 k3 invstd, D = -k1 k2 + k1 k3 invstd mean, from
    fp32 k1, k2, k3 (the coef table, or gamma invstd, sum g / n, sum g xhat / n of the PUBLISHED sums),
    g already masked. coef_roundings = (a, b, d1, d2): the roundings behind A, B and the two terms of D
    (bn_bwd_apply reads k1..k3: 0, 2, 1 + 1, 3 + 1; the *_fin prologue also forms k1, k2, k3: 1, 4, 3 + 1,
    5 + 1). Then three products / adds and the optional add: 4U sum |terms|; then the bf16 rounding."""
    a, b, d1, d2 = coef_roundings
    k1, k2, k3, mu, isd = (t.double() for t in (k1, k2, k3, mean, invstd))
    A, B = k1, -k1 * k3 * isd
    t1, t2 = -k1 * k2, k1 * k3 * isd * mu
    gg, xx = g.double(), x.double()
    ref = A * gg + B * xx + (t1 + t2)
    mag = (A * gg).abs() + (B * xx).abs() + t1.abs() + t2.abs()
    e = U * (a * (A * gg).abs() + b * (B * xx).abs() + d1 * t1.abs() + d2 * t2.abs())
    if add is not None:
        ref = ref + add.double()
        mag = mag + add.double().abs()
    e = e + 4 * U * mag
    return ref, (1 + BF) * e + BF * ref.abs()


def bn_bwd_apply_nested(g, x, gamma, invstd, mean, sg, sgx, count, add):
    """bn_bwd_apply_stats_kernel's form dx = bf16(k1 (g - k2 - xhat k3) (+ add)), k1 = gamma invstd, k2 = sg / n,
    k3 = sgx / n, xhat = (x - mean) invstd, g already masked. Roundings on the way to the product with k1
    (k1 itself, the two subtractions, the product: 4): g 4; k2 one more (5); xhat k3 four more (fl(x - mean),
    the product with invstd, k3, the product: 8); the add one more relative to the result."""
    n = float(np.float32(count))
    k1 = gamma.double() * invstd.double()
    k2, k3 = sg.double() / n, sgx.double() / n
    gg = g.double()
    t3 = (x.double() - mean.double()) * invstd.double() * k3
    ref = k1 * (gg - k2 - t3)
    e = U * k1.abs() * (4 * gg.abs() + 5 * k2.abs() + 8 * t3.abs())
    if add is not None:
        ref = ref + add.double()
        e = e + U * (ref.abs() + add.double().abs())
    return ref, (1 + BF) * e + BF * ref.abs()
