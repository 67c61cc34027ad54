"""Independent fp64 references of the head, pooling, optimizer and input kernels, written directly
with torch and numpy from each operation's definition (RefBackend is not used here: it is one of
the two implementations under test), and the one comparison helper, assert_within.

Every reference returns the exact result in fp64 together with a per-element bound that is derived
from the operation and computed in fp64 from the inputs:

  * an fp32 sum of n terms / a length-K dot product, in ANY summation order:
        (n + c) * 2^-24 * sum |terms|        (c: the roundings outside the sum, counted per op below)
  * a value rounded to bf16 at the end:  + 2^-8 * |ref|   (half a bf16 ulp plus the double rounding)
  * integers, maxima of bf16 values, hashes, casts, fills and untouched memory: torch.equal.
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
