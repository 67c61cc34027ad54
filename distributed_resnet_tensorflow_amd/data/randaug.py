"""RandAugment (Cubuk et al. 2020) for the Inception-style ImageNet input: the host-side draws, the per-image
descriptor records and the integer reference of csrc/kernels/randaug.hip.

Everything runs on 8-bit levels in integer arithmetic. After the box resample a pixel on [0, 1] is quantised
once, q = clamp(floor(255 x + 0.5), 0, 255) (`quantize_np`, fp32 like the kernel); every operation maps
integers to integers with a stated rounding, so `randaug_np` (numpy int64) and the kernel agree bit for bit.

The 14 operations are torchvision's `RandAugment` set, magnitude M in 0..30 (31 bins), signed operations
negated with probability 1/2. With gray = (77 R + 150 G + 29 B + 128) >> 8 and
blend(a, b, f) = clamp(floor((f a + (256 - f) b + 128) / 256), 0, 255), f = round(256 factor):

  Identity
  ShearX / ShearY      +-0.3 M/30                inverse affine map, nearest pixel, fill 128
  TranslateX / Y       +-(150/331) O M/30 px     same
  Rotate               +-30 deg M/30, centre     same (positive = counter-clockwise, like np.rot90)
  Brightness           factor 1 +- 0.9 M/30      blend(p, 0, f)
  Color                same                      blend(p, gray(p), f) per channel
  Contrast             same                      blend(p, m, f), m = floor((sum of gray + n//2) / n)
  Sharpness            same                      blend(p, s, f); interior s = floor((8 neighbours + 5 p + 6) / 13),
                                                 on the one-pixel border s = p
  Posterize            bits = 8 - round(4 M/30)  keep the top `bits` bits
  Solarize             t = round(255 - 255 M/30) p >= t ? 255 - p : p  (so, as in PIL, M = 0 still inverts level 255)
  AutoContrast                                   per channel lo, hi; hi > lo: floor(((p - lo) 255 + (hi - lo)//2) / (hi - lo))
  Equalize                                       per channel histogram h, step = (n - h[last non-zero level]) // 255;
                                                 step == 0: identity, else lut[i] = min(255, (step//2 + sum_{j<i} h[j]) // step)

The affine operations do not depend on floating-point rounding: the host computes the inverse 2 x 3 matrix in
fp64 and rounds its entries to 16.16 fixed point (`affine_entries`: A in units of 2^-16, T in units of 2^-16
half-pixels); for output pixel (x, y), u = 2x + 1 - O and v = 2y + 1 - O, the source column is
floor((A00 u + A01 v + T0 + O 2^16) / 2^17) and the source row likewise from the second matrix row; a source
outside [0, O) gives 128 in all three channels.

The draws are counter-based like data/mix.py's and data/drop_path.py's: the generator of sample n of batch i
is seeded with (seed, TAG, rank, i, n), so there is no generator state to checkpoint and a run resumed at
batch k redraws batch k's records.
"""
from __future__ import annotations

import math

import numpy as np

TAG = 240914  # keeps these draws apart from every other (seed, ...) stream of the input pipeline

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
       "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE,
 SOLARIZE, AUTOCONTRAST, EQUALIZE) = range(14)
SIGNED = frozenset(range(SHEAR_X, SHARPNESS + 1))
AFFINE = frozenset(range(SHEAR_X, ROTATE + 1))
NUM_BINS, MAX_LAYERS, MAX_SIDE, FILL = 31, 4, 224, 128

# numpy mirror of csrc/kernels/randaug.hip `struct RaDesc` (144 bytes): p is f, the bits kept or the threshold;
# m is A00, A01, T0, A10, A11, T1
RA_OP = np.dtype([("id", "<i4"), ("p", "<i4"), ("m", "<i4", (6,))])
RA_DESC = np.dtype([("nops", "<i4"), ("pad", "<i4", (3,)), ("op", RA_OP, (MAX_LAYERS,))])
assert RA_DESC.itemsize == 144 and RA_DESC.itemsize % 16 == 0

_IDENTITY_M = (1 << 16, 0, 0, 0, 1 << 16, 0)


def _round(v: float) -> int:
    return int(math.floor(v + 0.5))


def affine_entries(M, t=(0.0, 0.0)):
    """The six 16.16 entries (A00, A01, T0, A10, A11, T1) of the inverse of the forward map
    dst = M src + t, in pixels about the image centre with y down."""
    (a, b), (c, d) = ((float(v) for v in row) for row in M)
    det = a * d - b * c
    A = ((d / det, -b / det), (-c / det, a / det))
    T = tuple(-(A[r][0] * 2.0 * t[0] + A[r][1] * 2.0 * t[1]) for r in range(2))   # half-pixels
    return tuple(_round(v * 65536.0) for v in (A[0][0], A[0][1], T[0], A[1][0], A[1][1], T[1]))


def rotation(deg: float):
    """Forward matrix of a counter-clockwise rotation by `deg` degrees (y down)."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return ((c, s), (-s, c))


def op_record(op: int, magnitude: int, negate: bool, O: int):
    """(id, p, m) of operation `op` at magnitude bin `magnitude` for an O x O image: all magnitude arithmetic
    happens here, the kernel sees integers only."""
    if not (0 <= op < len(OPS) and 0 <= magnitude < NUM_BINS):
        raise ValueError(f"op must be in 0..13 and magnitude in 0..30, got {op!r}, {magnitude!r}")
    v = magnitude / (NUM_BINS - 1.0)
    sv = -v if (negate and op in SIGNED) else v
    p, m = 0, _IDENTITY_M
    if op == SHEAR_X:
        m = affine_entries(((1.0, 0.3 * sv), (0.0, 1.0)))
    elif op == SHEAR_Y:
        m = affine_entries(((1.0, 0.0), (0.3 * sv, 1.0)))
    elif op == TRANSLATE_X:
        m = affine_entries(((1.0, 0.0), (0.0, 1.0)), (150.0 / 331.0 * O * sv, 0.0))
    elif op == TRANSLATE_Y:
        m = affine_entries(((1.0, 0.0), (0.0, 1.0)), (0.0, 150.0 / 331.0 * O * sv))
    elif op == ROTATE:
        m = affine_entries(rotation(30.0 * sv))
    elif op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        p = _round(256.0 * (1.0 + 0.9 * sv))
    elif op == POSTERIZE:
        p = 8 - _round(4.0 * v)
    elif op == SOLARIZE:
        p = _round(255.0 - 255.0 * v)
    return op, p, m


def make_desc(chains, O: int) -> np.ndarray:
    """RA_DESC records from per-image chains of (op, magnitude, negate)."""
    d = np.zeros(len(chains), dtype=RA_DESC)
    for n, chain in enumerate(chains):
        if len(chain) > MAX_LAYERS:
            raise ValueError(f"a chain holds at most {MAX_LAYERS} operations, got {len(chain)}")
        d[n]["nops"] = len(chain)
        for k, (op, mag, neg) in enumerate(chain):
            d[n]["op"][k] = op_record(op, mag, neg, O)
    return d


class RandAugSampler:
    """draw(batch_index) -> RA_DESC[N]: per image `layers` operations, each uniform over the 14 with a fair
    sign, all at magnitude bin `magnitude`."""

    def __init__(self, N: int, side: int, layers: int, magnitude: int = 9, seed: int = 0, rank: int = 0):
        if N < 1 or not 1 <= layers <= MAX_LAYERS or not 0 <= magnitude < NUM_BINS:
            raise ValueError(f"RandAugSampler needs N >= 1, 1 <= layers <= {MAX_LAYERS} and 0 <= magnitude <= 30, "
                             f"got {N}, {layers}, {magnitude}")
        if not 1 <= side <= MAX_SIDE:
            raise ValueError(f"RandAugment keeps the image in LDS: side must be in 1..{MAX_SIDE}, got {side}")
        self.N, self.side, self.layers, self.magnitude = int(N), int(side), int(layers), int(magnitude)
        self.seed, self.rank = int(seed), int(rank)

    def draw_chain(self, batch_index: int, sample: int):
        rng = np.random.default_rng([self.seed, TAG, self.rank, int(batch_index), int(sample)])
        ops, neg = rng.integers(0, len(OPS), self.layers), rng.integers(0, 2, self.layers)
        return [(int(o), self.magnitude, bool(s)) for o, s in zip(ops, neg)]

    def draw(self, batch_index: int) -> np.ndarray:
        return make_desc([self.draw_chain(batch_index, n) for n in range(self.N)], self.side)


# -- the integer reference --------------------------------------------------------------------------------
def quantize_np(x) -> np.ndarray:
    """[0, 1] pixels -> int64 levels, in fp32 like the kernel: clamp(floor(255 x + 0.5), 0, 255)."""
    x = np.asarray(x, dtype=np.float32)
    return np.clip(np.floor(np.float32(255.0) * x + np.float32(0.5)), 0, 255).astype(np.int64)


def gray_np(q):
    return (77 * q[..., 0] + 150 * q[..., 1] + 29 * q[..., 2] + 128) >> 8


def blend_np(a, b, f: int):
    return np.clip((f * a + (256 - f) * b + 128) >> 8, 0, 255)


def affine_np(q, m):
    O = q.shape[0]
    a00, a01, t0, a10, a11, t1 = (int(v) for v in m)
    v, u = np.meshgrid(2 * np.arange(O, dtype=np.int64) + 1 - O, 2 * np.arange(O, dtype=np.int64) + 1 - O,
                       indexing="ij")
    sx = (a00 * u + a01 * v + t0 + (O << 16)) >> 17
    sy = (a10 * u + a11 * v + t1 + (O << 16)) >> 17
    ok = (sx >= 0) & (sx < O) & (sy >= 0) & (sy < O)
    out = np.full_like(q, FILL)
    out[ok] = q[sy[ok], sx[ok]]
    return out


def sharpness_np(q, f: int):
    s = q.copy()
    if q.shape[0] > 2:
        nb = sum(q[1 + dy:q.shape[0] - 1 + dy, 1 + dx:q.shape[1] - 1 + dx]
                 for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
        s[1:-1, 1:-1] = (nb + 5 * q[1:-1, 1:-1] + 6) // 13
    return blend_np(q, s, f)


def autocontrast_np(q):
    out = q.copy()
    for c in range(3):
        lo, hi = int(q[..., c].min()), int(q[..., c].max())
        if hi > lo:
            out[..., c] = ((q[..., c] - lo) * 255 + (hi - lo) // 2) // (hi - lo)
    return out


def equalize_np(q):
    out = q.copy()
    n = q.shape[0] * q.shape[1]
    for c in range(3):
        h = np.bincount(q[..., c].reshape(-1), minlength=256).astype(np.int64)
        step = (n - int(h[np.nonzero(h)[0][-1]])) // 255
        if step:
            lut = np.minimum(255, (step // 2 + np.cumsum(h) - h) // step)
            out[..., c] = lut[q[..., c]]
    return out


def apply_op_np(q, rec):
    """One operation record (id, p, m) on int64 [O, O, 3] levels."""
    op, p = int(rec["id"]), int(rec["p"])
    if op in AFFINE:
        return affine_np(q, rec["m"])
    if op == BRIGHTNESS:
        return blend_np(q, 0, p)
    if op == COLOR:
        return blend_np(q, gray_np(q)[..., None], p)
    if op == CONTRAST:
        n = q.shape[0] * q.shape[1]
        return blend_np(q, (int(gray_np(q).sum()) + n // 2) // n, p)
    if op == SHARPNESS:
        return sharpness_np(q, p)
    if op == POSTERIZE:
        return q & ((0xFF << (8 - min(max(p, 0), 8))) & 0xFF)
    if op == SOLARIZE:
        return np.where(q >= p, 255 - q, q)
    if op == AUTOCONTRAST:
        return autocontrast_np(q)
    if op == EQUALIZE:
        return equalize_np(q)
    return q


def randaug_np(q, d) -> np.ndarray:
    """The chain of RA_DESC record d on int64 [O, O, 3] levels (square images)."""
    q = np.asarray(q, dtype=np.int64)
    assert q.ndim == 3 and q.shape[0] == q.shape[1] and q.shape[2] == 3, q.shape
    for k in range(min(max(int(d["nops"]), 0), MAX_LAYERS)):
        q = apply_op_np(q, d["op"][k])
    return q


def normalize_np(q, mean, std) -> np.ndarray:
    """fp32 (float(q) * (1 / 255) - mean) * (1 / std), rounded like the kernel (bf16 on store apart)."""
    x = q.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    istd = np.float32(1.0) / np.asarray(std, dtype=np.float32)
    return (x - np.asarray(mean, dtype=np.float32)) * istd
