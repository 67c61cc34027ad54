"""Independent fp64 reference of the Inception-style input kernels (csrc/kernels/input_box.hip), written with
torch's own anti-aliased interpolate on the crop and the colour operations' definitions (neither
data.imagenet's numpy reference nor RefBackend is used here: they are implementations under test), with a
per-element bound derived as in tests/kernel_refs.py:

  resample, per axis with n taps: the weight 1 - |t| inv carries the rounding of inv, of the product and of
  the subtraction (<= 3 U absolute, t is an exact integer); the weighted sum and the weight sum are fp32 sums
  of n terms; one division. With S = sum of the raw weights >= 1/2 (a triangle of half-width >= 1 sampled
  at unit steps, at worst cut in half by the box edge) that is  |dh| <= (2n + 2 + 6n / S) U P <= (14n + 2) U P,
  P the largest pixel of the crop. Two passes, then the product with the rounded 1/255:
        e_x = (14 (n_x + n_y) + 6) U P                               on [0, 1] pixels
  colour operations x' = a x + (1 - a) y in fp32: e' = |a| e_x + |1 - a| e_y + 2 U |(1 - a) y| + U |a x| + U |x'|;
  gray is three products and two sums (4 U sum |c x|); the mean gray is an fp32 sum of OH OW terms in any order
  ((OH OW + 8) U m0); brightness: e' = |a| e + U |x'|
  normalisation (x - mean) istd with the rounded mean and 1 / rounded std: (e + U mean) / std + 4 U |ref|
  the bf16 store: + 2^-8 |ref|
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from kernel_refs import BF, U

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
GRAY = (0.299, 0.587, 0.114)


def taps(box_len, out_len):
    """Upper bound of the taps of one output along an axis: the filter's support is 2 max(scale, 1) wide."""
    return int(math.ceil(2.0 * max(box_len / out_len, 1.0))) + 1


def resample(img, box, OH, OW):
    """fp64 [OH, OW, 3] on [0, 1] pixels and the bound e_x (a scalar)."""
    by, bx, bh, bw = box
    crop = torch.from_numpy(np.ascontiguousarray(img[by:by + bh, bx:bx + bw])).double() / 255.0
    x = F.interpolate(crop.permute(2, 0, 1)[None], size=(OH, OW), mode="bilinear", align_corners=False,
                      antialias=True)[0].permute(1, 2, 0)
    return x, (14 * (taps(bh, OH) + taps(bw, OW)) + 6) * U * float(crop.max())


def gray(x):
    return x[..., 0] * GRAY[0] + x[..., 1] * GRAY[1] + x[..., 2] * GRAY[2]


def _gray_err(x, e):
    return gray(e) + 4 * U * gray(x.abs())


def jitter(x, e, ops, ab, ac, asat):
    """The three operations, step by step in fp64, on (value, bound) pairs. m is taken when contrast runs
    (the mean gray of the image at that moment), not from the m0 identity."""
    n = x.shape[0] * x.shape[1]
    e = torch.full_like(x, e) if not torch.is_tensor(e) else e
    for op in ops:
        if op == 0:
            x = ab * x
            e = abs(ab) * e + U * x.abs()
        else:
            a = ac if op == 1 else asat
            if op == 1:
                y = gray(x).mean().expand(x.shape[:2])
                ey = (_gray_err(x, e).mean() + (n + 8) * U * gray(x.abs()).mean()).expand(x.shape[:2])
            else:
                y, ey = gray(x), _gray_err(x, e)
            o = ((1.0 - a) * y)[..., None]
            eo = (abs(1.0 - a) * ey)[..., None] + 2 * U * o.abs()
            new = a * x + o
            e = abs(a) * e + eo + U * (a * x).abs() + U * new.abs()
            x = new
    return x, e


def normalise(x, e, flip):
    e = torch.full_like(x, e) if not torch.is_tensor(e) else e
    if flip:
        x, e = x.flip(1), e.flip(1)
    mean, std = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    ref = (x - mean) / std
    return ref, (e + U * mean) / std + (4 * U + BF) * ref.abs()


def box_preprocess(img, d, OH, OW, jit):
    """(reference, bound) [OH, OW, 3] of one image and its BOX_DESC record."""
    x, e = resample(img, tuple(int(d[k]) for k in ("by", "bx", "bh", "bw")), OH, OW)
    if jit:
        ops = tuple((int(d["order"]) >> (2 * k)) & 3 for k in range(3))
        x, e = jitter(x, e, ops, float(d["ab"]), float(d["ac"]), float(d["as"]))
    return normalise(x, e, int(d["flip"]))


def pack(images, boxes, flips, jitters=None):
    """One packed uint8 buffer (the images back to back: unaligned offsets) and the BOX_DESC records.
    jitters: per image (ops, ab, ac, as) or None for the identity."""
    from distributed_resnet_tensorflow_amd.data import imagenet as inet
    desc = np.zeros(len(images), dtype=inet.BOX_DESC)
    off = 0
    for i, (img, box, flip) in enumerate(zip(images, boxes, flips)):
        ops, ab, ac, asat = jitters[i] if jitters is not None else ((0, 1, 2), 1.0, 1.0, 1.0)
        desc[i] = (off, img.shape[0], img.shape[1], *box, flip, inet.pack_order(ops), ab, ac, asat, (0, 0, 0))
        off += img.size
    return np.concatenate([im.reshape(-1) for im in images]), desc
