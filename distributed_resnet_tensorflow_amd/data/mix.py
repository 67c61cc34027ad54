"""Host-side draws of Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) batches.

A batch of N samples is mixed with its own reversal (partner of sample n: N - 1 - n; the batch is
already shuffled, so the pairing is random). `MixSampler.draw(batch_index)` returns the batch's
table: one record per sample (ops/backend.py MIX_REC) that the image kernel (csrc/kernels/mix.hip)
and the loss kernel (csrc/kernels/head.hip softmax_xent_mix_kernel) both read from device memory.

The draws are counter-based like the CIFAR loader's crop draws: the generator of batch i is seeded
with (seed, TAG, rank, i), so a resumed run continues the same sequence from its batch counter alone
and every data-parallel rank mixes its own shard with its own draws.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from ..ops.backend import MIX_REC, mix_identity

TAG = 104729  # keeps these draws apart from every other (seed, ...) stream of the input pipeline


class MixSampler:
    """mixup_alpha > 0: Mixup, lam ~ Beta(a, a), w = lam, no box. cutmix_alpha > 0: CutMix, lam0 ~
    Beta(a, a), a box of sides H sqrt(1 - lam0), W sqrt(1 - lam0) around a uniform centre, clipped to
    the image, w = 1 and lam = 1 - box_area / (H W) from the clipped box. Both: CutMix with
    probability switch_prob. A batch is mixed with probability prob, else it gets identity records.
    per_sample: every sample draws its own kind, lam and box; otherwise one draw serves the batch."""

    def __init__(self, N: int, H: int, W: int, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0,
                 prob: float = 1.0, switch_prob: float = 0.5, per_sample: bool = False, seed: int = 0,
                 rank: int = 0):
        if N < 1 or H < 1 or W < 1:
            raise ValueError(f"MixSampler needs N, H, W >= 1, got {N}, {H}, {W}")
        if mixup_alpha < 0 or cutmix_alpha < 0 or not (mixup_alpha > 0 or cutmix_alpha > 0):
            raise ValueError("MixSampler needs mixup_alpha >= 0 and cutmix_alpha >= 0, one of them > 0")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"prob and switch_prob must be in [0, 1], got {prob}, {switch_prob}")
        self.N, self.H, self.W = int(N), int(H), int(W)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.per_sample = float(prob), float(switch_prob), bool(per_sample)
        self.seed, self.rank = int(seed), int(rank)

    def _one(self, rng, rec):
        """Fill one record (w, lam, box) from the next draws of rng."""
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = rng.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        if not cut:
            lam = np.float32(rng.beta(self.mixup_alpha, self.mixup_alpha))
            rec["w"] = rec["lam"] = lam
            return
        lam0 = rng.beta(self.cutmix_alpha, self.cutmix_alpha)
        H, W = self.H, self.W
        side = math.sqrt(max(0.0, 1.0 - lam0))
        bh, bw = int(H * side), int(W * side)
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        y0, x0 = cy - bh // 2, cx - bw // 2
        y1, x1 = min(max(y0 + bh, 0), H), min(max(x0 + bw, 0), W)
        y0, x0 = min(max(y0, 0), H), min(max(x0, 0), W)
        rec["w"] = 1.0
        rec["y0"], rec["x0"], rec["y1"], rec["x1"] = y0, x0, y1, x1
        rec["lam"] = np.float32(1.0 - (y1 - y0) * (x1 - x0) / (H * W))

    def draw(self, batch_index: int, labels: Optional[np.ndarray] = None) -> np.ndarray:
        """The MIX_REC [N] table of batch `batch_index`; label_b = the batch's labels reversed (0
        without labels)."""
        rng = np.random.default_rng([self.seed, TAG, self.rank, int(batch_index)])
        t = mix_identity(self.N)
        if labels is not None:
            lab = np.asarray(labels).reshape(-1)
            if lab.shape[0] != self.N:
                raise ValueError(f"{lab.shape[0]} labels for a batch of {self.N}")
            t["label_b"] = lab[::-1]
        if not rng.random() < self.prob:
            return t
        if self.per_sample:
            for n in range(self.N):
                self._one(rng, t[n:n + 1])
        else:
            self._one(rng, t[0:1])
            for k in ("w", "lam", "y0", "x0", "y1", "x1"):
                t[k] = t[k][0]
        return t
