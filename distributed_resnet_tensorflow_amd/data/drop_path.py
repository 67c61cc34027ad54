"""Host-side draws of stochastic depth (Huang et al. 2016; "drop path").

`DropPathSampler.draw(batch_index)` returns the batch's factor table: fp32 [blocks, N], f[b][n] = 0 when
sample n drops the residual branch of block b, else 1 / (1 - p_b) (inverted scaling, so evaluation is the
unscaled network). The executor's kernels (csrc/kernels/drop_path.hip) read it from device memory.

The draws are counter-based like the mix records' (data/mix.py): the generator of block b in batch i is
seeded with (seed, TAG, rank, i, b), so there is no generator state to checkpoint -- a resumed run
continues from its batch counter alone -- and every data-parallel rank draws for its own shard.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

TAG = 130363  # keeps these draws apart from every other (seed, ...) stream of the input pipeline


class DropPathSampler:
    def __init__(self, N: int, rates: Sequence[float], seed: int = 0, rank: int = 0):
        if N < 1:
            raise ValueError(f"DropPathSampler needs N >= 1, got {N}")
        self.rates = [float(p) for p in rates]
        if not all(0.0 <= p < 1.0 for p in self.rates):
            raise ValueError(f"drop probabilities must be in [0, 1), got {self.rates}")
        self.N, self.seed, self.rank = int(N), int(seed), int(rank)

    def draw_block(self, batch_index: int, block: int) -> np.ndarray:
        """The fp32 [N] factors of one block."""
        p = self.rates[block]
        if p == 0.0:
            return np.ones(self.N, dtype=np.float32)
        rng = np.random.default_rng([self.seed, TAG, self.rank, int(batch_index), int(block)])
        keep = rng.random(self.N) >= p
        return np.where(keep, np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32)

    def draw(self, batch_index: int) -> np.ndarray:
        """The fp32 [blocks, N] table of batch `batch_index`."""
        return np.stack([self.draw_block(batch_index, b) for b in range(len(self.rates))])
