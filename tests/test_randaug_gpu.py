"""RandAugment on gfx950 (csrc/kernels/randaug.hip) against the numpy int64 reference (data/randaug.py): every
operation at both signs and three magnitudes with exact equality, drawn chains through box_preprocess against
RefBackend, and the refusals."""
import functools

import numpy as np
import pytest
import torch

from distributed_resnet_tensorflow_amd.data import imagenet as inet
from distributed_resnet_tensorflow_amd.data import randaug as ra
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# 16: whole dwords; 37: odd, 1369 pixels (a tail in every dword loop), the centre is a pixel; the 224 case below
# is the full LDS footprint and the only one whose dword loops take more than one pass of the 1024 threads
SIDES = (16, 37)
SINGLE = [(op, M, neg) for op in range(len(ra.OPS)) for neg in ((False, True) if op in ra.SIGNED else (False,))
          for M in (0, 9, 30)]   # (op, magnitude, negate)


def _levels(O, seed):
    """N = 3 images of 8-bit levels: random, constant, two levels."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (3, O, O, 3)).astype(np.int64)
    q[1] = np.array([7, 130, 255])
    q[2] = np.where(rng.random((O, O, 1)) < 0.4, 40, 200)
    return q


def _run(q, desc):
    """The kernel on fp32 scratch values k / 255, normalised with mean 0 and std 1 / 255 (the bf16 output holds
    the level itself); the output is prefilled with NaN. -> (kernel output, expected) as float [N, O, O, 8]."""
    N, O = q.shape[0], q.shape[1]
    scratch = torch.zeros(N * O * O, 4)
    scratch[:, :3] = torch.from_numpy(q.reshape(-1, 3).astype(np.float32)) / torch.tensor(255.0)
    out = torch.full((N, O, O, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    HipBackend().randaug(scratch.cuda(), torch.from_numpy(desc.view(np.uint8)).cuda(), out, (0.0, 0.0, 0.0),
                         (1 / 255,) * 3)
    torch.cuda.synchronize()
    exp = torch.zeros(N, O, O, 8)
    exp[..., :3] = torch.from_numpy(np.stack([ra.randaug_np(q[n], desc[n]) for n in range(N)]).astype(np.float32))
    return out.float().cpu(), exp


@functools.lru_cache(maxsize=None)
def _singles(O):
    """Every single-operation case at side O in one launch: case c owns images 3 c .. 3 c + 2."""
    q = np.concatenate([_levels(O, 100 + c) for c in range(len(SINGLE))])
    desc = ra.make_desc([[case] for case in SINGLE for _ in range(3)], O)
    return _run(q, desc)


@pytest.mark.parametrize("O", SIDES)
@pytest.mark.parametrize("c", range(len(SINGLE)), ids=lambda c: "{}{}-M{}".format(
    ra.OPS[SINGLE[c][0]], "-neg" if SINGLE[c][2] else "", SINGLE[c][1]))
def test_single_operation_is_exact(c, O):
    got, exp = _singles(O)
    assert torch.equal(got[3 * c:3 * c + 3], exp[3 * c:3 * c + 3])


def test_full_lds_footprint_rotate_then_equalize():
    q = _levels(224, 7)
    got, exp = _run(q, ra.make_desc([[(ra.ROTATE, 9, False), (ra.EQUALIZE, 0, False)]] * 3, 224))
    assert torch.equal(got, exp)


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_drawn_chains_match_ref_backend(layers):
    """HipBackend.box_preprocess(randaug=) against RefBackend's, bit for bit, with the real mean / std: boxes that
    cover their O x O image resample it exactly, so both quantise the same levels; every other image is flipped."""
    N, O = 8, 37
    rng = np.random.default_rng(layers)
    packed = rng.integers(0, 256, N * O * O * 3, dtype=np.uint8)
    box = np.zeros(N, dtype=inet.BOX_DESC)
    for n in range(N):
        box[n] = (n * O * O * 3, O, O, 0, 0, O, O, n & 1, inet.ORDER_IDENTITY, 1.0, 1.0, 1.0, (0, 0, 0))
    desc = ra.RandAugSampler(N, O, layers, 9 + 7 * (layers - 1), seed=3).draw(layers)
    out = torch.full((N, O, O, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    HipBackend().box_preprocess(torch.from_numpy(packed).cuda(), torch.from_numpy(box.view(np.uint8)).cuda(), out,
                                inet.NORM_MEAN, inet.NORM_STD, randaug=torch.from_numpy(desc.view(np.uint8)).cuda())
    torch.cuda.synchronize()
    exp = torch.full((N, O, O, 8), float("nan"), dtype=torch.bfloat16)
    RefBackend().box_preprocess(packed, box, exp, inet.NORM_MEAN, inet.NORM_STD, randaug=desc)
    assert torch.equal(out.cpu().view(torch.int16), exp.view(torch.int16))


def test_refusals():
    be = HipBackend()
    out = torch.zeros(1, 256, 256, 8, dtype=torch.bfloat16, device="cuda")
    buf = torch.zeros(256 * 256 * 3, dtype=torch.uint8, device="cuda")
    box = torch.zeros(64, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(ra.RA_DESC.itemsize, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="224"):
        be.box_preprocess(buf, box, out, inet.NORM_MEAN, inet.NORM_STD, randaug=desc)
    scratch = torch.zeros(256 * 256, 4, device="cuda")
    assert be.L.drn_randaug(scratch.data_ptr(), desc.data_ptr(), out.data_ptr(), buf.data_ptr(), 1, 256,
                            0.0, 0.0, 0.0, 1.0, 1.0, 1.0, be.stream()) != 0
    with pytest.raises(ValueError, match="jitter"):
        be.box_preprocess(buf, box, out[:, :37, :37].contiguous(), inet.NORM_MEAN, inet.NORM_STD, jitter=True,
                          randaug=desc)
