"""Inception-style ImageNet input on the GPU (csrc/kernels/input_box.hip): the box-resample kernel, the colour
jitter launch and the feeder end to end, element by element against the fp64 reference and the derived
bound of tests/input_refs.py, on sentinel-prefilled outputs between guard elements.

Worst error / bound seen on an MI355X (the bf16 store's half ulp dominates: the fp32 terms are far smaller):
plain launch 0.959, multi-tile 0.981, direct taps 0.959, jitter 0.987 (constant image 0.256), feeder 0.991."""
import itertools

import numpy as np
import pytest
import torch

import input_refs as ir
from kernel_refs import assert_within

from distributed_resnet_tensorflow_amd.data import imagenet as inet
from distributed_resnet_tensorflow_amd.models.spec import imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor
from distributed_resnet_tensorflow_amd.train.feeder import ImagenetFeeder

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -77.0, 64   # (64 bf16 = 128 bytes: the output stays 16-byte aligned)

# (H, W), box (None: the whole image)
CASES = [((37, 53), None),                   # plain non-integer scales
         ((9, 300), None),                   # upscale in y, 12.5x downscale and 25 taps in x
         ((64, 48), (5, 7, 20, 20)),         # pure upscale, interior box
         ((24, 24), None),                   # identity: weights exactly 1 and 0
         ((175, 131), (3, 1, 170, 129)),     # 7x by 5.4x, the box touching no edge
         ((33, 35), (16, 17, 1, 1))]         # a 1 x 1 box: constant output


@pytest.fixture(scope="module")
def hip():
    return HipBackend("cuda")


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw, _ in CASES]
    boxes = [box or (0, 0) + hw for hw, box in CASES]
    return images, boxes


def launch(hip, packed, desc, N, OH, OW, **kw):
    """One box_preprocess on device copies into a sentinel-prefilled output between guards; checks the
    guards, the zero channels and that every pixel was written. Returns [N, OH, OW, 3] (CPU, bf16)."""
    n = N * OH * OW * 8
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    out = buf[GUARD:GUARD + n].view(N, OH, OW, 8)
    hip.box_preprocess(torch.from_numpy(packed).cuda(), torch.from_numpy(desc.view(np.uint8)).cuda(), out,
                       inet.NORM_MEAN, inet.NORM_STD, **kw)
    torch.cuda.synchronize()
    b = buf.cpu()
    assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all()), "guards"
    o = b[GUARD:GUARD + n].view(N, OH, OW, 8)
    assert bool((o[..., 3:] == 0).all()), "channels 3..7"
    assert bool(torch.isfinite(o[..., :3].float()).all())
    return o[..., :3].clone()


def check(o, images, desc, OH, OW, jit, what):
    for i, (img, d) in enumerate(zip(images, desc)):
        ref, bound = ir.box_preprocess(img, d, OH, OW, jit)
        assert_within(o[i], ref, bound, f"{what}: image {i} {img.shape[:2]} box "
                                        f"{tuple(int(d[k]) for k in ('by', 'bx', 'bh', 'bw'))} flip {int(d['flip'])}")


@pytest.mark.parametrize("flip0", [0, 1])
def test_box_kernel_matches_fp64_reference(hip, batch, flip0):
    images, boxes = batch
    packed, desc = ir.pack(images, boxes, [(i + flip0) % 2 for i in range(len(images))])
    assert any(int(o) % 4 for o in desc["offset"])          # the offsets are not aligned
    o = launch(hip, packed, desc, len(images), 24, 24)
    check(o, images, desc, 24, 24, False, "box_preprocess")
    assert bool((o[5] == o[5][0, 0]).all())                 # the 1 x 1 box
    # the identity box is the bf16 rounding of the normalised pixels
    x = (torch.from_numpy(images[3].astype(np.float64)) / 255.0 - torch.tensor(ir.MEAN)) / torch.tensor(ir.STD)
    x = x.flip(1) if desc["flip"][3] else x
    assert_within(o[3], x, (ir.BF + 8 * ir.U) * x.abs() + 4 * ir.U / min(ir.STD), "box_preprocess identity")


@pytest.mark.parametrize("flip", [0, 1])
def test_box_kernel_multi_tile(hip, flip):
    img = np.random.default_rng(12).integers(0, 256, (500, 375, 3), dtype=np.uint8)
    packed, desc = ir.pack([img], [(0, 0, 500, 375)], [flip])
    check(launch(hip, packed, desc, 1, 224, 224), [img], desc, 224, 224, False, "box_preprocess multi-tile")


def test_box_kernel_direct_tap_path(hip, batch):
    """The staged footprint is capped: forced for the six cases, and taken by itself for a box shrunk 16.7x by
    62.5x, whose footprint does not fit."""
    images, boxes = batch
    packed, desc = ir.pack(images, boxes, [i % 2 for i in range(len(images))])
    o = launch(hip, packed, desc, len(images), 24, 24, force_direct=True)
    check(o, images, desc, 24, 24, False, "box_preprocess direct")
    assert torch.equal(o, launch(hip, packed, desc, len(images), 24, 24))   # the same arithmetic on both paths
    big = np.random.default_rng(13).integers(0, 256, (400, 1500, 3), dtype=np.uint8)
    packed, desc = ir.pack([images[0], big], [boxes[0], (0, 0, 400, 1500)], [0, 1])
    check(launch(hip, packed, desc, 2, 24, 24), [images[0], big], desc, 24, 24, False, "box_preprocess direct (cap)")


FACTORS = (0.6, 1.0, 1.4)


@pytest.mark.parametrize("ops", inet.COLOR_ORDERS)
def test_jitter_matches_fp64_reference(hip, batch, ops):
    images, boxes = batch
    const = np.empty((20, 30, 3), dtype=np.uint8)
    const[...] = (200, 100, 50)
    images, boxes = images + [const], boxes + [(0, 0, 20, 30)]
    combos = list(itertools.product(FACTORS, repeat=3))
    k0 = 5 * inet.COLOR_ORDERS.index(ops)
    jit = [(ops,) + combos[(k0 + 4 * i) % len(combos)] for i in range(len(images))]
    jit[-1] = (ops, 0.6, 1.4, 0.6)
    packed, desc = ir.pack(images, boxes, [i % 2 for i in range(len(images))], jit)
    o = launch(hip, packed, desc, len(images), 24, 24, jitter=True)
    check(o, images, desc, 24, 24, True, "box_preprocess jitter")
    # the constant image: gray and mean gray are the same known number; contrast and saturation see it
    x = torch.tensor([200.0, 100.0, 50.0], dtype=torch.float64) / 255.0
    e0 = ir.resample(const, (0, 0, 20, 30), 24, 24)[1]     # (the resample's bound; its value is x exactly)
    ref, bound = ir.normalise(*ir.jitter(x.expand(24, 24, 3), e0, ops, 0.6, 1.4, 0.6), 0)
    assert_within(o[-1], ref, bound, "box_preprocess jitter constant image")
    assert torch.equal(o, launch(hip, packed, desc, len(images), 24, 24, jitter=True)), "two runs differ"


def test_jitter_with_unit_factors_is_the_plain_launch(hip, batch):
    images, boxes = batch
    flips = [i % 2 for i in range(len(images))]
    plain_packed, plain_desc = ir.pack(images, boxes, flips)
    plain = launch(hip, plain_packed, plain_desc, len(images), 24, 24)
    for ops in inet.COLOR_ORDERS:
        packed, desc = ir.pack(images, boxes, flips, [(ops, 1.0, 1.0, 1.0)] * len(images))
        assert torch.equal(launch(hip, packed, desc, len(images), 24, 24, jitter=True), plain), ops
    img = np.random.default_rng(14).integers(0, 256, (300, 260, 3), dtype=np.uint8)     # several tiles
    packed, desc = ir.pack([img], [(10, 20, 250, 200)], [1])
    assert torch.equal(launch(hip, packed, desc, 1, 224, 224, jitter=True), launch(hip, packed, desc, 1, 224, 224))


def test_box_kernel_rejects_bad_arguments_and_descriptors(hip, batch):
    images, boxes = batch
    packed, desc = ir.pack(images[:2], boxes[:2], [0, 0])
    out = torch.zeros(2, 24, 24, 8, dtype=torch.bfloat16, device="cuda")
    dp, dd = torch.from_numpy(packed).cuda(), torch.from_numpy(desc.view(np.uint8)).cuda()
    L = hip.L
    ms = [float(v) for v in inet.NORM_MEAN + inet.NORM_STD]
    assert L.drn_box_preprocess(dp.data_ptr(), dp.numel(), dd.data_ptr(), out.data_ptr(), 2, 24, 24, *ms, 0,
                                hip.stream()) == 0
    assert L.drn_box_preprocess(dp.data_ptr() + 1, dp.numel() - 1, dd.data_ptr(), out.data_ptr(), 2, 24, 24, *ms, 0,
                                hip.stream()) != 0
    assert L.drn_box_preprocess(dp.data_ptr(), dp.numel(), dd.data_ptr(), out.data_ptr(), 0, 24, 24, *ms, 0,
                                hip.stream()) != 0
    assert L.drn_box_desc_size() == inet.BOX_DESC.itemsize
    # a box outside its image, an image outside the buffer: nothing is read, the pixels are NaN
    desc["bh"][0] = 38
    desc["offset"][1] = packed.size - 10
    hip.box_preprocess(dp, torch.from_numpy(desc.view(np.uint8)).cuda(), out, inet.NORM_MEAN, inet.NORM_STD)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[..., :3].float()).all())


def _busy(n=6):
    """~10 ms of GPU work on the current stream: the host runs ahead while it executes."""
    a = torch.randn(4096, 4096, device="cuda")
    for _ in range(n):
        a = torch.tanh(a @ a * 1e-3)
    return a


@pytest.mark.parametrize("train,jit,ahead", [(True, 0.4, True), (True, 0.0, False), (False, 0.0, True)])
def test_feeder_end_to_end(tmp_path, train, jit, ahead):
    inet.write_fake_imagenet(str(tmp_path), shards=2, per_shard=6, is_training=train)
    N, steps = 4, 5 if train else 3

    def loader(pin):
        return inet.ImagenetLoader(str(tmp_path), N, train, seed=2, num_threads=2, pin=pin,
                                   pin_device=torch.device("cuda") if pin else None, preprocessing="inception",
                                   color_jitter=jit, num_epochs=None if train else 1)

    ref_ld = loader(False)
    batches = [tuple(np.array(x, copy=True) for x in next(ref_ld)) for _ in range(steps)]
    ref_ld.close()
    ex = Executor(imagenet_resnet_v2(18), N, HipBackend(), "cuda")
    f = ImagenetFeeder(ex, loader(True), train)
    hist_img = torch.empty(steps, N, 224, 224, 8, dtype=torch.bfloat16, device="cuda")
    hist_lab = torch.empty(steps, N, dtype=torch.int32, device="cuda")
    for k in range(steps):
        assert f.next()
        hist_img[k].copy_(ex.images)
        hist_lab[k].copy_(ex.labels)
        if ahead:
            _busy()
    torch.cuda.synchronize()
    f.close()
    hist = hist_img.cpu()
    assert bool((hist[..., 3:] == 0).all())
    for k, (packed, desc, labels) in enumerate(batches):
        assert desc.dtype == inet.BOX_DESC
        np.testing.assert_array_equal(hist_lab[k].cpu().numpy(), labels, err_msg=f"labels of batch {k}")
        for i, r in enumerate(desc):
            o, H, W = int(r["offset"]), int(r["H"]), int(r["W"])
            ref, bound = ir.box_preprocess(packed[o:o + H * W * 3].reshape(H, W, 3), r, 224, 224, train and jit > 0)
            assert_within(hist[k, i, :, :, :3], ref, bound, f"box_preprocess feeder: batch {k} image {i}")
