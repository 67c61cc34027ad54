"""Cost of the ImageNet input preprocessing on the GPU, per batch of 128 synthetic decoded images (one run with
500 x 375 images, one with 1000 x 750), the random-resized-crop boxes, flips and colour factors drawn with a
fixed seed (data.imagenet.draw_box / draw_jitter, --color_jitter=0.4):

  (a) box_preprocess, jitter off (one launch: csrc/kernels/input_box.hip);
  (b) box_preprocess, jitter on (two launches and an fp32 scratch copy);
  (c) vgg_preprocess on the same batch with its own draws (csrc/kernels/augment.hip; orientation only: a
      2 x 2-tap filter without anti-aliasing does less work per pixel);
  (d) the torch composition of (a): per image crop, F.interpolate(bilinear, antialias=True), flip, normalise,
      cast into the NHWC8 bf16 batch.

As in scripts/mix_step_cost.py each timed window is one replay of a HIP graph (of `--burst` back-to-back calls
for a-c, of one pass over the batch for d) between two device events, after warm-up replays, the candidates
alternating window by window; a figure is the median over `--iters` windows, and the whole measurement is
repeated `--repeats` times: the spread is max - min of those medians. Every candidate reads the same packed
device buffer and writes its own output buffer. Writes profiles/input_preprocess_cost.txt (--out).

    python scripts/input_preprocess_cost.py [--out FILE] [--iters 20] [--burst 10] [--repeats 3]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.data import imagenet as inet  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

N, OUT, JITTER = 128, 224, 0.4
SIZES = [(500, 375), (1000, 750)]


def window_us(graph, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def timed(graphs, calls, iters, warmup=3):
    """Median microseconds per call of each graph, the graphs alternating window by window."""
    for g, c in zip(graphs, calls):
        for _ in range(warmup):
            window_us(g, c)
    us = [[] for _ in graphs]
    for _ in range(iters):
        for i, (g, c) in enumerate(zip(graphs, calls)):
            us[i].append(window_us(g, c))
    return [sorted(u)[len(u) // 2] for u in us]


def make_batch(H, W, seed=0):
    rng = np.random.default_rng(seed)
    packed = rng.integers(0, 256, N * H * W * 3, dtype=np.uint8)
    box, vgg = np.zeros(N, dtype=inet.BOX_DESC), np.zeros(N, dtype=inet.IMG_DESC)
    for i in range(N):
        off = i * H * W * 3
        box[i] = (off, H, W) + inet.draw_box(H, W, True, rng) + inet.draw_jitter(JITTER, rng) + ((0, 0, 0),)
        vgg[i] = (off, H, W) + inet.draw_geometry(H, W, True, rng) + (0,)
    return packed, box, vgg


def torch_composition(d_packed, box, out, mean, std):
    for i, r in enumerate(box):
        off, H, W = int(r["offset"]), int(r["H"]), int(r["W"])
        by, bx, bh, bw = (int(r[k]) for k in ("by", "bx", "bh", "bw"))
        crop = d_packed[off:off + H * W * 3].view(H, W, 3)[by:by + bh, bx:bx + bw].permute(2, 0, 1)[None].float()
        x = F.interpolate(crop, size=(OUT, OUT), mode="bilinear", align_corners=False, antialias=True)[0]
        if int(r["flip"]):
            x = x.flip(2)
        out[i, :, :, :3] = ((x * (1.0 / 255.0) - mean) / std).permute(1, 2, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "input_preprocess_cost.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_preprocess_cost.py times HIP kernels: it needs a GPU")
    be = HipBackend("cuda")
    mean = torch.tensor(inet.NORM_MEAN, device="cuda").view(3, 1, 1)
    std = torch.tensor(inet.NORM_STD, device="cuda").view(3, 1, 1)
    lines = [f"ImageNet input preprocessing, {torch.cuda.get_device_name(0)}; us per batch of {N} decoded images -> "
             f"{N} x {OUT} x {OUT} x 8 bf16; median of {a.iters} replays of a HIP graph ({a.burst} back-to-back calls; "
             f"one pass for the torch composition), candidates alternating; {a.repeats} repeats, spread = max - min",
             f"boxes: random-resized crop, area U(0.08, 1), ratio [3/4, 4/3], seed 0; colour jitter {JITTER}"]
    for H, W in SIZES:
        packed, box, vgg = make_batch(H, W)
        d_packed = torch.from_numpy(packed).cuda()
        d_box, d_vgg = torch.from_numpy(box.view(np.uint8)).cuda(), torch.from_numpy(vgg.view(np.uint8)).cuda()
        outs = [torch.zeros(N, OUT, OUT, 8, dtype=torch.bfloat16, device="cuda") for _ in range(4)]
        fns = [lambda: be.box_preprocess(d_packed, d_box, outs[0], inet.NORM_MEAN, inet.NORM_STD),
               lambda: be.box_preprocess(d_packed, d_box, outs[1], inet.NORM_MEAN, inet.NORM_STD, jitter=True),
               lambda: be.vgg_preprocess(d_packed, d_vgg, outs[2], inet.RGB_MEANS),
               lambda: torch_composition(d_packed, box, outs[3], mean, std)]
        calls = [a.burst, a.burst, a.burst, 1]
        graphs = [StepGraph(lambda fn=fn, c=c: [fn() for _ in range(c)], warmup=1) for fn, c in zip(fns, calls)]
        torch.cuda.synchronize()
        # the kernel and the torch composition compute the same images (bf16 rounding apart)
        diff = (outs[0][..., :3].float() - outs[3][..., :3].float()).abs().max().item()
        reps = [timed(graphs, calls, a.iters) for _ in range(a.repeats)]
        scale = np.sqrt(np.mean(box["bh"].astype(np.float64) * box["bw"]) / (OUT * OUT))
        lines.append(f"{H} x {W} images ({packed.size / 1e6:.0f} MB packed; mean box {box['bh'].mean():.0f} x "
                     f"{box['bw'].mean():.0f}, ~{scale:.1f}x shrink per axis); max |kernel - torch| = {diff:.4f}")
        med = []
        for k, name in enumerate(("(a) box_preprocess", "(b) box_preprocess + jitter", "(c) vgg_preprocess",
                                  "(d) torch composition")):
            v = [r[k] for r in reps]
            med.append(sorted(v)[len(v) // 2])
            lines.append(f"  {name:<28} {med[-1]:9.1f} us   repeats " + " ".join(f"{x:.1f}" for x in v)
                         + f"   spread {max(v) - min(v):.1f}")
        lines.append(f"  (d) / (a) = {med[3] / med[0]:.1f}x   (d) / (b) = {med[3] / med[1]:.1f}x   "
                     f"(a) / (c) = {med[0] / med[2]:.2f}x   (b) / (a) = {med[1] / med[0]:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
