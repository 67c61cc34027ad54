"""Cost of RandAugment on the GPU (csrc/kernels/randaug.hip), per batch of 128 images of 224 x 224, beside
box_color_kernel (csrc/kernels/input_box.hip), the launch it replaces, on the same resampled batch:

  (a) box_color_kernel alone (colour jitter 0.4, factors drawn with a fixed seed);
  (b) randaug_kernel alone with every image running the same chain of 1, 2 and 3 operations, once made only of
      in-LDS operations (Equalize | + Contrast | + Color) and once only of gather operations, which go through
      the global slab (Rotate | + ShearX | + Sharpness), all at magnitude 9;
  (c) randaug_kernel alone with chains of 1, 2 and 3 operations drawn by data.randaug.RandAugSampler (seed 0);
  (d) the whole box_preprocess call: plain, with jitter, with the drawn two-operation chains.

As in scripts/input_preprocess_cost.py each timed window is one replay of a HIP graph of `--burst` back-to-back
calls between two device events, after warm-up replays, the candidates alternating window by window; a figure is
the median over `--iters` windows, and the whole measurement is repeated `--repeats` times: the spread is max - min
of those medians. Writes profiles/randaug_cost.txt (--out).

    python scripts/randaug_cost.py [--out FILE] [--iters 20] [--burst 10] [--repeats 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.data import imagenet as inet  # noqa: E402
from distributed_resnet_tensorflow_amd.data import randaug as ra  # noqa: E402
from distributed_resnet_tensorflow_amd.ops import _lib  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

N, OUT, JITTER, MAG, H, W = 128, 224, 0.4, 9, 500, 375
IN_LDS = [ra.EQUALIZE, ra.CONTRAST, ra.COLOR]
GATHER = [ra.ROTATE, ra.SHEAR_X, ra.SHARPNESS]


def window_us(graph, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def timed(graphs, calls, iters, warmup=3):
    """Median microseconds per call of each graph, the graphs alternating window by window."""
    for g in graphs:
        for _ in range(warmup):
            window_us(g, calls)
    us = [[] for _ in graphs]
    for _ in range(iters):
        for i, g in enumerate(graphs):
            us[i].append(window_us(g, calls))
    return [sorted(u)[len(u) // 2] for u in us]


def dev(a):
    return torch.from_numpy(a.view(np.uint8)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "randaug_cost.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_cost.py times HIP kernels: it needs a GPU")
    be = HipBackend("cuda")
    rng = np.random.default_rng(0)
    packed = torch.from_numpy(rng.integers(0, 256, N * H * W * 3, dtype=np.uint8)).cuda()
    box = np.zeros(N, dtype=inet.BOX_DESC)
    for i in range(N):
        box[i] = (i * H * W * 3, H, W) + inet.draw_box(H, W, True, rng) + inet.draw_jitter(JITTER, rng) + ((0, 0, 0),)
    d_box = dev(box)
    mean, std = inet.NORM_MEAN, inet.NORM_STD
    ms = [float(v) for v in mean + std]
    out = [torch.zeros(N, OUT, OUT, 8, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    be.box_preprocess(packed, d_box, out[0], mean, std, jitter=True)      # fills the fp32 copy every kernel reads
    scratch, partial = be._box_workspace(N, OUT, OUT, out[0].device)

    def color():
        _lib.check(be.L.drn_box_color(scratch.data_ptr(), partial.data_ptr(), d_box.data_ptr(), out[1].data_ptr(), N,
                                      OUT, OUT, *ms, be.stream()), "drn_box_color")

    names, fns = ["(a) box_color_kernel"], [color]
    for tag, ops in (("in-LDS", IN_LDS), ("gather", GATHER)):
        for k in (1, 2, 3):
            d = dev(ra.make_desc([[(o, MAG, False) for o in ops[:k]]] * N, OUT))
            names.append(f"(b) randaug {tag} x{k} ({' + '.join(ra.OPS[o] for o in ops[:k])})")
            fns.append(lambda d=d: be.randaug(scratch, d, out[1], mean, std))
    drawn = {}
    for k in (1, 2, 3):
        drawn[k] = dev(ra.RandAugSampler(N, OUT, k, MAG, seed=0).draw(0))
        names.append(f"(c) randaug drawn chains, {k} layer{'s' * (k > 1)}")
        fns.append(lambda d=drawn[k]: be.randaug(scratch, d, out[1], mean, std))
    names += ["(d) box_preprocess", "(d) box_preprocess + jitter", "(d) box_preprocess + randaug (2 layers)"]
    fns += [lambda: be.box_preprocess(packed, d_box, out[1], mean, std),
            lambda: be.box_preprocess(packed, d_box, out[1], mean, std, jitter=True),
            lambda: be.box_preprocess(packed, d_box, out[1], mean, std, randaug=drawn[2])]
    graphs = [StepGraph(lambda fn=fn: [fn() for _ in range(a.burst)], warmup=1) for fn in fns]
    torch.cuda.synchronize()
    reps = [timed(graphs, a.burst, a.iters) for _ in range(a.repeats)]
    lines = [f"RandAugment cost, {torch.cuda.get_device_name(0)}; us per batch of {N} images, {OUT} x {OUT} -> "
             f"{N} x {OUT} x {OUT} x 8 bf16; median of {a.iters} replays of a HIP graph ({a.burst} back-to-back calls), "
             f"candidates alternating; {a.repeats} repeats, spread = max - min",
             f"input: {H} x {W} random images, random-resized-crop boxes (seed 0); magnitude {MAG}; (a)-(c) read the "
             f"same fp32 resampled copy ({N * OUT * OUT * 16 / 1e6:.0f} MB) and write {N * OUT * OUT * 16 / 1e6:.0f} MB"]
    med = []
    for k, name in enumerate(names):
        v = [r[k] for r in reps]
        med.append(sorted(v)[len(v) // 2])
        lines.append(f"  {name:<58} {med[-1]:9.1f} us   repeats " + " ".join(f"{x:.1f}" for x in v)
                     + f"   spread {max(v) - min(v):.1f}   x(a) {med[-1] / med[0]:.2f}")
    lines.append("not measured: the eager ResNet-50 step through the feeder with --rand_augment_layers on and off")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
