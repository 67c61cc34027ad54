"""Cost of Mixup / CutMix in a training step: the in-place pair-mix kernel (drn_mix_pairs) at the ImageNet
and CIFAR batch shapes (128 x 224 x 224 x 8 and 128 x 32 x 32 x 8, bf16), for Mixup (lam = 0.7) and for
CutMix with a centred quarter-area box, against the torch expression torch.lerp(x.flip(0), x, lam) on the
same tensor; and the mixed-target loss kernel (drn_softmax_xent_mix) against drn_softmax_xent_ex at the
head shapes 128 x 1001 and 128 x 10. As in scripts/head_loss_cost.py each timed window is one replay of a
HIP graph of `--burst` back-to-back launches between two device events; the figure is the median (and
minimum) over `--iters` windows, per launch, the candidates alternating window by window. GB/s counts the
bytes the launch has to move: every image read and written once for Mixup, the box bytes for CutMix.
Writes profiles/mix_step_cost.txt (--out). A record, not a gate.

    python scripts/mix_step_cost.py [--out FILE] [--iters 30] [--burst 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, mix_identity, mix_table_tensor  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

IMAGE_SHAPES = [(128, 224, 224), (128, 32, 32)]
HEAD_SHAPES = [(128, 1001), (128, 10)]
LAM = 0.7


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def timed(fns, iters, burst, warmup=3):
    """Median and minimum microseconds per launch of each fn, the fns alternating window by window."""
    graphs = [StepGraph(lambda fn=fn: [fn() for _ in range(burst)], warmup=1) for fn in fns]
    for g in graphs:
        for _ in range(warmup):
            window_us(g, burst)
    us = [[] for _ in fns]
    for _ in range(iters):
        for i, g in enumerate(graphs):
            us[i].append(window_us(g, burst))
    return [(sorted(u)[len(u) // 2], min(u)) for u in us]


def tables(N, H, W):
    mixup = mix_identity(N)
    mixup["w"] = mixup["lam"] = LAM
    cut = mix_identity(N)
    cut["y0"], cut["x0"], cut["y1"], cut["x1"] = H // 4, W // 4, H // 4 + H // 2, W // 4 + W // 2
    cut["lam"] = 0.75
    return mixup, cut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mix_step_cost.txt"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_step_cost.py times HIP kernels: it needs a GPU")
    be = HipBackend("cuda")
    lines = [f"Mixup / CutMix kernels, {torch.cuda.get_device_name(0)}; us per launch, median (min) of {a.iters} "
             f"replays of a HIP graph of {a.burst} back-to-back launches, the candidates alternating",
             f"mix_pairs in place (bf16, 8 stored channels) vs torch.lerp(x.flip(0), x, lam) into a second buffer; "
             f"Mixup lam = {LAM}, CutMix a centred box of a quarter of the image; GB/s = bytes the mix has to move "
             f"(Mixup: every image read and written; CutMix: the boxes read and written) / time"]
    g = torch.Generator().manual_seed(0)
    for N, H, W in IMAGE_SHAPES:
        x = torch.zeros(N, H, W, 8, dtype=torch.bfloat16, device="cuda")
        x[..., :3] = (torch.rand(N, H, W, 3, generator=g) * 0.5 + 0.5).cuda().bfloat16()   # (stays bounded in place)
        y = torch.empty_like(x)
        nbytes = x.numel() * 2
        mixup, cut = (mix_table_tensor(t).cuda() for t in tables(N, H, W))
        lerp = lambda: torch.lerp(x.flip(0), x, LAM, out=y)  # noqa: E731
        (mm, mlo), (cm, clo), (tm, tlo) = timed([lambda: be.mix_pairs(x, x, mixup), lambda: be.mix_pairs(x, x, cut),
                                                 lerp], a.iters, a.burst)
        lines.append(f"{N} x {H} x {W} x 8  Mixup:  mix_pairs {mm:.1f} ({mlo:.1f}) us, {2 * nbytes / mm / 1e3:.0f} GB/s   "
                     f"torch.lerp {tm:.1f} ({tlo:.1f}) us, {2 * nbytes / tm / 1e3:.0f} GB/s   ratio {mm / tm:.2f}x")
        lines.append(f"{N} x {H} x {W} x 8  CutMix: mix_pairs {cm:.1f} ({clo:.1f}) us, "
                     f"{2 * nbytes / 4 / cm / 1e3:.0f} GB/s of box bytes   (torch.lerp above: {cm / tm:.2f}x)")
    for N, K in HEAD_SHAPES:
        z = (torch.randn(N, K, generator=g) * 3).cuda()
        labels = torch.randint(0, K, (N,), generator=g, dtype=torch.int32).cuda()
        t = mix_identity(N)
        t["w"] = t["lam"] = LAM
        t["label_b"] = np.asarray(labels.cpu())[::-1]
        table = mix_table_tensor(t).cuda()
        dl, loss = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        c, ck = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        ex = lambda: be.softmax_xent_ex(z, labels, 1.0 / N, dl, loss, c, smoothing=0.1, top_k=5, correct_k=ck)  # noqa: E731
        mix = lambda: be.softmax_xent_mix(z, labels, table, 1.0 / N, dl, loss, c, smoothing=0.1, top_k=5,  # noqa: E731
                                          correct_k=ck)
        (em, elo), (xm, xlo) = timed([ex, mix], a.iters, max(a.burst, 200))
        lines.append(f"{N} x {K}  eps 0.1 k 5:  softmax_xent_ex {em:.2f} ({elo:.2f})   softmax_xent_mix {xm:.2f} "
                     f"({xlo:.2f})   ratio {xm / em:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
