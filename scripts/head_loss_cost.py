"""Cost of the label-smoothing / top-k loss kernel (drn_softmax_xent_ex) against the existing
drn_softmax_xent, at the benchmark's head shape (128 x 1001) and the CIFAR one (128 x 10), for
(eps, k) = (0, 1), (0.1, 1), (0.1, 5). Both kernels are a few microseconds of launch-bound work, so
each timed window is one replay of a HIP graph of `--burst` back-to-back launches (no host enqueue
cost in the window, as in a graph / plan step) between two device events, and the figure is the
median (and minimum) over `--iters` windows, per launch; the two kernels alternate window by window.
Writes profiles/head_loss_cost.txt (--out). A record, not a gate.

    python scripts/head_loss_cost.py [--out FILE] [--iters 50] [--burst 200]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.ops.backend import HipBackend  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

SHAPES = [(128, 1001), (128, 10)]
VARIANTS = [(0.0, 1), (0.1, 1), (0.1, 5)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "head_loss_cost.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--burst", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_loss_cost.py times HIP kernels: it needs a GPU")
    be = HipBackend("cuda")
    lines = [f"softmax cross-entropy head kernels, {torch.cuda.get_device_name(0)}; us per launch, median (min) of "
             f"{a.iters} replays of a HIP graph of {a.burst} back-to-back launches (same buffers, cache-warm), the "
             f"two kernels alternating; every launch writes dlogits, loss and correct (and correct_k at k = 5)"]
    g = torch.Generator().manual_seed(0)
    for N, K in SHAPES:
        z = (torch.randn(N, K, generator=g) * 3).cuda()
        labels = torch.randint(0, K, (N,), generator=g, dtype=torch.int32).cuda()
        dl, loss = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        c, ck = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        for eps, k in VARIANTS:
            old = lambda: be.softmax_xent(z, labels, 1.0 / N, dl, loss, c)  # noqa: E731
            new = lambda: be.softmax_xent_ex(z, labels, 1.0 / N, dl, loss, c, smoothing=eps, top_k=k,  # noqa: E731
                                             correct_k=ck if k > 1 else None)
            (om, olo), (nm, nlo) = timed([old, new], a.iters, a.burst)
            lines.append(f"{N} x {K}  eps {eps:g} k {k}:  softmax_xent {om:.2f} ({olo:.2f})   softmax_xent_ex "
                         f"{nm:.2f} ({nlo:.2f})   ratio {nm / om:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
