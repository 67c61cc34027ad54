"""Cost of the weight EMA fused into the optimizer kernels, on the ResNet-50 ImageNet parameter store
(25.6 M elements, random gradients), for the momentum and the LARS update and for the fp32 and the
bf16 wire gradient. Three variants per row:

  (a) the plain update (drn_sgd_momentum / drn_lars_momentum),
  (b) the fused EMA update (drn_sgd_momentum_ema / drn_lars_momentum_ema),
  (c) (a) followed by a separate pass ema.lerp_(w, 1 - d) (torch).

Each timed window is one replay of a HIP graph of `--burst` back-to-back updates (no host enqueue
cost in the window, as in a graph / plan step) between two device events; the figure is the median
(and minimum) over `--iters` windows, per update, the three variants alternating window by window.
Writes profiles/ema_step_cost.txt (--out); the accepted outcome is (b) < (c) in every row, and the
file says so either way.

    python scripts/ema_step_cost.py [--out FILE] [--iters 30] [--burst 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, lars_table  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.params import ParamStore  # noqa: E402

DECAY = 0.999


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def timed(fns, iters, burst, warmup=3):
    """Median and minimum microseconds per call of each fn, the fns alternating window by window."""
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
    ap.add_argument("--out", default=os.path.join("profiles", "ema_step_cost.txt"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_step_cost.py times HIP kernels: it needs a GPU")
    be = HipBackend("cuda")
    P = ParamStore(build_spec("imagenet", 50), "cuda", keep_bf16=True, seed=0, ema=True)
    table = lars_table(P)
    partials = torch.zeros(2 * table.chunks, device="cuda")
    trust = torch.ones(table.n, device="cuda")
    lr = torch.full((1,), 1e-6, device="cuda")
    d = torch.full((1,), DECAY, device="cuda")
    lines = [f"ResNet-50 ImageNet ParamStore: {P.total} elements ({table.n} slots); {torch.cuda.get_device_name(0)}; "
             f"us per update, median (min) of {a.iters} replays of a HIP graph of {a.burst} back-to-back updates on "
             f"the same buffers, the three variants alternating. (a) plain update, (b) fused EMA update, (c) plain "
             f"update + a separate ema.lerp_(w, 1 - d) pass"]
    ok = True
    for opt in ("momentum", "lars"):
        for wire in ("fp32", "bf16"):
            g = torch.randn(P.total, device="cuda") * 1e-3
            g = g if wire == "fp32" else g.bfloat16()

            def update(ema=None, g=g):
                kw = dict(ema=ema, ema_decay_t=d) if ema is not None else {}
                if opt == "momentum":
                    be.sgd_momentum(P.master, P.momentum, g, P.wbf16, lr, 0.9, 1e-4, 1.0, **kw)
                else:
                    be.lars_momentum(P.master, P.momentum, g, P.wbf16, table, 0, table.n, partials, trust, lr, 0.9,
                                     1e-4, 1.0, 0.001, 1e-9, **kw)

            plain = update
            fused = lambda: update(P.ema)  # noqa: E731
            separate = lambda: (update(), P.ema.lerp_(P.master, 1.0 - DECAY))  # noqa: E731
            (am, alo), (bm, blo), (cm, clo) = timed([plain, fused, separate], a.iters, a.burst)
            # bytes of (b): w, m, ema read + written, w_bf16 written, g read (LARS: + w, g read by the norms pass)
            gsz = 4 if wire == "fp32" else 2
            gb = P.total * (4 * 6 + 2 + gsz + ((4 + gsz) if opt == "lars" else 0)) / 1e9
            ok = ok and bm < cm
            lines.append(f"{opt:8s} grad {wire}:  (a) {am:.1f} ({alo:.1f})   (b) {bm:.1f} ({blo:.1f}) = "
                         f"{gb / (bm * 1e-6) / 1e3:.2f} TB/s   (c) {cm:.1f} ({clo:.1f})   (b) - (a) {bm - am:+.1f}   "
                         f"(c) - (b) {cm - bm:+.1f}   {'(b) < (c)' if bm < cm else '(b) NOT faster than (c)'}")
    lines.append("accepted: (b) < (c) in every row" if ok else
                 "NOT accepted: the fused EMA update is not faster than the separate pass in every row")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
