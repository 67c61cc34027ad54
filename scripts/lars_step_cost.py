"""Cost of the LARS update against the plain momentum update on the ResNet-50 ImageNet parameter
store (25.6 M parameters, random gradients): 50 event-timed launches of each after warm-up, for
the fp32 gradient and the bf16 wire gradient. Writes profiles/lars_step_cost.txt (--out).

    python scripts/lars_step_cost.py [--out FILE] [--iters 50]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, lars_table  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.params import ParamStore  # noqa: E402


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "lars_step_cost.txt"))
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    be = HipBackend("cuda")
    P = ParamStore(build_spec("imagenet", 50), "cuda", keep_bf16=True, seed=0)
    table = lars_table(P)
    partials = torch.zeros(2 * table.chunks, device="cuda")
    trust = torch.ones(table.n, device="cuda")
    lr = torch.full((1,), 1e-6, device="cuda")
    lines = [f"ResNet-50 ImageNet ParamStore: {P.total} elements, {table.n} slots, {table.chunks} chunks; "
             f"{torch.cuda.get_device_name(0)}; median (min) of {a.iters} back-to-back launches on the same "
             f"buffers (cache-warm), ms"]
    for wire in ("fp32", "bf16"):
        g = torch.randn(P.total, device="cuda") * 1e-3
        g = g if wire == "fp32" else g.bfloat16()
        sgd = timed(lambda: be.sgd_momentum(P.master, P.momentum, g, P.wbf16, lr, 0.9, 1e-4, 1.0), a.iters)
        lars = timed(lambda: be.lars_momentum(P.master, P.momentum, g, P.wbf16, table, 0, table.n, partials, trust,
                                              lr, 0.9, 1e-4, 1.0, 0.001, 1e-9), a.iters)
        gb = P.total * (4 * 5 + 2 + (4 if wire == "fp32" else 2)) / 1e9  # w, m read + written, w_bf16 written, g read
        lines.append(f"grad {wire}: sgd_momentum {sgd[0]:.4f} ({sgd[1]:.4f})  = {gb / sgd[0]:.2f} TB/s   "
                     f"lars_momentum {lars[0]:.4f} ({lars[1]:.4f})   ratio {lars[0] / sgd[0]:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
