"""bench.py --dump-outputs / --full / --steps on one GPU: a plain run prints one result line whose
`steps` and `ms_per_step` describe the timed loop, and the dump holds, as float32 .npy files, one
step of the timed path from the seeded initial state (checked against the known initial weights
and BN moving statistics)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN_DECAY = 0.997


def _bench(args):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--dataset", "cifar10",
           "--resnet_size", "20", "--batch_size", "8"] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=REPO))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_dump_outputs_and_full(tmp_path):
    from distributed_resnet_tensorflow_amd.models.spec import build_spec
    from distributed_resnet_tensorflow_amd.runtime.params import ParamStore
    d = tmp_path / "dump"
    r = _bench(["--steps", "3", "--warmup", "1", "--full", "--dump-outputs", str(d)])
    assert r["steps"] == 3 and r["warmup"] == 1
    assert r["ms_per_step"] > 0 and r["unit"] == "images/sec" and r["higher_is_better"] is True
    # value and ms_per_step describe the same timed loop (both are rounded in the result line)
    assert r["value"] == pytest.approx(8 * 1e3 / r["ms_per_step"], rel=1e-2)
    spec = build_spec("cifar10", 20)
    P = ParamStore(spec, "cpu", keep_bf16=False, seed=1234)   # bench.py's initial state
    w0 = P.master.numpy().copy()
    names = sorted(p.name for p in d.iterdir())
    assert names == ["bn_moving.npy", "loss.npy", "weights.npy"]
    arrays = {n[:-4]: np.load(d / n) for n in names}
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1000 * 1000
    for n, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    assert arrays["loss"].shape == (8,) and arrays["weights"].shape == w0.shape
    assert arrays["bn_moving"].shape == tuple(P.bn_state.shape)
    # random-init 10-class logits: the loss is near ln(10), far from the ~0 of the memorised batch
    # the timed steps end in
    assert 1.0 < float(arrays["loss"].mean()) < 10.0
    # one SGD step (lr 0.1) away from the initial weights, not many
    dw = np.abs(arrays["weights"] - w0).max()
    assert 0 < dw < 0.5, dw
    # one moving-average update of the initial statistics (mean 0, variance 1):
    # mean = (1 - decay) * batch mean, variance = decay + (1 - decay) * batch variance >= decay
    P.bn_state.copy_(torch.from_numpy(arrays["bn_moving"]))
    moved = 0.0
    for bn in spec.batch_norms():
        mean, var = P.moving(bn.name)
        assert float(var.min()) >= BN_DECAY - 1e-6, bn.name
        moved = max(moved, float(mean.abs().max()))
    assert moved > 0
