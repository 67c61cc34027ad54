"""Stochastic depth (--drop_path_rate): the linear rule, the host sampler, the reference backend's operations, the
flags and the checkpoint .meta; no GPU."""
import json

import numpy as np
import pytest
import torch

from distributed_resnet_tensorflow_amd.data.drop_path import DropPathSampler
from distributed_resnet_tensorflow_amd.models.spec import build_spec
from distributed_resnet_tensorflow_amd.ops.backend import RefBackend


def test_linear_rule_on_resnet50():
    d, plain = build_spec("imagenet", 50, drop_path_rate=0.2), build_spec("imagenet", 50)
    assert [v[:3] for v in d.trainable_variables()] == [v[:3] for v in plain.trainable_variables()]
    rates = [b.drop_rate for b in d.blocks]
    assert len(rates) == 16 and rates[0] == 0.0 and rates[15] == 0.2
    assert np.allclose(rates, [0.2 * b / 15 for b in range(16)], rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match="drop_path_rate"):
        build_spec("imagenet", 50, drop_path_rate=1.0)


def test_sampler_is_counter_based():
    rates = [0.0, 0.1, 0.5]
    s = DropPathSampler(4096, rates, seed=7, rank=0)
    t = s.draw(3)
    assert t.shape == (3, 4096) and t.dtype == np.float32
    assert np.array_equal(t, DropPathSampler(4096, rates, seed=7, rank=0).draw(3))
    for other in (DropPathSampler(4096, rates, seed=7, rank=1).draw(3), s.draw(4),
                  DropPathSampler(4096, rates, seed=8, rank=0).draw(3)):
        assert not np.array_equal(t[1:], other[1:])
    for b, p in enumerate(rates):
        assert set(np.unique(t[b])) <= {np.float32(0.0), np.float32(1 / (1 - p))}
        assert abs((t[b] != 0).mean() - (1 - p)) <= 4 * (p * (1 - p) / 4096) ** 0.5


def test_reference_backend_matches_the_formula():
    be, g = RefBackend(dtype=torch.float64), torch.Generator().manual_seed(0)
    u, sc, dout = (torch.randn(3, 2, 2, 8, generator=g, dtype=torch.float64) for _ in range(3))
    f = torch.tensor([2.0, 0.0, 1.25], dtype=torch.float64)
    u[1] = dout[1] = float("nan")   # a dropped sample's branch is not read
    out, du, stats = torch.empty_like(u), torch.empty_like(u), torch.zeros(1, 2, 8, dtype=torch.float64)
    be.drop_path_fwd(u, sc, f, out, stats=stats)
    be.drop_path_bwd(dout, f, du)
    for n, fn in enumerate(f.tolist()):
        assert torch.equal(out[n], sc[n] + fn * u[n] if fn else sc[n])
        assert torch.equal(du[n], fn * dout[n] if fn else torch.zeros_like(du[n]))
    flat = out.reshape(-1, 8)
    assert torch.allclose(stats[0], torch.stack([flat.sum(0), (flat * flat).sum(0)]), rtol=1e-14, atol=0)


def test_flags_and_meta_round_trip(tmp_path):
    from distributed_resnet_tensorflow_amd import flags
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.cli import entry_flags
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = entry_flags("imagenet_main", ["--model=resnext", "--avg_down=True", "--drop_path_rate=0.1"])
    spec = model_spec_from_flags(F)
    assert spec.blocks[-1].drop_rate == 0.1 and spec.blocks[0].drop_rate == 0.0
    for bad in (["--drop_path_rate=1.0"], ["--drop_path_rate=-0.1"], ["--drop_path_rate=0.1", "--model=lrnet"],
                ["--drop_path_rate=0.1", "--se_ratio=8"]):
        with pytest.raises(flags.FlagsError):
            entry_flags("cifar_main", bad)
    (tmp_path / "model.ckpt-1.meta").write_text(json.dumps(_meta(F, spec)))
    assert Saver.restore_meta(str(tmp_path / "model.ckpt-1"))["drop_path_rate"] == 0.1
    plain = entry_flags("imagenet_main", [])
    assert "drop_path_rate" not in _meta(plain, model_spec_from_flags(plain))   # absent = 0
    assert Saver.restore_meta(str(tmp_path / "none"))["drop_path_rate"] == 0.0
