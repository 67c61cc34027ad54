"""Squeeze-and-Excitation (--se_ratio): the spec, the reference executor against oracle autograd, the
flags and the checkpoint .meta; no GPU."""
import json

import pytest
import torch

from distributed_resnet_tensorflow_amd.models import oracle
from distributed_resnet_tensorflow_amd.models.spec import build_spec, cifar_resnet_v2, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor


def test_spec_variables_and_parameter_count():
    se, plain = imagenet_resnet_v2(50, 1001, se_ratio=16), imagenet_resnet_v2(50, 1001)
    assert se.name == "se_imagenet_resnet50_v2"
    # per block 2 C C/16 + C/16 + C over 3 x 256, 4 x 512, 6 x 1024, 3 x 2048
    assert se.num_params() - plain.num_params() == 2_530_992
    names = [v[0] for v in se.trainable_variables()]
    assert names[-2:] == ["dense/kernel", "dense/bias"]
    i = names.index("squeeze_excite_1/reduce/kernel")   # right after the second block's last conv
    assert names[i - 1] == f"{se.blocks[1].convs[-1].name}/kernel"
    assert names[i:i + 4] == [f"squeeze_excite_1/{v}" for v in ("reduce/kernel", "reduce/bias", "expand/kernel",
                                                                 "expand/bias")]
    shapes = {n: (s, k) for n, s, k, _ in se.trainable_variables()}
    assert shapes["squeeze_excite_15/reduce/kernel"] == ((2048, 128), "se_w")
    assert shapes["squeeze_excite_15/expand/bias"] == ((2048,), "se_b")
    assert cifar_resnet_v2(8, se_ratio=16).blocks[0].se.hidden == 8   # max(C // r, 8)
    # se_ratio = 0 is today's network: the same variables, kinds and shapes through every entry
    for a, b in ((build_spec("imagenet", 50, se_ratio=0), plain), (build_spec("cifar10", 8, se_ratio=0), cifar_resnet_v2(8))):
        assert [v[:3] for v in a.trainable_variables()] == [v[:3] for v in b.trainable_variables()]
        assert a.name == b.name and all(blk.se is None for blk in a.blocks)
    with pytest.raises(ValueError):
        cifar_resnet_v2(8, se_ratio=3)


def test_reference_executor_matches_oracle_autograd():
    """As tests/test_executor.py::test_cifar_resnet8_fp32 (fp32, 1e-4), on the SE network: logits, loss and
    the gradient of every variable, the four SE ones of each block among them."""
    spec, N, dtype, tol = cifar_resnet_v2(8, se_ratio=4), 4, torch.float32, 1e-4
    torch.manual_seed(0)
    ex = Executor(spec, N, RefBackend(dtype=dtype), "cpu", seed=1)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 32, 32, 3, dtype=dtype)
    labels = torch.randint(0, spec.num_classes, (N,))
    ex.labels.copy_(labels.int())
    p, st = oracle.params_from_store(ex.P), oracle.state_from_store(ex.P)
    ex.forward(train=True)
    ex.backward()
    logits, xent, _ = oracle.loss_fn(spec, p, st, ex.images, labels)
    xent.backward()
    assert torch.allclose(logits, ex.logits, atol=tol * 10, rtol=tol * 10)
    assert abs(xent.item() - ex.loss_vec.mean().item()) < tol * 10
    assert sum(s.kind in ("se_w", "se_b") for s in ex.P.slots) == 4 * len(spec.blocks)
    for s in ex.P.slots:
        g_ex, g_or = ex.P.to_tf(s.name, buf=ex.P.grad, dtype=dtype), p[s.name].grad
        err = ((g_ex - g_or).norm() / (g_or.norm() + 1e-30)).item()
        assert err < tol, (s.name, err)
    for k in st:
        m, v = ex.P.moving(k)
        assert torch.allclose(m, st[k][0], atol=tol) and torch.allclose(v, st[k][1], atol=tol * 10)


def test_flags_and_meta_round_trip(tmp_path):
    from distributed_resnet_tensorflow_amd import flags
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.cli import entry_flags
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = entry_flags("imagenet_main", ["--model=resnext", "--se_ratio=16"])
    spec = model_spec_from_flags(F)
    assert spec.name == "se_resnext50_32x4d" and spec.blocks[-1].se.hidden == 128
    for bad in (["--se_ratio=3"], ["--se_ratio=8", "--model=lrnet"]):
        with pytest.raises(flags.FlagsError):
            entry_flags("imagenet_main", bad)
    meta = _meta(F, spec)
    assert meta["se_ratio"] == 16
    (tmp_path / "model.ckpt-1.meta").write_text(json.dumps(meta))
    assert Saver.restore_meta(str(tmp_path / "model.ckpt-1"))["se_ratio"] == 16
    plain = _meta(entry_flags("imagenet_main", []), build_spec("imagenet", 50))
    assert "se_ratio" not in plain                                  # absent = no gate
    assert Saver.restore_meta(str(tmp_path / "none"))["se_ratio"] == 0


def test_hip_backend_refuses_an_unsupported_gate_without_a_device():
    spec = cifar_resnet_v2(8, se_ratio=4)
    spec.blocks[0].se.hidden = 12   # not a multiple of 8
    with pytest.raises(ValueError, match="squeeze_excite.*HIP backend"):
        Executor(spec, 2, HipBackend.__new__(HipBackend), "cpu")
