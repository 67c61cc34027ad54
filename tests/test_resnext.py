"""ResNeXt (grouped bottleneck 3x3): the spec, the reference executor against oracle autograd, the
flags and the checkpoint .meta; no GPU."""
import json

import pytest
import torch

from distributed_resnet_tensorflow_amd.models import oracle
from distributed_resnet_tensorflow_amd.models.spec import build_spec, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor


def test_spec_names_shapes_and_parameter_count():
    spec = build_spec("imagenet", 50, model="resnext")
    assert spec.name == "resnext50_32x4d"
    plain = build_spec("imagenet", 50)
    assert [v[0] for v in spec.trainable_variables()] == [v[0] for v in plain.trainable_variables()]
    for stage, (mid, cg) in enumerate(((128, 4), (256, 8), (512, 16), (1024, 32)), start=1):
        blk = next(b for b in spec.blocks if b.stage == stage)
        c1, c2, c3 = blk.convs
        assert (c1.groups, c2.groups, c3.groups, blk.proj.groups) == (1, 32, 1, 1)
        assert (c1.cout, c2.cin, c2.cout, c3.cin, c3.cout) == (mid, mid, mid, mid, 256 * 2 ** (stage - 1))
        shapes = {n: s for n, s, _, _ in spec.trainable_variables()}
        assert shapes[f"{c2.name}/kernel"] == (3, 3, cg, mid)
        assert c2.params == 9 * cg * mid
    # the first bottleneck by hand: bn1, projection, 1x1, bn2, grouped 3x3, bn3, 1x1
    blk = spec.blocks[0]
    names = {f"{o.name}/" for o in [blk.bn1, blk.proj] + blk.convs + blk.bns}
    got = sum(torch.Size(s).numel() for n, s, _, _ in spec.trainable_variables() if n[:n.index("/") + 1] in names)
    assert got == 2 * 64 + 64 * 256 + 64 * 128 + 2 * 128 + 9 * 4 * 128 + 2 * 128 + 128 * 256


def test_reference_executor_matches_oracle_autograd():
    """As tests/test_executor.py (fp64, 1e-9), on a tiny ResNeXt."""
    spec, N, dtype, tol = imagenet_resnet_v2(50, num_classes=7, image_size=64, groups=32, width_per_group=4), 4, \
        torch.float64, 1e-9
    torch.manual_seed(0)
    ex = Executor(spec, N, RefBackend(dtype=dtype), "cpu", seed=1)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 64, 64, 3, dtype=dtype)
    labels = torch.randint(0, spec.num_classes, (N,))
    ex.labels.copy_(labels.int())
    p, st = oracle.params_from_store(ex.P), oracle.state_from_store(ex.P)
    ex.forward(train=True)
    ex.backward()
    logits, xent, _ = oracle.loss_fn(spec, p, st, ex.images, labels)
    xent.backward()
    assert torch.allclose(logits, ex.logits, atol=tol * 10, rtol=tol * 10)
    for s in ex.P.slots:
        g_ex, g_or = ex.P.to_tf(s.name, buf=ex.P.grad, dtype=dtype), p[s.name].grad
        err = ((g_ex - g_or).norm() / (g_or.norm() + 1e-30)).item()
        assert err < tol, (s.name, err)


def test_flags_and_meta_round_trip(tmp_path):
    from distributed_resnet_tensorflow_amd import flags
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.cli import entry_flags
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = entry_flags("imagenet_main", ["--model=resnext"])
    assert (F.cardinality, F.width_per_group) == (32, 4)
    assert model_spec_from_flags(F).name == "resnext50_32x4d"
    F = entry_flags("imagenet_main", ["--model=resnext", "--cardinality=16", "--width_per_group=8", "--resnet_size=101"])
    spec = model_spec_from_flags(F)
    assert spec.name == "resnext101_16x8d"
    with pytest.raises(flags.FlagsError):
        entry_flags("imagenet_main", ["--model=resnext", "--cardinality=1"])
    meta = _meta(F, spec)
    assert (meta["cardinality"], meta["width_per_group"]) == (16, 8)
    (tmp_path / "model.ckpt-1.meta").write_text(json.dumps(meta))
    back = Saver.restore_meta(str(tmp_path / "model.ckpt-1"))
    assert (back["model"], back["cardinality"], back["width_per_group"]) == ("resnext", 16, 8)
    plain = _meta(entry_flags("imagenet_main", []), build_spec("imagenet", 50))
    assert "cardinality" not in plain and "width_per_group" not in plain   # absent = a plain ResNet


def test_hip_backend_refuses_unsupported_group_width_without_a_device():
    """32x8d's stage 4 has 64-wide groups: refused when the executor is built on the HIP backend (the
    check needs no GPU); the reference backend builds it."""
    spec = imagenet_resnet_v2(50, num_classes=10, image_size=64, groups=32, width_per_group=8)
    with pytest.raises(ValueError, match="64 channels.*HIP backend"):
        Executor(spec, 2, HipBackend.__new__(HipBackend), "cpu")
    Executor(spec, 2, RefBackend(), "cpu", seed=0)
