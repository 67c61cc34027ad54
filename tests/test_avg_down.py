"""ResNet-D shortcuts (--avg_down): the spec, the fp64 reference executor against oracle autograd, the
flags and the checkpoint .meta; no GPU."""
import json

import pytest
import torch

from distributed_resnet_tensorflow_amd.models import oracle
from distributed_resnet_tensorflow_amd.models.spec import build_spec, cifar_resnet_v2, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor


def test_spec_marks_the_stride_2_projections_only():
    d, plain = build_spec("imagenet", 50, avg_down=True), build_spec("imagenet", 50)
    assert [v[:3] for v in d.trainable_variables()] == [v[:3] for v in plain.trainable_variables()]
    assert d.num_params() == plain.num_params() == 25_551_401 and d.forward_flops() == plain.forward_flops()
    for blk in d.blocks:
        assert blk.avg_down == (blk.proj is not None and blk.stride == 2), (blk.stage, blk.index)
        if blk.proj is not None:   # stage 1's stride-1 projection is untouched, the others convolve at stride 1
            assert (blk.proj.k, blk.proj.stride, blk.out_hw) == (1, 1, blk.in_hw // blk.stride)
    assert [b.stage for b in d.blocks if b.avg_down] == [2, 3, 4]
    assert [b.stage for b in cifar_resnet_v2(8, avg_down=True).blocks if b.avg_down] == [2, 3]
    assert not any(b.avg_down for b in plain.blocks) and plain.blocks[3].proj.stride == 2
    with pytest.raises(ValueError, match="odd"):   # 72 px: stage 3 would pool a 9 x 9 input
        imagenet_resnet_v2(50, image_size=72, avg_down=True)


def test_reference_executor_matches_oracle_autograd():
    """As tests/test_resnext.py (fp64, 1e-9): ResNet-50 topology at 64 px, loss and every gradient."""
    spec, N, dtype, tol = imagenet_resnet_v2(50, num_classes=7, image_size=64, avg_down=True), 4, torch.float64, 1e-9
    torch.manual_seed(0)
    ex = Executor(spec, N, RefBackend(dtype=dtype), "cpu", seed=1)
    assert [bp.ap is not None for bp in ex.blocks] == [b.avg_down for b in spec.blocks]
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
    assert abs(xent.item() - ex.loss_vec.mean().item()) < tol * 10
    for s in ex.P.slots:
        g_ex, g_or = ex.P.to_tf(s.name, buf=ex.P.grad, dtype=dtype), p[s.name].grad
        err = ((g_ex - g_or).norm() / (g_or.norm() + 1e-30)).item()
        assert err < tol, (s.name, err)


def test_flags_and_meta_round_trip(tmp_path):
    from distributed_resnet_tensorflow_amd import flags
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.cli import entry_flags
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = entry_flags("imagenet_main", ["--model=resnext", "--se_ratio=16", "--avg_down=True"])
    spec = model_spec_from_flags(F)
    assert spec.name == "se_resnext50_32x4d_avgdown" and sum(b.avg_down for b in spec.blocks) == 3
    with pytest.raises(flags.FlagsError):
        entry_flags("cifar_main", ["--avg_down=True", "--model=lrnet"])
    meta = _meta(F, spec)
    assert meta["avg_down"] is True
    (tmp_path / "model.ckpt-1.meta").write_text(json.dumps(meta))
    assert Saver.restore_meta(str(tmp_path / "model.ckpt-1"))["avg_down"] is True
    plain = entry_flags("imagenet_main", [])
    assert plain.avg_down is False and "avg_down" not in _meta(plain, model_spec_from_flags(plain))   # absent = off
    assert Saver.restore_meta(str(tmp_path / "none"))["avg_down"] is False


def test_hip_backend_refuses_outside_the_domain_without_a_device():
    check = HipBackend.pool_proj_check
    check((2, 6, 6, 64), (2, 3, 3, 128))
    for x, sc in (((2, 7, 6, 64), (2, 3, 3, 128)), ((2, 6, 6, 60), (2, 3, 3, 128)), ((2, 6, 6, 64), (2, 3, 3, 100))):
        with pytest.raises(ValueError, match="pooled projection"):
            check(x, sc)
    spec = cifar_resnet_v2(8, avg_down=True)
    spec.blocks[1].in_c = 12   # (no builder makes such a net: the executor's build-time refusal alone)
    with pytest.raises(ValueError, match="pooled projection.*HIP backend"):
        Executor(spec, 2, HipBackend.__new__(HipBackend), "cpu")
