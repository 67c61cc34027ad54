"""ResNet-C deep stem (--deep_stem): the spec, the flags and the checkpoint .meta, and the reference executor
(fused and composed forward) against oracle autograd; no GPU."""
import json

import pytest
import torch

from distributed_resnet_tensorflow_amd.models import oracle
from distributed_resnet_tensorflow_amd.models.spec import build_spec, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor


def test_spec_variables_counts_and_refusals():
    d, plain = build_spec("imagenet", 50, deep_stem=True), build_spec("imagenet", 50)
    assert [v[:2] for v in d.trainable_variables()[:8]] == [
        ("conv2d/kernel", (3, 3, 3, 32)), ("batch_normalization/gamma", (32,)), ("batch_normalization/beta", (32,)),
        ("conv2d_1/kernel", (3, 3, 32, 32)), ("batch_normalization_1/gamma", (32,)),
        ("batch_normalization_1/beta", (32,)), ("conv2d_2/kernel", (3, 3, 32, 64)),
        ("batch_normalization_2/gamma", (64,))]
    # the blocks follow unchanged, their names counted on
    assert [v[1] for v in d.trainable_variables()[7:]] == [v[1] for v in plain.trainable_variables()[1:]]
    assert d.num_params() == plain.num_params() + 19_232 and d.name == "imagenet_resnet50_v2_deepstem"
    assert (d.stem_hw, d.pool_hw, d.maxpool) == (plain.stem_hw, plain.pool_hw, True) == (112, 56, True)
    assert [b.name for b in d.batch_norms()[:3]] == ["batch_normalization", "batch_normalization_1",
                                                     "batch_normalization_2"]
    assert [c.name for c in d.convs()[:3]] == ["conv2d", "conv2d_1", "conv2d_2"] and not plain.stem_pre
    stem_flops = 2 * 112 * 112 * (27 * 32 + 288 * 32 + 288 * 64)
    assert d.forward_flops() - plain.forward_flops() == stem_flops - 2 * 112 * 112 * 147 * 64
    assert build_spec("imagenet", 50, model="resnext", avg_down=True, se_ratio=16, deep_stem=True).name == \
        "se_resnext50_32x4d_avgdown_deepstem"
    with pytest.raises(ValueError, match="ImageNet"):
        build_spec("cifar10", 8, deep_stem=True)
    with pytest.raises(ValueError, match="odd"):
        imagenet_resnet_v2(18, image_size=33, deep_stem=True)


def test_flags_and_meta_round_trip(tmp_path):
    from distributed_resnet_tensorflow_amd import flags
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.cli import entry_flags
    from distributed_resnet_tensorflow_amd.train.evaluator import checkpoint_deep_stem
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = entry_flags("imagenet_main", ["--deep_stem", "--avg_down=True"])
    spec = model_spec_from_flags(F)
    assert spec.name == "imagenet_resnet50_v2_avgdown_deepstem" and len(spec.stem_pre) == 2
    for entry, argv in (("imagenet_main", ["--deep_stem", "--model=lrnet"]), ("cifar_main", ["--deep_stem"])):
        with pytest.raises(flags.FlagsError):
            entry_flags(entry, argv)
    meta = _meta(F, spec)
    assert meta["deep_stem"] is True
    (tmp_path / "model.ckpt-1.meta").write_text(json.dumps(meta))
    prefix = str(tmp_path / "model.ckpt-1")
    assert Saver.restore_meta(prefix)["deep_stem"] is True
    plain = entry_flags("imagenet_main", [])
    assert plain.deep_stem is False and "deep_stem" not in _meta(plain, model_spec_from_flags(plain))   # absent = off
    assert Saver.restore_meta(str(tmp_path / "none"))["deep_stem"] is False
    # the evaluator takes the stem from the .meta; an explicit flag that contradicts it is an error
    assert checkpoint_deep_stem(entry_flags("imagenet_eval_main", []), prefix) is True
    with pytest.raises(flags.FlagsError, match="contradicts"):
        checkpoint_deep_stem(entry_flags("imagenet_eval_main", ["--deep_stem=False"]), prefix)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_reference_executor_matches_oracle_autograd(monkeypatch, fused):
    """As tests/test_avg_down.py (fp64, 1e-9): a deep-stem ResNet-18 at 32 px, N = 2, loss and every gradient,
    through the fused entry points' reference contract and through the composed forward."""
    monkeypatch.setenv("DRN_DEEP_STEM_FUSED", fused)
    spec, N, dtype, tol = imagenet_resnet_v2(18, num_classes=7, image_size=32, deep_stem=True), 2, torch.float64, 1e-9
    torch.manual_seed(0)
    ex = Executor(spec, N, RefBackend(dtype=dtype), "cpu", seed=1)
    assert ex.deep and ex.deep_fused == (fused == "1") and ex._stem_hi == 0
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
    for s in ex.P.slots:
        g_ex, g_or = ex.P.to_tf(s.name, buf=ex.P.grad, dtype=dtype), p[s.name].grad
        err = ((g_ex - g_or).norm() / (g_or.norm() + 1e-30)).item()
        assert err < tol, (s.name, err)


def test_hip_backend_refuses_outside_the_domain_without_a_device():
    assert HipBackend.stem_deep_check((2, 7, 9, 8), (32, 3, 3, 8), 2) == (4, 5)
    for x, w, s in (((2, 8, 8, 16), (32, 3, 3, 16), 1), ((2, 8, 8, 32), (48, 3, 3, 32), 1), ((2, 8, 8, 32), (64, 3, 3, 32), 3)):
        with pytest.raises(ValueError, match="deep-stem"):
            HipBackend.stem_deep_check(x, w, s)
