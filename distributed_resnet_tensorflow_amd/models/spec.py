"""ResNet v2 (pre-activation) topology specs with TensorFlow-1 variable naming.

One declarative description of the network drives the pure-PyTorch oracle
(``models.oracle``), the static-plan executor (``runtime.executor``), the parameter/FLOP
report (``models.analysis``) and the TensorBundle checkpoint layout (``ckpt``).

Reference semantics reproduced here (resnet_model_official.py):
  * CIFAR 6n+2 generator (:217-278): stem conv3x3/1 -> 16; three stages of n building blocks
    with 16/32/64 filters, strides 1/2/2; final BN-ReLU; global average pool; dense.
  * ImageNet generator (:281-366): stem conv7x7/2 -> 64; max-pool 3x3/2 SAME; four stages
    (64/128/256/512 filters, strides 1/2/2/2) of building (18/34) or bottleneck (50..200)
    blocks; final BN-ReLU; global average pool; dense (1001 classes for ImageNet).
  * The FIRST block of every stage has a 1x1 projection shortcut on the BN-ReLU output, even
    when the shape does not change (:202-209); the stride sits on the 3x3 conv (:166-168).
  * Stride>1 convs use fixed padding ((k-1)//2 before, the rest after) + VALID; stride-1 convs
    use SAME (:53-91). No conv bias.
  * tf.layers auto-naming in creation order: conv2d, conv2d_1, ...; batch_normalization,
    batch_normalization_1, ...; dense. Inside a block the creation order is
    BN1 -> (projection conv) -> conv1 -> BN2 -> conv2 [-> BN3 -> conv3] (:113-130, :153-175).

Extension (not in the reference, labelled as such): ``wide_resnet_50_2`` doubles the bottleneck
inner width (Wide ResNet paper cited in reference README.md:110-112).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional


@dataclass
class Conv:
    name: str           # TF scope, e.g. "conv2d_3" -> variable "conv2d_3/kernel"
    cin: int
    cout: int
    k: int
    stride: int
    cin_store: int = 0  # channels as stored/computed (stem input padded 3 -> 8); 0 = cin
    groups: int = 1     # grouped conv (ResNeXt): output group g reads input channels [g*cin/groups, ...)

    def __post_init__(self):
        if not self.cin_store:
            self.cin_store = self.cin
        if self.groups < 1 or self.cin % self.groups or self.cout % self.groups:
            raise ValueError(f"{self.name}: groups={self.groups} must divide cin={self.cin} and cout={self.cout}")

    @property
    def pad(self) -> int:
        """Leading pad: SAME for stride 1, fixed_padding (k-1)//2 for stride > 1 (same value for odd k)."""
        return (self.k - 1) // 2

    def out_hw(self, h: int) -> int:
        if self.stride == 1:
            return h
        total = self.k - 1
        return (h + total - self.k) // self.stride + 1

    @property
    def params(self) -> int:
        return self.k * self.k * (self.cin // self.groups) * self.cout


@dataclass
class BN:
    name: str  # "batch_normalization_7"
    c: int


@dataclass
class SE:
    """Squeeze-and-Excitation gate on a block's residual branch (extension, SE-PreResNet placement):
    out = shortcut + sigmoid(relu(mean_hw(u) W1 + b1) W2 + b2) * u, u the last main-path conv's output."""
    name: str   # TF scope "squeeze_excite_3" -> variables ".../reduce/kernel", ".../expand/bias", ...
    c: int
    hidden: int


@dataclass
class Block:
    kind: str                 # "basic" | "bottleneck"
    stage: int
    index: int
    in_c: int
    out_c: int
    in_hw: int
    out_hw: int
    stride: int
    bn1: BN
    proj: Optional[Conv]
    convs: List[Conv]         # basic: [conv3x3(stride), conv3x3]; bottleneck: [1x1, 3x3(stride), 1x1]
    bns: List[BN]             # BNs preceding convs[1:], i.e. bn2 (and bn3)
    se: Optional[SE] = None   # gate on the residual branch (se_ratio > 0)
    avg_down: bool = False    # ResNet-D shortcut: proj is 1x1 stride 1 on the 2x2 / 2 average-pooled input
    drop_rate: float = 0.0    # stochastic depth: probability that a training step drops the residual branch


@dataclass
class NetSpec:
    name: str
    dataset: str
    num_classes: int
    image_size: int
    in_channels: int          # 3 (stored as 8)
    stem: Conv
    stem_hw: int              # spatial size after the stem conv
    maxpool: bool             # ImageNet 3x3/2 SAME max-pool after the stem
    pool_hw: int              # spatial size entering stage 1
    blocks: List[Block] = field(default_factory=list)
    final_bn: Optional[BN] = None
    final_hw: int = 0
    final_c: int = 0
    dense_name: str = "dense"
    # ResNet-C deep stem (extension): the convs in front of `stem` (3x3 / 2 3 -> 32, 3x3 / 1 32 -> 32) and the
    # BatchNorm + ReLU behind each of them; `stem` is then the last conv (3x3 / 1 32 -> 64). Empty: one stem conv
    stem_pre: List[Conv] = field(default_factory=list)
    stem_bns: List[BN] = field(default_factory=list)

    # -- TF variable inventory, creation order ---------------------------------------------------
    def trainable_variables(self):
        """[(tf_name, tf_shape, kind, owner)] in tf.trainable_variables() order."""
        out = []

        def conv(c: Conv):
            out.append((f"{c.name}/kernel", (c.k, c.k, c.cin // c.groups, c.cout), "conv", c))

        def bn(b: BN):
            out.append((f"{b.name}/gamma", (b.c,), "gamma", b))
            out.append((f"{b.name}/beta", (b.c,), "beta", b))

        for c, b in zip(self.stem_pre, self.stem_bns):
            conv(c)
            bn(b)
        conv(self.stem)
        for blk in self.blocks:
            bn(blk.bn1)
            if blk.proj is not None:
                conv(blk.proj)
            conv(blk.convs[0])
            for b, c in zip(blk.bns, blk.convs[1:]):
                bn(b)
                conv(c)
            if blk.se is not None:
                e = blk.se
                out.append((f"{e.name}/reduce/kernel", (e.c, e.hidden), "se_w", e))
                out.append((f"{e.name}/reduce/bias", (e.hidden,), "se_b", e))
                out.append((f"{e.name}/expand/kernel", (e.hidden, e.c), "se_w", e))
                out.append((f"{e.name}/expand/bias", (e.c,), "se_b", e))
        bn(self.final_bn)
        out.append((f"{self.dense_name}/kernel", (self.final_c, self.num_classes), "dense_w", None))
        out.append((f"{self.dense_name}/bias", (self.num_classes,), "dense_b", None))
        return out

    def batch_norms(self) -> List[BN]:
        bns = list(self.stem_bns)
        for blk in self.blocks:
            bns.append(blk.bn1)
            bns.extend(blk.bns)
        bns.append(self.final_bn)
        return bns

    def convs(self) -> List[Conv]:
        cs = self.stem_pre + [self.stem]
        for blk in self.blocks:
            if blk.proj is not None:
                cs.append(blk.proj)
            cs.extend(blk.convs)
        return cs

    def num_params(self) -> int:
        n = 0
        for _, shape, _, _ in self.trainable_variables():
            p = 1
            for d in shape:
                p *= d
            n += p
        return n

    def forward_flops(self) -> int:
        """Multiply-add FLOPs (x2) of one image's forward pass: convs + dense."""
        fl = 0
        hw = self.image_size
        fl += 2 * sum(c.params for c in self.convs()[:len(self.stem_pre) + 1]) * self.stem_hw * self.stem_hw
        for blk in self.blocks:
            if blk.proj is not None:
                fl += 2 * blk.proj.params * blk.out_hw * blk.out_hw
            h = blk.in_hw
            for c in blk.convs:
                h = c.out_hw(h)
                fl += 2 * c.params * h * h
            if blk.se is not None:   # the two gate layers (the squeeze and the excite are not multiply-adds)
                fl += 2 * 2 * blk.se.c * blk.se.hidden
        fl += 2 * self.final_c * self.num_classes
        del hw
        return fl


class _Namer:
    def __init__(self):
        self.conv = 0
        self.bn = 0
        self.se = 0

    def next_conv(self) -> str:
        n = "conv2d" if self.conv == 0 else f"conv2d_{self.conv}"
        self.conv += 1
        return n

    def next_bn(self) -> str:
        n = "batch_normalization" if self.bn == 0 else f"batch_normalization_{self.bn}"
        self.bn += 1
        return n


    def next_se(self) -> str:
        n = "squeeze_excite" if self.se == 0 else f"squeeze_excite_{self.se}"
        self.se += 1
        return n


SE_RATIOS = (0, 4, 8, 16)


def _check_se_ratio(se_ratio: int):
    if se_ratio not in SE_RATIOS:
        raise ValueError(f"se_ratio must be one of {SE_RATIOS}, got {se_ratio!r}")


def drop_rates(rate: float, blocks: int) -> List[float]:
    """Stochastic depth's linear rule (Huang et al. 2016): block b of B, in network order, drops its residual
    branch with probability rate * b / (B - 1): 0 for the first block, `rate` for the last."""
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop_path_rate must be in [0, 1), got {rate!r}")
    return [rate * b / (blocks - 1) if blocks > 1 else 0.0 for b in range(blocks)]


def _set_drop_rates(spec: NetSpec, rate: float) -> NetSpec:
    for blk, p in zip(spec.blocks, drop_rates(float(rate), len(spec.blocks))):
        blk.drop_rate = p
    return spec


def _stage(spec: NetSpec, nm: _Namer, kind: str, stage: int, filters: int, blocks: int, stride: int,
           in_c: int, hw: int, width: int = 1, groups: int = 1, width_per_group: int = 64,
           se_ratio: int = 0, avg_down: bool = False) -> tuple[int, int]:
    out_c = filters * 4 if kind == "bottleneck" else filters
    for i in range(blocks):
        s = stride if i == 0 else 1
        bn1 = BN(nm.next_bn(), in_c)
        # ResNet-D: a stride-2 projection pools 2x2 / 2 first and convolves at stride 1 (same variable)
        pooled = avg_down and i == 0 and s == 2
        if pooled and hw % 2:
            raise ValueError(f"avg_down: stage {stage} downsamples an odd {hw} x {hw} input")
        proj = Conv(nm.next_conv(), in_c, out_c, 1, 1 if pooled else s) if i == 0 else None
        convs, bns = [], []
        if kind == "basic":
            c1 = Conv(nm.next_conv(), in_c, filters, 3, s)
            b2 = BN(nm.next_bn(), filters)
            c2 = Conv(nm.next_conv(), filters, filters, 3, 1)
            convs, bns = [c1, c2], [b2]
        else:
            # ResNeXt: `groups` paths of width_per_group * 2^(stage-1) channels through the 3x3 conv
            mid = filters * width if groups == 1 else groups * width_per_group * 2 ** (stage - 1)
            c1 = Conv(nm.next_conv(), in_c, mid, 1, 1)
            b2 = BN(nm.next_bn(), mid)
            c2 = Conv(nm.next_conv(), mid, mid, 3, s, groups=groups)
            b3 = BN(nm.next_bn(), mid)
            c3 = Conv(nm.next_conv(), mid, out_c, 1, 1)
            convs, bns = [c1, c2, c3], [b2, b3]
        out_hw = convs[0].out_hw(hw) if kind == "basic" else convs[1].out_hw(hw)
        se = SE(nm.next_se(), out_c, max(out_c // se_ratio, 8)) if se_ratio else None
        spec.blocks.append(Block(kind, stage, i, in_c, out_c, hw, out_hw, s, bn1, proj, convs, bns, se, pooled))
        in_c, hw = out_c, out_hw
    return in_c, hw


def cifar_resnet_v2(resnet_size: int = 50, num_classes: int = 10, se_ratio: int = 0,
                    avg_down: bool = False, drop_path_rate: float = 0.0) -> NetSpec:
    """cifar10_resnet_v2_generator (reference resnet_model_official.py:217-278); se_ratio > 0 ->
    every block gated by Squeeze-and-Excitation (extension); avg_down -> ResNet-D shortcuts (extension);
    drop_path_rate > 0 -> stochastic depth, Block.drop_rate by the linear rule (extension)."""
    if resnet_size % 6 != 2:
        raise ValueError(f"resnet_size must be 6n + 2: {resnet_size}")
    _check_se_ratio(se_ratio)
    n = (resnet_size - 2) // 6
    nm = _Namer()
    stem = Conv(nm.next_conv(), 3, 16, 3, 1, cin_store=8)
    spec = NetSpec(("se_" if se_ratio else "") + f"cifar_resnet{resnet_size}_v2" + ("_avgdown" if avg_down else ""),
                   "cifar", num_classes, 32, 3, stem, 32, False, 32)
    c, hw = 16, 32
    for stage, (f, s) in enumerate(((16, 1), (32, 2), (64, 2)), start=1):
        c, hw = _stage(spec, nm, "basic", stage, f, n, s, c, hw, se_ratio=se_ratio, avg_down=avg_down)
    spec.final_bn = BN(nm.next_bn(), c)
    spec.final_hw, spec.final_c = hw, c
    return _set_drop_rates(spec, drop_path_rate)


IMAGENET_SIZES = {
    18: ("basic", [2, 2, 2, 2]),
    34: ("basic", [3, 4, 6, 3]),
    50: ("bottleneck", [3, 4, 6, 3]),
    101: ("bottleneck", [3, 4, 23, 3]),
    152: ("bottleneck", [3, 8, 36, 3]),
    200: ("bottleneck", [3, 24, 36, 3]),
}


def imagenet_resnet_v2(resnet_size: int = 50, num_classes: int = 1001, width: int = 1,
                       image_size: int = 224, groups: int = 1, width_per_group: int = 64,
                       se_ratio: int = 0, avg_down: bool = False, drop_path_rate: float = 0.0,
                       deep_stem: bool = False) -> NetSpec:
    """imagenet_resnet_v2 (reference resnet_model_official.py:281-366); width=2 -> WRN-50-2 (extension);
    groups > 1 -> ResNeXt (extension): the bottleneck's 3x3 conv is grouped, its width in stage s is
    groups * width_per_group * 2^(s-1) (32x4d: 128 / 256 / 512 / 1024), the block output stays filters * 4.
    se_ratio > 0 -> every block gated by Squeeze-and-Excitation, hidden width max(C / se_ratio, 8) (extension).
    avg_down -> ResNet-D shortcuts (extension): every stride-2 projection becomes a 2x2 / 2 average pool + a 1x1
    stride-1 conv (Block.avg_down); variable names and shapes are unchanged.
    drop_path_rate > 0 -> stochastic depth (extension): Block.drop_rate by the linear rule; variables unchanged.
    deep_stem -> the ResNet-C stem (extension; He et al. 2019, section 4.2): the 7x7 / 2 conv becomes conv3x3 / 2
    3 -> 32, BN, ReLU, conv3x3 / 1 32 -> 32, BN, ReLU, conv3x3 / 1 32 -> 64 (NetSpec.stem_pre / stem_bns / stem);
    variables conv2d, batch_normalization, conv2d_1, batch_normalization_1, conv2d_2, then the blocks."""
    if resnet_size not in IMAGENET_SIZES:
        raise ValueError(f"Not a valid resnet_size: {resnet_size}")
    kind, layers = IMAGENET_SIZES[resnet_size]
    if groups < 1 or width_per_group < 1:
        raise ValueError(f"groups and width_per_group must be >= 1, got {groups}, {width_per_group}")
    if groups > 1 and (kind != "bottleneck" or width != 1):
        raise ValueError("ResNeXt (groups > 1) needs a bottleneck resnet_size (50, 101, 152, 200) and width 1")
    _check_se_ratio(se_ratio)
    nm = _Namer()
    stem_pre, stem_bns = [], []
    if deep_stem:
        if image_size % 2:
            raise ValueError(f"deep_stem: an odd image size ({image_size}) is not supported")
        for cin, store, stride in ((3, 8, 2), (32, 32, 1)):
            stem_pre.append(Conv(nm.next_conv(), cin, 32, 3, stride, cin_store=store))
            stem_bns.append(BN(nm.next_bn(), 32))
        stem = Conv(nm.next_conv(), 32, 64, 3, 1)
        stem_hw = stem_pre[0].out_hw(image_size)
    else:
        stem = Conv(nm.next_conv(), 3, 64, 7, 2, cin_store=8)
        stem_hw = stem.out_hw(image_size)
    pool_hw = (stem_hw + 1) // 2  # max_pooling2d(3, 2, 'SAME')
    tag = f"wide_resnet{resnet_size}_{width}" if width != 1 else f"imagenet_resnet{resnet_size}_v2"
    if groups > 1:
        tag = f"resnext{resnet_size}_{groups}x{width_per_group}d"
    if se_ratio:
        tag = "se_" + tag
    if avg_down:
        tag += "_avgdown"
    if deep_stem:
        tag += "_deepstem"
    spec = NetSpec(tag, "imagenet", num_classes, image_size, 3, stem, stem_hw, True, pool_hw,
                   stem_pre=stem_pre, stem_bns=stem_bns)
    c, hw = 64, pool_hw
    for stage, (f, s) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), start=1):
        c, hw = _stage(spec, nm, kind, stage, f, layers[stage - 1], s, c, hw, width=width, groups=groups,
                       width_per_group=width_per_group, se_ratio=se_ratio, avg_down=avg_down)
    spec.final_bn = BN(nm.next_bn(), c)
    spec.final_hw, spec.final_c = hw, c
    return _set_drop_rates(spec, drop_path_rate)


def build_spec(dataset: str, resnet_size: int | None = None, model: str = "resnet", width: int = 1,
               num_classes: int | None = None, cardinality: int = 32, width_per_group: int = 4,
               se_ratio: int = 0, avg_down: bool = False, drop_path_rate: float = 0.0,
               deep_stem: bool = False) -> NetSpec:
    """Network selection of the reference ResNet wrapper (resnet_model.py:71-74, size fixed to 50
    there; `--resnet_size` makes it selectable here). cifar100 is supported."""
    if model == "wide_resnet":
        width = max(width, 2)
    if deep_stem and dataset != "imagenet":
        raise ValueError("deep_stem is an ImageNet stem (the CIFAR nets have a single 3x3 stem conv)")
    if model == "resnext":
        if dataset != "imagenet":
            raise ValueError("model=resnext is an ImageNet network (bottleneck blocks)")
        return imagenet_resnet_v2(resnet_size or 50, num_classes or 1001, groups=cardinality,
                                  width_per_group=width_per_group, se_ratio=se_ratio, avg_down=avg_down,
                                  drop_path_rate=drop_path_rate, deep_stem=deep_stem)
    if dataset in ("cifar10", "cifar100", "cifar"):
        nc = num_classes or (100 if dataset == "cifar100" else 10)
        return cifar_resnet_v2(resnet_size or 50, nc, se_ratio=se_ratio, avg_down=avg_down,
                               drop_path_rate=drop_path_rate)
    if dataset == "imagenet":
        return imagenet_resnet_v2(resnet_size or 50, num_classes or 1001, width=width, se_ratio=se_ratio,
                                  avg_down=avg_down, drop_path_rate=drop_path_rate, deep_stem=deep_stem)
    raise ValueError(f"unknown dataset {dataset}")
