"""The CASAPose graph, described once: ResNet-18 at output stride 8 (resnet.py:183-328), decoder 1 and the class-adaptive decoder 2
(pose_models.py:513-635) with the switches that tell the registry's variants apart.  `initial_parameters`, the inference plan
(engine.ForwardPlan / CasaposeNet) and the training plan (train_engine.TrainPlan) all walk these records; what each of them does with a
record stays in that plan."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

from . import _lib

STAGE_FILTERS = (64, 128, 256, 512)
STAGE_STRIDE = (1, 2, 1, 1)  # resnet.py:262-290 (output_stride 8)
STAGE_DILATION = (1, 1, 2, 4)
DECODER_DIMS_DEFAULT = (256, 128, 64, 32, 32)
# decoder-2 configuration of blocks 6..10: which use a partial convolution, which upsample their output with the
# label-guided gather (else plain nearest x2).  CASAPoseConditional1-5 (pose_models.py:14-635) differ only in these.
PARTIAL_DEFAULT = (True, True, True, True, True)
GUIDED_DEFAULT = (False, True, True, True, False)
BILINEAR_DEFAULT = (False, False, False, False, False)  # with guided: GuidedBilinearUpsampling (casapose_c_gcu4_bilat)
SHARED_DEFAULT = (False, False, False, False, False)

LEVEL = (3, 3, 2, 1, 0)   # pyramid level each decoder block runs at (resolution / 2^level)
TAPS = ("x4s", "x8s", "x16s", "x32s")   # the activated output of each stage (resnet.py:291,303-305,319)
SKIP = (None, ("x8s", 128, 128), ("x4s", 64, 64), ("x2s", 64, 64), ("img4", 4, 3))   # skip tap of decoder block i: (name, ld, real channels)


@dataclass(frozen=True)
class Arch:
    """One network of the registry.  shared[i]: blocks i+1 and i+6 use the one PartialConvolution weight set pv_block_{i+1}_{i+6}_conv2d;
    reuse_first: block 6 normalises the raw output of block 1's convolution instead of convolving; skips2 False: decoder 2 has no skip
    connections (pose_models.py:699-1362, the `_sw*` entries); pvnet: decoder 1 only and ONE 1x1 head for seg + vertex (pose_models.py:645-696)."""
    seg_dim: int
    ver_dim: int
    decoder_dims: Tuple[int, ...] = DECODER_DIMS_DEFAULT
    partial: Tuple[bool, ...] = PARTIAL_DEFAULT
    guided: Tuple[bool, ...] = GUIDED_DEFAULT
    bilinear: Tuple[bool, ...] = BILINEAR_DEFAULT
    pvnet: bool = False
    shared: Tuple[bool, ...] = SHARED_DEFAULT
    reuse_first: bool = False
    skips2: bool = True

    def __post_init__(self):
        for f in ("partial", "guided", "bilinear", "shared"):
            object.__setattr__(self, f, tuple(bool(v) for v in getattr(self, f)))
        for f, t in (("seg_dim", int), ("ver_dim", int), ("pvnet", bool), ("reuse_first", bool), ("skips2", bool)):
            object.__setattr__(self, f, t(getattr(self, f)))
        object.__setattr__(self, "decoder_dims", tuple(int(d) for d in self.decoder_dims))
        if any(len(getattr(self, f)) != 5 for f in ("decoder_dims", "partial", "guided", "bilinear", "shared")):
            raise ValueError("decoder_dims and the variant switches describe the five decoder blocks")
        if any(b and not g for b, g in zip(self.bilinear, self.guided)):
            raise NotImplementedError("bilinear_upsampling without guided_upsampling in decoder 2 is not built")


@dataclass(frozen=True)
class Conv:
    name: str                            # layer name of the descriptor
    key: str                             # weight key in the parameter set
    layout: int                          # 0: HWIO, 1: [Cin,3,3,Cout] (PartialConvolution weights)
    k: int
    cout: int
    sources: Tuple[Tuple[int, int], ...]  # (ld, real channels) per input tensor
    stride: int = 1
    dilation: int = 1
    pad: int = 0
    partial: bool = False                # mask-aware: tap mask + row scale from the label pyramid

    @property
    def cin(self) -> int:
        return sum(c for _, c in self.sources)

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return (self.k, self.k, self.cin, self.cout) if self.layout == 0 else (self.cin, self.k, self.k, self.cout)


@dataclass(frozen=True)
class Norm:
    name: str
    channels: int
    clade: bool = False                  # ClassAdaptiveWeightedNormalization: [seg_dim, C] gamma / beta tables behind the moving statistics
    gamma: bool = True
    beta: bool = True


@dataclass(frozen=True)
class Unit:
    """ResNet basic block (resnet.py:199-243): bn1 + ReLU, conv1, bn2 + ReLU, conv2 + the shortcut (a strided 1x1 conv in a stage's first unit)."""
    base: str
    cin: int
    cout: int
    tap: Optional[str]                   # the backbone output that is this unit's activated output (last unit of a stage)
    sc: Optional[Conv]
    conv1: Conv
    conv2: Conv
    bn1: Norm
    bn2: Norm


@dataclass(frozen=True)
class Block:
    number: int                          # 1..10 (pv_block_<number>_*)
    decoder: int                         # 1 or 2
    level: int
    conv: Optional[Conv]                 # None: reuse_first block 6 normalises block 1's raw convolution output
    norm: Norm
    act: int                             # _lib.ACT_RELU / ACT_LEAKY01
    upsample: str                        # how the previous block's output reaches this block: none, bilinear, guided, nearest, guided_bilinear
    skip: Optional[str]                  # skip tap read as the second source


@dataclass(frozen=True)
class Graph:
    """The walk in forward order (the ResNet stem's input normalisation bn_data is folded into conv0 / its padding channel)."""
    bn_data: Norm
    conv0: Conv
    bn0: Norm
    units: Tuple[Unit, ...]
    bn1: Norm
    decoder1: Tuple[Block, ...]
    seg_head: Conv                       # pvnet: the one head pv_final_conv
    decoder2: Tuple[Block, ...]          # empty for pvnet
    ver_head: Optional[Conv]


def _block(a: Arch, i: int, second: bool) -> Block:
    dims = a.decoder_dims
    n = i + 6 if second else i + 1
    skip = SKIP[i] if (i > 0 and (a.skips2 or not second)) else None
    srcs = ((512, 512),) if i == 0 else ((dims[i - 1], dims[i - 1]),) + ((skip[1:],) if skip else ())
    partial = second and a.partial[i]
    if a.shared[i]:
        key, layout = "pv_block_%d_%d_conv2d.weights" % (i + 1, i + 6), 1
    elif partial:
        key, layout = "pv_block_%d_prepare_conv2d.weights" % n, 1
    else:
        key, layout = "pv_block_%d_conv2d.kernel" % n, 0
    name = ("pv_block_%d_prepare_conv2d" if partial else "pv_block_%d_conv2d") % n
    conv = None if (second and i == 0 and a.reuse_first) else Conv(name, key, layout, 3, dims[i], srcs, pad=1, partial=partial)
    up = "none" if i < 2 else "bilinear" if not second else "guided_bilinear" if a.bilinear[i - 1] else "guided" if a.guided[i - 1] else "nearest"
    norm = Norm("pv_block_%d_clade" % n, dims[i], clade=True) if second else Norm("pv_block_%d_bn" % n, dims[i])
    return Block(n, 2 if second else 1, LEVEL[i], conv, norm, _lib.ACT_RELU if i == 0 else _lib.ACT_LEAKY01, up, skip and skip[0])


def _plain(name: str, k: int, cin: int, cout: int, stride: int = 1, dilation: int = 1) -> Conv:
    return Conv(name, name + ".kernel", 0, k, cout, ((cin, cin),), stride, dilation, dilation * (k // 2))


def graph(a: Arch) -> Graph:
    units: List[Unit] = []
    cin = 64
    for s, f in enumerate(STAGE_FILTERS):
        for u in range(2):
            b, st, d = "stage%d_unit%d_" % (s + 1, u + 1), STAGE_STRIDE[s] if u == 0 else 1, STAGE_DILATION[s]
            units.append(Unit(b, cin, f, TAPS[s] if u == 1 else None, _plain(b + "sc", 1, cin, f, st) if u == 0 else None,
                              _plain(b + "conv1", 3, cin, f, st, d), _plain(b + "conv2", 3, f, f, 1, d), Norm(b + "bn1", cin), Norm(b + "bn2", f)))
            cin = f
    d4 = a.decoder_dims[4]
    stem = (Norm("bn_data", 3, gamma=False), Conv("conv0", "conv0.kernel", 0, 7, 64, ((4, 3),), stride=2, pad=3), Norm("bn0", 64), tuple(units),
            Norm("bn1", 512), tuple(_block(a, i, False) for i in range(5)))
    if a.pvnet:
        return Graph(*stem, _plain("pv_final_conv", 1, d4, a.seg_dim + a.ver_dim), (), None)
    return Graph(*stem, _plain("pv_final_conv_segmentation", 1, d4, a.seg_dim), tuple(_block(a, i, True) for i in range(5)),
                 _plain("pv_final_conv_vertex", 1, d4, a.ver_dim))

def forward_order() -> List[str]:
    """Layer names of every variant in the order the forward uses them (resnet.py:246-305; pose_models.py:541-616).  The flat parameter buffer
    follows this order, so the backward completes it from the END towards the start and gradient buckets are contiguous tail slices."""
    order = ["bn_data", "conv0", "bn0"]
    for s in range(1, 5):
        for u in range(1, 3):
            base = "stage%d_unit%d_" % (s, u)
            order += [base + "bn1", base + "sc", base + "conv1", base + "bn2", base + "conv2"]
    order.append("bn1")
    for i in range(1, 6):
        order += ["pv_block_%d_conv2d" % i, "pv_block_%d_%d_conv2d" % (i, i + 5), "pv_block_%d_bn" % i]
    order += ["pv_final_conv_segmentation", "pv_final_conv"]
    for i in range(6, 11):
        order += ["pv_block_%d_prepare_conv2d" % i, "pv_block_%d_conv2d" % i, "pv_block_%d_clade" % i]
    order.append("pv_final_conv_vertex")
    return order
