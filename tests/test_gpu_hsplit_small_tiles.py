"""The four 32-channel direct 3x3 layers of the decoders (blocks 4, 9, 5, 10) on the fp16-pair pipe of csrc/conv_hsplit.hip against the SAME descriptor
on the fp32-MFMA kernel, at the bound tests/test_gpu_hsplit.py uses for that comparison (2e-5 of the tensor's range).

Their loader waves read the kernel arguments where they use them (once per tile or phase) and each role builds the epilogue's operands for itself;
what that can break are the tile walk and the per-tile offsets, so the shapes are the smallest that exercise them:
  (a) 2 x 20 x 40: the last tile row (20 = 2.5 x 8) and the last tile column (40 = 32 + 8) are partial -- the range tests of border tiles decide;
  (b) 4 x 64 x 800: 800 tiles, at least three times the blocks of a persistent launch (asserted) -- every block walks three tiles or more, its
      increments carry across the row and the image, and the loader twin's deferred epilogue row sees both tile parities."""
import numpy as np
import pytest
import torch

from test_gpu_conv import _labels

pytestmark = pytest.mark.gpu
F16X2 = 102
TOL = 2e-5
SHAPES = [(2, 20, 40), (4, 64, 800)]
K = 5   # classes of the label map


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).numpy()


def _both_pipes(layer, outs, stream):
    """run the bound layer on the fp16-pair pipe and again on the fp32-MFMA kernel; returns [(f16x2, fp32)] per output tensor"""
    from casapose_amd import _lib

    assert layer.split_mode == _lib.PLANES_F16X2
    layer.run(stream)
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    for o in outs:
        o.zero_()
    layer.split_mode = 0
    layer.run(stream)
    torch.cuda.synchronize()
    return list(zip(got, [o.clone() for o in outs]))


def _near(a, b):
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert scale > 0 and err <= TOL * scale, "max|diff| %.3e vs range %.3e" % (err, scale)


def _label_maps(device, gen, b, h, w):
    from casapose_amd import ops

    lab = _labels(np.random.default_rng(int(torch.randint(1 << 30, (1,), generator=gen))), b, h, w, K)
    return ops.label_pyramid(torch.from_numpy(lab).to(device=device, dtype=torch.uint8))


def _clade_tables(device, gen, cout):
    from casapose_amd.engine import fold_clade

    p = {"c.gamma": 1.0 + 0.25 * _rand(gen, K, cout).clip(-2, 2), "c.beta": _rand(gen, K, cout, scale=0.2),
         "c.moving_mean": _rand(gen, cout, scale=0.1), "c.moving_variance": 1.0 + 0.25 * _rand(gen, cout).clip(-2, 2)}
    ts, tb = fold_clade(p, "c")
    return [torch.from_numpy(np.ascontiguousarray(t)).to(device=device, dtype=torch.float32) for t in (ts, tb)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("block", [4, 9, 5, 10])
def test_32_channel_blocks_match_the_fp32_kernel(device, block, shape):
    from casapose_amd import _lib, ops
    from casapose_amd.engine import FusedConv

    b, h, w = shape
    if b == 4:   # 8-row x 32-column tiles
        assert b * ((h + 7) // 8) * ((w + 31) // 32) >= 3 * _lib.load().cp_get_persistent_blocks()
    gen = torch.Generator().manual_seed(100 * block + h)
    stream = torch.cuda.current_stream(device).cuda_stream
    head = block in (5, 10)
    c0 = 32 if head else 64                # channels of the half-resolution source
    c1 = (4, 3) if head else (32, 32)      # the image (padded to four channels) or a full-resolution skip tensor
    low = torch.randn(b, h // 2, w // 2, c0, generator=gen).to(device)
    if head:
        second = ops.pad_channels_3to4((2 * torch.rand(b, h, w, 3, generator=gen) - 1).to(device))
    else:
        second = torch.randn(b, h, w, c1[0], generator=gen).to(device)
    cin = c0 + c1[1]
    wk = _rand(gen, 3, 3, cin, 32, scale=1.0 / np.sqrt(9 * cin)).astype(np.float32)
    layer = FusedConv("block%d" % block, wk, 0, 3, 3, 32, [(c0, c0), c1], device)
    kw = dict(batch=b, in_h=h, in_w=w, pad=1, act=2, tile_hint=F16X2)
    if block in (4, 5):    # decoder 1: x2 bilinear source, batch-norm table
        srcs = [dict(data=low, ld=c0, mode=_lib.SRC_BILINEAR_X2), dict(data=second, ld=c1[0])]
        kw.update(scale=(1.0 + 0.25 * torch.randn(32, generator=gen).clamp(-2, 2)).to(device), shift=(0.2 * torch.randn(32, generator=gen)).to(device))
    else:                  # decoder 2: guided x2 source, partial convolution, class-adaptive table
        labels, pnorm, sel = _label_maps(device, gen, b, h, w)
        srcs = [dict(data=low, ld=c0, mode=_lib.SRC_NEAREST_SEL, sel=sel[0]), dict(data=second, ld=c1[0])]
        ts, tb = _clade_tables(device, gen, 32)
        kw.update(scale=ts, shift=tb, epi_label=labels[0], tap_label=labels[0], row_scale=pnorm[0])
    if not head:
        act = torch.zeros(b, h, w, 32, device=device)
        layer.bind(srcs=srcs, out_act=act, **kw)
        (got, ref), = _both_pipes(layer, [act], stream)
        _near(got, ref)
        return
    q, off = (9, 0) if block == 5 else (27, 9)   # the heads' columns of the 36-float output records
    layer.attach_head(_rand(gen, 1, 1, 32, q, scale=1.0 / 6.0).astype(np.float32))
    out = torch.zeros(b, h, w, 36, device=device)
    hlab = torch.full((b, h, w), 255, dtype=torch.uint8, device=device)
    extra = dict(head_label_out=hlab, head_label_classes=q) if block == 5 else {}
    layer.bind(srcs=srcs, head_out=out[..., off:], head_out_ld=36, **extra, **kw)
    outs = [out, hlab] if block == 5 else [out]
    pairs = _both_pipes(layer, outs, stream)
    got, ref = pairs[0]
    _near(got[..., off:off + q], ref[..., off:off + q])
    rest = [c for c in range(36) if not off <= c < off + q]
    assert (got[..., rest] == 0).all()            # the other columns of the records stay untouched
    if block == 5:   # the label map is the arg-max (first maximum) of the logits this very launch stored
        assert (pairs[1][0].cpu().numpy() == got[..., :q].cpu().numpy().argmax(-1)).all()
