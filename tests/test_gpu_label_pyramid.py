"""cp_label_pyramid computes every level's maps from the level-0 label map in one launch.  Every output byte for byte against the oracle's
HalfSize, PartialConvolution norm and GuidedUpsampling selection, at the two production sizes, on noisy and blob label maps, and with the
optional outputs left out."""
import ctypes as C

import numpy as np
import pytest
import torch

import casapose_oracle as O

pytestmark = pytest.mark.gpu

K = 9


def _label_maps(b, h, w, seed):
    """Image 0: salt-and-pepper labels (every neighbourhood mixed); the others: blobs and bands on a background, with labels on the borders."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((b, h, w), np.uint8)
    lab[0] = rng.integers(0, K, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    for bi in range(1, b):
        for o in range(1, K):
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
            ry, rx = rng.uniform(0.05, 0.25) * h, rng.uniform(0.05, 0.25) * w
            lab[bi][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = o
        lab[bi, h - 3:, : w // 2] = 3      # a band on the last rows
        lab[bi, : h // 2, w - 5:] = 5      # and one on the last columns
        lab[bi, ::7, ::5] = 7              # isolated pixels
    return lab


def _oracle(lab0, levels=4):
    """labels[l], pnorm[l] (float32 [b,h,w]) and sel[l] (uint8, None where level l is not exactly twice level l + 1) from the oracle."""
    labs = [lab0]
    for _ in range(1, levels):
        labs.append(np.ascontiguousarray(O.half_size(labs[-1][..., None])[..., 0]))
    hot = [O.onehot_from_labels(l.astype(np.int64), K, np.float32) for l in labs]
    pnorm = [O.partial_conv_mask(m)[1][..., 0].astype(np.float32) for m in hot]
    sel = []
    for l in range(levels - 1):
        even = labs[l].shape[1] == 2 * labs[l + 1].shape[1] and labs[l].shape[2] == 2 * labs[l + 1].shape[2]
        sel.append(O.guided_upsampling_select(hot[l + 1], hot[l]).astype(np.uint8) if even else None)
    return labs, pnorm, sel


def _same(got, want, what):
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, what
    assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), "%s: %d elements differ" % (what, int((g != want).sum()))


@pytest.mark.parametrize("h,w", [(480, 640), (448, 448)])
def test_all_maps_at_production_sizes(device, h, w):
    from casapose_amd import ops

    lab0 = _label_maps(2, h, w, seed=h)
    labs, pnorm, sel = _oracle(lab0)
    g_lab, g_pn, g_sel = ops.label_pyramid(torch.from_numpy(lab0).to(device))
    for l in range(4):
        _same(g_lab[l], labs[l], "labels[%d]" % l)
        _same(g_pn[l], pnorm[l], "pnorm[%d]" % l)
    for l in range(3):
        assert sel[l] is not None and g_sel[l] is not None
        _same(g_sel[l], sel[l], "sel[%d]" % l)


def _call(lab0, want_labels, want_pnorm, want_sel, device):
    """cp_label_pyramid with chosen outputs: want_* are per-level booleans, or None for a null array.  Returns the tensors (None where not asked)
    pre-filled with a pattern, so that an output the call should not write is seen to be untouched."""
    from casapose_amd import _lib

    b, h, w = lab0.shape
    t0 = torch.from_numpy(lab0).to(device)
    labels = [t0] + [torch.full((b, h >> l, w >> l), 0xAB, dtype=torch.uint8, device=device) if want_labels[l] else None for l in range(1, 4)]
    pnorm = [torch.full((b, h >> l, w >> l), -1.0, device=device) if want_pnorm and want_pnorm[l] else None for l in range(4)]
    sel = [torch.full((b, h >> l, w >> l), 0xCD, dtype=torch.uint8, device=device) if want_sel and want_sel[l] else None for l in range(3)]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    rc = _lib.load().cp_label_pyramid(t0.data_ptr(), b, h, w, arr(labels), arr(pnorm) if want_pnorm else None, arr(sel) if want_sel else None,
                                      torch.cuda.current_stream(device).cuda_stream)
    _lib.check(rc, "cp_label_pyramid")
    torch.cuda.synchronize()
    return labels, pnorm, sel


@pytest.mark.parametrize("h,w", [(480, 640), (448, 448)])
def test_optional_outputs(device, h, w):
    lab0 = _label_maps(2, h, w, seed=w + 1)
    labs, pnorm, sel = _oracle(lab0)
    # labels only: pnorm and sel arrays null
    g_lab, _, _ = _call(lab0, [1, 1, 1, 1], None, None, device)
    for l in range(1, 4):
        _same(g_lab[l], labs[l], "labels[%d] alone" % l)
    # pnorm without sel, with a null entry in the middle
    g_lab, g_pn, _ = _call(lab0, [1, 1, 1, 1], [1, 0, 1, 1], None, device)
    for l in (0, 2, 3):
        _same(g_pn[l], pnorm[l], "pnorm[%d] without sel" % l)
    for l in range(1, 4):
        _same(g_lab[l], labs[l], "labels[%d] without sel" % l)
    # sel without pnorm, with a null entry
    g_lab, _, g_sel = _call(lab0, [1, 1, 1, 1], None, [1, 0, 1], device)
    for l in (0, 2):
        _same(g_sel[l], sel[l], "sel[%d] without pnorm" % l)
    # the pyramid stops at the first null labels entry: levels 0..1 only, level 0 without a pnorm
    g_lab, g_pn, g_sel = _call(lab0, [1, 1, 0, 0], [0, 1, 0, 0], [1, 0, 0], device)
    _same(g_lab[1], labs[1], "labels[1] of a two-level pyramid")
    _same(g_pn[1], pnorm[1], "pnorm[1] of a two-level pyramid")
    _same(g_sel[0], sel[0], "sel[0] of a two-level pyramid")


def test_odd_sizes_and_small_maps(device):
    """Sizes that do not halve exactly (HalfSize drops the last row / column, no selection map there) and widths that are no multiple of 4."""
    from casapose_amd import ops

    for (b, h, w) in [(3, 37, 50), (1, 30, 44), (2, 9, 11), (1, 64, 96)]:
        lab0 = _label_maps(b, h, w, seed=h * w)
        labs, pnorm, sel = _oracle(lab0)
        g_lab, g_pn, g_sel = ops.label_pyramid(torch.from_numpy(lab0).to(device))
        for l in range(4):
            _same(g_lab[l], labs[l], "%dx%d labels[%d]" % (h, w, l))
            _same(g_pn[l], pnorm[l], "%dx%d pnorm[%d]" % (h, w, l))
        for l in range(3):
            assert (sel[l] is None) == (g_sel[l] is None), (h, w, l)
            if sel[l] is not None:
                _same(g_sel[l], sel[l], "%dx%d sel[%d]" % (h, w, l))
