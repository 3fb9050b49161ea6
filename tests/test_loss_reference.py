"""tests/loss_reference.py (the staged fp64 restatement the GPU stage tests of the pose losses compare with) pinned on the CPU against the two
oracles, on every small case of tests/loss_cases.py -- whose property assertions run here as well, on the reference:
  merged    : torch_train_ref.losses, values and autograd gradient, all four filter combinations;
  separated : loss_functions_ref.compute_loss_separated, both settings of the segmentation filter.
The oracles take ONE label map.  With labels_ce == labels_fg they are called once, as they stand.  Where the two maps differ the oracle is called
twice: the mask term does not read labels_fg and the vertex / proxy terms (and both filters) do not read labels_ce, so mask(labels_ce) and
vertex, proxy(labels_fg) are the three terms of the two-map loss.
The oracles take sqrt(vy^2 + vx^2) before they mask the zero directions out, so their autograd gradient is NaN (0 * inf in sqrt's backward)
exactly at the direction pairs that are (0, 0); the `degenerate` case has such pairs.  There the reference is compared with the closed form
instead: the proxy term is constant 0 around a zero direction (divide_no_nan), the vertex error is |0 - target| <= 1, hence d/dv = vertex_w *
normaliser * (0 - target)."""
import numpy as np
import pytest
import torch

import loss_cases as Cs
import loss_functions_ref as F
import loss_reference as L
import torch_train_ref as R

TOL = 1e-12
W = Cs.WEIGHTS


def close(got, want):
    want = np.asarray(want, np.float64)
    scale = np.abs(want).max()
    return np.abs(np.asarray(got) - want).max() <= TOL * scale if scale > 0 else not np.asarray(got).any()


def unit_targets(kpts, fg, h, w):
    """[b,h,w,kp,2]: unit vectors from the pixel centres to the keypoints of the pixel's label (anything on background)"""
    b = fg.shape[0]
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    a = kpts.astype(np.float64)[np.arange(b)[:, None, None], np.maximum(fg.astype(np.int64) - 1, 0)] - np.stack([yy, xx], -1)[None, :, :, None, :]
    return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-12)


def compare_direction_gradient(ref, want, zero_pairs, closed_form):
    """want: the oracle's gradient [b,h,w,kp,2]; NaN exactly on `zero_pairs` [b,h,w,kp], where the closed form takes its place"""
    got = ref.reshape(want.shape)
    assert np.array_equal(np.isnan(want).any(-1), zero_pairs) and np.array_equal(np.isnan(want).all(-1), zero_pairs)
    assert np.isfinite(got).all()
    assert close(np.where(zero_pairs[..., None], 0.0, got), np.where(zero_pairs[..., None], 0.0, want))
    if zero_pairs.any():
        assert close(got[zero_pairs], closed_form[zero_pairs])


def oracle_merged(c, seg, prox):
    lab_ce, lab_fg = (torch.from_numpy(a.astype(np.int64)) for a in (c.labels_ce, c.labels_fg))
    kp64 = torch.from_numpy(c.kpts.astype(np.float64))
    ot = torch.tensor(c.out.astype(np.float64), requires_grad=True)
    if np.array_equal(c.labels_ce, c.labels_fg):
        ml, vl, pl = R.losses(ot, lab_fg, kp64, c.K, c.kp, seg, prox)
    else:
        ml = R.losses(ot, lab_ce, kp64, c.K, c.kp, seg, prox)[0]
        _, vl, pl = R.losses(ot, lab_fg, kp64, c.K, c.kp, seg, prox)
    (W[0] * ml + W[1] * vl + W[2] * pl).backward()
    return ml.item(), vl.item(), pl.item(), ot.grad.numpy()


@pytest.mark.parametrize("prox", (False, True), ids=("", "proxfilter"))
@pytest.mark.parametrize("seg", (False, True), ids=("", "segfilter"))
@pytest.mark.parametrize("name", Cs.MERGED)
def test_merged_reference_equals_the_autograd_oracle(name, seg, prox):
    c = Cs.checked(name)                                   # the case's properties, asserted on the reference
    r = Cs.reference(name, seg_filter=seg, proxy_filter=prox)
    ml, vl, pl, g = oracle_merged(c, seg, prox)
    assert close(r.mask, ml) and close(r.vertex, vl) and close(r.proxy, pl), ((r.mask, ml), (r.vertex, vl), (r.proxy, pl))
    b, h, w = c.labels_fg.shape
    assert close(r.grad_logits, g[..., :c.K])
    zero_pairs = (c.out[..., c.K:].reshape(b, h, w, c.kp, 2) == 0).all(-1)
    assert zero_pairs.any() == (name == "degenerate")
    nrm = 1.0 / ((2.0 * c.kp * r.count1 + 1e-3) * b)
    closed = -W[1] * nrm[:, None, None, None, None] * unit_targets(c.kpts, r.fg1, h, w) * (r.fg1 != 0)[..., None, None]
    compare_direction_gradient(r.grad_dirs, g[..., c.K:].reshape(b, h, w, c.kp, 2), zero_pairs, closed)
    # the stages hang together
    assert np.array_equal(r.count0, (r.fg0 != 0).reshape(b, -1).sum(1)) and np.array_equal(r.count1, (r.fg1 != 0).reshape(b, -1).sum(1))
    assert np.array_equal(r.objcnt.sum(1), r.count0) and ((r.fg1 == 0) | (r.fg1 == r.fg0)).all() and ((r.fg0 == 0) | (r.fg0 == c.labels_fg)).all()
    if not prox:
        assert np.array_equal(r.fg1, r.fg0)
    if not seg:
        assert np.array_equal(r.fg0, c.labels_fg)


def oracle_separated(c, seg):
    b, h, w = c.labels_fg.shape
    eye = torch.eye(c.K, dtype=torch.float64)
    hot_ce, hot_fg = (eye[torch.from_numpy(a.astype(np.int64))] for a in (c.labels_ce, c.labels_fg))
    pts = torch.from_numpy(c.kpts.astype(np.float64))[:, :, None]                            # [b,oc,1 instance,kp,2]
    ot = torch.tensor(c.out.astype(np.float64), requires_grad=True)
    zs, vs = ot[..., :c.K], ot[..., c.K:]
    field = F.get_all_vectorfields(hot_fg, pts, None, True)
    if np.array_equal(c.labels_ce, c.labels_fg):
        ml, vl, pl = F.compute_loss_separated(zs, hot_fg, vs, field, pts, seg)
    else:
        ml = F.compute_loss_separated(zs, hot_ce, vs, F.get_all_vectorfields(hot_ce, pts, None, True), pts, seg)[0]
        _, vl, pl = F.compute_loss_separated(zs, hot_fg, vs, field, pts, seg)
    (W[0] * ml + W[1] * vl + W[2] * pl).backward()
    return ml.item(), vl.item(), pl.item(), ot.grad.numpy()


@pytest.mark.parametrize("seg", (False, True), ids=("", "segfilter"))
@pytest.mark.parametrize("K", Cs.SEP_K)
@pytest.mark.parametrize("name", Cs.SEP)
def test_separated_reference_equals_the_oracle(name, K, seg):
    c = Cs.checked(name, K, 9, True)
    r = Cs.reference(name, K, 9, True, seg_filter=seg)
    ml, vl, pl, g = oracle_separated(c, seg)
    assert close(r.mask, ml) and close(r.vertex, vl) and close(r.proxy, pl), ((r.mask, ml), (r.vertex, vl), (r.proxy, pl))
    b, h, w = c.labels_fg.shape
    assert close(r.grad_logits, g[..., :K])
    oc, kp = K - 1, c.kp
    zero_pairs = (c.out[..., K:].reshape(b, h, w, oc * kp, 2) == 0).all(-1)
    assert zero_pairs.any() == (name == "degenerate")
    own = np.zeros((b, h, w, oc, kp), bool)                                                  # the slice of the pixel's own (kept) object
    for o in range(oc):
        own[..., o, :] = (r.fg == o + 1)[..., None]
    nrm = (1.0 / ((2.0 * kp * r.counts + 1e-3) * b))[np.arange(b)[:, None, None], r.fg.astype(np.int64)]
    closed = (-W[1] * nrm[..., None, None, None] * unit_targets(c.kpts, r.fg, h, w)[:, :, :, None] * own[..., None]).reshape(b, h, w, oc * kp, 2)
    compare_direction_gradient(r.grad_dirs, g[..., K:].reshape(b, h, w, oc * kp, 2), zero_pairs, closed)
    assert np.array_equal(r.counts[:, 1:].sum(1), (r.fg != 0).reshape(b, -1).sum(1)) and not r.counts[:, 0].any()
    assert not r.grad_dirs.reshape(b, h, w, oc, kp, 2)[~own].any()                           # nothing outside the pixel's own slice


def test_first_argmax_takes_the_first_of_equal_maxima():
    z = np.float64([[1, 3, 3, 0], [2, 2, 2, 2], [0, 1, 2, 2], [5, 1, 5, 5], [-1, -1, -2, -3]])
    assert L.first_argmax(z).tolist() == [1, 0, 2, 0, 0]
    lab = np.uint8([1, 0, 3, 2, 1])
    assert L.segmentation_filter(z, lab).tolist() == [1, 0, 0, 0, 0]


@pytest.mark.parametrize("name", ("second_trip_merged", "second_trip_sep"))
def test_large_cases_have_their_properties(name):
    """the two large cases are not compared with the oracles (the same code as the small ones runs on them); their properties are asserted"""
    c = Cs.checked(name)
    assert c.labels_fg.shape == {"second_trip_merged": (2, 260, 508), "second_trip_sep": (2, 516, 512)}[name] and (c.K, c.kp) == (3, 2)


@pytest.mark.parametrize("K,kp", Cs.RECORD_SHAPES)
def test_layout_sweep_cases_have_their_properties(K, kp):
    c = Cs.checked("subset_fg", K, kp)
    assert len(np.unique(c.labels_ce)) == K and c.out.shape[-1] == K + 2 * kp
