"""The LS voter with a given (component-filtered) label map reads the records of only those 64-pixel row segments that hold a kept pixel.
Its keypoints against oracle.ls_voting(..., filter_estimates=True), with the gate of test_gpu_voting.test_filtered_ls_voting_matches_fixture
(0.05 px), where the skipping has edges: kept pixels on strip corners, on the last row, in the last partial strip; nothing kept; everything
kept; and the generic kernel (another record stride)."""
import numpy as np
import pytest
import torch

import casapose_oracle as O

pytestmark = pytest.mark.gpu

GATE = 0.05  # px, as in test_filtered_ls_voting_matches_fixture


def _scene(h, w, boxes, seed, background_logit=4.0):
    """Eight objects, object o + 1 = the union of the boxes (y0, y1, x0, x1) in boxes[o]; unit directions towards nine keypoints per object with
    angular noise, N(0,1) confidences.  Returns seg [1,h,w,9], direct [1,h,w,18], conf [1,h,w,9] and the label map."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((h, w), np.int64)
    for o, bs in enumerate(boxes):
        for (y0, y1, x0, x1) in bs:
            lab[y0:y1, x0:x1] = o + 1
    seg = (rng.standard_normal((1, h, w, 9)) * 0.1).astype(np.float32)
    seg += background_logit * O.onehot_from_labels(lab[None], 9, np.float32)
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    direct = rng.standard_normal((1, h, w, 9, 2))  # anything outside the objects
    for o in range(8):
        m = lab == o + 1
        if not m.any():
            continue
        cy, cx = yy[m].mean(), xx[m].mean()
        kp = np.stack([cy + rng.uniform(-25, 25, 9), cx + rng.uniform(-25, 25, 9)], -1)
        ang = np.arctan2(kp[None, :, 0] - yy[m][:, None], kp[None, :, 1] - xx[m][:, None]) + 0.05 * rng.standard_normal((m.sum(), 9))
        direct[0][m] = np.stack([np.sin(ang), np.cos(ang)], -1)
    conf = rng.standard_normal((1, h, w, 9))
    return seg, direct.reshape(1, h, w, 18).astype(np.float32), conf.astype(np.float32), lab


def _vote(device, seg, direct, conf, ld=36):
    from casapose_amd.pose_estimation.voting_layers_2d import CoordLSVotingWeighted

    b, h, w, _ = seg.shape
    rec = torch.zeros(b, h, w, ld, device=device)
    rec[..., :36] = torch.from_numpy(np.concatenate([seg, direct, conf], -1)).to(device)
    s, d, c = rec[..., 0:9], rec[..., 9:27], rec[..., 27:36]  # slices of one record: voted in place, ld = 36 is the production kernel
    return CoordLSVotingWeighted("coords_ls_voting", 9, filter_estimates=True)([s, d, c]).cpu().numpy()


def _edge_boxes(h, w):
    """About 1.5 % of a 150-row, ~200-column image, one component per object, each at least 50 px (the filter's threshold), on the edges of the
    64 x 16 strips: rows 16 k, columns 64 k, the last row and the last (partial) strip."""
    assert h == 150 and 200 <= w < 256
    return [
        [(12, 20, 60, 68)],          # over the corner of four strips at (16, 64)
        [(28, 36, 124, 132)],        # over the corner at (32, 128)
        [(145, 150, 10, 20)],        # on the last row, inside the ragged last strip row (rows 144..149)
        [(40, 50, 193, w)],          # inside the last partial strip (columns 192..)
        [(143, 150, 188, w)],        # bottom-right corner: over row 144 and column 192, on the last row and the last column
        [(0, 7, 0, 8)],              # top-left corner: the first row of a strip
        [(79, 80, 100, 160)],        # one row only, the LAST row of its strips, over column 128
        [(81, 141, 63, 64)],         # one column only, the last lane of the first strip, through four strip rows
    ]


@pytest.mark.parametrize("w", [200, 203])  # 200: label words (W % 4 == 0); 203: label bytes
@pytest.mark.parametrize("ld", [36, 40])   # 36: the production kernel; 40: the generic kernel (case d)
def test_sparse_kept_pixels_on_strip_edges(device, w, ld):
    h = 150
    seg, direct, conf, lab = _scene(h, w, _edge_boxes(h, w), seed=7)
    assert h % 16 != 0 and w % 64 != 0
    frac = (lab > 0).mean()
    assert 0.005 < frac < 0.02
    want = O.ls_voting(seg, direct, conf, filter_estimates=True)
    assert np.isfinite(want).all() and all(np.abs(want[0, o]).max() > 0 for o in range(8))  # every object is kept and votes
    got = _vote(device, seg, direct, conf, ld)
    err = np.abs(got - want).max()
    print("sparse w=%d ld=%d: kept %.2f %%, max |keypoint - oracle| = %.3g px" % (w, ld, 100 * frac, err))
    assert err < GATE


@pytest.mark.parametrize("ld", [36, 40])
def test_no_kept_pixel_gives_zeros(device, ld):
    """Image 0 is background only; image 1 holds one object larger than the rest of the image, which the reference's component rule drops
    (test_gpu_voting.test_ccl_object_larger_than_rest_of_image_is_dropped).  No pixel is kept: exact zeros, as before and as the oracle."""
    h, w = 70, 136
    s0, d0, c0, _ = _scene(h, w, [[] for _ in range(8)], seed=1)
    s1, d1, c1, _ = _scene(h, w, [[(2, 68, 2, 134)]] + [[] for _ in range(7)], seed=2)
    seg, direct, conf = (np.concatenate(p, 0) for p in ((s0, s1), (d0, d1), (c0, c1)))
    want = O.ls_voting(seg, direct, conf, filter_estimates=True)
    assert not want.any()
    got = _vote(device, seg, direct, conf, ld)
    assert got.shape == (2, 8, 9, 2) and not got.any()


@pytest.mark.parametrize("ld", [36, 40])
def test_every_pixel_kept(device, ld):
    """Eight rectangles tile the image: every object is one component smaller than the rest, so the filter keeps every pixel and every row segment
    is read."""
    h, w = 150, 200
    boxes = [[(75 * (o // 4), 75 * (o // 4) + 75, 50 * (o % 4), 50 * (o % 4) + 50)] for o in range(8)]
    seg, direct, conf, lab = _scene(h, w, boxes, seed=3)
    assert (lab > 0).all()
    want = O.ls_voting(seg, direct, conf, filter_estimates=True)
    assert np.isfinite(want).all() and all(np.abs(want[0, o]).max() > 0 for o in range(8))
    got = _vote(device, seg, direct, conf, ld)
    err = np.abs(got - want).max()
    print("dense ld=%d: max |keypoint - oracle| = %.3g px" % (ld, err))
    assert err < GATE


def test_given_labels_equal_masked_argmax_vote(device):
    """The same sums by both paths of the production kernel: a label map handed in (rows without a label skipped) against the arg-max inside the
    kernel on logits whose arg-max is that label map (every row read).  The fp32 terms are the same, only fp64 additions reorder."""
    from casapose_amd import ops

    h, w = 150, 200
    seg, direct, conf, lab = _scene(h, w, _edge_boxes(h, w), seed=11)
    rec = torch.from_numpy(np.concatenate([seg, direct, conf], -1)).to(device)
    labels = torch.from_numpy(lab[None].astype(np.uint8)).to(device)
    a, sa = ops.ls_vote(rec, 0, 9, 27, 8, labels=labels, return_sums=True)
    b, sb = ops.ls_vote(rec, 0, 9, 27, 8, labels=None, return_sums=True)
    sa, sb = sa.cpu().numpy(), sb.cpu().numpy()
    assert np.abs(sa - sb).max() <= 1e-12 * np.abs(sb).max()
    assert np.abs(a.cpu().numpy() - b.cpu().numpy()).max() < 1e-3
