"""tests/instance_loss_reference.py (the fp64 restatement the GPU tests of cp_pose_loss_inst_f32 compare with) pinned on the CPU:
  I = 1          : it equals tests/loss_reference.py's `merged`, values and gradients, on every small case of tests/loss_cases.py, all four
                   filter combinations;
  I > 1, full counts, the nearest-centre rule : its target field equals oracle/loss_functions_ref.compute_vertex_hcoords_batch_v3, its proxy value
                   equals the oracle's proxy_voting_loss_v2 and its per-object values equal proxy_voting_dist.
The bound is tests/test_loss_reference.py's.  The property assertions of tests/instance_loss_cases.py run here as well, on the reference."""
import numpy as np
import pytest
import torch

import instance_loss_cases as Ci
import instance_loss_reference as RI
import loss_cases as Cs
import loss_functions_ref as F
from test_loss_reference import close

W = Cs.WEIGHTS


@pytest.mark.parametrize("prox", (False, True), ids=("", "proxfilter"))
@pytest.mark.parametrize("seg", (False, True), ids=("", "segfilter"))
@pytest.mark.parametrize("name", Cs.MERGED)
def test_one_instance_equals_the_merged_reference(name, seg, prox):
    c = Cs.checked(name)
    want = Cs.reference(name, seg_filter=seg, proxy_filter=prox)
    kpts, counts = Ci.single_instance(c)
    got = RI.merged_instances(c.out, c.labels_ce, c.labels_fg, kpts, counts, None, c.K, c.kp, seg, prox, W)
    for n in ("fg0", "count0", "objcnt", "bad", "fg1", "count1"):
        assert np.array_equal(getattr(got, n), getattr(want, n)), n
    for n in ("objsum", "value", "mask", "vertex", "proxy", "grad_logits", "grad_dirs"):
        assert close(getattr(got, n), getattr(want, n)), n


def full_count_case(seed, I):
    rng = np.random.default_rng(seed)
    b, h, w, K, kp = 2, 24, 32, 4, 9
    counts = np.full((b, K - 1), I, np.int32)
    out, ce, fg, kpts, counts, imap, K, kp = Ci.settle(rng, lambda: Ci._random_inputs(rng, counts, b, h, w, K, kp, I))
    fg = np.where(rng.random(fg.shape) < 0.9, fg, 0).astype(np.uint8)
    return out, ce, fg, kpts, counts, K, kp


@pytest.mark.parametrize("I", (2, 3, 5))
def test_several_instances_equal_the_oracle(I):
    out, ce, fg, kpts, counts, K, kp = full_count_case(40 + I, I)
    b, h, w = fg.shape
    r = RI.merged_instances(out, ce, fg, kpts, counts, None, K, kp, False, False, W)
    assert r.raw.on.sum() >= 300 and len(np.unique(r.raw.rv[r.raw.on])) == I and (r.raw.rp[r.raw.on] != r.raw.rv[r.raw.on][:, None]).any()
    pts = torch.from_numpy(kpts.astype(np.float64))
    lab = torch.from_numpy(fg.astype(np.int64))
    field = F.compute_vertex_hcoords_batch_v3(lab[..., None], pts).numpy()
    assert close(r.raw.target.reshape(b, h, w, -1), field)
    pred = torch.from_numpy(out[..., K:].astype(np.float64))
    hot = torch.eye(K, dtype=torch.float64)[lab][..., 1:]
    wts = (lab != 0).to(torch.float64)[..., None]
    assert close(r.proxy, F.proxy_voting_loss_v2(pred, pts, hot, wts).item())
    dist, per_object = F.proxy_voting_dist(pred, pts, hot, wts)
    assert close(r.raw.dist, dist.numpy()) and close(r.value, per_object.numpy())
    assert (r.objcnt >= 20).all()


@pytest.mark.parametrize("name", Ci.SMALL + ("second_trip",))
def test_cases_have_their_properties(name):
    Ci.checked(name)


@pytest.mark.parametrize("shape", Ci.LAYOUT_SHAPES, ids=str)
def test_layout_cases_have_their_properties(shape):
    Ci.checked("layouts", *shape)


def test_first_argmin_takes_the_first_of_equal_minima():
    v = torch.tensor([[1.0, 2.0, np.inf, 3.0], [1.0, 1.0, np.inf, 2.0], [0.5, 1.0, np.inf, 2.0]], dtype=torch.float64)
    assert RI.first_argmin(v).tolist() == [2, 1, 0, 1]
    assert RI.second_gap(v).tolist() == [0.5, 0.0, np.inf, 0.0]
