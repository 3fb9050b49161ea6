"""`cp_bpnp_loss_f64` on the GPU (csrc/bpnp.hip through `DeviceBPnPLoss`) against the host path `training.bpnp_reprojection_loss_host`, at the
smallest shapes at which the kernels can go wrong: 15 blocks of nine keypoints (126 hypotheses: two waves busy, two idle), 2 blocks of five (one
hypothesis) and 2 of eleven (the sampled table of 256), blocks that leave by an early exit, and the training plan's call.  Batches, references and
gates are those of tests/test_bpnp_twin_host.py: from the host path alone, never from the device or its twin."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import test_bpnp_twin_host as B
import test_pnp_twin_host as T
from casapose_amd import training as TR
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation.device_bpnp import DeviceBPnPLoss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_call(device, batch, weight=1.0, avail=None):
    dev = DeviceBPnPLoss(device, batch.coords.shape[2])
    loss, g, poses = dev.loss_and_grad(batch.coords, batch.gt, batch.affine, batch.avail if avail is None else avail, batch.points_3d, T.K32, B.CAP, weight)
    assert loss.is_cuda and g.is_cuda and poses.is_cuda and loss.dtype == torch.float64 and g.dtype == torch.float32
    assert tuple(g.shape) == batch.coords.shape and tuple(poses.shape) == batch.coords.shape[:2] + (1, 3, 4)
    return float(loss.item()), g.cpu().numpy(), poses.cpu().numpy(), dev


@pytest.mark.parametrize("name", ["hard", "percam", "n5", "n11"])
def test_device_against_the_host_path(device, monkeypatch, name):
    batch, ref = B.make_batch(name), B.host_reference(name, monkeypatch)
    B.assert_preconditions(ref, name)
    loss, g, poses, dev = device_call(device, batch)
    on = batch.avail.reshape(-1) != 0
    assert dev.last_counts.tolist() == [int(on.sum()), 0]
    assert np.array_equal(dev.last_info.reshape(len(on), 4)[:, 0], np.where(on, 0, 1))
    assert not g.reshape(len(on), -1)[~on].any(), "an unavailable pair has exactly zero gradient"
    B.assert_loss_and_gradient(loss, g, ref, "device against the host path, %s" % name)
    B.assert_poses(poses, ref, on, "device against the host path, %s" % name)


def test_two_launches_are_bit_identical(device):
    batch = B.make_batch("hard")
    dev = DeviceBPnPLoss(device, 9)
    args = (batch.coords, batch.gt, batch.affine, batch.avail, batch.points_3d, T.K32, B.CAP, 0.5)
    first = [t.cpu().numpy().tobytes() for t in dev.loss_and_grad(*args)]
    info = dev.last_info
    second = [t.cpu().numpy().tobytes() for t in dev.loss_and_grad(*args)]
    assert first == second and np.array_equal(info, dev.last_info)


def test_early_exits_write_zeros(device, monkeypatch):
    """A collapsed vote, a NaN keypoint and unavailable pairs are handled inputs: their blocks leave by the block-uniform early path and still
    write their zeros; the output buffers are filled with NaN first."""
    hard, ref = B.make_batch("hard"), B.host_reference("hard", monkeypatch)
    batch = B.collapsed(hard)
    loss, g, poses, dev = device_call(device, batch)
    assert dev.last_counts.tolist() == [14, 1] and dev.last_info[1, 2].tolist() == [3, -1, 0, 0]
    assert not g[1, 2].any() and not poses[1, 2].any()
    cleared = hard.avail.copy()
    cleared[1, 2] = 0
    want_loss, want_g, _, _ = B.host_run(hard, monkeypatch, avail=cleared)
    B.assert_loss_and_gradient(loss, g, ref, "device, collapsed vote, against the host path without that pair", want_loss, want_g)
    # all unavailable, through launch() into buffers that hold NaN: every element is written
    dev = DeviceBPnPLoss(device, 9)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)   # noqa: E731
    g_d = torch.full((3, 5, 9, 2), float("nan"), device=device)
    loss_d = torch.full((1,), float("nan"), dtype=torch.float64, device=device)
    poses_d = torch.full((3, 5, 1, 3, 4), float("nan"), device=device)
    info_d, counts_d = torch.full((3, 5, 4), -7, dtype=torch.int32, device=device), torch.full((2,), -7, dtype=torch.int32, device=device)
    ws = torch.full((dev.workspace_bytes(3, 5) // 8,), float("nan"), dtype=torch.float64, device=device)
    dev.launch(up(hard.coords), up(hard.gt), up(hard.affine), torch.zeros(3, 5, device=device), up(hard.points_3d), up(T.K32), B.CAP, 1.0, g_d, loss_d, poses_d,
               info_d, counts_d, ws)
    assert loss_d.item() == 0.0 and not g_d.cpu().numpy().any() and not poses_d.cpu().numpy().any()
    assert dev.last_counts.tolist() == [0, 0] and (dev.last_info[..., 0] == 1).all()
    nan = hard.coords.copy()
    nan[0, 0, 4, 1] = np.nan
    loss, g, _, dev = device_call(device, hard._replace(coords=nan))
    assert dev.last_counts.tolist() == [14, 1] and dev.last_info[0, 0, 0] == 2 and np.isfinite(loss) and np.isfinite(g).all() and not g[0, 0].any()


# ---- the training plan -------------------------------------------------------------------------------------------------------------------
def plan_case(b, h, w, k):
    """-> labels [b,h,w] uint8, an output field [b,h,w,k+27] whose LS vote is the fixture's keypoints, those keypoints (y,x) [b,oc,9,2], gt (x,y),
    points_3d [b,oc,9,3]: the first b * oc cases of the "hard" set under its camera K32.  The keypoints lie up to a few hundred pixels outside the
    64 x 64 crop; the voter intersects lines, so that is a matter of conditioning only, and the test asserts where the votes land."""
    from test_gpu_train import blob_labels

    oc, kp = k - 1, 9
    cases = T.fixture_set("hard")[:b * oc]
    xy = np.stack([c.points_2d for c in cases]).astype(np.float64).reshape(b, oc, kp, 2)
    x3 = np.stack([c.points_3d for c in cases]).reshape(b, oc, kp, 3)
    gt = (xy + np.random.default_rng(3).normal(0, 2.0, xy.shape)).astype(np.float32)
    lab = blob_labels(b, h, w, k, 10)
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    pix = np.stack([yy, xx], -1)[:, :, None, :]
    dirs = np.zeros((b, h, w, kp, 2))
    for n in range(b):
        for o in range(oc):
            m = lab[n] == o + 1
            d = xy[n, o, :, ::-1][None, None] - pix
            dirs[n][m] = (d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9))[m]
    field = np.concatenate([8.0 * np.eye(k)[lab], dirs.reshape(b, h, w, 2 * kp), np.zeros((b, h, w, kp))], -1).astype(np.float32)
    return lab, field, np.ascontiguousarray(xy[..., ::-1]), gt, x3


def test_train_plan_device_loss_against_the_host_closure(device, monkeypatch):
    import casapose_oracle as O
    from casapose_amd.train_engine import ParamStore, TrainPlan, crop_to_image_affine

    b, h, w, k, kp, kp_w = 2, 64, 64, 5, 9, 0.007
    lab, field, want_yx, gt, x3 = plan_case(b, h, w, k)
    plan = TrainPlan(ParamStore(O.init_params(k, 27, seed=5, dtype=np.float32), device), k, 27, b, h, w)
    labd = torch.from_numpy(lab).to(device)
    plan.refresh_weights(torch.cuda.current_stream(device).cuda_stream)
    plan.forward(torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (b, h, w, 3)).astype(np.float32)).to(device), labd)
    plan.out_view.copy_(torch.from_numpy(field))
    aff = torch.from_numpy(crop_to_image_affine(np.tile(np.array([[0.0, 0, 0, 0, 0, 0, 0, 1, 64, 64]]), (b, 1)))).to(device)
    gt_d = torch.from_numpy(gt).to(device)
    seen = {}

    def host_loss(c, av):
        seen["coords"], seen["avail"] = c.cpu().numpy(), av.cpu().numpy()
        return TR.bpnp_reprojection_loss_host(c, gt_d, aff, av, x3, T.K32, B.CAP, kp_w, rng=np.random.default_rng(0))[:2]

    call = dict(max_pixel_error=B.CAP, min_num=50, confidence_regularization=False, vote_with_gt=True, backward=False)
    host_val = float(plan.kp_loss_and_grad(labd, gt_d, aff, kp_w, host_loss=host_loss, **call).item())
    host_g = plan.ls_g.cpu().numpy().astype(np.float64)
    assert seen["avail"].all(), "every object of the synthesised field must be available"
    assert np.abs(seen["coords"] - want_yx).max() < 1.0, "the votes must land within a pixel of the fixture's keypoints"
    # gates of this batch, from the host path: the stopping-iterate spread (with the hard set's), and the four seeds must agree within them
    batch = B.Batch(seen["coords"], gt, aff.cpu().numpy().reshape(b, 6), seen["avail"], x3)
    runs = [TR.bpnp_reprojection_loss_host(batch.coords, gt, batch.affine, batch.avail, x3, T.K32, B.CAP, kp_w, rng=np.random.default_rng(s)) for s in range(4)]
    orig = P.refine_lm
    with monkeypatch.context() as m:
        m.setattr(P, "refine_lm", lambda *a, **kw: orig(*a, **(dict(kw, iters=100, eps=1e-16) if kw.get("iters") == 30 else kw)))
        tight = TR.bpnp_reprojection_loss_host(batch.coords, gt, batch.affine, batch.avail, x3, T.K32, B.CAP, kp_w, rng=np.random.default_rng(0))
    g0 = runs[0][1].astype(np.float64)
    pair_max = np.abs(g0).reshape(b * (k - 1), -1).max(axis=1)
    hard = B.host_reference("hard", monkeypatch)
    s_g = max(float((np.abs(tight[1] - g0).reshape(len(pair_max), -1).max(axis=1) / pair_max).max()), hard.s_g)
    s_l = max(abs(tight[0] - runs[0][0]) / abs(runs[0][0]), hard.s_l)
    ref = hard._replace(loss=runs[0][0], g=g0, s_g=s_g, s_l=s_l, gate_g=100.0 * s_g + 8.0 * B.ULP32, gate_l=100.0 * s_l + 8.0 * B.ULP64)
    for s in range(1, 4):
        B.assert_loss_and_gradient(runs[s][0], runs[s][1], ref, "host seed %d against seed 0" % s)
    # the device path, into the same buffers
    dev = DeviceBPnPLoss(device, kp).bind(x3, T.K32)
    plan.ls_g.fill_(float("nan"))
    dev_val = float(plan.kp_loss_and_grad(labd, gt_d, aff, kp_w, device_loss=dev, **call).item())
    assert plan.bpnp_counts.cpu().tolist() == [b * (k - 1), 0] and (plan.bpnp_info.cpu().numpy()[..., 0] == 0).all()
    assert tuple(plan.bpnp_poses.shape) == (b, k - 1, 1, 3, 4)
    B.assert_loss_and_gradient(dev_val, plan.ls_g.cpu().numpy(), ref, "plan: device_loss against the host closure", want_loss=host_val,
                               want_g=host_g)   # (ls_g as the plan keeps it: both paths carry the plan's loss scale)
    T.assert_within_gates(plan.bpnp_poses.cpu().numpy().reshape(-1, 3, 4), runs[0][2].reshape(-1, 3, 4), T.host_reference("hard"), "plan: device poses")
    with pytest.raises(ValueError, match="not both"):
        plan.kp_loss_and_grad(labd, gt_d, aff, kp_w, host_loss=host_loss, device_loss=dev, **call)


CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch
import test_gpu_bpnp as G
from casapose_amd.pose_estimation import pnp
def host_pnp(*a, **k):
    raise AssertionError("the host PnP ran")
pnp.pnp_rvec_t = host_pnp
losses, changed, unsolved = G.one_train_step(torch.device("cuda:0"))
print("losses " + " ".join(repr(float(v)) for v in losses))
print("changed %%d unsolved %%d" %% (changed, unsolved))
"""


def step_inputs(device):
    """The factory model and a batch at test_gpu_train.py::test_model_api_train_step's smallest shape (k = 5, 64 x 64, b = 2) with
    use_bpnp_reprojection_loss -> (net, batch, loss factors, options)"""
    from types import SimpleNamespace

    import torch_train_ref as R
    from casapose_amd.pose_models.tfkeras import Classifiers
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler
    from test_gpu_train import blob_labels

    b, h, w, k, kp = 2, 64, 64, 5, 9
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=k, input_shape=(h, w, 3), input_segmentation_shape=(h, w, k), weights=None,
                                             base_model="resnet18", device=device, seed=3)
    rng = np.random.default_rng(3)
    lab = blob_labels(b, h, w, k, 10)
    cam = np.array([[100.0, 0, 32.0], [0, 100.0, 32.0], [0, 0, 1]])
    p3d = rng.uniform(-20, 20, (b, k - 1, 1, kp, 3))
    poses = np.zeros((b, k - 1, 1, 3, 4))
    poses[..., :3, :3] = np.eye(3)
    poses[..., 2, 3] = 100.0
    xy = R.project_points(p3d.reshape(-1, kp, 3), cam, poses.reshape(-1, 3, 4)).reshape(b, k - 1, 1, kp, 2)
    batch = dict(img=torch.from_numpy(rng.uniform(-1, 1, (b, h, w, 3)).astype(np.float32)), target_seg=torch.from_numpy(np.eye(k, dtype=np.float32)[lab]),
                 keypoints3d=torch.from_numpy(p3d), target_vert=torch.from_numpy(xy[..., ::-1].copy()), cam_mat=torch.from_numpy(cam),
                 offsets=torch.from_numpy(np.tile(np.array([[0.0, 0, 0, 0, 0, 0, 0, 1, 64, 64]]), (b, 1))), poses_gt=torch.from_numpy(poses))
    opt = SimpleNamespace(train_vectors_with_ground_truth=True, estimate_coords=True, max_keypoint_pixel_error=12.5, confidence_regularization=True,
                          use_bpnp_reprojection_loss=True)
    return net, batch, LossWeightHandler(1.0, 0.5, 0.015, 0.007, filter_vertex_with_segmentation=True), opt


def one_train_step(device):
    """One train_step on step_inputs -> (the five losses, whether conv0's kernel changed, the plan's count of unsolved pairs)"""
    net, batch, lf, opt = step_inputs(device)
    before = net.get_parameters()["conv0.kernel"].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)   # an untrained network's votes may leave pairs unsolved: said once, counted below
        losses = TR.train_step(net, batch, lf, TR.Adam(learning_rate=1e-3), opt)
    plan, _ = net.training_plan(2, 64, 64, None, 1)
    return losses, not np.array_equal(net.get_parameters()["conv0.kernel"], before), int(plan.bpnp_unsolved)


def test_train_step_switch_in_a_fresh_process(device, monkeypatch):
    """CASAPOSE_DEVICE_BPNP=1: train_step says `bpnp: device` once, never calls the host PnP, returns five finite losses and updates the weights;
    without the variable the host path runs as before."""
    env = dict(os.environ, CASAPOSE_DEVICE_BPNP="1")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines.count("bpnp: device") == 1
    losses = [float(v) for v in [ln for ln in lines if ln.startswith("losses ")][0].split()[1:]]
    assert len(losses) == 5 and np.isfinite(losses).all()
    assert [ln for ln in lines if ln.startswith("changed ")][0].startswith("changed 1 ")
    # the host path, in this process
    monkeypatch.delenv("CASAPOSE_DEVICE_BPNP", raising=False)
    calls, host_pnp = [], P.pnp_rvec_t
    monkeypatch.setattr(P, "pnp_rvec_t", lambda *a, **k: calls.append(1) or host_pnp(*a, **k))
    losses, changed, unsolved = one_train_step(device)
    assert len(calls) > 0 and len(losses) == 5 and np.isfinite(losses).all() and changed and unsolved == 0


def test_train_step_warns_once_about_unsolved_pairs(device, monkeypatch):
    """The unsolved-pair rule through train_step: given coordinates (the "hard" set's first eight pairs, one of them a collapsed vote) with every
    object counted as available, the step stays finite, warns once per plan and keeps the running count."""
    monkeypatch.setenv("CASAPOSE_DEVICE_BPNP", "1")
    net, batch, lf, opt = step_inputs(device)
    cases = T.fixture_set("hard")[:8]
    xy, x3 = T.batch_of(cases, 2, 4)
    coords = np.ascontiguousarray(xy[..., ::-1])
    coords[1, 2] = np.float32([20.25, 31.5])
    batch = dict(batch, cam_mat=torch.from_numpy(T.K32.astype(np.float64)), keypoints3d=torch.from_numpy(x3[:, :, None].astype(np.float64)))
    optim = TR.Adam(learning_rate=1e-3)
    with pytest.warns(UserWarning, match="1 available .* unsolved") as caught:
        first = TR.train_step(net, batch, lf, optim, opt, coords=torch.from_numpy(coords).to(device), min_num=-1)
    assert len([w for w in caught if "unsolved" in str(w.message)]) == 1
    plan, _ = net.training_plan(2, 64, 64, None, 1)
    assert plan.bpnp_unsolved == 1 and plan.bpnp_counts.cpu().tolist() == [7, 1] and plan.bpnp_info[1, 2, 0].item() == 3
    with warnings.catch_warnings(record=True) as again:
        warnings.simplefilter("always")
        second = TR.train_step(net, batch, lf, optim, opt, coords=torch.from_numpy(coords).to(device), min_num=-1)
    assert not [w for w in again if "unsolved" in str(w.message)] and plan.bpnp_unsolved == 2
    assert np.isfinite(first).all() and np.isfinite(second).all() and first[4] > 0
