"""Training on several instances of one object, above the loss kernel (tests/test_gpu_instance_loss.py):
  the device scenes with an instance axis -- labels, instance_seg, counts and the small arrays byte-equal to the host path, two renders the same bytes;
  one train_step on a plan at 96 x 128 -- the returned losses and plan.dout equal tests/instance_loss_reference.py's merged_instances evaluated on
  plan.out, to test_gpu_loss_stages.py's bounds, the gradient multiplied by the plan's 2^loss_exp, under both rules; three steps train;
  the refusals, each naming what it refuses."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import instance_loss_reference as RI
from test_gpu_loss_stages import GRAD_TOL, SUM_TOL, block_error

pytestmark = pytest.mark.gpu
OC, I, KP = 2, 3, 9


def test_device_scenes_equal_the_host_path(device):
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset

    ds = SyntheticSceneDataset(OC, (48, 64), length=8, seed=21, instances=I)
    host = ds.batch(1, 2)
    first, second = ds.batch(1, 2, device=device), ds.batch(1, 2, device=device)
    torch.cuda.synchronize(device)
    assert list(first) == list(host)
    assert host["instance_count"].max() >= 2
    for k in ("target_seg", "filtered_seg", "instance_seg", "instance_count", "pixel_gt_count", "keypoints3d", "target_vert", "cam_mat", "diameters", "offsets",
              "poses_gt"):
        a, b = host[k], first[k].cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), k
    assert first["img"].shape == host["img"].shape and first["img"].dtype == host["img"].dtype
    for k in first:
        assert first[k].cpu().numpy().tobytes() == second[k].cpu().numpy().tobytes(), k
    # the noise is another sample of the same distribution: the noise-free pictures agree
    scenes = ds.device_scenes(device)
    clean, done = scenes.launch_records(scenes.host_half(range(2, 4))["records"], noise=False)
    done.synchronize()
    want = np.stack([ds._render(np.random.default_rng([ds.seed, i]), noise=False)["img"] for i in range(2, 4)])
    assert np.abs(clean["img"].cpu().numpy() - want).max() < 1e-6


@pytest.fixture(scope="module")
def trained(device):
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_models.tfkeras import Classifiers

    b, h, w, k = 2, 96, 128, OC + 1
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=k, input_shape=(h, w, 3), input_segmentation_shape=(h, w, k), weights=None,
                                             base_model="resnet18", device=device, seed=3)
    ds = SyntheticSceneDataset(OC, (h, w), length=8, seed=4, instances=2)
    batch = next(bt for bt in (ds.batch(i, b) for i in range(4)) if bt["instance_count"].max() == 2)
    return net, batch


def options(**kw):
    return SimpleNamespace(**dict(dict(train_vectors_with_ground_truth=True, estimate_coords=False, max_keypoint_pixel_error=12.5,
                                       confidence_regularization=False, use_bpnp_reprojection_loss=False), **kw))


def factors(seg_filter=True):
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler

    return LossWeightHandler(1.0, 0.5, 0.015, 0.0, filter_vertex_with_segmentation=seg_filter)


@pytest.mark.parametrize("rule", ("map", "nearest"))
def test_a_step_equals_the_reference_on_the_plans_output(device, trained, monkeypatch, rule):
    from casapose_amd.training import train_step

    net, batch = trained
    monkeypatch.setenv("CASAPOSE_TRAIN_INSTANCE_RULE", rule)
    lf = factors(seg_filter=False)     # an untrained network: its arg-max would leave the segmentation filter little foreground
    got = train_step(net, batch, lf, None, options(), train=False)
    plan, _ = net.training_plan(2, 96, 128)
    torch.cuda.synchronize(device)
    k = OC + 1
    out = plan.out_view.cpu().numpy()
    lab = batch["filtered_seg"].numpy()[..., 0].astype(np.uint8)
    imap = batch["instance_seg"].numpy() if rule == "map" else None
    wts = (1.0, 0.5, 0.015)
    ref = RI.merged_instances(out, lab, lab, batch["target_vert"].numpy(), batch["instance_count"].numpy(), imap, k, KP, False, False, wts)
    assert ref.count1.min() >= 200
    if rule == "nearest":      # the rules differ on this batch: an occluded instance's pixels lie nearer to another centre
        mapped = RI.merged_instances(out, lab, lab, batch["target_vert"].numpy(), batch["instance_count"].numpy(), batch["instance_seg"].numpy(), k, KP, False,
                                     False, wts)
        print("pixels whose instance differs between the rules: %d" % int((mapped.raw.rv != ref.raw.rv).sum()))
    failed = []
    for i, name in enumerate(("mask", "vertex", "proxy")):
        want = getattr(ref, name)
        print("%s %.9g reference %.9g" % (name, got[1 + i], want))
        if not abs(got[1 + i] - want) < SUM_TOL * abs(want):
            failed.append("%s loss %.9g, reference %.9g" % (name, got[1 + i], want))
    if not abs(got[0] - (wts[0] * ref.mask + wts[1] * ref.vertex + wts[2] * ref.proxy)) < SUM_TOL * abs(got[0]):
        failed.append("total loss %.9g" % got[0])
    scale = 2.0 ** plan.loss_exp
    dout = plan.dout.cpu().numpy().astype(np.float64) / scale
    used = np.zeros(dout.shape[-1], bool)
    for name, first, width, want in (("logit", 0, k, ref.grad_logits), ("direction", plan.VERT_OFF, 2 * KP, ref.grad_dirs)):
        used[first:first + width] = True
        for n in range(2):
            err = block_error(dout[n, :, :, first:first + width], want[n])
            print("image %d %s block: %.2e" % (n, name, err))
            if not err < GRAD_TOL:
                failed.append("gradient, image %d, %s columns: %.3g" % (n, name, err))
    if dout[..., ~used].any():
        failed.append("non-zero gradient outside the logit and direction columns")
    assert not failed, " | ".join(failed)


def test_three_steps_train(device, trained, monkeypatch):
    from casapose_amd.training import Adam, train_step
    from casapose_amd.utils.learning_rate_schedules import PiecewiseConstantDecay

    net, batch = trained
    monkeypatch.delenv("CASAPOSE_TRAIN_INSTANCE_RULE", raising=False)
    before = {n: a.copy() for n, a in net.get_parameters().items()}
    optim = Adam(learning_rate=PiecewiseConstantDecay([5], [1e-3, 5e-4]))
    hist = np.array([train_step(net, batch, factors(), optim, options()) for _ in range(3)])
    assert np.isfinite(hist).all() and optim.iterations == 3
    after = net.get_parameters()
    assert np.abs(after["conv0.kernel"] - before["conv0.kernel"]).max() > 0 and all(np.isfinite(a).all() for a in after.values())


def test_refusals_name_what_they_refuse(device, trained, monkeypatch):
    from casapose_amd.training import train_step

    net, batch = trained
    monkeypatch.delenv("CASAPOSE_TRAIN_INSTANCE_RULE", raising=False)
    with pytest.raises(NotImplementedError, match="estimate_coords"):
        train_step(net, batch, factors(), None, options(estimate_coords=True), train=False)
    monkeypatch.setenv("CASAPOSE_TRAIN_INSTANCE_RULE", "centre")
    with pytest.raises(ValueError, match="CASAPOSE_TRAIN_INSTANCE_RULE"):
        train_step(net, batch, factors(), None, options(), train=False)
    monkeypatch.delenv("CASAPOSE_TRAIN_INSTANCE_RULE")
    with pytest.raises(ValueError, match="instance_count"):
        train_step(net, {k: v for k, v in batch.items() if k != "instance_count"}, factors(), None, options(), train=False)
    too_many = dict(batch, instance_count=batch["instance_count"] + 1)
    with pytest.raises(ValueError, match=r"inst_counts.*0\.\.2"):
        train_step(net, dict(too_many, instance_seg=None), factors(), None, options(), train=False)
    orphan = batch["instance_seg"].clone()
    orphan[batch["filtered_seg"][..., 0] != 0] = 2
    with pytest.raises(ValueError, match="filtered_seg disagrees with instance_seg"):
        train_step(net, dict(batch, instance_seg=orphan), factors(), None, options(), train=False)
    # the plan's own check of its second form
    plan, _ = net.training_plan(2, 96, 128)
    lab = batch["filtered_seg"][..., 0].to(device=device, dtype=torch.uint8).contiguous()
    kp = batch["target_vert"].to(device).contiguous()
    with pytest.raises(ValueError, match="inst_counts"):
        plan.loss_and_grad(lab, lab, kp)
    with pytest.raises(ValueError, match=r"inst_counts.*0\.\.2"):
        plan.loss_and_grad(lab, lab, kp, inst_counts=torch.full((2, OC), 3, dtype=torch.int32))
