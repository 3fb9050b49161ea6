"""The graph description (casapose_amd/architecture.py) against the parameter sets it names, the flat buffer's forward order, and the
initial parameters of the tree it replaced (tests/golden/initial_parameters_digest.json, tests/golden/make_arch_golden.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import casapose_oracle as O
from casapose_amd.architecture import Arch, forward_order, graph
from casapose_amd.pose_models.models.model import initial_parameters

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_arch_golden as G  # noqa: E402

VARIANTS = G.variant_kwargs()
DIGEST = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "initial_parameters_digest.json")))


def records(g):
    """(layer, conv or norm record) in forward order"""
    yield g.bn_data
    yield g.conv0
    yield g.bn0
    for u in g.units:
        yield from (u.bn1, u.sc, u.conv1, u.bn2, u.conv2)
    yield g.bn1
    for b in g.decoder1:
        yield from (b.conv, b.norm)
    yield g.seg_head
    for b in g.decoder2:
        yield from (b.conv, b.norm)
    yield g.ver_head


def named(g, seg_dim):
    """{weight key: shape} of every record"""
    out = {}
    for r in records(g):
        if r is None:
            continue
        if hasattr(r, "key"):
            out[r.key] = r.shape
            continue
        tab = (seg_dim, r.channels) if r.clade else (r.channels,)
        out.update({r.name + ".gamma": tab} if r.gamma else {})
        out.update({r.name + ".beta": tab} if r.beta else {})
        out.update({r.name + ".moving_mean": (r.channels,), r.name + ".moving_variance": (r.channels,)})
    return out


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("seg_dim", G.SEG_DIMS)
def test_records_name_exactly_the_parameter_set_in_forward_order(variant, seg_dim):
    kw = VARIANTS[variant]
    g = graph(Arch(seg_dim, G.VER_DIM, G.DIMS, **kw))
    params = initial_parameters(seg_dim, G.VER_DIM, G.DIMS, seed=0, **kw)
    shapes = named(g, seg_dim)
    assert set(shapes) == set(params)
    assert all(tuple(params[k].shape) == s for k, s in shapes.items())
    # the gradient-bucket invariant (train_engine.ParamStore / TrainPlan.backward) for this variant: its layers in forward order
    rank = {n: i for i, n in enumerate(forward_order())}
    layers = list(dict.fromkeys(r.key.split(".")[0] if hasattr(r, "key") else r.name for r in records(g) if r is not None))
    assert all(n in rank for n in layers)
    assert [rank[n] for n in layers] == sorted(rank[n] for n in layers)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_initial_parameters_match_the_digest_fixture(variant):
    """same keys in the same insertion order (model.layers and the HDF5 writer follow it) and bit-identical seeded values"""
    ref = DIGEST[variant]
    for k in G.SEG_DIMS:
        p = initial_parameters(k, G.VER_DIM, G.DIMS, seed=0, **VARIANTS[variant])
        assert list(p) == ref["keys"]
        assert G.digest(p) == ref["sha256"][str(k)], (variant, k)


def test_arch_normalises_the_variant_switches():
    a = Arch(9, 27, [256, 128, 64, 32, 32], partial=[1, 0, 1, 0, 1], shared=np.array([0, 1, 0, 0, 0]))
    assert a.partial == (True, False, True, False, True) and a.shared == (False, True, False, False, False)
    assert a == Arch(9, 27, partial=(True, False, True, False, True), shared=(False, True, False, False, False))
    with pytest.raises(ValueError):
        Arch(9, 27, partial=(True,) * 4)


def test_decoder2_bilinear_without_guided_is_refused_by_both_plans():
    bil = dict(guided=(False, True, False, True, False), bilinear=(False, True, True, False, False))
    with pytest.raises(NotImplementedError):
        Arch(9, 27, **bil)
    from casapose_amd.train_engine import ParamStore, TrainPlan

    store = ParamStore(O.init_params(4, 27, seed=1, dtype=np.float32), torch.device("cpu"))
    with pytest.raises(NotImplementedError):   # before any device work
        TrainPlan(store, 4, 27, 2, 64, 96, **bil)
    from casapose_amd.engine import CasaposeNet

    with pytest.raises(NotImplementedError):
        CasaposeNet({}, 4, 27, torch.device("cuda"), **bil)
