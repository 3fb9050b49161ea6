"""Digest of `initial_parameters` for every registry variant (the oracle's VARIANTS with its SHARED sharing, plus PVNet): the key order
and one sha256 over (key, shape, float32 bytes) per seg_dim, seed 0.  Key order and values pin the RNG draw order, which seeded weights
and the HDF5 writer's layer order depend on.  Generated from the tree before the graph moved into casapose_amd/architecture.py.
Run:  python tests/golden/make_arch_golden.py  ->  tests/golden/initial_parameters_digest.json"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

SEG_DIMS = (4, 9)
VER_DIM = 27
DIMS = (256, 128, 64, 32, 32)


def variant_kwargs():
    import casapose_oracle as O

    out = {name: dict(partial=O.VARIANTS[name][0], **O.SHARED.get(name, {})) for name in sorted(O.VARIANTS)}
    out["pvnet"] = dict(pvnet=True)
    return out


def digest(params):
    h = hashlib.sha256()
    for k, v in params.items():
        h.update(("%s%s" % (k, v.shape)).encode())
        h.update(v.astype("<f4").tobytes())
    return h.hexdigest()


def main():
    from casapose_amd.pose_models.models.model import initial_parameters

    out = {}
    for name, kw in variant_kwargs().items():
        runs = {k: initial_parameters(k, VER_DIM, DIMS, seed=0, **kw) for k in SEG_DIMS}
        out[name] = dict(keys=list(runs[SEG_DIMS[0]]), sha256={str(k): digest(p) for k, p in runs.items()})
    with open(os.path.join(HERE, "initial_parameters_digest.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
