#!/usr/bin/env python3
"""Generate tests/golden/plane_fit.npz by running the REFERENCE's own Plane3D on seeded points.

TEST INFRASTRUCTURE ONLY (CPU, no GPU), run where a checkout of the reference exists:

    python tools/gen_golden_plane.py --reference <path to the reference checkout>

What is imported from the reference: src/plane_3d.py (Plane3D).  Its plotting imports (matplotlib, mpl_toolkits) are replaced by empty
stub modules in this script only; they take no part in the arithmetic recorded here.

Recorded, for N_TRIPLES seeded point triples [T, 3, 3] (rows = points) and one seeded cloud [N_CLOUD, 3] of the test scene's ranges:
  fit_param [T, 4]                  Plane3D.fit(triple, "min").param
  eval_none [T, N], eval_x1 / eval_x2 [T, N]   .eval(cloud) for the weight methods "none" and "x norm" with norm 1 and 2 (x0 = X0)
  vec1, vec2, pt1 [T, 3], vec_param [T, 4]     create_plane_from_vectors_and_point
  angles [T], rot_param [T, 4]      rotate_around_axis("y", angle) applied to the fitted plane
  vectors [T, 3], angle [T], angle_xz [T]      normal_angle_to_vector / normal_angle_to_vector_xz of the fitted plane
Data only -- no reference source text.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OUT = os.path.join(REPO, "tests", "golden", "plane_fit.npz")
SEED, N_TRIPLES, N_CLOUD, X0 = 20261018, 16, 40, 1.5


def stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    stub("matplotlib", pyplot=stub("matplotlib.pyplot"))
    stub("mpl_toolkits", mplot3d=stub("mpl_toolkits.mplot3d", Axes3D=object))
    Plane3D = load_module("plane_3d", os.path.join(args.reference, "src", "plane_3d.py")).Plane3D

    rng = np.random.default_rng(SEED)
    lo, hi = np.array([-10.0, -30.0, -2.5]), np.array([80.0, 30.0, -1.0])
    triples = rng.uniform(lo, hi, size=(N_TRIPLES, 3, 3))
    cloud = rng.uniform(lo, hi + np.array([0.0, 0.0, 7.0]), size=(N_CLOUD, 3))
    vec1, vec2 = rng.normal(0.0, 3.0, size=(2, N_TRIPLES, 3))
    pt1 = rng.uniform(lo, hi, size=(N_TRIPLES, 3))
    angles = rng.uniform(-0.5, 0.5, size=N_TRIPLES)
    vectors = rng.normal(0.0, 1.0, size=(N_TRIPLES, 3))
    weights = {"none": {'method': "none"}, "x1": {'method': "x norm", 'param': {'x0': X0, 'norm': 1}},
               "x2": {'method': "x norm", 'param': {'x0': X0, 'norm': 2}}}
    out = {"triples": triples, "cloud": cloud, "vec1": vec1, "vec2": vec2, "pt1": pt1, "angles": angles, "vectors": vectors,
           "x0": np.float64(X0)}
    rows = {k: [] for k in ("fit_param", "eval_none", "eval_x1", "eval_x2", "vec_param", "rot_param", "angle", "angle_xz")}
    for t in range(N_TRIPLES):
        rows["fit_param"].append(Plane3D.fit(triples[t], method="min").param.ravel())
        for key, weight in weights.items():
            rows["eval_" + key].append(Plane3D.fit(triples[t], method="min", weight=weight).eval(cloud))
        rows["vec_param"].append(Plane3D.create_plane_from_vectors_and_point(vec1[t], vec2[t], pt1[t]).param.ravel())
        plane = Plane3D.fit(triples[t], method="min")
        rows["angle"].append(plane.normal_angle_to_vector(vectors[t]))
        rows["angle_xz"].append(plane.normal_angle_to_vector_xz(vectors[t]))
        plane.rotate_around_axis("y", angles[t])
        rows["rot_param"].append(plane.param.ravel())
    for k, v in rows.items():
        out[k] = np.array(v, dtype=np.float64)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes, %d arrays)" % (args.out, os.path.getsize(args.out), len(out)))


if __name__ == "__main__":
    main()
