#!/usr/bin/env python3
"""Generate tests/golden/hull_backproject.npz by running the REFERENCE's own back-projection arithmetic on seeded pixels.

TEST INFRASTRUCTURE ONLY (CPU, no GPU), run where a checkout of the reference exists:

    python tools/gen_golden_hull.py --reference <path to the reference checkout>

What is imported from the reference: src/camera.py (Camera, camera_setup_1, camera_setup_6), src/plane_3d.py (Plane3D) and, through
camera.py, src/utils/utils.py (homogenize).  Their plotting and OpenCV imports (matplotlib, mpl_toolkits, cv2) and bounding_box are
replaced by empty stub modules in this script only; none of them takes part in the arithmetic recorded here.

Per camera (camera1, camera6): 24 seeded pixel positions [2, 24] over the 1920 x 1440 image (float64, as the node's scaled hull
vertices are), pixel_to_ray_vec's d [3, 24] and C [3, 1], pixel_to_ray(world=True / False) for the first four pixels, and for each of
three planes (given as raw a, b, c, d; one with c < 0 so that the constructor's sign flip shows) the normalised parameters,
plane_ray_intersection_vec [3, 24], plane_ray_intersection of the first ray, and both distance functions on 5 seeded points.
Data only -- no reference source text.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OUT = os.path.join(REPO, "tests", "golden", "hull_backproject.npz")
SEED, N_PIX = 20261017, 24
PLANES = np.array([[0.01, -0.02, 1.0, 1.8], [0.05, 0.03, -0.9, -1.6], [-0.2, 0.1, 2.0, 3.1]])


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
    src = os.path.join(args.reference, "src")
    stub("cv2")
    stub("matplotlib", pyplot=stub("matplotlib.pyplot"))
    stub("mpl_toolkits", mplot3d=stub("mpl_toolkits.mplot3d", Axes3D=object))
    stub("bounding_box", BoundingBox=object)
    plane_3d = load_module("plane_3d", os.path.join(src, "plane_3d.py"))
    stub("src", utils=stub("src.utils"))
    load_module("src.utils.utils", os.path.join(src, "utils", "utils.py"))
    camera = load_module("ref_camera", os.path.join(src, "camera.py"))

    rng = np.random.default_rng(SEED)
    out = {"planes_raw": PLANES}
    for name, cam in (("camera1", camera.camera_setup_1()), ("camera6", camera.camera_setup_6())):
        pts = rng.uniform([[0.0], [0.0]], [[1920.0], [1440.0]], size=(2, N_PIX))
        d, C = cam.pixel_to_ray_vec(pts)
        out[name + "_pts"], out[name + "_d"], out[name + "_C"] = pts, d, C
        out[name + "_K_inv"] = cam.K_inv
        for world in (True, False):
            rays = [cam.pixel_to_ray(pts[0, i], pts[1, i], world=world) for i in range(4)]
            out["%s_ray_d_%d" % (name, world)] = np.stack([r[0] for r in rays])
            out["%s_ray_C_%d" % (name, world)] = np.stack([r[1] for r in rays])
        cloud = rng.normal(0.0, 10.0, size=(5, 3))
        out[name + "_cloud"] = cloud
        for k, raw in enumerate(PLANES):
            plane = plane_3d.Plane3D.create_plane_from_list(list(raw))
            out["%s_plane%d_param" % (name, k)] = plane.param
            out["%s_plane%d_hit_vec" % (name, k)] = plane.plane_ray_intersection_vec(d, C)
            out["%s_plane%d_hit_one" % (name, k)] = plane.plane_ray_intersection(d[:, :1], C)
            out["%s_plane%d_dist" % (name, k)] = plane.distance_to_plane(cloud)
            out["%s_plane%d_dist_signed" % (name, k)] = plane.distance_to_plane_signed(cloud)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes, %d arrays)" % (args.out, os.path.getsize(args.out), len(out)))


if __name__ == "__main__":
    main()
