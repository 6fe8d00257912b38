"""The occlusion rule of include/avl_hip.h (struct avl_occlusion, rules 1 - 6) restated in NumPy, and the small seeded scenes the
occlusion tests share.  Nothing here is shared with the kernels: the projection comes from oracle/mapping_oracle.py, the buffer is
filled with np.minimum.at and the cull test is a plain Python loop in double arithmetic (a product, then a sum: two roundings).

MUTANTS names deliberately wrong variants of the rule; tests/test_occlusion_cpu.py asserts that each of them changes the culled set
on some scene, i.e. that the scenes can tell the rule from its likely mis-implementations."""
import math

import numpy as np

from oracle import mapping_oracle as mo

EMPTY = np.uint32(0xFFFFFFFF)
SIZES = [(96, 64), (97, 61)]               # projection images (img_w, img_h); the second leaves partial last cells at s = 8 and s = 7
COUNTS = [1, 63, 257, 3000]
RANGE_MAX = 100.0
DEFAULTS = dict(s=8, R=1, rel=0.05, abs_=0.5)      # MAPPING.OCCLUSION's defaults
MUTANTS = ("depth_from_v0", "radius_ignored", "classmap_pixels", "additive_only", "empty_reads_zero")


# ---------------------------------------------------------------------------------------------------------------- the rule
def depth_buffer(ix, iy, cand, key, img_w, img_h, s):
    """rule 3: uint32 [Hc, Wc], the minimum bit pattern of the valid candidates' float32 keys per cell, EMPTY elsewhere"""
    Wc, Hc = -(-img_w // s), -(-img_h // s)
    key = np.asarray(key, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        valid = cand & np.isfinite(key) & (key > 0)
    depth = np.full((Hc, Wc), EMPTY, dtype=np.uint32)
    np.minimum.at(depth, (iy[valid] // s, ix[valid] // s), key.view(np.uint32)[valid])
    return depth, valid


def visibility(ix, iy, cand, key, img_w, img_h, s, R, rel, abs_, mutant=None, v0=None, src_size=None):
    """rules 1 - 5 for one view -> uint8 [n]: 0 not a candidate, 1 visible, 2 culled.  ix, iy int32 [n] and cand bool [n] are the
    oracle's projection, key float32 [n] the candidates' depth keys (ignored where cand is False).  `mutant` (one of MUTANTS) breaks
    the rule on purpose: depth_from_v0 needs v0 (the velodyne-frame x), classmap_pixels needs src_size = (src_w, src_h)."""
    assert mutant is None or mutant in MUTANTS
    ix, iy, cand = np.asarray(ix, dtype=np.int64), np.asarray(iy, dtype=np.int64), np.asarray(cand, dtype=bool)
    key = np.asarray(key, dtype=np.float32)
    if mutant == "depth_from_v0":
        key = np.asarray(v0, dtype=np.float64).astype(np.float32)
    if mutant == "radius_ignored":
        R = 0
    if mutant == "classmap_pixels":             # cells counted in pixels of the (smaller) class map
        sw, sh = src_size
        ix, iy, img_w, img_h = ix * sw // img_w, iy * sh // img_h, sw, sh
    k = 1.0 if mutant == "additive_only" else 1.0 + float(rel)
    depth, valid = depth_buffer(np.where(cand, ix, 0), np.where(cand, iy, 0), cand, key, img_w, img_h, s)
    Hc, Wc = depth.shape
    state = cand.astype(np.uint8)
    for i in np.nonzero(valid)[0]:
        cx, cy = int(ix[i]) // s, int(iy[i]) // s
        m = depth[max(cy - R, 0):min(cy + R, Hc - 1) + 1, max(cx - R, 0):min(cx + R, Wc - 1) + 1].min()
        md = float(np.array([m], dtype=np.uint32).view(np.float32)[0])
        if mutant == "empty_reads_zero" and (depth[max(cy - R, 0):cy + R + 1, max(cx - R, 0):cx + R + 1] == EMPTY).any():
            md = 0.0
        prod = md * k                           # rule 5: two separately rounded double operations
        if float(key[i]) > prod + float(abs_):
            state[i] = 2
    return state


# ---------------------------------------------------------------------------------------------------------------- projection
def pinhole_P(img_w, img_h, f=60.0, yaw=0.0, pitch=0.06, cam=(0.3, 0.0, 0.0)):
    """P = K [R | t] of a camera at `cam` (velodyne frame) that looks along +x, turned by `yaw` about z and tipped down by `pitch`:
    with a pitch and an offset the depth p2 is not the velodyne-frame x."""
    cy_, sy_ = math.cos(yaw), math.sin(yaw)
    cp, sp = math.cos(pitch), math.sin(pitch)
    fwd = np.array([cy_ * cp, sy_ * cp, -sp])
    left = np.array([-sy_, cy_, 0.0])
    up = np.cross(fwd, left)
    R = np.stack([-left, -up, fwd])                    # camera axes: x right, y down, z forward
    t = -R @ np.asarray(cam, dtype=np.float64).reshape(3, 1)
    K = np.array([[f, 0.0, img_w / 2.0], [0.0, f, img_h / 2.0], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, t], axis=1)


class Projection(object):
    """the oracle's projection of a cloud through P: ix, iy, the candidate mask (rule 1), the float64 depth p2 (rule 2) and v0"""

    def __init__(self, pcd, P, img_w, img_h, range_max=RANGE_MAX, frame_id="velodyne", pose7=None):
        pcd = np.asarray(pcd, dtype=np.float64)
        blank = np.zeros((img_h, img_w, 3), dtype=np.uint8)
        T_vb = mo.velodyne_to_baselink()
        _, _, ixy, mask = mo.project_pcd(pcd, frame_id, blank, pose7, P, range_max, T_vb, return_debug=True)
        self.ix, self.iy, self.cand = ixy[0], ixy[1], mask
        with np.errstate(all="ignore"):
            xv = mo.homogenize(pcd[0:3, :])
            if frame_id != "velodyne":                                     # src/mapping.py:368-371
                xv = np.matmul(np.linalg.inv(np.matmul(mo.transform_from_pose(pose7), T_vb)), xv)
            self.p2 = np.matmul(P, xv)[2]                                  # the divisor of src/mapping.py:375
        self.v0 = xv[0]
        self.img_w, self.img_h = img_w, img_h

    def key32(self):
        with np.errstate(all="ignore"):
            return self.p2.astype(np.float32)

    def states(self, key=None, mutant=None, src_size=None, **par):
        p = dict(DEFAULTS, **par)
        return visibility(self.ix, self.iy, self.cand, self.key32() if key is None else key, self.img_w, self.img_h, p["s"], p["R"], p["rel"],
                          p["abs_"], mutant=mutant, v0=self.v0, src_size=src_size)


# ---------------------------------------------------------------------------------------------------------------- scenes
GROUND_Z = -2.0


def make_cloud(seed, n):
    """float64 [4, n], velodyne frame, camera near the origin 2 m above the ground: a ground plane, a wall patch at x ~ 10 m that covers
    the middle of the image, a post at x ~ 6 m, points at 20 - 30 m behind the wall and beside it.  The n points are the first n of
    one shuffled 3000-point scene, so the small clouds are sparse samples of the large one."""
    rng = np.random.default_rng(seed)
    m = max(n, 3000)
    kinds = rng.choice(5, size=m, p=[0.40, 0.20, 0.08, 0.20, 0.12])
    u = rng.random((3, m))
    x, y, z = np.empty(m), np.empty(m), np.empty(m)
    g = kinds == 0                                                         # ground
    x[g] = 4.0 + 36.0 * u[0, g] ** 2
    y[g] = (u[1, g] * 2 - 1) * 0.85 * x[g]                                 # a little wider than the image
    z[g] = GROUND_Z + 0.02 * u[2, g]
    w = kinds == 1                                                         # wall
    x[w], y[w], z[w] = 10.0 + 0.1 * u[0, w], -3.0 + 6.0 * u[1, w], GROUND_Z + 3.5 * u[2, w]
    p = kinds == 2                                                         # post, nearer than x = 8: off the test grids
    x[p], y[p], z[p] = 6.0 + 0.1 * u[0, p], -0.5 + u[1, p], GROUND_Z + 2.0 * u[2, p]
    b = kinds == 3                                                         # behind the wall
    x[b], y[b], z[b] = 20.0 + 10.0 * u[0, b], -6.0 + 12.0 * u[1, b], GROUND_Z + 4.0 * u[2, b]
    s = kinds == 4                                                         # beside it
    x[s] = 20.0 + 10.0 * u[0, s]
    y[s] = np.where(u[1, s] < 0.5, -1.0, 1.0) * (7.0 + 8.0 * u[2, s])
    z[s] = GROUND_Z + 14.0 * rng.random(int(s.sum()))                     # tall: up to and beyond the top of the image
    inten = 20.0 * rng.random(m)
    return np.ascontiguousarray(np.stack([x, y, z, inten])[:, :n])


def boundary(Hm, Wm, res):
    """map_boundary of an Hm x Wm grid whose x starts 8 m in front of the sensor (the post and the nearest ground are off it) and whose
    y is centred on it"""
    ox, oy = mo.PCD_ORIGIN_OFFSET[0], mo.PCD_ORIGIN_OFFSET[1]
    return [[ox + 8.0, ox + 8.0 + Hm * res], [oy - Wm * res / 2, oy + Wm * res / 2]]


def on_grid(pcd, Hm, Wm, res):
    return mo.cell_indices(np.asarray(pcd, dtype=np.float64), boundary(Hm, Wm, res), res, Hm, Wm)[1]


def scenes():
    """every (id, img_w, img_h, n, cloud, P) of SIZES x COUNTS"""
    out = []
    for k, (w, h) in enumerate(SIZES):
        for n in COUNTS:
            out.append(("%dx%d_n%d" % (w, h, n), w, h, n, make_cloud(100 + k, n), pinhole_P(w, h)))
    return out
