"""NumPy restatement of the ground-plane RANSAC (csrc/seg_plane.hip, steps 1 to 5 of include/avl_hip.h) that follows the reference's
Plane3D (src/plane_3d.py) line by line in float64, the synthetic scene the tests use, and the list of every case the GPU tests run --
tests/test_plane_cpu.py asserts on the CPU that in each of them no (hypothesis, point) cost lies within 1e-10 of the tolerance, so a
last-bit difference cannot flip an inlier.  NumPy only: nothing here imports the package under test."""
import functools

import numpy as np

TOLERANCE = 0.1
MIN_C = float(np.cos(np.deg2rad(30.0)))
MARGIN = 1e-10
WEIGHTS = [("none", 1), ("x norm", 1), ("x norm", 2)]           # (method, norm); x0 below
X0 = 0.0
SHAPES = [(3, 1), (63, 8), (64, 8), (65, 65), (1025, 64), (4097, 64), (20000, 256)]


def scene(rng, n, tilt=(0.03, -0.02), height=1.9, noise=0.03, outlier=0.35):
    """A tilted ground under a LiDAR `height` above it with structure above and below: float32 [n, 4] (x, y, z, intensity)."""
    x = rng.uniform(-10.0, 80.0, n)
    y = rng.uniform(-30.0, 30.0, n)
    z = -height + tilt[0] * x + tilt[1] * y + rng.normal(0.0, noise, n)
    k = int(outlier * n)
    z[rng.permutation(n)[:k]] = rng.uniform(-1.5, 6.0, k)
    return np.stack([x, y, z, rng.uniform(0.0, 30.0, n)], axis=1).astype(np.float32)


def sample_triples(n, n_hyp, seed):
    """The documented draw of ground_plane.sample_triples."""
    return np.random.default_rng(seed).integers(0, n, (n_hyp, 3)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the reference's Plane3D, restated
def fit_min(data):
    """plane_3d.py:47-51 then the constructor (:20-25) with normalize (:98-107) -> (a, b, c, d) as Python floats, or None where the
    reference gives up (:53-54) or leaves an all-zero normal as it is (:100-102)."""
    if not (len(data) == 3 and not np.all(data[0, :] - data[1, :] == 0)):
        return None
    a = (data[0, 1] - data[1, 1]) * (data[2, 2] - data[1, 2]) - (data[2, 1] - data[1, 1]) * (data[0, 2] - data[1, 2])
    b = (data[0, 2] - data[1, 2]) * (data[2, 0] - data[1, 0]) - (data[2, 2] - data[1, 2]) * (data[0, 0] - data[1, 0])
    c = (data[0, 0] - data[1, 0]) * (data[2, 1] - data[1, 1]) - (data[2, 0] - data[1, 0]) * (data[0, 1] - data[1, 1])
    d = -a * data[1, 0] - b * data[1, 1] - c * data[1, 2]
    a, b, c, d = float(a), float(b), float(c), float(d)
    s = np.sqrt(a**2 + b**2 + c**2)
    if s == 0 or not np.isfinite(s):
        return None
    if c < 0:
        s = -1 * s
    return a / s, b / s, c / s, d / s


def x_weight(data, method, x0, norm):
    """plane_3d.py:66-74 -> the weights [n] (ones for "none")."""
    if method == "none":
        return np.ones(data.shape[0])
    if norm == 1:
        x_norm = np.abs(data[:, 0] - x0)
    else:
        x_norm = (data[:, 0] - x0)**2
    x_distance_recip = 1 / (x_norm + 1)
    return x_distance_recip / np.max(x_distance_recip)


def plane_cost(plane, data, weight, method):
    """plane_3d.py:82-88 and :75 / :77."""
    a, b, c, d = plane
    param = np.array([[a, b, c, d]]).T
    length = np.sqrt(a**2 + b**2 + c**2)
    distance = np.abs(np.matmul(data, param[0:3, :]) + d).reshape([-1]) / length
    return distance if method == "none" else distance * weight


class Restated(object):
    pass


def ransac(xyz, triples, method="x norm", x0=X0, norm=1, tolerance=TOLERANCE, min_c=MIN_C, roi=None):
    """Steps 1 to 5 on xyz float64 [n, 3] in the fitted frame.  The cloud is filtered first (finite, inside the roi) and everything
    runs on the filtered cloud; a triple that names a point outside [0, n) or a filtered-out one is invalid."""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = xyz.shape[0]
    used = np.all(np.isfinite(xyz), axis=1)
    if roi is not None:
        for k in range(3):
            with np.errstate(invalid="ignore"):
                used &= (xyz[:, k] >= roi[2 * k]) & (xyz[:, k] <= roi[2 * k + 1])
    data = xyz[used]
    new_index = np.full(n, -1, dtype=np.int64)
    new_index[used] = np.arange(data.shape[0])
    weight = x_weight(data, method, x0, norm) if data.shape[0] else np.ones(0)
    H = len(triples)
    r = Restated()
    r.used, r.planes, r.counts, r.margin = int(data.shape[0]), np.zeros((H, 4)), np.zeros(H, dtype=np.int64), np.full(H, np.inf)
    costs = {}
    for h, tri in enumerate(np.asarray(triples, dtype=np.int64)):
        if np.any(tri < 0) or np.any(tri >= n) or np.any(new_index[tri] < 0):
            continue
        plane = fit_min(data[new_index[tri]])
        if plane is None or plane[2] < min_c:
            continue
        cost = plane_cost(plane, data, weight, method)
        r.planes[h] = plane
        r.counts[h] = int(np.sum(cost < tolerance))
        r.margin[h] = np.min(np.abs(cost - tolerance))
        costs[h] = cost
    r.valid = len(costs)
    r.best = int(np.argmax(r.counts)) if r.counts.max() > 0 else -1          # argmax: the first of equal counts
    r.inliers = int(r.counts[r.best]) if r.best >= 0 else 0
    r.p0, r.n, r.s1, r.s2, r.abs1, r.abs2, r.refined = np.zeros(3), 0, np.zeros(3), np.zeros(6), np.zeros(3), np.zeros(6), None
    if r.best >= 0:
        r.p0 = data[new_index[triples[r.best][0]]]
        delta = data[costs[r.best] < tolerance] - r.p0
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        terms2 = np.stack([delta[:, i] * delta[:, j] for i, j in pairs], axis=1)
        r.n, r.s1, r.s2 = delta.shape[0], delta.sum(axis=0), terms2.sum(axis=0)
        r.abs1, r.abs2 = np.abs(delta).sum(axis=0), np.abs(terms2).sum(axis=0)
        if r.n >= 3:
            r.refined, r.gap, r.centre = refit(r.p0, r.n, r.s1, r.s2)
    return r


def refit(p0, n, s1, s2):
    """Least-squares plane from the moments about p0 -> ((a, b, c, d) with c >= 0, eigen-gap of the two smallest eigenvalues, centroid)."""
    mean = s1 / n
    xx, xy, xz, yy, yz, zz = s2 / n
    cov = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) - np.outer(mean, mean)
    lam, vec = np.linalg.eigh(cov)
    normal = vec[:, 0]
    centre = p0 + mean
    d = -(normal[0] * centre[0] + normal[1] * centre[1] + normal[2] * centre[2])
    s = np.sqrt(normal[0]**2 + normal[1]**2 + normal[2]**2)
    if normal[2] < 0:
        s = -s
    return np.array([normal[0] / s, normal[1] / s, normal[2] / s, d / s]), float(lam[1] - lam[0]), centre


def covariance_bound(r):
    """The largest change (Frobenius norm) of refit's covariance when every moment moves by the bound the GPU test allows it,
    n 2^-53 sum|term|: d(S2 / n) = 2^-53 sum|dd|, d(mean) = 2^-53 sum|d|, d(mean mean^T)_ij <= |mean_i| dmean_j + |mean_j| dmean_i."""
    u = 2.0**-53
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    mean, dmean = np.abs(r.s1 / r.n), u * r.abs1
    full = np.zeros((3, 3))
    for k, (i, j) in enumerate(pairs):
        full[i, j] = full[j, i] = u * r.abs2[k] + mean[i] * dmean[j] + mean[j] * dmean[i] + dmean[i] * dmean[j]
    return float(np.linalg.norm(full))


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def _f64_cloud(cloud32, seed):
    """float64 values that no float32 holds: the float32 scene plus a seeded sub-float32 offset."""
    rng = np.random.default_rng(seed)
    return cloud32.astype(np.float64) + rng.uniform(-1e-7, 1e-7, cloud32.shape)


# seeds: the first of 0, 1, 2, ... for which the case's margin condition holds (seed 0 everywhere; test_plane_cpu.py asserts it)
SHAPE_SEED = {(3, 1): 0, (63, 8): 0, (64, 8): 0, (65, 65): 0, (1025, 64): 0, (4097, 64): 0, (20000, 256): 0}


@functools.lru_cache(maxsize=None)
def shape_cloud(n, n_hyp, dtype):
    seed = SHAPE_SEED[(n, n_hyp)]
    cloud = scene(np.random.default_rng(1000 * seed + n), n)
    if dtype == "f64":
        cloud = _f64_cloud(cloud, seed)
    triples = np.array([[0, 1, 2]], dtype=np.int32) if n == 3 else sample_triples(n, n_hyp, seed)
    return cloud, triples


@functools.lru_cache(maxsize=None)
def shape_case(n, n_hyp, dtype, method, norm):
    cloud, triples = shape_cloud(n, n_hyp, dtype)
    return ransac(cloud[:, :3], triples, method=method, norm=norm)


@functools.lru_cache(maxsize=None)
def reject_case():
    """Triples the fit must refuse, between ordinary ones: a repeated index in each position, an index equal to n, three collinear
    points, a triple naming a NaN point, a plane steeper than min_c."""
    n = 300
    cloud = scene(np.random.default_rng(77), n).astype(np.float64)
    cloud[10, :3], cloud[11, :3], cloud[12, :3] = (1.0, 2.0, -2.0), (2.0, 4.0, -2.0), (4.0, 8.0, -2.0)         # collinear, exactly
    cloud[20, :3], cloud[21, :3], cloud[22, :3] = (0.0, 0.0, -2.0), (1.0, 0.0, 0.0), (0.0, 1.0, -2.0)          # 63 degrees of tilt
    cloud[30, 1] = np.nan
    good = sample_triples(n, 12, 5)
    good = good[[i for i in range(len(good)) if not ({10, 11, 12, 20, 21, 22, 30} & set(good[i].tolist()))]]
    bad = np.array([[5, 5, 9], [5, 9, 5], [9, 5, 5], [1, 2, n], [n, 1, 2], [1, -1, 2], [10, 11, 12], [12, 10, 11], [3, 30, 4], [30, 3, 4],
                    [20, 21, 22]], dtype=np.int32)
    triples = np.concatenate([good[:4], bad, good[4:]]).astype(np.int32)
    bad_rows = np.arange(4, 4 + len(bad))
    return cloud, triples, bad_rows, ransac(cloud[:, :3], triples, method="x norm", norm=1)


ROI = (0.0, 60.0, -20.0, 20.0, -3.0, 1.0)


@functools.lru_cache(maxsize=None)
def dirty_case(with_roi):
    """5 % of the points carry a NaN or an infinity in one coordinate; optionally a roi on top."""
    n, n_hyp = 2500, 48
    rng = np.random.default_rng(4242)
    cloud = scene(rng, n)
    rows = rng.permutation(n)[:n // 20]
    cloud[rows, rng.integers(0, 3, rows.size)] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), rows.size)
    triples = sample_triples(n, n_hyp, 9)
    return cloud, triples, ransac(cloud[:, :3], triples, method="x norm", norm=2, roi=ROI if with_roi else None)


@functools.lru_cache(maxsize=None)
def world_case():
    """A velodyne scene moved into a world frame by T^-1; the estimate gets the world cloud and T."""
    n, n_hyp = 3000, 64
    rng = np.random.default_rng(515)
    velo = scene(rng, n).astype(np.float64)
    yaw, pitch = 0.7, 0.05
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
    Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1.0, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry, (-1369.05, -562.85, 3.2)
    world = velo.copy()
    world[:, :3] = (np.linalg.inv(T) @ np.concatenate([velo[:, :3], np.ones((n, 1))], axis=1).T).T[:, :3]
    back = (T @ np.concatenate([world[:, :3], np.ones((n, 1))], axis=1).T).T[:, :3]          # T p: what the kernel fits
    triples = sample_triples(n, n_hyp, 3)
    return world, T, triples, ransac(back, triples, method="x norm", norm=1)


MOMENT_SHAPES = [(1025, 64), (4097, 64)]


@functools.lru_cache(maxsize=None)
def node_case():
    """The cloud of the node test and the restatement of what the node's defaults ask for (256 hypotheses, seed 0, x norm 1)."""
    n = 6000
    cloud = scene(np.random.default_rng(2026), n)
    return cloud, ransac(cloud[:, :3].astype(np.float64), sample_triples(n, 256, 0), method="x norm", norm=1)


def all_cases():
    """(name, restatement) of every scene, seed and shape a GPU test runs."""
    for n, n_hyp in SHAPES:
        for dtype in ("f32", "f64"):
            for method, norm in WEIGHTS:
                yield "shape %d x %d %s %s %d" % (n, n_hyp, dtype, method, norm), shape_case(n, n_hyp, dtype, method, norm)
    yield "rejects", reject_case()[3]
    yield "dirty", dirty_case(False)[2]
    yield "dirty roi", dirty_case(True)[2]
    yield "world", world_case()[3]
    yield "node", node_case()[1]
