"""The ground plane from the LiDAR cloud that is already on the device: a RANSAC around the reference's plane model.

The reference ships the model half of a plane RANSAC (src/plane_3d.py: ``Plane3D.fit(data, "min")`` and ``Plane3D.eval``) and takes
the plane itself from another package on /estimated_plane (vision_semantic_segmentation_node.py:51, :199-201).  Here one call of the
library (avl_plane_ransac, csrc/seg_plane.hip) fits ``hypotheses`` point triples, scores each against every point with the
reference's weighted cost, selects the one with the most inliers and sums the inliers' moments -- all on the stream, with nothing
coming to the host until ``GroundPlaneResult.host()`` copies 24 words.  There is no CPU path: a missing library raises.

The reference has no RANSAC driver, so the number of hypotheses, the inlier tolerance (0.1, in the cost's unit: metres at x = x0,
more further out under the "x norm" weight), the largest accepted tilt (30 degrees between the normal and +z) and the least-squares
refit are this project's choices, not the reference's.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .plane_3d import Plane3D, default_weight


def sample_triples(n, n_hyp, seed):
    """The point triples of the hypotheses: ``np.random.default_rng(seed).integers(0, n, (n_hyp, 3))`` as int32 [n_hyp, 3] -- stated
    here so that anyone can draw the same triples.  A triple may repeat an index; such a hypothesis is invalid and scores 0."""
    return np.random.default_rng(seed).integers(0, n, (n_hyp, 3)).astype(np.int32)


def plane_from_moments(p0, n, s1, s2, weight=None):
    """The least-squares plane of points given by their moments about p0: n points, s1 = sum(delta) [3], s2 = sum(delta delta^T) as
    (xx, xy, xz, yy, yz, zz), delta = p - p0.  The normal is the eigenvector of the smallest eigenvalue of s2 / n - mean mean^T
    (np.linalg.eigh), the plane passes through the centroid p0 + mean; Plane3D's constructor fixes the sign (c >= 0)."""
    p0, s1, s2 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (p0, s1, s2))
    n = float(n)
    if n < 3:
        raise ValueError("plane_from_moments needs at least three points, got n = %g" % n)
    mean = s1 / n
    xx, xy, xz, yy, yz, zz = s2 / n
    cov = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) - np.outer(mean, mean)
    normal = np.linalg.eigh(cov)[1][:, 0]
    centre = p0 + mean
    d = -(normal[0] * centre[0] + normal[1] * centre[1] + normal[2] * centre[2])
    return Plane3D(normal[0], normal[1], normal[2], d, weight=weight)


def plane_coefficients(plane):
    """(a, b, c, d) of a Plane3D, of a GroundPlaneResult that has been to the host, or of four numbers -> float64 [4]."""
    plane = getattr(plane, "plane", plane)                          # GroundPlaneResult.plane
    if plane is None:
        raise ValueError("no plane: None, or a GroundPlaneResult without one (host() not called, or no hypothesis had an inlier)")
    if hasattr(plane, "a"):
        return np.array([plane.a, plane.b, plane.c, plane.d], dtype=np.float64)
    p = np.asarray(plane, dtype=np.float64).reshape(-1)
    if p.size != 4:
        raise ValueError("a plane is a Plane3D or four numbers (a, b, c, d), got %d values" % p.size)
    return p


def plane_to_frame(plane, T):
    """The plane a x + b y + c z + d = 0 of one frame, in the frame that the 4 x 4 transform ``T`` takes into it: a point X of that
    other frame lies on the plane when (a, b, c, d) . (T X) = 0, so the result is ``np.array([a, b, c, d]) @ T``, one float64
    matmul, not normalised.  ``T`` None gives the plane itself.  With the velodyne-frame ground plane and T = origin -> velodyne
    (SemanticMapping._origin_to_velodyne) this is the plane in the world frame, the frame of a world-frame grid."""
    p = plane_coefficients(plane)
    if T is None:
        return p
    return np.matmul(p, np.asarray(T, dtype=np.float64).reshape(4, 4))


def plane_tilt_deg(plane):
    """The angle in degrees between the plane's normal and the z axis, whichever way the normal points; NaN for a zero normal."""
    a, b, c, _ = plane_coefficients(plane)
    with np.errstate(all="ignore"):
        return float(np.degrees(np.arccos(abs(c) / np.sqrt(a * a + b * b + c * c))))


class GroundPlaneWorkspace(object):
    """Every device buffer one estimate needs, for clouds of up to n_max points and n_hyp hypotheses.  A result made with a
    workspace refers to the workspace's tensors: the next estimate with the same workspace overwrites them."""

    def __init__(self, n_max, n_hyp, device):
        n_max, n_hyp = int(n_max), int(n_hyp)
        need = int(_lib.lib().avl_plane_scratch_bytes(n_max, n_hyp))
        if need <= 0:
            raise ValueError("no ground-plane workspace for %d points and %d hypotheses (at least 3 points, 1 .. %d hypotheses)"
                             % (n_max, n_hyp, _lib.AVL_PLANE_MAX_HYP))
        self.n_max, self.n_hyp, self.device = n_max, n_hyp, torch.device(device)
        self.scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.planes = torch.empty((n_hyp, 4), dtype=torch.float64, device=self.device)
        self.counts = torch.empty(n_hyp, dtype=torch.int32, device=self.device)
        self.result = torch.empty(_lib.AVL_PLANE_RESULT_WORDS, dtype=torch.float64, device=self.device)

    def fits(self, n, n_hyp, device):
        return n <= self.n_max and n_hyp == self.n_hyp and torch.device(device) == self.device


class GroundPlaneResult(object):
    """``planes`` float64 [H, 4] and ``counts`` int32 [H] stay on the device.  ``host()`` copies the 24 result words once (this
    synchronises) and fills ``plane`` (a Plane3D, or None when no hypothesis has an inlier), ``hypothesis`` (its index, -1 for
    none), ``inliers``, ``used`` (points that took part), ``valid`` (hypotheses that did) and ``moments`` (p0, n, s1, s2 of the
    inliers: what plane_from_moments takes)."""

    def __init__(self, planes, counts, result, refine, weight, keep, stream):
        self.planes, self.counts, self._result, self._refine, self._weight, self._keep = planes, counts, result, refine, weight, keep
        self._stream = stream
        self.plane = self.hypothesis = self.inliers = self.used = self.valid = self.moments = self.words = None

    def host(self):
        if self.words is None:
            with torch.cuda.stream(self._stream):                     # the copy queues behind the kernels, on their stream
                words = self._result.cpu().numpy()
            ints = words.view(np.int64)
            self.words = words
            self.hypothesis, self.inliers, self.used, self.valid = (int(v) for v in ints[:4])
            self.moments = {"p0": words[8:11].copy(), "n": float(words[11]), "s1": words[12:15].copy(), "s2": words[15:21].copy()}
            if self.hypothesis >= 0:
                if self._refine and self.moments["n"] >= 3:
                    self.plane = plane_from_moments(weight=self._weight, **self.moments)
                else:
                    self.plane = Plane3D(words[4], words[5], words[6], words[7], weight=self._weight)
            self._keep = None
        return self


def _weight_args(weight):
    method = weight['method']
    if method == "none":
        return _lib.AVL_PLANE_W_NONE, 0.0, 1
    if method != "x norm":
        raise NotImplementedError("weight method %r" % (method,))              # plane_3d.py:78-79
    norm = weight['param']['norm']
    if norm not in (1, 2):
        raise NotImplementedError("x norm %r" % (norm,))                        # plane_3d.py:71-72
    return _lib.AVL_PLANE_W_XNORM, float(weight['param']['x0']), int(norm)


def estimate_ground_plane_device(points, *, triples=None, hypotheses=256, seed=0, tolerance=0.1, weight=None, max_tilt_deg=30.0,
                                 roi=None, T=None, refine=True, workspace=None, stream=None, device=None):
    """points: ndarray or tensor, [4, N] or [N, 4] (x, y, z, intensity), float32 or float64 -> GroundPlaneResult; asynchronous.

    triples int32 [H, 3] point indices (ndarray or tensor), default sample_triples(N, hypotheses, seed).  weight: a Plane3D weight
    dict, default the reference's {'method': "x norm", 'param': {'x0': 0.0, 'norm': 1}}.  A hypothesis whose normal is more than
    max_tilt_deg from +z is dropped.  roi = (xmin, xmax, ymin, ymax, zmin, zmax) keeps only the points inside; T (4x4) maps the
    points into the frame the plane is wanted in before anything else (roi and weight apply there).  Points with a NaN or infinite
    coordinate are left out.  refine: the returned plane is the least-squares plane of the winner's inliers (plane_from_moments)
    rather than the winning hypothesis.  stream: a torch.cuda.Stream or a raw HIP stream handle, default torch's current stream;
    uploads of host data, the kernels and ``host()``'s copy are all ordered on it (device tensors the caller hands in must already be
    ready on it; ``planes`` / ``counts`` are to be read on it).  tolerance, max_tilt_deg, hypotheses and refine are this project's choices: the reference
    has no RANSAC driver to take them from."""
    weight = default_weight() if weight is None else weight
    method, x0, norm = _weight_args(weight)
    if device is None:
        device = points.device if isinstance(points, torch.Tensor) and points.is_cuda else \
            (workspace.device if workspace is not None else torch.device("cuda", torch.cuda.current_device()))
    device = torch.device(device)
    if stream is None:
        stream = torch.cuda.current_stream(device)
    elif not isinstance(stream, torch.cuda.Stream):
        stream = torch.cuda.ExternalStream(int(stream), device=device)
    if roi is not None and len(roi) == 0:
        roi = None
    dbl = lambda a, k: None if a is None else (C.c_double * k)(*np.asarray(a, dtype=np.float64).reshape(k).tolist())  # noqa: E731
    min_c = float(np.cos(np.deg2rad(float(max_tilt_deg))))
    with torch.cuda.stream(stream):                 # the uploads, the kernels and later the result's copy all queue on `stream`
        pts, n, dtype, point_stride, comp_stride = _lib.points_view(points, device)
        if triples is None:
            triples = sample_triples(n, int(hypotheses), seed)
        if not isinstance(triples, torch.Tensor):
            triples = torch.from_numpy(np.ascontiguousarray(triples, dtype=np.int32))
        if triples.dim() != 2 or triples.shape[1] != 3 or triples.dtype != torch.int32:
            raise ValueError("triples must be int32 [H, 3]")
        n_hyp = int(triples.shape[0])
        if workspace is None or not workspace.fits(n, n_hyp, device):
            workspace = GroundPlaneWorkspace(n, n_hyp, device)
        tri = triples.to(device).contiguous()
        rc = _lib.lib().avl_plane_ransac(C.c_void_p(pts.data_ptr()), n, dtype, point_stride, comp_stride, dbl(T, 16), dbl(roi, 6),
                                         C.c_void_p(tri.data_ptr()), n_hyp, method, x0, norm, float(tolerance), min_c,
                                         C.c_void_p(workspace.planes.data_ptr()), C.c_void_p(workspace.counts.data_ptr()),
                                         C.c_void_p(workspace.result.data_ptr()), C.c_void_p(workspace.scratch.data_ptr()),
                                         C.c_void_p(stream.cuda_stream))
    _lib.check(rc, "avl_plane_ransac")
    return GroundPlaneResult(workspace.planes, workspace.counts, workspace.result, bool(refine), weight, (pts, tri, workspace), stream)
