"""The points-map mode without an external reducer: the site's prior point map on the device, tiled once, cropped per frame.

The reference's SemanticMapping subscribes to /reduced_map (src/mapping.py:61-62): a node outside the package crops the point map of
the whole site around the vehicle and republishes the crop, which pcd_callback unpacks (:172-183).  Here the map is loaded once
(``PointsMapIndex``), sorted into ground tiles, and every frame ``gather`` copies the tiles of one rectangle into a contiguous float32
[M, 4] cloud on the device -- what the frame entry points take as any other cloud.  The rectangle (``window``) is the bounding box of
the set of points that CAN vote in the frame, so the grid ends bit-equal to a frame on the whole map: votes are an idempotent OR per
cell and the apply pass adds in a fixed order, so neither the order nor the multiplicity of the voters matters.

The drop rule, the tile rule and the layout of the sorted cloud are stated once, in include/avl_hip.h.  The keys come from a HIP
kernel (avl_points_map_keys) and the per-frame copy is one (avl_points_map_gather); bounds, the stable sort, the histogram and its
prefix sum are torch's and run once, at load.  The window is host float64 and needs no GPU."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .utils.utils_ros import get_transform_from_pose

MAX_TILES = 1 << 24
MAX_POINTS = 1 << 31


def as_points(points):
    """A cloud [N, 4] or [4, N] (x, y, z, intensity; [4, N], the reference's layout, wins for a 4 x 4 input), NumPy or torch, float32
    or float64 -> a float32 tensor [N, 4] on the input's device.  ValueError for another shape and for N >= 2^31 (before any copy)."""
    t = points if isinstance(points, torch.Tensor) else None
    shape = tuple(points.shape) if hasattr(points, "shape") else tuple(np.shape(points))
    if len(shape) != 2 or 4 not in shape:
        raise ValueError("the points map must be [N, 4] or [4, N], got %s" % (shape,))
    soa = shape[0] == 4
    n = shape[1] if soa else shape[0]
    if n >= MAX_POINTS:
        raise ValueError("the points map has %d points (fewer than 2^31)" % n)
    if t is None:
        t = torch.from_numpy(np.asarray(points))
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError("the points map must be float32 or float64, got %s" % (t.dtype,))
    if soa:
        t = t.t()
    return t.to(torch.float32).contiguous()


def load_points(points_or_path):
    """``as_points`` of an array, or of the array a .npy file holds (nothing else is parsed)."""
    if isinstance(points_or_path, (str, bytes)) or hasattr(points_or_path, "__fspath__"):
        path = points_or_path
        if not str(path).endswith(".npy"):
            raise ValueError("a points map file is a .npy array [N, 4] or [4, N], got %r" % (path,))
        return as_points(np.load(path, allow_pickle=False))
    return as_points(points_or_path)


def keep_mask(pts):
    """The drop rule on a float32 tensor [N, 4] -> bool [N], True = kept: no field is NaN, x and y are finite."""
    return ~(torch.isnan(pts).any(dim=1) | torch.isinf(pts[:, 0]) | torch.isinf(pts[:, 1]))


def _check_tile_m(tile_m):
    if isinstance(tile_m, bool) or not isinstance(tile_m, (int, float, np.integer, np.floating)) or not (float(tile_m) > 0.0) \
            or math.isinf(float(tile_m)):
        raise ValueError("TILE_M = %r (a finite number > 0)" % (tile_m,))
    return float(tile_m)


def tile_grid(pts, tile_m):
    """The tile rule's constants for a float32 tensor [N, 4] -> (ox, oy, rows, cols, kept): the origin (float64), the tile counts and
    the number of points the drop rule keeps; (0.0, 0.0, 0, 0, 0) when it keeps none.  ValueError when rows * cols > 2^24."""
    tile_m = _check_tile_m(tile_m)
    keep = keep_mask(pts)
    kept = int(keep.sum().item())
    if kept == 0:
        return 0.0, 0.0, 0, 0, 0
    xy = pts[:, :2][keep]
    lo, hi = xy.min(dim=0).values.cpu().tolist(), xy.max(dim=0).values.cpu().tolist()    # float32 -> float: exact
    ox, oy = (math.floor(v / tile_m) * tile_m for v in lo)
    rows = int(math.floor((hi[0] - ox) / tile_m)) + 1
    cols = int(math.floor((hi[1] - oy) / tile_m)) + 1
    if rows * cols > MAX_TILES:
        raise ValueError("the points map spans %d x %d tiles of %g m (at most 2^24): raise MAPPING.POINTS_MAP.TILE_M" % (rows, cols, tile_m))
    return ox, oy, rows, cols, kept


class PointsMapIndex(object):
    """The prior point map on ``device``, sorted by ground tile (include/avl_hip.h: the drop rule, the tile rule).

    ``points``   float32 [N', 4] on the device: the kept points, sorted by tile key, input order inside a tile
    ``offsets``  int32 [rows * cols + 1] on the device, ``offsets_host`` the same as a NumPy array: tile ``key = ix * cols + iy`` is
                 ``points[offsets[key]:offsets[key + 1]]``
    ``ox, oy, tile_m, rows, cols``  the tile rule's constants; ``dropped`` the number of input points the drop rule removed
    ``keys``     None, or with ``keep_keys`` the int32 [N] keys in input order, -1 = dropped (4 bytes per input point that nothing
                 but a test reads after the build)"""

    def __init__(self, points, tile_m=10.0, device=None, keep_keys=False):
        self.tile_m = _check_tile_m(tile_m)
        pts = load_points(points)
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("PointsMapIndex needs a GPU (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        pts = pts.to(self.device)
        n = int(pts.shape[0])
        self.ox, self.oy, self.rows, self.cols, kept = tile_grid(pts, self.tile_m)
        self.dropped = n - kept
        tiles = self.rows * self.cols
        keys = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib().avl_points_map_keys(C.c_void_p(pts.data_ptr()), n, self.ox, self.oy, self.tile_m, self.rows, self.cols,
                                                      C.c_void_p(keys.data_ptr()), s), "avl_points_map_keys")
        self.keys = keys if keep_keys else None
        sorted_keys, order = torch.sort(keys, stable=True)         # the dropped points, key -1, come first
        if int((keys < 0).sum().item()) != self.dropped:
            raise RuntimeError("avl_points_map_keys dropped %d points, the drop rule %d" % (int((keys < 0).sum().item()), self.dropped))
        self.points = pts.index_select(0, order[self.dropped:]).contiguous()
        counts = torch.bincount(sorted_keys[self.dropped:].to(torch.int64), minlength=tiles) if kept else torch.zeros(tiles, dtype=torch.int64,
                                                                                                                     device=self.device)
        offsets = torch.zeros(tiles + 1, dtype=torch.int64, device=self.device)
        offsets[1:] = torch.cumsum(counts, dim=0)
        self.offsets = offsets.to(torch.int32)
        self.offsets_host = np.ascontiguousarray(self.offsets.cpu().numpy())
        assert int(self.offsets_host[-1]) == kept == int(self.points.shape[0])

    def __len__(self):
        return int(self.points.shape[0])

    def device_bytes(self):
        """Bytes of HBM the index holds (the sorted cloud and the offsets; the keys only when they were kept)."""
        return sum(int(t.numel()) * t.element_size() for t in (self.points, self.keys, self.offsets) if t is not None)


def frustum_vertices(camera, image_size, range_max):
    """-> float64 [3, 9] in the velodyne frame: the camera centre c = -R^T t and, for each corner pixel (-1, -1), (W, -1), (-1, H),
    (W, H) of ``image_size`` = (H, W), the two points where the line c + s R^T K^-1 (u, v, 1)^T meets the planes x = 0 and
    x = range_max.  A point votes only if 0 < x < range_max and its pixel, truncated towards zero, lies in the image
    (src/mapping.py:375-383), i.e. -1 < u < W and -1 < v < H, whatever the sign of its homogeneous w: it lies on a line through c whose
    direction is inside the corner directions.  With the directions scaled to x = 1 those form a convex quadrilateral, and the
    voters the two truncated pyramids the nine points span.  ValueError when the four directions' x components do not have one sign:
    the camera looks sideways past the range plane and the set is unbounded."""
    H, W = float(image_size[0]), float(image_size[1])
    R, t = np.asarray(camera.R, dtype=np.float64), np.asarray(camera.t, dtype=np.float64).reshape(3, 1)
    K_inv = np.linalg.inv(np.asarray(camera.K, dtype=np.float64))
    c = np.matmul(-R.T, t)
    corners = np.array([[-1.0, W, -1.0, W], [-1.0, -1.0, H, H], [1.0, 1.0, 1.0, 1.0]])
    d = np.matmul(R.T, np.matmul(K_inv, corners))
    if not ((d[0] > 0).all() or (d[0] < 0).all()):
        raise ValueError("the camera's corner rays do not all cross the planes x = 0 and x = RANGE_MAX of the velodyne frame (x components "
                         "%s): its voters are unbounded.  Set MAPPING.POINTS_MAP.RADIUS_M for a square crop instead" % (d[0].tolist(),))
    out = [c]
    for x in (0.0, float(range_max)):
        out.append(c + d * ((x - c[0, 0]) / d[0]))
    return np.hstack(out)


def velodyne_to_origin(pose):
    """T_base_to_origin T_velodyne_to_baselink (the inverse of what src/mapping.py:368-369 builds), host float64 4 x 4."""
    from .mapping import velodyne_to_baselink
    return np.matmul(get_transform_from_pose(pose), velodyne_to_baselink())


def window_box(pose, cameras, image_size, range_max, radius_m=0.0, margin_m=0.0):
    """-> (xmin, xmax, ymin, ymax) in the world frame.  radius_m == 0: the bounding box of every camera's frustum_vertices taken to
    the world; radius_m > 0: the square of that half-side around the velodyne origin (what an external reducer delivers).  Grown by
    margin_m on every side."""
    T = velodyne_to_origin(pose)
    if radius_m > 0.0:
        xy = T[:2, 3:4]
        lo, hi = xy[:, 0] - float(radius_m), xy[:, 0] + float(radius_m)
    else:
        cameras = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras]
        if not cameras:
            raise ValueError("the window needs at least one camera")
        v = np.hstack([frustum_vertices(cam, image_size, range_max) for cam in cameras])
        w = np.matmul(T, np.vstack([v, np.ones((1, v.shape[1]))]))[:2]
        lo, hi = w.min(axis=1), w.max(axis=1)
    m = float(margin_m)
    return float(lo[0]) - m, float(hi[0]) + m, float(lo[1]) - m, float(hi[1]) + m


def window(index, pose, cameras, image_size, range_max, radius_m=0.0, margin_m=0.0):
    """-> the tile rectangle (r0, r1, c0, c1) of ``index`` (anything with ox, oy, tile_m, rows, cols) that covers window_box(...):
    both ends included, clipped to the index, empty (r0 > r1 or c0 > c1) when the box misses it.  The box's edges go through the
    tile rule's own expression, which is monotone: a kept point inside the box has its tile inside the rectangle."""
    xmin, xmax, ymin, ymax = window_box(pose, cameras, image_size, range_max, radius_m, margin_m)

    def tile(v, origin):
        return math.floor((v - origin) / index.tile_m)
    return clip_rect((tile(xmin, index.ox), tile(xmax, index.ox), tile(ymin, index.oy), tile(ymax, index.oy)), index.rows, index.cols)


def clip_rect(rect, rows, cols):
    """A tile rectangle (r0, r1, c0, c1), both ends included, clipped to rows x cols tiles; r0 > r1 or c0 > c1 when nothing is left."""
    r0, r1, c0, c1 = rect
    return int(max(r0, 0)), int(min(r1, rows - 1)), int(max(c0, 0)), int(min(c1, cols - 1))


def window_count(offsets_host, rows, cols, rect):
    """avl_points_map_window -> (M, non-empty runs) of the rectangle, from the host copy of the offsets (no GPU)."""
    m, runs = C.c_int64(0), C.c_int32(0)
    r0, r1, c0, c1 = (int(v) for v in rect)
    rc = _lib.lib().avl_points_map_window(offsets_host.ctypes.data_as(C.c_void_p), int(rows), int(cols), r0, r1, c0, c1, C.byref(m), C.byref(runs))
    _lib.check(rc, "avl_points_map_window")
    return int(m.value), int(runs.value)


def gather(index, rect, dst, stream=None):
    """avl_points_map_gather: the rectangle's points to ``dst`` (float32 CUDA tensor [capacity, 4], contiguous), on ``stream`` (a raw
    stream handle; None = torch's current one).  Nothing is allocated, copied from the host or waited for."""
    r0, r1, c0, c1 = (int(v) for v in rect)
    assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.dim() == 2 and dst.shape[1] == 4 and dst.device == index.device
    s = torch.cuda.current_stream(index.device).cuda_stream if stream is None else stream
    with torch.cuda.device(index.device):
        rc = _lib.lib().avl_points_map_gather(C.c_void_p(index.points.data_ptr()), C.c_void_p(index.offsets.data_ptr()),
                                              index.offsets_host.ctypes.data_as(C.c_void_p), index.rows, index.cols, r0, r1, c0, c1,
                                              C.c_void_p(dst.data_ptr()), int(dst.shape[0]), C.c_void_p(s))
    _lib.check(rc, "avl_points_map_gather")
