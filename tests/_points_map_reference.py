"""NumPy float64 restatement of the points map's rules (include/avl_hip.h: the drop rule, the tile rule, the sorted cloud, the
rectangle's runs) and of the window (points_map.py), written from the rules and not from the package's code, plus the clouds the
CPU and GPU tests share.  Everything here is host code; nothing imports the package."""
import math

import numpy as np

RANGE_MAX = 12.0            # the GPU frame tests' PCD.RANGE_MAX: the frustum's box is then smaller than the 32 m x 24 m index


# ---------------------------------------------------------------------------------------------------------------- the index
def as_aos32(points):
    a = np.asarray(points)
    if a.shape[0] == 4:
        a = a.T
    return np.ascontiguousarray(a, dtype=np.float32)


def kept(p):
    """the drop rule: True = kept"""
    return ~(np.isnan(p).any(axis=1) | np.isinf(p[:, 0]) | np.isinf(p[:, 1]))


def build(points, tile_m):
    """-> dict(points = sorted float32 [N', 4], offsets = int32 [rows * cols + 1], keys = int32 [N] (-1 = dropped), ox, oy, rows, cols,
    dropped)"""
    p = as_aos32(points)
    k = kept(p)
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    tile_m = float(tile_m)
    ox = math.floor(x[k].min() / tile_m) * tile_m
    oy = math.floor(y[k].min() / tile_m) * tile_m
    with np.errstate(invalid="ignore", over="ignore"):
        ix = np.floor((x - ox) / tile_m)
        iy = np.floor((y - oy) / tile_m)
    rows, cols = int(ix[k].max()) + 1, int(iy[k].max()) + 1
    keys = np.full(len(p), -1, dtype=np.int64)
    keys[k] = ix[k].astype(np.int64) * cols + iy[k].astype(np.int64)
    idx = np.nonzero(k)[0]
    order = idx[np.argsort(keys[idx], kind="stable")]
    counts = np.bincount(keys[idx], minlength=rows * cols)
    offsets = np.zeros(rows * cols + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    return dict(points=np.ascontiguousarray(p[order]), offsets=offsets.astype(np.int32), keys=keys.astype(np.int32), ox=ox, oy=oy, rows=rows,
                cols=cols, tile_m=tile_m, dropped=int((~k).sum()), order=order)


def clip(rect, rows, cols):
    r0, r1, c0, c1 = rect
    return max(r0, 0), min(r1, rows - 1), max(c0, 0), min(c1, cols - 1)


def runs(ix, rect, last_column_off_by_one=False):
    """[(first, last + 1)] of the rectangle's rows in the sorted cloud, in row order (a clipped rectangle; empty -> [])"""
    r0, r1, c0, c1 = rect
    if r0 > r1 or c0 > c1:
        return []
    off, cols = ix["offsets"], ix["cols"]
    end = c1 if last_column_off_by_one else c1 + 1
    return [(int(off[r * cols + c0]), int(off[r * cols + end])) for r in range(r0, r1 + 1)]


def count(ix, rect):
    """-> (M, non-empty runs)"""
    rr = runs(ix, rect)
    return sum(b - a for a, b in rr), sum(1 for a, b in rr if b > a)


def gather(ix, rect, **kw):
    rr = runs(ix, rect, **kw)
    if not rr:
        return np.zeros((0, 4), dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([ix["points"][a:b] for a, b in rr]))


# ---------------------------------------------------------------------------------------------------------------- the window
def pose_matrix(pose7):
    """translation . rotation of a pose (tx, ty, tz, qx, qy, qz, qw)"""
    tx, ty, tz, x, y, z, w = (float(v) for v in pose7)
    n = x * x + y * y + z * z + w * w
    s = 2.0 / n
    R = np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                  [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                  [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (tx, ty, tz)
    return T


def velodyne_to_baselink():
    """a pitch of 0.140 rad and the lever (2.64, 0, 1.98) (src/mapping.py:165-170)"""
    c, s = math.cos(0.140), math.sin(0.140)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = (2.64, 0.0, 1.98)
    return T


def velodyne_to_world(pose7):
    return pose_matrix(pose7) @ velodyne_to_baselink()


def pose_from(x, y, z=0.0, yaw=0.0, pitch=0.0, roll=0.0):
    """(tx, ty, tz, qx, qy, qz, qw) of R = Rz(yaw) Ry(pitch) Rx(roll)"""
    cy, sy, cp, sp, cr, sr = math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(roll / 2), math.sin(roll / 2)
    return np.array([x, y, z, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def frustum_vertices(K, R, t, H, W, range_max):
    """[3, 9]: the camera centre and the corner lines' crossings of x = 0 and x = range_max, velodyne frame"""
    c = -(R.T @ t.reshape(3, 1))
    out = [c]
    for x in (0.0, float(range_max)):
        for u, v in ((-1.0, -1.0), (W, -1.0), (-1.0, H), (W, H)):
            d = R.T @ np.linalg.solve(K, np.array([[u], [v], [1.0]]))
            out.append(c + d * (x - c[0, 0]) / d[0, 0])
    return np.hstack(out)


def window_box(pose7, cams, H, W, range_max, radius_m=0.0, margin_m=0.0):
    T = velodyne_to_world(pose7)
    if radius_m > 0:
        lo, hi = T[:2, 3] - radius_m, T[:2, 3] + radius_m
    else:
        v = np.hstack([frustum_vertices(np.asarray(c.K), np.asarray(c.R), np.asarray(c.t), H, W, range_max) for c in cams])
        w = (T @ np.vstack([v, np.ones((1, v.shape[1]))]))[:2]
        lo, hi = w.min(axis=1), w.max(axis=1)
    return lo[0] - margin_m, hi[0] + margin_m, lo[1] - margin_m, hi[1] + margin_m


def window(ix, pose7, cams, H, W, range_max, radius_m=0.0, margin_m=0.0):
    xmin, xmax, ymin, ymax = window_box(pose7, cams, H, W, range_max, radius_m, margin_m)
    t = ix["tile_m"]
    rect = (math.floor((xmin - ix["ox"]) / t), math.floor((xmax - ix["ox"]) / t), math.floor((ymin - ix["oy"]) / t), math.floor((ymax - ix["oy"]) / t))
    return clip(rect, ix["rows"], ix["cols"])


# ---------------------------------------------------------------------------------------------------------------- the clouds
X0, Y0, TILE = -8.0, 4.0, 4.0                 # the 8 x 6 index: tiles of 4 m from (-8, 4); the cloud's least x is -7: the origin is floored
BIG, SINGLE = (3, 2), (5, 4)
EMPTY = {(6, j) for j in range(6)} | {(2, 1), (2, 4), (4, 1), (0, 5)}
# unclipped tile rectangles: inside (its row 2 starts and ends with an empty tile, its row 6 is empty), clipped on each side, wholly outside,
# the whole index, one point
RECTS = {"inside": (2, 6, 1, 4), "low_rows": (-2, 3, 1, 4), "high_rows": (5, 11, 1, 4), "low_cols": (2, 5, -3, 2), "high_cols": (2, 5, 3, 9),
         "outside": (9, 12, 0, 5), "whole": (0, 7, 0, 5), "one_point": (5, 5, 4, 4)}


def cloud_8x6(seed=0):
    """float32 [N, 4], N about 5600, in shuffled order.  Tile BIG holds 3000 points (a run over several workgroups that ends off a
    workgroup's boundary), SINGLE one, EMPTY none; points lie exactly on tile edges and one is the cloud's largest x and y; a block of
    points shares x, y, z so that only the order tells them apart; NaN in each field in turn and +-inf in x are dropped, an infinite
    z or intensity is not.  The intensity is the point's number in the input: every point's bytes are its own."""
    rng = np.random.default_rng(seed)
    pts = []
    for i in range(8):
        for j in range(6):
            if (i, j) in EMPTY:
                continue
            n = 3000 if (i, j) == BIG else (1 if (i, j) == SINGLE else 70)
            u = rng.uniform(0.26 if i == 0 else 0.01, 0.99, n)
            v = rng.uniform(0.01, 0.99, n)
            pts.append(np.stack([X0 + TILE * (i + u), Y0 + TILE * (j + v), rng.uniform(-0.5, 2.5, n)], axis=1))
    edges = [(X0 + TILE * 1, Y0 + 1.5, 0.0), (X0 + TILE * 3, Y0 + TILE * 2, 0.5), (X0 + 5.0, Y0, 0.25), (X0 + TILE * 7, Y0 + TILE * 5, 1.0),
             (X0 + TILE * 5, Y0 + TILE * 3, 0.0), (X0 + 31.98, Y0 + 23.98, 0.0)]
    pts.append(np.array(edges))
    pts.append(np.tile(np.array([[X0 + 13.0, Y0 + 9.0, 0.3]]), (40, 1)))              # 40 copies in tile BIG
    p = np.concatenate(pts)
    flag = np.zeros(len(p) + len(BAD_FIELDS), dtype=np.int64)
    flag[len(p):] = 1 + np.arange(len(BAD_FIELDS))
    p = np.concatenate([p, np.tile(np.array([[X0 + 10.0, Y0 + 10.0, 0.0]]), (len(BAD_FIELDS), 1))])          # tile (2, 2)
    perm = rng.permutation(len(p))
    p, flag = p[perm], flag[perm]
    out = np.concatenate([p, np.arange(len(p), dtype=np.float64)[:, None]], axis=1).astype(np.float32)
    for k, (col, val) in enumerate(BAD_FIELDS):
        out[np.nonzero(flag == k + 1)[0][0], col] = val
    return out


BAD_FIELDS = [(0, np.nan), (1, np.nan), (2, np.nan), (3, np.nan), (0, np.inf), (0, -np.inf), (1, np.inf), (2, np.inf), (3, -np.inf)]
N_DROPPED_8X6 = 7           # of the nine: an infinite z or intensity is kept


def cloud_rows70(seed=1):
    """float32 [700, 4] over 70 rows x 3 columns of 1 m tiles: the rows of one rectangle outnumber a wave's lanes"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0.0, 69.99, 700), rng.uniform(0.0, 2.99, 700), rng.uniform(0, 1, 700), np.arange(700)], axis=1)
    p[0, :2], p[1, :2] = (0.0, 0.0), (69.5, 2.5)
    return p.astype(np.float32)


def cloud_tall(seed=2):
    """float32 [1500, 4] over 1200 rows x 2 columns of 0.05 m tiles: more rows than one launch of the gather takes"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0.0, 59.99, 1500), rng.uniform(0.0, 0.0999, 1500), rng.uniform(0, 1, 1500), np.arange(1500)], axis=1)
    p[0, :2], p[1, :2] = (0.0, 0.0), (59.99, 0.09)
    return p.astype(np.float32)
