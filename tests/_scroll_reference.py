"""NumPy restatement of the scrolling grid (MAPPING.SCROLL), shared by test_scroll_cpu.py and test_gpu_scroll.py.

* the geometry, written out again from the rule (not imported from scroll.py);
* an executor of tile-job tables on NumPy byte buffers (struct avl_tile_job's rule: copy or fill, the emptiness flag);
* a "big array" site: one array that covers every window of a drive; a frame is applied by oracle.mapping_oracle.mapping_frame to
  the VIEW big[i0 - I : i0 - I + Hm, j0 - J : j0 - J + Wm] with window_boundary(origin)'s floats.  The view is written in place, so
  a cell's additions happen in frame order and bit equality holds for the log confusion matrix too;
* the drive of the end-to-end tests: poses, world-frame clouds and colour images.
"""
import math

import numpy as np

OFFSET = (1369.0496826171875, 562.84814453125)           # oracle.mapping_oracle.PCD_ORIGIN_OFFSET[:2]


# ------------------------------------------------------------------------------------------------ geometry
def window_boundary(anchor, origin, Hm, Wm, res):
    x0 = anchor[0] + float(origin[0]) * res
    y0 = anchor[1] + float(origin[1]) * res
    return [[x0, x0 + Hm * res], [y0, y0 + Wm * res]]


def vehicle_cell(pose7, anchor, res):
    c = [math.floor((pose7[k] + OFFSET[k] - anchor[k]) / res) if math.isfinite(pose7[k]) else None for k in range(2)]
    return None if None in c else (c[0], c[1])


def next_origin(current, cell, Ht, Wt, T, hysteresis):
    """current None = first call"""
    if cell is None:
        return current if current is not None else (0, 0)
    want = (math.floor(cell[0] / T) - Ht // 2, math.floor(cell[1] / T) - Wt // 2)
    if current is not None:
        cur = (current[0] // T, current[1] // T)
        if max(abs(want[0] - cur[0]), abs(want[1] - cur[1])) <= hysteresis:
            return current
    return want[0] * T, want[1] * T


def origins_of(poses, anchor, res, Ht, Wt, T, hysteresis):
    """-> [(origin after the frame's scroll_to, moved)] for every pose of a run that starts at origin (0, 0)"""
    out, cur, first = [], (0, 0), True
    for p in poses:
        new = next_origin(None if first else cur, vehicle_cell(p, anchor, res), Ht, Wt, T, hysteresis)
        first = False
        out.append((new, new != cur))
        cur = new
    return out


# ------------------------------------------------------------------------------------------------ the job executor
def execute_jobs(jobs, buffers, T, bpc, fill, n_flags):
    """``jobs``: scroll.Job records; ``buffers``: {key: np.uint8 array}, written in place.  -> int32 [n_flags]"""
    flags = np.zeros(n_flags, dtype=np.int32)
    row = T * bpc
    fill_row = np.full(row // 4, fill, dtype=np.uint32).view(np.uint8)
    for j in jobs:
        dst = buffers[j.dst]
        some = False
        for r in range(T):
            d0 = j.dst_off + r * j.dst_pitch
            if j.src is None:
                dst[d0:d0 + row] = fill_row
            else:
                s0 = j.src_off + r * j.src_pitch
                src_row = buffers[j.src][s0:s0 + row]
                some = some or bool((src_row.view(np.uint32) != np.uint32(fill)).any())
                dst[d0:d0 + row] = src_row
        if j.flag >= 0:
            flags[j.flag] |= int(some)
    return flags


# ------------------------------------------------------------------------------------------------ the big-array site
class BigSite(object):
    """One array over the tile rectangle [ti0, ti1] x [tj0, tj1] (inclusive); cell (i, j) of the site is big[i - I, j - J]."""

    def __init__(self, tile_rect, T, shape_tail, dtype):
        ti0, ti1, tj0, tj1 = tile_rect
        self.T, self.I, self.J = T, ti0 * T, tj0 * T
        self.tile_rect = tile_rect
        self.big = np.zeros(((ti1 - ti0 + 1) * T, (tj1 - tj0 + 1) * T) + tuple(shape_tail), dtype=dtype)

    def view(self, origin, Hm, Wm):
        a, b = origin[0] - self.I, origin[1] - self.J
        assert a >= 0 and b >= 0 and a + Hm <= self.big.shape[0] and b + Wm <= self.big.shape[1], "the big array does not cover the window"
        return self.big[a:a + Hm, b:b + Wm]

    def tile(self, t):
        a, b = t[0] * self.T - self.I, t[1] * self.T - self.J
        return self.big[a:a + self.T, b:b + self.T]

    def nonempty_tiles(self):
        ti0, ti1, tj0, tj1 = self.tile_rect
        out = []
        for ti in range(ti0, ti1 + 1):
            for tj in range(tj0, tj1 + 1):
                words = np.ascontiguousarray(self.tile((ti, tj))).view(np.uint32)      # bit patterns: a -0.0 is something
                if (words != 0).any():
                    out.append((ti, tj))
        return out

    def region(self, tiles):
        """the bounding rectangle of ``tiles`` -> ((i0, j0), array)"""
        ti0, ti1 = min(t[0] for t in tiles), max(t[0] for t in tiles)
        tj0, tj1 = min(t[1] for t in tiles), max(t[1] for t in tiles)
        a, b = ti0 * self.T - self.I, tj0 * self.T - self.J
        return (ti0 * self.T, tj0 * self.T), self.big[a:a + (ti1 - ti0 + 1) * self.T, b:b + (tj1 - tj0 + 1) * self.T]


# ------------------------------------------------------------------------------------------------ a scroll as a job table
class TableCase(object):
    """A random old window and store on one big array of bytes, the scroll by ``shift`` as a job table, and every buffer the table
    names as NumPy bytes (each with a fake 16-byte-aligned device address for the validator)."""

    def __init__(self, shift, bpc, fill, T4, HT, WT, CHUNK, OLD, seed=0):
        from vision_semantic_segmentation_amd import scroll as s
        rng = np.random.default_rng(seed + 17 * bpc + 101 * ((shift[0] + 10) * 21 + shift[1] + 10))
        self.T, self.bpc, self.fill, self.Ht, self.Wt, self.chunk, self.old = T4, bpc, fill, HT, WT, CHUNK, OLD
        self.Hm, self.Wm = HT * T4, WT * T4
        self.new = (OLD[0] + shift[0], OLD[1] + shift[1])
        ti0, ti1 = min(OLD[0], self.new[0]) - 1, max(OLD[0], self.new[0]) + HT
        tj0, tj1 = min(OLD[1], self.new[1]) - 1, max(OLD[1], self.new[1]) + WT
        self.site = BigSite((ti0, ti1, tj0, tj1), T4, (bpc,), np.uint8)
        self.site.big[...] = np.full(4, fill, dtype=np.uint32).view(np.uint8)[np.arange(bpc) % 4]         # everything empty
        old_tiles = s.window_tiles(OLD, HT, WT)
        entering = [t for t in s.window_tiles(self.new, HT, WT) if t not in old_tiles]
        self.stored = [t for k, t in enumerate(entering) if k % 3 != 1]                                   # stored tiles at some entering places
        some = bytes(range(1, 256))
        for k, t in enumerate(old_tiles + self.stored):
            tile = self.site.tile(t)
            if k % 5 == 3:
                continue                                               # an empty tile: its flag must stay 0
            if k % 5 == 4:                                              # the only non-fill word is the tile's last
                tile[-1, -1, -4:] = np.frombuffer(np.uint32(fill ^ 0x00010000).tobytes(), dtype=np.uint8)
                continue
            if k % 5 == 2 and bpc % 8 == 0 and fill == 0:               # all zero but one -0.0
                tile[1, 2, 0:8] = np.frombuffer(np.float64(-0.0).tobytes(), dtype=np.uint8)
                continue
            tile[...] = rng.choice(np.frombuffer(some, dtype=np.uint8), size=tile.shape)
        self.plan = s.plan_scroll(OLD, self.new, HT, WT, set(self.stored))
        self.slab_of_stored = {t: k for k, t in enumerate(self.stored)}
        self.fresh = list(range(len(self.stored), len(self.stored) + len(self.plan["leaving"])))
        n_slabs = len(self.stored) + len(self.fresh)
        slab = T4 * T4 * bpc
        self.bufs = {"old": np.ascontiguousarray(self.site.view((OLD[0] * T4, OLD[1] * T4), self.Hm, self.Wm)).reshape(-1).copy(),
                     "new": np.full(self.Hm * self.Wm * bpc, 0xAB, dtype=np.uint8)}
        for c in range(-(-n_slabs // CHUNK)):
            self.bufs[("chunk", c)] = np.full(CHUNK * slab, 0xAB, dtype=np.uint8)
        for t, k in self.slab_of_stored.items():
            key, off, _ = s.slab_ref(k, CHUNK, T4, bpc)
            self.bufs[key][off:off + slab] = self.site.tile(t).reshape(-1)
        self.jobs = s.scroll_jobs(self.plan, OLD, self.new, T4, self.Wm, bpc, CHUNK, self.fresh, self.slab_of_stored)
        self.extents = {key: (4096 * (k + 1) * 64, int(b.size)) for k, (key, b) in enumerate(self.bufs.items())}

    def want_flags(self):
        return np.array([int((np.ascontiguousarray(self.site.tile(t)).view(np.uint32) != self.fill).any()) for t in self.plan["leaving"]], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the drive
def yaw_pose(x, y, yaw):
    return np.array([x, y, 0.0, 0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0)], dtype=np.float64)


class Drive(object):
    """Poses, world-frame clouds and colour images of a drive on a window of Hm x Wm cells of ``res`` metres with tiles of ``tile_m``.
    ``route``: [(x, y, yaw)] in metres relative to the anchor's vehicle position: the vehicle at (0, 0) stands on global cell (0, 0).
    The clouds are synthetic.make_cloud draws through both cameras in the velodyne frame, taken to the world by the frame's pose."""

    IMG_H, IMG_W = 96, 128

    def __init__(self, route, res, Hm, Wm, tile_m, range_max=12.0, n_points=1500, seed=0, hysteresis=1):
        from oracle import mapping_oracle as mo
        from vision_semantic_segmentation_amd import synthetic as syn
        from vision_semantic_segmentation_amd.camera import camera_setup_1, camera_setup_6
        self.res, self.Hm, self.Wm, self.tile_m, self.range_max, self.hysteresis = res, Hm, Wm, tile_m, range_max, hysteresis
        self.T = int(round(tile_m / res))
        self.Ht, self.Wt = Hm // self.T, Wm // self.T
        self.anchor = (OFFSET[0], OFFSET[1])                              # pose (0, 0) is the corner of global cell (0, 0)
        self.boundary = [[self.anchor[0], self.anchor[0] + Hm * res], [self.anchor[1], self.anchor[1] + Wm * res]]
        self.poses = [yaw_pose(x, y, yaw) for x, y, yaw in route]
        self.cams = [camera_setup_1().scaled(self.IMG_W / 1920.0, self.IMG_H / 1440.0), camera_setup_6().scaled(self.IMG_W / 1920.0, self.IMG_H / 1440.0)]
        rng = np.random.default_rng(seed)
        self.T_vb = mo.velodyne_to_baselink()
        velo = [np.concatenate([syn.make_cloud(rng, n_points, c.K, c.R, c.t, self.IMG_W, self.IMG_H, depth=(1.5, range_max + 3.0)) for c in self.cams], axis=1)
                for _ in range(3)]
        images = [[syn.colorize(syn.make_label_map(rng, self.IMG_H, self.IMG_W, tile=7)) for _ in self.cams] for _ in range(3)]
        self.clouds, self.images = [], []
        for k, p in enumerate(self.poses):
            v = velo[k % 3]
            M = np.matmul(mo.transform_from_pose(p), self.T_vb)
            with np.errstate(all="ignore"):
                w = np.matmul(M, np.vstack([v[0:3], np.ones((1, v.shape[1]))]))
            self.clouds.append(np.ascontiguousarray(np.vstack([w[0:3], v[3:4]])))
            self.images.append(images[k % 3])
        self.origins = origins_of(self.poses, self.anchor, res, self.Ht, self.Wt, self.T, hysteresis)
        tiles_i = [o[0] // self.T for o, _ in self.origins] + [0]
        tiles_j = [o[1] // self.T for o, _ in self.origins] + [0]
        self.tile_rect = (min(tiles_i), max(tiles_i) + self.Ht - 1, min(tiles_j), max(tiles_j) + self.Wt - 1)

    def cfg(self, grid_dtype="f64", scroll=True, elevation=False, boundary=None):
        from vision_semantic_segmentation_amd import get_cfg_defaults
        cfg = get_cfg_defaults()
        cfg.MAPPING.BOUNDARY = self.boundary if boundary is None else boundary
        cfg.MAPPING.RESOLUTION = self.res
        cfg.MAPPING.PCD.RANGE_MAX = self.range_max
        cfg.MAPPING.GRID_DTYPE = grid_dtype
        cfg.MAPPING.DEPTH_METHOD = "points_raw"
        cfg.MAPPING.SCROLL.ENABLED = bool(scroll)
        cfg.MAPPING.SCROLL.TILE_M = self.tile_m
        cfg.MAPPING.SCROLL.HYSTERESIS_TILES = self.hysteresis
        cfg.MAPPING.SCROLL.POOL_CHUNK_TILES = 8
        cfg.MAPPING.ELEVATION.ENABLED = bool(elevation)
        return cfg

    def oracle_cfg(self, confusion_matrix, boundary, use_intensity=True):
        from oracle import mapping_oracle as mo
        return dict(range_max=self.range_max, boundary=boundary, resolution=self.res, label_names=mo.LABELS_NAMES,
                    label_colors=np.asarray(mo.LABEL_COLORS), confusion_matrix=confusion_matrix, use_pcd_intensity=use_intensity,
                    T_velodyne_to_baselink=self.T_vb)

    def numpy_site(self, confusion_matrix, dtype=np.float64, frames=None, stats=None):
        """The drive on the big array -> BigSite.  ``stats``: a dict that receives what the not-vacuous assertions need."""
        from oracle import mapping_oracle as mo
        site = BigSite(self.tile_rect, self.T, (len(mo.LABELS_NAMES),), dtype)
        frames = range(len(self.poses)) if frames is None else frames
        for k in frames:
            origin = self.origins[k][0]
            boundary = window_boundary(self.anchor, origin, self.Hm, self.Wm, self.res)
            view = site.view(origin, self.Hm, self.Wm)
            before = view.copy() if stats is not None else None
            ocfg = self.oracle_cfg(confusion_matrix, boundary)
            for image, cam in zip(self.images[k], self.cams):
                mo.mapping_frame(view, self.clouds[k], "world", image, self.poses[k], cam.P, ocfg)
                if stats is not None:
                    mp, lab = mo.project_pcd(self.clouds[k], "world", image, self.poses[k], cam.P, self.range_max, self.T_vb)
                    _, on = mo.cell_indices(mp, boundary, self.res, self.Hm, self.Wm)
                    votes = (lab.T[:, None, :] == np.asarray(mo.LABEL_COLORS)[None]).all(axis=2).any(axis=1)     # the pixel is a map class
                    stats.setdefault("outside", []).append(int((votes & ~on).sum()))
            if stats is not None:
                stats.setdefault("changed", []).append(np.any(view != before, axis=2))
        return site


# out along x across three tile edges, along y, diagonally back over stored tiles (heading back, so the frames add to them), one jump
# further than the window and back, then on past the anchor to negative cells
ROUTE = [(-1.5, 1.0, 0.0), (2.5, 1.0, 0.0), (6.5, 1.0, 0.0), (10.5, 1.0, 0.0), (14.5, 1.0, 0.0),
         (14.5, 5.0, 1.2), (14.5, 9.5, 1.5),
         (10.5, 5.5, math.pi), (6.5, 1.5, math.pi), (2.5, 1.5, math.pi),
         (62.5, 41.0, 0.3), (63.0, 41.5, 0.3),
         (2.5, 1.5, math.pi), (-1.5, 1.0, math.pi), (-5.5, -3.0, math.pi)]


def main_drive(seed=0):
    return Drive(ROUTE, res=0.5, Hm=48, Wm=32, tile_m=4.0, range_max=12.0, seed=seed)
