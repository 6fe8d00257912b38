"""The height rule of include/avl_hip.h (struct avl_height, rules 1 - 6) restated in NumPy, and the small seeded scenes the height
tests share.  Nothing here is shared with the kernels: the projection and the labels come from oracle/mapping_oracle.py (through
_occlusion_reference.Projection and, for logits, _point_logits_reference.full_labels), rules 1 - 3 are Python loops of scalar float64
operations in the stated order (one rounding each), and the elevation layer is built with np.add.at, np.minimum.at and np.maximum.at.

MUTANTS names deliberately wrong variants of the rule; tests/test_height_cpu.py asserts that each of them changes the result on some
scene, i.e. that the scenes can tell the rule from its likely mis-implementations."""
import math

import numpy as np

import _occlusion_reference as occ
import _point_logits_reference as plr
from oracle import mapping_oracle as mo

SIZES = occ.SIZES                                  # projection images (img_w, img_h): 96 x 64 and 97 x 61
GRIDS = {"g64": (64, 64, 0.5), "g50x30": (50, 30, 0.6)}      # the occlusion tests' grids
COUNTS = [1, 11, 63, 257, 3000]
RANGE_MAX = occ.RANGE_MAX
C = 5
# the ground in the velodyne frame: the example normal (0.02, -0.01, 1) with d = 2, scaled by 1.5 so that a rule which forgets to
# normalise is off by half
PLANE = (0.03, -0.015, 1.5, 3.0)
MIN_M = [-0.5] * C                                 # MAPPING.HEIGHT_GATE's defaults
MAX_M = [0.5, 0.5, 0.5, math.inf, 0.5]
SLOPE = 0.02
ELEV_CLASSES = 0b10111                             # MAPPING.ELEVATION's defaults: everything but vegetation
QUANTUM = 0.001
POSE7 = np.array([0.3, 0.25, 0.2, 0.0, 0.0, 0.0871557427, 0.9961946981])       # the vehicle in the world: yawed by 10 degrees
IDS = np.array([2, 1, 8, 10, 3, 0], dtype=np.uint8)          # the five map classes and one the map does not hold
MUTANTS = ("exclusive_bounds", "radial_slack", "bonus_survives", "one_bound", "unnormalised_plane", "velodyne_plane_on_world_cloud",
           "elevation_per_view")
EMPTY = (0, 0, np.iinfo(np.int32).max, np.iinfo(np.int32).min)


# ---------------------------------------------------------------------------------------------------------------- the rule
def normalise(plane):
    """the host's part of rule 1: n = sqrt((a * a + b * b) + c * c), each of the four divided by n, all negated when c < 0"""
    a, b, c, d = (float(v) for v in plane)
    n = math.sqrt((a * a + b * b) + c * c)
    a, b, c, d = a / n, b / n, c / n, d / n
    return (-a, -b, -c, -d) if c < 0.0 else (a, b, c, d)


def origin_to_velodyne(pose7):
    return np.linalg.inv(np.matmul(mo.transform_from_pose(pose7), mo.velodyne_to_baselink()))        # src/mapping.py:368-369


def plane_in_cloud_frame(plane, frame_id, pose7, mutant=None):
    """the velodyne-frame plane in the frame of the cloud, normalised: what goes to the kernel"""
    p = np.asarray(plane, dtype=np.float64)
    if frame_id != "velodyne" and mutant != "velodyne_plane_on_world_cloud":
        p = np.matmul(p, origin_to_velodyne(pose7))
    return tuple(float(v) for v in p) if mutant == "unnormalised_plane" else normalise(p)


def heights(pcd, plane_n):
    """rule 1 for every point -> float64 [n]; NaN for a point with a non-finite coordinate"""
    a, b, c, d = plane_n
    out = np.full(pcd.shape[1], np.nan)
    for k in range(pcd.shape[1]):
        x, y, z = float(pcd[0, k]), float(pcd[1, k]), float(pcd[2, k])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        t = a * x
        u = b * y
        t = t + u
        u = c * z
        t = t + u
        out[k] = t + d
    return out


def slacks(pcd, v0, slope, mutant=None, xy=None):
    """rule 2 for every point -> float64 [n]: slope * v0, v0 the forward distance of src/mapping.py:371; NaN as heights()"""
    out = np.full(pcd.shape[1], np.nan)
    for k in range(pcd.shape[1]):
        if not np.isfinite(pcd[0:3, k]).all():
            continue
        f = float(v0[k])
        if mutant == "radial_slack":
            f = math.sqrt(float(xy[0, k]) ** 2 + float(xy[1, k]) ** 2)
        out[k] = float(slope) * f
    return out


def gate(bits, h, s, min_m, max_m, n_classes=C, mutant=None):
    """rule 3 for every point: uint32 [n] vote bits (class i at bit i, its bonus at 16 + i) -> the bits that stay"""
    out = np.zeros_like(bits)
    for k in np.nonzero(bits)[0]:
        b, keep = int(bits[k]), 0
        for i in range(n_classes):
            j = 0 if mutant == "one_bound" else i
            lo = float(min_m[j]) - float(s[k])
            hi = float(max_m[j]) + float(s[k])
            ok = (lo < h[k] and h[k] < hi) if mutant == "exclusive_bounds" else (lo <= h[k] and h[k] <= hi)
            if ok:
                keep |= 1 << i
        mask = keep | (keep << 16)
        if mutant == "bonus_survives":
            mask |= 0xffff0000
        out[k] = b & mask
    return out


def empty_layer(Hm, Wm):
    return [np.full((Hm, Wm), EMPTY[0], dtype=np.int64)] + [np.full((Hm, Wm), v, dtype=np.int32) for v in EMPTY[1:]]


def elevate(layer, cells, z, kept_views, elev_classes=ELEV_CLASSES, quantum=QUANTUM, mutant=None):
    """rule 5 for one call: ``kept_views`` = the surviving bits per view, uint32 [V, n]; cells = the oracle's int32 [2, n]"""
    class_bits = np.asarray(kept_views) & 0xffff
    rounds = [row for row in class_bits] if mutant == "elevation_per_view" else [np.bitwise_or.reduce(class_bits, axis=0)]
    with np.errstate(all="ignore"):
        q = np.rint(np.asarray(z, dtype=np.float64) / float(quantum))
    fits = (q >= -2147483648.0) & (q <= 2147483647.0)
    for union in rounds:
        take = ((union & elev_classes) != 0) & fits
        i, j, qi = cells[0, take], cells[1, take], q[take].astype(np.int64)
        np.add.at(layer[0], (i, j), qi)
        np.add.at(layer[1], (i, j), 1)
        np.minimum.at(layer[2], (i, j), qi.astype(np.int32))
        np.maximum.at(layer[3], (i, j), qi.astype(np.int32))
    return layer


def elevation_mean(layer, quantum=QUANTUM):
    with np.errstate(all="ignore"):
        mean = (layer[0].astype(np.float64) / layer[1].astype(np.float64)) * float(quantum)
    return np.where(layer[1] == 0, np.nan, mean).astype(np.float32)


def apply_votes(grid, cells, bits_views, cm, use_intensity_bonus=True, n_classes=C):
    """the apply the header documents: view 0 first; inside a view class i ascending (+= CM[:, i] once per cell, the buffered add
    of src/mapping.py:424), each followed by its bonus (+2 once per cell, :437)"""
    for bits in bits_views:
        for i in range(n_classes):
            idx = ((bits >> i) & 1).astype(bool)
            grid[cells[0, idx], cells[1, idx], :] += np.asarray(cm)[:, i].reshape(1, -1).astype(grid.dtype)
            bon = ((bits >> (16 + i)) & 1).astype(bool)
            grid[cells[0, bon], cells[1, bon], i] += 2
    return grid


# ---------------------------------------------------------------------------------------------------------------- labels
def class_bits_of_colours(rg, colours):
    """uint8 [n, >= 2] red and green -> uint32 [n]: bit i where both match colour i (blue is ignored, src/mapping.py:419)"""
    bits = np.zeros(rg.shape[0], dtype=np.uint32)
    for i, col in enumerate(colours):
        bits |= (((rg[:, 0] == col[0]) & (rg[:, 1] == col[1])).astype(np.uint32) << np.uint32(i))
    return bits


def pixel_bits(proj, source, kind, colours=mo.LABEL_COLORS, palette=mo.PALETTE_19, min_margin=0.0):
    """the vote bits (no bonus yet) every candidate's pixel gives; 0 for the rest.  kind "rgb": a colour image of the projection size;
    "classmap": a class map sampled as its nearest-upscaled image; "logits": fp32 [h', w', K] interpolated to the projection size"""
    ix, iy = np.where(proj.cand, proj.ix, 0), np.where(proj.cand, proj.iy, 0)
    if kind == "rgb":
        bits = class_bits_of_colours(np.asarray(source)[iy, ix], colours)
    else:
        if kind == "logits":
            source = plr.full_labels(np.asarray(source), proj.img_h, proj.img_w, min_margin)
        lab = mo.resize_nearest(np.asarray(source), proj.img_h, proj.img_w)[iy, ix]
        pal = np.zeros((256, 3), dtype=np.uint8)
        pal[:len(palette)] = np.asarray(palette, dtype=np.uint8)
        lut = class_bits_of_colours(pal, colours)
        lut[len(palette):] = 0
        bits = lut[lab]
    return np.where(proj.cand, bits, 0).astype(np.uint32)


def with_bonus(bits, intensity, bonus_classes):
    """the lane bonus of src/mapping.py:431-437 at bit 16 + i"""
    with np.errstate(invalid="ignore"):
        odd = (intensity < 2) | (intensity > 14)
    lane = bits & np.uint32(bonus_classes)
    return np.where(odd, bits | (lane << np.uint32(16)), bits).astype(np.uint32)


def bonus_classes(use_intensity, names=mo.LABELS_NAMES):
    return sum(1 << i for i, n in enumerate(names) if n == "lane") if use_intensity else 0


# ---------------------------------------------------------------------------------------------------------------- scenes
def ground_z(x, y, plane=PLANE):
    a, b, c, d = plane
    return -(a * x + b * y + d) / c


def make_cloud(seed, n, frame_id="velodyne"):
    """float64 [4, n]: a ground sheet with +-0.2 m of noise, a canopy 2 to 5 m above it, shrubs that straddle the upper bound
    and its slack (0.3 to 1.6 m) and a few points below the ground (-0.3 to -2.5 m), 8 to 38 m in front of the sensor, all inside the image.  The n
    points are the first n of one shuffled 3000-point scene.  frame_id "world": the same points moved to the world by POSE7."""
    rng = np.random.default_rng(seed)
    m = max(n, 3000)
    kinds = rng.choice(4, size=m, p=[0.48, 0.26, 0.13, 0.13])
    u = rng.random((3, m))
    x = 8.0 + 30.0 * u[0]
    y = (u[1] * 2 - 1) * np.minimum(0.7 * x, 15.0)
    hgt = np.select([kinds == 0, kinds == 1, kinds == 2], [-0.2 + 0.4 * u[2], 2.0 + 3.0 * u[2], 0.3 + 1.3 * u[2]], -0.3 - 2.2 * u[2])
    pcd = np.stack([x, y, ground_z(x, y) + hgt * (math.sqrt(PLANE[0] ** 2 + PLANE[1] ** 2 + PLANE[2] ** 2) / PLANE[2]), 20.0 * rng.random(m)])[:, :n]
    if frame_id != "velodyne":
        pcd = np.concatenate([np.matmul(np.linalg.inv(origin_to_velodyne(POSE7)), mo.homogenize(pcd[0:3]))[0:3], pcd[3:4]])
    return np.ascontiguousarray(pcd)


def boundary(grid, frame_id="velodyne"):
    """map_boundary of the grid: as the occlusion tests' for a velodyne-frame cloud, moved to where POSE7 puts the scene for a
    world-frame one"""
    Hm, Wm, res = GRIDS[grid]
    if frame_id == "velodyne":
        return occ.boundary(Hm, Wm, res)
    ox, oy = mo.PCD_ORIGIN_OFFSET[0] + 11.0, mo.PCD_ORIGIN_OFFSET[1] + 4.0
    return [[ox, ox + Hm * res], [oy - Wm * res / 2, oy + Wm * res / 2]]


def make_sources(seed, w, h, V, kind):
    """V semantic sources (NumPy): colour images [h, w, 3], class maps of half the projection size, or logits of a quarter of it
    with K = 19 and the map's classes favoured"""
    from vision_semantic_segmentation_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    out = []
    for v in range(V):
        if kind == "rgb":
            out.append(syn.colorize(IDS[syn.make_label_map(rng, h, w, num_classes=6, tile=5)]))
        elif kind == "classmap":
            out.append(IDS[syn.make_label_map(rng, h // 2, w // 2, num_classes=6, tile=3)])
        else:
            out.append(np.ascontiguousarray(plr.make_logits(seed * 10 + v, h // 4, w // 4, 19, favour=1.5)))
    return out


YAWS = [0.0, 0.3, -0.3]


def cameras(w, h, V):
    return [occ.pinhole_P(w, h, yaw=YAWS[v % 3]) for v in range(V)]


class Scene(object):
    """One cloud seen by V views on one grid: the oracle's projections and cells, the pixel's vote bits per view, and the rule.
    ``culled`` (bool [V, n], default nothing) are the candidates occlusion removed before the rule."""

    def __init__(self, name, grid, size, n, seed, V=1, kind="rgb", frame_id="velodyne", use_intensity=True, plane=PLANE,
                 colours=mo.LABEL_COLORS, min_m=MIN_M, max_m=MAX_M, slope=SLOPE, cloud=None, sources=None):
        self.name, self.grid, self.n, self.V, self.kind, self.frame_id = name, grid, n, V, kind, frame_id
        self.w, self.h = size
        self.Hm, self.Wm, self.res = GRIDS[grid]
        self.pose7 = POSE7 if frame_id != "velodyne" else None
        self.pcd = make_cloud(seed, n, frame_id) if cloud is None else np.ascontiguousarray(cloud, dtype=np.float64)
        self.Ps = cameras(self.w, self.h, V)
        self.sources = make_sources(seed, self.w, self.h, V, kind) if sources is None else sources
        self.use_intensity, self.plane, self.colours = use_intensity, plane, colours
        self.min_m, self.max_m, self.slope = list(min_m), list(max_m), slope
        self.boundary = boundary(grid, frame_id)
        self._projs = None

    def see(self, pcd):
        """the scene as a cloud of other coordinates sees it (a float32 cloud converted back to float64)"""
        self.pcd, self._projs = np.ascontiguousarray(pcd, dtype=np.float64), None
        return self

    @property
    def projs(self):
        if self._projs is None:
            self._projs = [occ.Projection(self.pcd, P, self.w, self.h, frame_id=self.frame_id, pose7=self.pose7) for P in self.Ps]
        return self._projs

    def cells(self):
        return mo.cell_indices(self.pcd, self.boundary, self.res, self.Hm, self.Wm)

    def plane_n(self, mutant=None):
        return plane_in_cloud_frame(self.plane, self.frame_id, self.pose7, mutant)

    def heights(self, mutant=None):
        return heights(self.pcd, self.plane_n(mutant))

    def slacks(self, mutant=None):
        xv = mo.homogenize(self.pcd[0:3])
        if self.frame_id != "velodyne":
            with np.errstate(all="ignore"):
                xv = np.matmul(origin_to_velodyne(self.pose7), xv)
        return slacks(self.pcd, self.projs[0].v0, self.slope, mutant, xy=xv[0:2])

    def bits_before(self, culled=None):
        """uint32 [V, n]: the bits b of the points the rule applies to (candidate, on the grid, not culled, not abstaining)"""
        on = self.cells()[1]
        bon = bonus_classes(self.use_intensity)
        rows = []
        for v, pr in enumerate(self.projs):
            b = with_bonus(pixel_bits(pr, self.sources[v], self.kind, self.colours), self.pcd[3], bon)
            live = pr.cand & on if culled is None else pr.cand & on & ~np.asarray(culled[v], dtype=bool)
            rows.append(np.where(live, b, 0).astype(np.uint32))
        return np.stack(rows)

    def bits_after(self, before=None, s=None, mutant=None, culled=None):
        """rule 3 per view; ``s``: the slack to use (the GPU's, for a world-frame cloud), default the reference's own"""
        before = self.bits_before(culled) if before is None else before
        h = self.heights(mutant)
        s = self.slacks(mutant) if s is None else s
        return np.stack([gate(before[v], h, s, self.min_m, self.max_m, len(self.colours), mutant) for v in range(self.V)])

    def gated_counts(self, before, after):
        return [int(((before[v] != 0) & (after[v] == 0)).sum()) for v in range(self.V)]

    def grid_after(self, bits_views, cm, dtype=np.float64):
        return apply_votes(np.zeros((self.Hm, self.Wm, len(self.colours)), dtype=dtype), self.cells()[0], bits_views, cm)

    def layer_after(self, kept_views, layer=None, mutant=None, elev_classes=ELEV_CLASSES, quantum=QUANTUM):
        layer = empty_layer(self.Hm, self.Wm) if layer is None else layer
        return elevate(layer, self.cells()[0], self.pcd[2], kept_views, elev_classes, quantum, mutant)


def scenes():
    """the single-view scenes: every grid x size x count in the velodyne frame, and the same clouds in the world frame"""
    out = []
    for gi, grid in enumerate(GRIDS):
        for si, size in enumerate(SIZES):
            for n in COUNTS:
                for frame_id in ("velodyne", "world"):
                    out.append(Scene("%s_%dx%d_n%d_%s" % (grid, size[0], size[1], n, frame_id), grid, size, n, 40 + 10 * gi + si + n, 1,
                                     "rgb", frame_id))
    return out


def view_scenes():
    """three views of one cloud, for the layer's once-per-call rule"""
    return [Scene("views3_%s_n%d_%s" % (grid, n, frame_id), grid, SIZES[k % 2], n, 70 + n + k, 3, "rgb", frame_id)
            for k, (grid, n, frame_id) in enumerate([("g64", 257, "velodyne"), ("g64", 3000, "world"), ("g50x30", 3000, "velodyne")])]


# exact cases: plane (0, 0, 1, 2), slope 0, dyadic numbers.  A point at h == max_m votes, the point at the next double above it is gated
# (its h = 0.5 + 2^-52, the smallest step a z near -1.5 can make); the same at min_m.  (x, y) are on both grids and inside the image; every pixel is "road"
EXACT_PLANE = (0.0, 0.0, 1.0, 2.0)
EXACT_MIN, EXACT_MAX = -0.5, 0.5


def exact_cloud():
    """(float64 [4, 8], expected survival bool [8])"""
    zs = [EXACT_MAX - 2.0, np.nextafter(EXACT_MAX - 2.0, np.inf), EXACT_MIN - 2.0, np.nextafter(EXACT_MIN - 2.0, -np.inf),
          -2.0, np.nextafter(EXACT_MAX - 2.0, -np.inf), np.nextafter(EXACT_MIN - 2.0, np.inf), 1.0]
    keep = [True, False, True, False, True, True, True, False]
    pts = np.array([[12.0 + 0.75 * k, -1.5 + 0.5 * k, z, 5.0] for k, z in enumerate(zs)]).T
    return np.ascontiguousarray(pts), np.array(keep)


def exact_scene(grid="g64", size=SIZES[0]):
    w, h = size
    road = np.empty((h, w, 3), dtype=np.uint8)
    road[:] = np.asarray(mo.LABEL_COLORS[0], dtype=np.uint8)
    cloud, keep = exact_cloud()
    return Scene("exact_%s" % grid, grid, size, cloud.shape[1], 0, 1, "rgb", plane=EXACT_PLANE, min_m=[EXACT_MIN] * C,
                 max_m=[EXACT_MAX] * C, slope=0.0, cloud=cloud, sources=[road]), keep
