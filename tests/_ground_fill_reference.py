"""The ground-fill rule of include/avl_hip.h (struct avl_ground_fill, rules 1 - 6) restated in NumPy float64, and the seeded cases
the ground-fill tests share.  Nothing here is shared with the kernels or with the package: the window's cell centres are put on the
plane one rounded operation per line (rule 1) and become a VIRTUAL CLOUD that goes through oracle/mapping_oracle.py -- project_pcd
finds the candidates, their pixels and their labels (rule 2), update_map applies the votes (rule 5; every virtual point lies in its
own cell, which tests/test_ground_fill_cpu.py checks, so the buffered `+=` of one class touches a cell once).  Every semantic
source becomes the colour image the reference's mapper would have been sent: a class map through the oracle's nearest upscale and
palette, logits through _point_logits_reference.full_labels (255, which has no colour, where a pixel abstains).  The depth buffer of
rule 3 comes from _occlusion_reference.depth_buffer on the oracle's projection of the real cloud.

    expected(case, grid0)              -> (grid, counts): the grid after the fill and dict(filled, culled, abstained) per view
    expected(case, grid0, mutant=...)  the same with the rule broken on purpose (MUTANTS); test_ground_fill_cpu.py asserts that every
                                       mutant changes the grid of some case
"""
import numpy as np

import _occlusion_reference as occ
import _point_logits_reference as plr
from oracle import mapping_oracle as mo

MUTANTS = ("cell_corner", "plane_not_in_grid_frame", "z_sign", "class_mask_ignored", "cloud_range", "empty_culls", "views_reversed",
           "round_once")

HM, WM, RES = 96, 80, 0.25
GROUND = (0.0, 0.0, 1.0, 2.0)                      # z = -2 in the velodyne frame: the ground of _occlusion_reference.make_cloud
TILTED = (0.03, -0.02, 1.0, 2.0)
CLOUD_RANGE = 100.0                                # MAPPING.PCD.RANGE_MAX: sizes the depth buffer, not the fill
WORLD_POSE = np.array([-1369.0496826171875 + 1369.3, -562.84814453125 + 563.1, 0.2, 0.0, 0.0, 0.0871557427, 0.9961946981])
FAVOUR = 1.5                                       # added to the logits of the classes the map holds, so that most cells vote
IDS = np.array([2, 1, 8, 10, 3, 0], dtype=np.uint8)     # the five map classes and one the map does not hold


# ---------------------------------------------------------------------------------------------------------------- inputs
def velodyne_boundary():
    """the grid of a cloud in the velodyne frame: x from 2 m behind the sensor to 22 m in front of it, y centred"""
    ox, oy = mo.PCD_ORIGIN_OFFSET[0], mo.PCD_ORIGIN_OFFSET[1]
    return [[ox - 2.0, ox - 2.0 + HM * RES], [oy - WM * RES / 2, oy + WM * RES / 2]]


def world_boundary():
    """the grid of a cloud in the world frame, around WORLD_POSE"""
    return [[1369.3 - 6.0, 1369.3 - 6.0 + HM * RES], [563.1 - WM * RES / 2, 563.1 + WM * RES / 2]]


def label_sets(C):
    """(names, colours [C][3], palette of 19 network colours whose class k < C is map class k) for C map classes; C = 5 is the
    reference's own set with its own palette"""
    if C == 5:
        return list(mo.LABELS_NAMES), [list(c) for c in mo.LABEL_COLORS], [list(c) for c in mo.PALETTE_19]
    colours = [[10 * i + 5, 200 - 7 * i, 3 * i] for i in range(C)]
    palette = colours + [[1, 2 + k, 3] for k in range(19 - C)]
    return ["c%d" % i for i in range(C)], colours, palette


def net_ids(C):
    """the network class ids a source draws from: those of the map classes, and one more"""
    return IDS if C == 5 else np.arange(C + 1, dtype=np.uint8)


def confusion(C, seed=5):
    """float64 [C][C] log-probabilities, NOT symmetric: column i is what a class-i vote adds"""
    rng = np.random.default_rng(seed)
    m = 0.05 + 0.2 * rng.random((C, C)) + 0.75 * np.eye(C)
    return np.log(m / m.sum(axis=1, keepdims=True))


def tiles(rng, h, w, ids, tile):
    coarse = rng.integers(0, len(ids), size=(-(-h // tile), -(-w // tile)))
    return np.ascontiguousarray(ids[np.kron(coarse, np.ones((tile, tile), dtype=np.int64))[:h, :w]])


def make_source(seed, kind, img_w, img_h, C, palette, ld=19, logits_kind="normal"):
    """one view's semantic source as the GPU call takes it: "rgb" uint8 [img_h, img_w, 3], "classmap" uint8 of half the size,
    "logits" float32 [12, 16, 19] (rows of `ld` floats)"""
    rng = np.random.default_rng(seed)
    if kind == "rgb":
        return mo.apply_color_map(tiles(rng, img_h, img_w, net_ids(C), 5), palette)
    if kind == "classmap":
        return tiles(rng, img_h // 2, img_w // 2, net_ids(C), 3)
    assert kind == "logits" and C == 5
    return plr.make_logits(seed, 12, 16, 19, logits_kind, ld=ld, favour=FAVOUR)


def net_size(img_w, img_h):
    """the size the logits are interpolated to: half the projection image, rounded up"""
    return (-(-img_h // 2), -(-img_w // 2))


def make_case(name, kind="classmap", views=1, img=(64, 48), frame="velodyne", window=None, plane=GROUND, C=5, weight=1.0,
              range_max=15.0, classes=None, occl=None, cloud=None, min_margin=0.0, ld=19, logits_kind="normal", seed=0):
    img_w, img_h = img
    names, colours, palette = label_sets(C)
    yaws = [0.0, 0.5, -0.5, 0.25, -0.25]
    case = dict(name=name, kind=kind, img_w=img_w, img_h=img_h, frame=frame, pose7=WORLD_POSE if frame != "velodyne" else None,
                boundary=world_boundary() if frame != "velodyne" else velodyne_boundary(), res=RES, Hm=HM, Wm=WM,
                window=window if window is not None else ((0, 0), (HM, WM)), plane=np.array(plane, dtype=np.float64), C=C,
                names=names, colours=colours, palette=palette, cm=confusion(C), weight=weight, range_max=range_max,
                classes=[n for n in names if n != "vegetation"] if classes is None else classes, occl=occl, cloud=cloud,
                min_margin=min_margin, net=net_size(img_w, img_h),
                P=[occ.pinhole_P(img_w, img_h, f=40.0, pitch=0.25, yaw=yaws[v]) for v in range(views)])
    case["sources"] = [make_source(1000 * seed + 10 * len(name) + v, kind, img_w, img_h, C, palette, ld, logits_kind) for v in range(views)]
    return case


def cases():
    """the seeded cases: every one is compared bit for bit on the GPU, for f64 and f32 maps"""
    wall = occ.make_cloud(77, 2000)
    out = [
        make_case("classmap_1view"),
        make_case("rgb_1view", kind="rgb", img=(97, 61)),
        make_case("logits_1view", kind="logits", ld=24),
        make_case("classmap_3views", views=3, seed=1),
        make_case("rgb_3views", kind="rgb", views=3, seed=2),
        make_case("logits_3views", kind="logits", views=3, img=(97, 61), seed=3),
        make_case("world_classmap_3views", views=3, frame="world", seed=4),
        make_case("world_logits_1view", kind="logits", frame="world", seed=5),
        make_case("window_37x41", views=3, window=((45, 30), (37, 41)), seed=6),
        make_case("window_over_two_edges", views=3, window=((-9, -12), (90, 50)), seed=7),
        make_case("C5_4views", views=4, seed=8),
        make_case("classmap_5views", views=5, seed=16),             # more views than one call takes
        make_case("C16_4views", views=4, C=16, classes=["c%d" % i for i in range(16) if i != 3], seed=9),
        make_case("weight_half", kind="rgb", views=3, weight=0.5, seed=10),
        make_case("tilted_plane", views=3, plane=TILTED, seed=11),
        make_case("world_tilted_rgb", kind="rgb", views=3, frame="world", plane=TILTED, img=(97, 61), seed=12),
        make_case("wall_classmap", views=3, occl=dict(s=2, R=1, rel=0.25, abs_=0.5), cloud=wall, range_max=21.0, seed=13),
        make_case("wall_logits_1view", kind="logits", occl=dict(s=3, R=0, rel=0.1, abs_=0.3), cloud=wall, range_max=21.0, min_margin=0.3,
                  seed=14),
        make_case("gate_0", kind="logits", views=3, logits_kind="quantised", min_margin=0.0, seed=15),
        make_case("gate_0.3", kind="logits", views=3, logits_kind="quantised", min_margin=0.3, seed=15),
    ]
    return out


def seeded_grid(case, dtype, seed=3):
    """the non-zero grid a case starts from"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((case["Hm"], case["Wm"], case["C"])) * 3.0).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- the rule
def grid_T(case):
    """grid frame -> velodyne (src/mapping.py:368-369), None for a grid in the velodyne frame"""
    if case["frame"] == "velodyne":
        return None
    return np.linalg.inv(np.matmul(mo.transform_from_pose(case["pose7"]), mo.velodyne_to_baselink()))


def plane_in_grid_frame(case, mutant=None):
    T = grid_T(case)
    if T is None or mutant == "plane_not_in_grid_frame":
        return case["plane"].copy()
    return np.matmul(case["plane"], T)                 # (a, b, c, d) . (T X) = 0


def window_cells(case):
    """the window clipped to the grid -> (i, j) int64 arrays, j fastest"""
    (x0, y0), (h, w) = case["window"]
    i = np.arange(max(x0, 0), min(x0 + h, case["Hm"]), dtype=np.int64)
    j = np.arange(max(y0, 0), min(y0 + w, case["Wm"]), dtype=np.int64)
    ii, jj = np.meshgrid(i, j, indexing="ij")
    return ii.ravel(), jj.ravel()


def virtual_cloud(case, mutant=None):
    """rule 1 -> (float64 [4, n] with intensity 0, i, j)"""
    i, j = window_cells(case)
    a, b, c, d = (float(v) for v in plane_in_grid_frame(case, mutant))
    half = 0.0 if mutant == "cell_corner" else 0.5
    res = float(case["res"])
    x = (float(case["boundary"][0][0]) + (i.astype(np.float64) + half) * res) - mo.PCD_ORIGIN_OFFSET[0]
    y = (float(case["boundary"][1][0]) + (j.astype(np.float64) + half) * res) - mo.PCD_ORIGIN_OFFSET[1]
    t = a * x
    t = t + b * y
    t = t + d
    z = (t if mutant == "z_sign" else -t) / c
    return np.stack([x, y, z, np.zeros_like(x)]), i, j


def colour_image(case, v):
    """view v's source as the colour image of the projection size that the reference's mapper would have received"""
    src, kind = case["sources"][v], case["kind"]
    if kind == "rgb":
        return src
    if kind == "classmap":
        return mo.semantic_image_from_labels(src, case["img_h"], case["img_w"], case["palette"])
    labels = plr.full_labels(np.asarray(src), case["net"][0], case["net"][1], case["min_margin"])
    return mo.semantic_image_from_labels(labels, case["img_h"], case["img_w"], case["palette"])


def class_bits(case, label):
    """uint32 [m]: bit i where the colour label [3, m] matches map class i on R and G (src/mapping.py:419)"""
    bits = np.zeros(label.shape[1], dtype=np.uint32)
    for i, col in enumerate(case["colours"]):
        bits |= ((label[0] == col[0]) & (label[1] == col[1])).astype(np.uint32) << np.uint32(i)
    return bits


def class_mask(case):
    return sum(1 << i for i, n in enumerate(case["names"]) if n in case["classes"])


def real_depth(case, v):
    """rule 3's buffer of view v: from the real cloud (in the grid's frame), with the cloud's own range"""
    pr = occ.Projection(case["cloud"], case["P"][v], case["img_w"], case["img_h"], range_max=CLOUD_RANGE, frame_id=case["frame"],
                        pose7=case["pose7"])
    return occ.depth_buffer(np.where(pr.cand, pr.ix, 0), np.where(pr.cand, pr.iy, 0), pr.cand, pr.key32(), case["img_w"], case["img_h"],
                            case["occl"]["s"])[0]


def culled_cells(case, depth, ix, iy, cand, p2, mutant=None):
    """rule 3 -> bool [n], and bool [n]: candidates whose neighbourhood holds no real point"""
    o = case["occl"]
    s, R, k, abs_ = o["s"], o["R"], 1.0 + float(o["rel"]), float(o["abs_"])
    Hc, Wc = depth.shape
    with np.errstate(all="ignore"):
        key = p2.astype(np.float32)
        valid = cand & np.isfinite(key) & (key > 0)
    culled, empty = np.zeros(len(cand), dtype=bool), np.zeros(len(cand), dtype=bool)
    for n in np.nonzero(valid)[0]:
        cx, cy = int(ix[n]) // s, int(iy[n]) // s
        m = depth[max(cy - R, 0):min(cy + R, Hc - 1) + 1, max(cx - R, 0):min(cx + R, Wc - 1) + 1].min()
        empty[n] = m == occ.EMPTY
        md = float(np.array([m], dtype=np.uint32).view(np.float32)[0])          # 0xFFFFFFFF is a NaN: the comparison below is false
        prod = md * k
        culled[n] = float(key[n]) > prod + abs_
        if mutant == "empty_culls" and empty[n]:
            culled[n] = True
    return culled, empty


def apply_direct(grid, i, j, bits, cm):
    """rule 5 written out for cells known by index: class i ascending, every addition rounded to the grid's type"""
    for c in range(cm.shape[0]):
        sel = (bits >> np.uint32(c)) & np.uint32(1) == 1
        grid[i[sel], j[sel], :] += cm[:, c].reshape(1, -1)


def expected(case, grid0, mutant=None, stats=None, direct=False):
    """-> (the grid after the fill, dict of per-view counts).  The votes are applied by the oracle's update_map; with a mutant, or
    with `direct`, by apply_direct on the cells' own indices (a mutant's points need not lie in their cells).  `stats` (a dict)
    receives what test_ground_fill_cpu.py asserts of a case: candidates, cells cut by the fill's range, votes the class mask
    removed, culled cells, candidates with an empty neighbourhood, cells with votes of several views"""
    assert mutant is None or mutant in MUTANTS
    grid = np.array(grid0, copy=True)
    if mutant == "round_once":
        grid = grid.astype(np.float64)
    pcd, ci, cj = virtual_cloud(case, mutant)
    V = len(case["P"])
    cm = np.asarray(case["cm"], dtype=np.float64) * float(case["weight"])
    mask_bits = np.uint32((1 << case["C"]) - 1 if mutant == "class_mask_ignored" else class_mask(case))
    rng_max = CLOUD_RANGE if mutant == "cloud_range" else case["range_max"]
    T_vb = mo.velodyne_to_baselink()
    counts = dict(filled=[0] * V, culled=[0] * V, abstained=[0] * V)
    st = dict(candidates=np.zeros(pcd.shape[1], dtype=bool), range_cut=0, masked_votes=0, culled=0, empty=0, multi=0)
    votes = np.zeros(pcd.shape[1], dtype=np.int64)
    for v in (range(V - 1, -1, -1) if mutant == "views_reversed" else range(V)):
        image = colour_image(case, v)
        masked, label, ixy, cand = mo.project_pcd(pcd, case["frame"], image, case["pose7"], case["P"][v], rng_max, T_vb, return_debug=True)
        wide = mo.project_pcd(pcd, case["frame"], image, case["pose7"], case["P"][v], CLOUD_RANGE, T_vb, return_debug=True)[3]
        st["candidates"] |= cand
        st["range_cut"] += int((wide & ~cand).sum())
        keep = np.ones(pcd.shape[1], dtype=bool)
        if case["occl"] is not None:
            pr = occ.Projection(pcd, case["P"][v], case["img_w"], case["img_h"], range_max=rng_max, frame_id=case["frame"], pose7=case["pose7"])
            assert np.array_equal(pr.cand, cand)
            culled, empty = culled_cells(case, real_depth(case, v), ixy[0], ixy[1], cand, pr.p2, mutant)
            keep = ~culled
            counts["culled"][v] = int(culled.sum())
            st["culled"] += int(culled.sum())
            st["empty"] += int(empty.sum())
        if case["kind"] == "logits":
            ny = plr.nearest_index(np.where(cand, ixy[1], 0), case["net"][0], case["img_h"])
            nx = plr.nearest_index(np.where(cand, ixy[0], 0), case["net"][1], case["img_w"])
            state = plr.rule(np.asarray(case["sources"][v]), case["net"][0], case["net"][1], ny, nx, case["min_margin"])[0]
            counts["abstained"][v] = int(((state == plr.ABSTAINED) & cand & keep).sum())
        sel = keep[cand]
        masked, label = masked[:, sel], np.array(label[:, sel], copy=True)
        bits = class_bits(case, label)
        st["masked_votes"] += int(((bits & ~mask_bits) != 0).sum())
        label[:, (bits & ~mask_bits) != 0] = 0                               # a class the mask excludes casts no vote: no colour
        bits &= mask_bits
        counts["filled"][v] = int((bits != 0).sum())
        votes[np.nonzero(cand)[0][sel]] += bits != 0
        if mutant is None and not direct:
            mo.update_map(grid, masked, label, case["boundary"], case["res"], case["names"], case["colours"], cm, False)
        else:
            idx = np.nonzero(cand)[0][sel]
            apply_direct(grid, ci[idx], cj[idx], bits, cm)
    st["multi"] = int((votes > 1).sum())
    st["candidates"] = int(st["candidates"].sum())
    st["cells"] = pcd.shape[1]
    if stats is not None:
        stats.update(st)
    return grid.astype(np.asarray(grid0).dtype), counts
