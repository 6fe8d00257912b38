"""The scrolling grid (MAPPING.SCROLL) without a GPU: scroll.py's geometry against the rule restated in _scroll_reference.py, the
tile-job tables of a scroll (every destination once, leaving and entering complete) executed in NumPy against the same shift on one
big array, the emptiness flags, the host-side validator, the site file, the conditions the end-to-end drive must meet so that the
GPU test cannot pass on a drive that never scrolls, and avl_tile_copy's argument errors through the real library."""
import ctypes as C
import io
import math

import numpy as np
import pytest

import _scroll_reference as ref

SHIFTS = [(0, 1), (-1, 0), (1, -2), (6, 0), (9, -5)]
LAYERS = [(40, 0), (12, 0), (4, 0x7FFFFFFF)]


def scroll():
    from vision_semantic_segmentation_amd import scroll as s
    return s


# ------------------------------------------------------------------------------------------------ geometry
def test_config_defaults():
    from vision_semantic_segmentation_amd import get_cfg_defaults
    sc = get_cfg_defaults().MAPPING.SCROLL
    assert (sc.ENABLED, sc.TILE_M, sc.HYSTERESIS_TILES, sc.POOL_CHUNK_TILES) == (False, 10.0, 1, 64)


def test_vehicle_cell_floors_on_both_sides_of_the_anchor():
    s = scroll()
    anchor = (ref.OFFSET[0] + 3.0, ref.OFFSET[1] - 2.0)
    for x, y in [(3.05, -2.0), (2.95, -2.05), (-7.3, 11.9), (3.0, -2.5), (1.0e4, -1.0e4)]:
        pose = ref.yaw_pose(x, y, 0.3)
        assert s.vehicle_cell(pose, anchor, 0.1) == ref.vehicle_cell(pose, anchor, 0.1)
    assert s.vehicle_cell(ref.yaw_pose(2.95, -2.05, 0.0), anchor, 0.1) == (-1, -1)        # truncation would say (0, 0)
    assert s.vehicle_cell(ref.yaw_pose(float("nan"), 0.0, 0.0), anchor, 0.1) is None
    assert s.vehicle_cell(ref.yaw_pose(0.0, float("inf"), 0.0), anchor, 0.1) is None


def test_next_origin_hysteresis_first_call_and_limits():
    s = scroll()
    Ht, Wt, T = 6, 4, 8
    first = s.next_origin(None, (-3, 5), Ht, Wt, T, 1)
    assert first == ((-1 - 3) * T, (0 - 2) * T) == ref.next_origin(None, (-3, 5), Ht, Wt, T, 1)
    # a vehicle that oscillates across one tile edge never scrolls after the first call
    cur = s.next_origin(None, (7, 7), Ht, Wt, T, 1)
    for k in range(8):
        cell = (8, 7) if k % 2 == 0 else (7, 8)
        assert s.next_origin(cur, cell, Ht, Wt, T, 1) == cur
    # one that drifts two tiles away does, and then on both axes
    assert s.next_origin(cur, (15, 7), Ht, Wt, T, 1) == cur
    moved = s.next_origin(cur, (16, 9), Ht, Wt, T, 1)
    assert moved == ((2 - 3) * T, (1 - 2) * T) and moved != cur
    assert s.next_origin(cur, (7, -9), Ht, Wt, T, 1) == ((0 - 3) * T, (-2 - 2) * T)
    # a NaN pose: no scroll
    assert s.next_origin(cur, None, Ht, Wt, T, 1) == cur
    assert s.next_origin(None, None, Ht, Wt, T, 1) == (0, 0)
    # against the restatement on a random walk
    rng = np.random.default_rng(3)
    a, b = None, None
    cell = np.array([0, 0])
    for _ in range(300):
        cell = cell + rng.integers(-9, 10, 2)
        c = (int(cell[0]), int(cell[1]))
        a, b = s.next_origin(a, c, Ht, Wt, T, 1), ref.next_origin(b, c, Ht, Wt, T, 1)
        assert a == b
    # 2^30 is refused, just below is not
    lim = 1 << 30
    with pytest.raises(ValueError, match="2\\^30"):
        s.next_origin(None, (lim + Ht // 2 * T, 0), Ht, Wt, T, 1)
    with pytest.raises(ValueError, match="2\\^30"):
        s.next_origin(None, (0, -lim + Wt // 2 * T), Ht, Wt, T, 1)
    assert s.next_origin(None, (lim - T + Ht // 2 * T, 0), Ht, Wt, T, 1)[0] == lim - T


def test_window_boundary_is_the_stated_expression_to_the_bit():
    s = scroll()
    res, T, Hm, Wm = 0.1, 100, 2000, 1500
    anchor = (ref.OFFSET[0] - 100.0, ref.OFFSET[1] - 100.0)
    for ti in (-7, 0, 7):
        for tj in (7, -7):
            got = s.window_boundary(anchor, (ti * T, tj * T), Hm, Wm, res)
            x0 = anchor[0] + float(ti * T) * res
            y0 = anchor[1] + float(tj * T) * res
            assert got == [[x0, x0 + Hm * res], [y0, y0 + Wm * res]] == ref.window_boundary(anchor, (ti * T, tj * T), Hm, Wm, res)
            assert all(isinstance(v, float) for row in got for v in row)
    assert s.window_boundary(anchor, (0, 0), Hm, Wm, res)[0][0] == anchor[0]


def _cpu_mapping(boundary, res, tile_m, **kw):
    import torch
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = boundary
    cfg.MAPPING.RESOLUTION = res
    cfg.MAPPING.DEPTH_METHOD = kw.get("depth_method", "points_raw")
    cfg.MAPPING.SCROLL.ENABLED = kw.get("enabled", True)
    cfg.MAPPING.SCROLL.TILE_M = tile_m
    return SemanticMapping(cfg, device=torch.device("cpu"), logger=MyLogger("test", quiet=True))     # nothing is allocated before a frame


def test_construction_refuses_what_does_not_tile_and_names_the_numbers():
    with pytest.raises(ValueError, match="T = 6"):
        _cpu_mapping([[0.0, 24.0], [0.0, 12.0]], 0.5, 3.0)                 # T % 4 != 0
    with pytest.raises(ValueError, match="Hm = 44 x Wm = 32.*T = 8"):
        _cpu_mapping([[0.0, 22.0], [0.0, 16.0]], 0.5, 4.0)                 # Hm % T != 0
    with pytest.raises(ValueError, match="planar"):
        _cpu_mapping([[0.0, 24.0], [0.0, 16.0]], 0.5, 4.0, depth_method="planar")
    sm = _cpu_mapping([[0.0, 24.0], [0.0, 16.0]], 0.5, 4.0)
    assert (sm._scroll.T, sm._scroll.Ht, sm._scroll.Wt) == (8, 6, 4)
    assert sm.scroll_origin == (0, 0) and sm.scroll_count == 0 and sm.last_scroll is None
    with pytest.raises(RuntimeError, match="multi-GPU site map is out of scope"):
        sm.global_map()
    off = _cpu_mapping([[0.0, 22.0], [0.0, 16.0]], 0.5, 3.0, enabled=False)           # off: nothing is checked, nothing exists
    assert off._scroll is None
    with pytest.raises(RuntimeError, match="MAPPING.SCROLL.ENABLED is False"):
        off.scroll_to(ref.yaw_pose(0.0, 0.0, 0.0))


def test_the_frames_fast_path_is_next_origin():
    """scroll_to answers "no scroll" from two quotients and the hysteresis band; that must be next_origin's verdict for every pose,
    on cell and tile edges too (no GPU: the store is put at an origin by hand and only asked about poses that do not move it)"""
    s = scroll()
    sm = _cpu_mapping([[0.0, 24.0], [0.0, 16.0]], 0.1, 2.0)
    st = sm._scroll
    st.origin, st.first = (40, -20), False
    st._set_band()
    rng = np.random.default_rng(0)
    inside = 0
    for k in range(20000):
        x, y = rng.uniform(-1360.0, -1345.0), rng.uniform(-562.0, -552.0)
        if k % 3 == 0:
            x = round(x, 1)
        if k % 5 == 0:
            y = round(y * 0.5, 0) * 2.0
        pose = ref.yaw_pose(x, y, 0.0)
        stays = s.next_origin(st.origin, s.vehicle_cell(pose, st.anchor, st.res), st.Ht, st.Wt, st.T, st.hysteresis) == st.origin
        assert stays == (ref.next_origin(st.origin, ref.vehicle_cell(pose, st.anchor, st.res), st.Ht, st.Wt, st.T, st.hysteresis) == st.origin)
        b = st.band
        fast = b[0] <= (x + ref.OFFSET[0] - st.anchor[0]) / st.res < b[1] and b[2] <= (y + ref.OFFSET[1] - st.anchor[1]) / st.res < b[3]
        assert fast == stays, (x, y)
        if stays:
            inside += 1
            assert sm.scroll_to(pose) is False and sm.scroll_count == 0
    assert 2000 < inside < 18000
    assert sm.scroll_to(ref.yaw_pose(float("nan"), -556.0, 0.0)) is False


# ------------------------------------------------------------------------------------------------ job tables
T4, HT, WT, CHUNK = 4, 6, 4, 5
OLD = (2, -1)


def TableCase(shift, bpc, fill):
    return ref.TableCase(shift, bpc, fill, T4, HT, WT, CHUNK, OLD)


@pytest.mark.parametrize("shift", SHIFTS, ids=["%d_%d" % s for s in SHIFTS])
def test_every_destination_once_leaving_and_entering_complete(shift):
    s = scroll()
    case = TableCase(shift, 40, 0)
    plan = case.plan
    old_tiles, new_tiles = set(s.window_tiles(OLD, HT, WT)), set(s.window_tiles(case.new, HT, WT))
    dst_tiles = [t for t, _ in plan["dst"]]
    assert len(dst_tiles) == len(set(dst_tiles)) == HT * WT and set(dst_tiles) == new_tiles
    entering = {t for t, kind in plan["dst"] if kind != "overlap"}
    assert set(plan["leaving"]) == old_tiles - new_tiles and len(plan["leaving"]) == len(set(plan["leaving"]))
    assert entering == new_tiles - old_tiles and not entering & set(plan["leaving"])
    assert {t for t, kind in plan["dst"] if kind == "load"} == set(case.stored) and case.stored
    assert any(kind == "fill" for _, kind in plan["dst"])
    if abs(shift[0]) >= HT or abs(shift[1]) >= WT:
        assert not any(kind == "overlap" for _, kind in plan["dst"]) and len(plan["leaving"]) == HT * WT      # a jump: the same code
    dsts = [(j.dst, j.dst_off) for j in case.jobs]
    assert len(dsts) == len(set(dsts)) == len(plan["leaving"]) + HT * WT
    s.validate_jobs(case.jobs, case.extents, T4, 40, len(plan["leaving"]))


@pytest.mark.parametrize("bpc,fill", LAYERS, ids=["40", "12", "4_max"])
@pytest.mark.parametrize("shift", SHIFTS, ids=["%d_%d" % s for s in SHIFTS])
def test_executed_table_equals_the_shift_on_a_big_array(shift, bpc, fill):
    s = scroll()
    case = TableCase(shift, bpc, fill)
    s.validate_jobs(case.jobs, case.extents, T4, bpc, len(case.plan["leaving"]))
    flags = ref.execute_jobs(case.jobs, case.bufs, T4, bpc, fill, len(case.plan["leaving"]))
    want = case.site.view((case.new[0] * T4, case.new[1] * T4), case.Hm, case.Wm)
    assert np.array_equal(case.bufs["new"].reshape(case.Hm, case.Wm, bpc), want)
    slab = T4 * T4 * bpc
    for t, k in zip(case.plan["leaving"], case.fresh):
        key, off, _ = s.slab_ref(k, CHUNK, T4, bpc)
        assert np.array_equal(case.bufs[key][off:off + slab], case.site.tile(t).reshape(-1)), t
    assert np.array_equal(flags, case.want_flags())
    assert 0 < flags.sum() < flags.size                             # some leaving tile is empty, some is not
    # the encoded records carry the addresses the validator saw
    rec = np.zeros(len(case.jobs), dtype=s.JOB_DTYPE)
    assert s.JOB_DTYPE.itemsize == 40 and s.encode_jobs(case.jobs, case.extents, rec) == len(case.jobs)
    k = next(i for i, j in enumerate(case.jobs) if j.src is None)
    assert rec["src"][k] == 0 and rec["dst"][k] == case.extents["new"][0] + case.jobs[k].dst_off and rec["flag"][k] == -1


def test_flags_see_the_last_word_and_a_negative_zero():
    s = scroll()
    T, bpc = 4, 40
    slab = T * T * bpc
    bufs = {"w": np.zeros(3 * slab, dtype=np.uint8), ("chunk", 0): np.full(3 * slab, 0xAB, dtype=np.uint8)}
    bufs["w"][slab - 1] = 1                                                         # tile 0: only its last word
    bufs["w"][slab + 80:slab + 88] = np.frombuffer(np.float64(-0.0).tobytes(), dtype=np.uint8)   # tile 1: one -0.0
    jobs = [s.Job("w", k * slab, T * bpc, ("chunk", 0), k * slab, T * bpc, k) for k in range(3)]
    assert ref.execute_jobs(jobs, bufs, T, bpc, 0, 3).tolist() == [1, 1, 0]


def test_validator_refuses_a_job_past_its_buffer_and_a_misaligned_pitch():
    s = scroll()
    case = TableCase((1, -2), 40, 0)
    n = len(case.plan["leaving"])
    s.validate_jobs(case.jobs, case.extents, T4, 40, n)
    k = next(i for i, j in enumerate(case.jobs) if j.dst == "new")
    row = case.Wm * 40
    bad = list(case.jobs)
    bad[k] = case.jobs[k]._replace(dst_off=(case.Hm - T4 + 1) * row)               # one row past the window buffer
    with pytest.raises(ValueError, match="leave buffer 'new'"):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    bad[k] = case.jobs[k]._replace(dst_pitch=row + 8)
    with pytest.raises(ValueError, match="pitch"):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    bad[k] = case.jobs[k]._replace(dst_off=case.jobs[k].dst_off + 8)
    with pytest.raises(ValueError, match="16-byte aligned"):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    bad[k] = case.jobs[k]._replace(dst_off=-row)
    with pytest.raises(ValueError, match="leave buffer"):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    other = next(i for i, j in enumerate(case.jobs) if j.dst == "new" and i != k)
    bad[k] = case.jobs[k]._replace(dst_off=case.jobs[other].dst_off)
    with pytest.raises(ValueError, match="appears twice"):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    bad[k] = case.jobs[k]._replace(src="new", src_off=0, src_pitch=row)
    with pytest.raises(ValueError, match="read and written"):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    bad = list(case.jobs)
    bad[0] = case.jobs[0]._replace(flag=n)
    with pytest.raises(ValueError, match="flag %d of %d" % (n, n)):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    last = max(i for i, j in enumerate(case.jobs) if isinstance(j.src, tuple))
    j = case.jobs[last]
    bad = list(case.jobs)
    bad[last] = j._replace(src_off=case.extents[j.src][1] - T4 * T4 * 40 + 16)     # a slab that ends 16 bytes past its chunk
    with pytest.raises(ValueError, match="leave buffer"):
        s.validate_jobs(bad, case.extents, T4, 40, n)
    with pytest.raises(ValueError, match="bytes_per_cell"):
        s.validate_jobs(case.jobs, case.extents, T4, 6, n)


def test_a_table_of_one_kind_is_refused_as_the_other():
    """one validator, two modes: a copy table's fill job has no source for a merge, and only a merge table has half-row sources"""
    import _site_merge_reference as mref
    s = scroll()
    case = TableCase((1, -2), 40, 0)
    n = len(case.plan["leaving"])
    s.validate_jobs(case.jobs, case.extents, T4, 40, n)
    k = next(i for i, j in enumerate(case.jobs) if j.src is None)
    with pytest.raises(ValueError, match="merge job %d has no source" % k):
        s.validate_jobs(case.jobs, case.extents, T4, 40, n, merge=True)
    half = mref.MergeCase("ADD_F32_TO_F64", 4, 40, 0)
    s.validate_jobs(half.jobs, half.extents, 4, 40, half.n_flags, 20, merge=True)
    with pytest.raises(ValueError, match="tile jobs: a source of 20 bytes per cell"):
        s.validate_jobs(half.jobs, half.extents, 4, 40, half.n_flags, 20, merge=False)
    with pytest.raises(ValueError, match="tile job 0: src pitch 80 is misaligned or shorter than a tile row of 160"):
        s.validate_jobs(half.jobs, half.extents, 4, 40, half.n_flags)      # the same table read as a copy's: full rows


def test_job_record_is_the_struct_and_a_copy_table_encodes_a_zero_last_word():
    """_lib.AvlTileJob and JOB_DTYPE are struct avl_tile_job field by field, and encode_jobs writes a copy table as 40-byte records
    whose bytes follow from the jobs' fields alone: address = buffer base + offset (0 for a fill), the pitches, the flag, then 0."""
    import struct
    from vision_semantic_segmentation_amd import _lib
    s = scroll()
    names = ["src", "src_pitch", "dst", "dst_pitch", "flag", "fresh"]
    assert [f[0] for f in _lib.AvlTileJob._fields_] == names == list(s.JOB_DTYPE.names)
    for name, offset, size in zip(names, [0, 8, 16, 24, 32, 36], [8, 8, 8, 8, 4, 4]):
        field = getattr(_lib.AvlTileJob, name)
        assert (field.offset, field.size) == (offset, size) == (s.JOB_DTYPE.fields[name][1], s.JOB_DTYPE.fields[name][0].itemsize), name
    assert C.sizeof(_lib.AvlTileJob) == s.JOB_DTYPE.itemsize == 40 and s.JOB_DTYPE.fields["fresh"][1] == 36
    assert s.Job("a", 0, 16, "b", 0, 16, -1).fresh == 0                                  # the default: every copy job
    case = TableCase((1, -2), 40, 0)
    assert any(j.src is None for j in case.jobs) and any(j.flag >= 0 for j in case.jobs) and all(j.fresh == 0 for j in case.jobs)
    rec = np.full(len(case.jobs) + 1, 0xAB, dtype=np.uint8).repeat(40).view(s.JOB_DTYPE)  # garbage first: every byte is written
    assert s.encode_jobs(case.jobs, case.extents, rec) == len(case.jobs)
    want = b"".join(struct.pack("<QqQqii", 0 if j.src is None else case.extents[j.src][0] + j.src_off, j.src_pitch,
                                case.extents[j.dst][0] + j.dst_off, j.dst_pitch, j.flag, 0) for j in case.jobs)
    assert rec[:len(case.jobs)].tobytes() == want
    assert rec["fresh"][:len(case.jobs)].tolist() == [0] * len(case.jobs) and rec[len(case.jobs):].tobytes() == b"\xab" * 40


def test_site_file_round_trips():
    s = scroll()
    rng = np.random.default_rng(5)
    T = 8
    layers = {"map": (np.array([[-2, 3], [0, 0], [5, -1]]), rng.normal(size=(3, T, T, 5))),
              "elev_cnt": (np.zeros((0, 2), dtype=np.int64), np.zeros((0, T, T), dtype=np.int32))}
    arrays = s.pack_site((1.5, -2.25), 0.5, T, 5, "f64", layers)
    f = io.BytesIO()
    np.savez_compressed(f, **arrays)
    f.seek(0)
    with np.load(f) as data:
        meta, got = s.unpack_site(data, (1.5, -2.25), 0.5, T, 5, "f64")
        assert meta == {"anchor": (1.5, -2.25), "resolution": 0.5, "T": T, "C": 5, "dtype": "f64"}
        assert sorted(got) == ["elev_cnt", "map"]
        for name in layers:
            assert np.array_equal(got[name][0], layers[name][0]) and np.array_equal(got[name][1], layers[name][1])
            assert got[name][1].dtype == layers[name][1].dtype
        for kw in ({"T": 4}, {"resolution": 0.25}, {"C_": 4}, {"dtype": "f32"}):
            with pytest.raises(ValueError, match="site file"):
                s.unpack_site(data, **kw)


# ------------------------------------------------------------------------------------------------ the drive reaches every branch
def test_the_drive_reaches_every_branch():
    s = scroll()
    d = ref.main_drive()
    assert 14 <= len(d.poses) <= 20
    stats = {}
    site = d.numpy_site(np.eye(5), stats=stats)
    moves = [(k, o) for k, (o, moved) in enumerate(d.origins) if moved]
    assert len(moves) >= 5
    prev, shifts = (0, 0), []
    for k, (o, moved) in enumerate(d.origins):
        if moved:
            shifts.append((k, ((o[0] - prev[0]) // d.T, (o[1] - prev[1]) // d.T)))
        prev = o
    later = [sh for k, sh in shifts if k > 0]
    assert any(a != 0 and b == 0 for a, b in later) and any(a == 0 and b != 0 for a, b in later)        # a scroll on each axis
    assert any(a != 0 and b != 0 and abs(a) < d.Ht and abs(b) < d.Wt for a, b in later)                 # a diagonal one
    assert any(abs(a) >= d.Ht or abs(b) >= d.Wt for a, b in later)                                      # a jump with no overlap
    # the same origins from scroll.py's own functions
    cur, first = (0, 0), True
    for p, (o, _) in zip(d.poses, d.origins):
        cur = s.next_origin(None if first else cur, s.vehicle_cell(p, d.anchor, d.res), d.Ht, d.Wt, d.T, d.hysteresis)
        first = False
        assert cur == o
    # replay the store in tiles: what leaves non-empty is stored; a tile re-enters non-empty and a later frame adds to it
    nonempty_after = []                      # per frame: the site's non-empty tiles after it
    partial = ref.BigSite(d.tile_rect, d.T, (5,), np.float64)
    for k in range(len(d.poses)):
        view = partial.view(d.origins[k][0], d.Hm, d.Wm)
        view[stats["changed"][k]] = 1.0
        nonempty_after.append(set(partial.nonempty_tiles()))
    reentered_and_added, empty_leaving = False, False
    prev = (0, 0)
    for k, (o, moved) in enumerate(d.origins):
        if moved:
            have = nonempty_after[k - 1] if k else set()
            old_tiles, new_tiles = set(s.window_tiles((prev[0] // d.T, prev[1] // d.T), d.Ht, d.Wt)), set(s.window_tiles((o[0] // d.T, o[1] // d.T), d.Ht, d.Wt))
            empty_leaving = empty_leaving or (k > 0 and bool((old_tiles - new_tiles) - have))
            for t in (new_tiles - old_tiles) & have:
                a, b = t[0] * d.T - o[0], t[1] * d.T - o[1]
                for kk in range(k, len(d.poses)):
                    if d.origins[kk][0] != o:
                        break
                    reentered_and_added = reentered_and_added or bool(stats["changed"][kk][a:a + d.T, b:b + d.T].any())
        prev = o
    assert reentered_and_added and empty_leaving
    assert max(stats["outside"]) > 0                                               # points that would vote fall outside the window
    cells = [ref.vehicle_cell(p, d.anchor, d.res) for p in d.poses]
    assert any(c[0] < 0 for c in cells) and any(c[1] < 0 for c in cells)
    assert len(site.nonempty_tiles()) > d.Ht * d.Wt                                # the site outgrew the window


# ------------------------------------------------------------------------------------------------ the ABI
def test_tile_copy_argument_errors_do_not_need_a_gpu():
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.AvlTileJob) == 40 == scroll().JOB_DTYPE.itemsize
    jobs = (_lib.AvlTileJob * 2)()
    flags = (C.c_int32 * 4)()
    p, fl = C.cast(jobs, C.c_void_p), C.cast(flags, C.c_void_p)
    for args, word in [((None, 2, 4, 40, 0, fl, 4, None), "jobs_dev is NULL"),
                       ((p, 2, 4, 40, 0, fl, -1, None), "n_flags"),
                       ((p, 2, 4, 6, 0, fl, 4, None), "bytes_per_cell"),
                       ((p, 2, 4, 0, 0, fl, 4, None), "bytes_per_cell"),
                       ((p, 2, 4, 132, 0, fl, 4, None), "bytes_per_cell"),
                       ((p, 2, 2, 12, 0, fl, 4, None), "multiple of 16"),
                       ((p, 2, 0, 40, 0, fl, 4, None), "tile_cells"),
                       ((p, -1, 4, 40, 0, fl, 4, None), "n_jobs"),
                       ((p, 2, 4, 40, 0, None, 4, None), "flags is NULL")]:
        assert L.avl_tile_copy(*args) == -1, word
        assert word in _lib.last_error(), (word, _lib.last_error())
