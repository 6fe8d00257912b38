"""Merging sites on the GPU.

* k_tile_merge against the NumPy executor of _site_merge_reference.py, every written byte compared: the tables of
  test_site_merge_cpu.py (window tiles in place, stored slabs in place, fresh slabs over 0xAB garbage; -0.0, an exact negation, a
  last-word-only result, denormals, infinities and NaN, integer wrap, min / max against their fills) for every op at T = 4 and for
  rows of 4000 bytes at T = 100, every buffer and the flags between guard strips of 0xAB that must survive;
* merge_site end to end: two _scroll_reference.Drives play two vehicles, the second one's saved site is merged into the first one's
  map, and site_tiles() / site_map() equal the NumPy sum of the two numpy_sites keyed by tile, bit for bit (identity and log
  confusion matrix on f64, f32, once with the elevation layer); the left-fold order, a cancelling file, frames and scrolls after a
  merge, a refused file;
* global_site with two ranks on the one GPU under gloo."""
import ctypes as C
import os

import numpy as np
import pytest

import _scroll_reference as ref
import _site_merge_reference as mref

pytestmark = pytest.mark.gpu

GUARD = 256
AB32 = -0x54545455           # 0xABABABAB


# ------------------------------------------------------------------------------------------------ the kernel against the executor
def run_merge_on_device(case, device):
    """-> ({key: bytes after the launch, guards included}, flags with guards): case.jobs through validate_jobs, encode_jobs and
    avl_tile_merge, every buffer of case.bufs between two guard strips of 0xAB"""
    import torch
    from vision_semantic_segmentation_amd import _lib, scroll as s
    dev, extents = {}, {}
    for key, host in case.bufs.items():
        t = torch.full((GUARD + host.size + GUARD,), 0xAB, dtype=torch.uint8, device=device)
        t[GUARD:GUARD + host.size] = torch.from_numpy(host).to(device)
        dev[key] = t
        extents[key] = (t.data_ptr() + GUARD, int(host.size))
    s.validate_jobs(case.jobs, extents, case.T, case.bpc, case.n_flags, case.src_bpc, merge=True)
    rec = np.zeros(len(case.jobs), dtype=s.JOB_DTYPE)
    s.encode_jobs(case.jobs, extents, rec)
    table = torch.from_numpy(rec.view(np.uint8)).to(device)
    flags = torch.full((16 + case.n_flags + 16,), AB32, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = _lib.lib().avl_tile_merge(C.c_void_p(table.data_ptr()), len(case.jobs), mref.OPS[case.op], case.T, case.bpc, case.fill,
                                   C.c_void_p(flags.data_ptr() + 64), case.n_flags, C.c_void_p(stream))
    _lib.check(rc, "avl_tile_merge")
    torch.cuda.synchronize(device)
    return {k: t.cpu().numpy() for k, t in dev.items()}, flags.cpu().numpy()


def check_merge(case, device):
    got, got_flags = run_merge_on_device(case, device)
    want, want_flags = case.want()
    for key, w in want.items():
        g = got[key]
        assert (g[:GUARD] == 0xAB).all() and (g[-GUARD:] == 0xAB).all(), "guard strip of %r written" % (key,)
        if key == "stage":
            assert np.array_equal(g[GUARD:-GUARD], w), "the source was written"
        else:
            assert mref.same_bits_or_both_nan(g[GUARD:-GUARD], w, case.element), "%r: %d bytes differ" % (key, int((g[GUARD:-GUARD] != w).sum()))
    assert (got_flags[:16] == AB32).all() and (got_flags[-16:] == AB32).all(), "guard of the flags written"
    assert np.array_equal(got_flags[16:16 + case.n_flags], want_flags)
    assert want_flags.tolist() == [0, 1, 1, 1, 0, 1, 1]            # the negated tile and the -0.0 (fill) tile come out empty
    if np.issubdtype(case.element, np.floating):
        assert np.isnan(want["window"].view(case.element)).any() and np.isinf(want["window"].view(case.element)).any()


@pytest.mark.parametrize("op,bpc,fill", mref.CASES, ids=["%s_%d" % (c[0], c[1]) for c in mref.CASES])
def test_tile_merge_small_tiles(op, bpc, fill, cuda_device):
    check_merge(mref.MergeCase(op, 4, bpc, fill), cuda_device)


@pytest.mark.parametrize("op", ["ADD_F64", "ADD_F32_TO_F64"])
def test_tile_merge_rows_of_4000_bytes(op, cuda_device):
    check_merge(mref.MergeCase(op, 100, 40, 0), cuda_device)


def test_tile_merge_without_jobs_only_zeroes_the_flags(cuda_device):
    import torch
    from vision_semantic_segmentation_amd import _lib
    flags = torch.full((8,), 7, dtype=torch.int32, device=cuda_device)
    rc = _lib.lib().avl_tile_merge(None, 0, 0, 4, 40, 0, C.c_void_p(flags.data_ptr() + 8), 4, C.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream))
    _lib.check(rc, "avl_tile_merge")
    assert flags.cpu().tolist() == [7, 7, 0, 0, 0, 0, 7, 7]


# ------------------------------------------------------------------------------------------------ merge_site end to end
_DRIVES = {}


def drives():
    if not _DRIVES:
        _DRIVES["a"], _DRIVES["b"] = ref.main_drive(), mref.second_drive()
    return _DRIVES["a"], _DRIVES["b"]


def np_dtype(grid_dtype):
    return np.float64 if grid_dtype == "f64" else np.float32


def map_op(grid_dtype):
    return "ADD_F64" if grid_dtype == "f64" else "ADD_F32"


def two_maps(device, grid_dtype, cm, elevation=False):
    """-> (the first vehicle's map after its drive, the second one's, their NumPy sites keyed by tile)"""
    from test_gpu_scroll import make_sm, run_frames
    a, b = drives()
    maps = []
    for d in (a, b):
        sm = make_sm(d, device, grid_dtype, cm, elevation=elevation)
        if elevation:
            sm.set_ground_plane([0.0, 0.0, 1.0, 1.9])
        run_frames(sm, d, range(len(d.poses)))
        maps.append(sm)
    sites = [mref.tiles_of(d.numpy_site(maps[0].confusion_matrix, np_dtype(grid_dtype))) for d in (a, b)]
    return maps[0], maps[1], sites[0], sites[1]


def site_arrays(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def with_a_tile_of_minus_zero(arrays, tile):
    """the site arrays plus one map tile that holds nothing but -0.0: the sum turns it into +0.0, so it adds a slab and frees it"""
    out = dict(arrays)
    out["map_coords"] = np.concatenate([arrays["map_coords"], np.array([tile], dtype=np.int64)])
    out["map_tiles"] = np.concatenate([arrays["map_tiles"], np.full((1,) + arrays["map_tiles"].shape[1:], -0.0, dtype=arrays["map_tiles"].dtype)])
    return out


def check_tiles(sm, tiles, what=""):
    """site_tiles() and site_map() of ``sm`` against {tile: array}, by the bit-pattern rule and bit for bit"""
    from test_gpu_scroll import check_site
    some = mref.nonempty(tiles)
    first = next(iter(some.values()))
    check_site(sm, mref.big_site(some, first.shape[0], first.shape[2:], first.dtype), what)


@pytest.mark.parametrize("cm,grid_dtype", [("identity", "f64"), ("log", "f64"), ("log", "f32")], ids=["identity_f64", "log_f64", "log_f32"])
def test_merged_site_equals_the_numpy_sum(cm, grid_dtype, tmp_path, cuda_device):
    own, other, s_own, s_other = two_maps(cuda_device, grid_dtype, cm)
    path = os.path.join(str(tmp_path), "other.npz")
    other.save_site(path)
    far = (900, -900)
    file_tiles = dict(s_other)
    file_tiles[far] = np.full_like(next(iter(s_other.values())), -0.0)
    own.site_tiles()                                                 # retires the last scroll's flags: the directory is settled
    slabs_before = len(own._scroll.directory)
    rec = own.merge_site(with_a_tile_of_minus_zero(site_arrays(path), far))
    total = mref.sum_sites(s_own, [file_tiles], map_op(grid_dtype))
    assert far in total and far not in mref.nonempty(total)
    check_tiles(own, total, "%s %s" % (cm, grid_dtype))
    assert min(rec) > 0, rec                                         # window, store, added and freed: every branch ran
    assert rec.freed == 1 and rec.window + rec.store + rec.added == len(file_tiles)
    assert len(own._scroll.directory) == slabs_before + rec.added - rec.freed and far not in own._scroll.directory
    # the file itself is left alone and the other map too
    check_tiles(other, s_other, "the other map")


def test_merge_is_a_left_fold_and_takes_a_path(tmp_path, cuda_device):
    from vision_semantic_segmentation_amd import scroll as s
    own, other, s_own, s_other = two_maps(cuda_device, "f64", "log")
    path = os.path.join(str(tmp_path), "other.npz")
    other.save_site(path)
    rec = own.merge_site(path)
    assert rec.freed == 0 and rec.window > 0 and rec.store > 0 and rec.added > 0
    rng = np.random.default_rng(11)
    shared = sorted(set(s_own) & set(s_other))
    third = {t: rng.normal(size=s_own[t].shape) * 3.0 for t in shared[:4]}
    third[(-40, 33)] = rng.normal(size=s_own[shared[0]].shape)
    a, b = drives()
    arrays = s.pack_site(a.anchor, a.res, a.T, 5, "f64", {"map": (np.array(sorted(third)), np.stack([third[t] for t in sorted(third)]))})
    own.merge_site(arrays)
    fold = mref.sum_sites(s_own, [s_other, third])
    check_tiles(own, fold, "left fold")
    other_order = mref.sum_sites(s_own, [mref.sum_sites(s_other, [third])])
    assert any(not np.array_equal(fold[t], other_order[t]) for t in third)           # own + (B + C) is another number: the order is pinned


def test_a_cancelling_file_frees_the_slab_and_a_refused_file_changes_nothing(tmp_path, cuda_device):
    from vision_semantic_segmentation_amd import scroll as s
    own, other, s_own, s_other = two_maps(cuda_device, "f64", "log")
    a, b = drives()
    store = own._scroll
    own.site_tiles()                                                                  # retires the last scroll's flags
    stored = sorted(t for t in store.directory if t in s_own)
    t = stored[len(stored) // 2]
    slab = store.directory[t]
    before = own.site_map()[1].cpu().numpy()
    # refused: a tile named twice, another tile size, other layers -- the map is as it was
    twice = s.pack_site(a.anchor, a.res, a.T, 5, "f64", {"map": (np.array([t, (0, 0), t]), np.ones((3, a.T, a.T, 5)))})
    with pytest.raises(ValueError, match="twice"):
        own.merge_site(twice)
    with pytest.raises(ValueError, match="site file has T = 4"):
        own.merge_site(s.pack_site(a.anchor, a.res, 4, 5, "f64", {"map": (np.array([t]), np.ones((1, 4, 4, 5)))}))
    with pytest.raises(ValueError, match="layers"):
        own.merge_site(s.pack_site(a.anchor, a.res, a.T, 5, "f64", {"map": (np.array([t]), np.ones((1, a.T, a.T, 5))),
                                                                   "elev_cnt": (np.array([t]), np.ones((1, a.T, a.T), dtype=np.int32))}))
    assert np.array_equal(own.site_map()[1].cpu().numpy(), before) and store.directory[t] == slab and own.site_tiles() == sorted(s_own)
    # the exact negation of one stored tile: it leaves the site and its slab is free again
    rec = own.merge_site(s.pack_site(a.anchor, a.res, a.T, 5, "f64", {"map": (np.array([t]), -s_own[t][None])}))
    assert tuple(rec) == (0, 1, 0, 1)
    assert t not in own.site_tiles() and t not in store.directory and t not in store.nonempty and slab in store.free
    rest = {k: v for k, v in s_own.items() if k != t}
    check_tiles(own, rest, "cancelled")


def test_frames_and_scrolls_after_a_merge(tmp_path, cuda_device):
    from oracle import mapping_oracle as mo
    from test_gpu_scroll import check_site, run_frames
    own, other, s_own, s_other = two_maps(cuda_device, "f64", "log")
    path = os.path.join(str(tmp_path), "other.npz")
    other.save_site(path)
    own.merge_site(path)
    a, b = drives()
    total = mref.nonempty(mref.sum_sites(s_own, [s_other]))
    # a jump away, back over merged tiles of the window and the store, then the second vehicle's frame on tiles that the file added
    replay = [(a, 10), (a, 12), (b, 5)]
    origins, cur = [], a.origins[-1][0]
    for d, k in replay:
        new = ref.next_origin(cur, ref.vehicle_cell(d.poses[k], a.anchor, a.res), a.Ht, a.Wt, a.T, a.hysteresis)
        assert new != cur                                              # every replayed frame scrolls
        origins.append(new)
        cur = new
    ti, tj = [o[0] // a.T for o in origins], [o[1] // a.T for o in origins]
    site = mref.big_site(total, a.T, (5,), np.float64, cover=(min(ti), max(ti) + a.Ht - 1, min(tj), max(tj) + a.Wt - 1))
    added = set(s_other) - set(s_own)
    last = {(origins[-1][0] // a.T + i, origins[-1][1] // a.T + j) for i in range(a.Ht) for j in range(a.Wt)}
    assert added & last
    count = own.scroll_count
    for (d, k), origin in zip(replay, origins):
        run_frames(own, d, [k])
        assert own.scroll_origin == origin
        boundary = ref.window_boundary(a.anchor, origin, a.Hm, a.Wm, a.res)
        view = site.view(origin, a.Hm, a.Wm)
        for image, cam in zip(d.images[k], d.cams):
            mo.mapping_frame(view, d.clouds[k], "world", image, d.poses[k], cam.P, d.oracle_cfg(own.confusion_matrix, boundary))
    assert own.scroll_count == count + 3 and own.last_scroll["loaded"] > 0
    check_site(own, site, "after the merge")


def test_merge_with_the_elevation_layer(tmp_path, cuda_device):
    own, other, s_own, s_other = two_maps(cuda_device, "f64", "log", elevation=True)
    a, b = drives()
    T = a.T
    fills = [f for _, f in (mref.LAYER_OPS[n] for n in ("elev_sum", "elev_cnt", "elev_min", "elev_max"))]

    def elevation_tiles(sm):
        (i0, j0), arrays = sm.site_map(layer="elevation")
        out = []
        for arr, fill in zip(arrays, fills):
            arr = arr.cpu().numpy()
            tiles = {(i0 // T + i, j0 // T + j): arr[i * T:(i + 1) * T, j * T:(j + 1) * T].copy() for i in range(arr.shape[0] // T) for j in range(arr.shape[1] // T)}
            out.append(mref.nonempty(tiles, fill))
        return out
    e_own, e_other = elevation_tiles(own), elevation_tiles(other)
    assert all(e_own) and all(e_other) and set(e_own[1]) & set(e_other[1]) and set(e_other[1]) - set(e_own[1])
    path = os.path.join(str(tmp_path), "other.npz")
    other.save_site(path)
    rec = own.merge_site(path)
    assert rec.window > 0 and rec.store > 0 and rec.added > 0
    check_tiles(own, mref.sum_sites(s_own, [s_other]), "map with elevation")
    want = [mref.nonempty(mref.sum_sites(e_own[k], [e_other[k]], *mref.LAYER_OPS[name]), fills[k])
            for k, name in enumerate(("elev_sum", "elev_cnt", "elev_min", "elev_max"))]
    assert own.site_tiles("elevation") == sorted(set().union(*[set(w) for w in want]))
    got = elevation_tiles(own)
    for k in range(4):
        assert sorted(got[k]) == sorted(want[k]), k
        assert all(got[k][t].dtype == want[k][t].dtype and np.array_equal(got[k][t], want[k][t]) for t in want[k]), k
    shared = sorted(set(e_own[1]) & set(e_other[1]))[0]
    assert np.array_equal(got[1][shared], e_own[1][shared] + e_other[1][shared])                # counts add
    both = sorted(set(e_own[2]) & set(e_other[2]))[0]
    assert np.array_equal(got[2][both], np.minimum(e_own[2][both], e_other[2][both]))           # minima take the minimum


# ------------------------------------------------------------------------------------------------ global_site, two ranks
def _global_site_worker(rank, world, port, q):
    """One rank of test_global_site_two_ranks: rank r maps drive r, then global_site() -- plain, and with the float32 exchange on an
    identity-matrix and a log-matrix map"""
    import sys
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    except Exception as e:            # (port in use, ...): the parent must not wait for a result that never comes
        q.put(("error", rank, "rank %d: init_process_group: %r" % (rank, e)))
        raise
    try:
        from test_gpu_scroll import make_sm, run_frames
        dev = torch.device("cuda", 0)
        d = drives()[rank]
        out = {}
        for name, cm, exchange in (("plain", "log", None), ("identity32", "identity", torch.float32), ("log32", "log", torch.float32)):
            sm = make_sm(d, dev, "f64", cm)
            run_frames(sm, d, range(len(d.poses)))
            merged = sm.global_site(exchange_dtype=exchange)
            assert len(merged) == world and merged[0].added > 0 and merged[0].store == 0 and merged[1].store > 0
            assert sm.last_exchange[0] == "tiles" and sm.last_exchange[1] > 0
            assert sm.scroll_origin == (0, 0) and not bool(sm.map_dev.any())
            origin, site = sm.site_map()
            out[name] = (origin, site.cpu().numpy(), sm.site_tiles(), sm.last_exchange[1])
            with pytest.raises(RuntimeError, match="global_site\\(\\) has run"):
                sm.global_site()
        assert out["log32"][3] < 0.6 * out["plain"][3]                 # half the payload, but for the coordinates
        q.put(("ok", rank, out))
        dist.barrier()
    except Exception as e:
        import traceback
        q.put(("error", rank, "rank %d: %s" % (rank, traceback.format_exc(limit=5))))
        raise
    finally:
        dist.destroy_process_group()


def test_global_site_two_ranks(cuda_device):
    """The GPU box has one MI355X and RCCL refuses two ranks on one device, so the two ranks share cuda:0 and the collective is gloo's
    all-gather on the CUDA tensors (as test_gpu_e2e.test_two_ranks_hip_grids_through_a_collective)."""
    import queue
    import socket
    import torch.multiprocessing as mp
    from vision_semantic_segmentation_amd import synthetic as syn
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sock:            # a free port
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = [ctx.Process(target=_global_site_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        while len(results) < 2:
            status, rank, payload = q.get(timeout=240)    # a worker that dies puts ("error", ...) first; one that hangs runs into the timeout
            if status != "ok":
                raise RuntimeError(payload)
            results[rank] = payload
    except (queue.Empty, RuntimeError) as e:
        for p in procs:
            p.terminate()
        pytest.fail("no result from both ranks: %r (exit codes %r)" % (e, [p.exitcode for p in procs]))
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    a, b = drives()
    for name, cm, rounded in (("plain", syn.log_confusion(5), False), ("identity32", np.eye(5), True), ("log32", syn.log_confusion(5), True)):
        s0, s1 = (mref.tiles_of(d.numpy_site(cm)) for d in (a, b))
        if rounded:                                                    # the twin rounds each rank's tiles to float32 first
            r0, r1 = ({t: v.astype(np.float32) for t, v in s.items()} for s in (s0, s1))
            total = mref.sum_sites({}, [r0, r1], "ADD_F32_TO_F64")
        else:
            total = mref.sum_sites({}, [s0, s1])
        if name == "identity32":
            assert all(np.array_equal(total[t], mref.sum_sites({}, [s0, s1])[t]) for t in total)      # small integers: exact
        some = mref.nonempty(total)
        (i0, j0), want = mref.big_site(some, a.T, (5,), np.float64).region(sorted(some))
        for rank in (0, 1):
            origin, got, tiles, _ = results[rank][name]
            assert tiles == sorted(some), (name, rank)
            assert origin == (i0, j0) and got.dtype == want.dtype and got.shape == want.shape, (name, rank)
            assert np.array_equal(got, want), "%s rank %d: %d values differ" % (name, rank, int((got != want).sum()))
        assert np.array_equal(results[0][name][1], results[1][name][1])
