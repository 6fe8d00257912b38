#!/usr/bin/env python3
"""Times merging sites (SemanticMapping.merge_site; scroll.py, csrc/seg_sitemerge.hip) on the default 2000 x 2000 x 5 float64 window of
0.1 m cells with 10 m tiles (T = 100): a site of 3 x 3 windows (3600 tiles, 1.44 GB; 400 of them in the window, 3200 in the store)
receives a like site whose tiles are already on the device (what global_site merges; a site file adds its upload):

    overlap      every tile of the source meets a tile of the receiving site: 400 jobs in place in the window, 3200 in place in slabs
    disjoint     none does (the source lies 60 tiles further along x): 3600 fresh slabs, which the tool gives back after every call
    f32 source   overlap, the source tiles float32 (the exchange form: acc + (double)src)
    elevation    overlap, the elevation layer's four arrays (8 + 4 + 4 + 4 bytes per cell, four launches), no map tiles

each measured four ways in ONE process, alternating, `rounds` times over (every other round in reverse order):
    kernel   avl_tile_merge alone on the ready-made, validated, uploaded tables, between two device events;
    call     TileStore._merge, wall clock per call with a synchronisation behind each: planning, validation and encoding of the
             tables, their upload, the launches and the wait for the result flags (merge_site's own work behind its checks);
    copy     dst.copy_(src) of a tensor of HALF the bytes the kernel moves (source + destination read + destination write; a fresh
             job reads no destination), so that its read plus its write are as many bytes: the project's yardstick;
    parent   site_map() of both sites over their common rectangle and a torch add_ (for the elevation layer add_, add_, minimum,
             maximum): the only route the parent commit has -- it assembles both rectangles and cannot put the result back.
The f32 source has no parent route of its own.  merge_site() from host arrays (the file route) is timed once for `overlap`.

    python tools/bench_site_merge.py [--reps 5] [--warmup 2] [--rounds 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from vision_semantic_segmentation_amd import SemanticMapping, _lib, get_cfg_defaults, scroll as S, synthetic as syn  # noqa: E402
from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET  # noqa: E402
from vision_semantic_segmentation_amd.utils.logger import MyLogger  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda", 0)
RES, TILE_M, HALF = 0.1, 10.0, 100.0
ANCHOR = (PCD_ORIGIN_OFFSET[0] - HALF, PCD_ORIGIN_OFFSET[1] - HALF)
ELEV = [("elev_sum", torch.int64), ("elev_cnt", torch.int32), ("elev_min", torch.int32), ("elev_max", torch.int32)]


def pose_at(ti, tj):
    return np.array([ANCHOR[0] - PCD_ORIGIN_OFFSET[0] + (ti + 0.5) * TILE_M, ANCHOR[1] - PCD_ORIGIN_OFFSET[1] + (tj + 0.5) * TILE_M, 0.0, 0.0, 0.0, 0.0, 1.0])


def make_site(elevation=False, first_tile=0):
    """a site of 3 x 3 full windows whose first tile is (first_tile, 0)"""
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], HALF)
    cfg.MAPPING.RESOLUTION = RES
    cfg.MAPPING.DEPTH_METHOD = "points_raw"
    cfg.MAPPING.SCROLL.ENABLED = True
    cfg.MAPPING.SCROLL.TILE_M = TILE_M
    cfg.MAPPING.SCROLL.HYSTERESIS_TILES = 0
    cfg.MAPPING.ELEVATION.ENABLED = elevation
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    for a in range(3):
        for b in range(3):
            sm.scroll_to(pose_at(first_tile + 10 + 20 * a, 10 + 20 * b))
            sm.map_dev.fill_(1.0)
            if elevation:
                for t in sm.elevation_layer():
                    t.fill_(3)
    assert len(sm.site_tiles()) == 3600
    return sm


def stats(samples):
    return {"median_us": round(statistics.median(samples), 1), "min_us": round(min(samples), 1), "max_us": round(max(samples), 1)}


def event_time(fn, reps, after=None):
    out = []
    for k in range(args.warmup + reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= args.warmup:
            out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def wall_time(fn, reps, after=None):
    out = []
    for k in range(args.warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= args.warmup:
            out.append((time.perf_counter() - t0) * 1e6)
        if after is not None:
            after()
    return statistics.median(out)


def alternate(arms, reps):
    samples = {name: [] for name, _, _, _ in arms}
    for r in range(args.rounds):
        for name, fn, timer, after in (arms if r % 2 == 0 else arms[::-1]):
            samples[name].append(timer(fn, reps, after))
    return {name: stats(v) for name, v in samples.items()}


def ready_table(store, l, coords, src, src_bpc, slabs):
    """the merge table of layer ``l`` for the source tiles ``src`` at ``coords``, validated and uploaded -> (device table, jobs)"""
    L = store._layers()[l]
    T = store.T
    a, b = store.origin[0] // T, store.origin[1] // T
    entries = []
    for k, t in enumerate(coords):
        if a <= t[0] < a + store.Ht and b <= t[1] < b + store.Wt:
            entries.append((t, k, "window", None, k))
        elif t in store.directory:
            entries.append((t, k, "store", store.directory[t], k))
        else:
            entries.append((t, k, "fresh", slabs[t], k))
    jobs = S.merge_jobs(entries, T, store.Wm, L.bpc, store.chunk_tiles, (a, b), src_bpc)
    buffers = store._buffers(L, {"window": store._extent(L.get()), "stage": store._extent(src)})
    S.validate_jobs(jobs, buffers, T, L.bpc, len(coords), src_bpc, merge=True)
    rec = np.zeros(len(jobs), dtype=S.JOB_DTYPE)
    S.encode_jobs(jobs, buffers, rec)
    return torch.from_numpy(rec.view(np.uint8)).to(dev), jobs


def bench(name, sm, coords, layers, src_dtypes=None, parent=None):
    """``layers``: {layer name: CUDA tiles [n, T, T, ...]} of the source at ``coords`` (the other layers come without tiles)"""
    store = sm._scroll
    store.retire()
    T = store.T
    names = [L.name for L in store._layers()]
    empty = np.zeros((0, 2), dtype=np.int64)
    site = {}
    for L in store._layers():
        cur = L.get()
        site[L.name] = (np.array(coords, dtype=np.int64), layers[L.name]) if L.name in layers else \
            (empty, torch.empty((0, T, T) + tuple(cur.shape[2:]), dtype=cur.dtype, device=dev))
    tiles_of = store._check_site(site, src_dtypes)
    fresh = [t for t in coords if t not in store.directory and not (store.origin[0] // T <= t[0] < store.origin[0] // T + store.Ht and
                                                                   store.origin[1] // T <= t[1] < store.origin[1] // T + store.Wt)]
    st = torch.cuda.current_stream(dev)

    def give_back():                                           # the slabs a disjoint merge added: the next call adds them again
        for t in fresh:
            store.free.append(store.directory.pop(t))
            store.nonempty.pop(t, None)

    def call():
        return store._merge(site, tiles_of, st, src_dtypes)
    record = call()
    give_back()
    slabs = dict(zip(fresh, store._slabs(len(fresh))))
    tables, moved = [], 0
    for name_l, tiles in layers.items():
        l = names.index(name_l)
        L = store._layers()[l]
        src_bpc = L.bpc * tiles.element_size() // L.get().element_size()
        table, jobs = ready_table(store, l, coords, tiles.view(torch.uint8).reshape(-1), src_bpc, slabs)
        op = S.merge_op(name_l, store._dtype_name(), "f32" if tiles.dtype == torch.float32 and name_l == "map" else None)
        tables.append((table, len(jobs), op, L.bpc, L.fill))
        moved += sum(T * T * (src_bpc + L.bpc * (1 if j.fresh else 2)) for j in jobs)
    flags = torch.zeros(len(coords), dtype=torch.int32, device=dev)
    stream = C.c_void_p(st.cuda_stream)

    def kernel():
        for table, n, op, bpc, fill in tables:
            rc = _lib.lib().avl_tile_merge(C.c_void_p(table.data_ptr()), n, op, T, bpc, fill, C.c_void_p(flags.data_ptr()), len(coords), stream)
            if rc:
                raise RuntimeError(_lib.last_error())
    yard_src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    yard_dst = torch.empty_like(yard_src)
    arms = [("kernel", kernel, event_time, None), ("copy", lambda: yard_dst.copy_(yard_src), event_time, None)]
    row = {"what": name, "tiles": len(coords), "record": list(record), "moved_mb": round(moved / 1e6, 1)}
    row.update(alternate(arms, args.reps))
    store.free.extend(slabs.values())
    del yard_src, yard_dst
    arms = [("call", call, wall_time, give_back)]
    if parent is not None:
        arms.append(("parent", parent, wall_time, None))
    row.update(alternate(arms, args.reps))
    row["kernel_gb_s"] = round(moved / row["kernel"]["median_us"] / 1e3, 1)
    row["copy_gb_s"] = round(moved / row["copy"]["median_us"] / 1e3, 1)
    row["kernel_over_copy"] = round(row["kernel"]["median_us"] / row["copy"]["median_us"], 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    rows = []
    sm, other = make_site(), make_site()
    T = sm._scroll.T
    coords = sm.site_tiles()
    rect = (min(t[0] for t in coords), max(t[0] for t in coords), min(t[1] for t in coords), max(t[1] for t in coords))
    src = torch.full((len(coords), T, T, 5), 0.5, dtype=torch.float64, device=dev)

    def parent_overlap():
        a, b = sm.site_map(rect)[1], other.site_map(rect)[1]
        a.add_(b)
    rows.append(bench("overlap", sm, coords, {"map": src}, parent=parent_overlap))
    # the file route once: the same tiles as host arrays, merge_site's checks and the upload included
    arrays = S.pack_site(sm._scroll.anchor, RES, T, 5, "f64", {"map": (np.array(coords), src.cpu().numpy())})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sm.merge_site(arrays)
    torch.cuda.synchronize()
    host_route = (time.perf_counter() - t0) * 1e6
    del arrays
    rows.append(bench("f32 source", sm, coords, {"map": src.to(torch.float32)}, src_dtypes={"map": torch.float32}))
    del other
    far = make_site(first_tile=60)
    both = (rect[0], rect[1] + 60, rect[2], rect[3])

    def parent_disjoint():
        a, b = sm.site_map(both)[1], far.site_map(both)[1]
        a.add_(b)
    rows.append(bench("disjoint", sm, [(t[0] + 60, t[1]) for t in coords], {"map": src}, parent=parent_disjoint))
    del sm, far, src
    torch.cuda.empty_cache()
    sm, other = make_site(elevation=True), make_site(elevation=True)
    coords = sm.site_tiles("elevation")
    assert len(coords) == 3600

    def parent_elevation():
        a, b = sm.site_map(rect, "elevation")[1], other.site_map(rect, "elevation")[1]
        a[0].add_(b[0]), a[1].add_(b[1])
        torch.minimum(a[2], b[2], out=a[2]), torch.maximum(a[3], b[3], out=a[3])
    layers = {n: torch.full((len(coords), T, T), 2, dtype=dt, device=dev) for n, dt in ELEV}
    rows.append(bench("elevation", sm, coords, layers, parent=parent_elevation))
    print("\n%-11s %6s %9s | kernel us (min..max)          GB/s | copy_ us (min..max)           GB/s | kernel/copy | call wall us (min..max)        | parent wall us"
          % ("case", "tiles", "moved MB"))
    for r in rows:
        k, c, w = r["kernel"], r["copy"], r["call"]
        print("%-11s %6d %9.1f | %9.1f (%9.1f..%9.1f) %6.1f | %9.1f (%9.1f..%9.1f) %6.1f | %6.3f      | %9.1f (%9.1f..%9.1f) | %s" % (
            r["what"], r["tiles"], r["moved_mb"], k["median_us"], k["min_us"], k["max_us"], r["kernel_gb_s"], c["median_us"], c["min_us"],
            c["max_us"], r["copy_gb_s"], r["kernel_over_copy"], w["median_us"], w["min_us"], w["max_us"],
            "%.1f" % r["parent"]["median_us"] if "parent" in r else "-"))
    print("\nmerge_site() of the overlap case from host arrays (checks, a 1.44 GB upload, the merge): %.1f us, once" % host_route)


if __name__ == "__main__":
    main()
