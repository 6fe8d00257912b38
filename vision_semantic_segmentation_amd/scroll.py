"""The scrolling grid (MAPPING.SCROLL): the device grid [Hm, Wm, C] as a window that follows the vehicle over an unbounded site.

The reference's grid is the fixed rectangle of MAPPING.BOUNDARY (src/mapping.py:106-117); a point outside it is dropped (:410-411).
Here the window's origin moves in whole tiles of T x T cells so that the vehicle stays near the centre; tiles that leave go to a tile
store in HBM, tiles that enter come back from it or start in the empty state.  Off by default: nothing of this module then runs.

GEOMETRY (pure host functions, float64 and Python integers):
  * global cell (0, 0) is the configured MAPPING.BOUNDARY minimum, the ANCHOR; it never changes.
  * the window's origin (i0, j0) is in global cells, both multiples of T = int(round(TILE_M / RESOLUTION)); T % 4 == 0, Hm % T == 0,
    Wm % T == 0; |i0|, |j0| < 2^30.
  * THE WINDOW'S BOUNDARY, stated once, here:  minimum = anchor + float(i0) * resolution  (one float64 product, one float64 sum; the
    same along y), maximum = minimum + Hm * resolution (Wm along y).  With a resolution such as 0.1 the cell edges of two origins
    differ by ulps; that is accepted, and the tests' NumPy site uses the same floats.
  * the vehicle's cell is floor((pose.xy + PCD_ORIGIN_OFFSET.xy - anchor) / resolution): floor, a site extends to both sides.

DEVICE WORK is one operation, a table of tile jobs (struct avl_tile_job of include/avl_hip.h, k_tile_copy of csrc/seg_scroll.hip): a
scroll, a reload, the assembly of a site and a save build such a table on the host, VALIDATE it on the host -- every source and
destination range inside the buffer it names, validate_jobs -- and launch it once per layer.  A table that fails is never launched.

THE SITE OVERVIEW (TileStore.site_overview) is the one reader that assembles nothing: a table of tile SOURCES (struct avl_tile_src,
k_site_overview of csrc/seg_overview.hip), built with index arithmetic on whole arrays (overview_sources), validated on the host
(validate_sources) and launched once, gives the site reduced by k x k cells per pixel and its picture.

THE SITE FINISH (TileStore.site_finish) is the run's end result for the whole site -- the filtered picture at one pixel per cell, its
labels and the ground-truth/label counts -- by the same scheme: a table of tile RECORDS (struct avl_tile_fin, k_site_finish of
csrc/seg_sitefinish.hip), which is the overview's table plus a NULL record for every absent tile that touches a present one and every
record's eight neighbour indices (finish_sources), validated on the host (validate_finish) and launched once.

MERGING SITES (TileStore.merge_site, TileStore.global_site) sums another run's or another rank's tiles into the tiles where they live
-- the live window buffer, a slab of the store, a new slab -- by a table of the same tile jobs, read by another kernel (k_tile_merge of
csrc/seg_sitemerge.hip: result = acc (+) src, in place; a job's ``fresh`` word says that acc is the fill word), built by merge_jobs
and validated, encoded, uploaded and launched once per layer by the code that serves the copy tables (validate_jobs(merge=True),
encode_jobs, TileStore._run).  A frame's contribution never reads the grid, so the sum of two sites is the site of all their frames.

THE STORE.  One pool per layer (the map; with MAPPING.ELEVATION its four arrays), made of chunks of POOL_CHUNK_TILES slabs of
T * T * bytes_per_cell bytes; a chunk is a CUDA tensor.  The pool grows by whole chunks, so a stored tile never moves and jobs carry
plain device addresses.  The host owns the directory {(ti, tj): slab} and the free list; a slab index names the same slot in every
layer's pool.  Nothing spills to host memory: the pool grows until the allocator refuses.
"""
import collections
import math

import numpy as np

from .mapping import PCD_ORIGIN_OFFSET            # mapping.py imports this module only inside functions

MAX_ORIGIN = 1 << 30

Job = collections.namedtuple("Job", "src src_off src_pitch dst dst_off dst_pitch flag fresh", defaults=(0,))
"""One tile job in host form: ``src`` / ``dst`` name a buffer ("old", "new", "out", ("chunk", k), ...; src None = fill, in a copy table
only), the offsets and pitches are bytes.  ``fresh`` is read by a merge alone: true when the accumulator is the layer's fill word and
the destination is not read.  encode_jobs turns it into struct avl_tile_job with the buffers' device addresses."""

JOB_DTYPE = np.dtype([("src", "<u8"), ("src_pitch", "<i8"), ("dst", "<u8"), ("dst_pitch", "<i8"), ("flag", "<i4"), ("fresh", "<i4")])

Layer = collections.namedtuple("Layer", "name bpc fill")
ELEVATION_LAYERS = (Layer("elev_sum", 8, 0), Layer("elev_cnt", 4, 0), Layer("elev_min", 4, 0x7FFFFFFF), Layer("elev_max", 4, 0x80000000))


# ------------------------------------------------------------------------------------------------ geometry
def tile_cells(tile_m, resolution):
    return int(round(float(tile_m) / float(resolution)))


def check_geometry(Hm, Wm, T):
    """ValueError, naming the numbers, unless T % 4 == 0, Hm % T == 0 and Wm % T == 0."""
    if T < 4 or T % 4 != 0:
        raise ValueError("MAPPING.SCROLL: a tile of T = %d cells (TILE_M / RESOLUTION) must be a positive multiple of 4" % T)
    if Hm % T != 0 or Wm % T != 0:
        raise ValueError("MAPPING.SCROLL: the grid of Hm = %d x Wm = %d cells is no whole number of tiles of T = %d cells" % (Hm, Wm, T))


def check_origin(origin, T):
    i0, j0 = int(origin[0]), int(origin[1])
    if i0 % T != 0 or j0 % T != 0:
        raise ValueError("scroll origin (%d, %d) is no multiple of the tile size T = %d" % (i0, j0, T))
    if abs(i0) >= MAX_ORIGIN or abs(j0) >= MAX_ORIGIN:
        raise ValueError("scroll origin (%d, %d) is at or beyond 2^30 cells from the anchor" % (i0, j0))
    return i0, j0


def rect_shape(rect, T):
    """(nh, nw), the tiles per side of the tile rectangle ``rect`` = (ti0, ti1, tj0, tj1), both ends included (0 for an empty side);
    ValueError unless its first cell is an origin check_origin admits."""
    ti0, ti1, tj0, tj1 = (int(v) for v in rect)
    check_origin((ti0 * T, tj0 * T), T)
    return max(ti1 - ti0 + 1, 0), max(tj1 - tj0 + 1, 0)


def window_boundary(anchor, origin, Hm, Wm, res):
    """[[x_min, x_max], [y_min, y_max]] of the window at ``origin`` = (i0, j0): the module's one statement of the expression."""
    res = float(res)
    x0 = float(anchor[0]) + float(int(origin[0])) * res
    y0 = float(anchor[1]) + float(int(origin[1])) * res
    return [[x0, x0 + int(Hm) * res], [y0, y0 + int(Wm) * res]]


def vehicle_cell(pose, anchor, res):
    """The vehicle's global cell (i, j), Python integers, or None for a pose that is not finite (no scroll).  Plain float64
    arithmetic, no array: this runs in front of every frame."""
    if pose is None:
        return None
    if hasattr(pose, "position"):
        x, y = float(pose.position.x), float(pose.position.y)
    else:
        x, y = float(pose[0]), float(pose[1])
    cx = (x + PCD_ORIGIN_OFFSET[0] - anchor[0]) / res
    cy = (y + PCD_ORIGIN_OFFSET[1] - anchor[1]) / res
    if not (math.isfinite(cx) and math.isfinite(cy)):
        return None
    return math.floor(cx), math.floor(cy)


def next_origin(current, cell, Ht, Wt, T, hysteresis):
    """The window's next origin in cells.  ``current`` None = the first call of a run: the desired origin is taken.  Otherwise the
    desired origin tile, vehicle tile - (Ht // 2, Wt // 2), replaces the current one on BOTH axes when it differs from it by more
    than ``hysteresis`` tiles on either; else the origin stays.  ``cell`` None (vehicle_cell of a non-finite pose): no scroll,
    ``current`` comes back ((0, 0) on a first call).  ValueError at or beyond 2^30 cells."""
    if cell is None:
        return (0, 0) if current is None else (int(current[0]), int(current[1]))
    want = (cell[0] // T - Ht // 2, cell[1] // T - Wt // 2)                  # Python's // floors
    if current is not None:
        cur = (int(current[0]) // T, int(current[1]) // T)
        if abs(want[0] - cur[0]) <= hysteresis and abs(want[1] - cur[1]) <= hysteresis:
            return int(current[0]), int(current[1])
    return check_origin((want[0] * T, want[1] * T), T)


# ------------------------------------------------------------------------------------------------ job tables
def window_tiles(origin_tile, Ht, Wt):
    a, b = origin_tile
    return [(a + i, b + j) for i in range(Ht) for j in range(Wt)]


def plan_scroll(old_tile, new_tile, Ht, Wt, stored, window_valid=True):
    """What a move of the window from origin tile ``old_tile`` to ``new_tile`` does, in tiles: {"leaving": tiles of the old window
    that are not in the new one, "dst": [(tile, kind)] for every tile of the new window, kind "overlap" (it was in the old window),
    "load" (it is in ``stored``) or "fill"}.  ``window_valid`` False: the old window holds nothing (after load_site) -- no tile
    leaves, none overlaps.  A jump further than the window has no overlap; the code is the same."""
    (a0, b0), (a1, b1) = old_tile, new_tile

    def inside(t, a, b):
        return a <= t[0] < a + Ht and b <= t[1] < b + Wt
    leaving = [t for t in window_tiles(old_tile, Ht, Wt) if not inside(t, a1, b1)] if window_valid else []
    dst = []
    for t in window_tiles(new_tile, Ht, Wt):
        if window_valid and inside(t, a0, b0):
            dst.append((t, "overlap"))
        else:
            dst.append((t, "load" if t in stored else "fill"))
    return {"leaving": leaving, "dst": dst}


def window_ref(tile, origin_tile, T, Wm, bpc):
    """(byte offset, pitch) of ``tile`` inside a window buffer [Hm, Wm, bpc bytes] whose first tile is ``origin_tile``"""
    return (((tile[0] - origin_tile[0]) * T * Wm) + (tile[1] - origin_tile[1]) * T) * bpc, Wm * bpc


def slab_ref(slab, chunk_tiles, T, bpc):
    """(buffer key, byte offset, pitch) of slab ``slab`` in a pool of chunks of ``chunk_tiles`` slabs"""
    return ("chunk", slab // chunk_tiles), (slab % chunk_tiles) * T * T * bpc, T * bpc


def scroll_jobs(plan, old_tile, new_tile, T, Wm, bpc, chunk_tiles, slab_of_leaving, slab_of_stored):
    """The job table of one layer for ``plan``: first one job "old" window -> fresh slab per leaving tile (flag k for the k-th),
    then one job per tile of the new window into "new".  ``slab_of_leaving``: a slab per leaving tile, in order; ``slab_of_stored``:
    {tile: slab} for the tiles of kind "load"."""
    jobs = []
    for k, t in enumerate(plan["leaving"]):
        so, sp = window_ref(t, old_tile, T, Wm, bpc)
        dk, do, dp = slab_ref(slab_of_leaving[k], chunk_tiles, T, bpc)
        jobs.append(Job("old", so, sp, dk, do, dp, k))
    for t, kind in plan["dst"]:
        do, dp = window_ref(t, new_tile, T, Wm, bpc)
        if kind == "overlap":
            so, sp = window_ref(t, old_tile, T, Wm, bpc)
            jobs.append(Job("old", so, sp, "new", do, dp, -1))
        elif kind == "load":
            sk, so, sp = slab_ref(slab_of_stored[t], chunk_tiles, T, bpc)
            jobs.append(Job(sk, so, sp, "new", do, dp, -1))
        else:
            jobs.append(Job(None, 0, 0, "new", do, dp, -1))
    return jobs


def fill_int32(fill):
    """a layer's fill word as the int32 of the same bits, for tensors viewed as torch.int32"""
    return fill - (1 << 32) if fill >= (1 << 31) else fill


def tile_row_bytes(what, T, bpc):
    """T * bpc, the bytes of a tile row of a table of ``what``; ValueError unless the tile kernels can move such rows"""
    row = T * bpc
    if bpc % 4 != 0 or not 4 <= bpc <= 128 or row % 16 != 0:
        raise ValueError("%s: bytes_per_cell = %d, T = %d (bytes_per_cell a multiple of 4 up to 128, T * bytes_per_cell of 16)" % (what, bpc, T))
    return row


def validate_jobs(jobs, buffers, T, bpc, n_flags=None, src_bpc=None, merge=False):
    """ValueError, naming the job, unless every job of the table is safe to launch: a copy table (avl_tile_copy), with ``merge`` a
    merge table (avl_tile_merge).  ``buffers``: {key: (device address, bytes)}.  Every source and destination tile -- T rows,
    ``pitch`` apart -- lies inside the buffer it names; every address and pitch is a multiple of 16 and a pitch is at least a row; no
    destination tile is named twice; no job's source is any job's destination, and a buffer is read or written, never both, except
    distinct slabs of a chunk; a flag is below ``n_flags``.  A row is T * bpc bytes.  The two kinds differ in the source alone: a
    copy job without one fills its destination, a merge job must have one; and a merge table's source rows may be T * ``src_bpc``
    bytes with src_bpc = bpc // 2, the float32 source of the exchange form (None = bpc; a copy table takes None only).  In both, the
    only range a job may read and write is a merge job's own destination, which the kernel reads by itself and no ``src`` names."""
    what = "merge job" if merge else "tile job"
    dst_row = tile_row_bytes(what + "s", T, bpc)
    if src_bpc is not None and not merge:
        raise ValueError("tile jobs: a source of %d bytes per cell; only a merge table has source rows of their own" % src_bpc)
    src_bpc = bpc if src_bpc is None else src_bpc
    if src_bpc not in (bpc, bpc // 2) or (T * src_bpc) % 16 != 0:
        raise ValueError("merge jobs: a source of %d bytes per cell for a destination of %d, T = %d (the same or half of it, rows a "
                         "multiple of 16 bytes)" % (src_bpc, bpc, T))
    src_row, last = T * src_bpc, T - 1
    written, read = {}, {}                                                 # {(key, off): the first job that names it}
    # this loop is most of a scroll's host time: what a side of a job needs is bound once, (name, row bytes, first namer of a place)
    extent_of = buffers.get
    src_side, dst_side = ("src", src_row, read.setdefault), ("dst", dst_row, written.setdefault)
    for k, (src, src_off, src_pitch, dst, dst_off, dst_pitch, flag, _) in enumerate(jobs):
        for (side, row, first), key, off, pitch in ((src_side, src, src_off, src_pitch), (dst_side, dst, dst_off, dst_pitch)):
            if key is None:
                if side == "src" and not merge:
                    continue                                               # a fill
                raise ValueError("%s %d has no %s" % (what, k, "source" if side == "src" else "destination"))
            extent = extent_of(key)
            if extent is None:
                raise ValueError("%s %d: %s names the unknown buffer %r" % (what, k, side, key))
            base, nbytes = extent
            if (pitch | (base + off)) & 15 or pitch < row:                 # one test for both alignments
                if pitch % 16 != 0 or pitch < row:
                    raise ValueError("%s %d: %s pitch %d is misaligned or shorter than a tile row of %d bytes" % (what, k, side, pitch, row))
                raise ValueError("%s %d: %s address %d + %d is not 16-byte aligned" % (what, k, side, base, off))
            end = off + last * pitch + row
            if off < 0 or end > nbytes:
                raise ValueError("%s %d: %s bytes %d .. %d leave buffer %r of %d bytes" % (what, k, side, off, end, key, nbytes))
            if first((key, off), k) != k and side == "dst":
                raise ValueError("%s %d: destination tile %r + %d appears twice (job %d)" % (what, k, key, off, written[(key, off)]))
        if n_flags is not None and flag >= n_flags:
            raise ValueError("%s %d: flag %d of %d" % (what, k, flag, n_flags))
    both = written.keys() & read.keys()
    if both:
        place = min(both, key=read.get)
        raise ValueError("%s %d: its source %r + %d is the destination of job %d: read and written in one table"
                         % (what, read[place], place[0], place[1], written[place]))
    for key in {key for key, _ in read} & {key for key, _ in written}:
        if not (isinstance(key, tuple) and key[0] == "chunk"):
            raise ValueError("%s %d: its source buffer %r is written in the same table"
                             % (what, min(k for (other, _), k in read.items() if other == key), key))


def encode_jobs(jobs, buffers, out):
    """``jobs`` as struct avl_tile_job records into the structured array ``out`` (JOB_DTYPE, at least len(jobs) long)."""
    n = len(jobs)
    if n:
        base = {key: extent[0] for key, extent in buffers.items()}
        out[:n] = [(0 if src is None else base[src] + src_off, src_pitch, base[dst] + dst_off, dst_pitch, flag, fresh)
                   for src, src_off, src_pitch, dst, dst_off, dst_pitch, flag, fresh in jobs]       # one pass, one assignment of whole records
    return n


# ------------------------------------------------------------------------------------------------ merge tables
SiteMerge = collections.namedtuple("SiteMerge", "window store added freed")
"""What merge_site returns, in tiles: summed into the window in place, summed into slabs of the store, added as new slabs, and slabs
(old or new) that went back to the free list because the result is empty in every layer."""


def merge_op(layer_name, dst_dtype, src_dtype=None):
    """avl_tile_merge's op for a layer: the elevation layer's arrays by name, the map by its type ("f64" | "f32"); a float32 source
    on a float64 map is the exchange form AVL_MERGE_ADD_F32_TO_F64."""
    from . import _lib
    ops = {"elev_sum": _lib.AVL_MERGE_ADD_I64, "elev_cnt": _lib.AVL_MERGE_ADD_I32, "elev_min": _lib.AVL_MERGE_MIN_I32,
           "elev_max": _lib.AVL_MERGE_MAX_I32}
    if layer_name in ops:
        return ops[layer_name]
    src_dtype = dst_dtype if src_dtype is None else src_dtype
    if (dst_dtype, src_dtype) == ("f64", "f32"):
        return _lib.AVL_MERGE_ADD_F32_TO_F64
    if dst_dtype != src_dtype or dst_dtype not in ("f64", "f32"):
        raise ValueError("no merge of %s tiles into a %s map" % (src_dtype, dst_dtype))
    return _lib.AVL_MERGE_ADD_F64 if dst_dtype == "f64" else _lib.AVL_MERGE_ADD_F32


def merge_jobs(entries, T, Wm, bpc, chunk_tiles, origin_tile, src_bpc=None, src="stage"):
    """The merge table of one layer.  ``entries``: [(tile, k, kind, slab, flag)] -- the tile's data is the k-th tile of the buffer
    ``src`` (tiles of T * T * src_bpc bytes, one after the other; src_bpc None = bpc, bpc // 2 = the float32 exchange form); kind
    "window": the destination is the tile's place in the live window buffer "window", whose first tile is ``origin_tile``, merged in
    place and without a flag (the window's emptiness is looked up when it is asked for); "store": slab ``slab``, in place; "fresh":
    slab ``slab``, a new one, never read.  A slab's job reports its result in ``flag``."""
    src_bpc = bpc if src_bpc is None else src_bpc
    jobs = []
    for t, k, kind, slab, flag in entries:
        if kind == "window":
            do, dp = window_ref(t, origin_tile, T, Wm, bpc)
            jobs.append(Job(src, k * T * T * src_bpc, T * src_bpc, "window", do, dp, -1, 0))
        elif kind in ("store", "fresh"):
            dk, do, dp = slab_ref(slab, chunk_tiles, T, bpc)
            jobs.append(Job(src, k * T * T * src_bpc, T * src_bpc, dk, do, dp, flag, int(kind == "fresh")))
        else:
            raise ValueError("merge entry %r: kind %r" % (t, kind))
    return jobs


# ------------------------------------------------------------------------------------------------ the overview's source table
SOURCE_DTYPE = np.dtype([("buf", "<i4"), ("row", "<i4"), ("col", "<i4"), ("off", "<i8"), ("pitch", "<i8")])
"""One tile of a site overview in host form: ``buf`` indexes a list of buffers -- 0 the window, 1 + c chunk c of the pool -- ``off`` and
``pitch`` are bytes, (``row``, ``col``) is the tile's place in the rectangle.  encode_sources turns it into struct avl_tile_src."""

SRC_DTYPE = np.dtype([("src", "<u8"), ("src_pitch", "<i8"), ("row", "<i4"), ("col", "<i4")])


def overview_sources(rect, T, bpc, Wm, origin_tile, window_mask, stored_tiles, stored_slabs, chunk_tiles):
    """The source table (SOURCE_DTYPE, sorted by row, col) of the tile rectangle ``rect`` = (ti0, ti1, tj0, tj1), both ends included:
    one record per tile that holds something, none for the others.  ``window_mask``: bool [Ht, Wt], the window's tiles that hold
    something (None: the window holds nothing), the window's first tile being ``origin_tile``; ``stored_tiles`` int [n, 2] and
    ``stored_slabs`` int [n]: the stored tiles that hold something and their slabs.  Index arithmetic on whole arrays: the cost
    follows what was mapped, not the rectangle."""
    ti0, tj0 = int(rect[0]), int(rect[2])
    nh, nw = rect_shape(rect, T)
    parts = []
    if window_mask is not None:
        wi, wj = np.nonzero(np.asarray(window_mask))
        part = np.zeros(wi.size, dtype=SOURCE_DTYPE)
        part["off"], part["pitch"] = (wi.astype(np.int64) * (T * Wm) + wj.astype(np.int64) * T) * bpc, Wm * bpc
        parts.append((part, wi + int(origin_tile[0]) - ti0, wj + int(origin_tile[1]) - tj0))
    stored_tiles = np.asarray(stored_tiles, dtype=np.int64).reshape(-1, 2)
    slabs = np.asarray(stored_slabs, dtype=np.int64).reshape(-1)
    part = np.zeros(slabs.size, dtype=SOURCE_DTYPE)
    part["buf"] = 1 + slabs // chunk_tiles
    part["off"], part["pitch"] = (slabs % chunk_tiles) * (T * T * bpc), T * bpc
    parts.append((part, stored_tiles[:, 0] - ti0, stored_tiles[:, 1] - tj0))
    kept = []
    for part, r, c in parts:                                   # the window and the store: two trips
        inside = (r >= 0) & (r < nh) & (c >= 0) & (c < nw)
        part = part[inside]
        part["row"], part["col"] = r[inside], c[inside]
        kept.append(part)
    table = np.concatenate(kept)
    return table[np.lexsort((table["col"], table["row"]))]


def validate_sources(table, buffers, T, bpc, nh, nw):
    """ValueError unless every record of the source table is safe to launch.  ``buffers``: [(device address, bytes)], indexed by
    ``buf``.  Every tile -- T rows of T * bpc bytes, ``pitch`` apart -- lies inside the buffer it names; every address and pitch is a
    multiple of 16 and a pitch is at least a row; row and col are inside nh x nw; no (row, col) appears twice."""
    row = tile_row_bytes("tile sources", T, bpc)
    if len(table) == 0:
        return
    refuse = _refuser("source", table)
    buf = table["buf"].astype(np.int64)
    bad = (buf < 0) | (buf >= len(buffers))
    if bad.any():
        refuse(bad, "names a buffer outside the %d given" % len(buffers))
    base = np.array([b[0] for b in buffers], dtype=np.int64)[buf]
    nbytes = np.array([b[1] for b in buffers], dtype=np.int64)[buf]
    off, pitch = table["off"], table["pitch"]
    bad = (pitch % 16 != 0) | (pitch < row)
    if bad.any():
        refuse(bad, "has a pitch that is misaligned or shorter than a tile row of %d bytes" % row)
    bad = (base + off) % 16 != 0
    if bad.any():
        refuse(bad, "is not 16-byte aligned")
    bad = (off < 0) | (off + (T - 1) * pitch + row > nbytes)
    if bad.any():
        refuse(bad, "leaves its buffer")
    _validate_places(table, nh, nw, refuse)


def _refuser(kind, table):
    """refuse(bad, what): ValueError that names the first record of ``table`` that the bool array ``bad`` marks"""
    def refuse(bad, what):
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("tile %s %d of %d %s: %r" % (kind, k, len(table), what, table[k]))
    return refuse


def _validate_places(table, nh, nw, refuse):
    """every record's (row, col) is inside nh x nw and none appears twice, or refuse(...)"""
    r, c = table["row"].astype(np.int64), table["col"].astype(np.int64)
    bad = (r < 0) | (r >= nh) | (c < 0) | (c >= nw)
    if bad.any():
        refuse(bad, "lies outside the rectangle of %d x %d tiles" % (nh, nw))
    place = r * nw + c
    order = np.argsort(place, kind="stable")
    twice = np.flatnonzero(np.diff(place[order]) == 0)
    if twice.size:
        bad = np.zeros(len(table), dtype=bool)
        bad[order[twice[0] + 1]] = True
        refuse(bad, "names a (row, col) that an earlier record names")


def encode_sources(table, buffers, out):
    """``table`` as struct avl_tile_src records into the structured array ``out`` (SRC_DTYPE, at least len(table) long)."""
    n = len(table)
    if n:
        base = np.array([b[0] for b in buffers], dtype=np.uint64)
        out["src"][:n] = base[table["buf"]] + table["off"].astype(np.uint64)
        out["src_pitch"][:n] = table["pitch"]
        out["row"][:n] = table["row"]
        out["col"][:n] = table["col"]
    return n


# ------------------------------------------------------------------------------------------------ the finish's record table
FINISH_DTYPE = np.dtype([("buf", "<i4"), ("row", "<i4"), ("col", "<i4"), ("off", "<i8"), ("pitch", "<i8"), ("nb", "<i4", (9,))])
"""One tile of a site finish in host form: SOURCE_DTYPE's fields -- ``buf`` -1 = a NULL record, a tile that holds nothing but is computed
because a present tile touches it -- and ``nb``, the index of the record at (row + dr, col + dc) in nb[(dr + 1) * 3 + (dc + 1)], -1 where
there is none; nb[4] is the record's own index.  encode_finish turns it into struct avl_tile_fin."""

FIN_DTYPE = np.dtype([("src", "<u8"), ("src_pitch", "<i8"), ("row", "<i4"), ("col", "<i4"), ("nb", "<i4", (9,)), ("pad", "<i4")])

NEIGHBOUR_OFFSETS = [(dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1)]


def finish_neighbours(row, col, nh, nw):
    """int32 [n, 9]: for records at (row[i], col[i]) -- no place twice -- the index of the record at each of NEIGHBOUR_OFFSETS, -1
    where there is none or the place lies outside the rectangle.  A sort and nine searches on whole arrays."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = row.size
    nb = np.full((n, 9), -1, dtype=np.int32)
    if n == 0:
        return nb
    place = row * nw + col
    in_order = bool((place[1:] > place[:-1]).all())                         # finish_sources' own tables are sorted by (row, col)
    order = None if in_order else np.argsort(place, kind="stable")
    sorted_place = place if in_order else place[order]
    for k, (dr, dc) in enumerate(NEIGHBOUR_OFFSETS):
        r, c = row + dr, col + dc
        inside = (r >= 0) & (r < nh) & (c >= 0) & (c < nw)
        want = r * nw + c
        at = np.minimum(np.searchsorted(sorted_place, want), n - 1)
        found = inside & (sorted_place[at] == want)
        nb[:, k] = np.where(found, at if in_order else order[at], -1)
    return nb


def finish_sources(rect, T, bpc, Wm, origin_tile, window_mask, stored_tiles, stored_slabs, chunk_tiles):
    """The record table (FINISH_DTYPE, sorted by row, col) of the tile rectangle ``rect``: overview_sources' records, a NULL record
    (``buf`` -1) for every absent tile of the rectangle with at least one present 8-neighbour, and every record's neighbour indices.
    The arguments are overview_sources'.  Index arithmetic on whole arrays: the cost follows what was mapped, not the rectangle."""
    nh, nw = rect_shape(rect, T)
    present = overview_sources(rect, T, bpc, Wm, origin_tile, window_mask, stored_tiles, stored_slabs, chunk_tiles)
    r, c = present["row"].astype(np.int64), present["col"].astype(np.int64)
    around = []
    for dr, dc in NEIGHBOUR_OFFSETS:
        rr, cc = r + dr, c + dc
        inside = (rr >= 0) & (rr < nh) & (cc >= 0) & (cc < nw)
        around.append((rr * nw + cc)[inside])
    ring = np.setdiff1d(np.concatenate(around) if around else np.zeros(0, dtype=np.int64), r * nw + c)
    table = np.zeros(len(present) + ring.size, dtype=FINISH_DTYPE)
    for name in SOURCE_DTYPE.names:
        table[name][:len(present)] = present[name]
    table["buf"][len(present):] = -1
    if ring.size:
        table["row"][len(present):], table["col"][len(present):] = ring // nw, ring % nw
    table = table[np.lexsort((table["col"], table["row"]))]
    table["nb"] = finish_neighbours(table["row"], table["col"], nh, nw)
    return table


def validate_finish(table, buffers, T, bpc, nh, nw):
    """ValueError, naming the first bad record, unless the record table is safe to launch: everything validate_sources checks for the
    records with a source; T >= 2; every record, NULL ones included, inside nh x nw and no (row, col) twice; every neighbour index names
    the record at exactly that offset, or is -1 where there is none (so no index leaves the table)."""
    if T < 2:
        raise ValueError("tile records: T = %d cells (at least 2: the filter reflects at the rectangle's edge)" % T)
    n = len(table)
    validate_sources(table[table["buf"] >= 0], buffers, T, bpc, nh, nw)
    if n == 0:
        return
    refuse = _refuser("record", table)
    _validate_places(table, nh, nw, refuse)                                 # the NULL records too
    bad = (np.asarray(table["nb"]).reshape(n, 9) != finish_neighbours(table["row"], table["col"], nh, nw)).any(axis=1)
    if bad.any():
        refuse(bad, "has a neighbour index that does not name the record at that offset")


def encode_finish(table, buffers, out):
    """``table`` as struct avl_tile_fin records into the structured array ``out`` (FIN_DTYPE, at least len(table) long)."""
    n = encode_sources(table, list(buffers) + [(0, 0)], out)                        # buf -1, a NULL record: the appended address 0 ...
    if n:
        out["src"][:n][table["buf"] < 0] = 0                                       # ... whatever its offset says
        out["nb"][:n] = table["nb"]
        out["pad"][:n] = 0
    return n


SiteFinish = collections.namedtuple("SiteFinish", "origin picture labels counts tiles")
"""What site_finish returns: ``origin`` the global cell of the first element, ``picture`` uint8 [H, W, 3] and ``labels`` uint8 [H, W]
(CUDA tensors, or None when not asked for), ``counts`` int64 NumPy [8, 8] over the whole rectangle (None without truth), ``tiles`` =
(records with a source, NULL records)."""


def overview_cells_per_pixel(T, nh, nw, max_side_px):
    """MAPPING.SITE_OVERVIEW.CELLS_PER_PIXEL = 0: the smallest divisor k of T for which the longer side of the picture of nh x nw tiles,
    max(nh, nw) * T / k pixels, is at most ``max_side_px``; T (one pixel per tile) when none is."""
    for k in range(1, T + 1):
        if T % k == 0 and max(nh, nw) * (T // k) <= max_side_px:
            return k
    return T


# ------------------------------------------------------------------------------------------------ the site file
def pack_site(anchor, resolution, T, C_, dtype, layers):
    """The arrays of a site file (one .npz).  ``layers``: {layer name: (coords int [n, 2], tiles [n, T, T, ...])}."""
    out = {"anchor": np.asarray(anchor, dtype=np.float64), "resolution": np.float64(resolution), "T": np.int64(T), "C": np.int64(C_),
           "dtype": np.array(str(dtype)), "layers": np.array(sorted(layers))}
    for name, (coords, tiles) in layers.items():
        out[name + "_coords"] = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
        out[name + "_tiles"] = np.asarray(tiles)
    return out


def unpack_site(data, anchor=None, resolution=None, T=None, C_=None, dtype=None):
    """-> (meta dict, {layer name: (coords, tiles)}) of the arrays of a site file; ValueError when a given ``anchor``, ``resolution``,
    ``T``, ``C_`` or ``dtype`` is not the file's."""
    meta = {"anchor": tuple(float(v) for v in data["anchor"]), "resolution": float(data["resolution"]), "T": int(data["T"]),
            "C": int(data["C"]), "dtype": str(data["dtype"])}
    for name, want in (("anchor", None if anchor is None else tuple(float(v) for v in anchor)),
                       ("resolution", None if resolution is None else float(resolution)), ("T", T), ("C", C_), ("dtype", dtype)):
        if want is not None and meta[name] != want:
            raise ValueError("the site file has %s = %r, this map %r" % (name, meta[name], want))
    layers = {}
    for name in [str(n) for n in data["layers"]]:
        coords, tiles = np.asarray(data[name + "_coords"]), np.asarray(data[name + "_tiles"])
        if coords.shape[0] != tiles.shape[0] or (tiles.shape[0] and tuple(tiles.shape[1:3]) != (meta["T"], meta["T"])):
            raise ValueError("the site file's layer %r holds %s coordinates and tiles of shape %s" % (name, coords.shape, tiles.shape))
        layers[name] = (coords, tiles)
    return meta, layers


# ------------------------------------------------------------------------------------------------ the store
class _DeviceLayer(object):
    """One persistent layer on the device: its two window buffers and its pool"""

    def __init__(self, layer, get, put, alloc):
        self.name, self.bpc, self.fill = layer
        self.get, self.put, self.alloc = get, put, alloc       # the current window tensor, its replacement, a fresh one like it
        self.alt = None                                        # the second window buffer, allocated by the first scroll
        self.chunks = []


class TileStore(object):
    """The window's origin, the tile store and the scroll step of one SemanticMapping (MAPPING.SCROLL.ENABLED)."""

    def __init__(self, sm):
        import torch
        sc = sm.cfg.MAPPING.SCROLL
        if sm.depth_method not in ("points_map", "points_raw"):
            raise ValueError("MAPPING.SCROLL.ENABLED needs a LiDAR DEPTH_METHOD, not %r: the planar mode's discretize_matrix is tied to a "
                             "fixed boundary" % (sm.depth_method,))
        self.sm = sm
        self.torch = torch
        self.Hm, self.Wm, self.C = sm.map_height, sm.map_width, sm.map_depth
        self.res = float(sm.resolution)
        self.T = tile_cells(sc.TILE_M, self.res)
        check_geometry(self.Hm, self.Wm, self.T)
        self.Ht, self.Wt = self.Hm // self.T, self.Wm // self.T
        self.hysteresis = int(sc.HYSTERESIS_TILES)
        self.chunk_tiles = int(sc.POOL_CHUNK_TILES)
        if self.hysteresis < 0 or self.chunk_tiles < 1:
            raise ValueError("MAPPING.SCROLL: HYSTERESIS_TILES = %r (>= 0), POOL_CHUNK_TILES = %r (>= 1)" % (sc.HYSTERESIS_TILES, sc.POOL_CHUNK_TILES))
        self.anchor = (float(sm.map_boundary[0][0]), float(sm.map_boundary[1][0]))
        self.origin = (0, 0)
        self.first = True                 # no scroll_to has run: the next takes the desired origin
        self.band = None                  # set by a scroll: see _set_band; None = take the slow path (first call, after load_site)
        self.window_valid = True          # False after load_site: the window holds nothing and the next scroll_to always runs
        self.layers = None                # [_DeviceLayer], fixed by the first device operation
        self.directory = {}               # (ti, tj) -> slab
        self.nonempty = {}                # (ti, tj) -> bit mask of the layers whose stored tile holds something
        self.free = []
        self.n_slabs = 0
        self.pending = None               # (leaving tiles, number of layers) of the last scroll until its flags are retired
        self.tables = [None, None]        # ring of two job tables: [pinned host uint8, device uint8, event]
        self.table_turn = 0
        self.flags_dev = None
        self.flags_host = None
        self.flags_event = None
        self.exchanged = False            # global_site has run: the site holds the other ranks' frames

    # -------------------------------------------------------------------------------------------- layers and pools
    def _layers(self):
        if self.layers is None:
            sm, torch = self.sm, self.torch
            es = 8 if sm.grid.torch_dtype == torch.float64 else 4

            def put_map(t):
                sm.grid.map = t
            layers = [_DeviceLayer(Layer("map", es * self.C, 0), lambda: sm.grid.map, put_map, lambda: torch.empty_like(sm.grid.map))]
            if sm.elevation_enabled():
                sm.elevation_layer()                          # allocated, empty, now: the set of layers is fixed for the run
                for k, layer in enumerate(ELEVATION_LAYERS):
                    def put(t, k=k):
                        e = list(sm._elevation)
                        e[k] = t
                        sm._elevation = tuple(e)
                    layers.append(_DeviceLayer(layer, lambda k=k: sm._elevation[k], put, lambda k=k: torch.empty_like(sm._elevation[k])))
            self.layers = layers
        return self.layers

    def _slabs(self, n):
        """n slab indices off the free list, the pools grown by whole chunks as needed"""
        torch = self.torch
        while len(self.free) < n:
            first = self.n_slabs
            for L in self._layers():
                L.chunks.append(torch.empty(self.chunk_tiles * self.T * self.T * L.bpc, dtype=torch.uint8, device=self.sm.device))
            self.n_slabs += self.chunk_tiles
            self.free.extend(range(self.n_slabs - 1, first - 1, -1))       # popped from the end: lowest first
        return [self.free.pop() for _ in range(n)]

    def _buffers(self, L, extra=None):
        b = {("chunk", k): (c.data_ptr(), int(c.numel())) for k, c in enumerate(L.chunks)}
        if extra:
            b.update(extra)
        return b

    @staticmethod
    def _extent(t):
        return t.data_ptr(), int(t.numel()) * int(t.element_size())

    # -------------------------------------------------------------------------------------------- launching a table
    def _stream(self, stream):
        torch = self.torch
        if stream is None:
            return torch.cuda.current_stream(self.sm.device)
        if isinstance(stream, torch.cuda.Stream):
            return stream
        return torch.cuda.ExternalStream(int(stream), device=self.sm.device)

    def _ring_slot(self, nbytes):
        """[pinned host uint8, device uint8, event] for a table of ``nbytes``: the ring's next slot, waited for if its last table is
        still in flight, grown if it is too small.  The caller fills the host part, copies it on its stream and records the event."""
        torch = self.torch
        turn = self.table_turn
        self.table_turn ^= 1
        slot = self.tables[turn]
        if slot is not None:
            slot[2].synchronize()                                          # a table in flight is not overwritten
        if slot is None or int(slot[0].numel()) < nbytes:
            cap = max(2 * nbytes, 1 << 14)
            slot = self.tables[turn] = [torch.empty(cap, dtype=torch.uint8).pin_memory(),
                                        torch.empty(cap, dtype=torch.uint8, device=self.sm.device), torch.cuda.Event()]
        return slot

    def _launch_table(self, st, nbytes, fill, launch):
        """A table of ``nbytes`` through the ring on the torch stream ``st``: fill(records), the slot's pinned bytes as a NumPy
        uint8 array, writes it; it is copied to the device on ``st``; launch(address), called with ``st`` current, starts the
        kernels that read it there; the slot's event is recorded behind them."""
        host, dev, event = self._ring_slot(nbytes)
        fill(host.numpy()[:nbytes])
        with self.torch.cuda.stream(st):
            dev[:nbytes].copy_(host[:nbytes], non_blocking=True)
            launch(dev.data_ptr())
            event.record(st)

    def _run(self, per_layer, st, n_flags=0):
        """``per_layer``: [(layer, jobs, buffers)] for copy tables (avl_tile_copy), [(layer, jobs, buffers, op, src_bpc)] for merge
        tables (avl_tile_merge), all validated here, uploaded as one table through the ring and launched once per layer on the torch
        stream ``st``; with ``n_flags`` every layer's flags go to flags_dev[l * n_flags ...] and their copy into pinned memory is
        started, flags_event recorded behind it."""
        import ctypes as C
        from . import _lib
        per_layer = [e if len(e) == 5 else tuple(e) + (None, None) for e in per_layer]       # op None: a copy
        for L, jobs, buffers, op, src_bpc in per_layer:                   # raises before anything is uploaded or launched
            validate_jobs(jobs, buffers, self.T, L.bpc, n_flags, src_bpc, merge=op is not None)
        total = sum(len(e[1]) for e in per_layer)
        nbytes = max(total, 1) * JOB_DTYPE.itemsize
        starts = []

        def fill(records):
            rec, at = records.view(JOB_DTYPE), 0
            for _, jobs, buffers, _, _ in per_layer:
                starts.append(at)
                at += encode_jobs(jobs, buffers, rec[at:])
        n_layers = len(per_layer)
        self._flags_room(n_layers * n_flags)

        def launch(table):
            lib = _lib.lib()
            for l, (L, jobs, _, op, _) in enumerate(per_layer):
                flags = C.c_void_p(self.flags_dev.data_ptr() + 4 * l * n_flags) if n_flags else None
                head = (C.c_void_p(table + starts[l] * JOB_DTYPE.itemsize), len(jobs))
                tail = (self.T, L.bpc, L.fill, flags, n_flags, C.c_void_p(st.cuda_stream))
                if op is None:
                    _lib.check(lib.avl_tile_copy(*head, *tail), "avl_tile_copy")
                else:
                    _lib.check(lib.avl_tile_merge(*head, op, *tail), "avl_tile_merge")
        self._launch_table(st, nbytes, fill, launch)
        self._flags_home(st, n_layers * n_flags)

    def _flags_room(self, n):
        """flags_dev / flags_host hold at least ``n`` flags (grown once no copy of the old ones is in flight)"""
        torch = self.torch
        if n and (self.flags_dev is None or int(self.flags_dev.numel()) < n):
            if self.flags_event is not None:
                self.flags_event.synchronize()
            self.flags_event = torch.cuda.Event()
            cap = max(2 * n, 256)
            self.flags_dev = torch.empty(cap, dtype=torch.int32, device=self.sm.device)
            self.flags_host = torch.empty(cap, dtype=torch.int32).pin_memory()

    def _flags_home(self, st, n):
        """starts the copy of the first ``n`` flags into pinned memory on ``st`` and records flags_event behind it"""
        if n:
            with self.torch.cuda.stream(st):
                self.flags_host[:n].copy_(self.flags_dev[:n], non_blocking=True)
                self.flags_event.record(st)

    # -------------------------------------------------------------------------------------------- the scroll
    def retire(self):
        """The previous scroll's emptiness flags, whose copy completed long ago: the slabs of leaving tiles that turned out empty in
        every layer go back to the free list and leave the directory; the others keep the mask of their non-empty layers."""
        if self.pending is None:
            return
        leaving, n_layers = self.pending
        self.pending = None
        self.flags_event.synchronize()
        n = len(leaving)
        flags = self.flags_host[:n_layers * n].numpy().reshape(n_layers, n)
        for k, t in enumerate(leaving):
            mask = sum(1 << l for l in range(n_layers) if flags[l, k])
            if mask:
                self.nonempty[t] = mask
            else:
                self.free.append(self.directory.pop(t))
                self.nonempty.pop(t, None)

    def _set_band(self):
        """the vehicle cells for which the origin stays, as float bounds [lo, hi) per axis: floor(c) lies in an integer range exactly
        when c lies in [first, last + 1)"""
        T, h = self.T, self.hysteresis
        a, b = self.origin[0] // T + self.Ht // 2, self.origin[1] // T + self.Wt // 2
        self.band = (float((a - h) * T), float((a + h + 1) * T), float((b - h) * T), float((b + h + 1) * T))

    def scroll_to(self, pose, stream=None):
        band = self.band
        if band is not None and pose is not None:     # the frame's fast path: vehicle_cell's two quotients against the hysteresis band
            x, y = (pose.position.x, pose.position.y) if hasattr(pose, "position") else (pose[0], pose[1])
            if band[0] <= (x + PCD_ORIGIN_OFFSET[0] - self.anchor[0]) / self.res < band[1] and \
                    band[2] <= (y + PCD_ORIGIN_OFFSET[1] - self.anchor[1]) / self.res < band[3]:
                return False
        sm = self.sm
        cell = vehicle_cell(pose, self.anchor, self.res)
        if cell is None:
            return False
        new = next_origin(None if self.first else self.origin, cell, self.Ht, self.Wt, self.T, self.hysteresis)
        self.first = False
        if new == self.origin and self.window_valid:
            if self.band is None:
                self._set_band()
            return False
        self.retire()
        T = self.T
        old_tile, new_tile = (self.origin[0] // T, self.origin[1] // T), (new[0] // T, new[1] // T)
        plan = plan_scroll(old_tile, new_tile, self.Ht, self.Wt, self.directory, self.window_valid)
        leaving = plan["leaving"]
        layers = self._layers()
        fresh = self._slabs(len(leaving))
        loaded = [t for t, kind in plan["dst"] if kind == "load"]
        per_layer = []
        for L in layers:
            if L.alt is None:
                L.alt = L.alloc()
            jobs = scroll_jobs(plan, old_tile, new_tile, T, self.Wm, L.bpc, self.chunk_tiles, fresh, self.directory)
            per_layer.append((L, jobs, self._buffers(L, {"old": self._extent(L.get()), "new": self._extent(L.alt)})))
        try:
            self._run(per_layer, self._stream(stream), len(leaving))
        except Exception:
            self.free.extend(fresh)
            raise
        for t, s in zip(leaving, fresh):
            self.directory[t] = s
            self.nonempty[t] = (1 << len(layers)) - 1          # until the flags say otherwise
        for t in loaded:                                       # behind the launch, in stream order: the slab is free again
            self.free.append(self.directory.pop(t))
            self.nonempty.pop(t, None)
        self.pending = (leaving, len(layers)) if leaving else None
        for L in layers:                                       # the window is the second buffer now
            cur = L.get()
            L.put(L.alt)
            L.alt = cur
        filled = sum(1 for _, kind in plan["dst"] if kind == "fill")
        sm.last_scroll = {"shift": (new_tile[0] - old_tile[0], new_tile[1] - old_tile[1]), "leaving": len(leaving),
                          "entering": len(loaded) + filled, "loaded": len(loaded), "filled": filled}
        self.origin = new
        self.window_valid = True
        self._set_band()
        boundary = window_boundary(self.anchor, new, self.Hm, self.Wm, self.res)
        sm.grid.boundary = boundary
        sm.map_boundary = boundary
        sm._map_host = None
        sm.scroll_origin = new
        sm.scroll_count += 1
        return True

    # -------------------------------------------------------------------------------------------- the site
    def _window_nonempty(self):
        """{tile of the window: mask of its non-empty layers}, by bit pattern (a -0.0 is something)"""
        if not self.window_valid:
            return {}
        masks = self._window_masks()
        a, b = self.origin[0] // self.T, self.origin[1] // self.T
        return {(a + i, b + j): int(masks[i, j]) for i in range(self.Ht) for j in range(self.Wt) if masks[i, j]}

    def _window_masks(self, bits=-1):
        """int64 ndarray [Ht, Wt]: per tile of the window the mask of its non-empty layers, by bit pattern; only the layers of ``bits``
        are looked at"""
        torch = self.torch
        T, masks = self.T, None
        for l, L in enumerate(self._layers()):
            if not bits >> l & 1:
                continue
            words = L.get().contiguous().view(torch.int32).view(self.Ht, T, self.Wt, T, L.bpc // 4)
            some = words.ne(fill_int32(L.fill)).any(dim=4).any(dim=3).any(dim=1).to(torch.int64) << l
            masks = some if masks is None else masks | some
        return masks.cpu().numpy()

    def _layer_bits(self, layer):
        names = [L.name for L in self._layers()]
        if layer == "map":
            return 1
        if layer == "elevation":
            if len(names) < 5:
                raise ValueError("site layer 'elevation' needs MAPPING.ELEVATION.ENABLED")
            return 0b11110
        raise ValueError("site layer must be 'map' or 'elevation', not %r" % (layer,))

    def site_tiles(self, layer="map"):
        self.retire()
        bits = self._layer_bits(layer)
        tiles = {t for t, m in self._window_nonempty().items() if m & bits}
        tiles |= {t for t, m in self.nonempty.items() if m & bits}
        return sorted(tiles)

    def _homes(self, tiles):
        """where each tile of ``tiles`` lives: "window" (the window is valid and covers it), "store" (it has a slab) or None"""
        a, b = self.origin[0] // self.T, self.origin[1] // self.T
        a1, b1 = (a + self.Ht, b + self.Wt) if self.window_valid else (a, b)          # not valid: the window covers nothing
        stored = self.directory
        return ["window" if a <= t[0] < a1 and b <= t[1] < b1 else "store" if t in stored else None for t in tiles]

    def _gather_jobs(self, L, tiles, dst_ref):
        """one job per tile of ``tiles`` from wherever the tile lives (_homes; nowhere = fill) to dst_ref(k) = (key, off, pitch)"""
        T = self.T
        origin_tile = (self.origin[0] // T, self.origin[1] // T)
        jobs = []
        for k, (t, home) in enumerate(zip(tiles, self._homes(tiles))):
            dk, do, dp = dst_ref(k)
            if home == "window":
                so, sp = window_ref(t, origin_tile, T, self.Wm, L.bpc)
                jobs.append(Job("window", so, sp, dk, do, dp, -1))
            elif home == "store":
                sk, so, sp = slab_ref(self.directory[t], self.chunk_tiles, T, L.bpc)
                jobs.append(Job(sk, so, sp, dk, do, dp, -1))
            else:
                jobs.append(Job(None, 0, 0, dk, do, dp, -1))
        return jobs

    def site_map(self, rect=None, layer="map", stream=None):
        torch = self.torch
        self.retire()
        bits = self._layer_bits(layer)
        layers = [L for l, L in enumerate(self._layers()) if bits >> l & 1]
        if rect is None:
            tiles = self.site_tiles(layer)
            if not tiles:
                rect = (0, -1, 0, -1)
            else:
                rect = (min(t[0] for t in tiles), max(t[0] for t in tiles), min(t[1] for t in tiles), max(t[1] for t in tiles))
        T = self.T
        ti0, tj0 = int(rect[0]), int(rect[2])
        nh, nw = rect_shape(rect, T)
        st = self._stream(stream)
        outs, per_layer = [], []
        tiles = [(ti0 + i, tj0 + j) for i in range(nh) for j in range(nw)]
        for L in layers:
            cur = L.get()
            with torch.cuda.stream(st):
                out = torch.empty((nh * T, nw * T) + tuple(cur.shape[2:]), dtype=cur.dtype, device=cur.device)
            outs.append(out)
            pitch = nw * T * L.bpc

            def dst_ref(k, pitch=pitch, bpc=L.bpc):
                return "out", ((k // nw) * T * nw * T + (k % nw) * T) * bpc, pitch
            jobs = self._gather_jobs(L, tiles, dst_ref)
            per_layer.append((L, jobs, self._buffers(L, {"window": self._extent(cur), "out": self._extent(out)})))
        if tiles:
            self._run(per_layer, st)
        return (ti0 * T, tj0 * T), (outs[0] if layer == "map" else tuple(outs))

    def overview_table(self, rect=None, sources=overview_sources):
        """-> (rect, source table, buffers) of the map layer: overview_sources on the window's non-empty tiles and the store's
        directory and masks (``sources`` = finish_sources: the finish's record table instead).  ``rect`` None = the bounding rectangle
        of what holds something, (0, -1, 0, -1) for an empty site."""
        self.retire()
        L = self._layers()[0]
        T = self.T
        window = (self._window_masks(1) & 1).astype(bool) if self.window_valid else None
        masks = np.fromiter(self.nonempty.values(), dtype=np.int64, count=len(self.nonempty))
        tiles = np.array(list(self.nonempty), dtype=np.int64).reshape(-1, 2)
        slabs = np.fromiter(map(self.directory.__getitem__, self.nonempty), dtype=np.int64, count=len(self.nonempty))
        has_map = (masks & 1) != 0
        tiles, slabs = tiles[has_map], slabs[has_map]
        origin_tile = (self.origin[0] // T, self.origin[1] // T)
        if rect is None:
            wi, wj = np.nonzero(window) if window is not None else (np.zeros(0, dtype=np.int64),) * 2
            ti = np.concatenate([wi + origin_tile[0], tiles[:, 0]])
            tj = np.concatenate([wj + origin_tile[1], tiles[:, 1]])
            rect = (int(ti.min()), int(ti.max()), int(tj.min()), int(tj.max())) if ti.size else (0, -1, 0, -1)
        rect = tuple(int(v) for v in rect)
        table = sources(rect, T, L.bpc, self.Wm, origin_tile, window, tiles, slabs, self.chunk_tiles)
        buffers = [self._extent(L.get())] + [(c.data_ptr(), int(c.numel())) for c in L.chunks]
        return rect, table, buffers

    def _site_render_params(self, colors, thresholds, priority):
        """renderer.render_params for the site calls: no or no thresholds at all mean the arg-max renderer, and a priority without
        thresholds is ignored"""
        from . import renderer
        if thresholds is None or not len(thresholds):
            thresholds = priority = None
        return renderer.render_params(self.sm.label_colors if colors is None else colors, self.C, thresholds, priority)

    def site_overview(self, cells_per_pixel, rect=None, colors=None, thresholds=None, priority=None, reduced=False, out=None, stream=None,
                      max_side_px=4096):
        import ctypes as C
        from . import _lib, renderer
        torch = self.torch
        sm = self.sm
        rect, table, buffers = self.overview_table(rect)
        T, Cn = self.T, self.C
        nh, nw = rect_shape(rect, T)
        origin = (rect[0] * T, rect[2] * T)
        k = int(cells_per_pixel) if cells_per_pixel else overview_cells_per_pixel(T, nh, nw, int(max_side_px))
        if k < 1 or T % k != 0:
            raise ValueError("site_overview: cells_per_pixel = %d does not divide the tile size T = %d" % (k, T))
        P = T // k
        if nh * P * nw * P >= 1 << 31:
            raise ValueError("site_overview: a picture of %d x %d pixels; choose more cells per pixel than %d" % (nh * P, nw * P, k))
        st = self._stream(stream)
        cur = self._layers()[0].get()
        with torch.cuda.stream(st):
            out = renderer.out_picture(out, nh * P, nw * P, cur.device)
            red = torch.empty((nh * P, nw * P, Cn), dtype=cur.dtype, device=cur.device) if reduced else None
        result = (origin, out, red) if reduced else (origin, out)
        sm.last_site_overview = {"rect": rect, "cells_per_pixel": k, "tiles": len(table)}
        if nh == 0 or nw == 0:
            return result                                                  # an empty site: nothing is launched
        validate_sources(table, buffers, T, self._layers()[0].bpc, nh, nw)  # raises before anything is uploaded or launched
        col, pr, th = self._site_render_params(colors, thresholds, priority)
        dt = _lib.AVL_F64 if cur.dtype == torch.float64 else _lib.AVL_F32

        def launch(tiles):
            rc = _lib.lib().avl_site_overview(C.c_void_p(tiles), len(table), nh, nw, T, Cn, dt, k, col, pr, th, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(red.data_ptr()) if reduced else None, C.c_void_p(st.cuda_stream))
            _lib.check(rc, "avl_site_overview")
        self._launch_table(st, max(len(table), 1) * SRC_DTYPE.itemsize, lambda rec: encode_sources(table, buffers, rec.view(SRC_DTYPE)), launch)
        return result

    def site_finish(self, rect=None, colors=None, filter=True, thresholds=None, priority=None, truth=None, picture=True, labels=False,
                    out=None, stream=None):
        """-> SiteFinish: the rule of struct avl_tile_fin (include/avl_hip.h) on the tile rectangle ``rect``, one launch.  The kernel
        counts the tiles with a record; the truth histograms of the rectangle's other tiles (``truth.tile_hist``, exact integers)
        are added on the host into label 0.  The window and the store are only read."""
        import ctypes as C
        from . import _lib, renderer
        torch = self.torch
        rect, table, buffers = self.overview_table(rect, finish_sources)
        T, Cn = self.T, self.C
        nh, nw = rect_shape(rect, T)
        origin = (rect[0] * T, rect[2] * T)
        H, W = nh * T, nw * T
        if H * W >= 1 << 31:
            raise ValueError("site_finish: a rectangle of %d x %d cells (below 2^31)" % (H, W))
        if out is not None and not picture:
            raise ValueError("site_finish: out must be given with picture=True")
        st = self._stream(stream)
        cur = self._layers()[0].get()
        with torch.cuda.stream(st):
            pic = renderer.out_picture(out, H, W, cur.device) if picture else None
            lab = torch.empty((H, W), dtype=torch.uint8, device=cur.device) if labels else None
        n = len(table)
        n_null = int((table["buf"] < 0).sum())
        tiles = (n - n_null, n_null)
        counts = None
        if truth is not None:                                              # the tiles without a record: truth against label 0
            counts = np.zeros((8, 8), dtype=np.int64)
            if nh == 0 or nw == 0:                                         # an empty site: nothing was mapped, all of the truth is missed
                counts[:, 0] = truth.total_hist()
            else:
                counts[:, 0] = truth.rect_hist(T, rect) - truth.tiles_hist(T, table["row"].astype(np.int64) + rect[0],
                                                                           table["col"].astype(np.int64) + rect[2])
        if nh == 0 or nw == 0 or (pic is None and lab is None and truth is None):
            return SiteFinish(origin, pic, lab, counts, tiles)             # an empty site, or nothing asked for: nothing is launched
        validate_finish(table, buffers, T, self._layers()[0].bpc, nh, nw)  # raises before anything is uploaded or launched
        col, pr, th = self._site_render_params(colors, thresholds, priority)
        gt = mask = cnt = None
        Hg = Wg = r0 = c0 = 0
        if truth is not None:
            gt, mask = truth.on(cur.device)
            Hg, Wg = int(gt.shape[0]), int(gt.shape[1])
            r0, c0 = truth.origin_cell[0] - origin[0], truth.origin_cell[1] - origin[1]
            if max(abs(r0), abs(c0)) >= 1 << 31:
                raise ValueError("site_finish: the truth raster starts %d, %d cells from the rectangle" % (r0, c0))
            with torch.cuda.stream(st):
                cnt = torch.empty(64, dtype=torch.int64, device=cur.device)
        dt = _lib.AVL_F64 if cur.dtype == torch.float64 else _lib.AVL_F32
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

        def launch(records):
            rc = _lib.lib().avl_site_finish(C.c_void_p(records), n, nh, nw, T, Cn, dt, _lib.AVL_LIVE_FILTER if filter else 0, col, pr, th,
                                            p(gt), Hg, Wg, Wg, r0, c0, p(mask), Wg, p(pic), p(lab), p(cnt), C.c_void_p(st.cuda_stream))
            _lib.check(rc, "avl_site_finish")
        self._launch_table(st, max(n, 1) * FIN_DTYPE.itemsize, lambda rec: encode_finish(table, buffers, rec.view(FIN_DTYPE)), launch)
        if cnt is not None:
            with torch.cuda.stream(st):
                counts += cnt.cpu().numpy().reshape(8, 8)                  # waits for the kernel: the counts are a host result
        return SiteFinish(origin, pic, lab, counts, tiles)

    def _pack(self, st):
        """-> (coords, outs): per layer the sorted non-empty tiles of the whole site, the window's own included, and a device tensor
        [n, T, T, ...] of them, gathered by the tile-job kernel on ``st``"""
        torch = self.torch
        self.retire()
        T = self.T
        window = self._window_nonempty()
        masks = dict(self.nonempty)
        masks.update(window)                                   # a tile is in the window or in the store, never both
        outs, per_layer, coords = [], [], []
        for l, L in enumerate(self._layers()):
            tiles = sorted(t for t, m in masks.items() if m >> l & 1)
            cur = L.get()
            with torch.cuda.stream(st):
                out = torch.empty((len(tiles), T, T) + tuple(cur.shape[2:]), dtype=cur.dtype, device=cur.device)
            slab = T * T * L.bpc
            jobs = self._gather_jobs(L, tiles, lambda k, slab=slab, bpc=L.bpc: ("out", k * slab, T * bpc))
            coords.append(tiles)
            outs.append(out)
            if tiles:
                per_layer.append((L, jobs, self._buffers(L, {"window": self._extent(cur), "out": self._extent(out)})))
        if per_layer:
            self._run(per_layer, st)
        return coords, outs

    def _dtype_name(self):
        return "f64" if self.sm.grid_dtype == "f64" else "f32"

    def save_site(self, path, stream=None):
        st = self._stream(stream)
        coords, outs = self._pack(st)
        st.synchronize()
        arrays = pack_site(self.anchor, self.res, self.T, self.C, self._dtype_name(),
                           {L.name: (np.array(c, dtype=np.int64).reshape(-1, 2), o.cpu().numpy()) for L, c, o in zip(self._layers(), coords, outs)})
        with open(path, "wb") as f:
            np.savez_compressed(f, **arrays)

    def _reset(self, st):
        """the store starts over: every slab free, the window empty (not valid) at origin (0, 0), its buffers cleared on ``st``"""
        sm = self.sm
        g = sm.grid
        self._layers()
        self.directory, self.nonempty = {}, {}
        self.free = list(range(self.n_slabs - 1, -1, -1))
        with self.torch.cuda.stream(st):
            g.map.zero_()
            if sm.elevation_enabled():
                sm.reset_elevation(st.cuda_stream)
        self.origin, self.first, self.window_valid, self.band = (0, 0), True, False, None
        self.exchanged = False
        boundary = window_boundary(self.anchor, (0, 0), self.Hm, self.Wm, self.res)
        g.boundary = boundary
        sm.map_boundary = boundary
        sm._map_host = None
        sm.scroll_origin = (0, 0)

    def load_site(self, path, stream=None):
        torch = self.torch
        sm = self.sm
        with np.load(path) as data:
            meta, file_layers = unpack_site(data, self.anchor, self.res, self.T, self.C, self._dtype_name())
        layers = self._layers()
        if sorted(file_layers) != sorted(L.name for L in layers):
            raise ValueError("the site file holds the layers %r, this map %r" % (sorted(file_layers), sorted(L.name for L in layers)))
        self.retire()
        st = self._stream(stream)
        self._reset(st)
        union = sorted({(int(c[0]), int(c[1])) for coords, _ in file_layers.values() for c in coords})
        for t in union:
            check_origin((t[0] * self.T, t[1] * self.T), self.T)
        slabs = dict(zip(union, self._slabs(len(union))))
        per_layer, keep = [], []
        T = self.T
        for l, L in enumerate(layers):
            coords, tiles = file_layers[L.name]
            cur = L.get()
            want = (T, T) + tuple(cur.shape[2:])
            if tiles.shape[0] and (tuple(tiles.shape[1:]) != want or torch.from_numpy(tiles[:0]).dtype != cur.dtype):
                raise ValueError("the site file's layer %r has tiles %s %s, this map %s %s" % (L.name, tiles.shape[1:], tiles.dtype, want, cur.dtype))
            with torch.cuda.stream(st):
                stage = torch.from_numpy(np.ascontiguousarray(tiles)).to(sm.device) if tiles.shape[0] else torch.empty(16, dtype=torch.uint8, device=sm.device)
            keep.append(stage)
            have = {(int(c[0]), int(c[1])): k for k, c in enumerate(coords)}
            jobs = []
            for t in union:
                dk, do, dp = slab_ref(slabs[t], self.chunk_tiles, T, L.bpc)
                if t in have:
                    jobs.append(Job("stage", have[t] * T * T * L.bpc, T * L.bpc, dk, do, dp, -1))
                    self.nonempty[t] = self.nonempty.get(t, 0) | 1 << l
                else:
                    jobs.append(Job(None, 0, 0, dk, do, dp, -1))
            per_layer.append((L, jobs, self._buffers(L, {"stage": self._extent(stage)})))
        if union:
            self._run(per_layer, st)
        self.directory = slabs
        for s in keep:
            s.record_stream(st)
        return meta

    # -------------------------------------------------------------------------------------------- merging sites
    def _check_site(self, file_layers, src_dtypes=None):
        """ValueError, naming the numbers, unless ``file_layers`` = {name: (coords, tiles)} can be merged into this map: its layers,
        tiles of this map's shape and type (``src_dtypes``: {layer: torch dtype} where the exchange form brings another), tile
        coordinates unique per layer and inside check_origin's range.  -> {name: [(ti, tj)]}"""
        T = self.T
        specs = [("map", (self.C,), "float64" if self._dtype_name() == "f64" else "float32")]      # from the configuration: nothing
        if self.sm.elevation_enabled():                                                           # is allocated for a refusal
            specs += [(L.name, (), "int64" if L.bpc == 8 else "int32") for L in ELEVATION_LAYERS]
        if sorted(file_layers) != sorted(name for name, _, _ in specs):
            raise ValueError("the site to merge holds the layers %r, this map %r" % (sorted(file_layers), sorted(name for name, _, _ in specs)))
        out = {}
        for name, tail, own_dtype in specs:
            coords, tiles = file_layers[name]
            want = (T, T) + tail
            want_dtype = str((src_dtypes or {}).get(name, own_dtype)).replace("torch.", "")
            dtype = str(tiles.dtype).replace("torch.", "")
            if len(coords) != int(tiles.shape[0]) or (len(coords) and (tuple(tiles.shape[1:]) != want or dtype != want_dtype)):
                raise ValueError("the site to merge has %d coordinates and tiles %s %s in layer %r, this map tiles %s %s"
                                 % (len(coords), tuple(tiles.shape), dtype, name, want, want_dtype))
            ts = [(int(c[0]), int(c[1])) for c in np.asarray(coords).reshape(-1, 2)]
            seen = {}
            for k, t in enumerate(ts):
                if t in seen:
                    raise ValueError("the site to merge names tile (%d, %d) of layer %r twice, at %d and %d" % (t[0], t[1], name, seen[t], k))
                seen[t] = k
                check_origin((t[0] * T, t[1] * T), T)
            out[name] = ts
        return out

    def merge_site(self, site, stream=None):
        if isinstance(site, dict):
            data = site
        else:
            with np.load(site) as f:
                data = {k: f[k] for k in f.files}
        meta, file_layers = unpack_site(data, self.anchor, self.res, self.T, self.C, self._dtype_name())
        tiles = self._check_site(file_layers)
        return self._merge(file_layers, tiles, self._stream(stream))

    def _merge(self, file_layers, tiles_of, st, src_dtypes=None):
        """``file_layers`` (checked: ``tiles_of`` is _check_site's answer) summed into this site, one avl_tile_merge launch per layer on
        ``st``; waits for the result flags.  -> SiteMerge"""
        torch = self.torch
        sm = self.sm
        self.retire()
        layers = self._layers()
        T = self.T
        a, b = self.origin[0] // T, self.origin[1] // T
        union = sorted({t for ts in tiles_of.values() for t in ts})
        kinds = {t: home or "fresh" for t, home in zip(union, self._homes(union))}
        new = [t for t in union if kinds[t] == "fresh"]
        slabs = dict(zip(new, self._slabs(len(new))))
        per_layer, keep, bits = [], [], []
        try:
            for l, L in enumerate(layers):
                coords, tiles = file_layers[L.name]
                have = {t: k for k, t in enumerate(tiles_of[L.name])}
                cur = L.get()
                src_dtype = (src_dtypes or {}).get(L.name, cur.dtype)
                src_bpc = L.bpc * torch.empty(0, dtype=src_dtype).element_size() // cur.element_size()
                lacking = [t for t in new if t not in have]           # a new slab the file has nothing for: fill (+) fill = fill
                n = len(have)
                with torch.cuda.stream(st):
                    if torch.is_tensor(tiles):
                        stage = tiles.contiguous().view(torch.uint8).reshape(-1)
                    else:
                        stage = torch.from_numpy(np.ascontiguousarray(tiles)).to(sm.device).view(torch.uint8).reshape(-1)
                    if lacking:
                        empty = torch.full((T * T * src_bpc // 4,), fill_int32(L.fill), dtype=torch.int32, device=sm.device).view(torch.uint8)
                        stage = torch.cat([stage, empty])
                keep.append(stage)
                entries = []                                           # none for a tile that exists and gets nothing in this layer
                for k, t in enumerate(union):
                    if t in have:
                        entries.append((t, have[t], kinds[t], slabs[t] if t in slabs else self.directory.get(t), k))
                    elif t in slabs:
                        entries.append((t, n, "fresh", slabs[t], k))
                jobs = merge_jobs(entries, T, self.Wm, L.bpc, self.chunk_tiles, (a, b), src_bpc)
                op = merge_op(L.name, self._dtype_name(), "f32" if src_dtype == torch.float32 and L.name == "map" else None)
                if jobs:
                    per_layer.append((L, jobs, self._buffers(L, {"window": self._extent(cur), "stage": self._extent(stage)}), op, src_bpc))
                    bits.append(1 << l)                                # the layer's bit in a tile's nonempty mask
            if per_layer:
                self._run(per_layer, st, len(union))
        except Exception:
            self.free.extend(slabs.values())
            raise
        for s in keep:
            s.record_stream(st)
        self.directory.update(slabs)
        counts = collections.Counter(kinds.values())
        freed = 0
        if per_layer:
            self.flags_event.synchronize()                             # merging is rare: the call waits for its flags
            flags = self.flags_host[:len(per_layer) * len(union)].numpy().reshape(len(per_layer), len(union))
            masks = {t: self.nonempty.get(t, 0) for t in union if kinds[t] != "window"}
            for p, (_, jobs, _, _, _) in enumerate(per_layer):         # a layer's bit follows the result where the layer had a job
                for j in jobs:
                    if j.flag >= 0:
                        t = union[j.flag]
                        masks[t] = masks[t] & ~bits[p] | (bits[p] if flags[p, j.flag] else 0)
            for t, mask in masks.items():
                if mask:
                    self.nonempty[t] = mask
                else:                                                  # empty in every layer: as retire() does
                    self.free.append(self.directory.pop(t))
                    self.nonempty.pop(t, None)
                    freed += 1
        sm._map_host = None
        return SiteMerge(counts["window"], counts["store"], counts["fresh"], freed)

    def global_site(self, group=None, exchange_dtype=None, stream=None):
        from . import distributed as D
        torch = self.torch
        if self.exchanged:
            raise RuntimeError("global_site() has run on this map: the site already holds the other ranks' frames, a second exchange "
                               "would count them again")
        layers = self._layers()
        cur = layers[0].get()
        src_dtypes = {}
        if exchange_dtype is not None and exchange_dtype != cur.dtype:
            if (cur.dtype, exchange_dtype) != (torch.float64, torch.float32):
                raise ValueError("global_site: exchange_dtype %s on a %s map (torch.float32 on a float64 map, or None)" % (exchange_dtype, cur.dtype))
            src_dtypes["map"] = exchange_dtype
        st = self._stream(stream)
        coords, outs = self._pack(st)
        gathered, sent = [], 0
        with torch.cuda.stream(st):
            for L, c, o in zip(layers, coords, outs):
                if L.name in src_dtypes:
                    o = o.to(src_dtypes[L.name])                       # the copy that travels: half the payload
                ct = torch.tensor(c, dtype=torch.int64, device=o.device).reshape(-1, 2)
                parts = D.gather_sites(ct, o, group=group)
                longest = max(int(p[0].shape[0]) for p in parts)
                if len(parts) > 1:                                     # one rank: nothing travels
                    sent += 8 + longest *(16 + int(np.prod(o.shape[1:])) * o.element_size())     # the count; coordinates and tiles, padded
                gathered.append(parts)
        sites = []
        for r in range(len(gathered[0])):                              # checked before the store is reset
            site = {L.name: (gathered[l][r][0].cpu().numpy(), gathered[l][r][1]) for l, L in enumerate(layers)}
            sites.append((site, self._check_site(site, src_dtypes)))
        self._reset(st)
        self.exchanged = True
        merged = [self._merge(site, tiles_of, st, src_dtypes) for site, tiles_of in sites]   # ((empty + S_0) + S_1) + ...
        self.sm.last_exchange = ("tiles", sent)
        return merged
