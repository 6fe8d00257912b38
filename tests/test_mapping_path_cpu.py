"""avl_fused_frame_path: the vote / apply path avl_fused_frame picks (include/avl_hip.h), pinned case by case.  The function looks
at sizes and pointer values only, so the grids here carry fake, never dereferenced pointers and no GPU is needed.  Every expected
value below is worked out by hand from the rule as the header states it (csrc/mapping.hip: byte_mask_ok, list_geom, use_lists,
use_scan); the bench's mapping configurations depend on these choices, so a change of the heuristics has to show up here."""
import ctypes as C

import pytest

MASK = 0x7f0000100000          # 16-byte aligned fake addresses
BIG_CAP = 1 << 30


def grid(Hm, Wm, C_=5, touched_cap=BIG_CAP, counter_len=256, mask=MASK, map_dtype=None):
    from vision_semantic_segmentation_amd import _lib
    g = _lib.AvlGrid()
    g.map, g.touched, g.counter = 0x7f0000200000, 0x7f0000300000, 0x7f0000400000
    g.cell_mask = mask
    g.map_dtype = _lib.AVL_F64 if map_dtype is None else map_dtype
    g.Hm, g.Wm, g.C = Hm, Wm, C_
    g.off_x, g.off_y, g.b00, g.b10, g.resolution = 1369.0496826171875, 562.84814453125, 1244.0, 437.0, 0.25
    g.touched_cap, g.counter_len = touched_cap, counter_len
    return g


def path(g, n, bonus):
    from vision_semantic_segmentation_amd import _lib
    return _lib.lib().avl_fused_frame_path(C.byref(g), n, bonus)


LANE2 = 1 << 2                 # the default label set: one "lane" class at index 2
TWO_LANES_6 = (1 << 2) | (1 << 5)

# list capacity of n points: ceil(ceil(n / 256) / 64) * 256 entries per list, 64 lists
#   n = 30000: 118 workgroups -> 2 per list -> 64 x 512 = 32768;  n = 100000: 391 -> 7 -> 64 x 1792 = 114688
#   n = 250000: 977 -> 16 -> 262144;  n = 20000: 79 -> 2 -> 32768;  n = 1023: 4 -> 1 -> 16384
CASES = [
    # (id, grid kwargs, n, bonus, expected path)
    # C + popcount(bonus): 8 bits keep the byte mask, 9 do not (1000 x 1000: cells % 16 == 0; 30000 * 128 >= 1e6 -> sweep)
    ("c5_one_lane_6_bits", dict(Hm=1000, Wm=1000, C_=5), 30000, LANE2, 3),
    ("c6_two_lanes_8_bits", dict(Hm=1000, Wm=1000, C_=6), 30000, TWO_LANES_6, 3),
    ("c8_no_lane_8_bits", dict(Hm=1000, Wm=1000, C_=8), 30000, 0, 3),
    ("c8_one_lane_9_bits", dict(Hm=1000, Wm=1000, C_=8), 30000, 1, 1),
    ("c7_two_lanes_9_bits", dict(Hm=1000, Wm=1000, C_=7), 30000, (1 << 2) | (1 << 6), 1),
    ("c16_lanes_0_15", dict(Hm=1000, Wm=1000, C_=16), 30000, 1 | (1 << 15), 1),
    ("c7_two_lanes_9_bits_sparse", dict(Hm=1000, Wm=1000, C_=7), 7812, (1 << 2) | (1 << 6), 0),      # 7812 * 128 < 1e6
    ("c7_two_lanes_9_bits_at_sweep", dict(Hm=1000, Wm=1000, C_=7), 7813, (1 << 2) | (1 << 6), 1),    # 7813 * 128 >= 1e6
    # Hm*Wm % 16 == 4 (1004004 cells): no byte mask, the 32-bit sweep from n * 128 >= cells (n >= 7844)
    ("cells_mod16_4_dense", dict(Hm=1002, Wm=1002), 30000, LANE2, 1),
    ("cells_mod16_4_at_sweep", dict(Hm=1002, Wm=1002), 7844, LANE2, 1),
    ("cells_mod16_4_below_sweep", dict(Hm=1002, Wm=1002), 7843, LANE2, 0),
    # odd cell count (999999): no sweep at all
    ("odd_cells_sparse", dict(Hm=999, Wm=1001), 30000, LANE2, 0),
    ("odd_cells_dense", dict(Hm=999, Wm=1001), 600000, LANE2, 0),
    # cell_mask 4 bytes off 16-byte alignment: neither the byte mask nor a sweep
    ("mask_misaligned_sparse", dict(Hm=1000, Wm=1000, mask=MASK + 4), 30000, LANE2, 0),
    ("mask_misaligned_dense", dict(Hm=1000, Wm=1000, mask=MASK + 4), 600000, LANE2, 0),
    # n <= 250000 for the lists
    ("n_250000", dict(Hm=1000, Wm=1000), 250000, LANE2, 3),
    ("n_250001", dict(Hm=1000, Wm=1000), 250001, LANE2, 2),
    # 2n <= cells for the lists (200 x 200 = 40000 cells)
    ("two_n_eq_cells", dict(Hm=200, Wm=200), 20000, LANE2, 3),
    ("two_n_eq_cells_plus_2", dict(Hm=200, Wm=200), 20001, LANE2, 2),
    # n * 1024 (byte mask) and n * 128 (32-bit mask) either side of the cells (1024 x 1024 = 1048576), lists off (counter_len 131)
    ("byte_sweep_n_1024", dict(Hm=1024, Wm=1024, counter_len=131), 1024, LANE2, 2),
    ("byte_sweep_n_1023", dict(Hm=1024, Wm=1024, counter_len=131), 1023, LANE2, 0),
    ("word_sweep_n_8192", dict(Hm=1024, Wm=1024, C_=16), 8192, 0, 1),
    ("word_sweep_n_8191", dict(Hm=1024, Wm=1024, C_=16), 8191, 0, 0),
    ("lists_need_no_density", dict(Hm=1024, Wm=1024), 1023, LANE2, 3),
    # counter_len >= 4 + 2 x 64 for the lists
    ("counter_len_132", dict(Hm=1000, Wm=1000, counter_len=132), 30000, LANE2, 3),
    ("counter_len_131", dict(Hm=1000, Wm=1000, counter_len=131), 30000, LANE2, 2),
    # touched_cap >= 64 x cap
    ("touched_cap_one_short", dict(Hm=1000, Wm=1000, touched_cap=32767), 30000, LANE2, 2),
    ("touched_cap_exact", dict(Hm=1000, Wm=1000, touched_cap=32768), 30000, LANE2, 3),
    ("touched_cap_one_short_100k", dict(Hm=1000, Wm=1000, touched_cap=114687), 100000, LANE2, 2),
    ("touched_cap_exact_100k", dict(Hm=1000, Wm=1000, touched_cap=114688), 100000, LANE2, 3),
    # the dense grid of the GPU tests (160 x 160 = 25600 cells)
    ("dense_160_byte", dict(Hm=160, Wm=160), 20000, LANE2, 2),
    ("dense_160_word", dict(Hm=160, Wm=160, C_=7), 20000, (1 << 2) | (1 << 6), 1),
    ("f32_grid_same_rule", dict(Hm=1000, Wm=1000, map_dtype=0), 30000, LANE2, 3),
]


@pytest.mark.parametrize("kw,n,bonus,want", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_fused_frame_path_rule(kw, n, bonus, want):
    assert path(grid(**kw), n, bonus) == want


def test_fused_frame_path_refuses_what_the_frame_refuses():
    from vision_semantic_segmentation_amd import _lib
    cases = [
        (grid(1000, 1000, C_=0), 10, 0, "C must be"),
        (grid(1000, 1000, C_=17), 10, 0, "C must be"),
        (grid(1000, 1000, C_=5), 10, 1 << 5, "bonus_classes"),
        (grid(1000, 1000, map_dtype=7), 10, 0, "map dtype"),
        (grid(1000, 1000), -1, 0, "n = -1"),
    ]
    g = grid(1000, 1000)
    g.cell_mask = None
    cases.append((g, 10, 0, "NULL"))
    for g, n, bonus, msg in cases:
        assert path(g, n, bonus) == -1
        assert msg in _lib.last_error(), (msg, _lib.last_error())


# ---------------------------------------------------------------- cm_host is checked before the empty cloud returns
# one grid per path, from CASES (every one with 6 vote bits, so that two views take it as well)
EMPTY_CLOUD_GRIDS = [("odd_cells_sparse", 0), ("cells_mod16_4_dense", 1), ("counter_len_131", 2), ("c5_one_lane_6_bits", 3)]


def _empty_frame(g, bonus, cm, n_views=None):
    """avl_fused_frame (or avl_fused_frame_views with n_views views) on an EMPTY cloud: n = 0 returns before any HIP call, so the fake
    pointers are never handed to a device.  -> (rc, message)"""
    from vision_semantic_segmentation_amd import _lib
    L = _lib.lib()
    P = (C.c_double * (12 * (n_views or 1)))()
    lut, colors = (C.c_uint32 * 256)(), (C.c_uint8 * 48)()
    cm_c = (C.c_double * 256)() if cm else None
    head = (C.byref(g), 0x7f0000500000, 0, _lib.AVL_F32, 16, 4)
    tail = (640, 480, 640, 480, lut, colors, cm_c, bonus, None)
    if n_views is None:
        rc = L.avl_fused_frame(*head, P, None, 100.0, _lib.AVL_SRC_CLASSMAP, 0x7f0000600000, *tail)
    else:
        src = (C.c_void_p * n_views)(*[0x7f0000600000 + 0x100000 * v for v in range(n_views)])
        rc = L.avl_fused_frame_views(*head, n_views, P, None, 100.0, _lib.AVL_SRC_CLASSMAP, src, *tail)
    return rc, _lib.last_error()


@pytest.mark.parametrize("case_id,want_path", EMPTY_CLOUD_GRIDS, ids=["path%d" % p for _, p in EMPTY_CLOUD_GRIDS])
@pytest.mark.parametrize("n_views", [None, 2], ids=["single", "two_views"])
def test_null_cm_host_is_refused_on_every_path(case_id, want_path, n_views):
    """a NULL cm_host is AVL_E_ARG from both fused entry points whatever path the grid would take (path 3 used to read through it),
    and a valid one still maps the empty cloud"""
    kw, n, bonus, want = {c[0]: c[1:] for c in CASES}[case_id]
    assert want == want_path and path(grid(**kw), n, bonus) == want_path
    rc, err = _empty_frame(grid(**kw), bonus, cm=False, n_views=n_views)
    assert rc == -1, (rc, err)
    assert "cm_host is NULL" in err, err
    rc, err = _empty_frame(grid(**kw), bonus, cm=True, n_views=n_views)
    assert rc == 0, (rc, err)
