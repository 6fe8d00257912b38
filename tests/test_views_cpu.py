"""avl_fused_frame_views without a GPU: the symbol from the header to the ctypes shim, every argument refusal with its message
(argument errors return before anything touches the device, so the grids carry fake, never dereferenced pointers as in
tests/test_mapping_path_cpu.py), the path rule of avl_fused_frame_views_path worked out by hand from the header's statement, and
the bookkeeping of SemanticMapping.mapping_views / image_callback_views around a stubbed frame_device_views."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MASK = 0x7f0000100000          # 16-byte aligned fake addresses
PTS = 0x7f0000500000
SRC = (0x7f0000600000, 0x7f0000700000, 0x7f0000800000, 0x7f0000900000, 0x7f0000a00000)
BIG_CAP = 1 << 30
LANE2 = 1 << 2


def grid(Hm=1000, Wm=1000, C_=5, touched_cap=BIG_CAP, counter_len=256, mask=MASK, map_dtype=None):
    from vision_semantic_segmentation_amd import _lib
    g = _lib.AvlGrid()
    g.map, g.touched, g.counter = 0x7f0000200000, 0x7f0000300000, 0x7f0000400000
    g.cell_mask = mask
    g.map_dtype = _lib.AVL_F64 if map_dtype is None else map_dtype
    g.Hm, g.Wm, g.C = Hm, Wm, C_
    g.off_x, g.off_y, g.b00, g.b10, g.resolution = 1369.0496826171875, 562.84814453125, 1244.0, 437.0, 0.25
    g.touched_cap, g.counter_len = touched_cap, counter_len
    return g


def test_symbol_is_declared_exported_and_bound():
    from vision_semantic_segmentation_amd import _lib
    text = open(os.path.join(ROOT, "include", "avl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("avl_fused_frame_views", "avl_fused_frame_views_path"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.exported_symbols()
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int
    assert len(_lib.lib().avl_fused_frame_views.argtypes) == 21
    assert re.search(r"#define\s+AVL_MAX_VIEWS\s+4\b", text) and _lib.AVL_MAX_VIEWS == 4


def call(g=None, pts=PTS, n=1000, dtype=None, pstride=16, cstride=4, n_views=2, P=True, T=None, src_kind=None, src=SRC, src_w=640, src_h=480,
         img_w=640, img_h=480, lut=True, colors=True, cm=True, bonus=LANE2):
    """avl_fused_frame_views with valid arguments except the ones given -> (rc, message)"""
    from vision_semantic_segmentation_amd import _lib
    g = grid() if g is None else g
    dtype = _lib.AVL_F32 if dtype is None else dtype
    src_kind = _lib.AVL_SRC_CLASSMAP if src_kind is None else src_kind
    P_c = (C.c_double * (12 * max(n_views, 1)))() if P else None
    src_c = None if src is None else (C.c_void_p * max(len(src), 1))(*src)
    lut_c = (C.c_uint32 * 256)() if lut else None
    col_c = (C.c_uint8 * 48)() if colors else None
    cm_c = (C.c_double * 256)() if cm else None
    rc = _lib.lib().avl_fused_frame_views(C.byref(g), pts, n, dtype, pstride, cstride, n_views, P_c, T, 100.0, src_kind, src_c, src_w, src_h,
                                          img_w, img_h, lut_c, col_c, cm_c, bonus, None)
    return rc, _lib.last_error()


REFUSALS = [
    # what the issue lists for the views
    ("n_views_0", dict(n_views=0), "n_views = 0"),
    ("n_views_negative", dict(n_views=-3), "n_views = -3"),
    ("n_views_over_limit", dict(n_views=5), "n_views = 5 exceeds the limit of 4"),
    ("src_host_null", dict(src=None), "src_host is NULL"),
    ("view_pointer_null", dict(n_views=3, src=(SRC[0], SRC[1], None)), "view 2: semantic source is NULL"),
    ("first_view_pointer_null", dict(src=(None, SRC[1])), "view 0: semantic source is NULL"),
    ("nine_vote_bits", dict(g=dict(C_=8), bonus=1), "= 9 vote bits"),
    ("nine_vote_bits_two_lanes", dict(g=dict(C_=7), bonus=(1 << 2) | (1 << 6)), "= 9 vote bits"),
    ("sixteen_classes", dict(g=dict(C_=16), bonus=0), "= 16 vote bits"),
    # everything avl_fused_frame refuses
    ("pts_null", dict(pts=None), "pts is NULL"),
    ("n_negative", dict(n=-1), "n = -1"),
    ("point_dtype", dict(dtype=7), "point dtype 7"),
    ("strides", dict(pstride=6), "point strides 6/4"),
    ("P_null", dict(P=False), "P_host is NULL"),
    ("image_size", dict(img_w=0), "image size 0x480"),
    ("grid_C_0", dict(g=dict(C_=0)), "C must be"),
    ("grid_C_17", dict(g=dict(C_=17)), "C must be"),
    ("grid_null_member", dict(g=dict(mask=None)), "NULL members"),
    ("map_dtype", dict(g=dict(map_dtype=7)), "map dtype 7"),
    ("bonus_beyond_C", dict(bonus=1 << 5), "bonus_classes has bits beyond C"),
    ("src_kind", dict(src_kind=2), "src_kind 2"),
    ("src_size", dict(src_w=0), "bad semantic source"),
    ("lut_null", dict(lut=False), "lut_host is NULL"),
    ("rgb_colors_null", dict(src_kind=0, colors=False), "label_colors_host is NULL"),
    ("rgb_size_differs", dict(src_kind=0, src_w=320), "RGB source must be 640x480"),
    ("cm_null", dict(cm=False), "cm_host is NULL"),
    ("touched_cap", dict(g=dict(touched_cap=999)), "touched_cap 999 too small"),
]


@pytest.mark.parametrize("kw,msg", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_argument_errors_return_before_the_gpu(kw, msg):
    kw = dict(kw)
    if "g" in kw:
        kw["g"] = grid(**kw["g"])
    rc, err = call(**kw)
    assert rc == -1, (rc, err)
    assert msg in err, (msg, err)


def test_one_view_forwards_to_the_single_view_entry():
    """n_views == 1 is avl_fused_frame: it takes 9 vote bits (the 32-bit mask) and refuses with avl_fused_frame's own messages"""
    rc, err = call(n_views=1, g=grid(C_=8), bonus=1, n=0)
    assert rc == 0, err
    rc, err = call(n_views=1, lut=False)
    assert rc == -1 and "lut_host is NULL" in err
    rc, err = call(n_views=2, n=0)                   # an empty cloud is valid and launches nothing
    assert rc == 0, err


def path(g, n, n_views, bonus=LANE2):
    from vision_semantic_segmentation_amd import _lib
    return _lib.lib().avl_fused_frame_views_path(C.byref(g), n, n_views, bonus)


# list capacity of n points: ceil(ceil(n / 256) / 64) * 256 entries per list, 64 lists (tests/test_mapping_path_cpu.py):
#   n = 30000 -> 64 x 512 = 32768;  n = 100000 -> 64 x 1792 = 114688;  n = 250000 -> 262144
PATH_CASES = [
    # (id, grid kwargs, n, n_views, bonus, expected)
    ("sparse_v2", dict(), 30000, 2, LANE2, 4),
    ("sparse_v4", dict(), 30000, 4, LANE2, 4),
    ("sparse_v3_f32_grid", dict(map_dtype=0), 30000, 3, LANE2, 4),
    ("config_C_120k_on_2000", dict(Hm=2000, Wm=2000), 120000, 2, LANE2, 4),
    ("config_E_1M_on_4000", dict(Hm=4000, Wm=4000), 1000000, 2, LANE2, 5),
    ("n_250000", dict(), 250000, 2, LANE2, 4),
    ("n_250001", dict(), 250001, 2, LANE2, 5),
    ("two_n_eq_cells", dict(Hm=200, Wm=200), 20000, 2, LANE2, 4),
    ("two_n_eq_cells_plus_2", dict(Hm=200, Wm=200), 20001, 2, LANE2, 5),
    ("counter_len_132", dict(counter_len=132), 30000, 2, LANE2, 4),
    ("counter_len_131", dict(counter_len=131), 30000, 2, LANE2, 5),
    ("touched_cap_exact", dict(touched_cap=32768), 30000, 2, LANE2, 4),
    ("touched_cap_one_short", dict(touched_cap=32767), 30000, 2, LANE2, 5),
    ("touched_cap_exact_100k", dict(touched_cap=114688), 100000, 4, LANE2, 4),
    ("touched_cap_one_short_100k", dict(touched_cap=114687), 100000, 4, LANE2, 5),
    # unlike the byte mask of the single-view paths, the word mask needs neither whole vectors nor alignment
    ("odd_cells_sparse", dict(Hm=999, Wm=1001), 30000, 2, LANE2, 4),
    ("odd_cells_dense", dict(Hm=999, Wm=1001), 600000, 2, LANE2, 5),
    ("mask_misaligned_sparse", dict(mask=MASK + 4), 30000, 2, LANE2, 4),
    ("mask_misaligned_dense", dict(mask=MASK + 4), 600000, 2, LANE2, 5),
    ("eight_bits_two_lanes", dict(C_=6), 30000, 2, (1 << 2) | (1 << 5), 4),
    ("n_0", dict(), 0, 2, LANE2, 4),
    # one view: the single-view rule (tests/test_mapping_path_cpu.py)
    ("v1_lists", dict(), 30000, 1, LANE2, 3),
    ("v1_byte_sweep", dict(), 250001, 1, LANE2, 2),
    ("v1_word_sweep_9_bits", dict(C_=8), 30000, 1, 1, 1),
    ("v1_single_list", dict(Hm=999, Wm=1001), 30000, 1, LANE2, 0),
]


@pytest.mark.parametrize("kw,n,n_views,bonus,want", [c[1:] for c in PATH_CASES], ids=[c[0] for c in PATH_CASES])
def test_views_path_rule(kw, n, n_views, bonus, want):
    assert path(grid(**kw), n, n_views, bonus) == want


def test_views_path_refuses_what_the_call_refuses():
    from vision_semantic_segmentation_amd import _lib
    cases = [
        (grid(), 10, 0, 0, "n_views = 0"),
        (grid(), 10, 5, 0, "n_views = 5 exceeds the limit of 4"),
        (grid(C_=8), 10, 2, 1, "= 9 vote bits"),
        (grid(C_=17), 10, 2, 0, "C must be"),
        (grid(), 10, 2, 1 << 5, "bonus_classes"),
        (grid(), -1, 2, 0, "n = -1"),
        (grid(), -1, 1, 0, "n = -1"),
        (grid(mask=None), 10, 2, 0, "NULL"),
    ]
    for g, n, v, bonus, msg in cases:
        assert path(g, n, v, bonus) == -1
        assert msg in _lib.last_error(), (msg, _lib.last_error())


# ---------------------------------------------------------------- SemanticMapping bookkeeping (no kernel runs)
class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __call__(self, pcd, pcd_frame_id, semantics, pose, cameras, **kw):
        self.calls.append((pcd, pcd_frame_id, list(semantics), pose, list(cameras), kw))


@pytest.fixture
def sm(monkeypatch):
    """a SemanticMapping on the CPU device with the device calls stubbed out: queues, records and flags are host code"""
    import torch
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    s = SemanticMapping(get_cfg_defaults(), device=torch.device("cpu"), logger=MyLogger("test", quiet=True))
    s.recorder = _Recorder()
    monkeypatch.setattr(s, "frame_device_views", s.recorder)
    monkeypatch.setattr(s, "_as_device_u8", lambda a: a)
    finished = []
    monkeypatch.setattr(s, "finish_run", lambda *a, **k: finished.append(len(s.recorder.calls)))
    s.finished = finished
    return s


def _msgs(frame_ids, secs=10):
    from vision_semantic_segmentation_amd.utils import Header, Message, Stamp
    return [Message(Header(Stamp(secs, 0), fid), data=np.full((4, 6, 3), k, dtype=np.uint8)) for k, fid in enumerate(frame_ids)]


def _feed(sm, stamps=(9, 10, 12)):
    from vision_semantic_segmentation_amd.utils import Header, Message, Stamp
    for k, t in enumerate(stamps):
        sm.pcd_callback(Message(Header(Stamp(t, 0), "velodyne"), points=np.full((4, 3), float(k))))
        sm.pose_callback(Message(Header(Stamp(t, 0)), pose="pose%d" % k))


def test_image_callback_views_unknown_frame_id(sm):
    _feed(sm)
    with pytest.raises(ValueError, match="cannot find camera for frame_id camera9"):
        sm.image_callback_views(_msgs(["camera1", "camera9"]))
    assert sm.recorder.calls == [] and len(sm.pcd_queue) == 3          # refused before the queues are touched
    with pytest.raises(ValueError):
        sm.image_callback_views([])


def test_image_callback_views_empty_queues_return_none(sm):
    from vision_semantic_segmentation_amd.utils import Header, Message, Stamp
    assert sm.image_callback_views(_msgs(["camera1", "camera6"])) is None          # no cloud yet
    sm.pcd_callback(Message(Header(Stamp(10, 0), "velodyne"), points=np.zeros((4, 3))))
    assert sm.image_callback_views(_msgs(["camera1", "camera6"])) is None          # a cloud, no pose yet
    assert sm.recorder.calls == [] and sm.input_list == []


def test_image_callback_views_picks_cloud_and_pose_once_by_the_first_stamp(sm):
    _feed(sm)
    sm.record_inputs = True
    msgs = _msgs(["camera6", "camera1"], secs=10)
    msgs[0].header.stamp.nsecs = 400000000            # 10.4 s: between the clouds of 10 s and 12 s, closer to 10 s
    msgs[1].header.stamp.secs = 12                    # a later stamp on the second message is not looked at
    sm.image_callback_views(msgs)
    assert len(sm.recorder.calls) == 1
    pcd, frame_id, semantics, pose, cams, kw = sm.recorder.calls[0]
    assert frame_id == "velodyne" and pose == "pose1" and float(pcd[0, 0]) == 1.0
    assert cams == [sm.cam6, sm.cam1] and kw == {"src_kind": "rgb"}
    assert [int(s[0, 0, 0]) for s in semantics] == [0, 1]
    # one record per view, each with the shared cloud and pose (mapping.py:309-313)
    assert len(sm.input_list) == 2
    for k, rec in enumerate(sm.input_list):
        assert rec["pcd_frame_id"] == "velodyne" and rec["pose"] == "pose1" and float(rec["pcd"][0, 0]) == 1.0
        assert int(rec["semantic_image"][0, 0, 0]) == k
    assert sm.finished == []


def test_mapping_views_saves_once_after_the_last_view(sm):
    sm.pcd, sm.pcd_frame_id = np.zeros((4, 3)), "velodyne"
    sm.save_map_to_file = True
    imgs = [m.data for m in _msgs(["camera1", "camera6", "camera1"])]
    sm.mapping_views(imgs, "pose", [sm.cam1, sm.cam6, sm.cam1])
    assert sm.finished == [1] and sm.save_map_to_file is False       # the shutdown branch ran once, after the views were mapped
    assert sm.input_list == []                                       # MAPPING.INPUT_DIR is empty: nothing recorded
    with pytest.raises(ValueError, match="one camera per semantic image"):
        sm.mapping_views(imgs, "pose", [sm.cam1])
    sm.pcd = None
    sm.mapping_views(imgs, "pose", [sm.cam1, sm.cam6, sm.cam1])       # no cloud: nothing happens (mapping.py:305-306)
    assert len(sm.recorder.calls) == 1
