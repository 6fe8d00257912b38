"""ctypes binding of libavl_hip.so (include/avl_hip.h).

The product path has NO CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AVL_HIP_LIB", os.path.join(_HERE, "libavl_hip.so"))   # override: another build of the library (A/B of two builds, tools/ab_lib.sh)

AVL_F32, AVL_F64, AVL_BF16, AVL_F16 = 0, 1, 2, 3
AVL_SRC_RGB, AVL_SRC_CLASSMAP = 0, 1
AVL_MAX_MAP_CLASSES = 16
AVL_MAX_VIEWS = 4               # views of one avl_fused_frame_views call
AVL_LABEL_ABSTAINED, AVL_LABEL_NONE = 254, 255   # avl_point_labels' states beside the classes
AVL_COUNTER_INTS = 256          # avl_grid.counter block (include/avl_hip.h)
AVL_LIVE_FILTER, AVL_LIVE_THRESHOLDS, AVL_LIVE_FILL = 1, 2, 4   # avl_live_map's flags
(AVL_MERGE_ADD_F64, AVL_MERGE_ADD_F32, AVL_MERGE_ADD_F32_TO_F64, AVL_MERGE_ADD_I64, AVL_MERGE_ADD_I32, AVL_MERGE_MIN_I32,
 AVL_MERGE_MAX_I32) = range(7)   # avl_tile_merge's ops
AVL_LIVE_CAR_DOUBLES = 8        # avl_live_map's car block
AVL_LIVE_VIEW_MAX_SPAN = 2.875  # avl_live_view: the largest |M00| + |M01| and |M10| + |M11|
AVL_COST_LETHAL, AVL_COST_FAR, AVL_COST_MAX_RADIUS = 100, 65535, 32   # avl_cost_map: the lethal cost, "no lethal cell within R", the largest R
AVL_PLANE_W_NONE, AVL_PLANE_W_XNORM = 0, 1
AVL_PLANE_MAX_HYP = 1024
AVL_PLANE_RESULT_WORDS = 24     # 8-byte words of avl_plane_ransac's result block
AVL_STEM_CAMERA_BYTES = 64      # one camera block of a pre-processing stem (avl_stem_camera_set); a raw batch has one per image

_lib = None
_lock = threading.Lock()


class AvlGrid(C.Structure):
    """struct avl_grid of include/avl_hip.h"""
    _fields_ = [
        ("map", C.c_void_p), ("map_dtype", C.c_int),
        ("Hm", C.c_int), ("Wm", C.c_int), ("C", C.c_int),
        ("off_x", C.c_double), ("off_y", C.c_double), ("b00", C.c_double), ("b10", C.c_double),
        ("resolution", C.c_double),
        ("cell_mask", C.c_void_p), ("touched", C.c_void_p), ("touched_cap", C.c_int32), ("counter", C.c_void_p),
        ("counter_len", C.c_int32),
    ]


class AvlOcclusion(C.Structure):
    """struct avl_occlusion of include/avl_hip.h"""
    _fields_ = [
        ("cell_px", C.c_int32), ("radius", C.c_int32), ("rel_tol", C.c_double), ("abs_tol", C.c_double),
        ("depth", C.c_void_p), ("depth_words", C.c_int64), ("culled", C.c_void_p),
    ]


class AvlPointLogits(C.Structure):
    """struct avl_point_logits of include/avl_hip.h"""
    _fields_ = [
        ("logits", C.c_void_p * AVL_MAX_VIEWS), ("h", C.c_int), ("w", C.c_int), ("K", C.c_int), ("ld", C.c_int64),
        ("net_h", C.c_int), ("net_w", C.c_int), ("min_margin", C.c_float), ("abstained", C.c_void_p),
    ]


class AvlGroundFill(C.Structure):
    """struct avl_ground_fill of include/avl_hip.h"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("plane", C.c_double * 4),
        ("range_max", C.c_double), ("class_mask", C.c_uint32), ("filled", C.c_void_p),
    ]


class AvlHeight(C.Structure):
    """struct avl_height of include/avl_hip.h"""
    _fields_ = [
        ("gate", C.c_int32), ("plane", C.c_double * 4), ("min_m", C.c_double * AVL_MAX_MAP_CLASSES),
        ("max_m", C.c_double * AVL_MAX_MAP_CLASSES), ("slope", C.c_double), ("gated", C.c_void_p), ("elev_classes", C.c_uint32),
        ("quantum", C.c_double), ("elev_sum", C.c_void_p), ("elev_cnt", C.c_void_p), ("elev_min", C.c_void_p), ("elev_max", C.c_void_p),
    ]


class AvlTileJob(C.Structure):
    """struct avl_tile_job of include/avl_hip.h"""
    _fields_ = [
        ("src", C.c_void_p), ("src_pitch", C.c_int64), ("dst", C.c_void_p), ("dst_pitch", C.c_int64), ("flag", C.c_int32), ("fresh", C.c_int32),
    ]


class AvlTileSrc(C.Structure):
    """struct avl_tile_src of include/avl_hip.h"""
    _fields_ = [("src", C.c_void_p), ("src_pitch", C.c_int64), ("row", C.c_int32), ("col", C.c_int32)]


_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double

_SIGNATURES = {
    "avl_version": (C.c_char_p, []),
    "avl_last_error": (_i, [C.c_char_p, _i]),
    "avl_project_points": (_i, [_vp, _i, _i, _i64, _i64, _vp, _vp, _d, _i, _i, _vp, _vp, _vp]),
    "avl_project_pcd_scratch_bytes": (_i64, [_i]),
    "avl_project_pcd": (_i, [_vp, _i, _i, _i64, _i64, _vp, _vp, _d, _vp, _i, _i, _vp, _vp, _i64, _vp, _vp, _vp]),
    "avl_update_map": (_i, [C.POINTER(AvlGrid), _vp, _vp, _i64, _i, _vp, _vp, _vp, C.c_uint32, _vp]),
    "avl_vote_points": (_i, [C.POINTER(AvlGrid), _vp, _vp, _i64, _i, _vp, _vp, C.c_uint32, _vp]),
    "avl_grid_apply": (_i, [C.POINTER(AvlGrid), _vp, _vp, _i, _vp]),
    "avl_fused_frame": (_i, [C.POINTER(AvlGrid), _vp, _i, _i, _i64, _i64, _vp, _vp, _d, _i, _vp, _i, _i, _i, _i,
                             _vp, _vp, _vp, C.c_uint32, _vp]),
    "avl_fused_frame_path": (_i, [C.POINTER(AvlGrid), _i, C.c_uint32]),
    "avl_fused_frame_views": (_i, [C.POINTER(AvlGrid), _vp, _i, _i, _i64, _i64, _i, _vp, _vp, _d, _i, _vp, _i, _i, _i, _i,
                                   _vp, _vp, _vp, C.c_uint32, _vp]),
    "avl_fused_frame_views_path": (_i, [C.POINTER(AvlGrid), _i, _i, C.c_uint32]),
    "avl_occlusion_depth_words": (_i64, [_i, _i, _i, _i]),
    "avl_fused_frame_occl": (_i, [C.POINTER(AvlGrid), _vp, _i, _i, _i64, _i64, _vp, _vp, _d, _i, _vp, _i, _i, _i, _i,
                                  _vp, _vp, _vp, C.c_uint32, C.POINTER(AvlOcclusion), _vp]),
    "avl_fused_frame_views_occl": (_i, [C.POINTER(AvlGrid), _vp, _i, _i, _i64, _i64, _i, _vp, _vp, _d, _i, _vp, _i, _i, _i, _i,
                                        _vp, _vp, _vp, C.c_uint32, C.POINTER(AvlOcclusion), _vp]),
    "avl_occlusion_visibility": (_i, [_vp, _i, _i, _i64, _i64, _i, _vp, _vp, _d, _i, _i, C.POINTER(AvlOcclusion), _vp, _vp, _vp]),
    "avl_fused_frame_logits": (_i, [C.POINTER(AvlGrid), _vp, _i, _i, _i64, _i64, _vp, _vp, _d, C.POINTER(AvlPointLogits), _i, _i,
                                    _vp, _vp, C.c_uint32, C.POINTER(AvlOcclusion), _vp]),
    "avl_fused_frame_views_logits": (_i, [C.POINTER(AvlGrid), _vp, _i, _i, _i64, _i64, _i, _vp, _vp, _d, C.POINTER(AvlPointLogits), _i, _i,
                                          _vp, _vp, C.c_uint32, C.POINTER(AvlOcclusion), _vp]),
    "avl_point_labels": (_i, [_vp, _i, _i, _i64, _i64, _i, _vp, _vp, _d, _i, _i, C.POINTER(AvlPointLogits), _vp, _vp, _vp]),
    "avl_ground_fill_views": (_i, [C.POINTER(AvlGrid), C.POINTER(AvlGroundFill), _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp,
                                   C.POINTER(AvlOcclusion), _vp]),
    "avl_ground_fill_views_logits": (_i, [C.POINTER(AvlGrid), C.POINTER(AvlGroundFill), _i, _vp, _vp, C.POINTER(AvlPointLogits), _i, _i,
                                          _vp, _vp, C.POINTER(AvlOcclusion), _vp]),
    "avl_occlusion_depth": (_i, [_vp, _i, _i, _i64, _i64, _i, _vp, _vp, _d, _i, _i, C.POINTER(AvlOcclusion), _vp]),
    "avl_fused_frame_views_height": (_i, [C.POINTER(AvlGrid), _vp, _i, _i, _i64, _i64, _i, _vp, _vp, _d, _i, _vp, _i, _i, _i, _i,
                                          _vp, _vp, _vp, C.c_uint32, C.POINTER(AvlPointLogits), C.POINTER(AvlOcclusion),
                                          C.POINTER(AvlHeight), _vp]),
    "avl_point_heights": (_i, [_vp, _i, _i, _i64, _i64, _vp, C.POINTER(AvlHeight), _vp, _vp, _vp]),
    "avl_elevation_mean": (_i, [_vp, _vp, _i64, _d, _vp, _vp]),
    "avl_elevation_reset": (_i, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "avl_colorize_labels": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "avl_preprocess_image": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "avl_preprocess_image_area": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "avl_stem_camera_set": (_i, [_vp, _vp, _vp, _vp]),
    "avl_pack_semantic_cloud": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "avl_unpack_pointcloud2": (_i, [_vp, _i64, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "avl_planar_update": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp, _i, _vp]),
    "avl_render_bev_map": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "avl_render_bev_map_thresholds": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "avl_grid_box_filter": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "avl_live_map": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "avl_live_view": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "avl_fill_black": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "avl_eval_map": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "avl_upsample_logits": (_i, [_vp, _i, _i, _i, _i64, _vp, _i, _i, _vp]),
    "avl_seg_eval_scratch_bytes": (_i64, [_i, _i]),
    "avl_seg_eval_full_res": (_i, [_vp, _i, _i, _i, _i64, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "avl_upsample_logits_batch": (_i, [_vp, _i, _i64, _i, _i, _i, _i64, _vp, _i, _i, _vp]),
    "avl_seg_eval_scratch_bytes_batch": (_i64, [_i, _i, _i]),
    "avl_seg_eval_full_res_batch": (_i, [_vp, _i, _i64, _i, _i, _i, _i64, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "avl_hull_scratch_bytes": (_i64, [_i, _i, _i, _i]),
    "avl_label_components": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "avl_class_hulls": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "avl_plane_scratch_bytes": (_i64, [_i, _i]),
    "avl_plane_ransac": (_i, [_vp, _i, _i, _i64, _i64, _vp, _vp, _vp, _i, _i, _d, _i, _d, _d, _vp, _vp, _vp, _vp, _vp]),
    "avl_points_map_keys": (_i, [_vp, _i64, _d, _d, _d, _i, _i, _vp, _vp]),
    "avl_points_map_window": (_i, [_vp, _i, _i, _i, _i, _i, _i, C.POINTER(_i64), C.POINTER(C.c_int32)]),
    "avl_points_map_gather": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    "avl_tile_copy": (_i, [_vp, _i, _i, _i, C.c_uint32, _vp, _i, _vp]),
    "avl_tile_merge": (_i, [_vp, _i, _i, _i, _i, C.c_uint32, _vp, _i, _vp]),
    "avl_site_overview": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "avl_site_finish": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i64, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp]),
    "avl_cost_map_scratch_bytes": (_i64, [_i, _i, _i]),
    "avl_cost_map": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
}


def exported_symbols():
    """Every symbol include/avl_hip.h declares (kept in step with the header by a test)."""
    return sorted(_SIGNATURES) + sorted(_SEG_SIGNATURES)


_SEG_SIGNATURES = {}


def _register_seg(sigs):
    _SEG_SIGNATURES.update(sigs)


def lib():
    """Load (once) and return the library; raise RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libavl_hip.so not found at %s -- build it with `make -C vision_semantic_segmentation_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback." % LIB_PATH)
        # torch ships its own HIP/HSA runtime (same SONAME as /opt/rocm's).  It must be in the process
        # first so that libavl_hip.so binds to that copy: two HSA runtimes in one process cannot
        # both own the GPU ("no ROCm-capable device is detected").
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in list(_SIGNATURES.items()) + list(_SEG_SIGNATURES.items()):
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def last_error():
    buf = C.create_string_buffer(512)
    lib().avl_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what or "libavl_hip call", rc, last_error()))


def host_array(values, ctype):
    """A ctypes array holding `values` (flattened); keep the return value alive across the call."""
    flat = [v for v in values]
    return (ctype * len(flat))(*flat)


def points_view(pcd, device):
    """A point cloud [4, N] (the reference's layout) or [N, 4], ndarray or tensor, as avl_project_points addresses it ->
    (tensor on `device` that must outlive the call, n, avl dtype, point_stride, comp_stride).  float32 and float64 are kept,
    anything else becomes float64."""
    import numpy as np
    import torch
    if not isinstance(pcd, torch.Tensor):
        a = np.asarray(pcd)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        pcd = torch.from_numpy(np.ascontiguousarray(a))
    if pcd.dtype not in (torch.float32, torch.float64):
        pcd = pcd.to(torch.float64)
    t = pcd.to(device).contiguous()
    es = t.element_size()
    dtype = AVL_F64 if t.dtype == torch.float64 else AVL_F32
    if t.dim() == 2 and t.shape[0] == 4:            # SoA [4,N]: the reference layout
        n = int(t.shape[1])
        return t, n, dtype, es, es * max(n, 1)
    if t.dim() == 2 and t.shape[1] == 4:            # AoS [N,4]
        return t, int(t.shape[0]), dtype, 4 * es, es
    raise ValueError("point cloud must be [4,N] or [N,4], got %s" % (tuple(t.shape),))
