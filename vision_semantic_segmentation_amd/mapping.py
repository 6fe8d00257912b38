"""SemanticMapping -- the reference's mapping node (src/mapping.py:39-541) with its per-frame
arithmetic on the MI355X.

Same class name, method names, argument layouts and attributes as the reference, so a ROS shell or
the replay driver can call it unchanged:

    sm = SemanticMapping(cfg)
    sm.pcd_callback(msg); sm.pose_callback(msg); sm.image_callback(msg)      # mapping.py:172,221,261
    pcd_in_range, label = sm.project_pcd(pcd, frame_id, image, pose, cam)    # mapping.py:357
    grid = sm.update_map(grid, pcd_in_range, label)                           # mapping.py:391
    sm.mapping(semantic_image, pose, cam)                                     # mapping.py:292

What differs from the reference, by design:
  * project_pcd / update_map / mapping run as HIP kernels through libavl_hip.so (csrc/mapping.hip);
    there is no NumPy fallback -- a missing library or GPU raises.
  * the grid lives in HBM (``self.map_dev``, float64 like the reference unless MAPPING.GRID_DTYPE is
    "f32"); ``self.map`` downloads it on access.
  * ``mapping()`` is fused: points are projected, labelled, voted and applied without the
    intermediate masked point list; ``frame_device()`` does the same for inputs already in HBM
    (e.g. the argmax label map straight from SemanticSegmentation).
  * ``live_map()`` renders the window of the grid around the vehicle (filter, renderer, hole fill, ego car) in one kernel; with
    MAPPING.LIVE_MAP.ENABLED ``mapping()`` / ``mapping_views()`` do so after the grid update.  The reference renders once, at
    shutdown.  ``live_view()`` is the same picture heading-up: rotated about the vehicle, scaled, the vehicle at a chosen pixel
    (MAPPING.LIVE_VIEW), still one kernel.
  * ``cost_map()`` is the same window as a planner reads it: an int8 cost per cell from the cell's class (100 lethal, -1 no
    information), 0 under the ego footprint, and an inflated margin around the lethal cells, in nav_msgs/OccupancyGrid's order
    (MAPPING.COST_MAP; the rule at avl_cost_map in include/avl_hip.h); ``cost_map_info()`` has the grid's other fields.  Off by default.
  * with MAPPING.OCCLUSION.ENABLED, points hidden behind nearer ones in a view's image do not vote (a per-view depth buffer, the
    rule at struct avl_occlusion in include/avl_hip.h); ``visibility_device()`` returns the verdict per point.  The reference lets
    every point that lands in the image vote.  Off by default.
  * ``frame_device(..., src_kind="logits")`` labels the points from a plan's fp32 logits, interpolated at each point's pixel as the
    reference model's full-resolution prediction is, and lets a point whose top-1 minus top-2 margin is below
    MAPPING.CONFIDENCE.MIN_MARGIN abstain (the rule at struct avl_point_logits in include/avl_hip.h); ``point_labels_device()``
    returns label and margin per point.  The reference votes the nearest low-resolution arg-max with full weight.
  * with MAPPING.GROUND_FILL.ENABLED and a ground plane (``set_ground_plane()`` / ``plane_callback()``), every cell of a window around
    the vehicle puts its centre on the plane, projects it into the cameras and takes the pixel's label as one update, after the
    LiDAR frame (``ground_fill_device()``; the rule at struct avl_ground_fill in include/avl_hip.h): the map becomes dense where the
    cameras see ground, not only where a LiDAR ring fell.  The reference has nothing of the kind that works.  Off by default.
  * with MAPPING.POINTS_MAP.SOURCE = "index" the points-map mode needs no node that crops the site's point map and publishes
    /reduced_map (mapping.py:61-62): ``load_points_map()`` puts the whole map on the device, sorted into ground tiles, and every frame
    takes its cloud from ``reduced_map_device()``, one kernel that copies the tiles that can hold a voting point (points_map.py).  The
    grid ends bit-equal to a frame on the whole map.  Off ("topic") by default.
  * with MAPPING.HEIGHT_GATE.ENABLED and a ground plane, a point votes class i only while its height above the plane lies in that
    class's band (the rule at struct avl_height in include/avl_hip.h; ``last_gated``, ``point_heights_device()``): the reference
    projects the cloud onto z = 0, so a canopy point votes into the road cell beneath it.  With MAPPING.ELEVATION.ENABLED the z of
    the points that vote a ground class is accumulated per cell (``elevation_device()``, ``elevation_layer()``).  Both off by default.
  * with MAPPING.SCROLL.ENABLED the grid is a window that follows the vehicle: its origin moves in whole tiles (``scroll_to()``, called
    by ``mapping()`` / ``mapping_views()``), tiles that leave are kept in a store in HBM and come back when the vehicle returns
    (scroll.py; ``site_map()``, ``site_tiles()``, ``save_site()``, ``load_site()``).  The reference drops every point outside
    MAPPING.BOUNDARY.  Off by default.  ``site_overview()`` is the picture of the whole site at k cells per pixel, rendered from the
    tiles where they live; with MAPPING.SITE_OVERVIEW.ENABLED ``finish_run()`` also writes it as site_map.png.  ``site_finish()`` is the
    run's result for the whole site -- the filtered picture at one pixel per cell, its labels and the counts behind the IoU lines -- by
    one kernel from the tiles; with MAPPING.SITE_FINISH.ENABLED ``finish_run()`` also writes it as site_global_map.png.
  * rospy subscribers/publishers are only created when ``use_ros=True`` and rospy imports; a lock
    serialises the three callbacks (the reference mutates its queues from three threads unlocked).
"""
import ctypes as C
import os
import os.path as osp
import threading

import numpy as np
import torch

from . import _lib
from .camera import camera_setup_1, camera_setup_6
from .config import get_cfg_defaults
from .data.confusion_matrix import ConfusionMatrix
from .labels import PALETTE_19, vote_lut
from .utils.utils_ros import euler_matrix, get_transform_from_pose, quaternion_matrix
from .utils.logger import MyLogger

# src/mapping.py:404 (= minus the global_map pose of :232-233)
PCD_ORIGIN_OFFSET = (1369.0496826171875, 562.84814453125, 0.0)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _raw_stream(s):
    """A torch.cuda.Stream or a raw stream handle -> the raw handle; None stays None (torch's current stream)."""
    return None if s is None else int(getattr(s, "cuda_stream", s))


_DBL_CACHE = {}


def _dbl(a):
    """float64 ctypes array of a small host matrix (P, T, CM); memoised on the bytes -- the same few matrices are
    passed every frame and building a ctypes array element by element costs more than the kernel launch."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    key = a.tobytes()
    hit = _DBL_CACHE.get(key)
    if hit is None:
        if len(_DBL_CACHE) > 256:
            _DBL_CACHE.clear()
        hit = (C.c_double * a.size).from_buffer_copy(key)
        _DBL_CACHE[key] = hit
    return hit


def confidence_min_margin(cfg):
    """MAPPING.CONFIDENCE.MIN_MARGIN as a float (0.0 for a configuration without the node).  ValueError unless it is a number >= 0:
    a bool, a string, a negative value and a NaN are refused."""
    node = getattr(cfg.MAPPING, "CONFIDENCE", None)
    v = 0.0 if node is None else node.MIN_MARGIN
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not float(v) >= 0.0:
        raise ValueError("MAPPING.CONFIDENCE.MIN_MARGIN = %r (a float >= 0)" % (v,))
    return float(v)


def logits_views(semantics, n_views=None):
    """The views of a logits source (src_kind="logits") -> (list of fp32 CUDA tensors [h', w', K], (h', w', K), ld).  ``semantics``:
    one tensor [h', w', K] (n_views None), a tensor [V, h', w', K] or a list of V tensors [h', w', K] -- SegNet.logits of a plan or
    a batched plan goes in as it is.  Every view's pixels lie ``ld`` >= K floats apart with the classes next to each other (a
    contiguous tensor, or the first K columns of one), one ld for all views; K is 1..254.  ValueError otherwise."""
    if n_views is None:
        if not isinstance(semantics, torch.Tensor) or semantics.dim() != 3:
            raise ValueError("a logits source is a tensor [h', w', K], got %s" % (
                tuple(semantics.shape) if isinstance(semantics, torch.Tensor) else type(semantics).__name__,))
        views = [semantics]
    elif isinstance(semantics, torch.Tensor):
        if semantics.dim() != 4 or int(semantics.shape[0]) != n_views:
            raise ValueError("semantics has shape %s for %d logits views" % (tuple(semantics.shape), n_views))
        views = [semantics[v] for v in range(n_views)]
    else:
        views = list(semantics)
        if len(views) != n_views:
            raise ValueError("%d semantic sources for %d cameras" % (len(views), n_views))
    shape, ld = None, None
    for t in views:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("logits must be float32 tensors, got %s" % (t.dtype if isinstance(t, torch.Tensor) else type(t).__name__,))
        if t.dim() != 3 or min(t.shape) < 1:
            raise ValueError("a logits view is [h', w', K], got %s" % (tuple(t.shape),))
        h, w, K = (int(d) for d in t.shape)
        if K > 254:
            raise ValueError("logits of K = %d classes (1..254)" % K)
        t_ld = int(t.stride(1)) if w > 1 else (int(t.stride(0)) if h > 1 else K)
        if (K > 1 and t.stride(2) != 1) or t_ld < K or (h > 1 and int(t.stride(0)) != w * t_ld):
            raise ValueError("logits view of shape %s has strides %s: its pixels must lie ld >= K floats apart, row after row" % (
                tuple(t.shape), tuple(t.stride())))
        if shape is None:
            shape, ld = (h, w, K), t_ld
        elif (h, w, K) != shape or t_ld != ld:
            raise ValueError("the views' logits must have one shape and one row stride")
    for t in views:
        if not t.is_cuda:
            raise ValueError("logits must be CUDA tensors")
    return views, shape, ld


class DeviceGrid(object):
    """The BEV grid and its per-frame scratch in HBM (struct avl_grid of include/avl_hip.h)."""

    def __init__(self, Hm, Wm, C_, boundary, resolution, dtype, device):
        self.Hm, self.Wm, self.C = int(Hm), int(Wm), int(C_)
        self.boundary = boundary
        self.resolution = float(resolution)
        self.device = device
        self.torch_dtype = torch.float64 if dtype == "f64" else torch.float32
        self.map = torch.zeros((self.Hm, self.Wm, self.C), dtype=self.torch_dtype, device=device)
        self.cell_mask = torch.zeros(self.Hm * self.Wm, dtype=torch.int32, device=device)
        self.counter = torch.zeros(_lib.AVL_COUNTER_INTS, dtype=torch.int32, device=device)
        self.touched = None
        self.touched_cap = 0
        self.ensure_capacity(1 << 17)

    def ensure_capacity(self, n):
        need = min(int(n), self.Hm * self.Wm) + 64 * 256      # + the rounding slack of the partitioned lists (mapping.hip, kLists)
        if need > self.touched_cap:
            self.touched_cap = max(need, 2 * self.touched_cap)
            self.touched = torch.empty(self.touched_cap, dtype=torch.int32, device=self.device)

    def struct(self, map_tensor=None):
        m = self.map if map_tensor is None else map_tensor
        g = _lib.AvlGrid()
        g.map = m.data_ptr()
        g.map_dtype = _lib.AVL_F64 if m.dtype == torch.float64 else _lib.AVL_F32
        g.Hm, g.Wm, g.C = self.Hm, self.Wm, self.C
        g.off_x, g.off_y = PCD_ORIGIN_OFFSET[0], PCD_ORIGIN_OFFSET[1]
        g.b00, g.b10 = float(self.boundary[0][0]), float(self.boundary[1][0])
        g.resolution = self.resolution
        g.cell_mask = self.cell_mask.data_ptr()
        g.touched = self.touched.data_ptr()
        g.touched_cap = self.touched_cap
        g.counter = self.counter.data_ptr()
        g.counter_len = int(self.counter.numel())
        return g


class SemanticMapping(object):
    """Create a semantic bird's eye view map from LiDAR points and 2-D semantic segmentation images
    (reference class: src/mapping.py:39)."""

    def __init__(self, cfg=None, device=None, use_ros=False, logger=None):
        cfg = get_cfg_defaults() if cfg is None else cfg
        assert len(cfg.LABELS) == len(cfg.LABELS_NAMES) == len(cfg.LABEL_COLORS)     # mapping.py:53
        _lib.lib()  # fail loudly, now, if the HIP library is missing
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("SemanticMapping needs a GPU (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.cfg = cfg
        self._lock = threading.RLock()

        self.depth_method = cfg.MAPPING.DEPTH_METHOD
        # the points-map mode's own index (MAPPING.POINTS_MAP); SOURCE "topic", the default: nothing of it runs and nothing is allocated
        self.points_map_cfg = getattr(cfg.MAPPING, "POINTS_MAP", None)
        self.points_map_source = "topic" if self.points_map_cfg is None else self.points_map_cfg.SOURCE
        if self.points_map_source not in ("topic", "index"):
            raise ValueError("MAPPING.POINTS_MAP.SOURCE must be 'topic' or 'index', not %r" % (self.points_map_source,))
        if self.points_map_source == "index" and self.depth_method != "points_map":
            raise ValueError("MAPPING.POINTS_MAP.SOURCE = 'index' needs MAPPING.DEPTH_METHOD = 'points_map', not %r" % (self.depth_method,))
        self.points_map_index = None           # points_map.PointsMapIndex (load_points_map)
        self.last_reduced = None               # {"points": M, "tiles": ..., "rows": ..., "reused": bool} of the last reduced_map_device
        self._reduced_buf = None               # float32 CUDA [capacity, 4]: grows geometrically
        self._reduced_rect = None              # the rectangle _reduced_buf holds
        self._reduced_stream = None            # the stream the gather that filled it ran on
        if self.points_map_indexed() and self.points_map_cfg.PATH != "":
            self.load_points_map(self.points_map_cfg.PATH)     # before the subscribers exist: no frame can arrive ahead of the index
        self._ros = None
        if use_ros:
            self._setup_ros()

        output_dir = cfg.OUTPUT_DIR
        if "@" in output_dir:
            output_dir = output_dir.replace("@", osp.join(osp.dirname(__file__), "../"))
            output_dir = osp.abspath(osp.join(output_dir, cfg.TASK_NAME))
        self.logger = logger if logger is not None else MyLogger("mapping", save_dir=None)
        self.output_dir = output_dir

        self.pose = None
        self.pose_queue = []
        self.pose_time = None
        self.cam1 = camera_setup_1()
        self.cam6 = camera_setup_6()

        self.pcd = None
        self.pcd_frame_id = None
        self.pcd_queue = []
        self.pcd_header_queue = []
        self.pcd_time = None
        self.pcd_range_max = cfg.MAPPING.PCD.RANGE_MAX
        self.use_pcd_intensity = cfg.MAPPING.PCD.USE_INTENSITY
        # build-specific: unpack PointCloud2 payloads on the GPU (self.pcd is then a CUDA float32 [N,4] tensor, not ndarray [4,N])
        self.unpack_on_device = bool(getattr(cfg.MAPPING.PCD, "UNPACK_ON_DEVICE", False))
        self._pc2_stage = None

        # map[x, y] (mapping.py:106-117)
        self._grid = None
        self._map_host = None
        self.map_pose = None
        self.save_map_to_file = False
        self.map_boundary = cfg.MAPPING.BOUNDARY
        self.resolution = cfg.MAPPING.RESOLUTION
        self.label_names = cfg.LABELS_NAMES
        self.label_colors = np.array(cfg.LABEL_COLORS)
        self.map_height = int((self.map_boundary[0][1] - self.map_boundary[0][0]) / self.resolution)
        self.map_width = int((self.map_boundary[1][1] - self.map_boundary[1][0]) / self.resolution)
        self.map_depth = len(self.label_names)
        if self.map_depth > _lib.AVL_MAX_MAP_CLASSES:
            raise ValueError("at most %d map classes are supported" % _lib.AVL_MAX_MAP_CLASSES)
        self.grid_dtype = getattr(cfg.MAPPING, "GRID_DTYPE", "f64")
        self.planar_match = getattr(cfg.MAPPING, "PLANAR_MATCH", "reference")
        self.local_to_base_lookup = None       # planar mode: callable(pose_time) -> 4x4 /local_map -> /base_link (the reference's TF lookup)

        self.position_rel = np.array([[0, 0, 0]]).T
        self.yaw_rel = 0
        self.preprocessing()

        self.test_cut_time = cfg.TEST_END_TIME
        if cfg.MAPPING.CONFUSION_MTX.LOAD_PATH != "":                                  # mapping.py:127-132
            confusion_matrix = ConfusionMatrix(load_path=cfg.MAPPING.CONFUSION_MTX.LOAD_PATH)
            self.confusion_matrix = confusion_matrix.get_submatrix(cfg.LABELS, to_probability=True, use_log=True)
        else:
            self.confusion_matrix = np.eye(len(self.label_names))

        self.ground_truth_dir = cfg.GROUND_TRUTH_DIR
        self.input_list = []
        self.input_dir = cfg.MAPPING.INPUT_DIR
        self.record_inputs = cfg.MAPPING.INPUT_DIR != ""
        self.frames_mapped = 0

        # live vehicle-centred map (MAPPING.LIVE_MAP); off by default
        self.live_cfg = cfg.MAPPING.LIVE_MAP
        self.live_view_cfg = cfg.MAPPING.LIVE_VIEW   # the heading-up view's geometry
        self.live_view_matrix_last = None      # 2 x 3 float64: the matrix of the last live_view()
        self.live_map_image = None             # uint8 [h, w, 3] on the device, the last live map
        self.live_map_host = None              # the same in pinned host memory, valid once the stream is synchronised
        self.live_map_origin = None            # grid cell of live_map_image[0, 0]
        self.live_map_ready = None             # event recorded behind the copy into live_map_host
        self.pub_semantic_local_map = getattr(self, "pub_semantic_local_map", None)
        self._live_pose = None

        # live cost map (MAPPING.COST_MAP); off by default: then nothing below is touched
        self.cost_cfg = cfg.MAPPING.COST_MAP
        self.cost_map_image = None             # int8 [w, h] (ORDER "yx") or [h, w] ("xy") on the device, the last cost map
        self.cost_map_host = None              # the same in pinned host memory, valid once the stream is synchronised
        self.cost_map_origin = None            # grid cell of the cost map's element (i, j) = (0, 0)
        self.cost_map_size = None              # (h, w) cells of the last cost map
        self.cost_map_ready = None             # event recorded behind the copy into cost_map_host
        self.pub_semantic_cost_map = getattr(self, "pub_semantic_cost_map", None)
        self._cost_par = self._parse_cost_map() if self.cost_cfg.ENABLED else None      # ValueError for a CLASS_COST or a radius that does not fit

        # occlusion culling (MAPPING.OCCLUSION); off by default: then nothing below is touched
        self.occlusion_cfg = getattr(cfg.MAPPING, "OCCLUSION", None)
        self.last_culled = None                # int32 CUDA tensor [V]: culled candidates per view of the last culling call (no sync to fill it)
        self._occl_depth = {}                  # (V, Hc, Wc) -> the depth scratch of that shape

        # labels from interpolated logits (src_kind="logits") and their confidence gate (MAPPING.CONFIDENCE)
        self.min_margin = confidence_min_margin(cfg)   # a point whose top-1 minus top-2 margin is below it abstains; 0 gates nothing
        self.last_abstained = None             # int32 CUDA tensor [V]: votes the gate withheld per view in the last logits call (no sync)

        # dense ground fill (MAPPING.GROUND_FILL); off by default: then nothing below is touched
        self.ground_fill_cfg = getattr(cfg.MAPPING, "GROUND_FILL", None)
        self.ground_plane = None               # float64 [4]: (a, b, c, d) in the velodyne frame (set_ground_plane, plane_callback)
        self.last_filled = None                # int32 CUDA tensor [V]: cells that took a vote per view in the last ground fill (no sync)

        # height-aware mapping (MAPPING.HEIGHT_GATE, MAPPING.ELEVATION); both off by default: then nothing below is touched
        self.height_gate_cfg = getattr(cfg.MAPPING, "HEIGHT_GATE", None)
        self.elevation_cfg = getattr(cfg.MAPPING, "ELEVATION", None)
        self.last_gated = None                 # int32 CUDA tensor [V]: votes the height gate withheld per view in the last gated call (no sync)
        self._height_bounds = self._parse_height_gate() if self.height_gate_enabled() else None    # (min_m [C], max_m [C], slope)
        self._elevation_par = self._parse_elevation() if self.elevation_enabled() else None        # (class mask, quantum)
        self._elevation = None                 # (sum int64, cnt, min, max int32) CUDA [Hm, Wm]: allocated on first use

        # the scrolling grid (MAPPING.SCROLL); off by default: then there is no store, no second buffer and nothing of scroll.py
        self.scroll_cfg = getattr(cfg.MAPPING, "SCROLL", None)
        self.scroll_origin = (0, 0)            # the window's origin in global cells, multiples of the tile size
        self.last_scroll = None                # {"shift": (di, dj) in tiles, "leaving", "entering", "loaded", "filled"} of the last scroll
        self.scroll_count = 0
        self._scroll = None                    # scroll.TileStore
        self.last_site_overview = None         # {"rect": (ti0, ti1, tj0, tj1), "cells_per_pixel": k, "tiles": entries launched} of the last site_overview
        if self.scroll_enabled():
            from .scroll import TileStore
            self._scroll = TileStore(self)     # ValueError for a tile size that does not fit the grid, and for the planar mode

        # device-side caches
        self._scratch = None
        self._pcd_dev = None
        self._out_pcd = None
        self._out_label = None
        self._out_count = torch.zeros(4, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------ ROS plumbing (optional)
    def _setup_ros(self):
        import rospy  # noqa: F401  (only when asked for)
        from geometry_msgs.msg import PoseStamped
        from sensor_msgs.msg import Image, PointCloud2
        self._ros = rospy
        self.sub_pose = rospy.Subscriber("/current_pose", PoseStamped, self.pose_callback)
        self.image_sub_cam1 = rospy.Subscriber("/camera1/semantic", Image, self.image_callback)
        self.image_sub_cam6 = rospy.Subscriber("/camera6/semantic", Image, self.image_callback)
        self.pub_semantic_local_map = rospy.Publisher("/semantic_local_map", Image, queue_size=5)     # mapping.py:69
        self._ros_image_cls = Image
        if self.cfg.MAPPING.COST_MAP.ENABLED:
            from nav_msgs.msg import OccupancyGrid
            self.pub_semantic_cost_map = rospy.Publisher("/semantic_cost_map", OccupancyGrid, queue_size=5)
            self._ros_grid_cls = OccupancyGrid
        if self.depth_method == "points_map":
            if not self.points_map_indexed():                  # with the index nothing outside the package has to publish the crop
                self.sub_pcd = rospy.Subscriber("/reduced_map", PointCloud2, self.pcd_callback)
        elif self.depth_method == "points_raw":
            self.sub_pcd = rospy.Subscriber("/points_raw", PointCloud2, self.pcd_callback)
        if self.cfg.MAPPING.GROUND_FILL.ENABLED:
            from shape_msgs.msg import Plane
            self.sub_plane = rospy.Subscriber("/estimated_plane", Plane, self.plane_callback)

    # ------------------------------------------------------------------ constants (mapping.py:142-170)
    def preprocessing(self):
        """Setup constant matrices (mapping.py:142-163; only the ones the LiDAR path uses)."""
        self.T_velodyne_to_basklink = self.set_velodyne_to_baselink()
        self.T_cam1_to_base = np.matmul(self.T_velodyne_to_basklink, self.cam1.T)
        self.T_cam6_to_base = np.matmul(self.T_velodyne_to_basklink, self.cam6.T)
        self.discretize_matrix_inv = np.array([
            [self.resolution, 0, self.map_boundary[0][0]],
            [0, self.resolution, self.map_boundary[1][1]],
            [0, 0, 1],
        ]).astype(np.float64)
        self.discretize_matrix = np.linalg.inv(self.discretize_matrix_inv)
        self.anchor_points_2 = np.array([                                          # mapping.py:160-163
            [self.map_width, self.map_width / 2, self.map_width / 2, self.map_width],
            [self.map_height / 4, self.map_height / 4, self.map_height * 3 / 4, self.map_height * 3 / 4],
        ], dtype=np.float64)

    def set_velodyne_to_baselink(self):
        """mapping.py:165-170"""
        return velodyne_to_baselink()

    # ------------------------------------------------------------------ the grid
    @property
    def grid(self):
        if self._grid is None:
            self._grid = DeviceGrid(self.map_height, self.map_width, self.map_depth, self.map_boundary,
                                    self.resolution, self.grid_dtype, self.device)
        return self._grid

    @property
    def map_dev(self):
        """The grid in HBM: torch tensor [map_height, map_width, map_depth].  With MAPPING.SCROLL.ENABLED this is the window's CURRENT
        buffer: a scroll swaps the two buffers, and a caller who kept the tensor from before the scroll holds stale memory."""
        return self.grid.map

    @property
    def map(self):
        """The grid as a NumPy array (downloaded on access), or None before the first frame
        (mapping.py:107,303-304)."""
        if self._grid is None:
            return None
        if self._map_host is None:
            self._map_host = self._grid.map.cpu().numpy()
        return self._map_host

    @map.setter
    def map(self, value):
        self._map_host = None
        if value is None:
            self._grid = None
            return
        t = torch.as_tensor(np.ascontiguousarray(value))
        g = self.grid
        g.map.copy_(t.to(self.device, dtype=g.torch_dtype))

    # ------------------------------------------------------------------ callbacks
    def pcd_callback(self, msg):
        """mapping.py:172-183.  Accepts (a) any message with ``.points`` = array [4,N] or [N,4]
        (x,y,z,intensity), or (b) a sensor_msgs/PointCloud2, unpacked with one vectorised
        ``np.frombuffer`` instead of the reference's per-point Python loop."""
        if hasattr(msg, "points"):
            pts = np.asarray(msg.points)
            pcd = pts if pts.shape[0] == 4 else pts.T
            pcd = np.ascontiguousarray(pcd, dtype=np.float64)
        elif self.unpack_on_device:
            pcd = self.unpack_pointcloud2_device(msg)[0]       # float32 [N,4] in HBM; NaN points keep their slot, x = NaN
        else:
            pcd = unpack_pointcloud2(msg)
        with self._lock:
            self.pcd_queue.append(pcd)
            self.pcd_header_queue.append(msg.header)
            self.pcd_frame_id = msg.header.frame_id

    def unpack_pointcloud2_device(self, msg, stream=None):
        """pcd_callback's unpacking (mapping.py:172-183) on the GPU: the message payload is uploaded once (through a reused
        pinned staging buffer, asynchronously on `stream`) and avl_unpack_pointcloud2 writes float32 [N,4] (x,y,z,intensity)
        straight into the layout the fused frame reads.  Returns (points CUDA float32 [N,4], n_valid CUDA int32 [1]) --
        n_valid is what read_points(skip_nans=True) would have yielded; points that it would have skipped keep their slot
        with x = NaN and are rejected by the projection kernel.
        With an explicit `stream` the upload and the kernel overlap whatever the current stream is doing (they wait for it only when the
        staging buffer has just been (re)allocated).  The returned tensors then belong to THAT stream: a caller that consumes them on
        another stream must make it wait for `stream` first and call ``tensor.record_stream(consumer_stream)`` before dropping them."""
        offs = {f.name: f.offset for f in msg.fields}
        n = int(msg.width) * int(msg.height)
        step = int(msg.point_step)
        nbytes = n * step
        # Everything this call enqueues -- the zero-fill of `count`, the upload, the kernel -- goes on ONE stream `st` (the caller's,
        # or torch's current one), and the tensors it returns are allocated under that stream so that the caching allocator
        # knows who uses them (with an explicit stream the zero-fill used to run on torch's current stream and could
        # race with the kernel's atomic increments).
        st = torch.cuda.current_stream(self.device) if stream is None else torch.cuda.ExternalStream(int(stream), device=self.device)
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            points = torch.empty((max(n, 1), 4), dtype=torch.float32, device=self.device)[:n]
            count = torch.zeros(1, dtype=torch.int32, device=self.device)
        if n == 0:
            return points, count
        payload = _pointcloud2_payload(msg)                   # uint8 [n * point_step]: rows without their row_step padding
        if self._pc2_stage is None or self._pc2_stage[0].numel() < nbytes:
            cap = max(nbytes, 1 << 22)
            self._pc2_stage = (torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.empty(cap, dtype=torch.uint8, device=self.device),
                               torch.cuda.Event(), torch.cuda.Event())
            if st.cuda_stream != cur.cuda_stream:
                st.wait_stream(cur)        # the fresh device buffer comes from the CURRENT stream's allocator pool: work queued there may still own the block
                                           # (only here -- reuse is ordered by the two events, and an unconditional wait removed the overlap a caller passes a stream for)
        host, dev, staged, unpacked = self._pc2_stage
        # The kernel reads what the copy wrote (same stream).  The pinned buffer is reused only after the previous message's copy
        # has executed (`staged`), the shared device staging buffer only after the previous message's KERNEL has (`unpacked`:
        # this stream waits for it, so consecutive calls may use different streams).
        staged.synchronize()                                   # no-op for a never-recorded event
        host.numpy()[:nbytes] = payload                        # one memcpy into pinned memory
        with torch.cuda.stream(st):
            st.wait_event(unpacked)
            dev[:nbytes].copy_(host[:nbytes], non_blocking=True)
            staged.record(st)
        rc = _lib.lib().avl_unpack_pointcloud2(_ptr(dev), n, step, offs["x"], offs["y"], offs["z"], offs["intensity"], _ptr(points),
                                               _ptr(count), C.c_void_p(st.cuda_stream))
        unpacked.record(st)
        if st.cuda_stream != cur.cuda_stream:
            dev.record_stream(st)                              # (the staging buffer lives in the current stream's allocator pool)
        _lib.check(rc, "avl_unpack_pointcloud2")
        return points, count

    @staticmethod
    def _nearest_in_queue(stamps, target_stamp):
        """Index selection shared by update_pcd / update_pose (mapping.py:185-219, :238-259): walk the queue for the first
        pair that brackets `target_stamp` strictly and keep the closer of the two (the earlier one on a tie); the
        queue is then trimmed from the earlier element of that pair.  Without a bracketing pair: the latest element,
        and the queue shrinks to it.  Returns (index of the pick, index to trim from)."""
        for i in range(len(stamps) - 1):
            if stamps[i + 1] > target_stamp and stamps[i] < target_stamp:
                later_is_closer = (target_stamp - stamps[i]) > (stamps[i + 1] - target_stamp)
                return (i + 1 if later_is_closer else i), i
        return len(stamps) - 1, len(stamps) - 1

    def update_pcd(self, target_stamp):
        """Closest point cloud w.r.t. target_stamp (mapping.py:185-219)."""
        pick, keep = self._nearest_in_queue([h.stamp for h in self.pcd_header_queue], target_stamp)
        pcd, stamp = self.pcd_queue[pick], self.pcd_header_queue[pick].stamp
        self.pcd_header_queue = self.pcd_header_queue[keep:]
        self.pcd_queue = self.pcd_queue[keep:]
        return pcd, stamp

    def pose_callback(self, msg):
        """mapping.py:221-226"""
        with self._lock:
            self.pose_queue.append(msg)
            if msg.header.stamp.secs >= self.test_cut_time:
                self.save_map_to_file = True

    def update_pose(self, target_stamp):
        """Closest pose w.r.t. target_stamp (mapping.py:238-259)."""
        pick, keep = self._nearest_in_queue([m.header.stamp for m in self.pose_queue], target_stamp)
        msg = self.pose_queue[pick]
        self.pose_queue = self.pose_queue[keep:]
        return msg.pose, msg.header.stamp

    def image_callback(self, msg):
        """mapping.py:261-290: semantic image arrives -> pick cloud and pose by stamp -> mapping()."""
        self.logger.log("Mapping image at: {}.{:09d}s".format(msg.header.stamp.secs, msg.header.stamp.nsecs))
        image_in = msg.data if isinstance(getattr(msg, "data", None), (np.ndarray, torch.Tensor)) else _imgmsg_to_array(msg)
        if msg.header.frame_id == "camera1":
            camera_calibration = self.cam1
        elif msg.header.frame_id == "camera6":
            camera_calibration = self.cam6
        else:
            # the reference only warns and then fails on an unbound variable (mapping.py:277-278)
            raise ValueError("cannot find camera for frame_id %s" % msg.header.frame_id)
        with self._lock:
            if self.depth_method in ["points_map", "points_raw"] and not self.points_map_indexed():
                if len(self.pcd_header_queue) == 0:
                    return
                self.pcd, self.pcd_time = self.update_pcd(msg.header.stamp)
            if len(self.pose_queue) == 0:
                return
            self.pose, self.pose_time = self.update_pose(msg.header.stamp)
            self.mapping(image_in, self.pose, camera_calibration)

    def _camera_for(self, frame_id):
        if frame_id == "camera1":
            return self.cam1
        if frame_id == "camera6":
            return self.cam6
        raise ValueError("cannot find camera for frame_id %s" % frame_id)

    def image_callback_views(self, msgs):
        """V semantic images of one trigger (mapping.py:261-290 once per message, with the stamps equal): every message names its
        camera by frame_id (:273-276); the cloud and the pose are looked up once, by the first message's stamp -- V calls of
        image_callback with one stamp pick the same pair V times (:280-285) -- and mapping_views() maps all of them in one pass."""
        msgs = list(msgs)
        if not msgs:
            raise ValueError("image_callback_views needs at least one message")
        stamp = msgs[0].header.stamp
        self.logger.log("Mapping %d images at: %d.%09ds" % (len(msgs), stamp.secs, stamp.nsecs))
        images = [m.data if isinstance(getattr(m, "data", None), (np.ndarray, torch.Tensor)) else _imgmsg_to_array(m) for m in msgs]
        cameras = [self._camera_for(m.header.frame_id) for m in msgs]
        with self._lock:
            if self.depth_method in ["points_map", "points_raw"] and not self.points_map_indexed():
                if len(self.pcd_header_queue) == 0:
                    return
                self.pcd, self.pcd_time = self.update_pcd(stamp)
            if len(self.pose_queue) == 0:
                return
            self.pose, self.pose_time = self.update_pose(stamp)
            self.mapping_views(images, self.pose, cameras)

    # ------------------------------------------------------------------ the points map's own index (MAPPING.POINTS_MAP)
    def points_map_indexed(self):
        return self.points_map_source == "index"

    def load_points_map(self, points_or_path, tile_m=None):
        """Put the site's prior point map on the device and sort it into ground tiles (points_map.PointsMapIndex; once, not per
        frame).  ``points_or_path``: [N, 4] or [4, N] (x, y, z, intensity in the world frame), NumPy or torch, float32 or float64, or
        the path of a .npy file that holds one.  ``tile_m`` None = MAPPING.POINTS_MAP.TILE_M.  Returns the index."""
        from .points_map import PointsMapIndex
        if tile_m is None:
            tile_m = self.points_map_cfg.TILE_M if self.points_map_cfg is not None else 10.0
        with self._lock:
            self.points_map_index = PointsMapIndex(points_or_path, tile_m, self.device)
            self._reduced_rect = None
            self.last_reduced = None
        return self.points_map_index

    def reduced_map_device(self, pose, cameras=None, image_size=None, stream=None):
        """The frame's cloud, cropped from the index: a float32 CUDA tensor [M, 4] in the world frame, for frame_device(pcd, "world",
        ...) and every other entry point that takes a cloud.  The crop is the tile rectangle of points_map.window for ``pose``,
        ``cameras`` (None = both of the vehicle's) and ``image_size`` = (H, W) of the projection image (None = the calibrations' own),
        with MAPPING.POINTS_MAP's RADIUS_M and MARGIN_M and the cloud's RANGE_MAX; one kernel copies it (avl_points_map_gather) on
        ``stream``.  The tensor is a view of a buffer that the next call overwrites.  When the rectangle is the previous call's,
        and the stream is the one that gather ran on, that buffer is returned as it is and nothing is launched; on another stream
        the gather runs again, so the cloud is always ordered on the stream asked for.  The buffer itself is one: a caller who
        alternates streams orders the earlier stream's readers before the later gather, as with any reused buffer.
        ``last_reduced`` = {"points": M, "tiles": tiles of the rectangle, "rows": its rows that hold a point, "reused": bool,
        "rect": (r0, r1, c0, c1)}."""
        from . import points_map as pm
        index = self.points_map_index
        if index is None:
            raise RuntimeError("MAPPING.POINTS_MAP.SOURCE = 'index' but no points map is loaded: set MAPPING.POINTS_MAP.PATH or call "
                               "SemanticMapping.load_points_map() before the first frame")
        if pose is None:
            raise ValueError("reduced_map_device needs the frame's pose: the points map is in the world frame")
        cameras = [self.cam1, self.cam6] if cameras is None else (list(cameras) if isinstance(cameras, (list, tuple)) else [cameras])
        pc = self.points_map_cfg
        radius, margin = (float(pc.RADIUS_M), float(pc.MARGIN_M)) if pc is not None else (0.0, 1.0)
        if image_size is None and radius <= 0.0:
            sizes = {tuple(cam.imSize) if cam.imSize is not None else None for cam in cameras}
            if len(sizes) != 1 or None in sizes:
                raise ValueError("reduced_map_device needs image_size = (H, W): the cameras do not carry one image size")
            w, h = sizes.pop()
            image_size = (h, w)
        rect = pm.window(index, pose, cameras, image_size, float(self.pcd_range_max), radius, margin)
        s = int(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)
        if self._reduced_buf is not None and rect == self._reduced_rect and s == self._reduced_stream:
            self.last_reduced = dict(self.last_reduced, reused=True)
            return self._reduced_buf[:self.last_reduced["points"]]
        m, runs = pm.window_count(index.offsets_host, index.rows, index.cols, rect)
        if self._reduced_buf is None or int(self._reduced_buf.shape[0]) < m:
            cap = max(m, 2 * (0 if self._reduced_buf is None else int(self._reduced_buf.shape[0])), 1 << 12)
            self._reduced_buf = torch.empty((cap, 4), dtype=torch.float32, device=self.device)
        pm.gather(index, rect, self._reduced_buf, s)
        self._reduced_rect, self._reduced_stream = rect, s
        r0, r1, c0, c1 = rect
        self.last_reduced = {"points": m, "tiles": max(r1 - r0 + 1, 0) * max(c1 - c0 + 1, 0), "rows": runs, "reused": False, "rect": rect}
        return self._reduced_buf[:m]

    # ------------------------------------------------------------------ per-frame hot path
    def mapping(self, semantic_image, pose, camera_calibration):
        """mapping.py:292-321 for the LiDAR depth methods: one fused project+vote+apply on the GPU.
        semantic_image: uint8[H,W,3] colourised labels (NumPy or a CUDA tensor)."""
        if pose is not None:
            self._live_pose = pose                                               # live_map(pose=None): the last pose mapped
            if self._scroll is not None:
                self._scroll.scroll_to(pose)                                     # host arithmetic only unless the window moves
        if self.depth_method not in ["points_map", "points_raw"]:                 # mapping.py:320-321
            img = self._as_device_u8(semantic_image)
            self.update_map_planar(self.map_dev, img, camera_calibration)
            self.frames_mapped += 1
        else:
            img = None
            if self.points_map_indexed():                                        # the frame's cloud is cropped from the index
                img = self._as_device_u8(semantic_image)
                pcd, frame_id = self.reduced_map_device(pose, [camera_calibration], img.shape[:2]), "world"
            else:
                if self.pcd is None:
                    return
                pcd, frame_id = self.pcd, self.pcd_frame_id
            if self.record_inputs:                                               # mapping.py:309-313
                self.input_list.append({"pcd": np.array(_to_numpy(pcd)), "pcd_frame_id": frame_id,
                                        "semantic_image": np.array(_to_numpy(semantic_image)), "pose": pose})
            img = self._as_device_u8(semantic_image) if img is None else img
            self.frame_device(pcd, frame_id, img, pose, camera_calibration, src_kind="rgb", **self._gate_if_plane())
            self._ground_fill_step([img], pose, [camera_calibration], pcd, frame_id)
        if self.live_cfg.ENABLED:
            self._live_map_step(pose)
        if self.cost_cfg.ENABLED:
            self._cost_map_step(pose)
        if self.save_map_to_file:                                                # mapping.py:323-345, both depth modes
            self.save_map_to_file = False
            self.finish_run()

    def mapping_views(self, semantic_images, pose, cameras):
        """mapping() for V colour images of one trigger: what V mapping() calls in view order do to the grid (bit for bit), to
        input_list (one record per view, mapping.py:309-313) and to the save_map_to_file branch (:323-345), which the first of V
        calls would run before the later views are in -- here it runs once, after the last view."""
        semantic_images, cameras = list(semantic_images), list(cameras)
        if len(semantic_images) != len(cameras) or not cameras:
            raise ValueError("mapping_views needs one camera per semantic image, got %d and %d" % (len(semantic_images), len(cameras)))
        if pose is not None:
            self._live_pose = pose
            if self._scroll is not None:
                self._scroll.scroll_to(pose)
        if self.depth_method not in ["points_map", "points_raw"]:                 # planar mode has no cloud to share
            for img, cam in zip(semantic_images, cameras):
                self.update_map_planar(self.map_dev, self._as_device_u8(img), cam)
                self.frames_mapped += 1
        else:
            images = None
            if self.points_map_indexed():
                images = [self._as_device_u8(img) for img in semantic_images]
                pcd, frame_id = self.reduced_map_device(pose, cameras, images[0].shape[:2]), "world"
            else:
                if self.pcd is None:
                    return
                pcd, frame_id = self.pcd, self.pcd_frame_id
            if self.record_inputs:
                for img in semantic_images:
                    self.input_list.append({"pcd": np.array(_to_numpy(pcd)), "pcd_frame_id": frame_id,
                                            "semantic_image": np.array(_to_numpy(img)), "pose": pose})
            images = [self._as_device_u8(img) for img in semantic_images] if images is None else images
            self.frame_device_views(pcd, frame_id, images, pose, cameras, src_kind="rgb", **self._gate_if_plane())
            self._ground_fill_step(images, pose, cameras, pcd, frame_id)
        if self.live_cfg.ENABLED:
            self._live_map_step(pose)
        if self.cost_cfg.ENABLED:
            self._cost_map_step(pose)
        if self.save_map_to_file:
            self.save_map_to_file = False
            self.finish_run()

    def finish_run(self, output_dir=None):
        """The shutdown branch of mapping() (mapping.py:323-345): dump the recorded inputs, smooth the grid
        (apply_filter), render it (render_bev_map), write global_map.png and -- with GROUND_TRUTH_DIR set --
        print IoU / accuracy / missing rate.  Filter, renderer and evaluation are GPU kernels; only the PNG and
        the printed numbers leave the device.  Returns the colour map (uint8 [Hm,Wm,3] NumPy).  A scrolling map with
        MAPPING.SITE_OVERVIEW.ENABLED first writes site_map.png, the overview of the whole, unfiltered site (site_overview), and
        with MAPPING.SITE_FINISH.ENABLED site_global_map.png, the filtered site at one pixel per cell, and the site's IoU lines
        (site_finish); global_map.png and the GROUND_TRUTH_DIR branch stay the window's."""
        from .evaluation import Test
        from .renderer import apply_filter, render_bev_map
        if self.record_inputs and self.input_list:
            self.save_inputs()
        output_dir = output_dir or self.output_dir
        os.makedirs(output_dir, exist_ok=True)
        if self._scroll is not None and self.cfg.MAPPING.SITE_OVERVIEW.ENABLED:
            self._write_site_overview(output_dir)                                # before the filter: window and store in one state
        if self._scroll is not None and self.cfg.MAPPING.SITE_FINISH.ENABLED:
            self._write_site_finish(output_dir)                                  # before the filter too: it would be applied twice
        smooth = apply_filter(self.map_dev)                                   # :332, the filtered grid replaces the map
        self.map_dev.copy_(smooth.to(self.map_dev.dtype))
        self._map_host = None
        color_dev = render_bev_map(self.map_dev, self.label_colors)              # :334
        color_map = color_dev.cpu().numpy()
        output_file = _write_picture(osp.join(output_dir, "global_map.png"), color_map)
        if output_file.endswith(".png"):
            self.logger.log("Saving image to %s" % output_file)
        if self.ground_truth_dir != "":                                          # :342-345
            Test(ground_truth_dir=self.ground_truth_dir, logger=self.logger).test_single_map(color_dev)
        return color_map

    def _write_site_overview(self, output_dir):
        """site_map.png: site_overview() with MAPPING.SITE_OVERVIEW's settings, of the unfiltered site (global_map.png is the filtered
        window).  Written by _write_picture, like global_map.png."""
        (i0, j0), picture = self.site_overview()
        picture = picture.cpu().numpy()
        if picture.size == 0:
            self.logger.log("The site is empty: no site_map.png")
            return
        k = self.last_site_overview["cells_per_pixel"]
        output_file = _write_picture(osp.join(output_dir, "site_map.png"), picture)
        self.logger.log("Saving the site overview to %s: first cell (%d, %d), %d cells per pixel" % (output_file, i0, j0, k))

    def _write_site_finish(self, output_dir):
        """site_global_map.png: site_finish() with MAPPING.SITE_FINISH's settings, the FILTERED site at one pixel per cell -- what
        global_map.png is for the window -- and, with TRUTH_PATH, the site's IoU lines.  Written by _write_picture, like
        global_map.png."""
        from .evaluation import SiteTruth, Test
        fc = self.cfg.MAPPING.SITE_FINISH
        T = self._scroll.T
        tiles = self.site_tiles("map")
        if not tiles:
            self.logger.log("The site is empty: no site_global_map.png")
            return
        cells = (max(t[0] for t in tiles) - min(t[0] for t in tiles) + 1) * (max(t[1] for t in tiles) - min(t[1] for t in tiles) + 1) * T * T
        picture = cells <= int(fc.MAX_PIXELS)
        if not picture:
            self.logger.log("The site's rectangle has %d cells, more than MAPPING.SITE_FINISH.MAX_PIXELS = %d: site_global_map.png is "
                            "skipped" % (cells, int(fc.MAX_PIXELS)))
        truth = SiteTruth.load(fc.TRUTH_PATH, T) if fc.TRUTH_PATH != "" else None
        if not picture and truth is None:
            return
        result = self.site_finish(truth=truth, picture=picture)
        if picture:
            output_file = _write_picture(osp.join(output_dir, "site_global_map.png"), result.picture.cpu().numpy())
            self.logger.log("Saving the filtered site to %s: first cell (%d, %d), %d + %d tiles" % ((output_file,) + tuple(result.origin) + tuple(result.tiles)))
        if truth is not None:
            Test.for_site(logger=self.logger).test_site(result.counts)

    # ------------------------------------------------------------------ live vehicle-centred map
    def live_map_window(self, pose, size_cells=None):
        """-> ((x0, y0), (h, w), (cx, cy)): the live map's window for `pose`.  The vehicle's cell is
        trunc((pose.xy + PCD_ORIGIN_OFFSET.xy - boundary minimum) / resolution), the expression that puts points on the grid
        (mapping.py:404-409); the window's first cell is that cell minus size // 2; (cx, cy) is the un-truncated position in cells."""
        if size_cells is None:
            size_cells = [int(float(v) / self.resolution) for v in self.live_cfg.SIZE_M]
        h, w = int(size_cells[0]), int(size_cells[1])
        xy = np.array(_pose_to_array(pose)[:2], dtype=np.float64)
        cxy = (xy + np.array(PCD_ORIGIN_OFFSET[:2]) - np.array([self.map_boundary[0][0], self.map_boundary[1][0]], dtype=np.float64)) / self.resolution
        with np.errstate(invalid="ignore"):
            centre = cxy.astype(np.int32)
        return (int(centre[0]) - h // 2, int(centre[1]) - w // 2), (h, w), (float(cxy[0]), float(cxy[1]))

    def _live_settings(self, pose):
        """MAPPING.LIVE_MAP's filter, renderer, fill and car settings as keyword arguments of renderer.render_window / render_view"""
        from . import renderer
        lc = self.live_cfg
        car = None
        if lc.DRAW_CAR:
            c, s = pose_heading(pose)
            cx, cy = self.live_map_window(pose, (1, 1))[2]
            car = renderer.car_block(cx, cy, c, s, self.resolution, lc.CAR_SIZE)
        if lc.RENDER not in ("argmax", "thresholds"):
            raise ValueError("MAPPING.LIVE_MAP.RENDER must be 'argmax' or 'thresholds', not %r" % (lc.RENDER,))
        thresholds = priority = None
        if lc.RENDER == "thresholds":
            thresholds = lc.THRESHOLDS if lc.THRESHOLDS is not None else [0.01] * self.map_depth
            priority = lc.PRIORITY
        return dict(filter=bool(lc.FILTER), thresholds=thresholds, priority=priority, fill=bool(lc.FILL_BLACK),
                    fill_priority=lc.FILL_PRIORITY, car=car)

    def live_map(self, pose=None, size_cells=None, out=None, stream=None):
        """The map around the vehicle as a uint8 CUDA tensor [h, w, 3], rendered by one kernel (renderer.render_window with
        MAPPING.LIVE_MAP's settings): out[i, j] is grid cell (x0 + i, y0 + j) in the global map's orientation (live_view() is the
        heading-up picture), black where the window leaves the grid, the ego footprint painted last.  ``pose`` None = the last pose mapped;
        ``size_cells`` None = LIVE_MAP.SIZE_M.  Reads the grid only -- unlike finish_run, which replaces it by its filtered self.
        On several GPUs this is the rank's private grid, not global_map()."""
        from . import renderer
        pose = self._live_pose if pose is None else pose
        if pose is None:
            raise RuntimeError("live_map needs a pose: none was given and no frame has been mapped with one")
        origin, size, _ = self.live_map_window(pose, size_cells)
        img = renderer.render_window(self.map_dev, self.label_colors, origin, size, out=out, stream=stream, **self._live_settings(pose))
        self.live_map_origin = origin
        return img

    def live_view_matrix(self, pose, size_px=None):
        """-> 2 x 3 float64 ndarray: renderer.view_matrix for `pose` with MAPPING.LIVE_VIEW's geometry -- the vehicle's un-truncated
        grid position (live_map_window's) at pixel ANCHOR * size, its heading up, METRES_PER_PIXEL / RESOLUTION cells per pixel
        (0 = one cell per pixel).  ``size_px`` None = LIVE_VIEW.SIZE_PX."""
        from . import renderer
        vc = self.live_view_cfg
        size = vc.SIZE_PX if size_px is None else size_px
        mpp = float(vc.METRES_PER_PIXEL)
        return renderer.view_matrix(self.live_map_window(pose, (1, 1))[2], pose_heading(pose),
                                    mpp / self.resolution if mpp > 0.0 else 1.0, size, vc.ANCHOR)

    def live_view(self, pose=None, size_px=None, out=None, stream=None):
        """The heading-up live map as a uint8 CUDA tensor [h, w, 3], rendered by one kernel (renderer.render_view through
        live_view_matrix(pose), with MAPPING.LIVE_MAP's filter, renderer, fill and car settings): the vehicle's heading points up,
        black where the view leaves the grid, the ego footprint painted last.  ``pose`` None = the last pose mapped; ``size_px``
        None = LIVE_VIEW.SIZE_PX.  Reads the grid only."""
        from . import renderer
        pose = self._live_pose if pose is None else pose
        if pose is None:
            raise RuntimeError("live_view needs a pose: none was given and no frame has been mapped with one")
        size = [int(v) for v in (self.live_view_cfg.SIZE_PX if size_px is None else size_px)]
        matrix = self.live_view_matrix(pose, size)
        img = renderer.render_view(self.map_dev, self.label_colors, matrix, size, out=out, stream=stream, **self._live_settings(pose))
        self.live_view_matrix_last = matrix
        return img

    def _live_map_step(self, pose):
        """mapping()'s live branch: on every EVERY-th call (the first included) render the window (the heading-up view with
        MAPPING.LIVE_VIEW.HEADING_UP), keep it, start its copy into pinned memory and --
        under ROS -- publish it (sensor_msgs/Image, 8UC3, as mapping.py:349-350 does with the end-of-run map)."""
        self._live_frames = getattr(self, "_live_frames", 0) + 1
        if self._live_pose is None or (self._live_frames - 1) % max(int(self.live_cfg.EVERY), 1) != 0:
            return
        if self.live_view_cfg.HEADING_UP:
            img = self.live_view()                            # records live_view_matrix_last
            self.live_map_origin = None                       # the picture is no window of the grid
        else:
            img = self.live_map()
        self.live_map_image = img
        if self.live_map_host is None or self.live_map_host.shape != img.shape:
            self.live_map_host = torch.empty(tuple(img.shape), dtype=torch.uint8).pin_memory()
            self.live_map_ready = torch.cuda.Event()
        self.live_map_host.copy_(img, non_blocking=True)      # stream-ordered behind the kernel and behind the previous copy
        self.live_map_ready.record(torch.cuda.current_stream(self.device))
        if self._ros is not None and self.pub_semantic_local_map is not None:
            self.live_map_ready.synchronize()
            msg = self._ros_image_cls()
            msg.height, msg.width = int(img.shape[0]), int(img.shape[1])
            msg.encoding, msg.is_bigendian, msg.step = "8UC3", 0, int(img.shape[1]) * 3
            msg.data = self.live_map_host.numpy().tobytes()
            msg.header.frame_id = "semantic_local_map"
            self.pub_semantic_local_map.publish(msg)

    # ------------------------------------------------------------------ live cost map (MAPPING.COST_MAP)
    def _parse_cost_map(self):
        """MAPPING.COST_MAP as renderer.cost_window's keyword arguments (without the car, which needs a pose).  ValueError for a
        CLASS_COST that has not one entry per map class and for an inflation radius above _lib.AVL_COST_MAX_RADIUS cells."""
        from . import renderer
        cc = self.cost_cfg
        class_cost = [int(v) for v in cc.CLASS_COST]
        if len(class_cost) != self.map_depth:
            raise ValueError("MAPPING.COST_MAP.CLASS_COST has %d entries for %d map classes (LABELS_NAMES)" % (len(class_cost), self.map_depth))
        radius = int(float(cc.INFLATION_RADIUS_M) / self.resolution)
        if not 0 <= radius <= _lib.AVL_COST_MAX_RADIUS:
            raise ValueError("MAPPING.COST_MAP.INFLATION_RADIUS_M = %g is %d cells of %g m: 0 .. %d" % (
                float(cc.INFLATION_RADIUS_M), radius, self.resolution, _lib.AVL_COST_MAX_RADIUS))
        if cc.RENDER not in ("argmax", "thresholds"):
            raise ValueError("MAPPING.COST_MAP.RENDER must be 'argmax' or 'thresholds', not %r" % (cc.RENDER,))
        if cc.ORDER not in ("xy", "yx"):
            raise ValueError("MAPPING.COST_MAP.ORDER must be 'xy' or 'yx', not %r" % (cc.ORDER,))
        thresholds = priority = None
        if cc.RENDER == "thresholds":
            thresholds = cc.THRESHOLDS if cc.THRESHOLDS is not None else [0.01] * self.map_depth
            priority = cc.PRIORITY
        table = renderer.inflation_table(radius, self.resolution, float(cc.INSCRIBED_RADIUS_M), float(cc.DECAY_PER_M))
        return dict(class_cost=class_cost, unknown_cost=int(cc.UNKNOWN_COST), radius_cells=radius, inflation=table,
                    filter=bool(cc.FILTER), thresholds=thresholds, priority=priority, order=str(cc.ORDER))

    def _cost_window(self, pose, size_cells):
        if size_cells is None:
            size_cells = [int(float(v) / self.resolution) for v in self.cost_cfg.SIZE_M]
        return self.live_map_window(pose, size_cells)

    def cost_map(self, pose=None, size_cells=None, d2=False, out=None, stream=None):
        """The cost map around the vehicle as an int8 CUDA tensor (renderer.cost_window with MAPPING.COST_MAP's settings): the
        window is live_map_window's for COST_MAP.SIZE_M, element (i, j) stands for grid cell (x0 + i, y0 + j) and the tensor is
        [w, h] with ORDER "yx" -- nav_msgs/OccupancyGrid's data, x fastest; cost_map_info() has its other fields -- or [h, w] with
        "xy".  With CLEAR_FOOTPRINT the cells under the ego rectangle (car_block, CAR_SIZE) cost 0 and do not inflate.  ``d2`` True
        also returns the squared clearance in cells, uint16 (65535: no lethal cell within the radius): -> (cost, d2).  ``pose``
        None = the last pose mapped; ``size_cells`` None = COST_MAP.SIZE_M.  Reads the grid only."""
        from . import renderer
        pose = self._live_pose if pose is None else pose
        if pose is None:
            raise RuntimeError("cost_map needs a pose: none was given and no frame has been mapped with one")
        if self._cost_par is None:
            self._cost_par = self._parse_cost_map()
        origin, size, (cx, cy) = self._cost_window(pose, size_cells)
        car = None
        if self.cost_cfg.CLEAR_FOOTPRINT:
            c, s = pose_heading(pose)
            car = renderer.car_block(cx, cy, c, s, self.resolution, self.cost_cfg.CAR_SIZE)
        res = renderer.cost_window(self.map_dev, origin, size, car=car, out=out, d2_out=True if d2 else None, stream=stream, **self._cost_par)
        self.cost_map_origin, self.cost_map_size = origin, size
        return res

    def cost_map_info(self, pose=None, size_cells=None):
        """The nav_msgs/OccupancyGrid fields of the cost map -- of the last one, or with ``pose`` of the one cost_map(pose, size_cells)
        gives: {"resolution", "width", "height", "origin_x", "origin_y"}.  width counts the cells along the grid's x (the window's
        h), height those along y (its w); (origin_x, origin_y) is the corner of the window's first cell in the map frame, the inverse
        of live_map_window's expression: boundary minimum + cell * resolution - PCD_ORIGIN_OFFSET."""
        if pose is not None:
            origin, size, _ = self._cost_window(pose, size_cells)
        elif self.cost_map_origin is not None:
            origin, size = self.cost_map_origin, self.cost_map_size
        else:
            raise RuntimeError("cost_map_info needs a pose or a cost map: none was given and cost_map has not run")
        return {"resolution": float(self.resolution), "width": int(size[0]), "height": int(size[1]),
                "origin_x": float(self.map_boundary[0][0]) + origin[0] * float(self.resolution) - PCD_ORIGIN_OFFSET[0],
                "origin_y": float(self.map_boundary[1][0]) + origin[1] * float(self.resolution) - PCD_ORIGIN_OFFSET[1]}

    def _cost_map_step(self, pose):
        """mapping()'s cost map branch: on every EVERY-th call (the first included) compute the cost map, keep it, start its copy into
        pinned memory and -- under ROS -- publish it as a nav_msgs/OccupancyGrid on /semantic_cost_map."""
        self._cost_frames = getattr(self, "_cost_frames", 0) + 1
        if self._live_pose is None or (self._cost_frames - 1) % max(int(self.cost_cfg.EVERY), 1) != 0:
            return
        img = self.cost_map()
        self.cost_map_image = img
        if self.cost_map_host is None or self.cost_map_host.shape != img.shape:
            self.cost_map_host = torch.empty(tuple(img.shape), dtype=torch.int8).pin_memory()
            self.cost_map_ready = torch.cuda.Event()
        self.cost_map_host.copy_(img, non_blocking=True)      # stream-ordered behind the kernels and behind the previous copy
        self.cost_map_ready.record(torch.cuda.current_stream(self.device))
        if self._ros is not None and self.pub_semantic_cost_map is not None:
            self.cost_map_ready.synchronize()
            info = self.cost_map_info()
            host = self.cost_map_host.numpy()
            msg = self._ros_grid_cls()
            msg.header.frame_id = "map"
            msg.info.resolution = info["resolution"]
            msg.info.width, msg.info.height = info["width"], info["height"]
            msg.info.origin.position.x, msg.info.origin.position.y = info["origin_x"], info["origin_y"]
            msg.info.origin.orientation.w = 1.0
            msg.data = (host if self.cost_cfg.ORDER == "yx" else host.T).ravel().tolist()
            self.pub_semantic_cost_map.publish(msg)

    # ------------------------------------------------------------------ occlusion culling (MAPPING.OCCLUSION)
    def occlusion_enabled(self):
        return self.occlusion_cfg is not None and bool(self.occlusion_cfg.ENABLED)

    def _occlusion(self, V, ih, iw, culled=None):
        """struct avl_occlusion for V views of an ih x iw projection image, from MAPPING.OCCLUSION.  The depth scratch is allocated on
        first use per (V, Hc, Wc) and reused (every call resets it itself).  ``culled``: (int32 CUDA tensor, first element) that
        receives the V counts; None = a fresh-or-reused ``self.last_culled`` of V elements."""
        oc = self.occlusion_cfg
        s = int(oc.CELL_PX)
        words = int(_lib.lib().avl_occlusion_depth_words(int(iw), int(ih), s, int(V)))
        if words <= 0:
            raise ValueError("MAPPING.OCCLUSION.CELL_PX = %r (1..64) for %d views of %dx%d" % (oc.CELL_PX, V, iw, ih))
        key = (int(V), -(-int(ih) // s), -(-int(iw) // s))
        depth = self._occl_depth.get(key)
        if depth is None:
            depth = self._occl_depth[key] = torch.empty(words, dtype=torch.int32, device=self.device)
        if culled is None:
            if self.last_culled is None or int(self.last_culled.numel()) != V:
                self.last_culled = torch.zeros(V, dtype=torch.int32, device=self.device)
            culled = (self.last_culled, 0)
        o = _lib.AvlOcclusion()
        o.cell_px, o.radius = s, int(oc.RADIUS)
        o.rel_tol, o.abs_tol = float(oc.REL_TOL), float(oc.ABS_TOL)
        o.depth, o.depth_words = depth.data_ptr(), words
        o.culled = culled[0].data_ptr() + 4 * int(culled[1])
        return o

    def visibility_device(self, pcd, pcd_frame_id, pose, cameras, image_size, return_keys=False):
        """The occlusion rule alone (avl_occlusion_visibility, MAPPING.OCCLUSION's parameters whether ENABLED or not): for every
        camera of ``cameras`` (one calibration or a list) and every point of ``pcd``, 0 = the point is no candidate of that view
        (behind the vehicle, out of range or outside the ``image_size`` = (H, W) image), 1 = visible, 2 = culled.  Returns a uint8
        CUDA tensor [V, N]; with ``return_keys`` also the float32 depth keys [V, N] (0 where the state is 0).  ``last_culled``
        receives the per-view counts of state 2.  A caller who wants a culled semantic cloud filters project_pcd's input with it."""
        cameras = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras]
        V = len(cameras)
        if V < 1:
            raise ValueError("visibility_device needs at least one camera")
        ih, iw = int(image_size[0]), int(image_size[1])
        n = int(_lib.points_view(pcd, self.device)[1])
        state = torch.empty((V, n), dtype=torch.uint8, device=self.device)
        keys = torch.empty((V, n), dtype=torch.float32, device=self.device) if return_keys else None
        self.last_culled = torch.zeros(V, dtype=torch.int32, device=self.device)
        for v0 in range(0, V, _lib.AVL_MAX_VIEWS):
            cams = cameras[v0:v0 + _lib.AVL_MAX_VIEWS]
            view, T, _, P, s = self._frame_args(pcd, pcd_frame_id, pose, np.stack([np.asarray(c.P, dtype=np.float64) for c in cams]), grid=False)
            occ = self._occlusion(len(cams), ih, iw, culled=(self.last_culled, v0))
            rc = _lib.lib().avl_occlusion_visibility(*view, len(cams), P, T, float(self.pcd_range_max), iw, ih, C.byref(occ),
                                                     _ptr(state[v0:]), _ptr(keys[v0:]) if return_keys else None, s)
            _lib.check(rc, "avl_occlusion_visibility")
        return (state, keys) if return_keys else state

    def frame_device(self, pcd, pcd_frame_id, semantic, pose, camera_calibration, src_kind="rgb",
                     image_size=None, net_palette=PALETTE_19, stream=None, _culled=None, net_size=None, _abstained=None, _gate=None,
                     _gated=None):
        """Fused frame (avl_fused_frame; avl_fused_frame_occl with MAPPING.OCCLUSION.ENABLED).  ``pcd``: NumPy/torch [4,N]
        float64|float32 (SoA, the reference layout) or [N,4] float32 (AoS); ``semantic``: CUDA uint8 tensor, either the colour
        image [H,W,3] (src_kind="rgb") or a class-id map [h,w] (src_kind="classmap", sampled as the
        nearest-upscaled image of size ``image_size`` = (H, W)).  With src_kind="logits" ``semantic`` is a plan's fp32 logits
        [h',w',K] (SegNet.logits): every point takes the arg-max of the logits interpolated to ``net_size`` = (h, w) (the network's
        input; ``image_size`` by default) at its pixel, and abstains when the top-1 minus top-2 margin is below ``self.min_margin``
        (MAPPING.CONFIDENCE.MIN_MARGIN); ``last_abstained`` receives the count (avl_fused_frame_logits).  With
        MAPPING.HEIGHT_GATE.ENABLED or MAPPING.ELEVATION.ENABLED every source goes through avl_fused_frame_views_height: the gate
        needs a ground plane (set_ground_plane; RuntimeError without one) and ``last_gated`` receives its count."""
        if src_kind == "logits":
            return self._frame_device_logits(pcd, pcd_frame_id, logits_views(semantic)[0], pose, [camera_calibration], image_size, net_size,
                                             net_palette, stream, _culled, _abstained, _gate, _gated)
        assert semantic.dtype == torch.uint8
        sh, sw, ih, iw, kind, lut = self._semantic_source(semantic.shape, src_kind, image_size, net_palette)
        view, T, gs, P, s = self._frame_args(pcd, pcd_frame_id, pose, camera_calibration.P, stream)
        semantic = semantic.contiguous()
        if self._height_routed(_gate):
            occ = C.byref(self._occlusion(1, ih, iw, _culled)) if self.occlusion_enabled() else None
            ht = self._height(1, pose, pcd_frame_id, _gate, _gated)
            src = (C.c_void_p * 1)(semantic.data_ptr())
            rc = _lib.lib().avl_fused_frame_views_height(C.byref(gs), *view, 1, P, T, float(self.pcd_range_max), kind, src, sw, sh, iw, ih, lut,
                                                         self._colors_host(), _dbl(self.confusion_matrix), self._bonus_classes(), None, occ,
                                                         C.byref(ht), s)
            _lib.check(rc, "avl_fused_frame_views_height")
        elif self.occlusion_enabled():
            occ = self._occlusion(1, ih, iw, _culled)
            rc = _lib.lib().avl_fused_frame_occl(C.byref(gs), *view, P, T, float(self.pcd_range_max), kind, _ptr(semantic), sw, sh, iw, ih, lut,
                                                 self._colors_host(), _dbl(self.confusion_matrix), self._bonus_classes(), C.byref(occ), s)
            _lib.check(rc, "avl_fused_frame_occl")
        else:
            rc = _lib.lib().avl_fused_frame(C.byref(gs), *view, P, T, float(self.pcd_range_max), kind, _ptr(semantic), sw, sh, iw, ih, lut,
                                            self._colors_host(), _dbl(self.confusion_matrix), self._bonus_classes(), s)
            _lib.check(rc, "avl_fused_frame")
        self._map_host = None
        self.frames_mapped += 1

    def frame_device_views(self, pcd, pcd_frame_id, semantics, pose, cameras, src_kind="classmap", image_size=None,
                           net_palette=PALETTE_19, stream=None, net_size=None, _gate=None):
        """V cameras on one cloud in one fused pass (avl_fused_frame_views): the grid ends bit-identical to V frame_device calls
        in view order.  ``semantics``: a uint8 CUDA tensor [V,h,w] of class maps (a batched plan's label buffer goes in as it is)
        or [V,H,W,3] of colour images (src_kind="rgb"), or a list of V such tensors of one size; with src_kind="logits" an fp32
        CUDA tensor [V,h',w',K] (a batched plan's logits) or a list of V tensors [h',w',K], ``net_size`` as in frame_device;
        ``cameras``: V calibrations.  More than AVL_MAX_VIEWS views, or more vote bits than a view's byte of the mask holds
        (classes + lane classes > 8), are mapped by sequential frame_device calls.  With MAPPING.HEIGHT_GATE.ENABLED or
        MAPPING.ELEVATION.ENABLED the pass is avl_fused_frame_views_height; the sequential fall-back then gates per call
        (``last_gated`` still holds one count per view) and lets the elevation layer take a point once per CALL, so a point that
        several of the fall-back's views see enters the layer once per such view, not once per trigger."""
        cameras = list(cameras)
        V = len(cameras)
        if V < 1:
            raise ValueError("frame_device_views needs at least one camera")
        if src_kind == "logits":
            return self._frame_device_logits(pcd, pcd_frame_id, logits_views(semantics, V)[0], pose, cameras, image_size, net_size,
                                             net_palette, stream, _gate=_gate)
        want_dim = 3 if src_kind == "rgb" else 2
        if isinstance(semantics, torch.Tensor):
            if semantics.dim() != want_dim + 1 or int(semantics.shape[0]) != V:
                raise ValueError("semantics has shape %s for %d %s views" % (tuple(semantics.shape), V, src_kind))
            views = [semantics[v] for v in range(V)]
        else:
            views = list(semantics)
            if len(views) != V:
                raise ValueError("%d semantic sources for %d cameras" % (len(views), V))
        shape = tuple(views[0].shape)
        for t in views:
            if tuple(t.shape) != shape or t.dtype != torch.uint8 or not t.is_cuda:
                raise ValueError("the views' semantic sources must be uint8 CUDA tensors of one size")
        sh, sw, ih, iw, kind, lut = self._semantic_source(shape, src_kind, image_size, net_palette)
        bonus = self._bonus_classes()
        occlusion = self.occlusion_enabled()
        gating = self._height_routed(_gate) and self._gate_on(_gate)
        if V > _lib.AVL_MAX_VIEWS or (V > 1 and self.map_depth + bin(bonus).count("1") > 8):
            culled = torch.zeros(V, dtype=torch.int32, device=self.device) if occlusion else None
            gated = torch.zeros(V, dtype=torch.int32, device=self.device) if gating else None
            for v, (t, cam) in enumerate(zip(views, cameras)):
                self.frame_device(pcd, pcd_frame_id, t, pose, cam, src_kind=src_kind, image_size=image_size, net_palette=net_palette,
                                  stream=stream, _culled=(culled, v) if occlusion else None, _gate=_gate,
                                  _gated=(gated, v) if gating else None)
            if occlusion:
                self.last_culled = culled
            if gating:
                self.last_gated = gated
            return
        view, T, gs, P, s = self._frame_args(pcd, pcd_frame_id, pose, np.stack([np.asarray(cam.P, dtype=np.float64) for cam in cameras]), stream)
        views = [t.contiguous() for t in views]
        src = (C.c_void_p * V)(*[t.data_ptr() for t in views])
        if self._height_routed(_gate):
            occ = C.byref(self._occlusion(V, ih, iw)) if occlusion else None
            ht = self._height(V, pose, pcd_frame_id, _gate)
            rc = _lib.lib().avl_fused_frame_views_height(C.byref(gs), *view, V, P, T, float(self.pcd_range_max), kind, src, sw, sh, iw, ih, lut,
                                                         self._colors_host(), _dbl(self.confusion_matrix), bonus, None, occ, C.byref(ht), s)
            _lib.check(rc, "avl_fused_frame_views_height")
        elif occlusion:
            occ = self._occlusion(V, ih, iw)
            rc = _lib.lib().avl_fused_frame_views_occl(C.byref(gs), *view, V, P, T, float(self.pcd_range_max), kind, src, sw, sh, iw, ih, lut,
                                                       self._colors_host(), _dbl(self.confusion_matrix), bonus, C.byref(occ), s)
            _lib.check(rc, "avl_fused_frame_views_occl")
        else:
            rc = _lib.lib().avl_fused_frame_views(C.byref(gs), *view, V, P, T, float(self.pcd_range_max), kind, src, sw, sh, iw, ih, lut,
                                                  self._colors_host(), _dbl(self.confusion_matrix), bonus, s)
            _lib.check(rc, "avl_fused_frame_views")
        self._map_host = None
        self.frames_mapped += V

    # ------------------------------------------------------------------ labels from interpolated logits (MAPPING.CONFIDENCE)
    def _point_logits(self, views, image_size, net_size, abstained=None):
        """-> (struct avl_point_logits for the checked ``views`` of logits_views(), ih, iw): the points are projected to
        ``image_size`` (``net_size``, else the logits' own size, when None) and the logits interpolated to ``net_size``
        (``image_size`` when None).  ``abstained``: (int32 CUDA tensor, first element) that receives the counts, or None."""
        _, (h, w, K), ld = logits_views(views, len(views))
        size = image_size if image_size is not None else (net_size if net_size is not None else (h, w))
        ih, iw = int(size[0]), int(size[1])
        nh, nw = (ih, iw) if net_size is None else (int(net_size[0]), int(net_size[1]))
        pl = _lib.AvlPointLogits()
        for v, t in enumerate(views):
            pl.logits[v] = t.data_ptr()
        pl.h, pl.w, pl.K, pl.ld = h, w, K, ld
        pl.net_h, pl.net_w = nh, nw
        pl.min_margin = float(self.min_margin)
        pl.abstained = None if abstained is None else abstained[0].data_ptr() + 4 * int(abstained[1])
        return pl, ih, iw

    def _frame_device_logits(self, pcd, pcd_frame_id, views, pose, cameras, image_size, net_size, net_palette, stream,
                             _culled=None, _abstained=None, _gate=None, _gated=None):
        """frame_device / frame_device_views for src_kind="logits": ``views`` are V checked logits tensors (logits_views)."""
        V = len(cameras)
        bonus = self._bonus_classes()
        occlusion = self.occlusion_enabled()
        gating = self._height_routed(_gate) and self._gate_on(_gate)
        if V > _lib.AVL_MAX_VIEWS or (V > 1 and self.map_depth + bin(bonus).count("1") > 8):
            abstained = torch.zeros(V, dtype=torch.int32, device=self.device)
            culled = torch.zeros(V, dtype=torch.int32, device=self.device) if occlusion else None
            gated = torch.zeros(V, dtype=torch.int32, device=self.device) if gating else None
            for v, (t, cam) in enumerate(zip(views, cameras)):
                self._frame_device_logits(pcd, pcd_frame_id, [t], pose, [cam], image_size, net_size, net_palette, stream,
                                          (culled, v) if occlusion else None, (abstained, v), _gate, (gated, v) if gating else None)
            self.last_abstained = abstained
            if occlusion:
                self.last_culled = culled
            if gating:
                self.last_gated = gated
            return
        if _abstained is None:
            if self.last_abstained is None or int(self.last_abstained.numel()) != V:
                self.last_abstained = torch.zeros(V, dtype=torch.int32, device=self.device)
            _abstained = (self.last_abstained, 0)
        pl, ih, iw = self._point_logits(views, image_size, net_size, _abstained)
        view, T, gs, P, s = self._frame_args(pcd, pcd_frame_id, pose, np.stack([np.asarray(cam.P, dtype=np.float64) for cam in cameras]), stream)
        occ = C.byref(self._occlusion(V, ih, iw, _culled)) if occlusion else None
        lut, cm = self._lut_host(net_palette), _dbl(self.confusion_matrix)
        if self._height_routed(_gate):
            ht = self._height(V, pose, pcd_frame_id, _gate, _gated)
            rc = _lib.lib().avl_fused_frame_views_height(C.byref(gs), *view, V, P, T, float(self.pcd_range_max), 0, None, 0, 0, iw, ih, lut, None,
                                                         cm, bonus, C.byref(pl), occ, C.byref(ht), s)
            _lib.check(rc, "avl_fused_frame_views_height")
        elif V == 1:
            rc = _lib.lib().avl_fused_frame_logits(C.byref(gs), *view, P, T, float(self.pcd_range_max), C.byref(pl), iw, ih, lut, cm, bonus, occ, s)
            _lib.check(rc, "avl_fused_frame_logits")
        else:
            rc = _lib.lib().avl_fused_frame_views_logits(C.byref(gs), *view, V, P, T, float(self.pcd_range_max), C.byref(pl), iw, ih, lut, cm,
                                                         bonus, occ, s)
            _lib.check(rc, "avl_fused_frame_views_logits")
        self._map_host = None
        self.frames_mapped += V

    def point_labels_device(self, pcd, pcd_frame_id, pose, cameras, logits, image_size, net_size=None):
        """The logits rule alone (avl_point_labels; struct avl_point_logits in include/avl_hip.h), with ``self.min_margin``: for every
        camera of ``cameras`` (one calibration or a list) and every point of ``pcd``, on the grid or not, the class the point takes
        from that view's ``logits`` ([h',w',K], [V,h',w',K] or a list), 254 where it abstains and 255 where it is no candidate of the
        view.  Returns (state uint8 CUDA [V, N], margin float32 CUDA [V, N], 0 where the state is 255).  ``last_abstained`` receives
        the per-view counts of state 254."""
        single = not isinstance(cameras, (list, tuple))
        cameras = [cameras] if single else list(cameras)
        V = len(cameras)
        if V < 1:
            raise ValueError("point_labels_device needs at least one camera")
        if single and isinstance(logits, torch.Tensor) and logits.dim() == 3:
            logits = [logits]
        views = logits_views(logits, V)[0]
        n = int(_lib.points_view(pcd, self.device)[1])
        state = torch.empty((V, n), dtype=torch.uint8, device=self.device)
        margin = torch.empty((V, n), dtype=torch.float32, device=self.device)
        self.last_abstained = torch.zeros(V, dtype=torch.int32, device=self.device)
        for v0 in range(0, V, _lib.AVL_MAX_VIEWS):
            cams = cameras[v0:v0 + _lib.AVL_MAX_VIEWS]
            pl, ih, iw = self._point_logits(views[v0:v0 + len(cams)], image_size, net_size, (self.last_abstained, v0))
            view, T, _, P, s = self._frame_args(pcd, pcd_frame_id, pose, np.stack([np.asarray(c.P, dtype=np.float64) for c in cams]), grid=False)
            rc = _lib.lib().avl_point_labels(*view, len(cams), P, T, float(self.pcd_range_max), iw, ih, C.byref(pl), _ptr(state[v0:]),
                                             _ptr(margin[v0:]), s)
            _lib.check(rc, "avl_point_labels")
        return state, margin

    # ------------------------------------------------------------------ dense ground fill (MAPPING.GROUND_FILL)
    def ground_fill_enabled(self):
        return self.ground_fill_cfg is not None and bool(self.ground_fill_cfg.ENABLED)

    def set_ground_plane(self, plane):
        """The ground plane of the fill, in the VELODYNE frame: a Plane3D (the node's ``plane``), a GroundPlaneResult that has been
        to the host (``estimate_ground_plane().host()``) or four numbers (a, b, c, d).  ValueError for anything that is not finite."""
        from .ground_plane import plane_coefficients
        p = plane_coefficients(plane)
        if not np.isfinite(p).all():
            raise ValueError("ground plane %r is not finite" % (p.tolist(),))
        self.ground_plane = p

    def plane_callback(self, msg):
        """shape_msgs/Plane on /estimated_plane, as the segmentation node takes it (vision_semantic_segmentation_node.py:199-201)."""
        self.set_ground_plane([msg.coef[0], msg.coef[1], msg.coef[2], msg.coef[3]])

    def _ground_fill_class_mask(self):
        names = list(self.ground_fill_cfg.CLASSES)
        unknown = [n for n in names if n not in self.label_names]
        if unknown:
            raise ValueError("MAPPING.GROUND_FILL.CLASSES names %r, LABELS_NAMES has %r" % (unknown, list(self.label_names)))
        return sum(1 << i for i, name in enumerate(self.label_names) if name in names)

    def ground_fill_device(self, semantics, pose, cameras, plane=None, grid_frame_id=None, src_kind="classmap", image_size=None,
                           net_size=None, net_palette=PALETTE_19, window=None, pcd=None, pcd_frame_id=None, stream=None):
        """Dense ground fill (avl_ground_fill_views / _logits; the rule at struct avl_ground_fill in include/avl_hip.h): every cell of
        ``window`` puts its centre on the ground plane, projects it into each camera of ``cameras`` (one calibration or a list) and
        takes that pixel's label of ``semantics`` as one update, with MAPPING.GROUND_FILL's RANGE_MAX, CLASSES and WEIGHT.  Sources
        as frame_device_views takes them (``src_kind`` "classmap", "rgb" or "logits"; one tensor for one camera).  ``plane``: in the
        velodyne frame (set_ground_plane's forms), None = the plane last set.  ``grid_frame_id``: the frame of the clouds mapped onto
        this grid (None = ``self.pcd_frame_id``, "velodyne" without a cloud); any other than "velodyne" needs the pose.  ``window``:
        ((x0, y0), (h, w)) in cells, None = live_map_window of GROUND_FILL.SIZE_M around the vehicle (around the frame's origin for a
        velodyne-frame grid).  With MAPPING.OCCLUSION.ENABLED and a cloud ``pcd`` (in ``pcd_frame_id``, None = the grid's frame) the
        depth buffer is filled from it first (avl_occlusion_depth, the cloud's own range) and a cell behind a real point is culled.
        Sets ``last_filled`` and, as the frame calls do, ``last_abstained`` and ``last_culled``.  ValueError for a plane whose normal
        in the grid's frame is more than GROUND_FILL.MAX_TILT_DEG from the z axis."""
        from .ground_plane import plane_tilt_deg
        gf_cfg = self.ground_fill_cfg
        single = not isinstance(cameras, (list, tuple))
        cameras = [cameras] if single else list(cameras)
        V = len(cameras)
        if V < 1:
            raise ValueError("ground_fill_device needs at least one camera")
        if isinstance(semantics, torch.Tensor) and semantics.dim() == {"rgb": 3, "logits": 3}.get(src_kind, 2):
            semantics = [semantics]                                  # one view's tensor, not a stack of views
        plane = self.ground_plane if plane is None else plane
        if plane is None:
            raise RuntimeError("ground_fill_device needs a ground plane: none was given and set_ground_plane has not been called")
        if grid_frame_id is None:
            grid_frame_id = self.pcd_frame_id if self.pcd_frame_id is not None else "velodyne"
        plane_g, T_np = self._plane_in_grid_frame(plane, pose, grid_frame_id)
        tilt = plane_tilt_deg(plane_g)
        if not tilt <= float(gf_cfg.MAX_TILT_DEG):                   # a NaN (zero normal) fails the comparison too
            raise ValueError("ground plane %r is tilted by %g degrees in the grid's frame (MAPPING.GROUND_FILL.MAX_TILT_DEG = %g)" % (
                plane_g.tolist(), tilt, float(gf_cfg.MAX_TILT_DEG)))
        if window is None:
            centre = pose if grid_frame_id != "velodyne" else np.zeros(7)
            window = self.live_map_window(centre, [int(float(v) / self.resolution) for v in gf_cfg.SIZE_M])[:2]
        (x0, y0), (h, w) = window
        if src_kind == "logits":
            views = logits_views(semantics, V)[0]
        else:
            views = [semantics[v] for v in range(V)] if isinstance(semantics, torch.Tensor) else list(semantics)
            if len(views) != V:
                raise ValueError("%d semantic sources for %d cameras" % (len(views), V))
            shape = tuple(views[0].shape)
            for t in views:
                if tuple(t.shape) != shape or t.dtype != torch.uint8 or not t.is_cuda:
                    raise ValueError("the views' semantic sources must be uint8 CUDA tensors of one size")
            sh, sw, ih, iw, kind, lut = self._semantic_source(shape, src_kind, image_size, net_palette)
            views = [t.contiguous() for t in views]
        cm = _dbl(np.asarray(self.confusion_matrix, dtype=np.float64) * float(gf_cfg.WEIGHT))
        T = _dbl(T_np) if T_np is not None else None
        s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)
        gs = self.grid.struct()
        occlusion = self.occlusion_enabled() and pcd is not None
        self.last_filled = torch.zeros(V, dtype=torch.int32, device=self.device)
        if src_kind == "logits":
            self.last_abstained = torch.zeros(V, dtype=torch.int32, device=self.device)
        if occlusion:
            self.last_culled = torch.zeros(V, dtype=torch.int32, device=self.device)
        gf = _lib.AvlGroundFill()
        gf.x0, gf.y0, gf.h, gf.w = int(x0), int(y0), int(h), int(w)
        gf.plane[:] = [float(v) for v in plane_g]
        gf.range_max = float(gf_cfg.RANGE_MAX)
        gf.class_mask = self._ground_fill_class_mask()
        for v0 in range(0, V, _lib.AVL_MAX_VIEWS):       # a cell takes its views in order whether one call holds them all or not
            cams = cameras[v0:v0 + _lib.AVL_MAX_VIEWS]
            n = len(cams)
            P = _dbl(np.stack([np.asarray(c.P, dtype=np.float64) for c in cams]))
            gf.filled = self.last_filled.data_ptr() + 4 * v0
            if src_kind == "logits":
                pl, ih, iw = self._point_logits(views[v0:v0 + n], image_size, net_size, (self.last_abstained, v0))
            occ = None
            if occlusion:
                o = self._occlusion(n, ih, iw, (self.last_culled, v0))
                pview, pT, _, _, _ = self._frame_args(pcd, grid_frame_id if pcd_frame_id is None else pcd_frame_id, pose, cams[0].P, grid=False)
                rc = _lib.lib().avl_occlusion_depth(*pview, n, P, pT, float(self.pcd_range_max), iw, ih, C.byref(o), s)
                _lib.check(rc, "avl_occlusion_depth")
                occ = C.byref(o)
            if src_kind == "logits":
                rc = _lib.lib().avl_ground_fill_views_logits(C.byref(gs), C.byref(gf), n, P, T, C.byref(pl), iw, ih, self._lut_host(net_palette),
                                                             cm, occ, s)
                _lib.check(rc, "avl_ground_fill_views_logits")
            else:
                src = (C.c_void_p * n)(*[t.data_ptr() for t in views[v0:v0 + n]])
                rc = _lib.lib().avl_ground_fill_views(C.byref(gs), C.byref(gf), n, P, T, kind, src, sw, sh, iw, ih, lut, self._colors_host(),
                                                      cm, occ, s)
                _lib.check(rc, "avl_ground_fill_views")
        self._map_host = None

    def _ground_fill_step(self, semantic_images, pose, cameras, pcd, pcd_frame_id):
        """mapping()'s / mapping_views()'s fill branch: with GROUND_FILL.ENABLED and a plane set, the fill from the frame's own colour
        images, pose, cameras and cloud, right after the LiDAR frame.  With OCCLUSION.ENABLED the depth pass runs again for the fill."""
        if self.ground_fill_enabled() and self.ground_plane is not None:
            self.ground_fill_device(semantic_images, pose, cameras, grid_frame_id=pcd_frame_id, src_kind="rgb", pcd=pcd,
                                    pcd_frame_id=pcd_frame_id)

    def _plane_in_grid_frame(self, plane, pose, grid_frame_id):
        """-> (the velodyne-frame ``plane`` (set_ground_plane's forms) in the frame of a grid whose clouds are in ``grid_frame_id``,
        float64 [4], not normalised; the 4 x 4 grid frame -> velodyne transform, None for a velodyne-frame grid).  Any frame but
        "velodyne" needs the pose."""
        from .ground_plane import plane_to_frame
        T_np = self._origin_to_velodyne(pose) if grid_frame_id != "velodyne" else None
        return plane_to_frame(plane, T_np), T_np

    # ------------------------------------------------------------------ height-aware mapping (MAPPING.HEIGHT_GATE, MAPPING.ELEVATION)
    def height_gate_enabled(self):
        return self.height_gate_cfg is not None and bool(self.height_gate_cfg.ENABLED)

    def elevation_enabled(self):
        return self.elevation_cfg is not None and bool(self.elevation_cfg.ENABLED)

    def _gate_on(self, _gate):
        return self.height_gate_enabled() if _gate is None else bool(_gate)

    def _height_routed(self, _gate):
        """whether a frame call takes avl_fused_frame_views_height: either option enabled (``_gate`` False: this call does not gate)"""
        return self._gate_on(_gate) or self.elevation_enabled()

    def _gate_if_plane(self):
        """what mapping() / mapping_views() add to their frame call: with the gate enabled and no plane set yet the frame is mapped
        ungated (``_gate=False``) and ``last_gated`` stays None, as the ground fill waits for its plane; otherwise nothing"""
        return {"_gate": False} if self.height_gate_enabled() and self.ground_plane is None else {}

    def _per_label(self, value, what):
        """a number for every class, or one per entry of LABELS_NAMES -> float64 [C]; ValueError for a wrong length, a NaN or a
        value that is no number"""
        n = len(self.label_names)
        vals = [value] * n if not isinstance(value, (list, tuple, np.ndarray)) else list(value)
        if len(vals) != n:
            raise ValueError("%s has %d entries, LABELS_NAMES has %d: %r" % (what, len(vals), n, list(self.label_names)))
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
                raise ValueError("%s = %r (numbers, inf for no bound, never a NaN)" % (what, value))
        return np.array(vals, dtype=np.float64)

    def _parse_height_gate(self):
        hc = self.height_gate_cfg
        lo, hi = self._per_label(hc.MIN_M, "MAPPING.HEIGHT_GATE.MIN_M"), self._per_label(hc.MAX_M, "MAPPING.HEIGHT_GATE.MAX_M")
        if (lo > hi).any():
            raise ValueError("MAPPING.HEIGHT_GATE: MIN_M %r exceeds MAX_M %r" % (lo.tolist(), hi.tolist()))
        slope = hc.SLOPE
        if isinstance(slope, bool) or not isinstance(slope, (int, float, np.integer, np.floating)) or not 0.0 <= float(slope) < np.inf:
            raise ValueError("MAPPING.HEIGHT_GATE.SLOPE = %r (a finite number >= 0)" % (slope,))
        return lo, hi, float(slope)

    def _parse_elevation(self):
        ec = self.elevation_cfg
        names = list(ec.CLASSES)
        unknown = [n for n in names if n not in self.label_names]
        if unknown:
            raise ValueError("MAPPING.ELEVATION.CLASSES names %r, LABELS_NAMES has %r" % (unknown, list(self.label_names)))
        q = ec.QUANTUM_M
        if isinstance(q, bool) or not isinstance(q, (int, float, np.integer, np.floating)) or not 0.0 < float(q) < np.inf:
            raise ValueError("MAPPING.ELEVATION.QUANTUM_M = %r (a finite number > 0)" % (q,))
        return sum(1 << i for i, name in enumerate(self.label_names) if name in names), float(q)

    def height_plane(self, pose, grid_frame_id, plane=None):
        """The plane the height gate hands the kernel, float64 [4]: ``plane`` (set_ground_plane's forms, velodyne frame; None = the
        plane last set) taken to the frame of a grid whose clouds are in ``grid_frame_id`` as ground_fill_device takes it, then
        normalised in float64: n = sqrt((a * a + b * b) + c * c), each of the four divided by n, all four negated when c < 0.
        RuntimeError without a plane; ValueError for one that is not finite or has c = 0 in the grid's frame."""
        plane = self.ground_plane if plane is None else plane
        if plane is None:
            raise RuntimeError("the height gate needs a ground plane: none was given and set_ground_plane has not been called")
        p = self._plane_in_grid_frame(plane, pose, grid_frame_id)[0]
        if not np.isfinite(p).all() or p[2] == 0.0:
            raise ValueError("ground plane %r in the grid's frame is not finite or is vertical" % (p.tolist(),))
        p = p / np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
        return -p if p[2] < 0.0 else p

    def elevation_layer(self):
        """The elevation layer, four CUDA tensors [Hm, Wm]: (sum int64, cnt int32, min int32, max int32) of q = rint(z / QUANTUM_M)
        over the points that voted one of MAPPING.ELEVATION.CLASSES (rule 5 at struct avl_height); an empty cell holds (0, 0,
        INT32_MAX, INT32_MIN).  Allocated, empty, on first use; the frames write into these very tensors."""
        if self._elevation is None:
            shape = (self.map_height, self.map_width)
            self._elevation = (torch.empty(shape, dtype=torch.int64, device=self.device),) + tuple(
                torch.empty(shape, dtype=torch.int32, device=self.device) for _ in range(3))
            self.reset_elevation()
        return self._elevation

    def reset_elevation(self, stream=None):
        """Every cell of the layer back to empty (avl_elevation_reset)."""
        if self._elevation is None:
            self.elevation_layer()             # allocates and comes back here
            return
        s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)
        rc = _lib.lib().avl_elevation_reset(*[_ptr(t) for t in self._elevation], self.map_height * self.map_width, s)
        _lib.check(rc, "avl_elevation_reset")

    def elevation_device(self, stream=None):
        """The mean elevation per cell in metres, float32 CUDA [Hm, Wm]: (float)((sum / cnt) * QUANTUM_M) in float64, NaN for a cell
        without a point (avl_elevation_mean)."""
        q = (self._elevation_par or self._parse_elevation())[1]
        esum, ecnt = self.elevation_layer()[:2]
        out = torch.empty((self.map_height, self.map_width), dtype=torch.float32, device=self.device)
        s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)
        rc = _lib.lib().avl_elevation_mean(_ptr(esum), _ptr(ecnt), self.map_height * self.map_width, q, _ptr(out), s)
        _lib.check(rc, "avl_elevation_mean")
        return out

    def _height(self, V, pose, grid_frame_id, _gate=None, gated=None):
        """struct avl_height for a frame call of V views on a cloud in ``grid_frame_id``: the gate's fields with the gate on for this
        call, the layer's with MAPPING.ELEVATION.ENABLED.  ``gated``: (int32 CUDA tensor, first element) that receives the V counts;
        None = a fresh-or-reused ``self.last_gated`` of V elements."""
        ht = _lib.AvlHeight()
        if self._gate_on(_gate):
            lo, hi, slope = self._height_bounds or self._parse_height_gate()
            ht.gate = 1
            ht.plane[:] = [float(v) for v in self.height_plane(pose, grid_frame_id)]
            ht.min_m[:len(lo)] = lo.tolist()
            ht.max_m[:len(hi)] = hi.tolist()
            ht.slope = slope
            if gated is None:
                if self.last_gated is None or int(self.last_gated.numel()) != V:
                    self.last_gated = torch.zeros(V, dtype=torch.int32, device=self.device)
                gated = (self.last_gated, 0)
            ht.gated = gated[0].data_ptr() + 4 * int(gated[1])
        if self.elevation_enabled():
            ht.elev_classes, ht.quantum = self._elevation_par or self._parse_elevation()
            ht.elev_sum, ht.elev_cnt, ht.elev_min, ht.elev_max = (t.data_ptr() for t in self.elevation_layer())
        return ht

    def point_heights_device(self, pcd, pcd_frame_id, pose, plane=None):
        """Rules 1 and 2 of struct avl_height alone (avl_point_heights, MAPPING.HEIGHT_GATE.SLOPE whether ENABLED or not): for every
        point of ``pcd``, candidate or not, its height h above ``plane`` (velodyne frame, None = the plane last set; taken to the
        cloud's frame by height_plane) and its slack s = SLOPE x forward distance.  Returns two float64 CUDA tensors [N], both NaN
        for a point with a non-finite coordinate."""
        slope = (self._height_bounds or self._parse_height_gate())[2]
        ht = _lib.AvlHeight()
        ht.plane[:] = [float(v) for v in self.height_plane(pose, pcd_frame_id, plane)]
        ht.slope = slope
        view, T, _, _, s = self._frame_args(pcd, pcd_frame_id, pose, np.zeros(12), grid=False)
        n = view[1]
        h = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)[:n]
        sl = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)[:n]
        rc = _lib.lib().avl_point_heights(*view, T, C.byref(ht), _ptr(h), _ptr(sl), s)
        _lib.check(rc, "avl_point_heights")
        return h, sl

    def project_pcd(self, pcd, pcd_frame_id, image, pose, camera_calibration):
        """mapping.py:357-389.  NumPy in, NumPy out: (pcd[:, mask] float64[4,M], label uint8[3,M]).
        Pass ``as_device=True`` through project_pcd_device for CUDA tensors instead."""
        if pcd is None:
            return
        out_pcd, out_label, m = self.project_pcd_device(pcd, pcd_frame_id, image, pose, camera_calibration)
        m = int(m.item())
        return out_pcd[:, :m].cpu().numpy(), out_label[:, :m].cpu().numpy()

    def project_pcd_device(self, pcd, pcd_frame_id, image, pose, camera_calibration):
        """avl_project_pcd: returns CUDA tensors (out_pcd f64[4,N], out_label u8[3,N], count int32[1]);
        only the first `count` columns are meaningful."""
        view, T, _, P, s = self._frame_args(pcd, pcd_frame_id, pose, camera_calibration.P, grid=False)
        img = self._as_device_u8(image)
        assert img.dim() == 3 and img.shape[2] == 3
        n = view[1]
        ld = max(n, 1)
        out_pcd = torch.empty((4, ld), dtype=torch.float64, device=self.device)
        out_label = torch.empty((3, ld), dtype=torch.uint8, device=self.device)
        count = torch.zeros(4, dtype=torch.int32, device=self.device)
        need = int(_lib.lib().avl_project_pcd_scratch_bytes(n))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=self.device)
        rc = _lib.lib().avl_project_pcd(*view, P, T, float(self.pcd_range_max), _ptr(img), int(img.shape[1]), int(img.shape[0]),
                                        _ptr(out_pcd), _ptr(out_label), ld, _ptr(count), _ptr(self._scratch), s)
        _lib.check(rc, "avl_project_pcd")
        return out_pcd, out_label, count[:1]

    def semantic_cloud_device(self, pcd, pcd_frame_id, image, pose, camera_calibration):
        """The semantic point cloud mapping() publishes (mapping.py:314-317): project_pcd followed by
        create_point_cloud (utils_ros.py:31-59), both on the GPU.  Returns (records uint8[M,16] CUDA tensor in
        PointCloud2 layout x,y,z float32 + rgba uint32, M)."""
        out_pcd, out_label, count = self.project_pcd_device(pcd, pcd_frame_id, image, pose, camera_calibration)
        n = int(out_pcd.shape[1])
        rec = torch.empty((max(n, 1), 16), dtype=torch.uint8, device=self.device)
        s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.lib().avl_pack_semantic_cloud(_ptr(out_pcd), _ptr(out_label), n, n, _ptr(count), _ptr(rec), s),
                   "avl_pack_semantic_cloud")
        m = int(count.item())
        return rec[:m], m

    def update_map(self, map, pcd, label):
        """mapping.py:391-444.  ``map`` may be
          * a CUDA tensor [Hm,Wm,C] (float64/float32): updated in place on the GPU and returned;
          * a NumPy array (the reference's type): the vote kernel finds the touched cells, their rows
            are moved to the GPU, updated there by the same apply kernel, and written back -- the host
            only moves bytes, it does no arithmetic.  The array is mutated in place and returned."""
        m = int(pcd.shape[1])
        if m == 0:
            return map
        pcd_d = self._as_device(pcd, torch.float64)
        label_d = self._as_device_u8(label)
        assert pcd_d.shape[0] == 4 and label_d.shape[0] == 3 and label_d.shape[1] == m
        pcd_d, label_d = pcd_d.contiguous(), label_d.contiguous()
        g = self.grid
        assert tuple(map.shape) == (g.Hm, g.Wm, g.C), "map shape %s != grid %s" % (tuple(map.shape), (g.Hm, g.Wm, g.C))
        g.ensure_capacity(m)
        s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        colors, cm, bonus = self._colors_host(), _dbl(self.confusion_matrix), self._bonus_classes()
        L = _lib.lib()
        if isinstance(map, torch.Tensor):
            assert map.is_cuda and map.is_contiguous()
            gs = g.struct(map)
            _lib.check(L.avl_update_map(C.byref(gs), _ptr(pcd_d), _ptr(label_d), m, m, None, colors, cm, bonus, s),
                       "avl_update_map")
            if map.data_ptr() == g.map.data_ptr():
                self._map_host = None
            return map
        # NumPy grid: vote on the GPU, move only the touched rows
        gs = g.struct()
        _lib.check(L.avl_vote_points(C.byref(gs), _ptr(pcd_d), _ptr(label_d), m, m, None, colors, bonus, s), "avl_vote_points")
        u = int(g.counter[0].item())
        if u == 0:
            return map
        cells = g.touched[:u].cpu().numpy().astype(np.int64)
        cx, cy = cells // g.Wm, cells % g.Wm
        np_dtype = np.float64 if map.dtype != np.float32 else np.float32
        rows = torch.from_numpy(np.ascontiguousarray(map[cx, cy, :], dtype=np_dtype)).to(self.device)
        row_dtype = _lib.AVL_F64 if np_dtype == np.float64 else _lib.AVL_F32
        _lib.check(L.avl_grid_apply(C.byref(gs), cm, _ptr(rows), row_dtype, s), "avl_grid_apply")
        map[cx, cy, :] = rows.cpu().numpy()
        return map

    def update_map_planar(self, map_local, image, cam, T_local_to_base=None):
        """mapping.py:446-488: project the semantic image onto the map plane through a 4-point homography and update the grid
        (avl_planar_update: warp + class test + clamp in one pass over the grid).  ``map_local``: CUDA tensor [Hm,Wm,C] (updated
        in place) or NumPy array (uploaded, updated, written back); ``image``: uint8 [H,W,3].  The reference looks the
        /local_map -> /base_link transform up in a live ROS TF tree (:454-457); here it is ``T_local_to_base`` (4x4) or, when
        None, ``self.local_to_base_lookup(self.pose_time)``.  ``MAPPING.PLANAR_MATCH`` picks the class test (see config.py):
        with "reference" the warp cannot influence the result and is skipped."""
        match = 1 if self.planar_match == "colour" else 0
        is_np = not isinstance(map_local, torch.Tensor)
        grid_t = torch.from_numpy(np.ascontiguousarray(map_local)).to(self.device) if is_np else map_local
        assert grid_t.is_cuda and grid_t.is_contiguous() and tuple(grid_t.shape) == (self.map_height, self.map_width, self.map_depth)
        img = self._as_device_u8(image)
        hinv = None
        if match:
            if T_local_to_base is None:
                if getattr(self, "local_to_base_lookup", None) is None:
                    raise RuntimeError("update_map_planar needs T_local_to_base (the reference reads it from ROS TF): pass it or set "
                                       "SemanticMapping.local_to_base_lookup")
                T_local_to_base = self.local_to_base_lookup(self.pose_time)
            pts_img = planar_points_image(self.anchor_points_2, self.discretize_matrix_inv, np.asarray(T_local_to_base, dtype=np.float64),
                                          self.T_velodyne_to_basklink, cam.P)
            hinv = _dbl(np.linalg.inv(find_homography(pts_img.T, self.anchor_points_2.T)))
        # :468-470 `mask[:, 0:sep] = 0` with Python's slice rules: a negative sep (map_boundary[0][0] > 8, as in the reference's
        # own base_cfg) masks columns [0, Wm + sep), a sep beyond the width masks every column
        sep = int((8 - self.map_boundary[0][0]) / self.resolution)
        sep = len(range(*slice(0, sep).indices(self.map_width)))
        dt = _lib.AVL_F64 if grid_t.dtype == torch.float64 else _lib.AVL_F32
        s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = _lib.lib().avl_planar_update(_ptr(grid_t), dt, self.map_height, self.map_width, self.map_depth, _ptr(img), int(img.shape[0]),
                                          int(img.shape[1]), hinv, sep, self._colors_host(), match, s)
        _lib.check(rc, "avl_planar_update")
        if is_np:
            map_local[...] = grid_t.cpu().numpy()
            return map_local
        if self._grid is not None and grid_t.data_ptr() == self._grid.map.data_ptr():
            self._map_host = None
        return map_local

    # ------------------------------------------------------------------ the scrolling grid (MAPPING.SCROLL)
    def scroll_enabled(self):
        return self.scroll_cfg is not None and bool(self.scroll_cfg.ENABLED)

    def _scroll_store(self):
        if self._scroll is None:
            raise RuntimeError("MAPPING.SCROLL.ENABLED is False: this map is the fixed rectangle of MAPPING.BOUNDARY")
        return self._scroll

    def scroll_to(self, pose, stream=None):
        """Move the window so that the vehicle at ``pose`` is near its centre (scroll.next_origin: whole tiles, a hysteresis band);
        True when it moved.  While the origin stays this is host arithmetic: nothing is launched, copied or waited for, and
        ``last_scroll`` is untouched.  A move is one avl_tile_copy launch per layer (the map; with MAPPING.ELEVATION its four arrays)
        on ``stream``: leaving tiles go to the store, the overlap moves to the second window buffer, entering tiles come from the
        store or start empty; then the buffers swap -- ``map_dev`` is another tensor afterwards -- and ``grid.boundary`` /
        ``map_boundary`` become scroll.window_boundary(new origin), which is what every consumer of the boundary reads.
        mapping() and mapping_views() call this before the frame's vote; frame_device*, ground_fill_device and the other
        device-level entry points do not: their callers do.  All scrolls, frames and site calls of one map belong on one stream (or
        the caller orders them): a slab freed by one call is reused by the next."""
        with self._lock:
            return self._scroll_store().scroll_to(pose, stream)

    def site_tiles(self, layer="map"):
        """The sorted tile coordinates (ti, tj) that hold something, in the window or in the store; ``layer`` "map" or "elevation".
        Waits for the last scroll's emptiness flags."""
        with self._lock:
            return self._scroll_store().site_tiles(layer)

    def site_map(self, rect=None, layer="map", stream=None):
        """-> ((i0, j0), CUDA tensor): the tile rectangle ``rect`` = (ti0, ti1, tj0, tj1), both ends included, assembled from window
        tiles, stored tiles and the empty state by the tile-job kernel; (i0, j0) is the global cell of its first element.  ``rect``
        None = the bounding rectangle of site_tiles(layer).  ``layer`` "elevation" returns the layer's four arrays.  The window and
        the store are left as they are.  render_bev_map(site_map()[1]) is the picture of the whole site."""
        with self._lock:
            return self._scroll_store().site_map(rect, layer, stream)

    def site_overview(self, cells_per_pixel=None, rect=None, thresholds=None, priority=None, reduced=False, out=None, stream=None):
        """-> ((i0, j0), picture) or, with ``reduced``, ((i0, j0), picture, R): the tile rectangle ``rect`` (as site_map's; None = the
        bounding rectangle of site_tiles("map")) at ``cells_per_pixel`` = k cells per pixel, by one kernel that reads the tiles where
        they live (avl_site_overview; the rule: include/avl_hip.h).  R [h, w, C] is the k x k sum of every class in the map's type and
        a fixed order, picture uint8 [h, w, 3] is render_bev_map's rule on R -- with ``thresholds`` render_bev_map_with_thresholds'
        with ``priority`` -- and black where nothing was mapped; h = tile rows * T / k.  k must divide the tile size; None =
        MAPPING.SITE_OVERVIEW.CELLS_PER_PIXEL, where 0 chooses the smallest k whose picture has no side above MAX_SIDE_PX.
        ``thresholds`` None = MAPPING.SITE_OVERVIEW.THRESHOLDS ([] = arg-max).  ``out``: a contiguous uint8 CUDA tensor of the
        picture's shape.  An empty site gives a 0 x 0 x 3 picture and launches nothing.  Nothing of the site is assembled: cost and
        memory follow the mapped tiles and the output.  Same stream contract as site_map; the window and the store are only read."""
        oc = self.cfg.MAPPING.SITE_OVERVIEW
        if cells_per_pixel is None:
            cells_per_pixel = int(oc.CELLS_PER_PIXEL)
        if thresholds is None:
            thresholds = list(oc.THRESHOLDS)
        with self._lock:
            return self._scroll_store().site_overview(cells_per_pixel, rect, self.label_colors, thresholds, priority, reduced, out, stream,
                                                      int(oc.MAX_SIDE_PX))

    def site_finish(self, rect=None, filter=True, thresholds=None, priority=None, truth=None, picture=True, labels=False, out=None,
                    stream=None):
        """-> scroll.SiteFinish(origin, picture, labels, counts, tiles): the run's end result for the whole site -- finish_run's chain
        apply_filter -> render_bev_map -> convert_labels -> Test.iou's counting -- on the tile rectangle ``rect`` (as site_map's; None =
        the bounding rectangle of site_tiles("map")), by one kernel that reads the tiles where they live (avl_site_finish; the rule:
        include/avl_hip.h).  ``picture`` uint8 [H, W, 3] is render_bev_map(apply_filter(site_map(rect)[1])) byte for byte -- with
        ``thresholds`` (None = MAPPING.SITE_FINISH.THRESHOLDS, [] = arg-max) render_bev_map_with_thresholds' with ``priority`` --
        ``filter`` False leaves the smoothing out; ``labels`` uint8 [H, W] is convert_labels of it (0 where ``truth``'s mask is 0);
        ``counts`` (with ``truth``, an evaluation.SiteTruth) is the int64 [8, 8] histogram J[truth][label] over the whole rectangle,
        what evaluation._run gives on the assembled route, for evaluation.Test.test_site.  ``origin`` is the global cell of the first
        element, ``tiles`` = (records with a source, empty records computed around them).  With picture=False and labels=False nothing
        of the rectangle's size is allocated: the way to score a site whose rectangle no buffer could hold.  An empty site gives
        empty tensors, launches nothing, and counts all of the truth as missed.  ``out``: a contiguous uint8 CUDA tensor of the
        picture's shape.  Same stream contract as site_map; unlike finish_run's filter, the window and the store are only read."""
        if thresholds is None:
            thresholds = list(self.cfg.MAPPING.SITE_FINISH.THRESHOLDS)
        with self._lock:
            return self._scroll_store().site_finish(rect, self.label_colors, filter, thresholds, priority, truth, picture, labels, out, stream)

    def save_site(self, path, stream=None):
        """The whole site -- the window's own tiles included -- as one .npz: anchor, resolution, T, C, dtype and, per layer, the
        coordinates and a [n, T, T, ...] array of its non-empty tiles (scroll.pack_site)."""
        with self._lock:
            return self._scroll_store().save_site(path, stream)

    def load_site(self, path, stream=None):
        """A site file into the store: every tile goes to a slab, the window is left empty at origin (0, 0) and the next scroll_to
        brings in what belongs there.  What the map held before is dropped.  ValueError when the file's anchor, resolution, T, C,
        dtype or layers are not this map's."""
        with self._lock:
            return self._scroll_store().load_site(path, stream)

    def merge_site(self, path_or_arrays, stream=None):
        """Another run's or another vehicle's site -- a save_site file, or the dict scroll.pack_site makes -- SUMMED into this map:
        a frame's contribution never reads the grid, so the sum of two sites is the site of all their frames.  Per cell the result
        is own (+) theirs by the rule of avl_tile_merge (include/avl_hip.h): one IEEE add for the map; with MAPPING.ELEVATION
        its sum and count add (the int32 count WRAPS past 2^31 - 1), its minimum and maximum take the minimum and maximum.  Merging
        is a left fold: merge_site(B); merge_site(C) gives (own + B) + C.  A tile of the file inside the current window is summed
        into the live window buffer in place, a stored one into its slab, a tile this map does not have gets a new slab; nothing is
        assembled, cost and memory follow the file's tiles.  A tile of this map that the file lacks is left as it is; where both
        have the tile, the file's +0 cells turn a -0.0 of this map into +0.0.  A stored tile whose result is empty in every layer
        gives its slab back.  One avl_tile_merge launch per layer on ``stream``; the call waits for the result flags.  -> scroll.SiteMerge
        (tiles summed in the window, summed in the store, added, freed).  ValueError, naming the numbers, before any device work
        and with the map untouched: the file's anchor, resolution, T, C, dtype or layers are not this map's -- sites of another
        anchor or resolution would need resampling and are out of scope, as for load_site -- a tile named twice in a layer, a
        tile at or beyond 2^30 cells.  Same stream contract as site_map."""
        with self._lock:
            return self._scroll_store().merge_site(path_or_arrays, stream)

    def global_site(self, group=None, exchange_dtype=None, stream=None):
        """The end-of-run collective of a scrolled multi-GPU run: every rank's site becomes the sum of all ranks' sites.  Each rank
        packs its non-empty tiles on the device (save_site's gather without the host copy), the ranks all-gather coordinates and
        tiles layer by layer (distributed.gather_sites), and every rank rebuilds its site as ((empty + S_0) + S_1) + ... in rank
        order with merge_site's kernel -- the store is reset as load_site resets it, the window is left empty at origin (0, 0) -- so
        all ranks hold the bit-identical sum.  ``exchange_dtype=torch.float32`` on a float64 map: the packed copy of the map layer is
        cast first and summed as acc + (double)tile, half the payload; identity-matrix sites stay exact, log-matrix sites take each
        rank's float32 rounding.  With world size 1 only the own site is folded: empty + S_0, which is S_0 but for a -0.0 (it becomes
        +0.0) and, with a float32 exchange, its rounding.  ``last_exchange`` = ("tiles", bytes this rank sent).  -> [scroll.SiteMerge],
        one per rank.  A SECOND call on the same map raises RuntimeError: the site already holds the other ranks' frames and would
        count them again (load_site starts over).  global_map() keeps refusing a scrolled map: there is no common window to return."""
        with self._lock:
            return self._scroll_store().global_site(group, exchange_dtype, stream)

    # ------------------------------------------------------------------ multi-GPU: shared global grid
    def global_map(self, group=None, dst=None, exchange_dtype=None, mode="dense"):
        """Sum of every rank's private grid: each rank maps its own camera stream into its
        own grid; since a frame's contribution never depends on the grid's content, the shared grid
        is the element-wise sum.  mode "dense": all_reduce (or reduce to ``dst``) over RCCL on a copy, so the private
        grid keeps accumulating; ``exchange_dtype=torch.float32`` halves the payload (see distributed.reduce_grids).
        mode "sparse": an all-gather of every rank's (cell int32, delta float32 [C]) records instead (distributed.reduce_grids_sparse:
        ~0.6 MB per GPU at config C against 80 MB); "auto": sparse while every rank touched fewer than 5 % of the cells.
        Returns the CUDA tensor (valid on every rank, or on dst only); ``.last_exchange`` = (mode used, bytes this rank sent)."""
        from . import distributed as D
        if self._scroll is not None:
            raise RuntimeError("global_map() with MAPPING.SCROLL.ENABLED: every rank's window has its own origin, and a multi-GPU site "
                               "map is out of scope; exchange site_map() regions instead")
        if mode == "dense":
            total = D.reduce_grids(self.grid.map, group=group, dst=dst, exchange_dtype=exchange_dtype)
            self.last_exchange = ("dense", int(total.numel() * total.element_size()))
            return total
        assert dst is None, "the record exchange is an all-gather: every rank gets the sum"
        vdt = torch.float32 if exchange_dtype is None else exchange_dtype
        if mode == "sparse":
            total, sent = D.reduce_grids_sparse(self.grid.map, group=group, value_dtype=vdt)
            self.last_exchange = ("sparse", sent)
            return total
        if mode != "auto":
            raise ValueError("global_map mode must be 'dense', 'sparse' or 'auto', not %r" % mode)
        total, used, sent = D.reduce_grids_auto(self.grid.map, group=group, exchange_dtype=vdt)
        self.last_exchange = (used, sent)
        return total

    def save_inputs(self, path=None):
        """The reference dumps input_list with hickle (mapping.py:324-326); hickle is optional here,
        so frames go to one .npz each with the same field names (pose as 7 numbers)."""
        path = path or self.input_dir
        os.makedirs(path, exist_ok=True)
        for k, fr in enumerate(self.input_list):
            pose = fr["pose"]
            pose7 = pose.to_array() if hasattr(pose, "to_array") else _pose_to_array(pose)
            np.savez_compressed(osp.join(path, "frame_%06d.npz" % k), pcd=fr["pcd"], pcd_frame_id=np.array(fr["pcd_frame_id"]),
                                semantic_image=fr["semantic_image"], pose=pose7)

    def get_extrinsics(self, pose, camera_id):
        """mapping.py:528-540"""
        T_base_to_origin = get_transform_from_pose(pose)
        if camera_id == "camera1":
            T_cam_to_origin = np.matmul(T_base_to_origin, self.T_cam1_to_base)
        elif camera_id == "camera6":
            T_cam_to_origin = np.matmul(T_base_to_origin, self.T_cam6_to_base)
        else:
            raise ValueError("unable to find camera to base for camera_id %s" % camera_id)
        return np.linalg.inv(T_cam_to_origin)[0:3]

    # ------------------------------------------------------------------ helpers
    def _origin_to_velodyne(self, pose):
        """mapping.py:368-369 (host, float64 4x4)."""
        return origin_to_velodyne(pose, self.T_velodyne_to_basklink)

    def estimate_ground_plane(self, pose=None, **kw):
        """The ground plane of the current cloud (``self.pcd`` in ``self.pcd_frame_id``) in the velodyne frame, estimated on the GPU:
        ground_plane.estimate_ground_plane_device with its keyword arguments.  A cloud that is not in the velodyne frame needs the
        pose (the transform of project_pcd, mapping.py:368-373).  Returns the GroundPlaneResult (asynchronous until ``.host()``).
        With MAPPING.POINTS_MAP.SOURCE = "index" the cloud is ``reduced_map_device(pose)``, the crop of the vehicle's cameras around
        ``pose``, a "world" cloud: the pose is needed."""
        from .ground_plane import estimate_ground_plane_device
        with self._lock:
            if self.points_map_indexed():
                if pose is None:
                    raise ValueError("a cloud in frame 'world' needs the pose to reach the velodyne frame")
                cloud = self.reduced_map_device(pose, stream=_raw_stream(kw.get("stream")))
                return estimate_ground_plane_device(cloud, T=self._origin_to_velodyne(pose), device=self.device, **kw)
            if self.pcd is None:
                raise RuntimeError("estimate_ground_plane needs a point cloud: no pcd yet")
            T = None
            if self.pcd_frame_id != "velodyne":
                if pose is None:
                    raise ValueError("a cloud in frame %r needs the pose to reach the velodyne frame" % (self.pcd_frame_id,))
                T = self._origin_to_velodyne(pose)
            return estimate_ground_plane_device(self.pcd, T=T, device=self.device, **kw)

    def _colors_host(self):
        c = np.ascontiguousarray(self.label_colors, dtype=np.uint8).ravel()
        key = c.tobytes()
        if getattr(self, "_colors_key", None) != key:
            self._colors_key, self._colors_c = key, (C.c_uint8 * c.size).from_buffer_copy(key)
        return self._colors_c

    def _lut_host(self, net_palette):
        key = (np.asarray(net_palette, dtype=np.uint8).tobytes(), np.ascontiguousarray(self.label_colors, dtype=np.uint8).tobytes())
        if getattr(self, "_lut_key", None) != key:
            lut_np = vote_lut(net_palette, self.label_colors)
            self._lut_key, self._lut_c = key, (C.c_uint32 * 256).from_buffer_copy(lut_np.astype(np.uint32).tobytes())
        return self._lut_c

    def _bonus_classes(self):
        """bit i set when class i is a "lane" class and USE_INTENSITY is on (mapping.py:427-431)."""
        if not self.use_pcd_intensity:
            return 0
        return sum(1 << i for i, name in enumerate(self.label_names) if name == "lane")

    def _as_device(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(self.device, dtype=dtype)
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device, dtype=dtype)

    def _as_device_u8(self, a):
        if isinstance(a, torch.Tensor):
            assert a.dtype == torch.uint8
            return a.to(self.device).contiguous()
        a = np.ascontiguousarray(a)
        assert a.dtype == np.uint8, "semantic images / labels must be uint8"
        return torch.from_numpy(a).to(self.device)

    def _semantic_source(self, shape, src_kind, image_size, net_palette):
        """-> (sh, sw, ih, iw, kind, lut) of a semantic source of ``shape``: a colour image [H,W,3] is its own image; a class map
        [h,w] stands for the image of ``image_size`` (its own size if None) and votes through the palette's LUT."""
        if src_kind == "rgb":
            assert len(shape) == 3 and shape[2] == 3
            sh, sw = int(shape[0]), int(shape[1])
            return sh, sw, sh, sw, _lib.AVL_SRC_RGB, None
        assert len(shape) == 2
        sh, sw = int(shape[0]), int(shape[1])
        ih, iw = (sh, sw) if image_size is None else (int(image_size[0]), int(image_size[1]))
        return sh, sw, ih, iw, _lib.AVL_SRC_CLASSMAP, self._lut_host(net_palette)

    def _frame_args(self, pcd, pcd_frame_id, pose, P, stream=None, grid=True):
        """What every frame call hands the library alike -> (points view, T or None, grid struct grown to the cloud or None,
        P, stream), each in its ctypes form."""
        view = self._points_view(pcd)
        T = _dbl(self._origin_to_velodyne(pose)) if pcd_frame_id != "velodyne" else None
        gs = None
        if grid:
            self.grid.ensure_capacity(view[1])
            gs = self.grid.struct()
        s = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        return view, T, gs, _dbl(P), C.c_void_p(s)

    def _points_view(self, pcd):
        """-> (ctypes ptr, n, avl dtype, point_stride, comp_stride) and keeps the tensor alive."""
        t, n, dtype, point_stride, comp_stride = _lib.points_view(pcd, self.device)
        self._pcd_dev = t
        return _ptr(t), n, dtype, point_stride, comp_stride


def velodyne_to_baselink():
    """mapping.py:165-170 (host, float64 4x4)."""
    T = euler_matrix(0., 0.140, 0.)
    t = np.array([[2.64, 0, 1.98]]).T
    T[0:3, -1::] = t
    return T


def origin_to_velodyne(pose, T_velodyne_to_baselink):
    """mapping.py:368-369 (host, float64 4x4)."""
    T_base_to_origin = get_transform_from_pose(pose)
    return np.linalg.inv(np.matmul(T_base_to_origin, T_velodyne_to_baselink))


def pose_heading(pose):
    """(cos yaw, sin yaw) of the vehicle's x axis in the map's x, y plane, from the pose quaternion (host float64): the first column
    of its rotation matrix, projected on the plane and normalised; (1, 0) for a vertical one."""
    q = _pose_to_array(pose)[3:7]
    R = quaternion_matrix(q)
    c, s = float(R[0, 0]), float(R[1, 0])
    n = float(np.hypot(c, s))
    return (c / n, s / n) if n > 0.0 else (1.0, 0.0)


def _to_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _write_picture(png_path, picture):
    """``picture`` (uint8 [h, w, 3] NumPy) as the file cv2.imwrite would write (mapping.py:340): channel 0 of the array is stored as
    BLUE.  Without PIL the array goes to a .npy file of the same name.  Returns the path written."""
    try:
        from PIL import Image
    except ImportError:
        npy_path = png_path[:-4] + ".npy"
        np.save(npy_path, picture)
        return npy_path
    Image.fromarray(np.ascontiguousarray(picture[:, :, ::-1])).save(png_path)
    return png_path


def _pose_to_array(pose):
    if not hasattr(pose, "position"):
        return np.asarray(pose, dtype=np.float64)[:7]
    p, o = pose.position, pose.orientation
    return np.array([p.x, p.y, p.z, o.x, o.y, o.z, o.w], dtype=np.float64)


def _imgmsg_to_array(msg):
    """sensor_msgs/Image (rgb8/bgr8/8UC3 or mono8) -> ndarray, without cv_bridge."""
    ch = 3 if msg.encoding in ("rgb8", "bgr8", "8UC3") else 1
    a = np.frombuffer(msg.data, dtype=np.uint8).reshape(msg.height, msg.step)[:, :msg.width * ch]
    return a.reshape(msg.height, msg.width, ch) if ch == 3 else a.reshape(msg.height, msg.width)


def find_homography(pts_src, pts_dst):
    """cv2.findHomography(pts_src, pts_dst) for the four anchor correspondences of the planar mode (homography.py:37): the exact
    projective map by the normalised DLT, h33 = 1.  Host float64 (a 8 x 9 SVD)."""
    src, dst = np.asarray(pts_src, dtype=np.float64), np.asarray(pts_dst, dtype=np.float64)

    def normalise(p):
        c = p.mean(axis=0)
        s = np.sqrt(2.0) / max(np.sqrt(((p - c) ** 2).sum(axis=1)).mean(), 1e-300)
        return (p - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    a, Ta = normalise(src)
    b, Tb = normalise(dst)
    A = []
    for (x, y), (u, v) in zip(a, b):
        A.append([-x, -y, -1, 0, 0, 0, u * x, u * y, u])
        A.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
    Hn = np.linalg.svd(np.array(A))[2][-1].reshape(3, 3)
    H = np.linalg.inv(Tb) @ Hn @ Ta
    return H / H[2, 2]


def planar_points_image(anchor, discretize_matrix_inv, T_local_to_base, T_velodyne_to_baselink, P):
    """mapping.py:449-463: anchor cells -> local metres (z = 0) -> velodyne -> image pixels ([2][4]); host float64."""
    pm = np.vstack([anchor, np.ones((1, anchor.shape[1]))])
    pl = np.matmul(discretize_matrix_inv, pm)
    pl[2, :] = 0
    pl = np.vstack([pl, np.ones((1, pl.shape[1]))])
    pv = np.matmul(np.matmul(np.linalg.inv(T_velodyne_to_baselink), T_local_to_base), pl)
    pi = np.matmul(P, pv)
    return pi[0:2] / pi[2]


def _pointcloud2_payload(msg):
    """The points of a sensor_msgs/PointCloud2 as one uint8 array [width * height * point_step]: organised clouds
    (height > 1) may pad each row to row_step, which is dropped here; big-endian payloads are refused (the reference's
    read_points would byte-swap them; nothing on this path produces one)."""
    if getattr(msg, "is_bigendian", False):
        raise NotImplementedError("big-endian PointCloud2 payloads are not supported")
    width, height, step = int(msg.width), int(msg.height), int(msg.point_step)
    row_step = int(getattr(msg, "row_step", 0) or width * step)
    if row_step < width * step:
        raise ValueError("PointCloud2 row_step %d < width * point_step %d" % (row_step, width * step))
    if height <= 1 or row_step == width * step:
        return np.frombuffer(msg.data, dtype=np.uint8, count=width * height * step)
    rows = np.frombuffer(msg.data, dtype=np.uint8, count=height * row_step).reshape(height, row_step)
    return np.ascontiguousarray(rows[:, :width * step]).reshape(-1)


def unpack_pointcloud2(msg):
    """sensor_msgs/PointCloud2 -> float64[4,N] (x,y,z,intensity), NaN points dropped
    (what mapping.py:178-180 does with a per-point loop; SURVEY Q8: the buffer is sized to the
    number of valid points instead of leaving garbage columns)."""
    offs = {f.name: f.offset for f in msg.fields}
    n = msg.width * msg.height
    raw = _pointcloud2_payload(msg).reshape(n, msg.point_step)
    cols = []
    for name in ("x", "y", "z", "intensity"):
        o = offs[name]
        cols.append(raw[:, o:o + 4].copy().view(np.float32).reshape(n))
    pts = np.stack(cols).astype(np.float64)
    keep = ~np.isnan(pts).any(axis=0)
    return np.ascontiguousarray(pts[:, keep])
