"""Configuration tree with the reference's key names.

Mirrors src/config/base_cfg.py:12-112 (which embeds the network tree of
src/network/deeplab_v3_plus/config/demo.py:5-44 and deeplab_v3_plus.py:1-34).  yacs is not
available offline, so ``CfgNode`` here is a small attribute-dict with the three yacs operations the
reference uses: ``clone()``, ``merge_from_file(yaml)`` and ``merge_from_list([k, v, ...])``.
Unknown keys in an override file raise ``KeyError`` (as yacs does).
"""
import copy

import yaml

from .labels import LABELS, LABELS_NAMES, LABEL_COLORS


class CfgNode(dict):
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def clone(self):
        return copy.deepcopy(self)

    def _merge(self, other, path=""):
        for k, v in other.items():
            if k not in self:
                raise KeyError("Non-existent config key: %s%s" % (path, k))
            if isinstance(self[k], CfgNode):
                if not isinstance(v, dict):
                    raise ValueError("config key %s%s expects a mapping" % (path, k))
                self[k]._merge(v, path + k + ".")
            else:
                self[k] = v

    def merge_from_file(self, filename):
        with open(filename) as f:
            data = yaml.safe_load(f) or {}
        self._merge(data)

    def merge_from_list(self, kv):
        assert len(kv) % 2 == 0
        for key, value in zip(kv[0::2], kv[1::2]):
            node = self
            parts = key.split(".")
            for p in parts[:-1]:
                node = node[p]
            if parts[-1] not in node:
                raise KeyError("Non-existent config key: %s" % key)
            node[parts[-1]] = value

    def __str__(self):
        return yaml.safe_dump(_plain(self), default_flow_style=False)


def _plain(node):
    if isinstance(node, dict):
        return {k: _plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_plain(v) for v in node]
    return node


def get_network_cfg_defaults():
    """demo.py:5-44 with the overrides of base_cfg.py:96-112."""
    C = CfgNode()
    C.OUTPUT_DIR = "@"
    C.OUTPUT_NAME = ""
    C.TRAIN_DATASET = "Mapillary"
    C.DATASET_CONFIG = ""          # reference default points at the authors' NAS; "" = built-in 19-class table
    C.DATASET = CfgNode()
    C.DATASET.NAME = "AVL"
    C.DATASET.IN_CHANNELS = 3
    C.DATASET.NUM_CLASSES = 19
    C.DATASET.ROOT_DIR = ""
    C.MODEL = CfgNode()
    C.MODEL.TYPE = "DeepLabv3+"
    C.MODEL.WEIGHT = ""            # reference default is a NAS path; "" = seeded random weights
    C.MODEL.SYNC_BN = False
    C.MODEL.BACKBONE = "resnext50_32x4d"
    C.MODEL.OUTPUT_STRIDE = 8
    C.MODEL.ASPP = CfgNode()
    C.MODEL.ASPP.OUT_CHANNELS = 256
    C.MODEL.ASPP.ATROUS_CHANNELS = [256, 256, 256, 256]
    C.MODEL.ASPP.ATROUS_KERNEL_SIZE = [1, 3, 3, 3]
    C.MODEL.ASPP.ATROUS_DILATION = [1, 6, 12, 18]   # ignored: deeplab_v3_plus.py:30-36 picks by OUTPUT_STRIDE
    C.MODEL.ASPP.DROPOUT = 0.5
    C.MODEL.DECODER = CfgNode()
    C.MODEL.DECODER.LOW_LEVEL_OUT_CHANNELS = 256
    C.MODEL.DECODER.REFINE_CHANNELS = [256, 256]
    C.MODEL.DECODER.REFINE_KERNEL_SIZE = [3, 3]
    # build-specific (not in the reference): activation precision of the HIP conv stack
    # "mixed" (default): f16 MFMA on split hi+lo operands + MX-FP4 correction passes, logits within 1e-3 of the reference's fp32
    # forward on every weights draw measured (tests/test_gpu_mixed.py::test_mixed_logits_across_weight_seeds);
    # "f16" | "bf16": one 16-bit rounding per tensor (fastest; 2e-3 / 2e-2); "f32": fp32-input MFMA (1e-6, slowest)
    C.MODEL.PRECISION = "mixed"
    C.MODEL.MIXED_GCONV_MX = True       # "mixed" only: FP4 corrections inside the grouped 3x3 too (conv1's output keeps an FP4 lo part): -10..-30 % logits error for
                                        # -5 % frames/s; False was the round-2 default, whose error passed 1e-3 on one weights draw in four (profiles/r02/seed_sweep.log)
    C.MODEL.MIXED_TRUNK_FP4 = True      # "mixed" only: keep the lo part of the residual trunk / 3x3 outputs as FP4 only (False: f16 lo planes, 12 % slower, -0..14 % error)
    C.MODEL.MIXED_CONV2_SPLIT = True    # "mixed" only: keep every bottleneck's 3x3 output as hi + lo (conv3 corrects for both parts)
    C.MODEL.MIXED_LAYER1_LO = True      # "mixed" only: every block of layer1 keeps a lo plane of its output (default since the end of round 5: with layer1's blocks
                                        # fused the planes cost 0.03 ms per frame and the worst measured 1080p logits error is 7.3e-4 instead of 8.8e-4,
                                        # profiles/r05/seed_sweep.log); False = the first two blocks write ONE f16 plane (the self-check ladder's "mixed" rung)
    C.MODEL.MIXED_SELF_CHECK = "auto"   # "mixed" only: before the first plan, measure a ladder of plans (mixed -> + layer1 lo planes -> all-f16 split ->
                                        # f32) against the fp32-input HIP path on four seeded frames, scan every 16-bit tensor for Inf / NaN, and keep the
                                        # first plan within 1e-3 (SemanticSegmentation.check_mixed_against_f32).  "auto" = when MODEL.WEIGHT names a
                                        # checkpoint (the margins of DESIGN section 4 were measured on seeded weights); True / False force it
    C.MODEL.MIXED_ON_FAIL = "f32"       # what the self-check does when no 16-bit plan passes: "f32" = run the fp32 plan (4x slower), "raise", or "warn"
                                        # (keep the best finite 16-bit plan)
    C.MODEL.SEED = 0               # seed of the random weights used when MODEL.WEIGHT == ""
    C.MODEL.HIP_GRAPH = True       # replay the ~90-kernel plan as one hipGraph launch per frame
    C.MODEL.VALIDATE_BATCH = False # SemanticSegmentation.validate_step also takes a batch [N, h, w, 3] with labels [N, h, w] (one batch-N forward and
                                   # one fused full-resolution pass).  Off by default: validate_step has always refused anything but one image with
                                   # NotImplementedError, and callers that rely on that keep it.  DeepLabV3Plus.validate_step takes batches regardless
    return C


def get_cfg_defaults():
    """base_cfg.py:15-18 -- a fresh clone of the defaults."""
    C = CfgNode()
    C.TASK_NAME = "cfn_mtx_with_intensity"
    C.OUTPUT_DIR = "@/outputs"
    C.TEST_END_TIME = 1581541450
    C.GROUND_TRUTH_DIR = ""
    C.RNG_SEED = -1
    C.LABELS = list(LABELS)
    C.LABELS_NAMES = list(LABELS_NAMES)
    C.LABEL_COLORS = [list(c) for c in LABEL_COLORS]
    C.MAPPING = CfgNode()
    C.MAPPING.RESOLUTION = 0.1
    C.MAPPING.BOUNDARY = [[100, 300], [800, 1000]]
    C.MAPPING.DEPTH_METHOD = "points_map"
    C.MAPPING.PCD = CfgNode()
    C.MAPPING.PCD.USE_INTENSITY = True
    C.MAPPING.PCD.RANGE_MAX = 100.0
    # build-specific: unpack PointCloud2 messages on the GPU (SemanticMapping.pcd then is a CUDA float32 [N,4] tensor)
    C.MAPPING.PCD.UNPACK_ON_DEVICE = False
    C.MAPPING.CONFUSION_MTX = CfgNode()
    C.MAPPING.CONFUSION_MTX.LOAD_PATH = ""
    C.MAPPING.INPUT_DIR = ""
    # build-specific: the planar (no-LiDAR) mode's class test: "reference" = as written (mapping.py:474 compares a uint8 channel
    # with the label NAME: never true, the mode only clamps negatives), "colour" = the R,G colour match of update_map
    C.MAPPING.PLANAR_MATCH = "reference"
    # build-specific: element type of the grid on the GPU ("f64" = the reference's, "f32")
    C.MAPPING.GRID_DTYPE = "f64"
    # build-specific: the live vehicle-centred map (SemanticMapping.live_map; the reference renders its map once, at shutdown).  With
    # ENABLED, mapping() / mapping_views() render the window around the vehicle after every EVERY-th mapped frame into
    # SemanticMapping.live_map_image (device) and live_map_host (pinned, valid once the stream is synchronised) and publish it on
    # pub_semantic_local_map under ROS.  The live path only reads the grid.  On several GPUs it shows the rank's private grid
    C.MAPPING.LIVE_MAP = CfgNode()
    C.MAPPING.LIVE_MAP.ENABLED = False
    C.MAPPING.LIVE_MAP.SIZE_M = [60.0, 60.0]              # window in metres along the grid's x, y; cells = int(size / RESOLUTION)
    C.MAPPING.LIVE_MAP.EVERY = 1
    C.MAPPING.LIVE_MAP.FILTER = True                      # renderer.apply_filter
    C.MAPPING.LIVE_MAP.RENDER = "argmax"                  # render_bev_map; "thresholds": render_bev_map_with_thresholds
    C.MAPPING.LIVE_MAP.PRIORITY = None
    C.MAPPING.LIVE_MAP.THRESHOLDS = None
    C.MAPPING.LIVE_MAP.FILL_BLACK = False                 # renderer.fill_black
    C.MAPPING.LIVE_MAP.FILL_PRIORITY = [0, 3, 4, 2, 1]    # low to high (renderer.py:67)
    C.MAPPING.LIVE_MAP.DRAW_CAR = True
    C.MAPPING.LIVE_MAP.CAR_SIZE = [4.0, 1.8]              # length, width in metres (src/mapping.py:502-503)
    # build-specific: the live map's geometry as a heading-up view (SemanticMapping.live_view): the vehicle's heading points up, the
    # vehicle sits at pixel ANCHOR * SIZE_PX, one pixel spans METRES_PER_PIXEL.  Filter, renderer, fill and car stay LIVE_MAP's.  With
    # LIVE_MAP.ENABLED, HEADING_UP makes mapping() / mapping_views() render this view instead of the axis-aligned window
    C.MAPPING.LIVE_VIEW = CfgNode()
    C.MAPPING.LIVE_VIEW.HEADING_UP = False
    C.MAPPING.LIVE_VIEW.SIZE_PX = [600, 600]              # height, width of the picture
    C.MAPPING.LIVE_VIEW.METRES_PER_PIXEL = 0.0            # 0: MAPPING.RESOLUTION (one cell per pixel)
    C.MAPPING.LIVE_VIEW.ANCHOR = [0.5, 0.5]               # fraction of the height from the top, of the width from the left
    # build-specific: the live cost map (SemanticMapping.cost_map): LIVE_MAP's window as what a planner reads -- an int8 cost per cell
    # (0 .. 100, 100 lethal, -1 no information) and an inflated margin around the lethal cells (the rule: include/avl_hip.h,
    # avl_cost_map).  With ENABLED, mapping() / mapping_views() compute it after every EVERY-th mapped frame into
    # SemanticMapping.cost_map_image (device) and cost_map_host (pinned, valid once the stream is synchronised) and publish a
    # nav_msgs/OccupancyGrid on /semantic_cost_map under ROS.  The cost map only reads the grid
    C.MAPPING.COST_MAP = CfgNode()
    C.MAPPING.COST_MAP.ENABLED = False
    C.MAPPING.COST_MAP.SIZE_M = [60.0, 60.0]              # window in metres along the grid's x, y; cells = int(size / RESOLUTION)
    C.MAPPING.COST_MAP.EVERY = 1
    C.MAPPING.COST_MAP.FILTER = True                      # renderer.apply_filter before the class is taken
    C.MAPPING.COST_MAP.RENDER = "argmax"                  # the class of render_bev_map; "thresholds": of render_bev_map_with_thresholds
    C.MAPPING.COST_MAP.PRIORITY = None
    C.MAPPING.COST_MAP.THRESHOLDS = None
    C.MAPPING.COST_MAP.CLASS_COST = [0, 0, 0, 100, 100]   # per entry of LABELS_NAMES: vegetation and sidewalk are lethal
    C.MAPPING.COST_MAP.UNKNOWN_COST = -1                  # an empty cell and everything off the grid: no information
    C.MAPPING.COST_MAP.INFLATION_RADIUS_M = 1.5           # cells = int(radius / RESOLUTION), 32 at the most
    C.MAPPING.COST_MAP.INSCRIBED_RADIUS_M = 0.9           # within it the cost stays 99
    C.MAPPING.COST_MAP.DECAY_PER_M = 3.0                  # beyond it: max(1, round(99 exp(-DECAY_PER_M (d - INSCRIBED_RADIUS_M))))
    C.MAPPING.COST_MAP.CLEAR_FOOTPRINT = True             # cells under the ego rectangle cost 0 and do not inflate
    C.MAPPING.COST_MAP.CAR_SIZE = [4.0, 1.8]              # length, width in metres (src/mapping.py:502-503)
    C.MAPPING.COST_MAP.ORDER = "yx"                       # "yx": [w, h], OccupancyGrid's data with x fastest; "xy": [h, w], the live map's
    # build-specific: occluded points do not vote (the reference lets a map point behind a wall take the wall's label).  Every view gets a
    # depth buffer of CELL_PX x CELL_PX pixel cells of the projection image; a point is culled when its depth exceeds
    # m * (1 + REL_TOL) + ABS_TOL, m the nearest depth within RADIUS cells (the rule: include/avl_hip.h, avl_occlusion).  Off by
    # default: nothing of it runs and no scratch is allocated.  The defaults are reasoned, not tuned on a recorded drive: at 20 m, with
    # the camera 2 m above the ground and f ~ 1000 px, the ground's depth changes by ~0.2 m per image row, so an 8 px cell spans ~8 %
    # of its depth.  The planar mode ignores the option
    C.MAPPING.OCCLUSION = CfgNode()
    C.MAPPING.OCCLUSION.ENABLED = False
    C.MAPPING.OCCLUSION.CELL_PX = 8                       # 1..64
    C.MAPPING.OCCLUSION.RADIUS = 1                        # 0..2 cells
    C.MAPPING.OCCLUSION.REL_TOL = 0.05
    C.MAPPING.OCCLUSION.ABS_TOL = 0.5                     # metres
    # build-specific: the confidence gate of the logits source (frame_device(..., src_kind="logits")).  A point takes the arg-max of the
    # plan's logits interpolated at its pixel; when the top-1 minus top-2 margin (fp32 logit units) is below MIN_MARGIN it abstains
    # instead of voting (the rule: include/avl_hip.h, avl_point_logits).  0.0 gates nothing.  A float >= 0 (SemanticMapping refuses
    # anything else).  The other sources ignore it
    C.MAPPING.CONFIDENCE = CfgNode()
    C.MAPPING.CONFIDENCE.MIN_MARGIN = 0.0
    # build-specific: dense ground fill.  After the LiDAR frame, every cell of a SIZE_M window around the vehicle puts its centre on the
    # ground plane (SemanticMapping.set_ground_plane / plane_callback), projects it into each camera and takes that pixel's label as one
    # update (the rule: include/avl_hip.h, avl_ground_fill), with OCCLUSION.ENABLED only where no LiDAR point hides the ground.  Off by
    # default: nothing of it runs.  RANGE_MAX is the fill's own range along the vehicle's x axis (a camera's label of the ground is
    # worth little at the cloud's 100 m); CLASSES names the map classes a cell may take (LABELS_NAMES; vegetation is no ground);
    # WEIGHT scales the confusion matrix of the fill's updates; a plane whose normal in the grid's frame is more than MAX_TILT_DEG
    # from the z axis is refused.  The planar mode ignores the option
    C.MAPPING.GROUND_FILL = CfgNode()
    C.MAPPING.GROUND_FILL.ENABLED = False
    C.MAPPING.GROUND_FILL.SIZE_M = [60.0, 60.0]           # window in metres along the grid's x, y, centred on the vehicle's cell
    C.MAPPING.GROUND_FILL.RANGE_MAX = 30.0
    C.MAPPING.GROUND_FILL.CLASSES = ["road", "crosswalk", "lane", "sidewalk"]
    C.MAPPING.GROUND_FILL.WEIGHT = 1.0
    C.MAPPING.GROUND_FILL.MAX_TILT_DEG = 30.0
    # build-specific: height-aware mapping, two independent options, both off by default (then every call runs what it ran before).
    # HEIGHT_GATE: with a ground plane (SemanticMapping.set_ground_plane / plane_callback) a LiDAR point votes class i only while its
    # height above the plane lies in [MIN_M[i] - s, MAX_M[i] + s], s = SLOPE x its forward distance (the rule: include/avl_hip.h,
    # avl_height): a canopy point no longer votes into the road cell beneath it.  MIN_M / MAX_M: one number for every class, or one
    # per entry of LABELS_NAMES (inf = unbounded).  ELEVATION: the z of the points that vote one of CLASSES is accumulated per cell
    # in steps of QUANTUM_M (sum, count, minimum, maximum: SemanticMapping.elevation_layer / elevation_device).  The ground fill,
    # the planar mode and update_map ignore both
    C.MAPPING.HEIGHT_GATE = CfgNode()
    C.MAPPING.HEIGHT_GATE.ENABLED = False
    C.MAPPING.HEIGHT_GATE.MIN_M = -0.5
    C.MAPPING.HEIGHT_GATE.MAX_M = [0.5, 0.5, 0.5, float("inf"), 0.5]   # road, crosswalk, lane, vegetation (unbounded), sidewalk
    C.MAPPING.HEIGHT_GATE.SLOPE = 0.02                    # metres of extra tolerance per metre of forward distance
    C.MAPPING.ELEVATION = CfgNode()
    C.MAPPING.ELEVATION.ENABLED = False
    C.MAPPING.ELEVATION.CLASSES = ["road", "crosswalk", "lane", "sidewalk"]
    C.MAPPING.ELEVATION.QUANTUM_M = 0.001
    # build-specific: where the cloud of DEPTH_METHOD "points_map" comes from.  "topic" = /reduced_map (the reference: a node outside
    # the package crops the site's point map around the vehicle and republishes it); nothing below is touched.  "index" = the whole
    # point map is loaded once from PATH (a .npy array [N, 4] or [4, N]: x, y, z, intensity in the world frame; or
    # SemanticMapping.load_points_map), sorted into ground tiles of TILE_M metres on the device, and every frame one kernel copies the
    # tiles that can hold a voting point into the frame's cloud (points_map.py; the rules: include/avl_hip.h, avl_points_map_gather).
    # RADIUS_M 0 = the exact window of the frame's cameras (the grid ends bit-equal to a frame on the whole map); > 0 = the square of
    # that half-side around the sensor, an external reducer's crop.  MARGIN_M grows either.  Another DEPTH_METHOD refuses "index"
    C.MAPPING.POINTS_MAP = CfgNode()
    C.MAPPING.POINTS_MAP.SOURCE = "topic"
    C.MAPPING.POINTS_MAP.PATH = ""
    C.MAPPING.POINTS_MAP.TILE_M = 10.0
    C.MAPPING.POINTS_MAP.RADIUS_M = 0.0
    C.MAPPING.POINTS_MAP.MARGIN_M = 1.0
    # build-specific: the scrolling grid.  Off: the grid is the fixed rectangle of BOUNDARY, as in the reference, and nothing below is
    # touched.  On: the device grid keeps its size but is a window whose origin moves in whole tiles of TILE_M metres so that the
    # vehicle stays near its centre (SemanticMapping.scroll_to, called by mapping() / mapping_views()); the BOUNDARY minimum is global
    # cell (0, 0) for good.  The origin moves when the vehicle's tile is more than HYSTERESIS_TILES from the centred position on
    # either axis.  Tiles that leave go to a store in HBM that grows by POOL_CHUNK_TILES tiles at a time (no host spill: until the
    # allocator refuses), tiles that enter come back from it or start empty (scroll.py; the job kernel: include/avl_hip.h,
    # avl_tile_job).  TILE_M / RESOLUTION must be a multiple of 4 cells and divide the grid; the planar mode and global_map() refuse
    C.MAPPING.SCROLL = CfgNode()
    C.MAPPING.SCROLL.ENABLED = False
    C.MAPPING.SCROLL.TILE_M = 10.0
    C.MAPPING.SCROLL.HYSTERESIS_TILES = 1
    C.MAPPING.SCROLL.POOL_CHUNK_TILES = 64
    # build-specific: the picture of a whole scrolled site (SemanticMapping.site_overview: one kernel from the tiles, where they live,
    # to a grid reduced by k x k cells per pixel and its picture; the rule: include/avl_hip.h, avl_tile_src).  ENABLED: finish_run()
    # of a scrolling map also writes site_map.png; off, nothing of it runs.  CELLS_PER_PIXEL 0 = the smallest divisor of the tile size
    # for which the picture's longer side is at most MAX_SIDE_PX.  THRESHOLDS [] = the arg-max renderer (render_bev_map's rule), else
    # one share per class (render_bev_map_with_thresholds' rule)
    C.MAPPING.SITE_OVERVIEW = CfgNode()
    C.MAPPING.SITE_OVERVIEW.ENABLED = False
    C.MAPPING.SITE_OVERVIEW.CELLS_PER_PIXEL = 0
    C.MAPPING.SITE_OVERVIEW.MAX_SIDE_PX = 4096
    C.MAPPING.SITE_OVERVIEW.THRESHOLDS = []
    # build-specific: the end-of-run result of a whole scrolled site (SemanticMapping.site_finish: one kernel from the tiles, where they
    # live, to the FILTERED picture at one pixel per cell, its labels and the ground-truth/label counts; the rule: include/avl_hip.h,
    # avl_tile_fin).  ENABLED: finish_run() of a scrolling map also writes site_global_map.png -- skipped, with a log line, when the
    # site's rectangle has more than MAX_PIXELS cells -- and, with TRUTH_PATH (an .npz of evaluation.SiteTruth.save), prints the site's
    # IoU / accuracy / missing-rate lines; off, nothing of it runs.  THRESHOLDS as in SITE_OVERVIEW
    C.MAPPING.SITE_FINISH = CfgNode()
    C.MAPPING.SITE_FINISH.ENABLED = False
    C.MAPPING.SITE_FINISH.TRUTH_PATH = ""
    C.MAPPING.SITE_FINISH.THRESHOLDS = []
    C.MAPPING.SITE_FINISH.MAX_PIXELS = 1 << 28
    C.VISION_SEM_SEG = CfgNode()
    C.VISION_SEM_SEG.IMAGE_SCALE = 1.0
    # build-specific: class indices whose convex hulls the node extracts from every frame's label map and back-projects onto the ground
    # plane (vision_semantic_segmentation_node.py:104-106, commented out in the reference: [2, 1] is what those two lines ask for).
    # [] = off: the hull code is never touched
    C.VISION_SEM_SEG.CONVEX_HULL_CLASSES = []
    # build-specific: where the ground plane of the extraction comes from.  "callback" = plane_callback only (the reference: another
    # package publishes /estimated_plane); nothing below is touched.  "cloud" = VisionSemanticSegmentationNode.cloud_callback estimates
    # it from the LiDAR cloud on the GPU (ground_plane.estimate_ground_plane_device; plane_callback keeps working).  The values
    # are this project's choices -- the reference has the plane model but no RANSAC driver
    C.VISION_SEM_SEG.GROUND_PLANE = CfgNode()
    C.VISION_SEM_SEG.GROUND_PLANE.SOURCE = "callback"
    C.VISION_SEM_SEG.GROUND_PLANE.HYPOTHESES = 256
    C.VISION_SEM_SEG.GROUND_PLANE.SEED = 0
    C.VISION_SEM_SEG.GROUND_PLANE.TOLERANCE = 0.1         # on Plane3D.eval's cost: metres at x = WEIGHT_X0, looser further out
    C.VISION_SEM_SEG.GROUND_PLANE.MAX_TILT_DEG = 30.0     # hypotheses whose normal is further from +z are dropped
    C.VISION_SEM_SEG.GROUND_PLANE.WEIGHT_X0 = 0.0         # Plane3D's "x norm" weight (plane_3d.py:19): x0 and the norm, 1 or 2
    C.VISION_SEM_SEG.GROUND_PLANE.WEIGHT_NORM = 1
    C.VISION_SEM_SEG.GROUND_PLANE.REFINE = True           # least-squares plane of the winner's inliers instead of the winner itself
    C.VISION_SEM_SEG.GROUND_PLANE.ROI = []                # [xmin, xmax, ymin, ymax, zmin, zmax] in the velodyne frame; [] = none
    C.VISION_SEM_SEG.SEM_SEG_NETWORK = get_network_cfg_defaults()
    return C
