"""VisionSemanticSegmentationNode -- the reference's segmentation node
(src/vision_semantic_segmentation_node.py:41-136) around the HIP segmentation stack.

image_callback keeps the reference's sequence (:74-136): BGR->RGB, cv2.undistort, optional INTER_AREA downscale,
``SemanticSegmentation.segmentation``, uint8 cast, INTER_NEAREST upscale to the input size, palette
colouring, publish.  Pre-processing runs inside the network's first kernel (the stem's loader applies BGR->RGB, undistort and
INTER_AREA per pixel while it fills its LDS tile; avl_preprocess_image is the same function as a stand-alone kernel), the
upscale + colouring is one more kernel (avl_colorize_labels); the frame is uploaded once and only the colour image comes back.

Semantic extraction (:104-106, :138-201) is the node's second product: with VISION_SEM_SEG.CONVEX_HULL_CLASSES set, the convex
hulls of the listed classes are taken from the frame's device labels in one call (semantic_convex_hull.class_hulls_device), only the
vertices come to the host, and they are back-projected onto the ground plane of plane_callback in the reference's float64 arithmetic.
With VISION_SEM_SEG.GROUND_PLANE.SOURCE = "cloud" that plane can also come from the LiDAR cloud (cloud_callback, ground_plane.py).
"""
import ctypes as C
import logging
import threading
import types

import numpy as np
import torch

from . import _lib
from .camera import camera_setup_1, camera_setup_6
from .labels import get_labels

_log = logging.getLogger(__name__)

# the topic cam_back_project_convex_hull publishes a class's hulls on (:194-197), and the marker look (:178-183)
CROSSWALK_HULL_TOPIC, ROAD_HULL_TOPIC = "/crosswalk_convex_hull_rviz", "/road_convex_hull_rviz"


def _palette_host(labels):
    pal = np.zeros((256, 3), dtype=np.uint8)
    for k, lab in enumerate(labels[:256]):
        pal[k] = lab["color"]
    return (C.c_uint8 * 768)(*pal.ravel().tolist())


def preprocess_device(bgr, camera=None, factor=1, stream=None):
    """vision_semantic_segmentation_node.py:83-98 on the GPU (avl_preprocess_image): BGR->RGB, cv2.undistort with the
    camera's K / dist (skipped when camera is None), INTER_AREA downscale by the integer `factor`.
    bgr: uint8 [H,W,3] ndarray or CUDA tensor -> uint8 CUDA tensor [H/factor, W/factor, 3] (RGB)."""
    t = bgr if isinstance(bgr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(bgr))
    t = t.cuda().contiguous() if not t.is_cuda else t.contiguous()
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
    h, w = int(t.shape[0]), int(t.shape[1])
    out = torch.empty((h // factor, w // factor, 3), dtype=torch.uint8, device=t.device)
    K = dist = None
    if camera is not None:
        K = (C.c_double * 9)(*np.asarray(camera.K, dtype=np.float64).ravel().tolist())
        dist = (C.c_double * 5)(*np.asarray(camera.dist, dtype=np.float64).ravel()[:5].tolist())
    s = torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().avl_preprocess_image(C.c_void_p(t.data_ptr()), h, w, K, dist, int(factor), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(s)), "avl_preprocess_image")
    return out


def preprocess_area_device(bgr, camera, out_h, out_w, stream=None):
    """The same chain with cv2.resize(INTER_AREA) to ANY smaller size (avl_preprocess_image_area): what the reference does for an
    IMAGE_SCALE that is not 1 / integer (:92-98: width = int(W * scale), height = int(H * scale))."""
    t = bgr if isinstance(bgr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(bgr))
    t = t.cuda().contiguous() if not t.is_cuda else t.contiguous()
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
    h, w = int(t.shape[0]), int(t.shape[1])
    out = torch.empty((int(out_h), int(out_w), 3), dtype=torch.uint8, device=t.device)
    K = dist = None
    if camera is not None:
        K = (C.c_double * 9)(*np.asarray(camera.K, dtype=np.float64).ravel().tolist())
        dist = (C.c_double * 5)(*np.asarray(camera.dist, dtype=np.float64).ravel()[:5].tolist())
    s = torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().avl_preprocess_image_area(C.c_void_p(t.data_ptr()), h, w, K, dist, int(out_h), int(out_w), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(s)), "avl_preprocess_image_area")
    return out


def colorize_labels_device(labels_small, out_h, out_w, labels=None, stream=None):
    """uint8 CUDA tensor [h,w] of class ids -> uint8 CUDA tensor [out_h,out_w,3]:
    cv2.resize(INTER_NEAREST) (:109-110) followed by apply_color_map
    (mapillary_visualization.py:70-89), fused."""
    assert labels_small.is_cuda and labels_small.dtype == torch.uint8 and labels_small.dim() == 2
    labels_small = labels_small.contiguous()
    out = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=labels_small.device)
    pal = _palette_host(labels if labels is not None else get_labels())
    s = torch.cuda.current_stream(labels_small.device).cuda_stream if stream is None else stream
    rc = _lib.lib().avl_colorize_labels(C.c_void_p(labels_small.data_ptr()), int(labels_small.shape[1]),
                                        int(labels_small.shape[0]), pal, C.c_void_p(out.data_ptr()), int(out_w), int(out_h),
                                        C.c_void_p(s))
    _lib.check(rc, "avl_colorize_labels")
    return out


class VisionSemanticSegmentationNode(object):
    """Reference class: src/vision_semantic_segmentation_node.py:41."""

    def __init__(self, cfg, seg=None, use_ros=False, publish=None, undistort=True, publish_markers=None):
        if cfg.VISION_SEM_SEG.IMAGE_SCALE < 0 or cfg.VISION_SEM_SEG.IMAGE_SCALE > 1:
            raise ValueError("image scale should be in the range of [0, 1]")       # :43-44
        network_cfg = cfg.VISION_SEM_SEG.SEM_SEG_NETWORK
        if seg is None:
            from .semantic_segmentation import SemanticSegmentation
            seg = SemanticSegmentation(network_cfg)
        self.seg = seg
        self.seg_color_ref = get_labels(network_cfg.DATASET_CONFIG)                # :63
        self.cam6 = camera_setup_6()
        self.cam1 = camera_setup_1()
        self.image_scale = cfg.VISION_SEM_SEG.IMAGE_SCALE
        self.publish = publish          # callable(frame_id, colour image, header) or None
        self.undistort = undistort      # the reference always undistorts camera1 / camera6 frames (:84-87)
        self.last_labels = None         # CUDA uint8 [h', w'] of the last frame (feeds the fused mapping path)
        self.publish_markers = publish_markers       # callable(topic, list of marker dicts) or None
        self.hull_classes = [int(c) for c in cfg.VISION_SEM_SEG.CONVEX_HULL_CLASSES]   # [] = no semantic extraction (:105-106 stay off)
        self.plane = None               # Plane3D of the last plane_callback (:65)
        self.hull_id = 0                # :70
        self._hull_workspace = None
        self._warned_no_plane = False
        self.ground_plane_cfg = cfg.VISION_SEM_SEG.GROUND_PLANE
        if self.ground_plane_cfg.SOURCE not in ("callback", "cloud"):
            raise ValueError("VISION_SEM_SEG.GROUND_PLANE.SOURCE must be \"callback\" or \"cloud\", got %r" % (self.ground_plane_cfg.SOURCE,))
        self._plane_workspace = None
        self._plane_lock = threading.Lock()
        self._warned_no_cloud_plane = False
        self._marker_msgs = None        # (Marker, MarkerArray, Point) once ROS markers are wanted
        self.pub_crosswalk_markers = self.pub_road_markers = None
        # rospy runs each subscription's callback on its own thread, and both cameras share one compiled plan (fixed
        # input / activation / label buffers on one stream): one frame at a time through upload -> net -> colour -> download
        self._lock = threading.Lock()
        self._ros_image_cls = None
        self.image_pub_cam1 = self.image_pub_cam6 = None
        if use_ros:
            self._setup_ros()

    def _setup_ros(self):
        import rospy
        from sensor_msgs.msg import Image
        self.image_sub_cam1 = rospy.Subscriber("/camera1/image_raw", Image, self.image_callback)
        self.image_sub_cam6 = rospy.Subscriber("/camera6/image_raw", Image, self.image_callback)
        self.image_pub_cam1 = rospy.Publisher("/camera1/semantic", Image, queue_size=1)
        self.image_pub_cam6 = rospy.Publisher("/camera6/semantic", Image, queue_size=1)
        self._ros_image_cls = Image
        from shape_msgs.msg import Plane
        from visualization_msgs.msg import Marker, MarkerArray
        from geometry_msgs.msg import Point
        self.plane_sub = rospy.Subscriber("/estimated_plane", Plane, self.plane_callback)                       # :51
        self.pub_crosswalk_markers = rospy.Publisher(CROSSWALK_HULL_TOPIC, MarkerArray, queue_size=10)          # :56-57
        self.pub_road_markers = rospy.Publisher(ROAD_HULL_TOPIC, MarkerArray, queue_size=10)
        self._marker_msgs = (Marker, MarkerArray, Point)

    def _publish_ros(self, colored, header):
        """:118-134 -- the colour image as an 8UC3 sensor_msgs/Image (cv_bridge's "passthrough" of a uint8 H x W x 3 array)
        with the INPUT message's stamp and frame_id, on the publisher of that camera."""
        pub = {"camera1": self.image_pub_cam1, "camera6": self.image_pub_cam6}.get(header.frame_id)
        if pub is None:
            return None                                           # :135-136: the reference only warns
        out = self._ros_image_cls()
        out.height, out.width = int(colored.shape[0]), int(colored.shape[1])
        out.encoding, out.is_bigendian, out.step = "8UC3", 0, int(colored.shape[1]) * 3
        out.data = np.ascontiguousarray(colored).tobytes()
        out.header.stamp = header.stamp
        out.header.frame_id = header.frame_id
        pub.publish(out)
        return out

    def _downscale_factor(self, h=None, w=None):
        """IMAGE_SCALE -> integer INTER_AREA factor (:92-98), or None when the frame does not shrink by an integer ratio (the reference's
        configs use 1.0 and 0.5): the general area resize (preprocess_area_device) then makes the (int(h * scale), int(w * scale)) input."""
        if self.image_scale >= 1:
            return 1
        f = int(round(1.0 / self.image_scale))
        if abs(f * self.image_scale - 1.0) > 1e-9 or (h is not None and (h % f or w % f)):
            return None
        return f

    # ------------------------------------------------------------------------------------------ semantic extraction
    def plane_callback(self, msg):
        """:199-201 -- shape_msgs/Plane: msg.coef[0..3] = a, b, c, d of the estimated ground plane."""
        from .plane_3d import Plane3D
        self.plane = Plane3D(msg.coef[0], msg.coef[1], msg.coef[2], msg.coef[3])

    def cloud_callback(self, points, pcd_frame_id="velodyne", pose=None):
        """With GROUND_PLANE.SOURCE == "cloud": estimates the ground plane from the cloud (ndarray or tensor, [4, N] or [N, 4]) on the
        GPU and sets ``self.plane`` exactly as plane_callback does, from the plane's four coefficients.  A cloud that is not in the
        velodyne frame is taken there with the pose (SemanticMapping._origin_to_velodyne, mapping.py:368-373).  When no hypothesis
        has an inlier the previous plane stays and one warning is logged.  With SOURCE == "callback" this does nothing.  Returns the
        GroundPlaneResult, or None when nothing was estimated."""
        gp = self.ground_plane_cfg
        if gp.SOURCE != "cloud":
            return None
        from .ground_plane import GroundPlaneWorkspace, estimate_ground_plane_device
        T = None
        if pcd_frame_id != "velodyne":
            if pose is None:
                raise ValueError("a cloud in frame %r needs the pose to reach the velodyne frame" % (pcd_frame_id,))
            from .mapping import origin_to_velodyne, velodyne_to_baselink
            T = origin_to_velodyne(pose, velodyne_to_baselink())
        device = points.device if isinstance(points, torch.Tensor) and points.is_cuda else torch.device("cuda", torch.cuda.current_device())
        points, n = _lib.points_view(points, device)[:2]
        # its own lock: the workspace is shared between calls and a result refers to it until host() has read it.  The frame lock is
        # not taken, so image callbacks go on while the estimate runs; plane_callback takes no lock (one attribute store)
        with self._plane_lock:
            ws = self._plane_workspace
            if ws is None or not ws.fits(n, int(gp.HYPOTHESES), device):
                ws = self._plane_workspace = GroundPlaneWorkspace(n, int(gp.HYPOTHESES), device)
            weight = {'method': "x norm", 'param': {'x0': float(gp.WEIGHT_X0), 'norm': int(gp.WEIGHT_NORM)}}
            result = estimate_ground_plane_device(points, hypotheses=int(gp.HYPOTHESES), seed=int(gp.SEED), tolerance=float(gp.TOLERANCE),
                                                  weight=weight, max_tilt_deg=float(gp.MAX_TILT_DEG), roi=list(gp.ROI) or None, T=T,
                                                  refine=bool(gp.REFINE), workspace=ws, device=device).host()
        if result.plane is None:
            if not self._warned_no_cloud_plane:
                _log.warning("no ground plane in the cloud (%d points used, %d valid hypotheses): the previous plane stays",
                             result.used, result.valid)
                self._warned_no_cloud_plane = True
            return result
        p = result.plane
        self.plane_callback(types.SimpleNamespace(coef=[p.a, p.b, p.c, p.d]))
        return result

    def _camera_of(self, cam_frame_id):
        return {"camera1": self.cam1, "camera6": self.cam6}.get(cam_frame_id)

    def generate_and_publish_convex_hull(self, image, cam_frame_id, index_care_about=1):
        """:138-152 -- hulls of class index_care_about in the label map `image` (ndarray or the device labels), scaled from the
        network's output size to the camera's image size, back-projected and published.  Returns the markers."""
        from .semantic_convex_hull import generate_convex_hull
        cam = self._camera_of(cam_frame_id)
        if cam is None:
            raise ValueError("no camera model for frame id %r" % (cam_frame_id,))      # the reference fails on its unbound `cam`
        vertice_list = generate_convex_hull(image, index_care_about=index_care_about, vis=False)
        vertice_list = self._scale_to_camera(cam, vertice_list, int(image.shape[0]), int(image.shape[1]))
        markers = self.cam_back_project_convex_hull(cam, vertice_list, index_care_about=index_care_about)
        self._send_markers([(index_care_about, markers)])
        return markers

    @staticmethod
    def _scale_to_camera(cam, vertice_list, h, w):
        scale = np.array([[float(cam.imSize[0]) / w, float(cam.imSize[1]) / h]]).T                              # :147-150
        return [v * scale for v in vertice_list]

    def cam_back_project_convex_hull(self, cam, vertice_list, index_care_about=1):
        """:154-197 -- every hull's pixels [2, n] become rays (Camera.pixel_to_ray_vec) that are cut with the ground plane
        (Plane3D.plane_ray_intersection_vec); one line-strip marker per hull in the "velodyne" frame, ids counted in ``hull_id``.
        Returns the list of marker dicts (id, frame_id, type, scale, color, lifetime, points [n, 3]); nothing is sent from here."""
        markers = []
        if len(vertice_list) == 0:
            return markers
        if self.plane is None:
            raise RuntimeError("cam_back_project_convex_hull needs a ground plane: no plane_callback yet")
        for vertices in vertice_list:
            d_vec, C_vec = cam.pixel_to_ray_vec(vertices)
            intersection_vec = self.plane.plane_ray_intersection_vec(d_vec, C_vec)
            self.hull_id += 1
            if index_care_about == 1:
                color, vis_time = [0.8, 0., 0., 0.8], 10.0
            else:
                color, vis_time = [0.0, 0, 0.8, 0.8], 3.0
            markers.append({"id": self.hull_id, "frame_id": "velodyne", "type": "line_strip", "scale": 0.1, "color": color,
                            "lifetime": vis_time, "points": intersection_vec.T})
        return markers

    def _extract_hulls(self, labels, frame_ids):
        """Under the lock, between segmentation and colourising (:104-106): ONE class_hulls_device call for every view and every
        listed class, one copy of the vertices to the host, then the host-side back-projection.  labels [h', w'] or [V, h', w'].
        Returns [(class index, markers)] in view order, classes in the configured order."""
        if not self.hull_classes:
            return []
        if self.plane is None:
            if not self._warned_no_plane:
                _log.warning("no ground plane received yet (plane_callback): semantic extraction is skipped until one arrives")
                self._warned_no_plane = True
            return []
        from .semantic_convex_hull import class_hulls_device, hull_workspace_bytes
        batch = labels if labels.dim() == 3 else labels[None]
        V, h, w = (int(v) for v in batch.shape)
        need = hull_workspace_bytes(h, w, V * len(self.hull_classes), 1)
        if self._hull_workspace is None or self._hull_workspace.numel() < need or self._hull_workspace.device != batch.device:
            self._hull_workspace = torch.empty(need, dtype=torch.uint8, device=batch.device)
        polygons = class_hulls_device(batch, self.hull_classes, workspace=self._hull_workspace).polygons()
        out = []
        for v, frame_id in enumerate(frame_ids):
            cam = self._camera_of(frame_id)
            if cam is None:
                continue                                         # no model to back-project with (:139-142 know two cameras)
            for k, index in enumerate(self.hull_classes):
                vertice_list = self._scale_to_camera(cam, polygons[v][k], h, w)
                out.append((index, self.cam_back_project_convex_hull(cam, vertice_list, index_care_about=index)))
        return out

    def _send_markers(self, hulls):
        for index, markers in hulls:
            if not markers:
                continue                                         # :155-157: nothing is published for an empty list
            topic = CROSSWALK_HULL_TOPIC if index == 1 else ROAD_HULL_TOPIC                                     # :194-197
            if self.publish_markers is not None:
                self.publish_markers(topic, markers)
            if self._marker_msgs is not None:
                self._publish_markers_ros(index, markers)

    def _publish_markers_ros(self, index, markers):
        """The marker dicts as a visualization_msgs/MarkerArray of LINE_STRIP markers (src/vis.py:19-107)."""
        import rospy
        Marker, MarkerArray, Point = self._marker_msgs
        array = MarkerArray()
        for m in markers:
            mk = Marker()
            mk.header.frame_id, mk.header.stamp = m["frame_id"], rospy.get_rostime()
            mk.action, mk.id, mk.type = 0, m["id"], Marker.LINE_STRIP
            mk.lifetime.secs, mk.lifetime.nsecs = int(m["lifetime"]), int(m["lifetime"] % 1.0 * 1e9)
            mk.color.r, mk.color.g, mk.color.b, mk.color.a = m["color"]
            mk.scale.x = mk.scale.y = mk.scale.z = m["scale"]
            for p in m["points"]:
                mk.points.append(Point(x=float(p[0]), y=float(p[1]), z=float(p[2])))
            array.markers.append(mk)
        (self.pub_crosswalk_markers if index == 1 else self.pub_road_markers).publish(array)

    def image_callback(self, msg):
        """:74-136.  msg.data: uint8[H,W,3] BGR (as the camera driver publishes it).  The whole chain runs on the GPU:
        pre-processing (:83-98), segmentation (:101-102), nearest upscale + palette (:109-116); only the published
        colour image comes back to the host.  Returns that uint8[H,W,3] image (also handed to ``publish``)."""
        if isinstance(msg.data, (np.ndarray, torch.Tensor)):
            bgr = msg.data
        else:                                         # a sensor_msgs/Image: bytes + height / width / step / encoding (:76-80)
            from .mapping import _imgmsg_to_array
            bgr = _imgmsg_to_array(msg)
            if bgr.ndim != 3:
                raise ValueError("image_callback needs a 3-channel image, got encoding %r" % (msg.encoding,))
        h, w = int(bgr.shape[0]), int(bgr.shape[1])
        cam = {"camera1": self.cam1, "camera6": self.cam6}.get(msg.header.frame_id)   # unknown frame ids: no undistortion (:88-89)
        with self._lock:
            cam = cam if self.undistort else None
            factor = self._downscale_factor(h, w)
            if factor is None:                                   # any other IMAGE_SCALE: OpenCV's general area resize as a stand-alone kernel
                labels = self.seg.segmentation_device(preprocess_area_device(bgr, cam, int(h * self.image_scale), int(w * self.image_scale)))
            else:                                                # pre-processing inside the stem's loader (no RGB frame in between)
                labels = self.seg.segmentation_device_raw(bgr, None if cam is None else cam.K, None if cam is None else cam.dist, factor)
            self.last_labels = labels
            hulls = self._extract_hulls(labels, [msg.header.frame_id])
            colored = colorize_labels_device(labels, h, w, self.seg_color_ref)
            out = colored.cpu().numpy()
        self._send_markers(hulls)
        if self.publish is not None:
            self.publish(msg.header.frame_id, out, msg.header)                     # :129-134
        if self._ros_image_cls is not None:
            self._publish_ros(out, msg.header)
        return out

    def image_callback_views(self, msgs):
        """V raw frames of one trigger through ONE batched plan.  With an integer INTER_AREA factor (IMAGE_SCALE 1.0, 0.5, ...) the raw
        frames go straight into the batched raw-frame plan (segmentation_device_raw_batch): each is pre-processed inside the stem's
        loader with its own camera's model (:83-98), as image_callback does it for one frame.  Any other IMAGE_SCALE: each frame goes
        through preprocess_area_device into one [V, h, w, 3] buffer and a single segmentation_device call labels the batch.  Every
        view is colourised and published as image_callback does it.  Returns the plan's [V, h', w'] label tensor (CUDA uint8; also in
        ``last_labels``), which SemanticMapping.frame_device_views takes as it is.  Frames of different sizes raise ValueError."""
        msgs = list(msgs)
        if not msgs:
            raise ValueError("image_callback_views needs at least one message")
        frames = []
        for msg in msgs:
            if isinstance(msg.data, (np.ndarray, torch.Tensor)):
                bgr = msg.data
            else:
                from .mapping import _imgmsg_to_array
                bgr = _imgmsg_to_array(msg)
                if bgr.ndim != 3:
                    raise ValueError("image_callback_views needs 3-channel images, got encoding %r" % (msg.encoding,))
            frames.append(bgr)
        h, w = int(frames[0].shape[0]), int(frames[0].shape[1])
        for bgr in frames:
            if (int(bgr.shape[0]), int(bgr.shape[1])) != (h, w):
                raise ValueError("the frames of one trigger must have one size: %dx%d and %dx%d" % (h, w, int(bgr.shape[0]), int(bgr.shape[1])))
        with self._lock:
            factor = self._downscale_factor(h, w)
            cams = [{"camera1": self.cam1, "camera6": self.cam6}.get(msg.header.frame_id) if self.undistort else None for msg in msgs]
            if factor is None:                                   # any other IMAGE_SCALE: the general area resize, one stand-alone kernel per view
                batch = None
                for v, (cam, bgr) in enumerate(zip(cams, frames)):
                    rgb = preprocess_area_device(bgr, cam, int(h * self.image_scale), int(w * self.image_scale))
                    if batch is None:
                        batch = torch.empty((len(msgs),) + tuple(rgb.shape), dtype=torch.uint8, device=rgb.device)
                    batch[v].copy_(rgb)
                labels = self.seg.segmentation_device(batch)
            else:                                                # pre-processing inside the batched stem's loader, one camera block per view
                labels = self.seg.segmentation_device_raw_batch(frames, [None if c is None else c.K for c in cams],
                                                                [None if c is None else c.dist for c in cams], factor)
            self.last_labels = labels
            hulls = self._extract_hulls(labels, [msg.header.frame_id for msg in msgs])
            outs = [colorize_labels_device(labels[v], h, w, self.seg_color_ref).cpu().numpy() for v in range(len(msgs))]
        self._send_markers(hulls)
        for msg, out in zip(msgs, outs):
            if self.publish is not None:
                self.publish(msg.header.frame_id, out, msg.header)
            if self._ros_image_cls is not None:
                self._publish_ros(out, msg.header)
        return labels
