"""End-of-run rendering on the GPU -- counterpart of src/renderer.py (render_bev_map :32-59,
render_bev_map_with_thresholds :131-172, apply_filter :175-189), which the reference runs once at shutdown
(src/mapping.py:332-334).  Same function names and argument meaning; inputs may be NumPy arrays (results come
back as NumPy) or CUDA tensors (results stay on the GPU), so a live map can be rendered every frame.

The renderer's remaining functions are here too: fill_black with resume_color (:62-105) and fill_edge (:192-196), which the reference
defines and never calls, and render_window, the per-frame front end: filter, renderer, hole fill and the ego car
(src/mapping.py:490-526) over a window of the grid in one kernel (avl_live_map), bit-equal to a crop of the chain of the functions
above.  render_view is the same picture through a 2 x 3 matrix from output pixels to grid cells (avl_live_view): rotated, scaled,
heading-up with view_matrix.  cost_window is the window as a planner reads it (avl_cost_map): an int8 cost per cell from its class and
an inflated margin around the lethal cells, from inflation_table.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .labels import LABEL_COLORS

FILL_PRIORITY = (0, 3, 4, 2, 1)          # renderer.py:67, from low to high
CAR_SIZE = (4.0, 1.8)                    # src/mapping.py:502-503: length, width in metres
CAR_COLOR = (255, 0, 0)                  # src/mapping.py:525


def _prep(map_):
    is_np = not isinstance(map_, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(map_)).cuda() if is_np else map_.contiguous()
    if t.dtype not in (torch.float64, torch.float32):
        t = t.to(torch.float64)
    assert t.dim() == 3, "map must be [W, H, C]"
    return t, is_np, (_lib.AVL_F64 if t.dtype == torch.float64 else _lib.AVL_F32)


def _colors(label_colors, c):
    lc = np.ascontiguousarray(np.asarray(label_colors), dtype=np.uint8)
    for col in lc:
        if len(col) != 3:
            raise ValueError("Color should be an RGB value.")
    if len(lc) != c:
        raise ValueError("Each channel should have a color!")
    return (C.c_uint8 * lc.size)(*lc.ravel().tolist())


def render_params(label_colors, c, thresholds=None, priority=None):
    """(colours, priority, thresholds) of a map of ``c`` channels as the ctypes arrays every renderer entry point of the library takes;
    ``priority`` / ``thresholds`` None stay None (the library's defaults: 0 .. c - 1, and the arg-max renderer where it has the
    choice).  Fewer thresholds than channels raise IndexError, as the reference's ``thresholds[i]`` does; further ones are ignored."""
    colors = _colors(label_colors, c)
    th = pr = None
    if thresholds is not None:
        thresholds = list(thresholds)
        if len(thresholds) < c:
            raise IndexError("%d thresholds for %d channels: every channel needs one" % (len(thresholds), c))
        th = (C.c_double * c)(*[float(x) for x in thresholds[:c]])
    if priority is not None:
        if len(priority) != c:
            raise ValueError("Each channel should have a priority.")
        pr = (C.c_int32 * c)(*[int(p) for p in priority])
    return colors, pr, th


def out_picture(out, h, w, device):
    """``out`` if it is a contiguous uint8 [h, w, 3] tensor on ``device`` (ValueError otherwise), a new one for None"""
    if out is None:
        return torch.empty((max(h, 0), max(w, 0), 3), dtype=torch.uint8, device=device)
    if tuple(out.shape) != (h, w, 3) or out.dtype != torch.uint8 or out.device != device or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 [%d, %d, 3] tensor on %s" % (h, w, device))
    return out


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def render_bev_map(map, label_colors):
    """renderer.py:32-59: colour of each cell = colour of its arg-max channel; all-zero cells stay black."""
    t, is_np, dt = _prep(map)
    h, w, c = t.shape
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=t.device)
    _lib.check(_lib.lib().avl_render_bev_map(C.c_void_p(t.data_ptr()), dt, h, w, c, _colors(label_colors, c),
                                             C.c_void_p(out.data_ptr()), _stream(t)), "avl_render_bev_map")
    return out.cpu().numpy() if is_np else out


def render_bev_map_with_thresholds(map, label_colors, priority=None, thresholds=(0.01, 0.01, 0.01, 0.01, 0.01)):
    """renderer.py:131-172: a label is drawn where its normalised share reaches its threshold; `priority` lists the
    labels from low to high, higher ones overwrite lower ones.  Fewer thresholds than channels raise IndexError, as the
    reference's `thresholds[i]` does."""
    colors, pr, th = render_params(label_colors, int(map.shape[-1]), thresholds, priority)     # raises before the map is uploaded
    t, is_np, dt = _prep(map)
    h, w, c = t.shape
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=t.device)
    _lib.check(_lib.lib().avl_render_bev_map_thresholds(C.c_void_p(t.data_ptr()), dt, h, w, c, colors, pr, th,
                                                        C.c_void_p(out.data_ptr()), _stream(t)), "avl_render_bev_map_thresholds")
    return out.cpu().numpy() if is_np else out


def apply_filter(src):
    """renderer.py:175-189: 3x3 mean filter of every channel (cv2.filter2D, reflect-101 border)."""
    t, is_np, dt = _prep(src)
    h, w, c = t.shape
    dst = torch.empty_like(t)
    _lib.check(_lib.lib().avl_grid_box_filter(C.c_void_p(t.data_ptr()), C.c_void_p(dst.data_ptr()), dt, h, w, c, _stream(t)),
               "avl_grid_box_filter")
    return dst.cpu().numpy() if is_np else dst


def fill_black(img, label_colors=LABEL_COLORS, priority_list=FILL_PRIORITY):
    """renderer.py:62-98 with resume_color (:101-105), as written: EVERY pixel of the interior, black or not, takes the colour of the
    highest-priority label whose R value occurs among the R values of its 3 x 3 neighbourhood (black if none does).  Matching is
    on R only.  img uint8 [X, Y, 3] -> [X - 2, Y - 2, 3]; the colours and the priority list (low to high) are module constants in
    the reference and arguments here.  NumPy in gives NumPy out, a CUDA tensor stays on the device."""
    is_np = not isinstance(img, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda() if is_np else img.contiguous()
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("fill_black takes a uint8 [X, Y, 3] colour image")
    x, y = int(t.shape[0]), int(t.shape[1])
    lc = np.asarray(label_colors)
    prio = [int(p) for p in priority_list]
    out = torch.empty((max(x - 2, 0), max(y - 2, 0), 3), dtype=torch.uint8, device=t.device)
    _lib.check(_lib.lib().avl_fill_black(C.c_void_p(t.data_ptr()), x, y, _colors(lc, len(lc)), len(lc), (C.c_int32 * max(len(prio), 1))(*prio),
                                         len(prio), C.c_void_p(out.data_ptr()), _stream(t)), "avl_fill_black")
    return out.cpu().numpy() if is_np else out


def fill_edge(color_map):
    """renderer.py:192-196: 250 on the outer ring, 254 in the 5 x 5 corner; in place (array or tensor) and returned."""
    color_map[0, :, :] = 250
    color_map[-1, :, :] = 250
    color_map[:, 0, :] = 250
    color_map[:, -1, :] = 250
    color_map[0:5, 0:5] = 254
    return color_map


def car_block(cx, cy, cos_yaw, sin_yaw, resolution, size=CAR_SIZE):
    """avl_live_map's car block: the vehicle at the un-truncated grid position (cx, cy) cells, heading (cos, sin) in the grid's x, y
    axes, footprint `size` = (length, width) metres with the reference point a quarter length from the rear
    (src/mapping.py:502-511)."""
    length, width, res = float(size[0]), float(size[1]), float(resolution)
    return (float(cx), float(cy), float(cos_yaw), float(sin_yaw),
            -length / (4.0 * res), 3.0 * length / (4.0 * res), -width / (2.0 * res), width / (2.0 * res))


def _live_args(t, label_colors, size, filter, thresholds, priority, fill, fill_priority, car, car_color, out, stream):
    """the arguments avl_live_map and avl_live_view share, as ctypes values (kept alive by the caller's tuple)"""
    hm, wm, c = t.shape
    h, w = int(size[0]), int(size[1])
    colors, pr, th = render_params(label_colors, c, thresholds, priority)
    flags = (_lib.AVL_LIVE_FILTER if filter else 0) | (_lib.AVL_LIVE_THRESHOLDS if th is not None else 0) | \
            (_lib.AVL_LIVE_FILL if fill else 0)
    fp = [int(p) for p in fill_priority] if fill else []
    car_c = col_c = None
    if car is not None:
        if len(car) != _lib.AVL_LIVE_CAR_DOUBLES:
            raise ValueError("car is car_block(...): %d numbers" % _lib.AVL_LIVE_CAR_DOUBLES)
        car_c = (C.c_double * _lib.AVL_LIVE_CAR_DOUBLES)(*[float(v) for v in car])
        col_c = (C.c_uint8 * 3)(*[int(v) for v in car_color])
    out = out_picture(out, h, w, t.device)
    s = _stream(t) if stream is None else C.c_void_p(int(stream))
    return h, w, colors, flags, pr, th, (C.c_int32 * max(len(fp), 1))(*fp), len(fp), car_c, col_c, out, s


def render_window(map, label_colors, origin, size, filter=True, thresholds=None, priority=None, fill=False,
                  fill_priority=FILL_PRIORITY, car=None, car_color=CAR_COLOR, out=None, stream=None):
    """The window of `size` = (h, w) cells whose first cell is grid cell `origin` = (x0, y0), uint8 [h, w, 3]: what
    ``render_bev_map(apply_filter(map).astype(map.dtype), label_colors)[x0:x0 + h, y0:y0 + w]`` gives (bit for bit), black where the
    window leaves the grid -- in one kernel, reading about nine windows' worth of the grid and writing no temporary.
    filter=False skips apply_filter; `thresholds` (with `priority`, low to high) picks render_bev_map_with_thresholds; fill=True
    applies fill_black (label_colors, fill_priority) over the grid's interior, with a one-cell black ring where its output is
    smaller than the grid; `car` = car_block(...) paints the ego footprint last.  The grid is only read."""
    t, is_np, dt = _prep(map)
    hm, wm, c = t.shape
    h, w, colors, flags, pr, th, fp, n_fp, car_c, col_c, out, s = _live_args(t, label_colors, size, filter, thresholds, priority, fill,
                                                                             fill_priority, car, car_color, out, stream)
    _lib.check(_lib.lib().avl_live_map(C.c_void_p(t.data_ptr()), dt, hm, wm, c, colors, int(origin[0]), int(origin[1]), h, w,
                                       flags, pr, th, fp, n_fp, car_c, col_c, C.c_void_p(out.data_ptr()), s), "avl_live_map")
    return out.cpu().numpy() if is_np else out


def view_matrix(centre_cells, heading, cells_per_pixel, size, anchor=(0.5, 0.5)):
    """The 2 x 3 float64 matrix of render_view for a heading-up picture of `size` = (h, w) pixels: pixel centre (anchor[0] * h,
    anchor[1] * w) -- fractions of the height from the top and of the width from the left -- shows the grid position `centre_cells`
    = (cx, cy) in cells, up in the picture is `heading` = (cos, sin) in the grid's x, y axes (mapping.pose_heading), right is the
    vehicle's right seen from above, (sin, -cos), and one pixel spans `cells_per_pixel` cells.  heading (-1, 0) at 1 cell per pixel
    is the orientation of render_window."""
    k, (c, s) = float(cells_per_pixel), (float(heading[0]), float(heading[1]))
    cx, cy = float(centre_cells[0]), float(centre_cells[1])
    ai, aj = float(anchor[0]) * int(size[0]), float(anchor[1]) * int(size[1])
    m00, m01, m10, m11 = -k * c, k * s, -k * s, -k * c
    return np.array([[m00, m01, (cx - m00 * ai) - m01 * aj], [m10, m11, (cy - m10 * ai) - m11 * aj]], dtype=np.float64)


def render_view(map, label_colors, matrix, size, filter=True, thresholds=None, priority=None, fill=False,
                fill_priority=FILL_PRIORITY, car=None, car_color=CAR_COLOR, out=None, stream=None):
    """The live picture through `matrix` (2 x 3, float64), uint8 [h, w, 3] for `size` = (h, w): pixel (i, j) shows the grid cell
    (floor(gx), floor(gy)) with gx = (M00 (i + 0.5) + M01 (j + 0.5)) + M02 and gy likewise from row 1 -- nearest-cell sampling of
    what render_window draws for the whole grid (filter, renderer, fill_black with its black ring), black where (gx, gy) leaves
    the grid; `car` = car_block(...) is tested on (gx, gy) itself and painted last.  One kernel, no temporary; the other arguments
    are render_window's.  With matrix [[1, 0, x0], [0, 1, y0]] this is render_window(origin=(x0, y0)) byte for byte.  |M00| + |M01|
    and |M10| + |M11| may not exceed _lib.AVL_LIVE_VIEW_MAX_SPAN (any rotation up to 2 cells per pixel does not)."""
    t, is_np, dt = _prep(map)
    hm, wm, c = t.shape
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64))
    if m.shape != (2, 3):
        raise ValueError("matrix must be 2 x 3, not %s" % (m.shape,))
    h, w, colors, flags, pr, th, fp, n_fp, car_c, col_c, out, s = _live_args(t, label_colors, size, filter, thresholds, priority, fill,
                                                                             fill_priority, car, car_color, out, stream)
    _lib.check(_lib.lib().avl_live_view(C.c_void_p(t.data_ptr()), dt, hm, wm, c, colors, (C.c_double * 6)(*m.ravel().tolist()), h, w,
                                        flags, pr, th, fp, n_fp, car_c, col_c, C.c_void_p(out.data_ptr()), s), "avl_live_view")
    return out.cpu().numpy() if is_np else out


# ---------------------------------------------------------------------------------------------------- the live cost map
_cost_scratch = {}       # (device, stream, bytes) -> uint8 CUDA tensor: avl_cost_map's byte plane


def inflation_table(radius_cells, resolution, inscribed_m, decay_per_m, max_cost=99):
    """avl_cost_map's inflation table, uint8 [R * R + 1] indexed by the squared distance in cells to the nearest lethal cell: entry 0
    is 100 (the lethal cell itself); for d = sqrt(d2) * resolution metres, ``max_cost`` while d <= inscribed_m, else
    max(1, round(max_cost * exp(-decay_per_m * (d - inscribed_m)))) -- costmap_2d's inflation curve.  float64, host only: the
    kernels see the table alone."""
    r = int(radius_cells)
    if not 0 <= r <= _lib.AVL_COST_MAX_RADIUS:
        raise ValueError("radius_cells = %d: 0 .. %d" % (r, _lib.AVL_COST_MAX_RADIUS))
    if not 1 <= int(max_cost) <= _lib.AVL_COST_LETHAL or float(decay_per_m) < 0.0:
        raise ValueError("max_cost must lie in 1 .. %d and decay_per_m may not be negative" % _lib.AVL_COST_LETHAL)
    d = np.sqrt(np.arange(r * r + 1, dtype=np.float64)) * float(resolution)
    beyond = np.maximum(d - float(inscribed_m), 0.0)
    table = np.maximum(1.0, np.round(float(max_cost) * np.exp(-float(decay_per_m) * beyond)))
    table[d <= float(inscribed_m)] = float(max_cost)
    table = table.astype(np.uint8)
    table[0] = _lib.AVL_COST_LETHAL
    return table


def cost_window(map, origin, size, class_cost, unknown_cost=-1, radius_cells=0, inflation=None, filter=True, thresholds=None,
                priority=None, car=None, order="xy", out=None, d2_out=None, stream=None):
    """The cost map of the window of `size` = (h, w) cells whose first cell is grid cell `origin` = (x0, y0), an int8 CUDA tensor
    (avl_cost_map, include/avl_hip.h): every cell's class by render_window's rule (`filter`, `thresholds`, `priority`), its cost
    ``class_cost[class]`` (``unknown_cost`` for an empty cell and off the grid; 0 .. 100 or -1 = no information, 100 lethal), 0 under
    `car` = car_block(...), then for every cell within `radius_cells` of a lethal one ``inflation[d2]`` (inflation_table; d2 the
    squared distance in cells) where that is higher; a cell without information takes it where it is above 0.  order "xy" gives
    [h, w], the live map's; "yx" gives [w, h], nav_msgs/OccupancyGrid's row-major data with x fastest.  `d2_out`: True, or a uint16
    tensor of the result's shape, also returns the squared clearance (65535 = none within the radius): -> (cost, d2).  `map` is a
    CUDA tensor or a NumPy array (uploaded); the result stays on the device.  The grid is only read."""
    t, _, dt = _prep(map)
    hm, wm, c = t.shape
    h, w, r = int(size[0]), int(size[1]), int(radius_cells)
    if order not in ("xy", "yx"):
        raise ValueError("order must be 'xy' ([h, w]) or 'yx' ([w, h]), not %r" % (order,))
    if len(class_cost) != c:
        raise ValueError("%d class costs for a map of %d channels" % (len(class_cost), c))
    if not 0 <= r <= _lib.AVL_COST_MAX_RADIUS:
        raise ValueError("radius_cells = %d: 0 .. %d" % (r, _lib.AVL_COST_MAX_RADIUS))
    if inflation is None:
        if r:
            raise ValueError("radius_cells = %d needs an inflation table (inflation_table)" % r)
        inflation = [_lib.AVL_COST_LETHAL]
    infl = np.ascontiguousarray(np.asarray(inflation), dtype=np.uint8)
    if infl.shape != (r * r + 1,):
        raise ValueError("the inflation table of radius %d has %d entries, not %s" % (r, r * r + 1, infl.shape))
    costs = [int(v) for v in class_cost] + [int(unknown_cost)]
    if any(v < -128 or v > 127 for v in costs):
        raise ValueError("a cost is -1 or 0 .. 100")
    _, pr, th = render_params(np.zeros((c, 3), dtype=np.uint8), c, thresholds, priority)
    flags = (_lib.AVL_LIVE_FILTER if filter else 0) | (_lib.AVL_LIVE_THRESHOLDS if th is not None else 0)
    car_c = None
    if car is not None:
        if len(car) != _lib.AVL_LIVE_CAR_DOUBLES:
            raise ValueError("car is car_block(...): %d numbers" % _lib.AVL_LIVE_CAR_DOUBLES)
        car_c = (C.c_double * _lib.AVL_LIVE_CAR_DOUBLES)(*[float(v) for v in car])
    shape = (max(h, 0), max(w, 0)) if order == "xy" else (max(w, 0), max(h, 0))
    stride_i, stride_j = (w, 1) if order == "xy" else (1, h)

    def result(given, dtype, name):
        if given is None:
            return torch.empty(shape, dtype=dtype, device=t.device)
        if tuple(given.shape) != shape or given.dtype != dtype or given.device != t.device or not given.is_contiguous():
            raise ValueError("%s must be a contiguous %s %s tensor on %s" % (name, dtype, list(shape), t.device))
        return given

    out = result(out, torch.int8, "out")
    d2 = None if d2_out is None or d2_out is False else result(None if d2_out is True else d2_out, torch.uint16, "d2_out")
    s = _stream(t) if stream is None else C.c_void_p(int(stream))
    need = int(_lib.lib().avl_cost_map_scratch_bytes(h, w, r))
    key = (t.device, int(s.value or 0), need)
    scratch = _cost_scratch.get(key)
    if scratch is None:
        scratch = _cost_scratch[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=t.device)
    _lib.check(_lib.lib().avl_cost_map(C.c_void_p(t.data_ptr()), dt, hm, wm, c, int(origin[0]), int(origin[1]), h, w, flags, pr, th,
                                       (C.c_int8 * (c + 1))(*costs), car_c, r, (C.c_uint8 * infl.size)(*infl.tolist()),
                                       C.c_void_p(out.data_ptr()), stride_i, stride_j, C.c_void_p(d2.data_ptr()) if d2 is not None else None,
                                       C.c_void_p(scratch.data_ptr()), need, s), "avl_cost_map")
    return out if d2 is None else (out, d2)
