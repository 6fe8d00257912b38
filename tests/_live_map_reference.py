"""NumPy restatements for the live-map tests.  TEST INFRASTRUCTURE ONLY (CPU).

fill_black restates src/renderer.py:62-105 (fill_black + resume_color) for any colour table and priority list; with the reference's
own it is pinned byte for byte by tests/golden/fill_black.npz, which tools/gen_golden_live_map.py writes by running the reference's
renderer.py.  fill_edge restates :192-196.  The rest states what avl_live_map is defined to give (include/avl_hip.h): the window's
geometry, the crop of a rendered grid with fill_black put back into the grid's frame, and the ego car's pixel test in float64 with the
kernel's operation order."""
import numpy as np

REF_COLORS = np.array([[128, 64, 128], [140, 140, 200], [255, 255, 255], [107, 142, 35], [244, 35, 232]])   # renderer.py:19-25
REF_PRIORITY = (0, 3, 4, 2, 1)                                                                               # renderer.py:67
PCD_ORIGIN_OFFSET = (1369.0496826171875, 562.84814453125)                                                    # mapping.py:404


def fill_black(img, label_colors=REF_COLORS, priority_list=REF_PRIORITY):
    """renderer.py:62-98 + resume_color: matching on the R channel only, every interior pixel rewritten."""
    label_colors = np.asarray(label_colors)
    xmax, ymax = img.shape[0], img.shape[1]
    r = img[:, :, 0]
    stacked = np.stack([r[1 + dx:xmax - 1 + dx, 1 + dy:ymax - 1 + dy] for dx in (-1, 0, 1) for dy in (-1, 0, 1)])   # :71-79
    out_r = np.zeros((xmax - 2, ymax - 2), dtype=np.uint8)
    for label in priority_list:                                                                                  # :88-89
        out_r[np.any(stacked == label_colors[label, 0], axis=0)] = label_colors[label, 0]
    out = np.repeat(out_r[:, :, None], 3, axis=2)                                                                # :93-95
    for i in range(len(label_colors)):                                                                           # resume_color :101-105
        out[out[:, :, 0] == label_colors[i, 0]] = label_colors[i]
    return out


def fill_edge(color_map):
    """renderer.py:192-196"""
    color_map[[0, -1], :, :] = 250
    color_map[:, [0, -1], :] = 250
    color_map[0:5, 0:5] = 254
    return color_map


def window_of(pose7, boundary, resolution, size_cells):
    """-> (x0, y0), (cx, cy): centre cell = trunc((pose.xy + offset - boundary minimum) / resolution) (mapping.py:404-409),
    first cell = centre - size // 2; (cx, cy) is the same quotient before truncation."""
    xy = np.asarray(pose7, dtype=np.float64)[:2]
    cxy = (xy + np.array(PCD_ORIGIN_OFFSET) - np.array([boundary[0][0], boundary[1][0]], dtype=np.float64)) / resolution
    centre = cxy.astype(np.int32)
    return (int(centre[0]) - int(size_cells[0]) // 2, int(centre[1]) - int(size_cells[1]) // 2), (float(cxy[0]), float(cxy[1]))


def heading(pose7):
    """(cos yaw, sin yaw): first column of the quaternion's rotation matrix (tf.transformations.quaternion_matrix), projected on
    the x, y plane and normalised."""
    q = np.array(pose7[3:7], dtype=np.float64)
    q *= np.sqrt(2.0 / np.dot(q, q))
    q = np.outer(q, q)
    c, s = 1.0 - q[1, 1] - q[2, 2], q[0, 1] + q[2, 3]
    n = np.hypot(c, s)
    return float(c / n), float(s / n)


def car_block(cx, cy, c, s, resolution, size=(4.0, 1.8)):
    """mapping.py:502-511: length 4.0 m, width 1.8 m, reference point a quarter length from the rear; in cells"""
    length, width = size
    return (cx, cy, c, s, -length / (4.0 * resolution), 3.0 * length / (4.0 * resolution), -width / (2.0 * resolution),
            width / (2.0 * resolution))


def car_mask(origin, size, car):
    """window pixels whose cell centre lies in the car's rectangle; float64, the kernel's operation order"""
    cx, cy, c, s, u_lo, u_hi, v_lo, v_hi = [np.float64(v) for v in car]
    gx = (np.arange(size[0], dtype=np.int64) + origin[0]).astype(np.float64)[:, None]
    gy = (np.arange(size[1], dtype=np.int64) + origin[1]).astype(np.float64)[None, :]
    dx = (gx + 0.5) - cx
    dy = (gy + 0.5) - cy
    u = c * dx + s * dy
    v = c * dy - s * dx
    return (u_lo <= u) & (u < u_hi) & (v_lo <= v) & (v < v_hi)


def compose(rendered, origin, size, fill=False, label_colors=None, fill_priority=REF_PRIORITY, car=None, car_color=(255, 0, 0)):
    """The live map from `rendered` = the renderer's output for the WHOLE grid, uint8 [Hm, Wm, 3]: fill_black put back into the grid's
    frame with a one-cell black ring, the crop (black outside the grid), then the car."""
    rendered = np.asarray(rendered)
    hm, wm = rendered.shape[:2]
    b = rendered
    if fill:
        b = np.zeros_like(rendered)
        b[1:hm - 1, 1:wm - 1] = fill_black(rendered, label_colors, fill_priority)
    h, w = size
    out = np.zeros((h, w, 3), dtype=np.uint8)
    x0, y0 = origin
    i0, i1 = max(0, -x0), min(h, hm - x0)
    j0, j1 = max(0, -y0), min(w, wm - y0)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = b[x0 + i0:x0 + i1, y0 + j0:y0 + j1]
    if car is not None:
        out[car_mask(origin, size, car)] = car_color
    return out
