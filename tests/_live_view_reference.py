"""NumPy restatement of the heading-up live view (avl_live_view, include/avl_hip.h), and the grid and the cases that
tests/test_gpu_live_view.py runs and tests/test_live_view_cpu.py examines.  TEST INFRASTRUCTURE ONLY (CPU).

The view samples the whole-grid live picture B of _live_map_reference.compose through a 2 x 3 float64 matrix from output pixel
centres to continuous grid coordinates; the float64 operations are written in the order the header states.  `sample` and
`car_mask_view` take switches that state the definition WRONGLY on purpose (truncation, pixel corners, cell centres): the CPU tests
use them to show that the cases tell right from wrong."""
import collections

import numpy as np

import _live_map_reference as lr


def view_matrix(centre_cells, heading, cells_per_pixel, size, anchor=(0.5, 0.5)):
    """Heading-up: one pixel down the picture moves k cells against the heading (c, s); one pixel to the right moves k cells to the
    vehicle's right seen from above, (s, -c); pixel centre (anchor * size) shows `centre_cells`."""
    k, (c, s), (h, w) = np.float64(cells_per_pixel), (np.float64(heading[0]), np.float64(heading[1])), size
    down, right = np.array([-(k * c), -(k * s)]), np.array([k * s, -(k * c)])
    ai, aj = np.float64(anchor[0]) * h, np.float64(anchor[1]) * w
    m = np.empty((2, 3), dtype=np.float64)
    m[:, 0], m[:, 1] = down, right
    m[:, 2] = (np.array(centre_cells, dtype=np.float64) - down * ai) - right * aj
    return m


def mirrored(m, size):
    """the matrix of the opposite handedness: right and left exchanged about the picture's vertical centre line"""
    out = np.array(m, dtype=np.float64)
    out[:, 1] = -out[:, 1]
    out[:, 2] = m[:, 2] + m[:, 1] * float(size[1])
    return out


def coordinates(m, size, offset=0.5):
    """gx, gy [h, w] float64 of every output pixel; offset 0.5 = pixel centres (the definition)"""
    m = np.asarray(m, dtype=np.float64)
    a = (np.arange(size[0], dtype=np.float64) + offset)[:, None]
    b = (np.arange(size[1], dtype=np.float64) + offset)[None, :]
    return (m[0, 0] * a + m[0, 1] * b) + m[0, 2], (m[1, 0] * a + m[1, 1] * b) + m[1, 2]


def cells(m, size, grid_shape, offset=0.5, truncate=False):
    """-> inside [h, w] bool, fx, fy [h, w] int64 (0 where outside).  The definition: the range is tested on the doubles, then
    floor.  truncate=True is the wrong version: conversion towards zero first, range test on the integers."""
    gx, gy = coordinates(m, size, offset)
    hm, wm = grid_shape
    if truncate:
        with np.errstate(invalid="ignore"):
            fx, fy = np.trunc(gx), np.trunc(gy)
        inside = (fx >= 0) & (fx < hm) & (fy >= 0) & (fy < wm)
    else:
        inside = (0.0 <= gx) & (gx < float(hm)) & (0.0 <= gy) & (gy < float(wm))
        fx, fy = np.floor(gx), np.floor(gy)
    fx = np.where(inside, fx, 0.0).astype(np.int64)
    fy = np.where(inside, fy, 0.0).astype(np.int64)
    return inside, fx, fy


def sample(b, m, size, offset=0.5, truncate=False):
    """out[i, j] = b[floor(gx), floor(gy)] inside the grid, black outside"""
    b = np.asarray(b)
    inside, fx, fy = cells(m, size, b.shape[:2], offset, truncate)
    out = np.zeros((size[0], size[1], 3), dtype=np.uint8)
    out[inside] = b[fx[inside], fy[inside]]
    return out


def car_mask_view(m, size, car, offset=0.5, cell_centres=False):
    """pixels whose continuous grid coordinates lie in the car's rectangle (float64, the kernel's operation order).
    cell_centres=True is the wrong version: the sampled cell's centre instead."""
    cx, cy, c, s, u_lo, u_hi, v_lo, v_hi = [np.float64(v) for v in car]
    gx, gy = coordinates(m, size, offset)
    if cell_centres:
        gx, gy = np.floor(gx) + 0.5, np.floor(gy) + 0.5
    dx, dy = gx - cx, gy - cy
    u = c * dx + s * dy
    v = c * dy - s * dx
    return (u_lo <= u) & (u < u_hi) & (v_lo <= v) & (v < v_hi)


def compose_view(rendered, m, size, fill=False, label_colors=None, fill_priority=lr.REF_PRIORITY, car=None, car_color=(255, 0, 0),
                 offset=0.5, truncate=False, cell_centres=False):
    """The view from `rendered` = the renderer's output for the WHOLE grid: the whole-grid live picture (fill_black in the grid's
    frame with its black ring), sampled through m, then the car."""
    rendered = np.asarray(rendered)
    b = lr.compose(rendered, (0, 0), rendered.shape[:2], fill, label_colors, fill_priority)
    out = sample(b, m, size, offset, truncate)
    if car is not None:
        out[car_mask_view(m, size, car, offset, cell_centres)] = car_color
    return out


# ------------------------------------------------------------------------------------------------ the grid and the cases
HM, WM = 96, 120
SIZE = (77, 83)                      # two tiles at least and a ragged last one both ways, for 16 x 64, 32 x 32 and 64 x 16 tiles
CAR_RES = 0.25                       # 4.0 m x 1.8 m = 16 x 7.2 cells
CAR_OFFSET = (-0.35, 0.35)           # the car's reference point, in cells from the point the anchor pixel shows: a fraction of a cell,
#                                      so that at the headings along an axis its edges pass between a pixel's centre and its cell's
CENTRE = (48.3, 60.6)                # the vehicle in the middle of the grid
CORNER = (9.3, 11.6)                 # ... and near the grid's first corner
MAX_SPAN = 2.875                     # AVL_LIVE_VIEW_MAX_SPAN
HEADINGS = collections.OrderedDict([(0.0, (1.0, 0.0)), (90.0, (0.0, 1.0)), (180.0, (-1.0, 0.0))] +
                                   [(d, (float(np.cos(np.deg2rad(d))), float(np.sin(np.deg2rad(d))))) for d in (30.0, 45.0, 201.7)])
SCALES = (0.5, 1.0, 1.7)


def colors(c):
    return lr.REF_COLORS.tolist() if c == 5 else [[(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256] for i in range(c)]


def fill_priority(c):
    return list(lr.REF_PRIORITY) if c == 5 else [(2 * k + 1) % c for k in range(c)]


def render_priority(c):
    return [(3 * k + 1) % c for k in range(c)] if c % 3 else list(range(1, c)) + [0]


def thresholds(c):
    return [0.01, 1.0 / 3.0, 0.5, 0.01, 0.25][:c]


def make_grid(c, dtype):
    """96 x 120 x c: about 30 % of the cells hold log-odds-like values, thin structured stripes (a diagonal, a row, a column), cells
    on the grid's outer ring, one exact tie and one NaN cell"""
    rng = np.random.default_rng(4200 + c)
    m = np.zeros((HM, WM, c), dtype=dtype)
    filled = rng.random((HM, WM)) < 0.30
    vals = (rng.normal(size=(HM, WM, c)) * 4) * (rng.random((HM, WM, c)) < 0.6)
    m[filled] = vals[filled].astype(dtype)
    one = np.eye(c, dtype=dtype)
    for t in range(70):
        m[10 + t, 25 + t] = 6 * one[2 % c]                   # a lane-like diagonal, one cell wide
    m[50, 20:100] = 5 * one[1 % c]
    m[15:85, 70] = 7 * one[2 % c]
    m[0, 10:60] = 3 * one[0]                                 # the ring that fill_black blackens
    m[HM - 1, 30:110] = 3 * one[1 % c]
    m[20:70, 0] = 4 * one[0]
    m[5:90, WM - 1] = 4 * one[2 % c]
    m[30, 40] = 0
    m[30, 40, :2] = 2.0                                      # an exact tie (c >= 2): the first maximum wins
    m[20, 25, 0] = np.nan
    m.setflags(write=False)
    return m


def translation(x0, y0):
    return np.array([[1.0, 0.0, float(x0)], [0.0, 1.0, float(y0)]])


def _case(name, m, c=5, dtype=np.float64, filt=True, thr=False, fill=True, car=None, heading=None, **geometry):
    return dict(name=name, m=m, c=c, dtype=dtype, filt=filt, thr=thr, fill=fill, car=car, heading=heading, geometry=geometry)


def heading_case(deg, k, c=5, dtype=np.float64, filt=True, thr=False, fill=None, car=True, name=None):
    """the view of SIZE pixels at k cells per pixel, the vehicle (heading `deg`) in the middle of the grid and of the picture -- at
    k = 0.5 near the grid's first corner and at 0.8 of the height, so that the view crosses the grid's negative side; there the
    fill is off by default: its black ring would hide which cell a pixel just off the grid was given"""
    heading = HEADINGS[deg]
    fill = (k != 0.5) if fill is None else fill
    centre, anchor = (CORNER, (0.8, 0.5)) if k == 0.5 else (CENTRE, (0.5, 0.5))
    m = view_matrix(centre, heading, k, SIZE, anchor)
    block = lr.car_block(centre[0] + CAR_OFFSET[0], centre[1] + CAR_OFFSET[1], heading[0], heading[1], CAR_RES) if car else None
    return _case(name or "heading %g k %g" % (deg, k), m, c, dtype, filt, thr, fill, block, heading, centre=centre, k=k, anchor=anchor)


def identity_case(dtype):
    """a pure translation by whole cells: avl_live_map's window at (-4, 45), which leaves the grid on two sides"""
    car = lr.car_block(30.3, 80.6, float(np.cos(0.7)), float(np.sin(0.7)), CAR_RES)
    return _case("identity %s" % np.dtype(dtype).name, translation(-4, 45), dtype=dtype, car=car, origin=(-4, 45))


def largest_case():
    """a rotation by 45 degrees whose |M00| + |M01| = |M10| + |M11| = MAX_SPAN exactly (2.0329... cells per pixel)"""
    a = MAX_SPAN / 2.0
    m = np.array([[-a, a, 0.0], [-a, -a, 0.0]])
    ai, aj = 0.5 * SIZE[0], 0.5 * SIZE[1]
    m[:, 2] = (np.array(CENTRE) - m[:, 0] * ai) - m[:, 1] * aj
    r = float(np.sqrt(0.5))
    return _case("largest admitted matrix", m, car=lr.car_block(CENTRE[0] + CAR_OFFSET[0], CENTRE[1] + CAR_OFFSET[1], r, r, CAR_RES),
                 heading=(r, r))


def cross_cases(deg):
    return [heading_case(deg, 1.0, filt=filt, thr=thr, fill=fill, car=car,
                         name="heading %g k 1 filter %d thresholds %d fill %d car %d" % (deg, filt, thr, fill, car))
            for filt in (False, True) for thr in (False, True) for fill in (False, True) for car in (False, True)]


def gpu_cases():
    """every picture tests/test_gpu_live_view.py compares, but the two that go through SemanticMapping"""
    cases = [identity_case(np.float64), identity_case(np.float32)]
    cases += [heading_case(deg, k) for deg in HEADINGS for k in SCALES]
    cases += cross_cases(30.0) + cross_cases(45.0)
    cases += [heading_case(30.0, 1.0, dtype=np.float32, name="heading 30 k 1 float32"),
              heading_case(30.0, 1.0, c=3, name="heading 30 k 1 C 3"), largest_case()]
    return cases


def case_kwargs(case):
    """the arguments of compose_view / renderer.render_view that a case fixes, but for the rendered grid or the map"""
    c = case["c"]
    return dict(fill=case["fill"], fill_priority=fill_priority(c), car=case["car"])
