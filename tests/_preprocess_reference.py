"""Float64 reference and inputs for the camera pre-processing tests (tests/test_preprocess_reference_cpu.py without a GPU,
tests/test_gpu_preprocess_edges.py with one).  NumPy only.

* exact_undistort: cv2.undistort's plumb-bob remap (the model of csrc/seg_preprocess.h) evaluated in float64 from the double K / dist with
  no float32 step, the REAL-VALUED bilinear sample per pixel and channel, zeros outside.
* bar: what a byte may differ from that by -- half a grey level for the rounding plus `delta` for the kernel's float32 steps.
* model_undistort: the same chain with one step replaced (float32 parameters and map, k3 dropped, p1 and p2 swapped, 5-bit weights, a cast
  for floorf): the CPU test shows with it that the inputs below tell every such kernel from the right one.
* frames and cameras: full-range uint8 noise (a block frame hides weight errors), 67 x 83 after pre-processing at every factor, and three
  synthetic cameras with k3 != 0 whose zero border is reached on all four sides.
* area_axis_table / reduce_axis / resize_area_with: computeResizeAreaTab for one axis as arrays, for any scale expression, and the
  float32 reduction along an axis with it (oracle/preprocess_oracle.resize_area's loops, every destination at once)."""
import numpy as np

NET_H, NET_W = 67, 83
# factor -> raw frame (rows, columns); every factor > 1 leaves remainder rows and columns, and all of them pre-process to 67 x 83
RAW = {1: (67, 83), 2: (135, 167), 3: (203, 251), 4: (271, 335)}

# (fx, fy, cx, cy), (k1, k2, p1, p2, k3) at 67 x 83
CAMERAS = {
    # k1 > 0, k2 < 0, k3 != 0, both tangential terms nonzero
    "pincushion": ((70.0, 66.0, 44.3, 30.6), (0.35, -0.12, 0.02, -0.015, 0.05)),
    # the signs reversed
    "barrel": ((70.0, 66.0, 44.3, 30.6), (-0.3, 0.1, -0.01, 0.02, -0.02)),
    # the principal point left of the frame
    "offcentre": ((90.0, 85.0, -5.5, 41.2), (0.08, 0.02, -0.03, 0.03, 0.01)),
}


class Cam(object):
    """what preprocess_device and set_camera read of a camera: K (3 x 3) and dist (k1 k2 p1 p2 k3), both float64"""

    def __init__(self, K, dist):
        self.K, self.dist = np.asarray(K, dtype=np.float64), np.asarray(dist, dtype=np.float64)

    def scaled(self, sx, sy):
        """as Camera.scaled: K's rows scaled"""
        K = self.K.copy()
        K[0] *= sx
        K[1] *= sy
        return Cam(K, self.dist)

    def with_dist(self, **kw):
        d = dict(zip(("k1", "k2", "p1", "p2", "k3"), self.dist.tolist()))
        d.update(kw)
        return Cam(self.K, [d[k] for k in ("k1", "k2", "p1", "p2", "k3")])


def camera(name, factor=1, size=None):
    """the synthetic camera `name` (None: no undistortion) for the raw frame of `factor`, or for a frame of size = (rows, columns)"""
    if name is None:
        return None
    (fx, fy, cx, cy), dist = CAMERAS[name]
    cam = Cam([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dist)
    h, w = RAW[factor] if size is None else size
    return cam if (h, w) == (NET_H, NET_W) else cam.scaled(w / float(NET_W), h / float(NET_H))


def noise_frame(factor, seed=0):
    """uint8 BGR noise over the full range at the raw size of `factor`"""
    h, w = RAW[factor]
    return np.random.default_rng(1000 * factor + seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def source_coords(h, w, K, dist, f32_params=False, f32_map=False):
    """(sx, sy): where destination pixel (u, v) samples the source, float64 [h, w] each.  f32_params: K / dist rounded to float32 first
    (make_pre_camera); f32_map: the result rounded to float32 (cv2's map type, the kernel's sx / sy)."""
    K, dist = np.asarray(K, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    if f32_params:
        K, dist = K.astype(np.float32).astype(np.float64), dist.astype(np.float32).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3 = dist[:5]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    radial = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    sx, sy = fx * xd + cx, fy * yd + cy
    if f32_map:
        sx, sy = sx.astype(np.float32).astype(np.float64), sy.astype(np.float32).astype(np.float64)
    return sx, sy


def taps(sx, sy, cast=False):
    """(x0, y0) of the bilinear sample's first tap: floor, or with cast=True C's (int) conversion, which rounds towards zero"""
    if cast:
        return np.trunc(sx).astype(np.int64), np.trunc(sy).astype(np.int64)
    return np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)


def bilinear(img, sx, sy, weight_bits=None, cast=False):
    """real-valued bilinear sample of img [h, w, c] at (sx, sy), zeros outside, float64.  weight_bits = n: the fractions rounded to
    n bits first (cv2.remap's INTER_BITS = 5)."""
    h, w = img.shape[:2]
    x0, y0 = taps(sx, sy, cast)
    ax, ay = sx - x0, sy - y0
    if weight_bits is not None:
        q = float(1 << weight_bits)
        ax, ay = np.rint(ax * q) / q, np.rint(ay * q) / q
    out = np.zeros(sx.shape + (img.shape[2],), dtype=np.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            wgt = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            px = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float64)
            out += (wgt * ok)[..., None] * px
    return out


def exact_undistort(rgb, K, dist):
    """-> (E, sx, sy): E float64 [h, w, 3], the real-valued bilinear sample of the RGB frame at the plumb-bob source position of every
    pixel, zeros outside; everything in float64 from the double K / dist.  sx, sy: those positions."""
    sx, sy = source_coords(rgb.shape[0], rgb.shape[1], K, dist)
    return bilinear(rgb, sx, sy), sx, sy


def model_undistort(rgb, K, dist, f32=False, weight_bits=None, cast=False):
    """the real-valued result of a kernel that differs from exact_undistort in the named step; f32: float32 camera parameters and a
    float32 map, which is the kernel as it is written (double polynomial in between)"""
    sx, sy = source_coords(rgb.shape[0], rgb.shape[1], K, dist, f32_params=f32, f32_map=f32)
    return bilinear(rgb, sx, sy, weight_bits=weight_bits, cast=cast)


def to_bytes(real):
    return np.clip(np.rint(real), 0, 255).astype(np.uint8)


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def bar(sx, sy):
    """|byte - E| <= 0.5 + delta on every pixel and channel.  delta = 255 (ulp32(max|sx|) + ulp32(max|sy|)) + 255 * 16 * 2^-24: a float32
    map and float32 camera parameters move the sample point by about an ulp of the coordinate per axis, and one grey level per pixel of
    movement is at most 255; the four float32 multiply-adds of the sample itself carry 2^-24 relative each, with room to spare."""
    delta = 255.0 * (ulp32(np.abs(sx).max()) + ulp32(np.abs(sy).max())) + 255.0 * 16.0 * 2.0 ** -24
    return 0.5 + delta


def excess(got, E):
    """max|got - E| - 0.5: what of the bar's delta the bytes `got` use"""
    return float(np.abs(got.astype(np.float64) - E).max()) - 0.5


def outside_share(sx, sy, h, w):
    """share of the pixels whose four taps all lie outside the frame"""
    x0, y0 = taps(sx, sy)
    return float(((x0 < -1) | (x0 >= w) | (y0 < -1) | (y0 >= h)).mean())


def half_outside_counts(sx, sy, h, w):
    """pixels with one tap column (row) outside and the other inside, the other axis reaching the frame: {side: count}"""
    x0, y0 = taps(sx, sy)
    y_in, x_in = (y0 >= -1) & (y0 < h), (x0 >= -1) & (x0 < w)
    return {"left": int(((x0 == -1) & y_in).sum()), "right": int(((x0 == w - 1) & y_in).sum()),
            "top": int(((y0 == -1) & x_in).sum()), "bottom": int(((y0 == h - 1) & x_in).sum())}


# ------------------------------------------------------------------------------------------------ INTER_AREA, one axis
def scale_plain(ssize, dsize):
    """the kernel's and the restatement's expression"""
    return ssize / float(dsize)


def scale_opencv(ssize, dsize):
    """OpenCV's: scale_x = 1. / inv_scale_x with inv_scale_x = (double)dsize.width / ssize.width"""
    return 1.0 / (float(dsize) / ssize)


def area_axis_table(dsize, ssize, scale):
    """computeResizeAreaTab for one axis as arrays over the destination index (csrc/seg_conv.hip's area_axis, for every d at once):
    (s1, s2, w_first, w_mid, w_last), a weight of 0 = no such entry.  The source span of d is [s1 - (w_first > 0), s2 + (w_last > 0))."""
    d = np.arange(dsize, dtype=np.float64)
    f1 = d * scale
    f2 = f1 + scale
    cell = np.minimum(scale, ssize - f1)
    s1, s2 = np.ceil(f1).astype(np.int64), np.floor(f2).astype(np.int64)
    s2 = np.minimum(s2, ssize - 1)
    s1 = np.minimum(s1, s2)
    w_first = np.where(s1 - f1 > 1e-3, ((s1 - f1) / cell).astype(np.float32), np.float32(0))
    w_mid = (1.0 / cell).astype(np.float32)
    w_last = np.where(f2 - s2 > 1e-3, (np.minimum(np.minimum(f2 - s2, 1.0), cell) / cell).astype(np.float32), np.float32(0))
    return s1, s2, w_first.astype(np.float32), w_mid, w_last.astype(np.float32)


def table_entries(tab):
    """the arrays of area_axis_table as oracle/preprocess_oracle._area_table's list of [(source index, weight)]"""
    s1, s2, w_first, w_mid, w_last = tab
    out = []
    for d in range(len(s1)):
        ent = []
        if w_first[d] > 0:
            ent.append((int(s1[d]) - 1, w_first[d]))
        ent += [(s, w_mid[d]) for s in range(int(s1[d]), int(s2[d]))]
        if w_last[d] > 0:
            ent.append((int(s2[d]), w_last[d]))
        out.append(ent)
    return out


def reduce_axis(src, tab):
    """float32 [..., ssize] reduced along its last axis with the table -> float32 [..., dsize]: value x weight added in table order in
    float32, multiply then add (no FMA), as oracle/preprocess_oracle.resize_area does it.  Every destination at once, one step per entry."""
    s1, s2, w_first, w_mid, w_last = tab
    src = np.asarray(src, dtype=np.float32)
    start, end = s1 - (w_first > 0), s2 + (w_last > 0)
    buf = np.zeros(src.shape[:-1] + (len(s1),), dtype=np.float32)
    for j in range(int((end - start).max())):
        pos = start + j
        w = np.where(pos < s1, w_first, np.where(pos < s2, w_mid, w_last)).astype(np.float32)
        term = (src[..., np.minimum(pos, src.shape[-1] - 1)] * w).astype(np.float32)
        buf = np.where(pos < end, (buf + term).astype(np.float32), buf)
    return buf


def reduce_row(row, tab):
    """one uint8 row [ssize] -> uint8 [dsize], rounded half to even"""
    return np.clip(np.rint(reduce_axis(row, tab)), 0, 255).astype(np.uint8)


def resize_area_with(img, out_h, out_w, scale_of):
    """oracle/preprocess_oracle.resize_area with the scale expression scale_of(ssize, dsize): rows reduced along x, then across rows"""
    h, w = img.shape[:2]
    xt, yt = area_axis_table(out_w, w, scale_of(w, out_w)), area_axis_table(out_h, h, scale_of(h, out_h))
    rows = reduce_axis(img.astype(np.float32).transpose(0, 2, 1), xt)          # [h, c, out_w]
    out = reduce_axis(rows.transpose(1, 2, 0), yt)                              # [c, out_w, out_h]
    return np.ascontiguousarray(np.clip(np.rint(out), 0, 255).astype(np.uint8).transpose(2, 1, 0))
