"""The logits rule of include/avl_hip.h (struct avl_point_logits, rules 1 - 6) restated in NumPy float32, one rounded operation per
line, and the seeded logits the tests share.  Nothing here is shared with the kernels: the projection comes from
oracle/mapping_oracle.py (through _occlusion_reference.Projection), the interpolation is written out on float32 arrays (NumPy rounds
every float32 operation on its own; nothing is fused) and the arg-max is a loop over the classes with the rule's comparison.

    full_labels(logits, net_h, net_w, min_margin)   uint8 [net_h, net_w]: the label of every pixel, 255 where it abstains
    full_margins(logits, net_h, net_w)              float32 [net_h, net_w]
    point_states(proj, logits, net_h, net_w, min_margin)   (uint8 [n], float32 [n]): what avl_point_labels writes for one view
"""
import numpy as np

ABSTAINED, NONE = 254, 255
F32 = np.float32


def scale(src, dst):
    """rule 3, as avl_seg_eval_full_res computes it on the host: a float32 division"""
    return F32(src - 1) / F32(dst - 1) if dst > 1 else F32(0.0)


def nearest_index(i, src, dst):
    """rule 2: the cv2 INTER_NEAREST source index of pixel i of a dst-sized image in a src-sized one (float64, as fetch_vote)"""
    i = np.asarray(i, dtype=np.int64)
    if src == dst:
        return i
    return np.minimum(np.floor(i.astype(np.float64) * (float(src) / float(dst))).astype(np.int64), src - 1)


def interpolate(logits, net_h, net_w, ny, nx):
    """rules 3 and 4 at the pixels (ny[i], nx[i]) of the net_h x net_w image -> z float32 [n, K]"""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32 and logits.ndim == 3
    h, w, _ = logits.shape
    ny, nx = np.asarray(ny, dtype=np.int64), np.asarray(nx, dtype=np.int64)
    fy = scale(h, net_h) * ny.astype(F32)
    fx = scale(w, net_w) * nx.astype(F32)
    assert fy.dtype == np.float32 and fx.dtype == np.float32
    y0 = np.minimum(fy.astype(np.int32), h - 1)
    x0 = np.minimum(fx.astype(np.int32), w - 1)
    y1 = y0 + (y0 < h - 1)
    x1 = x0 + (x0 < w - 1)
    ly = fy - y0.astype(F32)
    lx = fx - x0.astype(F32)
    hy = F32(1.0) - ly
    hx = F32(1.0) - lx
    ly, lx, hy, hx = ly[:, None], lx[:, None], hy[:, None], hx[:, None]
    a, b, c, d = logits[y0, x0], logits[y0, x1], logits[y1, x0], logits[y1, x1]
    with np.errstate(all="ignore"):
        t0 = hx * a
        t1 = lx * b
        top = t0 + t1
        t2 = hx * c
        t3 = lx * d
        bot = t2 + t3
        u0 = hy * top
        u1 = ly * bot
        z = u0 + u1
    assert z.dtype == np.float32
    return z


def top_and_margin(z):
    """rule 5 -> (top int64 [n], margin float32 [n])"""
    n, K = z.shape
    best, top = z[:, 0].copy(), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(1, K):
            v = z[:, k]
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
            best = np.where(take, v, best)
            top = np.where(take, k, top)
        if K == 1:
            return top, np.full(n, np.inf, dtype=np.float32)
        others = z.copy()
        others[np.arange(n), top] = -np.inf                  # a NaN among the others means a NaN at the top: the margin is NaN either way
        second = np.fmax.reduce(others, axis=1)
        margin = best - second
    assert margin.dtype == np.float32
    return top, margin


def rule(logits, net_h, net_w, ny, nx, min_margin):
    """rules 3 - 6 at the pixels (ny[i], nx[i]) -> (label uint8 [n]: top, or ABSTAINED; margin float32 [n])"""
    top, margin = top_and_margin(interpolate(logits, net_h, net_w, ny, nx))
    with np.errstate(invalid="ignore"):
        abstains = margin < F32(min_margin)
    return np.where(abstains, ABSTAINED, top).astype(np.uint8), margin


def _all_pixels(net_h, net_w):
    ny, nx = np.divmod(np.arange(net_h * net_w, dtype=np.int64), net_w)
    return ny, nx


def full_margins(logits, net_h, net_w):
    ny, nx = _all_pixels(net_h, net_w)
    return top_and_margin(interpolate(logits, net_h, net_w, ny, nx))[1].reshape(net_h, net_w)


def full_labels(logits, net_h, net_w, min_margin):
    """the label map the class-map source has to be fed for the same grid: 255 (which votes nothing) where the pixel abstains"""
    ny, nx = _all_pixels(net_h, net_w)
    label, _ = rule(logits, net_h, net_w, ny, nx, min_margin)
    return np.where(label == ABSTAINED, NONE, label).astype(np.uint8).reshape(net_h, net_w)


def point_pixels(proj, net_h, net_w):
    """rule 2 for the candidates of a Projection -> (ny, nx), 0 where the point is no candidate"""
    ny = nearest_index(np.where(proj.cand, proj.iy, 0), net_h, proj.img_h)
    nx = nearest_index(np.where(proj.cand, proj.ix, 0), net_w, proj.img_w)
    return ny, nx


def point_states(proj, logits, net_h, net_w, min_margin):
    """avl_point_labels for one view: state uint8 [n] (top, 254 abstained, 255 no candidate), margin float32 [n] (0 for 255)"""
    ny, nx = point_pixels(proj, net_h, net_w)
    label, margin = rule(logits, net_h, net_w, ny, nx, min_margin)
    return np.where(proj.cand, label, NONE).astype(np.uint8), np.where(proj.cand, margin, F32(0.0)).astype(np.float32)


def near_tie_bound(logits, net_h, net_w, ny, nx):
    """16 * 2^-24 * max|corner logit| per pixel: four roundings per interpolated value (each at most 2^-24 relative to a magnitude
    bounded by the largest corner, the weights being in [0, 1]) and two values in a comparison bound the difference of two evaluations
    of the same margin by 2 * 2 * 4 * 2^-24 * max|corner|"""
    logits = np.asarray(logits, dtype=np.float32)
    h, w, _ = logits.shape
    fy = scale(h, net_h) * np.asarray(ny).astype(F32)
    fx = scale(w, net_w) * np.asarray(nx).astype(F32)
    y0, x0 = np.minimum(fy.astype(np.int32), h - 1), np.minimum(fx.astype(np.int32), w - 1)
    y1, x1 = y0 + (y0 < h - 1), x0 + (x0 < w - 1)
    peak = np.abs(np.stack([logits[y0, x0], logits[y0, x1], logits[y1, x0], logits[y1, x1]])).max(axis=(0, 2))
    return 16.0 * 2.0 ** -24 * peak.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- inputs
# (logits h', w') -> (net_h, net_w) with the projection images (img_h, img_w) the tests use for it
SHAPES = {"9x13_to_33x50": ((9, 13), (33, 50), [(33, 50), (66, 100)]),
          "1x7_to_5x29": ((1, 7), (5, 29), [(5, 29)]),
          "9x13_same": ((9, 13), (9, 13), [(9, 13)])}
KS = [2, 5, 19, 33]
MAP_CLASSES = [2, 1, 8, 10, 3]             # the network classes PALETTE_19 maps onto the five map classes


def make_logits(seed, h, w, K, kind="normal", ld=None, favour=0.0):
    """float32 [h, w, K]: "normal" = standard normal draws; "quantised" = the same rounded to multiples of 0.25, so that exact ties
    occur between classes and between pixels.  `ld` > K: the array is a view of the first K columns of an [h, w, ld] array whose other
    columns hold large values (a kernel that read them would see them win).  `favour` is added to MAP_CLASSES (those below K)."""
    rng = np.random.default_rng(seed)
    ld = K if ld is None else ld
    full = np.full((h, w, ld), 1000.0, dtype=np.float32)
    z = rng.standard_normal((h, w, K)).astype(np.float32)
    if kind == "quantised":
        z = (np.round(z * 4.0) / 4.0).astype(np.float32)
    else:
        assert kind == "normal"
    for k in MAP_CLASSES:
        if k < K:
            z[:, :, k] += np.float32(favour)
    full[:, :, :K] = z
    return full[:, :, :K]
