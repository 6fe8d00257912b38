// LiDAR -> image -> BEV grid kernels (gfx950).  Compiled with -ffp-contract=off: the float64
// arithmetic below has to round exactly where the reference's NumPy does, so every fused
// multiply-add is written out.
//
// Reference arithmetic (src/mapping.py):
//   :371  Xv  = T @ [x y z 1]^T            (np.matmul -> OpenBLAS dgemm, K = 4: p0*x0 then an FMA chain)
//   :375  IXY = ((P @ Xv)[0:2] / (P @ Xv)[2]).astype(int32)
//   :378  0 < Xv.x < RANGE_MAX             :381-383 0 <= IX < W, 0 <= IY < H
//   :405-411 cell = (((x,y) + offset) - (b00,b10)) / res -> astype(int32), on-grid test
//   :419-437 per class: R,G colour match, buffered += of CM[:, i] (once per cell), lane bonus
//
// Kernels are HBM/latency bound integer + f64 work: one point per lane, coalesced 16 B (f32 AoS)
// or 8 B (f64 SoA) loads, a label gather served by L2, and an idempotent atomicOr per point.
#include "avl_common.h"
#include "avl_render.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace {

constexpr int kBlock = 256;

struct ProjParams {
    double P[12];
    double T[16];
    int has_T;
    double range_max;
    int img_w, img_h;
};

struct PtsView {
    const char* base;
    int n;
    int dtype;
    long long point_stride, comp_stride;
    int aos_f32;  // 1: float4-per-point fast path (16-byte aligned, comp_stride 4, point_stride 16)
};

struct GridParams {
    double off_x, off_y, b00, b10, resolution;
    int Hm, Wm, C;
    unsigned bonus_classes;
    unsigned char colors[AVL_MAX_MAP_CLASSES * 3];
};

struct CmParams {
    double cm[AVL_MAX_MAP_CLASSES * AVL_MAX_MAP_CLASSES];  // row-major [C][C]
};

struct LutParams {
    unsigned lut[256];
};

// avl_occlusion in kernel-argument form
struct OcclParams {
    unsigned* depth;     // [n_views][Hc][Wc]: bit pattern of the nearest candidate's float32 depth, 0xFFFFFFFF = empty cell
    int* culled;         // [n_views] culled candidates, or NULL
    double k, abs_tol;   // a candidate of depth q is culled iff (double)q > (double)m * k + abs_tol; k = 1 + rel_tol
    int s, R, Wc, Hc;    // cell edge in pixels, neighbourhood radius in cells, buffer size
};

constexpr int kMaxViews = AVL_MAX_VIEWS;
static_assert(kMaxViews * 8 == 32, "one vote byte per view in the 32-bit mask word");

// several cameras, one cloud: one P and one byte source per view, T and the range shared
struct ViewsParams {
    double P[kMaxViews][12];
    double T[16];
    const unsigned char* src[kMaxViews];
    double range_max;
    int has_T, n_views, img_w, img_h;
};

// avl_point_logits in kernel-argument form
struct LogitsParams {
    const float* logits[kMaxViews];
    int* abstained;                   // [n_views] abstentions, or NULL
    long long ld;
    int h, w, K, net_h, net_w;
    float sy, sx, min_margin;
};

// The semantic source of a vote kernel: the two public kinds, and the plan's fp32 logits (avl_fused_frame_logits and its kin)
constexpr int kSrcLogits = 2;
static_assert(kSrcLogits != AVL_SRC_RGB && kSrcLogits != AVL_SRC_CLASSMAP, "the logits source is no public AVL_SRC_*");

__device__ __forceinline__ void load_point(const PtsView& v, int k, double& x, double& y, double& z, double& it) {
    if (v.aos_f32) {
        const float4 p = *reinterpret_cast<const float4*>(v.base + (long long)k * 16);
        x = (double)p.x; y = (double)p.y; z = (double)p.z; it = (double)p.w;
        return;
    }
    const char* p = v.base + (long long)k * v.point_stride;
    if (v.dtype == AVL_F64) {
        x = *reinterpret_cast<const double*>(p);
        y = *reinterpret_cast<const double*>(p + v.comp_stride);
        z = *reinterpret_cast<const double*>(p + 2 * v.comp_stride);
        it = *reinterpret_cast<const double*>(p + 3 * v.comp_stride);
    } else {
        x = (double)*reinterpret_cast<const float*>(p);
        y = (double)*reinterpret_cast<const float*>(p + v.comp_stride);
        z = (double)*reinterpret_cast<const float*>(p + 2 * v.comp_stride);
        it = (double)*reinterpret_cast<const float*>(p + 3 * v.comp_stride);
    }
}

// float64 -> int32 as NumPy on x86-64 does it (cvttsd2si): truncate toward zero; NaN, +-inf and
// anything that does not fit yield INT_MIN.  v_cvt_i32_f64 would saturate / give 0.
__device__ __forceinline__ int cvt_i32_numpy(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return INT_MIN;
    return (int)v;
}

// int32(num / den) exactly as NumPy computes it -- the correctly rounded float64 quotient, truncated (cvt_i32_numpy) -- without
// the ~35-instruction IEEE division sequence in the common case (round 4; four divisions per point).  `y` approximates 1 / den to
// a few ulp (refine_rcp).  q = num * y corrected once by its own residual is within ~2 ulp of the true quotient; the truncation of
// that equals the truncation of the correctly rounded quotient unless an integer lies within those ulps -- so lanes whose q is
// within 2^-44 (relative) of an integer, or is not an ordinary number (NaN, infinity, zero, |q| >= 2^40: zero / non-finite
// denominators, overflow), take the exact division instead.  Both paths give the same int32 for every input; the exact one runs
// for ~1e-10 of ordinary points (tests/test_gpu_mapping.py::test_truncating_divisions_on_integer_boundaries forces it).
__device__ __forceinline__ double refine_rcp(double den) {
    double y = __builtin_amdgcn_rcp(den);                 // v_rcp_f64: ~26 bits
    double e = __builtin_fma(-den, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-den, y, 1.0);
    return __builtin_fma(y, e, y);
}
__device__ __forceinline__ int div_i32_numpy(double num, double den, double y) {
    double q = num * y;
    const double r = __builtin_fma(-q, den, num);
    q = __builtin_fma(r, y, q);
    const double aq = __builtin_fabs(q);
    const bool safe = __builtin_fabs(q - __builtin_rint(q)) > aq * 0x1p-44 && aq > 0x1p-500 && aq < 0x1p40;
    if (!safe) q = num / den;
    return cvt_i32_numpy(q);
}

// dot of a 4-vector row with (a,b,c,d) in OpenBLAS's order: r0*a, then fma chain.
__device__ __forceinline__ double dot4(const double* r, double a, double b, double c, double d) {
    double s = r[0] * a;
    s = __builtin_fma(r[1], b, s);
    s = __builtin_fma(r[2], c, s);
    s = __builtin_fma(r[3], d, s);
    return s;
}

// :371 and :378: v = T . (x, y, z, 1), or the point itself without a T; true when 0 < v.x < range_max.  The same for every view.
__device__ __forceinline__ bool to_camera(const double* T, int has_T, double range_max, double x, double y, double z, double& v0,
                                          double& v1, double& v2, double& v3) {
    v0 = x; v1 = y; v2 = z; v3 = 1.0;
    if (has_T) {
        v0 = dot4(T + 0, x, y, z, 1.0);
        v1 = dot4(T + 4, x, y, z, 1.0);
        v2 = dot4(T + 8, x, y, z, 1.0);
        v3 = dot4(T + 12, x, y, z, 1.0);
    }
    return (0.0 < v0) && (v0 < range_max);
}

// :375 and :381-383 through one view's P: true when the pixel lies in the image.  `p2` = the third row of P . v, the divisor of
// :375: the depth the occlusion test compares (k_occl_depth, occl_culled)
__device__ __forceinline__ bool project_view(const double* P, double v0, double v1, double v2, double v3, int img_w, int img_h, int& ix,
                                             int& iy, double& p2) {
    const double p0 = dot4(P + 0, v0, v1, v2, v3);
    const double p1 = dot4(P + 4, v0, v1, v2, v3);
    p2 = dot4(P + 8, v0, v1, v2, v3);
    const double rp2 = refine_rcp(p2);
    ix = div_i32_numpy(p0, p2, rp2);
    iy = div_i32_numpy(p1, p2, rp2);
    return ix >= 0 && ix < img_w && iy >= 0 && iy < img_h;
}

// one camera: the pixel is computed whatever the range test says (k_project_points writes it)
__device__ __forceinline__ bool project(const ProjParams& pp, double x, double y, double z, int& ix, int& iy, double& p2) {
    double v0, v1, v2, v3;
    const bool positive = to_camera(pp.T, pp.has_T, pp.range_max, x, y, z, v0, v1, v2, v3);
    const bool in_image = project_view(pp.P, v0, v1, v2, v3, pp.img_w, pp.img_h, ix, iy, p2);
    return positive && in_image;
}
__device__ __forceinline__ bool project(const ProjParams& pp, double x, double y, double z, int& ix, int& iy) {
    double p2;
    return project(pp, x, y, z, ix, iy, p2);
}

// grid cell of a point in its ORIGINAL frame (:404-411); -1 if off-grid / non-finite
__device__ __forceinline__ int grid_cell(const GridParams& g, double x, double y, double z) {
    const double xl = x + g.off_x, yl = y + g.off_y, zl = z + 0.0;
    // :406 subtracts 0*z-like terms built from every coordinate: one non-finite coordinate makes both NaN
    if (!(__builtin_isfinite(xl) && __builtin_isfinite(yl) && __builtin_isfinite(zl))) return -1;
    const double rres = refine_rcp(g.resolution);
    const int cx = div_i32_numpy(xl - g.b00, g.resolution, rres);
    const int cy = div_i32_numpy(yl - g.b10, g.resolution, rres);
    if (cx < 0 || cx >= g.Hm || cy < 0 || cy >= g.Wm) return -1;
    return cx * g.Wm + cy;
}

__device__ __forceinline__ unsigned vote_from_rg(const GridParams& g, unsigned r, unsigned gch) {
    unsigned vote = 0;
    for (int i = 0; i < g.C; ++i)
        if (g.colors[3 * i] == r && g.colors[3 * i + 1] == gch) vote |= 1u << i;  // blue ignored (Q2)
    return vote;
}

__device__ __forceinline__ unsigned add_bonus(unsigned vote, unsigned bonus_classes, double intensity) {
    if ((vote & bonus_classes) && (intensity < 2.0 || intensity > 14.0)) vote |= (vote & bonus_classes) << 16;
    return vote;
}

// the label fetch of a byte source at pixel (ix, iy) of the img_w x img_h projection image -> vote bits
template <int SRC>
__device__ __forceinline__ unsigned fetch_vote(const GridParams& g, const LutParams& lut, const unsigned char* __restrict__ src, int src_w,
                                               int src_h, int img_w, int img_h, int ix, int iy) {
    if (SRC == AVL_SRC_RGB) {
        const unsigned char* px = src + 3ll * ((long long)iy * src_w + ix);
        return vote_from_rg(g, px[0], px[1]);
    }
    // cv2 INTER_NEAREST source index: min(floor(d * (src/dst)), src - 1), double arithmetic
    int sx = ix, sy = iy;
    if (src_w != img_w) sx = min((int)__builtin_floor((double)ix * ((double)src_w / (double)img_w)), src_w - 1);
    if (src_h != img_h) sy = min((int)__builtin_floor((double)iy * ((double)src_h / (double)img_h)), src_h - 1);
    return lut.lut[src[(long long)sy * src_w + sx]];
}

// ---------------------------------------------------------------- occlusion culling (avl_fused_frame_occl and its kin)
// A map point behind a wall projects onto the wall's pixels and takes its label.  Before the vote, every view gets a coarse depth
// buffer in image space; a point votes only if it is not clearly behind the nearest point of its image neighbourhood.  The rule
// (include/avl_hip.h states it in full):
//   candidate: a point that passes project(): 0 < v0 < range_max and 0 <= ix < img_w, 0 <= iy < img_h, on the grid or not;
//   key q = (float)p2, p2 the third row of P . v; only a finite key > 0 is written to the buffer or compared;
//   depth[iy / s][ix / s] = min of the keys' bit patterns (positive floats order as unsigned integers), 0xFFFFFFFF = empty;
//   m = min of depth over the (2R + 1)^2 cells around the candidate's, clipped to the buffer;
//   culled iff (double)q > (double)m * k + abs_tol (a multiplication and an addition, each rounded: -ffp-contract=off).
// Integer atomicMin and, for the counts, integer atomicAdd only: the result does not depend on the order of the points.

// the key of depth p2 as its bit pattern; false for a key that is not finite and > 0 (it is neither written nor culled)
__device__ __forceinline__ bool depth_key(double p2, unsigned& bits) {
    const float q = (float)p2;
    bits = __float_as_uint(q);
    return q > 0.0f && q < __builtin_inff();
}

__device__ __forceinline__ long long depth_cell(const OcclParams& oc, int v, int ix, int iy) {
    return ((long long)v * oc.Hc + iy / oc.s) * oc.Wc + ix / oc.s;
}

// the cull test of a candidate of view v with a valid key: its own cell is in the neighbourhood, so m <= bits and m is a key
__device__ __forceinline__ bool occl_culled(const OcclParams& oc, int v, int ix, int iy, unsigned bits) {
    const int cx = ix / oc.s, cy = iy / oc.s;
    const int x0 = max(cx - oc.R, 0), x1 = min(cx + oc.R, oc.Wc - 1), y0 = max(cy - oc.R, 0), y1 = min(cy + oc.R, oc.Hc - 1);
    const unsigned* depth = oc.depth + (long long)v * oc.Hc * oc.Wc;
    unsigned m = 0xffffffffu;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) m = min(m, depth[y * oc.Wc + x]);
    return (double)__uint_as_float(bits) > (double)__uint_as_float(m) * oc.k + oc.abs_tol;
}

// culled candidates of one view: one atomic per wave that has any.  Every lane of the wave must arrive here.
__device__ __forceinline__ void count_culled(int* counts, int v, bool culled) {
    if (!counts) return;
    const unsigned long long m = __ballot(culled);
    if (m != 0ull && (threadIdx.x & 63) == __builtin_ctzll(m)) atomicAdd(&counts[v], __builtin_popcountll(m));
}

// ---------------------------------------------------------------- points labelled from interpolated logits (avl_fused_frame_logits and its kin)
// The class-map source hands a point the arg-max of the nearest low-resolution pixel.  The logits source reads the plan's fp32 logits
// instead and evaluates the reference model's full-resolution prediction (bilinear, align_corners=True, then arg-max:
// deeplab_v3_plus.py:67-69) at the point's pixel alone, with the top-1 minus top-2 margin as a confidence: a point whose margin is
// below min_margin abstains.  The rule is stated in full at struct avl_point_logits in include/avl_hip.h; the interpolation is that of
// seg_head.hip (src_coord, corner, lerp4) with every float32 operation rounded on its own, which -ffp-contract=off gives here.
// What a lane fetches: the K logits of four source pixels, each a run of K consecutive floats (76 bytes at K = 19, ld = K: 4-byte
// aligned only, so no lane can count on a 16-byte boundary).  The loop takes four classes of each corner at a time -- sixteen
// independent loads in flight before the first is used, which the compiler merges into dwordx4 / dwordx2 loads of 4-byte alignment
// (gfx950 allows them on global memory) -- and keeps only the running best, second best and index.

// One more class for the running arg-max: the first maximal index wins and a NaN counts as maximal (AVL_OP_ARGMAX, eval_pixel of
// seg_head.hip); `second` follows as the largest of the others.  best = second = -inf, top = 0 to start with.
__device__ __forceinline__ void take_logit(float v, int k, float& best, float& second, int& top) {
    if (v > best || (v != v && best == best)) { second = best; best = v; top = k; }
    else if (v > second) second = v;
}

// rules 2 - 5 at pixel (ix, iy) of the img_w x img_h projection image: -> top, and the margin
__device__ __forceinline__ int point_label(const LogitsParams& lp, const float* __restrict__ src, int img_w, int img_h, int ix, int iy,
                                           float& margin) {
    int nx = ix, ny = iy;                                                  // the index rule of fetch_vote, towards the network's input
    if (lp.net_w != img_w) nx = min((int)__builtin_floor((double)ix * ((double)lp.net_w / (double)img_w)), lp.net_w - 1);
    if (lp.net_h != img_h) ny = min((int)__builtin_floor((double)iy * ((double)lp.net_h / (double)img_h)), lp.net_h - 1);
    const float fy = lp.sy * (float)ny, fx = lp.sx * (float)nx;
    const int y0 = min((int)fy, lp.h - 1), x0 = min((int)fx, lp.w - 1);
    const int y1 = y0 + (y0 < lp.h - 1 ? 1 : 0), x1 = x0 + (x0 < lp.w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* __restrict__ a = src + ((long long)y0 * lp.w + x0) * lp.ld;
    const float* __restrict__ b = src + ((long long)y0 * lp.w + x1) * lp.ld;
    const float* __restrict__ c = src + ((long long)y1 * lp.w + x0) * lp.ld;
    const float* __restrict__ d = src + ((long long)y1 * lp.w + x1) * lp.ld;
    float best = -__builtin_inff(), second = -__builtin_inff();
    int top = 0, k = 0;
    for (; k + 4 <= lp.K; k += 4) {
        float va[4], vb[4], vc[4], vd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { va[j] = a[k + j]; vb[j] = b[k + j]; vc[j] = c[k + j]; vd[j] = d[k + j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) take_logit(hy * (hx * va[j] + lx * vb[j]) + ly * (hx * vc[j] + lx * vd[j]), k + j, best, second, top);
    }
    for (; k < lp.K; ++k) take_logit(hy * (hx * a[k] + lx * b[k]) + ly * (hx * c[k] + lx * d[k]), k, best, second, top);
    margin = lp.K == 1 ? __builtin_inff() : best - second;
    return top;
}

// The vote of one candidate pixel, whatever the source: a byte source always has one (its bits may be zero); the logits source
// abstains where the margin is below min_margin.  `src` / `logits`: this view's image.
template <int SRC>
__device__ __forceinline__ unsigned pixel_vote(const GridParams& g, const LutParams& lut, const LogitsParams& lp, const unsigned char* __restrict__ src,
                                               const float* __restrict__ logits, int src_w, int src_h, int img_w, int img_h, int ix, int iy,
                                               double intensity, bool& abstains) {
    if (SRC == kSrcLogits) {
        float margin;
        const int top = point_label(lp, logits, img_w, img_h, ix, iy, margin);
        abstains = margin < lp.min_margin;
        return abstains ? 0u : add_bonus(lut.lut[top], g.bonus_classes, intensity);
    }
    return add_bonus(fetch_vote<SRC>(g, lut, src, src_w, src_h, img_w, img_h, ix, iy), g.bonus_classes, intensity);
}

// OR the vote into the cell; the lane that turns the mask non-zero records the cell.  The append
// counter is bumped once per wave (ballot + popcount) instead of once per lane.
__device__ __forceinline__ void cast_vote(unsigned* cell_mask, int* touched, int* counter, int cell, unsigned vote) {
    bool first = false;
    if (cell >= 0 && vote != 0) first = (atomicOr(&cell_mask[cell], vote) == 0u);
    const unsigned long long m = __ballot(first);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == __builtin_ctzll(m)) base = atomicAdd(counter, __builtin_popcountll(m));
    base = __shfl(base, __builtin_ctzll(m));
    if (first) touched[base + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = cell;
}

// Dense clouds: no touched list -- a fire-and-forget OR (no-return atomic, nothing depends on it); the apply
// pass then sweeps the whole mask instead of a list (k_grid_apply_scan).
__device__ __forceinline__ void cast_vote_nolist(unsigned* cell_mask, int cell, unsigned vote) {
    if (cell >= 0 && vote != 0) atomicOr(&cell_mask[cell], vote);
}

// Byte-wide vote mask (dense-cloud path, when C class bits + the bonus bits fit 8): bit i = class i seen, bit C + r = lane
// bonus of the r-th class of bonus_classes.  A quarter of the bytes of the 32-bit mask for the sweep to read; the OR goes
// to the containing dword (idempotent, so any interleaving of lanes gives the same mask).
__device__ __forceinline__ unsigned encode_vote_byte(unsigned vote, int C, unsigned bonus_classes) {
    unsigned enc = vote & ((1u << C) - 1u);
    unsigned rest = bonus_classes;
    int r = 0;
    while (rest) {
        const int j = __builtin_ctz(rest);
        rest &= rest - 1u;
        if ((vote >> (16 + j)) & 1u) enc |= 1u << (C + r);
        ++r;
    }
    return enc;
}
__device__ __forceinline__ void cast_vote_byte(unsigned* cell_mask, int cell, unsigned vote, int C, unsigned bonus_classes) {
    if (cell >= 0 && vote != 0) atomicOr(&cell_mask[cell >> 2], encode_vote_byte(vote, C, bonus_classes) << ((cell & 3) * 8));
}

// ---------------------------------------------------------------- projection only (:367-383)
__global__ void __launch_bounds__(kBlock) k_project_points(PtsView pv, ProjParams pp, int* __restrict__ out_ixy,
                                                           unsigned char* __restrict__ out_mask) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= pv.n) return;
    double x, y, z, it;
    load_point(pv, k, x, y, z, it);
    int ix, iy;
    const bool ok = project(pp, x, y, z, ix, iy);
    if (out_ixy) {
        out_ixy[k] = ix;
        out_ixy[pv.n + k] = iy;
    }
    if (out_mask) out_mask[k] = ok ? 1 : 0;
}

// ---------------------------------------------------------------- project_pcd with compaction
// pass 1: mask + pixel per point, survivors per block
__global__ void __launch_bounds__(kBlock) k_pcd_mask(PtsView pv, ProjParams pp, int* __restrict__ pix,
                                                     int* __restrict__ block_count) {
    __shared__ int wave_cnt[kBlock / 64];
    const int k = blockIdx.x * kBlock + threadIdx.x;
    bool ok = false;
    if (k < pv.n) {
        double x, y, z, it;
        load_point(pv, k, x, y, z, it);
        int ix, iy;
        ok = project(pp, x, y, z, ix, iy);
        pix[k] = ok ? iy * pp.img_w + ix : -1;
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __builtin_popcountll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kBlock / 64; ++w) s += wave_cnt[w];
        block_count[blockIdx.x] = s;
    }
}

// pass 2: exclusive scan of the block counts (one workgroup), total -> out_count
__global__ void __launch_bounds__(1024) k_scan_blocks(int* __restrict__ block_count, int nb, int* __restrict__ out_count) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (nb + 1023) / 1024;
    const int lo = t * per, hi = min(lo + per, nb);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += block_count[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
        int v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;  // exclusive prefix of this thread's chunk
    for (int i = lo; i < hi; ++i) {
        const int c = block_count[i];
        block_count[i] = run;
        run += c;
    }
    if (t == 1023) *out_count = part[1023];
}

// pass 3: order-preserving scatter of the survivors + RGB gather (:385-387)
__global__ void __launch_bounds__(kBlock) k_pcd_scatter(PtsView pv, const int* __restrict__ pix,
                                                        const int* __restrict__ block_off,
                                                        const unsigned char* __restrict__ image,
                                                        double* __restrict__ out_pcd, unsigned char* __restrict__ out_label,
                                                        long long out_ld) {
    __shared__ int wave_cnt[kBlock / 64];
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const int p = (k < pv.n) ? pix[k] : -1;
    const bool ok = p >= 0;
    const unsigned long long m = __ballot(ok);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[wave] = __builtin_popcountll(m);
    __syncthreads();
    if (!ok) return;
    int dst = block_off[blockIdx.x] + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) dst += wave_cnt[w];
    double x, y, z, it;
    load_point(pv, k, x, y, z, it);
    out_pcd[dst] = x;
    out_pcd[out_ld + dst] = y;
    out_pcd[2 * out_ld + dst] = z;
    out_pcd[3 * out_ld + dst] = it;
    const unsigned char* px = image + 3ll * p;
    out_label[dst] = px[0];
    out_label[out_ld + dst] = px[1];
    out_label[2 * out_ld + dst] = px[2];
}

// ---------------------------------------------------------------- update_map front end (:403-437)
__global__ void __launch_bounds__(kBlock) k_vote_labelled(const double* __restrict__ pcd, const unsigned char* __restrict__ label,
                                                          long long ld, int m_host, const int* __restrict__ m_dev,
                                                          GridParams g, unsigned* __restrict__ cell_mask,
                                                          int* __restrict__ touched, int* __restrict__ counter) {
    const int m = m_dev ? min(*m_dev, m_host) : m_host;
    const int k = blockIdx.x * kBlock + threadIdx.x;
    int cell = -1;
    unsigned vote = 0;
    if (k < m) {
        cell = grid_cell(g, pcd[k], pcd[ld + k], pcd[2 * ld + k]);
        if (cell >= 0) {
            vote = vote_from_rg(g, label[k], label[ld + k]);
            vote = add_bonus(vote, g.bonus_classes, pcd[3 * ld + k]);
        }
    }
    cast_vote(cell_mask, touched, counter, cell, vote);
}

// ---------------------------------------------------------------- fused project + vote
// Partitioned touched lists (MODE 3).  The single-counter list of cast_vote serialises on one L2 address (185 us for the 1 M
// points of config E); here a workgroup compacts its first-touch cells in LDS, reserves their range with ONE global atomic on
// counter kListBase + (workgroup % kLists) and appends to that list: 64 addresses, ~60 atomics each.  List k holds at most
// (workgroups of k) x 256 entries, so `cap` = ceil(nwg / kLists) * 256 never overflows.
constexpr int kLists = 64;
constexpr int kListBase = 4;                 // counter[4 .. 4 + kLists): cursors; counter[4 + kLists .. 4 + 2 kLists): apply tickets
// The append of the lane's cell (`first`: this lane turned the cell's mask non-zero) to the workgroup's list; every lane of the
// workgroup must arrive here.
__device__ __forceinline__ void append_listed(int* touched, int* counter, int cap, bool first, int cell) {
    __shared__ int wg_count, wg_base;
    if (threadIdx.x == 0) wg_count = 0;
    __syncthreads();
    const unsigned long long m = __ballot(first);
    const int lane = threadIdx.x & 63;
    int wave_off = 0;
    if (m != 0ull && lane == 0) wave_off = atomicAdd(&wg_count, __builtin_popcountll(m));
    wave_off = __shfl(wave_off, 0);
    __syncthreads();
    const int list = blockIdx.x % kLists;
    if (threadIdx.x == 0 && wg_count > 0) wg_base = atomicAdd(&counter[kListBase + list], wg_count);
    __syncthreads();
    // cap = (vote workgroups of this list) x 256 cannot overflow while the cursors start from zero; they would not after an apply
    // launch that failed (the host then resets them, lists_applied), so the append is bounded all the same: an entry
    // past cap is dropped, never written outside the list
    const int slot = wg_base + wave_off + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (first && slot < cap) touched[(long long)list * cap + slot] = cell;
}
// byte mask + lists (MODE 3 of k_fused_vote)
__device__ __forceinline__ void cast_vote_byte_lists(unsigned* cell_mask, int* touched, int* counter, int cap, int cell, unsigned vote,
                                                     int C, unsigned bonus_classes) {
    bool first = false;
    if (cell >= 0 && vote != 0) {
        const unsigned enc = encode_vote_byte(vote, C, bonus_classes);
        const unsigned sh = 8u * ((unsigned)cell & 3u);
        const unsigned old = atomicOr(&cell_mask[cell >> 2], enc << sh);
        first = ((old >> sh) & 0xffu) == 0u;          // this lane turned the cell's byte non-zero: it lists the cell
    }
    append_listed(touched, counter, cap, first, cell);
}
// word mask + lists (k_views_vote): the whole word is the cell's mask
__device__ __forceinline__ void cast_vote_word_lists(unsigned* cell_mask, int* touched, int* counter, int cap, int cell, unsigned word) {
    bool first = false;
    if (cell >= 0 && word != 0u) first = atomicOr(&cell_mask[cell], word) == 0u;   // this lane turned the word non-zero: it lists the cell
    append_listed(touched, counter, cap, first, cell);
}

// One lane per point: project, cull (OCCL), cell, label, vote.
// SRC:  AVL_SRC_RGB, AVL_SRC_CLASSMAP (src, src_w, src_h, lut) or kSrcLogits (lp, lut: class -> vote bits)
// MODE: 0 = 32-bit mask + touched list, 1 = 32-bit mask only (sweep), 2 = byte mask only (sweep, see encode_vote_byte),
//       3 = byte mask + partitioned touched lists (k_grid_apply_lists)
// OCCL: the cull test against the depth buffer of k_occl_depth stands between the projection and the cell.  A culled candidate never
//       evaluates grid_cell, so it casts no vote, fetches no label and, with the logits, is no abstention; it is counted.
// lp and oc are passed whether used or not.  No early return: every lane reaches the ballots of count_culled and the barriers of
// append_listed.
template <int SRC, int MODE, int OCCL>
__global__ void __launch_bounds__(kBlock) k_fused_vote(PtsView pv, ProjParams pp, GridParams g,
                                                       const unsigned char* __restrict__ src, int src_w, int src_h, LogitsParams lp,
                                                       LutParams lut, unsigned* __restrict__ cell_mask,
                                                       int* __restrict__ touched, int* __restrict__ counter, int list_cap, OcclParams oc) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    int cell = -1;
    unsigned vote = 0;
    bool culled = false, abstains = false;
    if (k < pv.n) {
        double x, y, z, it;
        load_point(pv, k, x, y, z, it);
        int ix, iy;
        double p2;
        if (project(pp, x, y, z, ix, iy, p2)) {
            if (OCCL) {
                unsigned bits;
                culled = depth_key(p2, bits) && occl_culled(oc, 0, ix, iy, bits);
            }
            if (!culled) cell = grid_cell(g, x, y, z);
            if (cell >= 0) vote = pixel_vote<SRC>(g, lut, lp, src, lp.logits[0], src_w, src_h, pp.img_w, pp.img_h, ix, iy, it, abstains);
        }
    }
    if (OCCL) count_culled(oc.culled, 0, culled);
    if (SRC == kSrcLogits) count_culled(lp.abstained, 0, abstains);
    if (MODE == 0) cast_vote(cell_mask, touched, counter, cell, vote);
    else if (MODE == 1) cast_vote_nolist(cell_mask, cell, vote);
    else if (MODE == 2) cast_vote_byte(cell_mask, cell, vote, g.C, g.bonus_classes);
    else cast_vote_byte_lists(cell_mask, touched, counter, list_cap, cell, vote, g.C, g.bonus_classes);
}

// Several cameras, one cloud (avl_fused_frame_views).  V synchronised cameras project the SAME cloud with the SAME pose
// (src/mapping.py:273-285), and the grid cell of a point comes from its original coordinates (:403-409), not from the camera: every
// view of a point votes into one cell.  So one lane per point loads it, applies T, tests the range and computes the cell ONCE, then
// projects through each view's P, fetches that view's label and builds that view's vote byte (encode_vote_byte); the 32-bit word of
// cell_mask holds byte v for view v and takes the votes of all views with one atomicOr.  The apply pass replays the bytes view by
// view (apply_views_word), which is what V sequential frames do to the cell.
// SRC, OCCL: as k_fused_vote, per view.  LISTS: 1 = word mask + partitioned lists (k_views_apply_lists), 0 = word mask only
// (k_views_sweep_words).
// An off-grid point casts no vote, so it is projected only with OCCL, where a culled off-grid candidate counts like any other (the
// counts are those of k_occl_visibility's state 2).  Where a count is kept (OCCL, logits) its ballot sits in the loop over the views,
// which every lane then runs in full; a plain byte source has no ballot, and only the lanes with a cell enter the loop.
template <int SRC, int LISTS, int OCCL>
__global__ void __launch_bounds__(kBlock) k_views_vote(PtsView pv, ViewsParams vp, GridParams g, int src_w, int src_h, LogitsParams lp,
                                                       LutParams lut, unsigned* __restrict__ cell_mask, int* __restrict__ touched,
                                                       int* __restrict__ counter, int list_cap, OcclParams oc) {
    constexpr bool kCounts = OCCL || SRC == kSrcLogits;
    const int k = blockIdx.x * kBlock + threadIdx.x;
    int cell = -1;
    unsigned word = 0;
    bool positive = false;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 1.0, it = 0.0;
    if (k < pv.n) {
        double x, y, z;
        load_point(pv, k, x, y, z, it);
        positive = to_camera(vp.T, vp.has_T, vp.range_max, x, y, z, v0, v1, v2, v3);
        if (positive) cell = grid_cell(g, x, y, z);                        // :378 and :404-411: the same for every view
    }
    const bool candidate = positive && (OCCL || cell >= 0);
    const int trips = (kCounts || candidate) ? vp.n_views : 0;             // kCounts: the same trip count in every lane
    for (int v = 0; v < trips; ++v) {
        bool culled = false, abstains = false;
        int ix, iy;
        double p2;
        if (candidate && project_view(vp.P[v], v0, v1, v2, v3, vp.img_w, vp.img_h, ix, iy, p2)) {   // else this view does not see the point
            if (OCCL) {
                unsigned bits;
                culled = depth_key(p2, bits) && occl_culled(oc, v, ix, iy, bits);
            }
            if (!culled && cell >= 0) {
                const unsigned vote = pixel_vote<SRC>(g, lut, lp, vp.src[v], lp.logits[v], src_w, src_h, vp.img_w, vp.img_h, ix, iy, it, abstains);
                word |= encode_vote_byte(vote, g.C, g.bonus_classes) << (8 * v);
            }
        }
        if (OCCL) count_culled(oc.culled, v, culled);
        if (SRC == kSrcLogits) count_culled(lp.abstained, v, abstains);
    }
    if (LISTS) cast_vote_word_lists(cell_mask, touched, counter, list_cap, cell, word);
    else if (cell >= 0 && word != 0u) atomicOr(&cell_mask[cell], word);                // fire and forget, as cast_vote_nolist
}

// ---------------------------------------------------------------- height-aware votes (avl_fused_frame_views_height and its kin)
// grid_cell() projects the cloud onto z = 0: a point in a tree canopy votes "vegetation" into the road cell beneath it.  With the
// ground plane in the grid's frame a point's height above the ground costs three products and three sums on values the lane holds
// anyway; a class bit stays only while that height lies in the class's band, and the same z, summed per cell in integer quanta,
// is the elevation of the drivable surface.  The rule is stated in full at struct avl_height in include/avl_hip.h.
// avl_height in kernel-argument form
struct HeightParams {
    double plane[4];                                   // unit normal, c > 0, in the frame of the cloud as passed in
    double min_m[AVL_MAX_MAP_CLASSES], max_m[AVL_MAX_MAP_CLASSES];
    double slope, quantum;
    int* gated;                                        // [n_views] votes the gate withheld, or NULL
    unsigned long long* elev_sum;                      // [Hm * Wm] sum of q (two's complement of an int64), NULL = no layer
    int *elev_cnt, *elev_min, *elev_max;
    unsigned elev_classes;
    int gate;
};

// rule 1: three products, three sums, each rounded on its own
__device__ __forceinline__ double point_height(const HeightParams& hp, double x, double y, double z) {
    double t = hp.plane[0] * x;
    double u = hp.plane[1] * y;
    t = t + u;
    u = hp.plane[2] * z;
    t = t + u;
    return t + hp.plane[3];
}

// rule 3: class bit i of `b` stays iff min_m[i] - s <= h <= max_m[i] + s, its bonus bit with it.  The bounds are read from the
// by-value kernel argument with a wave-uniform index, as vote_from_rg reads GridParams::colors.
__device__ __forceinline__ unsigned gate_vote(const HeightParams& hp, int C, unsigned b, double h, double s) {
    unsigned keep = 0;
    for (int i = 0; i < C; ++i) {
        const double lo = hp.min_m[i] - s, hi = hp.max_m[i] + s;
        if (lo <= h && h <= hi) keep |= 1u << i;                           // a NaN h fails both
    }
    return b & (keep | (keep << 16));
}

// rule 5: one point's z into its cell of the layer.  Integer atomics only.
__device__ __forceinline__ void elevate(const HeightParams& hp, int cell, double z) {
    const double r = __builtin_rint(z / hp.quantum);                       // IEEE division, then round half to even
    if (!(r >= -2147483648.0 && r <= 2147483647.0)) return;
    const int q = (int)r;
    atomicAdd(&hp.elev_sum[cell], (unsigned long long)(long long)q);
    atomicAdd(&hp.elev_cnt[cell], 1);
    atomicMin(&hp.elev_min[cell], q);
    atomicMax(&hp.elev_max[cell], q);
}

// k_fused_vote with the height rule behind pixel_vote.  Kernels of their own, so that the plain and OCCL instantiations above keep
// their code; the occlusion test is a wave-uniform run-time branch here (oc.depth), as are the gate and the layer.
template <int SRC, int MODE>
__global__ void __launch_bounds__(kBlock) k_fused_vote_height(PtsView pv, ProjParams pp, GridParams g,
                                                              const unsigned char* __restrict__ src, int src_w, int src_h, LogitsParams lp,
                                                              LutParams lut, unsigned* __restrict__ cell_mask, int* __restrict__ touched,
                                                              int* __restrict__ counter, int list_cap, OcclParams oc, HeightParams hp) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    int cell = -1;
    unsigned vote = 0;
    bool culled = false, abstains = false, gated = false;
    if (k < pv.n) {
        double x, y, z, it, v0, v1, v2, v3, p2;
        load_point(pv, k, x, y, z, it);
        int ix, iy;
        const bool positive = to_camera(pp.T, pp.has_T, pp.range_max, x, y, z, v0, v1, v2, v3);
        if (positive && project_view(pp.P, v0, v1, v2, v3, pp.img_w, pp.img_h, ix, iy, p2)) {
            if (oc.depth) {
                unsigned bits;
                culled = depth_key(p2, bits) && occl_culled(oc, 0, ix, iy, bits);
            }
            if (!culled) cell = grid_cell(g, x, y, z);
            if (cell >= 0) {
                vote = pixel_vote<SRC>(g, lut, lp, src, lp.logits[0], src_w, src_h, pp.img_w, pp.img_h, ix, iy, it, abstains);
                if (hp.gate && vote != 0u) {
                    vote = gate_vote(hp, g.C, vote, point_height(hp, x, y, z), hp.slope * v0);
                    gated = vote == 0u;
                }
                if (hp.elev_sum && (vote & hp.elev_classes)) elevate(hp, cell, z);
            }
        }
    }
    if (oc.depth) count_culled(oc.culled, 0, culled);
    if (SRC == kSrcLogits) count_culled(lp.abstained, 0, abstains);
    if (hp.gate) count_culled(hp.gated, 0, gated);
    if (MODE == 0) cast_vote(cell_mask, touched, counter, cell, vote);
    else if (MODE == 1) cast_vote_nolist(cell_mask, cell, vote);
    else if (MODE == 2) cast_vote_byte(cell_mask, cell, vote, g.C, g.bonus_classes);
    else cast_vote_byte_lists(cell_mask, touched, counter, list_cap, cell, vote, g.C, g.bonus_classes);
}

// k_views_vote with the height rule: the height and the slack once per point, the per-class comparison per view; the point enters
// the layer once, with the union of the views' surviving class bits.  Every lane runs the loop in full (the ballots of the counts).
template <int SRC, int LISTS>
__global__ void __launch_bounds__(kBlock) k_views_vote_height(PtsView pv, ViewsParams vp, GridParams g, int src_w, int src_h, LogitsParams lp,
                                                              LutParams lut, unsigned* __restrict__ cell_mask, int* __restrict__ touched,
                                                              int* __restrict__ counter, int list_cap, OcclParams oc, HeightParams hp) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    int cell = -1;
    unsigned word = 0, seen = 0;
    bool positive = false;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 1.0, it = 0.0, z = 0.0, h = 0.0, slack = 0.0;
    if (k < pv.n) {
        double x, y;
        load_point(pv, k, x, y, z, it);
        positive = to_camera(vp.T, vp.has_T, vp.range_max, x, y, z, v0, v1, v2, v3);
        if (positive) cell = grid_cell(g, x, y, z);
        if (hp.gate && cell >= 0) {
            h = point_height(hp, x, y, z);
            slack = hp.slope * v0;
        }
    }
    const bool candidate = positive && (oc.depth != nullptr || cell >= 0);
    for (int v = 0; v < vp.n_views; ++v) {
        bool culled = false, abstains = false, gated = false;
        int ix, iy;
        double p2;
        if (candidate && project_view(vp.P[v], v0, v1, v2, v3, vp.img_w, vp.img_h, ix, iy, p2)) {
            if (oc.depth) {
                unsigned bits;
                culled = depth_key(p2, bits) && occl_culled(oc, v, ix, iy, bits);
            }
            if (!culled && cell >= 0) {
                unsigned vote = pixel_vote<SRC>(g, lut, lp, vp.src[v], lp.logits[v], src_w, src_h, vp.img_w, vp.img_h, ix, iy, it, abstains);
                if (hp.gate && vote != 0u) {
                    vote = gate_vote(hp, g.C, vote, h, slack);
                    gated = vote == 0u;
                }
                seen |= vote;
                word |= encode_vote_byte(vote, g.C, g.bonus_classes) << (8 * v);
            }
        }
        if (oc.depth) count_culled(oc.culled, v, culled);
        if (SRC == kSrcLogits) count_culled(lp.abstained, v, abstains);
        if (hp.gate) count_culled(hp.gated, v, gated);
    }
    if (hp.elev_sum && (seen & hp.elev_classes)) elevate(hp, cell, z);         // seen != 0 only with a cell
    if (LISTS) cast_vote_word_lists(cell_mask, touched, counter, list_cap, cell, word);
    else if (cell >= 0 && word != 0u) atomicOr(&cell_mask[cell], word);
}

// Rules 1 and 2 alone, for every point of a cloud, candidate or not: h and the slack; both NaN for a non-finite coordinate.
__global__ void __launch_bounds__(kBlock) k_point_heights(PtsView pv, ProjParams pp, HeightParams hp, double* __restrict__ h,
                                                          double* __restrict__ s) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= pv.n) return;
    double x, y, z, it, v0, v1, v2, v3;
    load_point(pv, k, x, y, z, it);
    to_camera(pp.T, pp.has_T, pp.range_max, x, y, z, v0, v1, v2, v3);
    const bool finite = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
    h[k] = finite ? point_height(hp, x, y, z) : __builtin_nan("");
    s[k] = finite ? hp.slope * v0 : __builtin_nan("");
}

__global__ void __launch_bounds__(kBlock) k_elevation_mean(const long long* __restrict__ sum, const int* __restrict__ cnt, long long ncell,
                                                           double quantum, float* __restrict__ out) {
    const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (c >= ncell) return;
    const int n = cnt[c];
    out[c] = n == 0 ? __builtin_nanf("") : (float)(((double)sum[c] / (double)n) * quantum);
}

__global__ void __launch_bounds__(kBlock) k_elevation_reset(long long* __restrict__ sum, int* __restrict__ cnt, int* __restrict__ qmin,
                                                            int* __restrict__ qmax, long long ncell) {
    const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (c >= ncell) return;
    sum[c] = 0;
    cnt[c] = 0;
    qmin[c] = INT_MAX;
    qmax[c] = INT_MIN;
}

// Depth pass, one view or several: one read of the cloud, T and the range test once per point, one atomicMin per candidate and
// view (no return value: nothing waits for it).  Off-grid points take part: an off-grid wall hides what is behind it.
__global__ void __launch_bounds__(kBlock) k_occl_depth(PtsView pv, ViewsParams vp, OcclParams oc) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= pv.n) return;
    double x, y, z, it, v0, v1, v2, v3;
    load_point(pv, k, x, y, z, it);
    if (!to_camera(vp.T, vp.has_T, vp.range_max, x, y, z, v0, v1, v2, v3)) return;
    for (int v = 0; v < vp.n_views; ++v) {
        int ix, iy;
        double p2;
        unsigned bits;
        if (project_view(vp.P[v], v0, v1, v2, v3, vp.img_w, vp.img_h, ix, iy, p2) && depth_key(p2, bits))
            atomicMin(&oc.depth[depth_cell(oc, v, ix, iy)], bits);
    }
}

// One state per point and view: 0 not a candidate, 1 visible, 2 culled; key (optional): the candidate's float32 depth, 0 for the rest.
// Reads the depth buffer k_occl_depth filled.
__global__ void __launch_bounds__(kBlock) k_occl_visibility(PtsView pv, ViewsParams vp, OcclParams oc, unsigned char* __restrict__ state,
                                                            float* __restrict__ key) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const bool live = k < pv.n;
    bool positive = false;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 1.0;
    if (live) {
        double x, y, z, it;
        load_point(pv, k, x, y, z, it);
        positive = to_camera(vp.T, vp.has_T, vp.range_max, x, y, z, v0, v1, v2, v3);
    }
    for (int v = 0; v < vp.n_views; ++v) {
        unsigned char st = 0;
        unsigned bits = 0u;
        int ix, iy;
        double p2;
        if (positive && project_view(vp.P[v], v0, v1, v2, v3, vp.img_w, vp.img_h, ix, iy, p2))
            st = (depth_key(p2, bits) && occl_culled(oc, v, ix, iy, bits)) ? 2 : 1;
        if (live) {
            state[(long long)v * pv.n + k] = st;
            if (key) key[(long long)v * pv.n + k] = st ? __uint_as_float(bits) : 0.0f;
        }
        count_culled(oc.culled, v, st == 2);
    }
}

// The logits rule alone, per point and view, on the grid or not: state = top, 254 = abstained, 255 = no candidate of the view; margin
// (optional) = the candidate's margin, 0 for the rest.
__global__ void __launch_bounds__(kBlock) k_point_labels(PtsView pv, ViewsParams vp, LogitsParams lp, unsigned char* __restrict__ state,
                                                         float* __restrict__ margin) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const bool live = k < pv.n;
    bool positive = false;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 1.0;
    if (live) {
        double x, y, z, it;
        load_point(pv, k, x, y, z, it);
        positive = to_camera(vp.T, vp.has_T, vp.range_max, x, y, z, v0, v1, v2, v3);
    }
    for (int v = 0; v < vp.n_views; ++v) {
        unsigned char st = 255;
        float m = 0.f;
        int ix, iy;
        double p2;
        if (positive && project_view(vp.P[v], v0, v1, v2, v3, vp.img_w, vp.img_h, ix, iy, p2)) {
            const int top = point_label(lp, lp.logits[v], vp.img_w, vp.img_h, ix, iy, m);
            st = m < lp.min_margin ? 254 : (unsigned char)top;
        }
        if (live) {
            state[(long long)v * pv.n + k] = st;
            if (margin) margin[(long long)v * pv.n + k] = m;
        }
        count_culled(lp.abstained, v, st == 254);
    }
}

// ---------------------------------------------------------------- touched cells -> grid (:424,437)
// One lane per touched cell: adds CM[:, i] for every class bit in reference order, the bonus right
// after its class, clears the mask.  Each cell appears once in `touched`, so no atomics on the map.
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_grid_apply(MapT* __restrict__ map, MapT* __restrict__ rows, int C, CmParams cm,
                                                       unsigned* __restrict__ cell_mask, const int* __restrict__ touched,
                                                       const int* __restrict__ counter) {
    const int n = *counter;
    for (int k = blockIdx.x * kBlock + threadIdx.x; k < n; k += gridDim.x * kBlock) {
        const int cell = touched[k];
        const unsigned m = cell_mask[cell];
        cell_mask[cell] = 0u;
        MapT* row = rows ? rows + (long long)k * C : map + (long long)cell * C;
        double v[AVL_MAX_MAP_CLASSES];
#pragma unroll
        for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
            if (c < C) v[c] = (double)row[c];
        for (int i = 0; i < C; ++i) {
            if (m & (1u << i)) {
#pragma unroll
                for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                    if (c < C) v[c] = (double)(MapT)(v[c] + cm.cm[c * C + i]);
            }
            if (m & (1u << (16 + i))) {
#pragma unroll
                for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                    if (c == i) v[c] = (double)(MapT)(v[c] + 2.0);
            }
        }
#pragma unroll
        for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
            if (c < C) row[c] = (MapT)v[c];
    }
}

// Sweep variant of the apply pass for dense clouds: every lane inspects 4 consecutive cells' masks (one
// 16-byte load); non-zero ones are applied exactly like k_grid_apply and cleared.  Cost ~ Hm*Wm*4 bytes,
// independent of the number of points.
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_grid_apply_scan(MapT* __restrict__ map, int C, CmParams cm,
                                                            unsigned* __restrict__ cell_mask, long long ncell4) {
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < ncell4; q += (long long)gridDim.x * kBlock) {
        const uint4 m4 = reinterpret_cast<const uint4*>(cell_mask)[q];
        if ((m4.x | m4.y | m4.z | m4.w) == 0u) continue;
        const unsigned mm[4] = {m4.x, m4.y, m4.z, m4.w};
        for (int j = 0; j < 4; ++j) {
            const unsigned m = mm[j];
            if (m == 0u) continue;
            MapT* row = map + (q * 4 + j) * C;
            for (int i = 0; i < C; ++i) {
                if (m & (1u << i))
                    for (int c = 0; c < C; ++c) row[c] = (MapT)((double)row[c] + cm.cm[c * C + i]);
                if (m & (1u << (16 + i))) row[i] = (MapT)((double)row[i] + 2.0);
            }
        }
        reinterpret_cast<uint4*>(cell_mask)[q] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// Partitioned lists -> grid (MODE 3 of k_fused_vote).  Workgroup (list k, slice j) applies entries j*256 + lane, + W*256, ... of
// list k: reads the cell's vote byte, clears it, updates the row in the reference's class order.  The last workgroup of a list
// to finish (a ticket per list: 64 addresses again) zeroes the list's cursor and ticket, so the counters are all zero on return.
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_grid_apply_lists(MapT* __restrict__ map, int C, unsigned bonus_classes, CmParams cm,
                                                             unsigned char* __restrict__ mask, const int* __restrict__ touched,
                                                             int* __restrict__ counter, int cap, int wgs_per_list) {
    const int k = blockIdx.x % kLists, j = blockIdx.x / kLists;
    // the append drops entries past cap but its cursor still advances (k_vote_append): clamp here as well, or a stale / overrun
    // cursor would walk into the next list
    const int n = min(counter[kListBase + k], cap);
    const int* list = touched + (long long)k * cap;
    for (int e = j * kBlock + threadIdx.x; e < n; e += wgs_per_list * kBlock) {
        const int cell = list[e];
        const unsigned m = mask[cell];
        mask[cell] = 0;
        MapT* row = map + (long long)cell * C;
        double vals[AVL_MAX_MAP_CLASSES];
#pragma unroll
        for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
            if (c < C) vals[c] = (double)row[c];
        int r = 0;
        for (int i = 0; i < C; ++i) {
            if (m & (1u << i)) {
#pragma unroll
                for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                    if (c < C) vals[c] = (double)(MapT)(vals[c] + cm.cm[c * C + i]);
            }
            if ((bonus_classes >> i) & 1u) {
                if (m & (1u << (C + r))) {
#pragma unroll
                    for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                        if (c == i) vals[c] = (double)(MapT)(vals[c] + 2.0);
                }
                ++r;
            }
        }
#pragma unroll
        for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
            if (c < C) row[c] = (MapT)vals[c];
    }
    __syncthreads();                  // every lane of this workgroup has read n
    if (threadIdx.x == 0) {
        const int t = atomicAdd(&counter[kListBase + kLists + k], 1);
        if (t == wgs_per_list - 1) {
            counter[kListBase + k] = 0;
            counter[kListBase + kLists + k] = 0;
        }
    }
}

// Sweep of the BYTE mask.  The 32-bit sweep above is latency-bound (one dependent 16-byte load per lane and iteration, then
// a serial read-modify-write chain in the few lanes that found something: 57 us for the 64 MB mask of config E).  Here a
// workgroup takes 16 K cells at a time: every lane has four independent 16-byte mask loads in flight, the non-zero bytes
// are compacted into an LDS list (local cell index << 8 | bits) with one LDS atomic each, the mask bytes are cleared,
// and then ALL lanes apply one listed cell each: the grid rows are read, updated in the reference's class order
// (class i, then its lane bonus) and written back with every lane busy and every load independent.
// Cells per workgroup round: a camera frustum puts most touched cells into a few grid rows, and the sweep ends when its BUSIEST
// workgroup does -- 4096-cell rounds (one 16-byte mask vector per lane) instead of 16384: config E 38.4 -> 34.6 us per frame
// (profiles/r04/mapping_sweep_chunk_ab.log).
constexpr int kSweepVec = 1;                                  // 16-byte mask vectors per lane and round
constexpr int kSweepCells = kBlock * kSweepVec * 16;          // cells per workgroup round
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_grid_sweep_bytes(MapT* __restrict__ map, int C, unsigned bonus_classes, CmParams cm,
                                                             unsigned char* __restrict__ mask, long long ncell) {
    __shared__ unsigned list[kSweepCells];
    __shared__ int count;
    const long long rounds = (ncell + kSweepCells - 1) / kSweepCells;
    for (long long rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        if (threadIdx.x == 0) count = 0;
        __syncthreads();
        const long long base = rd * kSweepCells;
        uint4 v[kSweepVec];
#pragma unroll
        for (int u = 0; u < kSweepVec; ++u) {
            const long long c0 = base + ((long long)u * kBlock + threadIdx.x) * 16;
            v[u] = c0 < ncell ? *reinterpret_cast<const uint4*>(mask + c0) : make_uint4(0u, 0u, 0u, 0u);
        }
        // list slots: every lane counts its non-zero bytes, one ballot-free wave scan (shuffles) gives its offset inside the
        // wave, ONE LDS atomic per wave reserves the wave's range -- instead of one returning LDS atomic per listed cell
        int mine = 0;
#pragma unroll
        for (int u = 0; u < kSweepVec; ++u) {
            const unsigned w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned x = w4[q];
                // one bit per non-zero byte: (x | x >> 1 | ... | x >> 7) & 0x01010101
                unsigned t = x | (x >> 4);
                t |= t >> 2;
                t |= t >> 1;
                mine += __builtin_popcount(t & 0x01010101u);
            }
        }
        const int lane = threadIdx.x & 63;
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        int wave_base = 0;
        if (lane == 63 && incl > 0) wave_base = atomicAdd(&count, incl);
        wave_base = __shfl(wave_base, 63);
        int slot = wave_base + incl - mine;
        if (mine > 0) {
#pragma unroll
            for (int u = 0; u < kSweepVec; ++u) {
                if ((v[u].x | v[u].y | v[u].z | v[u].w) == 0u) continue;
                const int local0 = (u * kBlock + threadIdx.x) * 16;
                auto take = [&](unsigned x, int first) {          // the non-zero bytes of one dword -> list (registers only: no indexed arrays)
                    while (x) {
                        const int b = __builtin_ctz(x) >> 3;
                        list[slot++] = ((unsigned)(local0 + first + b) << 8) | ((x >> (8 * b)) & 0xffu);
                        x &= ~(0xffu << (8 * b));
                    }
                };
                take(v[u].x, 0);
                take(v[u].y, 4);
                take(v[u].z, 8);
                take(v[u].w, 12);
            }
        }
#pragma unroll
        for (int u = 0; u < kSweepVec; ++u)
            if ((v[u].x | v[u].y | v[u].z | v[u].w) != 0u)
                *reinterpret_cast<uint4*>(mask + base + (u * kBlock + threadIdx.x) * 16) = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        const int n = count;
        for (int k = threadIdx.x; k < n; k += kBlock) {
            const unsigned e = list[k];
            const unsigned m = e & 0xffu;
            MapT* row = map + (base + (e >> 8)) * C;
            double vals[AVL_MAX_MAP_CLASSES];
#pragma unroll
            for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                if (c < C) vals[c] = (double)row[c];
            int r = 0;
            for (int i = 0; i < C; ++i) {
                if (m & (1u << i)) {
#pragma unroll
                    for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                        if (c < C) vals[c] = (double)(MapT)(vals[c] + cm.cm[c * C + i]);
                }
                if ((bonus_classes >> i) & 1u) {
                    if (m & (1u << (C + r))) {
#pragma unroll
                        for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                            if (c == i) vals[c] = (double)(MapT)(vals[c] + 2.0);
                    }
                    ++r;
                }
            }
#pragma unroll
            for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                if (c < C) row[c] = (MapT)vals[c];
        }
        __syncthreads();
    }
}

// ================================================================ several cameras, one cloud: mask word -> grid
// One cell's word -> its grid row: view 0's votes, then view 1's, ...; inside a view class i adds CM[:, i], then its bonus +2,
// and every addition is rounded to the map type -- the sequence V calls of avl_fused_frame run on the cell, so the row ends
// bit-identical to theirs (a store to MapT and a reload between two views changes nothing: the value is already a MapT).
template <typename MapT>
__device__ __forceinline__ void apply_views_word(MapT* row, unsigned word, int C, unsigned bonus_classes, const CmParams& cm) {
    double vals[AVL_MAX_MAP_CLASSES];
#pragma unroll
    for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
        if (c < C) vals[c] = (double)row[c];
    for (; word != 0u; word >>= 8) {
        const unsigned m = word & 0xffu;
        if (m == 0u) continue;
        int r = 0;
        for (int i = 0; i < C; ++i) {
            if (m & (1u << i)) {
#pragma unroll
                for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                    if (c < C) vals[c] = (double)(MapT)(vals[c] + cm.cm[c * C + i]);
            }
            if ((bonus_classes >> i) & 1u) {
                if (m & (1u << (C + r))) {
#pragma unroll
                    for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                        if (c == i) vals[c] = (double)(MapT)(vals[c] + 2.0);
                }
                ++r;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
        if (c < C) row[c] = (MapT)vals[c];
}

// Partitioned lists -> grid: k_grid_apply_lists on mask words (same list geometry, same tickets).
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_views_apply_lists(MapT* __restrict__ map, int C, unsigned bonus_classes, CmParams cm,
                                                              unsigned* __restrict__ mask, const int* __restrict__ touched,
                                                              int* __restrict__ counter, int cap, int wgs_per_list) {
    const int k = blockIdx.x % kLists, j = blockIdx.x / kLists;
    const int n = min(counter[kListBase + k], cap);
    const int* list = touched + (long long)k * cap;
    for (int e = j * kBlock + threadIdx.x; e < n; e += wgs_per_list * kBlock) {
        const int cell = list[e];
        const unsigned m = mask[cell];
        mask[cell] = 0u;
        apply_views_word(map + (long long)cell * C, m, C, bonus_classes, cm);
    }
    __syncthreads();                  // every lane of this workgroup has read n
    if (threadIdx.x == 0) {
        const int t = atomicAdd(&counter[kListBase + kLists + k], 1);
        if (t == wgs_per_list - 1) {
            counter[kListBase + k] = 0;
            counter[kListBase + kLists + k] = 0;
        }
    }
}

// Sweep of the word mask (dense clouds), built like k_grid_sweep_bytes: a workgroup takes kViewsSweepCells cells per round with
// kViewsSweepVec independent 16-byte loads per lane in flight, compacts the non-zero words into an LDS list (local cell, word),
// clears them, and then all lanes apply one listed cell each.  `vec` = the mask is 16-byte aligned; a last partial vector and
// an unaligned mask go through bounds-checked dword accesses.
constexpr int kViewsSweepVec = 4;
constexpr int kViewsSweepCells = kBlock * kViewsSweepVec * 4;
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_views_sweep_words(MapT* __restrict__ map, int C, unsigned bonus_classes, CmParams cm,
                                                              unsigned* __restrict__ mask, long long ncell, int vec) {
    __shared__ unsigned short lcell[kViewsSweepCells];
    __shared__ unsigned lword[kViewsSweepCells];
    __shared__ int count;
    const long long rounds = (ncell + kViewsSweepCells - 1) / kViewsSweepCells;
    for (long long rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        if (threadIdx.x == 0) count = 0;
        __syncthreads();
        const long long base = rd * kViewsSweepCells;
        uint4 v[kViewsSweepVec];
#pragma unroll
        for (int u = 0; u < kViewsSweepVec; ++u) {
            const long long c0 = base + ((long long)u * kBlock + threadIdx.x) * 4;
            if (vec && c0 + 4 <= ncell) v[u] = *reinterpret_cast<const uint4*>(mask + c0);
            else v[u] = make_uint4(c0 < ncell ? mask[c0] : 0u, c0 + 1 < ncell ? mask[c0 + 1] : 0u, c0 + 2 < ncell ? mask[c0 + 2] : 0u,
                                   c0 + 3 < ncell ? mask[c0 + 3] : 0u);
        }
        int mine = 0;
#pragma unroll
        for (int u = 0; u < kViewsSweepVec; ++u) mine += (v[u].x != 0u) + (v[u].y != 0u) + (v[u].z != 0u) + (v[u].w != 0u);
        const int lane = threadIdx.x & 63;
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        int wave_base = 0;
        if (lane == 63 && incl > 0) wave_base = atomicAdd(&count, incl);
        wave_base = __shfl(wave_base, 63);
        int slot = wave_base + incl - mine;
        if (mine > 0) {
#pragma unroll
            for (int u = 0; u < kViewsSweepVec; ++u) {
                if ((v[u].x | v[u].y | v[u].z | v[u].w) == 0u) continue;
                const int local0 = (u * kBlock + threadIdx.x) * 4;
                const long long c0 = base + local0;
                auto take = [&](unsigned x, int j) {
                    if (x != 0u) {
                        lcell[slot] = (unsigned short)(local0 + j);
                        lword[slot] = x;
                        ++slot;
                    }
                };
                take(v[u].x, 0);
                take(v[u].y, 1);
                take(v[u].z, 2);
                take(v[u].w, 3);
                if (vec && c0 + 4 <= ncell) *reinterpret_cast<uint4*>(mask + c0) = make_uint4(0u, 0u, 0u, 0u);
                else {
                    if (v[u].x != 0u) mask[c0] = 0u;
                    if (v[u].y != 0u) mask[c0 + 1] = 0u;
                    if (v[u].z != 0u) mask[c0 + 2] = 0u;
                    if (v[u].w != 0u) mask[c0 + 3] = 0u;
                }
            }
        }
        __syncthreads();
        const int n = count;
        for (int k = threadIdx.x; k < n; k += kBlock)
            apply_views_word(map + (base + lcell[k]) * C, lword[k], C, bonus_classes, cm);
        __syncthreads();
    }
}

// ================================================================ dense ground fill (avl_ground_fill_views and its kin)
// The inverse direction of the vote kernels: one lane per CELL of a window of the grid.  The lane puts the cell's centre on the
// ground plane, takes it to the cameras as a point of the cloud would go (to_camera, project_view), tests it against the depth
// buffer of real points (OCCL), fetches each view's label (pixel_vote) and updates its own row of the map.  A cell belongs to one
// lane, so there is no vote mask, no atomic on the map and no apply pass.  The rule is stated in full at struct avl_ground_fill in
// include/avl_hip.h.  What bounds the kernel: ~150 float64 operations per cell and view (two truncating divisions) in every
// lane that is in front of the vehicle, a label gather served by L2, and, in voting lanes only, one read-modify-write of C map
// values.  No LDS, integer atomics only (the counts, one per wave that has any).

// avl_ground_fill in kernel-argument form: the window clipped to the grid
struct FillParams {
    double plane[4];
    int x0, y0, h, w;
    unsigned class_mask;
    int* filled;         // [n_views] cells with a vote per view, or NULL
};

// One cell's votes -> its grid row: 16 vote bits per view, view 0 in the low bits; view 0's votes first, inside a view class i
// adds CM[:, i], every addition rounded to the map type: apply_views_word without the byte packing and without a bonus.
template <typename MapT>
__device__ __forceinline__ void apply_fill_word(MapT* row, unsigned long long word, int C, const CmParams& cm) {
    double vals[AVL_MAX_MAP_CLASSES];
#pragma unroll
    for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
        if (c < C) vals[c] = (double)row[c];
    for (; word != 0ull; word >>= 16) {
        const unsigned m = (unsigned)(word & 0xffffull);
        if (m == 0u) continue;
        for (int i = 0; i < C; ++i) {
            if (m & (1u << i)) {
#pragma unroll
                for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
                    if (c < C) vals[c] = (double)(MapT)(vals[c] + cm.cm[c * C + i]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < AVL_MAX_MAP_CLASSES; ++c)
        if (c < C) row[c] = (MapT)vals[c];
}
static_assert(AVL_MAX_MAP_CLASSES * kMaxViews <= 64, "16 vote bits per view in the 64-bit word of apply_fill_word");

// SRC, OCCL: as k_views_vote.  Lane -> cell (x0 + idx / w, y0 + idx % w): neighbouring lanes own neighbouring rows of the map.
// g.bonus_classes is zero (a cell has no intensity), so pixel_vote adds no bonus.  Every lane runs the loop over the views in
// full: the ballots of the counts sit in it.
template <int SRC, int OCCL, typename MapT>
__global__ void __launch_bounds__(kBlock) k_ground_fill(MapT* __restrict__ map, ViewsParams vp, GridParams g, FillParams fp, int src_w,
                                                        int src_h, LogitsParams lp, LutParams lut, CmParams cm, OcclParams oc) {
    const long long lane = (long long)blockIdx.x * kBlock + threadIdx.x;      // the last workgroup of a 2^31 - 1 cell window goes past an int
    bool positive = false;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 1.0;
    long long cell = 0;
    if (lane < (long long)fp.h * fp.w) {
        const int idx = (int)lane;
        const int i = fp.x0 + idx / fp.w, j = fp.y0 + idx % fp.w;
        const double x = (g.b00 + ((double)i + 0.5) * g.resolution) - g.off_x;
        const double y = (g.b10 + ((double)j + 0.5) * g.resolution) - g.off_y;
        double t = fp.plane[0] * x;
        t = t + fp.plane[1] * y;
        t = t + fp.plane[3];
        const double z = (-t) / fp.plane[2];
        positive = to_camera(vp.T, vp.has_T, vp.range_max, x, y, z, v0, v1, v2, v3);
        cell = (long long)i * g.Wm + j;
    }
    unsigned long long word = 0ull;
    for (int v = 0; v < vp.n_views; ++v) {
        bool culled = false, abstains = false;
        unsigned bits = 0u;
        int ix, iy;
        double p2;
        if (positive && project_view(vp.P[v], v0, v1, v2, v3, vp.img_w, vp.img_h, ix, iy, p2)) {   // else this view does not see the cell
            if (OCCL) {
                unsigned key;
                culled = depth_key(p2, key) && occl_culled(oc, v, ix, iy, key);
            }
            if (!culled)
                bits = pixel_vote<SRC>(g, lut, lp, vp.src[v], lp.logits[v], src_w, src_h, vp.img_w, vp.img_h, ix, iy, 0.0, abstains) & fp.class_mask;
        }
        if (OCCL) count_culled(oc.culled, v, culled);
        if (SRC == kSrcLogits) count_culled(lp.abstained, v, abstains);
        count_culled(fp.filled, v, bits != 0u);
        word |= (unsigned long long)bits << (16 * v);
    }
    if (word != 0ull) apply_fill_word(map + cell * g.C, word, g.C, cm);
}

// ================================================================ end-of-run rendering (src/renderer.py), SURVEY 8f row 3
// The rule itself -- arg-max or thresholds pick, NumPy's row sum, class -> colour -- and the filter's tap loop are in avl_render.h.
using avl::RenderParams;

// render_bev_map (renderer.py:32-59) and render_bev_map_with_thresholds (renderer.py:131-172), one cell per thread
template <typename MapT, bool kThresholds>
__device__ __forceinline__ void render_cell(const MapT* __restrict__ map, long long ncell, int C, const RenderParams& rp,
                                            unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= ncell) return;
    unsigned char rgb[3];
    avl::row_colour(map + i * C, C, kThresholds, rp, rgb);
    out[3 * i] = rgb[0]; out[3 * i + 1] = rgb[1]; out[3 * i + 2] = rgb[2];
}

template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_render_bev(const MapT* __restrict__ map, long long ncell, int C, RenderParams rp,
                                                       unsigned char* __restrict__ out) {
    render_cell<MapT, false>(map, ncell, C, rp, out);
}

template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_render_thresholds(const MapT* __restrict__ map, long long ncell, int C, RenderParams rp,
                                                              unsigned char* __restrict__ out) {
    render_cell<MapT, true>(map, ncell, C, rp, out);
}

// apply_filter (renderer.py:175-189): cv2.filter2D with ones(3,3,float32)/9, BORDER_REFLECT_101, double accumulation
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_box_filter3(const MapT* __restrict__ src, MapT* __restrict__ dst, int Hm, int Wm, int C) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long total = (long long)Hm * Wm * C;
    if (i >= total) return;
    const int c = (int)(i % C);
    const long long cell = i / C;
    const int x = (int)(cell % Wm), y = (int)(cell / Wm);
    dst[i] = (MapT)avl::box_filter3_taps(src, Hm, Wm, C, y, x, c);
}

__global__ void __launch_bounds__(kBlock) k_colorize(const unsigned char* __restrict__ labels, int lw, int lh,
                                                     const unsigned* __restrict__ pal_packed_dummy, LutParams pal,
                                                     unsigned char* __restrict__ out, int out_w, int out_h) {
    (void)pal_packed_dummy;
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (long long)out_w * out_h) return;
    const int dx = (int)(idx % out_w), dy = (int)(idx / out_w);
    int sx = dx, sy = dy;
    if (lw != out_w) sx = min((int)__builtin_floor((double)dx * ((double)lw / (double)out_w)), lw - 1);
    if (lh != out_h) sy = min((int)__builtin_floor((double)dy * ((double)lh / (double)out_h)), lh - 1);
    const unsigned c = pal.lut[labels[(long long)sy * lw + sx]];
    out[3 * idx + 0] = (unsigned char)(c & 255u);
    out[3 * idx + 1] = (unsigned char)((c >> 8) & 255u);
    out[3 * idx + 2] = (unsigned char)((c >> 16) & 255u);
}

// ---------------------------------------------------------------- host helpers
int fill_proj(ProjParams& pp, const double* P, const double* T, double range_max, int img_w, int img_h) {
    if (!P) return avl::set_error(AVL_E_ARG, "P_host is NULL");
    if (img_w <= 0 || img_h <= 0) return avl::set_error(AVL_E_ARG, "image size %dx%d", img_w, img_h);
    memcpy(pp.P, P, sizeof(pp.P));
    pp.has_T = T ? 1 : 0;
    if (T) memcpy(pp.T, T, sizeof(pp.T));
    else memset(pp.T, 0, sizeof(pp.T));
    pp.range_max = range_max;
    pp.img_w = img_w;
    pp.img_h = img_h;
    return AVL_OK;
}

int fill_pts(PtsView& pv, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride) {
    if (n < 0) return avl::set_error(AVL_E_ARG, "n = %d", n);
    if (n > 0 && !pts) return avl::set_error(AVL_E_ARG, "pts is NULL");
    if (dtype != AVL_F32 && dtype != AVL_F64) return avl::set_error(AVL_E_ARG, "point dtype %d", dtype);
    const int64_t es = dtype == AVL_F64 ? 8 : 4;
    if (point_stride % es || comp_stride % es || point_stride <= 0 || comp_stride <= 0)
        return avl::set_error(AVL_E_ARG, "point strides %lld/%lld not multiples of %lld", (long long)point_stride,
                              (long long)comp_stride, (long long)es);
    pv.base = static_cast<const char*>(pts);
    pv.n = n;
    pv.dtype = dtype;
    pv.point_stride = point_stride;
    pv.comp_stride = comp_stride;
    pv.aos_f32 = (dtype == AVL_F32 && point_stride == 16 && comp_stride == 4 && (reinterpret_cast<uintptr_t>(pts) & 15) == 0);
    return AVL_OK;
}

// the map and its geometry alone: what a call that needs none of the grid's scratch reads (avl_ground_fill_views)
int fill_grid_map(GridParams& gp, const avl_grid* g, const uint8_t* colors, uint32_t bonus) {
    if (!g || !g->map) return avl::set_error(AVL_E_ARG, "avl_grid has NULL members");
    if (g->Hm <= 0 || g->Wm <= 0 || g->C <= 0 || g->C > AVL_MAX_MAP_CLASSES)
        return avl::set_error(AVL_E_ARG, "grid %dx%dx%d (C must be 1..%d)", g->Hm, g->Wm, g->C, AVL_MAX_MAP_CLASSES);
    if ((long long)g->Hm * g->Wm > 0x7fffffffLL) return avl::set_error(AVL_E_ARG, "grid has more than 2^31 cells");
    if (g->map_dtype != AVL_F32 && g->map_dtype != AVL_F64) return avl::set_error(AVL_E_ARG, "map dtype %d", g->map_dtype);
    if (!(g->resolution > 0.0)) return avl::set_error(AVL_E_ARG, "resolution %g", g->resolution);
    if (bonus >> g->C) return avl::set_error(AVL_E_ARG, "bonus_classes has bits beyond C");
    gp.off_x = g->off_x; gp.off_y = g->off_y; gp.b00 = g->b00; gp.b10 = g->b10; gp.resolution = g->resolution;
    gp.Hm = g->Hm; gp.Wm = g->Wm; gp.C = g->C;
    gp.bonus_classes = bonus;
    memset(gp.colors, 0, sizeof(gp.colors));
    if (colors) memcpy(gp.colors, colors, 3 * g->C);
    return AVL_OK;
}

int fill_grid(GridParams& gp, const avl_grid* g, const uint8_t* colors, uint32_t bonus) {
    if (!g || !g->map || !g->cell_mask || !g->touched || !g->counter) return avl::set_error(AVL_E_ARG, "avl_grid has NULL members");
    return fill_grid_map(gp, g, colors, bonus);
}

int fill_cm(CmParams& cm, const avl_grid* g, const double* cm_host) {
    if (!cm_host) return avl::set_error(AVL_E_ARG, "cm_host is NULL");
    memset(&cm, 0, sizeof(cm));
    memcpy(cm.cm, cm_host, sizeof(double) * g->C * g->C);
    return AVL_OK;
}

// The map's element type: launch(float()) or launch(double()) starts the kernel of that type, the launch check follows.  Every
// kernel that is a template over MapT goes through here.
template <typename Launch>
int launch_map_typed(int map_dtype, Launch&& launch) {
    if (map_dtype == AVL_F64) launch(double());
    else launch(float());
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// workgroups of a sweep over the whole grid, each round of one taking `wg_cells` cells
unsigned sweep_blocks(long long ncell, int wg_cells) {
    const long long rounds = (ncell + wg_cells - 1) / wg_cells;
    return (unsigned)(rounds < 8192 ? rounds : 8192);
}

int launch_apply(const avl_grid* g, const double* cm_host, void* rows, int rows_dtype, hipStream_t s) {
    CmParams cm;
    int rc;
    if ((rc = fill_cm(cm, g, cm_host))) return rc;
    const int dt = rows ? rows_dtype : g->map_dtype;
    if (dt != AVL_F32 && dt != AVL_F64) return avl::set_error(AVL_E_ARG, "rows dtype %d", dt);
    const int cap = g->touched_cap;
    int blocks = (cap + kBlock - 1) / kBlock;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    return launch_map_typed(dt, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_grid_apply<T>, dim3(blocks), dim3(kBlock), 0, s, static_cast<T*>(g->map), static_cast<T*>(rows), g->C, cm,
                           g->cell_mask, g->touched, g->counter);
    });
}

int launch_apply_scan(const avl_grid* g, const double* cm_host, hipStream_t s) {
    CmParams cm;
    int rc;
    if ((rc = fill_cm(cm, g, cm_host))) return rc;
    const long long ncell4 = (long long)g->Hm * g->Wm / 4;
    return launch_map_typed(g->map_dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_grid_apply_scan<T>, dim3(2048), dim3(kBlock), 0, s, static_cast<T*>(g->map), g->C, cm, g->cell_mask, ncell4);
    });
}

int launch_sweep_bytes(const avl_grid* g, const double* cm_host, unsigned bonus, hipStream_t s) {
    CmParams cm;
    int rc;
    if ((rc = fill_cm(cm, g, cm_host))) return rc;
    const long long ncell = (long long)g->Hm * g->Wm;
    unsigned char* mask = reinterpret_cast<unsigned char*>(g->cell_mask);
    return launch_map_typed(g->map_dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_grid_sweep_bytes<T>, dim3(sweep_blocks(ncell, kSweepCells)), dim3(kBlock), 0, s, static_cast<T*>(g->map), g->C,
                           bonus, cm, mask, ncell);
    });
}

// byte mask usable: class bits + bonus bits fit a byte, whole 16-byte vectors, aligned scratch
bool byte_mask_ok(const avl_grid* g, unsigned bonus) {
    const long long cells = (long long)g->Hm * g->Wm;
    return g->C + __builtin_popcount(bonus) <= 8 && cells % 16 == 0 && (reinterpret_cast<uintptr_t>(g->cell_mask) & 15) == 0;
}

// partitioned lists: geometry shared by the vote and the apply launch
struct ListGeom { int cap, wgs_per_list, apply_wgs; };
ListGeom list_geom(int n) {
    ListGeom lg;
    const int nwg = (n + kBlock - 1) / kBlock;
    const int per = (nwg + kLists - 1) / kLists;                 // vote workgroups per list
    lg.cap = per * kBlock;
    lg.wgs_per_list = per < 16 ? per : 16;                       // apply workgroups per list (grid-stride over the list)
    lg.apply_wgs = lg.wgs_per_list * kLists;
    return lg;
}
// The lists need the big counter block and room for kLists x cap entries.  Their cost grows with the cloud (returning atomics in
// the vote, rows visited in point order -- no locality -- in the apply), the sweep's is ~15 us whatever the cloud: measured 17 vs
// 22 us per frame at 120 k points on 4 M cells (config C), 54 vs 38 us at 1 M points on 16 M cells (config E).  With several views
// the lists are paid once per call, not once per view, so avl_fused_frame_views keeps the same crossover.
bool lists_fit(const avl_grid* g, int n) {
    if (g->counter_len < kListBase + 2 * kLists) return false;
    if ((long long)list_geom(n).cap * kLists > g->touched_cap) return false;
    return n <= 250000 && (long long)n * 2 <= (long long)g->Hm * g->Wm;
}
// MODE 3 reads the byte mask as well
bool use_lists(const avl_grid* g, int n, unsigned bonus) { return byte_mask_ok(g, bonus) && lists_fit(g, n); }
// Only the apply kernels return the list cursors to zero: if one did not launch (rc), reset them here so that the next frame's vote
// appends from the start of each list again.
int lists_applied(const avl_grid* g, int rc, hipStream_t s) {
    if (rc != AVL_OK) (void)hipMemsetAsync(g->counter + kListBase, 0, 2 * kLists * sizeof(int), s);
    return rc;
}
int launch_apply_lists(const avl_grid* g, const double* cm_host, unsigned bonus, int n, hipStream_t s) {
    CmParams cm;
    int rc;
    if ((rc = fill_cm(cm, g, cm_host))) return rc;
    const ListGeom lg = list_geom(n);
    unsigned char* mask = reinterpret_cast<unsigned char*>(g->cell_mask);
    return launch_map_typed(g->map_dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_grid_apply_lists<T>, dim3(lg.apply_wgs), dim3(kBlock), 0, s, static_cast<T*>(g->map), g->C, bonus, cm, mask,
                           g->touched, g->counter, lg.cap, lg.wgs_per_list);
    });
}

// list (sparse) vs sweep (dense) apply: the sweep reads Hm*Wm*4 bytes whatever the cloud; the list costs a
// returning atomic + an append per first touch.
bool use_scan(const avl_grid* g, int n, unsigned bonus) {
    const long long cells = (long long)g->Hm * g->Wm;
    if (cells % 4 != 0 || (reinterpret_cast<uintptr_t>(g->cell_mask) & 15)) return false;
    // measured (32-bit sweep): sweep wins at 120 k points on 4 M cells (25 vs 36 us) and 1 M on 16 M (73 vs 213 us); the byte
    // sweep reads a quarter of that, so it stays ahead down to much sparser clouds
    return (long long)n * (byte_mask_ok(g, bonus) ? 1024 : 128) >= cells;
}

// ---- avl_fused_frame_views: lists (sparse, lists_fit) or sweep (dense) of the word mask.  The sweep reads Hm*Wm*4 bytes whatever
// the cloud and takes any grid: it is the path for everything else.
int views_check(int n_views, const uint8_t* const* src_host) {
    if (n_views < 1) return avl::set_error(AVL_E_ARG, "n_views = %d (at least one view)", n_views);
    if (n_views > kMaxViews) return avl::set_error(AVL_E_ARG, "n_views = %d exceeds the limit of %d views", n_views, kMaxViews);
    if (!src_host) return avl::set_error(AVL_E_ARG, "src_host is NULL");
    for (int v = 0; v < n_views; ++v)
        if (!src_host[v]) return avl::set_error(AVL_E_ARG, "view %d: semantic source is NULL", v);
    return AVL_OK;
}
int views_bits_check(const avl_grid* g, uint32_t bonus) {
    const int bits = g->C + __builtin_popcount(bonus);
    if (bits > 8) return avl::set_error(AVL_E_ARG, "C + popcount(bonus_classes) = %d vote bits per view, the views mask holds 8", bits);
    return AVL_OK;
}

// The semantic source of a fused frame as its entry point hands it on: byte images as the caller gave them (fill_frame checks
// them), or the logits in kernel-argument form (logits_source has checked them).
struct VoteSource {
    bool logits;
    int kind;                        // bytes: AVL_SRC_RGB or AVL_SRC_CLASSMAP
    const uint8_t* const* bytes;     // bytes: one image per view
    LogitsParams lp;
    int w, h;
};

// What every fused frame takes, validated and in kernel-argument form.  Everything here is refused before the empty cloud returns;
// touched_cap matters only to a cloud that votes.  The logits stand where a class map stands: a source, its size and a LUT.
struct FrameArgs { PtsView pv; ProjParams pp; GridParams gp; LutParams lut; };
// what a frame and a ground fill refuse of a semantic source alike; the LUT of a class-map or logits source
int fill_source(LutParams& lut, const VoteSource& src, int img_w, int img_h, const uint32_t* lut_host, const uint8_t* label_colors_host,
                const double* cm_host) {
    const int src_kind = src.logits ? AVL_SRC_CLASSMAP : src.kind;
    const void* first = src.logits ? static_cast<const void*>(src.lp.logits[0]) : src.bytes[0];   // the only or first view's
    AVL_REQUIRE(src_kind == AVL_SRC_RGB || src_kind == AVL_SRC_CLASSMAP, "src_kind %d", src_kind);
    AVL_REQUIRE(first && src.w > 0 && src.h > 0, "bad semantic source");
    AVL_REQUIRE(cm_host, "cm_host is NULL");
    memset(&lut, 0, sizeof(lut));
    if (src_kind == AVL_SRC_RGB) {
        AVL_REQUIRE(label_colors_host, "label_colors_host is NULL");
        AVL_REQUIRE(src.w == img_w && src.h == img_h, "RGB source must be %dx%d", img_w, img_h);
    } else {
        AVL_REQUIRE(lut_host, "lut_host is NULL");
        memcpy(lut.lut, lut_host, sizeof(lut.lut));
    }
    return AVL_OK;
}
int fill_frame(FrameArgs& f, const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
               const double* P_host, const double* T_host, double range_max, const VoteSource& src, int img_w, int img_h,
               const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host, uint32_t bonus) {
    int rc;
    if ((rc = fill_pts(f.pv, pts, n, dtype, point_stride, comp_stride))) return rc;
    if ((rc = fill_proj(f.pp, P_host, T_host, range_max, img_w, img_h))) return rc;
    if ((rc = fill_grid(f.gp, g, label_colors_host, bonus))) return rc;
    if ((rc = fill_source(f.lut, src, img_w, img_h, lut_host, label_colors_host, cm_host))) return rc;
    if (n > 0) AVL_REQUIRE(g->touched_cap >= (n < g->Hm * g->Wm ? n : g->Hm * g->Wm), "touched_cap %d too small", g->touched_cap);
    return AVL_OK;
}

void fill_views(ViewsParams& vp, const FrameArgs& f, int n_views, const double* P_host, const uint8_t* const* src_host) {
    memset(&vp, 0, sizeof(vp));
    memcpy(vp.P, P_host, sizeof(double) * 12 * n_views);
    memcpy(vp.T, f.pp.T, sizeof(vp.T));
    for (int v = 0; v < n_views; ++v) vp.src[v] = src_host ? src_host[v] : nullptr;
    vp.range_max = f.pp.range_max;
    vp.has_T = f.pp.has_T;
    vp.n_views = n_views;
    vp.img_w = f.pp.img_w;
    vp.img_h = f.pp.img_h;
}

// ---- occlusion culling: an avl_occlusion validated for n_views views of img_w x img_h (host only) and in kernel-argument form
long long occl_cells(int img_w, int img_h, int s) { return (long long)((img_w + s - 1) / s) * ((img_h + s - 1) / s); }

int occl_fill(OcclParams& oc, const avl_occlusion* occl, int img_w, int img_h, int n_views) {
    AVL_REQUIRE(occl, "occl is NULL");
    AVL_REQUIRE(occl->cell_px >= 1 && occl->cell_px <= 64, "occlusion cell_px = %d (1..64)", occl->cell_px);
    AVL_REQUIRE(occl->radius >= 0 && occl->radius <= 2, "occlusion radius = %d (0..2)", occl->radius);
    AVL_REQUIRE(occl->rel_tol >= 0.0, "occlusion rel_tol = %g (must be >= 0)", occl->rel_tol);     // a NaN fails the comparison too
    AVL_REQUIRE(occl->abs_tol >= 0.0, "occlusion abs_tol = %g (must be >= 0)", occl->abs_tol);
    AVL_REQUIRE(img_w > 0 && img_h > 0 && n_views >= 1 && n_views <= kMaxViews, "occlusion: %d views of %dx%d", n_views, img_w, img_h);
    const long long words = occl_cells(img_w, img_h, occl->cell_px) * n_views;
    AVL_REQUIRE(occl->depth, "occlusion depth scratch is NULL");
    AVL_REQUIRE(occl->depth_words >= words, "occlusion depth scratch holds %lld words, %lld needed", (long long)occl->depth_words, words);
    AVL_REQUIRE(words * 4 <= 0x7fffffffLL, "occlusion depth buffer of %lld words is too large", words);
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(occl->depth) & 3) == 0, "occlusion depth scratch is not 4-byte aligned");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(occl->culled) & 3) == 0, "occlusion culled counts are not 4-byte aligned");
    oc.depth = occl->depth;
    oc.culled = occl->culled;
    oc.k = 1.0 + occl->rel_tol;
    oc.abs_tol = occl->abs_tol;
    oc.s = occl->cell_px;
    oc.R = occl->radius;
    oc.Wc = (img_w + oc.s - 1) / oc.s;
    oc.Hc = (img_h + oc.s - 1) / oc.s;
    return AVL_OK;
}

// every depth cell back to empty (`depth`) and the culled counts to zero: what makes a call independent of the last
int occl_reset(const OcclParams& oc, int n_views, bool depth, hipStream_t s) {
    if (depth) AVL_HIP_CHECK(hipMemsetAsync(oc.depth, 0xff, sizeof(unsigned) * (size_t)n_views * oc.Hc * oc.Wc, s));
    if (oc.culled) AVL_HIP_CHECK(hipMemsetAsync(oc.culled, 0, sizeof(int) * n_views, s));
    return AVL_OK;
}

int launch_occl_depth(const PtsView& pv, const ViewsParams& vp, const OcclParams& oc, hipStream_t s) {
    hipLaunchKernelGGL(k_occl_depth, dim3((pv.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pv, vp, oc);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// ---- logits: an avl_point_logits validated for n_views views (host only) and in kernel-argument form
int logits_fill(LogitsParams& lp, const avl_point_logits* pl, int n_views) {
    AVL_REQUIRE(pl, "avl_point_logits is NULL");
    AVL_REQUIRE(n_views >= 1, "n_views = %d (at least one view)", n_views);
    AVL_REQUIRE(n_views <= kMaxViews, "n_views = %d exceeds the limit of %d views", n_views, kMaxViews);
    AVL_REQUIRE(pl->h > 0 && pl->w > 0, "logits of %dx%d pixels", pl->w, pl->h);
    AVL_REQUIRE(pl->K >= 1 && pl->K <= 254, "logits K = %d (1..254)", pl->K);
    AVL_REQUIRE(pl->ld >= pl->K, "logits ld = %lld < K = %d", (long long)pl->ld, pl->K);
    AVL_REQUIRE(pl->ld <= (1ll << 61) / pl->h / pl->w, "logits of %dx%d pixels x ld %lld are too large", pl->w, pl->h, (long long)pl->ld);
    AVL_REQUIRE(pl->net_h > 0 && pl->net_w > 0, "logits net size %dx%d", pl->net_w, pl->net_h);
    AVL_REQUIRE(pl->min_margin >= 0.f, "logits min_margin = %g (must be >= 0)", (double)pl->min_margin);      // a NaN fails the comparison too
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(pl->abstained) & 3) == 0, "logits abstained counts are not 4-byte aligned");
    memset(&lp, 0, sizeof(lp));
    for (int v = 0; v < n_views; ++v) {
        AVL_REQUIRE(pl->logits[v], "view %d: logits are NULL", v);
        AVL_REQUIRE((reinterpret_cast<uintptr_t>(pl->logits[v]) & 3) == 0, "view %d: logits are not 4-byte aligned", v);
        lp.logits[v] = pl->logits[v];
    }
    lp.abstained = pl->abstained;
    lp.ld = pl->ld;
    lp.h = pl->h; lp.w = pl->w; lp.K = pl->K; lp.net_h = pl->net_h; lp.net_w = pl->net_w;
    lp.sy = pl->net_h > 1 ? (float)(pl->h - 1) / (float)(pl->net_h - 1) : 0.f;          // as avl_seg_eval_full_res (seg_head.hip)
    lp.sx = pl->net_w > 1 ? (float)(pl->w - 1) / (float)(pl->net_w - 1) : 0.f;
    lp.min_margin = pl->min_margin;
    return AVL_OK;
}

int logits_reset(const LogitsParams& lp, int n_views, hipStream_t s) {
    if (lp.abstained) AVL_HIP_CHECK(hipMemsetAsync(lp.abstained, 0, sizeof(int) * n_views, s));
    return AVL_OK;
}

// the source of the byte and of the logits entry points
VoteSource bytes_source(int src_kind, const uint8_t* const* src_host, int src_w, int src_h) {
    VoteSource src = {};
    src.kind = src_kind; src.bytes = src_host; src.w = src_w; src.h = src_h;
    return src;
}
int logits_source(VoteSource& src, const avl_point_logits* pl, int n_views) {
    src = {};
    src.logits = true;
    int rc;
    if ((rc = logits_fill(src.lp, pl, n_views))) return rc;
    src.w = pl->w; src.h = pl->h;
    return AVL_OK;
}

// ---- height: an avl_height validated (host only) and in kernel-argument form.  `g` NULL (avl_point_heights): the plane and the
// slope alone, whatever `gate` says; else the gate's fields when it is on, and the layer's for a grid of g's size.
int height_plane_fill(HeightParams& hp, const avl_height* ht) {
    for (int k = 0; k < 4; ++k) AVL_REQUIRE(std::isfinite(ht->plane[k]), "height plane coefficient %d = %g", k, ht->plane[k]);
    AVL_REQUIRE(ht->plane[2] > 0.0, "height plane with c = %g (the normal must point up: c > 0)", ht->plane[2]);
    AVL_REQUIRE(ht->slope >= 0.0 && std::isfinite(ht->slope), "height slope = %g (finite, >= 0)", ht->slope);   // a NaN fails the comparison too
    memcpy(hp.plane, ht->plane, sizeof(hp.plane));
    hp.slope = ht->slope;
    return AVL_OK;
}
int height_fill(HeightParams& hp, const avl_height* ht, const avl_grid* g) {
    AVL_REQUIRE(ht, "avl_height is NULL");
    memset(&hp, 0, sizeof(hp));
    int rc;
    if (!g) return height_plane_fill(hp, ht);
    AVL_REQUIRE(ht->gate == 0 || ht->gate == 1, "height gate = %d (0 or 1)", ht->gate);
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(ht->gated) & 3) == 0, "height gated counts are not 4-byte aligned");
    if (ht->gate) {
        if ((rc = height_plane_fill(hp, ht))) return rc;
        for (int i = 0; i < g->C; ++i) {
            AVL_REQUIRE(ht->min_m[i] == ht->min_m[i] && ht->max_m[i] == ht->max_m[i], "height bound of class %d is a NaN", i);
            AVL_REQUIRE(ht->min_m[i] <= ht->max_m[i], "height bounds of class %d: min %g > max %g", i, ht->min_m[i], ht->max_m[i]);
            hp.min_m[i] = ht->min_m[i];
            hp.max_m[i] = ht->max_m[i];
        }
        hp.gate = 1;
        hp.gated = ht->gated;
    }
    const int ptrs = (ht->elev_sum != nullptr) + (ht->elev_cnt != nullptr) + (ht->elev_min != nullptr) + (ht->elev_max != nullptr);
    AVL_REQUIRE(ptrs == 0 || ptrs == 4, "elevation layer with %d of its 4 arrays", ptrs);
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(ht->elev_sum) & 7) == 0, "elevation sum is not 8-byte aligned");
    AVL_REQUIRE(((reinterpret_cast<uintptr_t>(ht->elev_cnt) | reinterpret_cast<uintptr_t>(ht->elev_min) |
                  reinterpret_cast<uintptr_t>(ht->elev_max)) & 3) == 0, "elevation count, minimum or maximum is not 4-byte aligned");
    if (ptrs == 4 || ht->elev_classes != 0u) {
        AVL_REQUIRE(ht->quantum > 0.0 && std::isfinite(ht->quantum), "elevation quantum = %g (finite, > 0)", ht->quantum);
        AVL_REQUIRE(!(ht->elev_classes >> g->C), "elev_classes has bits beyond C");
    }
    if (ptrs == 4 && ht->elev_classes != 0u) {
        hp.elev_sum = reinterpret_cast<unsigned long long*>(ht->elev_sum);
        hp.elev_cnt = ht->elev_cnt; hp.elev_min = ht->elev_min; hp.elev_max = ht->elev_max;
        hp.elev_classes = ht->elev_classes;
        hp.quantum = ht->quantum;
    }
    return AVL_OK;
}

// ---- the vote.  A runtime value in [0, N) as a compile-time one: f(std::integral_constant<int, v>()); the template arguments of
// the two vote kernels go through here, as the map's element type goes through launch_map_typed.
template <int N, typename F>
void with_constant(int v, F&& f) {
    if constexpr (N == 1) f(std::integral_constant<int, 0>());
    else if (v == N - 1) f(std::integral_constant<int, N - 1>());
    else with_constant<N - 1>(v, f);
}

// `oc` is that of `occl`, or all zero without one
int launch_fused_vote(const FrameArgs& f, const VoteSource& src, int mode, bool occl, const OcclParams& oc, const avl_grid* g, int list_cap,
                      hipStream_t s) {
    const dim3 grid((f.pv.n + kBlock - 1) / kBlock), block(kBlock);
    const uint8_t* bytes = src.logits ? nullptr : src.bytes[0];
    with_constant<3>(src.logits ? kSrcLogits : src.kind, [&](auto S) {
        with_constant<4>(mode, [&](auto M) {
            with_constant<2>(occl, [&](auto O) {
                hipLaunchKernelGGL((k_fused_vote<decltype(S)::value, decltype(M)::value, decltype(O)::value>), grid, block, 0, s, f.pv, f.pp,
                                   f.gp, bytes, src.w, src.h, src.lp, f.lut, g->cell_mask, g->touched, g->counter, list_cap, oc);
            });
        });
    });
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

int launch_views_vote(const FrameArgs& f, const ViewsParams& vp, const VoteSource& src, bool lists, bool occl, const OcclParams& oc,
                      const avl_grid* g, int list_cap, hipStream_t s) {
    const dim3 grid((f.pv.n + kBlock - 1) / kBlock), block(kBlock);
    with_constant<3>(src.logits ? kSrcLogits : src.kind, [&](auto S) {
        with_constant<2>(lists, [&](auto L) {
            with_constant<2>(occl, [&](auto O) {
                hipLaunchKernelGGL((k_views_vote<decltype(S)::value, decltype(L)::value, decltype(O)::value>), grid, block, 0, s, f.pv, vp,
                                   f.gp, src.w, src.h, src.lp, f.lut, g->cell_mask, g->touched, g->counter, list_cap, oc);
            });
        });
    });
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// the height forms of the two launches above: one kernel per SRC and MODE / LISTS, the occlusion test a run-time branch on oc.depth
int launch_fused_vote_height(const FrameArgs& f, const VoteSource& src, int mode, const OcclParams& oc, const HeightParams& hp,
                             const avl_grid* g, int list_cap, hipStream_t s) {
    const dim3 grid((f.pv.n + kBlock - 1) / kBlock), block(kBlock);
    const uint8_t* bytes = src.logits ? nullptr : src.bytes[0];
    with_constant<3>(src.logits ? kSrcLogits : src.kind, [&](auto S) {
        with_constant<4>(mode, [&](auto M) {
            hipLaunchKernelGGL((k_fused_vote_height<decltype(S)::value, decltype(M)::value>), grid, block, 0, s, f.pv, f.pp, f.gp, bytes,
                               src.w, src.h, src.lp, f.lut, g->cell_mask, g->touched, g->counter, list_cap, oc, hp);
        });
    });
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

int launch_views_vote_height(const FrameArgs& f, const ViewsParams& vp, const VoteSource& src, bool lists, const OcclParams& oc,
                             const HeightParams& hp, const avl_grid* g, int list_cap, hipStream_t s) {
    const dim3 grid((f.pv.n + kBlock - 1) / kBlock), block(kBlock);
    with_constant<3>(src.logits ? kSrcLogits : src.kind, [&](auto S) {
        with_constant<2>(lists, [&](auto L) {
            hipLaunchKernelGGL((k_views_vote_height<decltype(S)::value, decltype(L)::value>), grid, block, 0, s, f.pv, vp, f.gp, src.w,
                               src.h, src.lp, f.lut, g->cell_mask, g->touched, g->counter, list_cap, oc, hp);
        });
    });
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// ---- the apply.  What follows the vote kernel of path `mode` (avl_fused_frame_path) for a cloud of n points
int apply_frame(const avl_grid* g, const double* cm_host, uint32_t bonus_classes, int mode, int n, hipStream_t s) {
    if (mode == 3) return lists_applied(g, launch_apply_lists(g, cm_host, bonus_classes, n, s), s);
    if (mode == 2) return launch_sweep_bytes(g, cm_host, bonus_classes, s);
    return mode == 1 ? launch_apply_scan(g, cm_host, s) : launch_apply(g, cm_host, nullptr, 0, s);
}

// what follows the views vote kernel: the lists' apply (path 4) or the sweep of the word mask (path 5)
int apply_views(const avl_grid* g, const double* cm_host, uint32_t bonus_classes, bool lists, const ListGeom& lg, hipStream_t s) {
    CmParams cm;
    int rc;
    if ((rc = fill_cm(cm, g, cm_host))) return rc;
    const dim3 block(kBlock);
    if (lists)
        return lists_applied(g, launch_map_typed(g->map_dtype, [&](auto t) {
            typedef decltype(t) T;
            hipLaunchKernelGGL(k_views_apply_lists<T>, dim3(lg.apply_wgs), block, 0, s, static_cast<T*>(g->map), g->C, bonus_classes, cm,
                               g->cell_mask, g->touched, g->counter, lg.cap, lg.wgs_per_list);
        }), s);
    const long long ncell = (long long)g->Hm * g->Wm;
    const int vec = (reinterpret_cast<uintptr_t>(g->cell_mask) & 15) == 0;
    return launch_map_typed(g->map_dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_views_sweep_words<T>, dim3(sweep_blocks(ncell, kViewsSweepCells)), block, 0, s, static_cast<T*>(g->map), g->C,
                           bonus_classes, cm, g->cell_mask, ncell, vec);
    });
}

// ---- the frame.  What every fused frame does once fill_frame has accepted it, whatever its source and arity: the resets, the
// path from n, with `occl` the depth pass, the vote, the apply.  The apply and sweep kernels know nothing of source or culling.
int run_frame(const avl_grid* g, const FrameArgs& f, int n_views, const double* P_host, const VoteSource& src, const double* cm_host,
              uint32_t bonus_classes, const avl_occlusion* occl, const HeightParams* hp, void* stream) {
    const int n = f.pv.n;
    OcclParams oc;
    int rc;
    memset(&oc, 0, sizeof(oc));
    if (occl && (rc = occl_fill(oc, occl, f.pp.img_w, f.pp.img_h, n_views))) return rc;
    hipStream_t s = avl::as_stream(stream);
    if (src.logits && (rc = logits_reset(src.lp, n_views, s))) return rc;
    if (hp && hp->gated) AVL_HIP_CHECK(hipMemsetAsync(hp->gated, 0, sizeof(int) * n_views, s));
    if (n == 0) return occl ? occl_reset(oc, n_views, false, s) : AVL_OK;         // an empty cloud resets the counts, not the depth buffer
    const int path = n_views == 1 ? avl_fused_frame_path(g, n, bonus_classes) : (lists_fit(g, n) ? 4 : 5);
    if (path < 0) return path;
    ViewsParams vp;
    fill_views(vp, f, n_views, P_host, src.logits ? nullptr : src.bytes);
    if (occl) {
        if ((rc = occl_reset(oc, n_views, true, s))) return rc;
        if ((rc = launch_occl_depth(f.pv, vp, oc, s))) return rc;
    }
    if (path == 0) AVL_HIP_CHECK(hipMemsetAsync(g->counter, 0, 16, s));      // only the single touched-list path counts there
    const ListGeom lg = list_geom(n);
    if (n_views == 1) {
        if ((rc = hp ? launch_fused_vote_height(f, src, path, oc, *hp, g, lg.cap, s)
                     : launch_fused_vote(f, src, path, occl != nullptr, oc, g, lg.cap, s)))
            return rc;
        return apply_frame(g, cm_host, bonus_classes, path, n, s);
    }
    if ((rc = hp ? launch_views_vote_height(f, vp, src, path == 4, oc, *hp, g, lg.cap, s)
                 : launch_views_vote(f, vp, src, path == 4, occl != nullptr, oc, g, lg.cap, s)))
        return rc;
    return apply_views(g, cm_host, bonus_classes, path == 4, lg, s);
}

// one camera: avl_fused_frame, _occl (`occl`) and _logits (`src`)
int fused_frame(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, const double* P_host,
                const double* T_host, double range_max, const VoteSource& src, int img_w, int img_h, const uint32_t* lut_host,
                const uint8_t* label_colors_host, const double* cm_host, uint32_t bonus_classes, const avl_occlusion* occl, void* stream,
                const avl_height* ht = nullptr) {
    FrameArgs f;
    HeightParams hp;
    int rc;
    if ((rc = fill_frame(f, g, pts, n, dtype, point_stride, comp_stride, P_host, T_host, range_max, src, img_w, img_h, lut_host,
                         label_colors_host, cm_host, bonus_classes)))
        return rc;
    if (ht && (rc = height_fill(hp, ht, g))) return rc;
    return run_frame(g, f, 1, P_host, src, cm_host, bonus_classes, occl, ht ? &hp : nullptr, stream);
}

// several cameras: avl_fused_frame_views, _views_occl and _views_logits; one view is the single camera's frame
int fused_frame_views(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, int n_views,
                      const double* P_host, const double* T_host, double range_max, const VoteSource& src, int img_w, int img_h,
                      const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host, uint32_t bonus_classes,
                      const avl_occlusion* occl, void* stream, const avl_height* ht = nullptr) {
    if (n_views == 1)
        return fused_frame(g, pts, n, dtype, point_stride, comp_stride, P_host, T_host, range_max, src, img_w, img_h, lut_host,
                           label_colors_host, cm_host, bonus_classes, occl, stream, ht);
    FrameArgs f;
    HeightParams hp;
    int rc;
    if ((rc = fill_frame(f, g, pts, n, dtype, point_stride, comp_stride, P_host, T_host, range_max, src, img_w, img_h, lut_host,
                         label_colors_host, cm_host, bonus_classes)))
        return rc;
    if ((rc = views_bits_check(g, bonus_classes))) return rc;
    if (ht && (rc = height_fill(hp, ht, g))) return rc;
    return run_frame(g, f, n_views, P_host, src, cm_host, bonus_classes, occl, ht ? &hp : nullptr, stream);
}

// ---- the ground fill: avl_ground_fill_views (bytes) and _logits.  Everything is refused before any GPU work; the window is clipped
// to the grid here, so the kernel's cells are all on it.
int ground_fill(const avl_grid* g, const avl_ground_fill* gf, int n_views, const double* P_host, const double* T_host, const VoteSource& src,
                int img_w, int img_h, const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host,
                const avl_occlusion* occl, void* stream) {
    FrameArgs f;
    FillParams fp;
    CmParams cm;
    OcclParams oc;
    int rc;
    AVL_REQUIRE(gf, "avl_ground_fill is NULL");
    AVL_REQUIRE(n_views >= 1, "n_views = %d (at least one view)", n_views);
    AVL_REQUIRE(n_views <= kMaxViews, "n_views = %d exceeds the limit of %d views", n_views, kMaxViews);
    AVL_REQUIRE(gf->range_max > 0.0, "ground fill range_max = %g (must be > 0)", gf->range_max);            // a NaN fails the comparison too
    if ((rc = fill_proj(f.pp, P_host, T_host, gf->range_max, img_w, img_h))) return rc;
    if ((rc = fill_grid_map(f.gp, g, label_colors_host, 0u))) return rc;
    if ((rc = fill_source(f.lut, src, img_w, img_h, lut_host, label_colors_host, cm_host))) return rc;
    if ((rc = fill_cm(cm, g, cm_host))) return rc;
    AVL_REQUIRE(gf->h >= 0 && gf->w >= 0, "ground fill window of %d x %d cells", gf->h, gf->w);
    AVL_REQUIRE((long long)gf->h * gf->w <= 0x7fffffffLL, "ground fill window of %d x %d cells has more than 2^31", gf->h, gf->w);
    for (int k = 0; k < 4; ++k) AVL_REQUIRE(std::isfinite(gf->plane[k]), "ground plane coefficient %d = %g", k, gf->plane[k]);
    AVL_REQUIRE(gf->plane[2] != 0.0, "ground plane with c = 0 is vertical");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(gf->filled) & 3) == 0, "ground fill filled counts are not 4-byte aligned");
    memset(&oc, 0, sizeof(oc));
    if (occl && (rc = occl_fill(oc, occl, img_w, img_h, n_views))) return rc;
    hipStream_t s = avl::as_stream(stream);
    if (src.logits && (rc = logits_reset(src.lp, n_views, s))) return rc;
    if (occl && (rc = occl_reset(oc, n_views, false, s))) return rc;             // the counts, not the buffer of real points
    if (gf->filled) AVL_HIP_CHECK(hipMemsetAsync(gf->filled, 0, sizeof(int) * n_views, s));
    const long long x0 = gf->x0 > 0 ? gf->x0 : 0, y0 = gf->y0 > 0 ? gf->y0 : 0;
    const long long x1 = std::min<long long>((long long)gf->x0 + gf->h, g->Hm), y1 = std::min<long long>((long long)gf->y0 + gf->w, g->Wm);
    if (x1 <= x0 || y1 <= y0) return AVL_OK;                                      // a window wholly off the grid
    memcpy(fp.plane, gf->plane, sizeof(fp.plane));
    fp.x0 = (int)x0; fp.y0 = (int)y0; fp.h = (int)(x1 - x0); fp.w = (int)(y1 - y0);
    fp.class_mask = gf->class_mask;
    fp.filled = gf->filled;
    ViewsParams vp;
    fill_views(vp, f, n_views, P_host, src.logits ? nullptr : src.bytes);
    const dim3 grid((unsigned)(((long long)fp.h * fp.w + kBlock - 1) / kBlock)), block(kBlock);
    return launch_map_typed(g->map_dtype, [&](auto t) {
        typedef decltype(t) T;
        with_constant<3>(src.logits ? kSrcLogits : src.kind, [&](auto S) {
            with_constant<2>(occl != nullptr, [&](auto O) {
                hipLaunchKernelGGL((k_ground_fill<decltype(S)::value, decltype(O)::value, T>), grid, block, 0, s, static_cast<T*>(g->map), vp,
                                   f.gp, fp, src.w, src.h, src.lp, f.lut, cm, oc);
            });
        });
    });
}

}  // namespace

// ============================================================================ C ABI
extern "C" int avl_project_points(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                  const double* P_host, const double* T_host, double range_max, int img_w, int img_h,
                                  int32_t* out_ixy, uint8_t* out_mask, void* stream) {
    PtsView pv;
    ProjParams pp;
    int rc;
    if ((rc = fill_pts(pv, pts, n, dtype, point_stride, comp_stride))) return rc;
    if ((rc = fill_proj(pp, P_host, T_host, range_max, img_w, img_h))) return rc;
    if (n == 0) return AVL_OK;
    hipLaunchKernelGGL(k_project_points, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, avl::as_stream(stream), pv, pp,
                       out_ixy, out_mask);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int64_t avl_project_pcd_scratch_bytes(int n) {
    if (n < 0) return 0;
    const int64_t nb = (n + kBlock - 1) / kBlock;
    return (int64_t)sizeof(int) * ((int64_t)n + nb + 16);
}

extern "C" int avl_project_pcd(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                               const double* P_host, const double* T_host, double range_max, const uint8_t* image,
                               int img_w, int img_h, double* out_pcd, uint8_t* out_label, int64_t out_ld,
                               int32_t* out_count, void* scratch, void* stream) {
    PtsView pv;
    ProjParams pp;
    int rc;
    if ((rc = fill_pts(pv, pts, n, dtype, point_stride, comp_stride))) return rc;
    if ((rc = fill_proj(pp, P_host, T_host, range_max, img_w, img_h))) return rc;
    AVL_REQUIRE(out_count, "out_count is NULL");
    hipStream_t s = avl::as_stream(stream);
    if (n == 0) {
        AVL_HIP_CHECK(hipMemsetAsync(out_count, 0, sizeof(int), s));
        return AVL_OK;
    }
    AVL_REQUIRE(image && out_pcd && out_label && scratch, "NULL buffer");
    AVL_REQUIRE(out_ld >= n, "out_ld %lld < n %d", (long long)out_ld, n);
    AVL_REQUIRE((long long)img_w * img_h < 0x7fffffffLL, "image too large");
    const int nb = (n + kBlock - 1) / kBlock;
    int* pix = static_cast<int*>(scratch);
    int* block_count = pix + n;
    hipLaunchKernelGGL(k_pcd_mask, dim3(nb), dim3(kBlock), 0, s, pv, pp, pix, block_count);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, block_count, nb, out_count);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pcd_scatter, dim3(nb), dim3(kBlock), 0, s, pv, pix, block_count, image, out_pcd, out_label,
                       (long long)out_ld);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_vote_points(const avl_grid* g, const double* pcd, const uint8_t* label, int64_t ld, int m_host,
                               const int32_t* m_dev, const uint8_t* label_colors_host, uint32_t bonus_classes,
                               void* stream) {
    GridParams gp;
    int rc;
    AVL_REQUIRE(label_colors_host, "label_colors_host is NULL");
    if ((rc = fill_grid(gp, g, label_colors_host, bonus_classes))) return rc;
    AVL_REQUIRE(m_host >= 0, "m = %d", m_host);
    hipStream_t s = avl::as_stream(stream);
    AVL_HIP_CHECK(hipMemsetAsync(g->counter, 0, 16, s));
    if (m_host == 0) return AVL_OK;
    AVL_REQUIRE(pcd && label, "NULL buffer");
    AVL_REQUIRE(ld >= m_host, "ld %lld < m %d", (long long)ld, m_host);
    AVL_REQUIRE(g->touched_cap >= (m_host < g->Hm * g->Wm ? m_host : g->Hm * g->Wm), "touched_cap %d too small", g->touched_cap);
    hipLaunchKernelGGL(k_vote_labelled, dim3((m_host + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pcd, label, (long long)ld,
                       m_host, m_dev, gp, g->cell_mask, g->touched, g->counter);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_grid_apply(const avl_grid* g, const double* cm_host, void* rows, int rows_dtype, void* stream) {
    AVL_REQUIRE(g && g->cell_mask && g->touched && g->counter && (rows || g->map), "avl_grid has NULL members");
    AVL_REQUIRE(g->C > 0 && g->C <= AVL_MAX_MAP_CLASSES, "C = %d", g->C);
    return launch_apply(g, cm_host, rows, rows_dtype, avl::as_stream(stream));
}

extern "C" int avl_update_map(const avl_grid* g, const double* pcd, const uint8_t* label, int64_t ld, int m_host,
                              const int32_t* m_dev, const uint8_t* label_colors_host, const double* cm_host,
                              uint32_t bonus_classes, void* stream) {
    AVL_REQUIRE(cm_host, "cm_host is NULL");
    int rc = avl_vote_points(g, pcd, label, ld, m_host, m_dev, label_colors_host, bonus_classes, stream);
    if (rc) return rc;
    return launch_apply(g, cm_host, nullptr, 0, avl::as_stream(stream));
}

extern "C" int avl_fused_frame_path(const avl_grid* g, int n, uint32_t bonus_classes) {
    GridParams gp;
    int rc;
    if ((rc = fill_grid(gp, g, nullptr, bonus_classes))) return rc;
    AVL_REQUIRE(n >= 0, "n = %d", n);
    if (use_lists(g, n, bonus_classes)) return 3;
    if (!use_scan(g, n, bonus_classes)) return 0;
    return byte_mask_ok(g, bonus_classes) ? 2 : 1;
}

extern "C" int avl_fused_frame_views_path(const avl_grid* g, int n, int n_views, uint32_t bonus_classes) {
    AVL_REQUIRE(n_views >= 1, "n_views = %d (at least one view)", n_views);
    AVL_REQUIRE(n_views <= kMaxViews, "n_views = %d exceeds the limit of %d views", n_views, kMaxViews);
    if (n_views == 1) return avl_fused_frame_path(g, n, bonus_classes);
    GridParams gp;
    int rc;
    if ((rc = fill_grid(gp, g, nullptr, bonus_classes))) return rc;
    if ((rc = views_bits_check(g, bonus_classes))) return rc;
    AVL_REQUIRE(n >= 0, "n = %d", n);
    return lists_fit(g, n) ? 4 : 5;
}

// The six fused frames: each puts its semantic source into a VoteSource and goes through fused_frame / fused_frame_views.
extern "C" int avl_fused_frame(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride,
                               int64_t comp_stride, const double* P_host, const double* T_host, double range_max,
                               int src_kind, const uint8_t* src, int src_w, int src_h, int img_w, int img_h,
                               const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host,
                               uint32_t bonus_classes, void* stream) {
    return fused_frame(g, pts, n, dtype, point_stride, comp_stride, P_host, T_host, range_max, bytes_source(src_kind, &src, src_w, src_h),
                       img_w, img_h, lut_host, label_colors_host, cm_host, bonus_classes, nullptr, stream);
}

extern "C" int avl_fused_frame_occl(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                    const double* P_host, const double* T_host, double range_max, int src_kind, const uint8_t* src,
                                    int src_w, int src_h, int img_w, int img_h, const uint32_t* lut_host, const uint8_t* label_colors_host,
                                    const double* cm_host, uint32_t bonus_classes, const avl_occlusion* occl, void* stream) {
    AVL_REQUIRE(occl, "occl is NULL");
    return fused_frame(g, pts, n, dtype, point_stride, comp_stride, P_host, T_host, range_max, bytes_source(src_kind, &src, src_w, src_h),
                       img_w, img_h, lut_host, label_colors_host, cm_host, bonus_classes, occl, stream);
}

extern "C" int avl_fused_frame_logits(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                      const double* P_host, const double* T_host, double range_max, const avl_point_logits* pl,
                                      int img_w, int img_h, const uint32_t* lut_host, const double* cm_host, uint32_t bonus_classes,
                                      const avl_occlusion* occl, void* stream) {
    VoteSource src;
    int rc;
    if ((rc = logits_source(src, pl, 1))) return rc;
    return fused_frame(g, pts, n, dtype, point_stride, comp_stride, P_host, T_host, range_max, src, img_w, img_h, lut_host, nullptr, cm_host,
                       bonus_classes, occl, stream);
}

extern "C" int avl_fused_frame_views(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                     int n_views, const double* P_host, const double* T_host, double range_max, int src_kind,
                                     const uint8_t* const* src_host, int src_w, int src_h, int img_w, int img_h,
                                     const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host,
                                     uint32_t bonus_classes, void* stream) {
    int rc;
    if ((rc = views_check(n_views, src_host))) return rc;
    return fused_frame_views(g, pts, n, dtype, point_stride, comp_stride, n_views, P_host, T_host, range_max,
                             bytes_source(src_kind, src_host, src_w, src_h), img_w, img_h, lut_host, label_colors_host, cm_host, bonus_classes,
                             nullptr, stream);
}

extern "C" int avl_fused_frame_views_occl(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                          int n_views, const double* P_host, const double* T_host, double range_max, int src_kind,
                                          const uint8_t* const* src_host, int src_w, int src_h, int img_w, int img_h,
                                          const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host,
                                          uint32_t bonus_classes, const avl_occlusion* occl, void* stream) {
    AVL_REQUIRE(occl, "occl is NULL");
    int rc;
    if ((rc = views_check(n_views, src_host))) return rc;
    return fused_frame_views(g, pts, n, dtype, point_stride, comp_stride, n_views, P_host, T_host, range_max,
                             bytes_source(src_kind, src_host, src_w, src_h), img_w, img_h, lut_host, label_colors_host, cm_host, bonus_classes,
                             occl, stream);
}

extern "C" int avl_fused_frame_views_logits(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                            int n_views, const double* P_host, const double* T_host, double range_max,
                                            const avl_point_logits* pl, int img_w, int img_h, const uint32_t* lut_host,
                                            const double* cm_host, uint32_t bonus_classes, const avl_occlusion* occl, void* stream) {
    VoteSource src;
    int rc;
    if ((rc = logits_source(src, pl, n_views))) return rc;
    return fused_frame_views(g, pts, n, dtype, point_stride, comp_stride, n_views, P_host, T_host, range_max, src, img_w, img_h, lut_host,
                             nullptr, cm_host, bonus_classes, occl, stream);
}

extern "C" int avl_fused_frame_views_height(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                            int n_views, const double* P_host, const double* T_host, double range_max, int src_kind,
                                            const uint8_t* const* src_host, int src_w, int src_h, int img_w, int img_h,
                                            const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host,
                                            uint32_t bonus_classes, const avl_point_logits* pl, const avl_occlusion* occl,
                                            const avl_height* ht, void* stream) {
    AVL_REQUIRE(ht, "avl_height is NULL");
    VoteSource src;
    int rc;
    if (pl) {
        if ((rc = logits_source(src, pl, n_views))) return rc;
    } else {
        if ((rc = views_check(n_views, src_host))) return rc;
        src = bytes_source(src_kind, src_host, src_w, src_h);
    }
    return fused_frame_views(g, pts, n, dtype, point_stride, comp_stride, n_views, P_host, T_host, range_max, src, img_w, img_h, lut_host,
                             pl ? nullptr : label_colors_host, cm_host, bonus_classes, occl, stream, ht);
}

extern "C" int avl_point_heights(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, const double* T_host,
                                 const avl_height* ht, double* h, double* s, void* stream) {
    PtsView pv;
    ProjParams pp;
    HeightParams hp;
    int rc;
    if ((rc = fill_pts(pv, pts, n, dtype, point_stride, comp_stride))) return rc;
    if ((rc = height_fill(hp, ht, nullptr))) return rc;
    AVL_REQUIRE(n == 0 || (h && s), "h or s is NULL");
    AVL_REQUIRE(((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(s)) & 7) == 0, "h or s is not 8-byte aligned");
    if (n == 0) return AVL_OK;
    memset(&pp, 0, sizeof(pp));
    pp.has_T = T_host ? 1 : 0;
    if (T_host) memcpy(pp.T, T_host, sizeof(pp.T));
    hipLaunchKernelGGL(k_point_heights, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, avl::as_stream(stream), pv, pp, hp, h, s);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_elevation_mean(const int64_t* sum, const int32_t* cnt, int64_t ncell, double quantum, float* out, void* stream) {
    AVL_REQUIRE(ncell >= 0 && ncell <= 0x7fffffffLL, "ncell = %lld", (long long)ncell);
    AVL_REQUIRE(quantum > 0.0 && std::isfinite(quantum), "elevation quantum = %g (finite, > 0)", quantum);
    AVL_REQUIRE(ncell == 0 || (sum && cnt && out), "NULL buffer");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(sum) & 7) == 0, "elevation sum is not 8-byte aligned");
    AVL_REQUIRE(((reinterpret_cast<uintptr_t>(cnt) | reinterpret_cast<uintptr_t>(out)) & 3) == 0, "cnt or out is not 4-byte aligned");
    if (ncell == 0) return AVL_OK;
    hipLaunchKernelGGL(k_elevation_mean, dim3((unsigned)((ncell + kBlock - 1) / kBlock)), dim3(kBlock), 0, avl::as_stream(stream),
                       reinterpret_cast<const long long*>(sum), cnt, (long long)ncell, quantum, out);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_elevation_reset(int64_t* sum, int32_t* cnt, int32_t* qmin, int32_t* qmax, int64_t ncell, void* stream) {
    AVL_REQUIRE(ncell >= 0 && ncell <= 0x7fffffffLL, "ncell = %lld", (long long)ncell);
    AVL_REQUIRE(ncell == 0 || (sum && cnt && qmin && qmax), "NULL buffer");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(sum) & 7) == 0, "elevation sum is not 8-byte aligned");
    AVL_REQUIRE(((reinterpret_cast<uintptr_t>(cnt) | reinterpret_cast<uintptr_t>(qmin) | reinterpret_cast<uintptr_t>(qmax)) & 3) == 0,
                "elevation count, minimum or maximum is not 4-byte aligned");
    if (ncell == 0) return AVL_OK;
    hipLaunchKernelGGL(k_elevation_reset, dim3((unsigned)((ncell + kBlock - 1) / kBlock)), dim3(kBlock), 0, avl::as_stream(stream),
                       reinterpret_cast<long long*>(sum), cnt, qmin, qmax, (long long)ncell);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int64_t avl_occlusion_depth_words(int img_w, int img_h, int cell_px, int n_views) {
    if (img_w <= 0 || img_h <= 0 || cell_px < 1 || cell_px > 64 || n_views < 1) return 0;
    return occl_cells(img_w, img_h, cell_px) * n_views;
}

extern "C" int avl_occlusion_visibility(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, int n_views,
                                        const double* P_host, const double* T_host, double range_max, int img_w, int img_h,
                                        const avl_occlusion* occl, uint8_t* state, float* key, void* stream) {
    FrameArgs f;
    OcclParams oc;
    int rc;
    AVL_REQUIRE(n_views >= 1, "n_views = %d (at least one view)", n_views);
    AVL_REQUIRE(n_views <= kMaxViews, "n_views = %d exceeds the limit of %d views", n_views, kMaxViews);
    if ((rc = fill_pts(f.pv, pts, n, dtype, point_stride, comp_stride))) return rc;
    if ((rc = fill_proj(f.pp, P_host, T_host, range_max, img_w, img_h))) return rc;
    if ((rc = occl_fill(oc, occl, img_w, img_h, n_views))) return rc;
    AVL_REQUIRE(n == 0 || state, "state is NULL");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(key) & 3) == 0, "key is not 4-byte aligned");
    hipStream_t s = avl::as_stream(stream);
    if (n == 0) return occl_reset(oc, n_views, false, s);
    ViewsParams vp;
    fill_views(vp, f, n_views, P_host, nullptr);
    if ((rc = occl_reset(oc, n_views, true, s))) return rc;
    if ((rc = launch_occl_depth(f.pv, vp, oc, s))) return rc;
    hipLaunchKernelGGL(k_occl_visibility, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, f.pv, vp, oc, state, key);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_occlusion_depth(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, int n_views,
                                   const double* P_host, const double* T_host, double range_max, int img_w, int img_h,
                                   const avl_occlusion* occl, void* stream) {
    FrameArgs f;
    OcclParams oc;
    int rc;
    AVL_REQUIRE(n_views >= 1, "n_views = %d (at least one view)", n_views);
    AVL_REQUIRE(n_views <= kMaxViews, "n_views = %d exceeds the limit of %d views", n_views, kMaxViews);
    if ((rc = fill_pts(f.pv, pts, n, dtype, point_stride, comp_stride))) return rc;
    if ((rc = fill_proj(f.pp, P_host, T_host, range_max, img_w, img_h))) return rc;
    if ((rc = occl_fill(oc, occl, img_w, img_h, n_views))) return rc;
    hipStream_t s = avl::as_stream(stream);
    if ((rc = occl_reset(oc, n_views, true, s))) return rc;                      // the buffer is the result: an empty cloud leaves it empty
    if (n == 0) return AVL_OK;
    ViewsParams vp;
    fill_views(vp, f, n_views, P_host, nullptr);
    return launch_occl_depth(f.pv, vp, oc, s);
}

extern "C" int avl_ground_fill_views(const avl_grid* g, const avl_ground_fill* gf, int n_views, const double* P_host, const double* T_host,
                                     int src_kind, const uint8_t* const* src_host, int src_w, int src_h, int img_w, int img_h,
                                     const uint32_t* lut_host, const uint8_t* label_colors_host, const double* cm_host,
                                     const avl_occlusion* occl, void* stream) {
    int rc;
    if ((rc = views_check(n_views, src_host))) return rc;
    return ground_fill(g, gf, n_views, P_host, T_host, bytes_source(src_kind, src_host, src_w, src_h), img_w, img_h, lut_host,
                       label_colors_host, cm_host, occl, stream);
}

extern "C" int avl_ground_fill_views_logits(const avl_grid* g, const avl_ground_fill* gf, int n_views, const double* P_host,
                                            const double* T_host, const avl_point_logits* pl, int img_w, int img_h, const uint32_t* lut_host,
                                            const double* cm_host, const avl_occlusion* occl, void* stream) {
    VoteSource src;
    int rc;
    if ((rc = logits_source(src, pl, n_views))) return rc;
    return ground_fill(g, gf, n_views, P_host, T_host, src, img_w, img_h, lut_host, nullptr, cm_host, occl, stream);
}

extern "C" int avl_point_labels(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, int n_views,
                                const double* P_host, const double* T_host, double range_max, int img_w, int img_h,
                                const avl_point_logits* pl, uint8_t* state, float* margin, void* stream) {
    FrameArgs f;
    LogitsParams lp;
    int rc;
    if ((rc = logits_fill(lp, pl, n_views))) return rc;
    if ((rc = fill_pts(f.pv, pts, n, dtype, point_stride, comp_stride))) return rc;
    if ((rc = fill_proj(f.pp, P_host, T_host, range_max, img_w, img_h))) return rc;
    AVL_REQUIRE(n == 0 || state, "state is NULL");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(margin) & 3) == 0, "margin is not 4-byte aligned");
    hipStream_t s = avl::as_stream(stream);
    if ((rc = logits_reset(lp, n_views, s))) return rc;
    if (n == 0) return AVL_OK;
    ViewsParams vp;
    fill_views(vp, f, n_views, P_host, nullptr);
    hipLaunchKernelGGL(k_point_labels, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, f.pv, vp, lp, state, margin);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_colorize_labels(const uint8_t* labels, int lw, int lh, const uint8_t* palette_host, uint8_t* out,
                                   int out_w, int out_h, void* stream) {
    AVL_REQUIRE(labels && palette_host && out, "NULL buffer");
    AVL_REQUIRE(lw > 0 && lh > 0 && out_w > 0 && out_h > 0, "bad sizes");
    LutParams pal;
    for (int k = 0; k < 256; ++k)
        pal.lut[k] = (unsigned)palette_host[3 * k] | ((unsigned)palette_host[3 * k + 1] << 8) | ((unsigned)palette_host[3 * k + 2] << 16);
    const long long total = (long long)out_w * out_h;
    hipLaunchKernelGGL(k_colorize, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, avl::as_stream(stream),
                       labels, lw, lh, nullptr, pal, out, out_w, out_h);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// ---------------------------------------------------------------------------------------- semantic point cloud
namespace {
// create_point_cloud (src/utils/utils_ros.py:31-59): one PointCloud2 record per point, fields x,y,z FLOAT32 at
// offsets 0/4/8 and rgba UINT32 at 12 = struct.pack('BBBB', r, g, b, 255) read back as a little-endian 'I'.
__global__ void __launch_bounds__(kBlock) k_pack_cloud(const double* __restrict__ pcd, const unsigned char* __restrict__ label,
                                                       long long ld, int m_host, const int* __restrict__ m_dev, uint4* __restrict__ out) {
    const int m = m_dev ? min(*m_dev, m_host) : m_host;
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const float x = (float)pcd[k], y = (float)pcd[ld + k], z = (float)pcd[2 * ld + k];
    const unsigned rgba = (unsigned)label[k] | ((unsigned)label[ld + k] << 8) | ((unsigned)label[2 * ld + k] << 16) | (255u << 24);
    out[k] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), rgba);
}
}  // namespace

extern "C" int avl_pack_semantic_cloud(const double* pcd, const uint8_t* label, int64_t ld, int m_host, const int32_t* m_dev,
                                       void* out_records, void* stream) {
    AVL_REQUIRE(m_host >= 0, "m = %d", m_host);
    if (m_host == 0) return AVL_OK;
    AVL_REQUIRE(pcd && label && out_records && ld >= m_host, "bad buffers");
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(out_records) % 16 == 0, "out_records must be 16-byte aligned");
    hipLaunchKernelGGL(k_pack_cloud, dim3((m_host + kBlock - 1) / kBlock), dim3(kBlock), 0, avl::as_stream(stream), pcd, label,
                       (long long)ld, m_host, m_dev, static_cast<uint4*>(out_records));
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

namespace {
struct PlanarParams {
    double hi[9];
    unsigned char colors[AVL_MAX_MAP_CLASSES * 3];
    int C, sep, match, img_h, img_w;
};
// One lane per grid cell: inverse-map the cell into the image (float64, the oracle's expression order: this file is
// compiled with -ffp-contract=off), bilinear R and G with a zero border, class test, +1, clamp.
template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_planar_update(MapT* __restrict__ map, int Hm, int Wm, const unsigned char* __restrict__ img,
                                                          PlanarParams pp) {
    const long long cell = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= (long long)Hm * Wm) return;
    const int y = (int)(cell / Wm), x = (int)(cell % Wm);
    MapT* row = map + cell * pp.C;
    if (pp.match && x >= pp.sep) {
        const double xs = (double)x, ys = (double)y;
        const double den = pp.hi[6] * xs + pp.hi[7] * ys + pp.hi[8];
        double sx = (pp.hi[0] * xs + pp.hi[1] * ys + pp.hi[2]) / den;
        double sy = (pp.hi[3] * xs + pp.hi[4] * ys + pp.hi[5]) / den;
        if (!(__builtin_isfinite(sx) && __builtin_isfinite(sy) && __builtin_fabs(sx) < 1e9 && __builtin_fabs(sy) < 1e9)) sx = sy = -10.0;
        const double fx = __builtin_floor(sx), fy = __builtin_floor(sy);
        const double ax = sx - fx, ay = sy - fy;
        const long long x0 = (long long)fx, y0 = (long long)fy;
        double acc[2] = {0.0, 0.0};
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const long long xx = x0 + dx, yy = y0 + dy;
                const bool inside = xx >= 0 && xx < pp.img_w && yy >= 0 && yy < pp.img_h;
                const double wgt = (dx ? ax : 1.0 - ax) * (dy ? ay : 1.0 - ay);
                const long long cx = xx < 0 ? 0 : (xx >= pp.img_w ? pp.img_w - 1 : xx), cy = yy < 0 ? 0 : (yy >= pp.img_h ? pp.img_h - 1 : yy);
                const unsigned char* px = img + 3 * (cy * pp.img_w + cx);
                const double wv = inside ? wgt : 0.0;
                acc[0] = acc[0] + wv * (double)px[0];
                acc[1] = acc[1] + wv * (double)px[1];
            }
        const double r = __builtin_rint(acc[0]), g = __builtin_rint(acc[1]);
        const int ri = r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r), gi = g < 0.0 ? 0 : (g > 255.0 ? 255 : (int)g);
        for (int i = 0; i < pp.C; ++i)
            if (pp.colors[3 * i] == ri && pp.colors[3 * i + 1] == gi) row[i] = (MapT)((double)row[i] + 1.0);
    }
    for (int i = 0; i < pp.C; ++i)
        if (row[i] < (MapT)0) row[i] = (MapT)0;                       // map_local[map_local < 0] = 0 (:481)
}
}  // namespace

extern "C" int avl_planar_update(void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* image, int img_h, int img_w,
                                 const double* Hinv_host, int sep, const uint8_t* label_colors_host, int match_colour, void* stream) {
    AVL_REQUIRE(map && Hm > 0 && Wm > 0 && C > 0 && C <= AVL_MAX_MAP_CLASSES, "bad grid %dx%dx%d", Hm, Wm, C);
    AVL_REQUIRE(map_dtype == AVL_F64 || map_dtype == AVL_F32, "map dtype %d", map_dtype);
    AVL_REQUIRE(!match_colour || (image && Hinv_host && label_colors_host && img_h > 0 && img_w > 0), "colour matching needs image, Hinv_host and label_colors_host");
    PlanarParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.C = C; pp.sep = sep; pp.match = match_colour ? 1 : 0; pp.img_h = img_h; pp.img_w = img_w;
    if (match_colour) {
        memcpy(pp.hi, Hinv_host, sizeof(pp.hi));
        memcpy(pp.colors, label_colors_host, 3 * C);
    }
    const long long n = (long long)Hm * Wm;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    return launch_map_typed(map_dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_planar_update<T>, grid, block, 0, avl::as_stream(stream), static_cast<T*>(map), Hm, Wm, image, pp);
    });
}

namespace {
// One lane per point; fields are 4-byte aligned, so each is one dword load (a point's record is usually 16-32 bytes:
// the wave reads a contiguous 1-2 KB).  The count goes through one ballot + one atomic per wave.
__global__ void __launch_bounds__(kBlock) k_unpack_cloud(const unsigned char* __restrict__ data, long long n, int step, int ox, int oy,
                                                         int oz, int oi, float4* __restrict__ out, int* __restrict__ n_valid) {
    const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool ok = false;
    if (k < n) {
        const unsigned char* rec = data + k * step;
        float x = *reinterpret_cast<const float*>(rec + ox);
        const float y = *reinterpret_cast<const float*>(rec + oy), z = *reinterpret_cast<const float*>(rec + oz);
        const float i = *reinterpret_cast<const float*>(rec + oi);
        ok = !(x != x || y != y || z != z || i != i);
        if (!ok) x = __uint_as_float(0x7fc00000u);
        out[k] = make_float4(x, y, z, i);
    }
    if (n_valid) {
        const unsigned long long b = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_valid, __popcll(b));
    }
}
}  // namespace

extern "C" int avl_unpack_pointcloud2(const uint8_t* data, int64_t n_points, int point_step, int off_x, int off_y, int off_z, int off_i,
                                      float* out_xyzi, int32_t* n_valid, void* stream) {
    AVL_REQUIRE(n_points >= 0, "n_points = %lld", (long long)n_points);
    if (n_valid) AVL_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int32_t), avl::as_stream(stream)));
    if (n_points == 0) return AVL_OK;
    AVL_REQUIRE(data && out_xyzi, "bad buffers");
    AVL_REQUIRE(point_step >= 16 && point_step % 4 == 0, "point_step = %d (FLOAT32 fields need 4-byte aligned records)", point_step);
    const int offs[4] = {off_x, off_y, off_z, off_i};
    for (int o : offs) AVL_REQUIRE(o >= 0 && o % 4 == 0 && o + 4 <= point_step, "field offset %d outside a %d-byte record / unaligned", o, point_step);
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(data) % 4 == 0 && reinterpret_cast<uintptr_t>(out_xyzi) % 16 == 0, "unaligned buffers");
    hipLaunchKernelGGL(k_unpack_cloud, dim3((unsigned)((n_points + kBlock - 1) / kBlock)), dim3(kBlock), 0, avl::as_stream(stream), data,
                       (long long)n_points, point_step, off_x, off_y, off_z, off_i, reinterpret_cast<float4*>(out_xyzi), n_valid);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// ---------------------------------------------------------------------------------------- rendering
namespace {
// the two end-of-run renderers: the checks, the parameter block and the launch of one thread per cell
int render_whole_map(const char* who, bool thresholds, const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host,
                     const int32_t* priority_host, const double* thresholds_host, uint8_t* out, void* stream) {
    AVL_REQUIRE(C > 0 && C <= AVL_MAX_MAP_CLASSES, "C = %d", C);
    AVL_REQUIRE(colors_host, "colors_host is NULL");
    RenderParams rp;
    int rc;
    if ((rc = avl::fill_render_params(rp, who, C, colors_host, priority_host, thresholds_host))) return rc;
    AVL_REQUIRE(map && out && Hm > 0 && Wm > 0, "bad map / out");
    AVL_REQUIRE(map_dtype == AVL_F64 || map_dtype == AVL_F32, "map dtype %d", map_dtype);
    const long long n = (long long)Hm * Wm;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    return launch_map_typed(map_dtype, [&](auto t) {
        typedef decltype(t) T;
        auto kernel = k_render_bev<T>;
        if (thresholds) kernel = k_render_thresholds<T>;
        hipLaunchKernelGGL(kernel, grid, block, 0, avl::as_stream(stream), static_cast<const T*>(map), n, C, rp, out);
    });
}
}  // namespace

extern "C" int avl_render_bev_map(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host, uint8_t* out,
                                  void* stream) {
    return render_whole_map("avl_render_bev_map", false, map, map_dtype, Hm, Wm, C, colors_host, nullptr, nullptr, out, stream);
}

extern "C" int avl_render_bev_map_thresholds(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host,
                                             const int32_t* priority_host, const double* thresholds_host, uint8_t* out, void* stream) {
    return render_whole_map("avl_render_bev_map_thresholds", true, map, map_dtype, Hm, Wm, C, colors_host, priority_host, thresholds_host,
                            out, stream);
}

// ---- end-of-run evaluation (test/test_semantic_mapping.py: convert_labels :6-19, Test.iou :127-161) -----------------
// One pass over the rendered colour map: label = 1..5 for the five map colours (exact three-channel match, 0 otherwise
// or where the validity mask is 0), and -- if a ground-truth map is given -- the joint histogram counts[gt][label]
// (8 x 8 bins; gt bin 7 = "positive, but none of 1..6") from which IoU, accuracy and missing rate are integer sums.
namespace {
__global__ void __launch_bounds__(kBlock) k_eval_map(const uint8_t* __restrict__ color, int H, int W, const uint8_t* __restrict__ mask,
                                                   int mask_ld, const uint8_t* __restrict__ gt, int gt_ld, uint8_t* __restrict__ labels,
                                                   unsigned long long* __restrict__ counts) {
    __shared__ unsigned int hist[64];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    __syncthreads();
    const long long n = (long long)H * W;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        int lab = avl::colour_label(color[i * 3], color[i * 3 + 1], color[i * 3 + 2]);
        if (mask && mask[(long long)y * mask_ld + x] == 0) lab = 0;
        if (labels) labels[i] = (uint8_t)lab;
        if (gt) {
            int gv = gt[(long long)y * gt_ld + x];
            gv = gv > 7 ? 7 : gv;
            atomicAdd(&hist[gv * 8 + lab], 1u);
        }
    }
    __syncthreads();
    if (gt && threadIdx.x < 64 && hist[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}
}  // namespace

extern "C" int avl_eval_map(const uint8_t* color_map, int H, int W, const uint8_t* mask, int mask_ld, const uint8_t* gt, int gt_ld,
                            uint8_t* labels_out, unsigned long long* counts, void* stream) {
    AVL_REQUIRE(color_map && H > 0 && W > 0, "bad colour map");
    AVL_REQUIRE(labels_out || gt, "avl_eval_map: nothing to compute (labels_out and gt are both NULL)");
    AVL_REQUIRE(!mask || mask_ld >= W, "mask row stride %d < W %d", mask_ld, W);
    AVL_REQUIRE(!gt || (gt_ld >= W && counts), "ground truth needs gt_ld >= W and a counts[64] buffer");
    hipStream_t s = avl::as_stream(stream);
    if (gt) AVL_HIP_CHECK(hipMemsetAsync(counts, 0, 64 * sizeof(unsigned long long), s));
    const long long n = (long long)H * W;
    long long blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 2048) blocks = 2048;                      // grid-stride: one LDS histogram flush per workgroup
    hipLaunchKernelGGL(k_eval_map, dim3((unsigned)blocks), dim3(kBlock), 0, s, color_map, H, W, mask, mask_ld, gt, gt_ld, labels_out, counts);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_grid_box_filter(const void* src, void* dst, int map_dtype, int Hm, int Wm, int C, void* stream) {
    AVL_REQUIRE(src && dst && src != dst, "box filter needs distinct src and dst");
    AVL_REQUIRE(Hm > 1 && Wm > 1 && C > 0, "grid %dx%dx%d", Hm, Wm, C);
    AVL_REQUIRE(map_dtype == AVL_F64 || map_dtype == AVL_F32, "map dtype %d", map_dtype);
    const long long n = (long long)Hm * Wm * C;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    return launch_map_typed(map_dtype, [&](auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_box_filter3<T>, grid, block, 0, avl::as_stream(stream), static_cast<const T*>(src), static_cast<T*>(dst), Hm, Wm, C);
    });
}

