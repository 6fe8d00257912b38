// Live vehicle-centred map (gfx950): one launch renders an h x w window of the BEV grid -- box filter, renderer, the reference's
// hole filler and the ego car -- without a temporary grid.  Compiled with -ffp-contract=off like mapping.hip: the filter's double
// accumulation, the MapT row sum and quotient, and the car's rotation have to round where apply_filter + render_bev_map and
// a NumPy float64 restatement round.
//
// Reference (src/renderer.py, src/mapping.py):
//   renderer.py:175-189  apply_filter            -> avl::box_filter3_taps (avl_render.h, shared with k_box_filter3)
//   renderer.py:32-59    render_bev_map          -> avl::argmax_class (avl_render.h, shared with k_render_bev)
//   renderer.py:131-172  render_bev_map_with_thresholds -> avl::thresholds_class (avl_render.h, shared with k_render_thresholds)
//   renderer.py:62-105   fill_black / resume_color, AS WRITTEN: every interior pixel (black or not, :91 is commented out) takes the
//                        highest-priority label whose R value occurs among the R values of its 3 x 3 neighbourhood; matching is
//                        on R only, so colours that share an R value are conflated (the last such label wins in resume_color)
//   mapping.py:490-526   add_car_to_map: its footprint (4.0 m x 1.8 m), its reference point (a quarter length from the rear) and
//                        its colour are kept; its forward scatter of truncated pixels (holes under rotation, "not tested" by its
//                        authors) is NOT: every window cell whose centre lies in the rotated rectangle is painted.
//
// k_live_map, one workgroup per 16 x 64 output tile (long side along the contiguous Wm axis):
//   A  every thread computes the class index (255 = black) of cells of the tile plus a one-cell halo -> one byte per cell in LDS.
//      The filter's 9 x C reads go to global memory; neighbouring cells share them through L1 / L2, as k_box_filter3's do.
//   B  after the barrier, the 3 x 3 priority pass over the LDS bytes (AVL_LIVE_FILL only)
//   C  RGB stores, the car last: its red has the lane's R value and fill_black matches on R
// The arg-max renderer streams the channels once (sum and arg-max in one pass); the thresholds renderer needs the sum before
// the shares and evaluates the filter a second time for them instead of keeping C values per thread (no scratch, no LDS rows).
//
// k_live_view, the same picture through a 2 x 3 matrix from output pixel centres to grid coordinates (avl_live_view), one workgroup
// per 32 x 32 output tile (square: its grid footprint is the same at every rotation):
//   A  the grid-space bounding box of the tile's footprint, from its four corner pixel centres (rounding is monotone, so the
//      extremes of gx and gy over the tile are at the corners), clamped to the grid plus one cell.  Lanes walk the box in GRID
//      row-major order -- the filter's reads stay contiguous along Wm whatever the rotation -- and every cell's class is computed
//      once, however many pixels sample it; with the fill, one more ring of cells -> one byte per cell in LDS
//   B  after the barrier every pixel finds its cell: floor of its coordinates, range-tested on the doubles; the fill's 3 x 3 pass
//      runs on the sampled cell's LDS neighbourhood, so filter and fill stay defined in the grid's frame
//   C  RGB stores, the car last, tested on the pixel's continuous coordinates
// The LDS box is static, kVBox x kVLd bytes, for the largest footprint avl_live_view admits (AVL_LIVE_VIEW_MAX_SPAN); the box's
// size is clamped to it and a pixel whose cell fell outside the box would read nothing, so no LDS index leaves the array whatever
// the matrix.
#include "avl_common.h"
#include "avl_render.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int kBlock = 256;
constexpr int kTH = 16, kTW = 64;            // output tile
constexpr int kPH = kTH + 2, kPW = kTW + 2;  // with the halo
constexpr int kBlack = 255;                  // "no class" byte of the LDS tile
constexpr int kMaxWindow = 32768;            // h, w: gridDim.y holds 65535 tiles
constexpr int kVT = 32;                      // k_live_view's output tile, kVT x kVT
// Cells per axis of a tile's footprint: its corner pixel centres are kVT - 1 apart, so gx spans at most (kVT - 1) * (|M00| + |M01|)
// <= 31 * 2.875 = 89.125 (plus roundings of 2^-20 at most: a pixel that samples the grid has |gx| < 2^31 + 2^17), and an interval
// of length L meets at most floor(L) + 2 cells: 91.  With the fill's ring on both sides: 93.
constexpr int kVBox = 93, kVLd = 96;
static_assert((kVT - 1) * AVL_LIVE_VIEW_MAX_SPAN + 0.5 < kVBox - 2 - 1, "the LDS box does not hold the largest admitted footprint");

// fill_black's label walk, prepared on the host: list position k names label prio[k]; a pixel that ends with that label's R value
// is coloured by resume_color as label final_[k] (the last label with the same R); no label present -> none (kBlack unless a
// label has R = 0).
struct FillTable {
    int n_colors, n_prio;
    unsigned char colors[AVL_MAX_MAP_CLASSES * 3];
    unsigned char prio[AVL_MAX_MAP_CLASSES];
    unsigned char final_[AVL_MAX_MAP_CLASSES];
    unsigned char none;
};

struct LiveParams {
    int Hm, Wm, C;
    int x0, y0, h, w, flags;
    int has_car;
    unsigned char car_rgb[4];
    double car[AVL_LIVE_CAR_DOUBLES];   // cx, cy, cos, sin, u_lo, u_hi, v_lo, v_hi
    avl::RenderParams rp;
    FillTable ft;
};

struct ViewParams {
    LiveParams p;     // x0, y0 unused
    double m[6];      // pixel centre (i + 0.5, j + 0.5) -> grid coordinates, row-major 2 x 3
};

// s_col[label] = its colour, s_col[16] = black; s_mask[byte] = labels whose R value the tile byte stands for.  A live tile holds
// class indices (kBlack: R = 0), an image tile holds R values.
template <bool kBytesAreClasses>
__device__ __forceinline__ void build_tables(const FillTable& ft, unsigned char* s_col, unsigned short* s_mask) {
    const int t = threadIdx.x;
    if (t < (AVL_MAX_MAP_CLASSES + 1) * 3) s_col[t] = t < ft.n_colors * 3 ? ft.colors[t] : 0;
    __syncthreads();
    const int r = kBytesAreClasses ? (t < ft.n_colors ? s_col[3 * t] : 0) : t;
    unsigned m = 0;
    for (int i = 0; i < ft.n_colors; ++i) m |= (unsigned)(s_col[3 * i] == r) << i;
    s_mask[t] = (unsigned short)m;
}

// label (or kBlack) of the pixel whose tile byte is *centre: fill_black's mask_dict + priority walk + resume_color
template <int kLd = kPW>
__device__ __forceinline__ int fill_pick(const unsigned char* centre, const unsigned short* s_mask, const FillTable& ft) {
    unsigned present = 0;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) present |= s_mask[centre[di * kLd + dj]];
    int label = ft.none;
    for (int k = 0; k < ft.n_prio; ++k)
        if ((present >> ft.prio[k]) & 1u) label = ft.final_[k];
    return label;
}

// class index of grid cell (gx, gy) -- row gx of Hm, column gy of Wm -- or kBlack: the render rule of avl_render.h on the cell's
// row, read as it is or through the filter
template <typename MapT>
__device__ __forceinline__ int cell_class(const MapT* __restrict__ map, const LiveParams& p, int gx, int gy) {
    const int Hm = p.Hm, Wm = p.Wm, C = p.C;
    const bool filt = p.flags & AVL_LIVE_FILTER;
    const MapT* row = map + ((long long)gx * Wm + gy) * C;
    auto value = [&](int c) -> MapT { return filt ? (MapT)avl::box_filter3_taps(map, Hm, Wm, C, gx, gy, c) : row[c]; };
    const int cls = (p.flags & AVL_LIVE_THRESHOLDS) ? avl::thresholds_class<MapT>(C, p.rp, value) : avl::argmax_class<MapT>(C, value);
    return cls == avl::kNoClass ? kBlack : cls;
}

template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_live_map(const MapT* __restrict__ map, LiveParams p, unsigned char* __restrict__ out) {
    __shared__ unsigned char s_tile[kPH * kPW];
    __shared__ unsigned char s_col[(AVL_MAX_MAP_CLASSES + 1) * 3 + 1];
    __shared__ unsigned short s_mask[256];
    build_tables<true>(p.ft, s_col, s_mask);
    const int ti0 = blockIdx.y * kTH, tj0 = blockIdx.x * kTW;   // window coordinates of the tile
    const bool fill = p.flags & AVL_LIVE_FILL;
    const int halo = fill ? 1 : 0;
    // ---- A: classes of the tile and (for the fill) its halo; cells beyond the window's own halo are never read
    for (int idx = threadIdx.x; idx < kPH * kPW; idx += kBlock) {
        const int li = idx / kPW, lj = idx - li * kPW;
        const int i = ti0 + li - 1, j = tj0 + lj - 1;
        int cls = kBlack;
        if (li >= 1 - halo && li <= kTH + halo && lj >= 1 - halo && lj <= kTW + halo && i < p.h + halo && j < p.w + halo) {
            const long long gx = (long long)p.x0 + i, gy = (long long)p.y0 + j;
            if (gx >= 0 && gx < p.Hm && gy >= 0 && gy < p.Wm) cls = cell_class(map, p, (int)gx, (int)gy);
        }
        s_tile[idx] = (unsigned char)cls;
    }
    __syncthreads();
    // ---- B, C
    for (int idx = threadIdx.x; idx < kTH * kTW; idx += kBlock) {
        const int li = idx / kTW, lj = idx - li * kTW;
        const int i = ti0 + li, j = tj0 + lj;
        if (i >= p.h || j >= p.w) continue;
        const long long gx = (long long)p.x0 + i, gy = (long long)p.y0 + j;
        const unsigned char* centre = s_tile + (li + 1) * kPW + lj + 1;
        int label = *centre;
        if (fill) {   // fill_black's output is the grid's interior; the one-cell ring around it and everything off the grid is black
            const bool interior = gx >= 1 && gx <= p.Hm - 2 && gy >= 1 && gy <= p.Wm - 2;
            label = interior ? fill_pick(centre, s_mask, p.ft) : kBlack;
        }
        const int ci = label == kBlack ? AVL_MAX_MAP_CLASSES : label;
        unsigned char r = s_col[3 * ci], g = s_col[3 * ci + 1], b = s_col[3 * ci + 2];
        if (p.has_car) {
            const double dx = ((double)gx + 0.5) - p.car[0], dy = ((double)gy + 0.5) - p.car[1];
            const double c = p.car[2], s = p.car[3];
            const double u = c * dx + s * dy, v = c * dy - s * dx;
            if (p.car[4] <= u && u < p.car[5] && p.car[6] <= v && v < p.car[7]) { r = p.car_rgb[0]; g = p.car_rgb[1]; b = p.car_rgb[2]; }
        }
        unsigned char* o = out + ((long long)i * p.w + j) * 3;
        o[0] = r; o[1] = g; o[2] = b;
    }
}

template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_live_view(const MapT* __restrict__ map, ViewParams vp, unsigned char* __restrict__ out) {
    __shared__ unsigned char s_box[kVBox * kVLd];
    __shared__ unsigned char s_col[(AVL_MAX_MAP_CLASSES + 1) * 3 + 1];
    __shared__ unsigned short s_mask[256];
    const LiveParams& p = vp.p;
    build_tables<true>(p.ft, s_col, s_mask);
    const int ti0 = blockIdx.y * kVT, tj0 = blockIdx.x * kVT;
    const bool fill = p.flags & AVL_LIVE_FILL;
    const double m00 = vp.m[0], m01 = vp.m[1], m02 = vp.m[2], m10 = vp.m[3], m11 = vp.m[4], m12 = vp.m[5];
    // ---- A: the box of grid cells [xlo, xlo + nx) x [ylo, ylo + ny) that the tile's pixels can sample, from the corners of its
    //         (ragged) pixel range; cells off the grid are black without a read, so the box is clamped to the grid plus one cell
    const double a0 = (double)ti0 + 0.5, a1 = (double)(min(ti0 + kVT, p.h) - 1) + 0.5;
    const double b0 = (double)tj0 + 0.5, b1 = (double)(min(tj0 + kVT, p.w) - 1) + 0.5;
    auto box = [&](double ma, double mb, double mc, int n, int& lo) -> int {
        const double c00 = (ma * a0 + mb * b0) + mc, c01 = (ma * a0 + mb * b1) + mc;
        const double c10 = (ma * a1 + mb * b0) + mc, c11 = (ma * a1 + mb * b1) + mc;
        const double top = (double)n;
        const double mn = fmin(fmax(floor(fmin(fmin(c00, c01), fmin(c10, c11))), -1.0), top);
        const double mx = fmin(fmax(floor(fmax(fmax(c00, c01), fmax(c10, c11))), -1.0), top);
        lo = (int)mn;
        return min((int)mx - lo + 1, kVBox - 2);
    };
    int xlo, ylo;
    const int nx = box(m00, m01, m02, p.Hm, xlo), ny = box(m10, m11, m12, p.Wm, ylo);
    // LDS byte (bi, bj), 0 <= bi <= nx + 1, 0 <= bj <= ny + 1, is grid cell (xlo - 1 + bi, ylo - 1 + bj): the ring is the fill's
    const int bw = ny + 2;
    for (int idx = threadIdx.x; idx < (nx + 2) * bw; idx += kBlock) {
        const int bi = idx / bw, bj = idx - bi * bw;
        const int gx = xlo - 1 + bi, gy = ylo - 1 + bj;
        int cls = kBlack;
        if ((fill || (bi >= 1 && bi <= nx && bj >= 1 && bj <= ny)) && gx >= 0 && gx < p.Hm && gy >= 0 && gy < p.Wm)
            cls = cell_class(map, p, gx, gy);
        s_box[bi * kVLd + bj] = (unsigned char)cls;
    }
    __syncthreads();
    // ---- B, C
    for (int idx = threadIdx.x; idx < kVT * kVT; idx += kBlock) {
        const int li = idx / kVT, lj = idx - li * kVT;
        const int i = ti0 + li, j = tj0 + lj;
        if (i >= p.h || j >= p.w) continue;
        const double a = (double)i + 0.5, b = (double)j + 0.5;
        const double gx = (m00 * a + m01 * b) + m02, gy = (m10 * a + m11 * b) + m12;
        int label = kBlack;
        if (0.0 <= gx && gx < (double)p.Hm && 0.0 <= gy && gy < (double)p.Wm) {
            const int cx = (int)gx, cy = (int)gy;                      // floor: both are >= 0 here
            const int bi = cx - xlo + 1, bj = cy - ylo + 1;
            if (bi >= 1 && bi <= nx && bj >= 1 && bj <= ny) {          // always, for a matrix avl_live_view admits
                const unsigned char* centre = s_box + bi * kVLd + bj;
                label = *centre;
                if (fill) {
                    const bool interior = cx >= 1 && cx <= p.Hm - 2 && cy >= 1 && cy <= p.Wm - 2;
                    label = interior ? fill_pick<kVLd>(centre, s_mask, p.ft) : kBlack;
                }
            }
        }
        const int ci = label == kBlack ? AVL_MAX_MAP_CLASSES : label;
        unsigned char r = s_col[3 * ci], g = s_col[3 * ci + 1], bl = s_col[3 * ci + 2];
        if (p.has_car) {
            const double dx = gx - p.car[0], dy = gy - p.car[1];
            const double c = p.car[2], s = p.car[3];
            const double u = c * dx + s * dy, v = c * dy - s * dx;
            if (p.car[4] <= u && u < p.car[5] && p.car[6] <= v && v < p.car[7]) { r = p.car_rgb[0]; g = p.car_rgb[1]; bl = p.car_rgb[2]; }
        }
        unsigned char* o = out + ((long long)i * p.w + j) * 3;
        o[0] = r; o[1] = g; o[2] = bl;
    }
}

// fill_black on an image: img [X][Y][3] -> out [X - 2][Y - 2][3]
__global__ void __launch_bounds__(kBlock) k_fill_black(const unsigned char* __restrict__ img, int X, int Y, FillTable ft,
                                                       unsigned char* __restrict__ out) {
    __shared__ unsigned char s_tile[kPH * kPW];
    __shared__ unsigned char s_col[(AVL_MAX_MAP_CLASSES + 1) * 3 + 1];
    __shared__ unsigned short s_mask[256];
    build_tables<false>(ft, s_col, s_mask);
    const int ti0 = blockIdx.y * kTH, tj0 = blockIdx.x * kTW;   // output coordinates of the tile = input coordinates of its halo
    for (int idx = threadIdx.x; idx < kPH * kPW; idx += kBlock) {
        const int li = idx / kPW, lj = idx - li * kPW;
        const int x = ti0 + li, y = tj0 + lj;
        s_tile[idx] = (x < X && y < Y) ? img[((long long)x * Y + y) * 3] : 0;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kTH * kTW; idx += kBlock) {
        const int li = idx / kTW, lj = idx - li * kTW;
        const int i = ti0 + li, j = tj0 + lj;
        if (i >= X - 2 || j >= Y - 2) continue;
        const int label = fill_pick(s_tile + (li + 1) * kPW + lj + 1, s_mask, ft);
        const int ci = label == kBlack ? AVL_MAX_MAP_CLASSES : label;
        unsigned char* o = out + ((long long)i * (Y - 2) + j) * 3;
        o[0] = s_col[3 * ci]; o[1] = s_col[3 * ci + 1]; o[2] = s_col[3 * ci + 2];
    }
}

int build_fill(FillTable& ft, const uint8_t* colors, int n, const int32_t* prio, int n_prio) {
    memset(&ft, 0, sizeof(ft));
    AVL_REQUIRE(n > 0 && n <= AVL_MAX_MAP_CLASSES, "%d colours (1..%d)", n, AVL_MAX_MAP_CLASSES);
    AVL_REQUIRE(colors, "colors_host is NULL");
    AVL_REQUIRE(n_prio >= 0 && n_prio <= AVL_MAX_MAP_CLASSES, "fill priority list of %d labels (0..%d)", n_prio, AVL_MAX_MAP_CLASSES);
    AVL_REQUIRE(n_prio == 0 || prio, "fill priority list is NULL");
    ft.n_colors = n;
    ft.n_prio = n_prio;
    memcpy(ft.colors, colors, 3 * n);
    auto last_with_r = [&](int r, int otherwise) {
        int hit = otherwise;
        for (int i = 0; i < n; ++i)
            if (colors[3 * i] == r) hit = i;
        return hit;
    };
    for (int k = 0; k < n_prio; ++k) {
        AVL_REQUIRE(prio[k] >= 0 && prio[k] < n, "fill priority[%d] = %d with %d colours", k, prio[k], n);
        ft.prio[k] = (unsigned char)prio[k];
        ft.final_[k] = (unsigned char)last_with_r(colors[3 * prio[k]], prio[k]);
    }
    ft.none = (unsigned char)last_with_r(0, kBlack);
    return AVL_OK;
}

// what avl_live_map and avl_live_view share: every check on the arguments, and the parameter block but for the window's geometry
int live_params(LiveParams& p, const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host, int h, int w, int flags,
                const int32_t* priority_host, const double* thresholds_host, const int32_t* fill_priority_host, int n_fill_priority,
                const double* car_host, const uint8_t* car_color_host, const uint8_t* out, const char* who) {
    AVL_REQUIRE(map, "map is NULL");
    AVL_REQUIRE(out, "out is NULL");
    AVL_REQUIRE(map_dtype == AVL_F64 || map_dtype == AVL_F32, "map dtype %d", map_dtype);
    AVL_REQUIRE(C > 0 && C <= AVL_MAX_MAP_CLASSES, "C = %d (1..%d)", C, AVL_MAX_MAP_CLASSES);
    AVL_REQUIRE(Hm > 0 && Wm > 0 && (long long)Hm * Wm <= 0x7fffffffLL, "grid %d x %d", Hm, Wm);
    AVL_REQUIRE(h >= 1 && w >= 1 && h <= kMaxWindow && w <= kMaxWindow, "window %d x %d (1..%d each)", h, w, kMaxWindow);
    AVL_REQUIRE(!(flags & ~(AVL_LIVE_FILTER | AVL_LIVE_THRESHOLDS | AVL_LIVE_FILL)), "flags 0x%x", flags);
    AVL_REQUIRE(colors_host, "colors_host is NULL");
    AVL_REQUIRE(!(flags & AVL_LIVE_FILTER) || (Hm > 1 && Wm > 1), "the box filter reflects at the grid's edge: grid %d x %d", Hm, Wm);
    AVL_REQUIRE(!(flags & AVL_LIVE_FILL) || (Hm >= 3 && Wm >= 3), "fill_black needs a 3 x 3 grid at least: %d x %d", Hm, Wm);
    AVL_REQUIRE(!(flags & AVL_LIVE_THRESHOLDS) || thresholds_host, "AVL_LIVE_THRESHOLDS without thresholds_host");
    memset(&p, 0, sizeof(p));
    p.Hm = Hm; p.Wm = Wm; p.C = C; p.h = h; p.w = w; p.flags = flags;
    int rc;
    if ((rc = avl::fill_render_params(p.rp, who, C, colors_host, priority_host, thresholds_host))) return rc;
    if ((rc = build_fill(p.ft, colors_host, C, fill_priority_host, (flags & AVL_LIVE_FILL) ? n_fill_priority : 0))) return rc;
    if (car_host) {
        p.has_car = 1;
        memcpy(p.car, car_host, sizeof(p.car));
        p.car_rgb[0] = car_color_host ? car_color_host[0] : 255;
        p.car_rgb[1] = car_color_host ? car_color_host[1] : 0;
        p.car_rgb[2] = car_color_host ? car_color_host[2] : 0;
    }
    return AVL_OK;
}

}  // namespace

extern "C" int avl_live_map(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host, int x0, int y0, int h,
                            int w, int flags, const int32_t* priority_host, const double* thresholds_host,
                            const int32_t* fill_priority_host, int n_fill_priority, const double* car_host,
                            const uint8_t* car_color_host, uint8_t* out, void* stream) {
    LiveParams p;
    int rc;
    if ((rc = live_params(p, map, map_dtype, Hm, Wm, C, colors_host, h, w, flags, priority_host, thresholds_host, fill_priority_host,
                          n_fill_priority, car_host, car_color_host, out, "avl_live_map"))) return rc;
    p.x0 = x0; p.y0 = y0;
    const dim3 grid((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kTH - 1) / kTH)), block(kBlock);
    if (map_dtype == AVL_F64) hipLaunchKernelGGL(k_live_map<double>, grid, block, 0, avl::as_stream(stream), static_cast<const double*>(map), p, out);
    else hipLaunchKernelGGL(k_live_map<float>, grid, block, 0, avl::as_stream(stream), static_cast<const float*>(map), p, out);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_live_view(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host, const double* matrix_host,
                             int h, int w, int flags, const int32_t* priority_host, const double* thresholds_host,
                             const int32_t* fill_priority_host, int n_fill_priority, const double* car_host,
                             const uint8_t* car_color_host, uint8_t* out, void* stream) {
    ViewParams vp;
    int rc;
    if ((rc = live_params(vp.p, map, map_dtype, Hm, Wm, C, colors_host, h, w, flags, priority_host, thresholds_host, fill_priority_host,
                          n_fill_priority, car_host, car_color_host, out, "avl_live_view"))) return rc;
    AVL_REQUIRE(matrix_host, "matrix_host is NULL");
    for (int k = 0; k < 6; ++k) {
        AVL_REQUIRE(std::isfinite(matrix_host[k]), "matrix[%d][%d] = %g is not finite", k / 3, k % 3, matrix_host[k]);
        vp.m[k] = matrix_host[k];
    }
    for (int r = 0; r < 2; ++r) {
        const double span = std::fabs(vp.m[3 * r]) + std::fabs(vp.m[3 * r + 1]);
        AVL_REQUIRE(span <= AVL_LIVE_VIEW_MAX_SPAN, "|M%d0| + |M%d1| = %.17g cells per pixel step: the limit is %g", r, r, span,
                    (double)AVL_LIVE_VIEW_MAX_SPAN);
    }
    const dim3 grid((unsigned)((w + kVT - 1) / kVT), (unsigned)((h + kVT - 1) / kVT)), block(kBlock);
    if (map_dtype == AVL_F64) hipLaunchKernelGGL(k_live_view<double>, grid, block, 0, avl::as_stream(stream), static_cast<const double*>(map), vp, out);
    else hipLaunchKernelGGL(k_live_view<float>, grid, block, 0, avl::as_stream(stream), static_cast<const float*>(map), vp, out);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int avl_fill_black(const uint8_t* img, int X, int Y, const uint8_t* colors_host, int n_colors, const int32_t* priority_host,
                              int n_priority, uint8_t* out, void* stream) {
    AVL_REQUIRE(img && out, "img / out is NULL");
    AVL_REQUIRE(X >= 3 && Y >= 3, "image %d x %d: fill_black needs 3 x 3 at least (X < 3 or Y < 3)", X, Y);
    AVL_REQUIRE(X - 2 <= kMaxWindow * kTH && (long long)X * Y <= 0x7fffffffLL, "image %d x %d", X, Y);
    FillTable ft;
    int rc;
    if ((rc = build_fill(ft, colors_host, n_colors, priority_host, n_priority))) return rc;
    const dim3 grid((unsigned)((Y - 2 + kTW - 1) / kTW), (unsigned)((X - 2 + kTH - 1) / kTH)), block(kBlock);
    hipLaunchKernelGGL(k_fill_black, grid, block, 0, avl::as_stream(stream), img, X, Y, ft, out);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}
