// Live drivable-area cost map (gfx950): the window of the BEV grid that avl_live_map draws, as what a planner reads -- one int8
// cost per cell, lethal cells and an inflated margin around them -- and the clearance to the nearest lethal cell.  The rule is
// stated in include/avl_hip.h above avl_cost_map.  Compiled with -ffp-contract=off like seg_livemap.hip: the filter's double
// accumulation and the ego rectangle's rotation have to round where k_live_map and the NumPy float64 restatement round.
//
// Two launches on the caller's stream and one caller-owned byte plane between them.  The class of a cell costs 9 x C map reads; a
// fused tile would evaluate its R-wide ring again in every neighbouring tile ((32 + 2R)(64 + 2R) / (32 * 64): 2.9 times the work
// at R = 15, 6 times at R = 32), the plane of the window plus its ring costs (h + 2R)(w + 2R) / hw: 1.1 times at 600 x 600, R = 15.
//
// k_cost_base, one workgroup per 16 x 64 tile of the plane (long side along the contiguous Wm axis, as k_live_map):
//   the base cost byte of every cell of the window and its ring of R cells: cost[class] by the render rule of avl_render.h, the
//   cost of "no class" off the grid without a read of the map, 0 under the ego rectangle.
// k_cost_inflate, one workgroup per 32 x 64 output tile, integers only:
//   A  stage: every wave reads rows of the tile plus ring from the plane, 64 bytes per load, and keeps of the ring only one bit
//      per cell: __ballot(byte == lethal), two words per staged row (64 + 2R <= 128 columns).  The tile's own bytes go to LDS.
//   B  row pass: for every staged row and tile column the distance |dx| <= R to the row's nearest lethal cell, or "none" -- the
//      R + 1 bits on either side of the column, then a count of trailing / leading zeros, instead of 2R + 1 byte reads.
//   C  column pass: d2 = min over |dy| <= R of hd(r + dy, c)^2 + dy^2, which is the minimum over the square exactly, walked
//      outwards from dy = 0 and left as soon as dy^2 alone reaches the best so far; then the R * R cut, the table, the rule.
//   D  the tile's results go through LDS so that the stores run along whichever of stride_i, stride_j is 1.
//   R = 0 does no distance work: A reads the tile's bytes alone and B, C are skipped.
#include "avl_common.h"
#include "avl_render.h"

#include <cstdint>

namespace {

constexpr int kBlock = 256;
constexpr int kBH = 16, kBW = 64;            // k_cost_base's tile of the plane
constexpr int kTH = 32, kTW = 64;            // k_cost_inflate's output tile; kTW = one ballot word
constexpr int kMaxR = AVL_COST_MAX_RADIUS;
constexpr int kSH = kTH + 2 * kMaxR;         // staged rows at the largest radius
constexpr int kLdO = kTW + 1;                // the result tile's row pitch in LDS: a column walk (stride_i == 1) spreads over the banks
constexpr int kNone = 255;                   // "no lethal cell within R in this row"; 255 * 255 is beyond every R * R
constexpr int kMaxWindow = 32768;
constexpr int kTabWords = (kMaxR * kMaxR + 1 + 3) / 4;
static_assert(kTW == 64 && kTW + 2 * kMaxR <= 128, "a staged row is two ballot words");
static_assert(kNone * kNone > kMaxR * kMaxR, "kNone must fall to the R * R cut");

struct BaseParams {
    int Hm, Wm, C, flags;
    long long px0, py0;                      // grid cell of the plane's first byte: (x0 - R, y0 - R)
    int ph, pw, ld;                          // the plane: (h + 2R) x (w + 2R) bytes, row pitch ld
    int has_car;
    double car[AVL_LIVE_CAR_DOUBLES];        // cx, cy, cos, sin, u_lo, u_hi, v_lo, v_hi
    signed char cost[AVL_MAX_MAP_CLASSES + 1];
    avl::RenderParams rp;
};

struct InflateParams {
    int h, w, R, ld;
    long long stride_i, stride_j;
    unsigned int tab[kTabWords];             // infl_host, four entries per word
};

// class index of grid cell (gx, gy) -- row gx of Hm, column gy of Wm -- or C for "no class": the composition of avl_render.h's
// helpers that cell_class of seg_livemap.hip makes
template <typename MapT>
__device__ __forceinline__ int cost_cell_class(const MapT* __restrict__ map, const BaseParams& p, int gx, int gy) {
    const int Hm = p.Hm, Wm = p.Wm, C = p.C;
    const bool filt = p.flags & AVL_LIVE_FILTER;
    const MapT* row = map + ((long long)gx * Wm + gy) * C;
    auto value = [&](int c) -> MapT { return filt ? (MapT)avl::box_filter3_taps(map, Hm, Wm, C, gx, gy, c) : row[c]; };
    const int cls = (p.flags & AVL_LIVE_THRESHOLDS) ? avl::thresholds_class<MapT>(C, p.rp, value) : avl::argmax_class<MapT>(C, value);
    return cls == avl::kNoClass ? C : cls;
}

template <typename MapT>
__global__ void __launch_bounds__(kBlock) k_cost_base(const MapT* __restrict__ map, BaseParams p, signed char* __restrict__ plane) {
    const int pi0 = blockIdx.y * kBH, pj0 = blockIdx.x * kBW;
    for (int idx = threadIdx.x; idx < kBH * kBW; idx += kBlock) {
        const int pi = pi0 + idx / kBW, pj = pj0 + idx % kBW;
        if (pi >= p.ph || pj >= p.pw) continue;
        const long long gx = p.px0 + pi, gy = p.py0 + pj;
        int cls = p.C;
        if (gx >= 0 && gx < p.Hm && gy >= 0 && gy < p.Wm) cls = cost_cell_class(map, p, (int)gx, (int)gy);
        int b = p.cost[cls];
        if (p.has_car) {
            const double dx = ((double)gx + 0.5) - p.car[0], dy = ((double)gy + 0.5) - p.car[1];
            const double c = p.car[2], s = p.car[3];
            const double u = c * dx + s * dy, v = c * dy - s * dx;
            if (p.car[4] <= u && u < p.car[5] && p.car[6] <= v && v < p.car[7]) b = 0;
        }
        plane[(long long)pi * p.ld + pj] = (signed char)b;
    }
}

// bits [pos, pos + 64) of the 128-bit row {w0 = columns 0 .. 63, w1 = columns 64 .. 127}, 0 <= pos < 128
__device__ __forceinline__ unsigned long long row_bits_from(unsigned long long w0, unsigned long long w1, int pos) {
    if (pos >= 64) return w1 >> (pos - 64);
    return pos ? (w0 >> pos) | (w1 << (64 - pos)) : w0;
}

__global__ void __launch_bounds__(kBlock) k_cost_inflate(const signed char* __restrict__ plane, InflateParams p,
                                                         signed char* __restrict__ cost_out, unsigned short* __restrict__ d2_out) {
    __shared__ unsigned long long s_bits[kSH * 2];
    __shared__ unsigned char s_hd[kSH * kTW];
    __shared__ signed char s_base[kTH * kTW];
    __shared__ signed char s_out[kTH * kLdO];
    __shared__ unsigned short s_d2[kTH * kLdO];
    __shared__ unsigned int s_tab[kTabWords];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int R = p.R, RR = R * R;
    const int ti0 = blockIdx.y * kTH, tj0 = blockIdx.x * kTW;     // window coordinates of the tile
    const int th = min(kTH, p.h - ti0), tw = min(kTW, p.w - tj0);  // its ragged extent: >= 1 each
    const int rows = th + 2 * R, cols = tw + 2 * R;                // staged; all inside the plane
    for (int k = t; k < (RR + 1 + 3) / 4; k += kBlock) s_tab[k] = p.tab[k];
    // ---- A: staged row sr is plane row ti0 + sr, staged column sc is plane column tj0 + sc; tile cell (r, c) is staged (r + R, c + R)
    for (int sr = wave; sr < rows; sr += kBlock / 64) {
        const signed char* prow = plane + (long long)(ti0 + sr) * p.ld + tj0;
        for (int k = 0; k < (R ? 2 : 1); ++k) {
            const int sc = 64 * k + lane;
            const int b = sc < cols ? prow[sc] : 0;
            const unsigned long long bits = __ballot(b == AVL_COST_LETHAL);
            if (lane == 0) s_bits[sr * 2 + k] = bits;
            const int r = sr - R, c = sc - R;
            if (r >= 0 && r < th && c >= 0 && c < tw) s_base[r * kTW + c] = (signed char)b;
        }
    }
    __syncthreads();
    // ---- B: hd of every staged row at every tile column
    if (R) {
        const unsigned long long side = (1ull << (R + 1)) - 1ull;  // R + 1 <= 33 bits: the column itself and R cells to one side
        for (int sr = wave; sr < rows; sr += kBlock / 64) {
            const unsigned long long w0 = s_bits[sr * 2], w1 = s_bits[sr * 2 + 1];
            const unsigned long long right = row_bits_from(w0, w1, lane + R) & side;   // bit k: dx = +k
            const unsigned long long left = row_bits_from(w0, w1, lane) & side;        // bit k: dx = k - R
            const int dr = right ? __builtin_ctzll(right) : kNone;
            const int dl = left ? R - (63 - __builtin_clzll(left)) : kNone;
            s_hd[sr * kTW + lane] = (unsigned char)min(dr, dl);
        }
        __syncthreads();
    }
    // ---- C
    for (int idx = t; idx < th * kTW; idx += kBlock) {
        const int r = idx / kTW, c = idx % kTW;
        if (c >= tw) continue;
        const int b = s_base[r * kTW + c];
        int d2;
        if (R) {
            const unsigned char* col = s_hd + (r + R) * kTW + c;
            int best = col[0];
            best *= best;
            for (int dy = 1; dy <= R && dy * dy < best; ++dy) {
                const int m = min((int)col[-dy * kTW], (int)col[dy * kTW]);
                best = min(best, m * m + dy * dy);
            }
            d2 = best <= RR ? best : AVL_COST_FAR;
        } else {
            d2 = b == AVL_COST_LETHAL ? 0 : AVL_COST_FAR;
        }
        const int v = d2 <= RR ? (int)reinterpret_cast<const unsigned char*>(s_tab)[d2] : 0;
        const int o = b >= 0 ? max(b, v) : (v > 0 ? v : -1);
        s_out[r * kLdO + c] = (signed char)o;
        s_d2[r * kLdO + c] = (unsigned short)d2;
    }
    __syncthreads();
    // ---- D: lanes along j unless only stride_i is 1 (nav_msgs/OccupancyGrid's order: x runs fastest)
    const bool along_i = p.stride_i == 1 && p.stride_j != 1;
    for (int idx = t; idx < kTH * kTW; idx += kBlock) {
        const int r = along_i ? idx % kTH : idx / kTW, c = along_i ? idx / kTH : idx % kTW;
        if (r >= th || c >= tw) continue;
        const long long off = (long long)(ti0 + r) * p.stride_i + (long long)(tj0 + c) * p.stride_j;
        cost_out[off] = s_out[r * kLdO + c];
        if (d2_out) d2_out[off] = s_d2[r * kLdO + c];
    }
}

bool sizes_ok(int h, int w, int R) { return h >= 1 && w >= 1 && h <= kMaxWindow && w <= kMaxWindow && R >= 0 && R <= kMaxR; }

int plane_ld(int w, int R) { return avl::round16(w + 2 * R); }

}  // namespace

extern "C" int64_t avl_cost_map_scratch_bytes(int h, int w, int radius_cells) {
    if (!sizes_ok(h, w, radius_cells)) return 0;
    return (int64_t)(h + 2 * radius_cells) * plane_ld(w, radius_cells);
}

extern "C" int avl_cost_map(const void* map, int map_dtype, int Hm, int Wm, int C, int x0, int y0, int h, int w, int flags,
                            const int32_t* priority_host, const double* thresholds_host, const int8_t* cost_host,
                            const double* car_host, int radius_cells, const uint8_t* infl_host, int8_t* cost_out, int64_t stride_i,
                            int64_t stride_j, uint16_t* d2_out, void* scratch, int64_t scratch_bytes, void* stream) {
    const int R = radius_cells;
    AVL_REQUIRE(map, "map is NULL");
    AVL_REQUIRE(cost_out, "cost_out is NULL");
    AVL_REQUIRE(cost_host, "cost_host is NULL");
    AVL_REQUIRE(infl_host, "infl_host is NULL");
    AVL_REQUIRE(scratch, "scratch is NULL");
    AVL_REQUIRE(map_dtype == AVL_F64 || map_dtype == AVL_F32, "map dtype %d", map_dtype);
    AVL_REQUIRE(C > 0 && C <= AVL_MAX_MAP_CLASSES, "C = %d (1..%d)", C, AVL_MAX_MAP_CLASSES);
    AVL_REQUIRE(Hm > 0 && Wm > 0 && (long long)Hm * Wm <= 0x7fffffffLL, "grid %d x %d", Hm, Wm);
    AVL_REQUIRE(h >= 1 && w >= 1 && h <= kMaxWindow && w <= kMaxWindow, "window %d x %d (1..%d each)", h, w, kMaxWindow);
    AVL_REQUIRE(R >= 0 && R <= kMaxR, "radius_cells = %d (0..%d)", R, kMaxR);
    AVL_REQUIRE(!(flags & AVL_LIVE_FILL), "AVL_LIVE_FILL: the hole filler is a picture operation, a cost map has none");
    AVL_REQUIRE(!(flags & ~(AVL_LIVE_FILTER | AVL_LIVE_THRESHOLDS)), "flags 0x%x", flags);
    AVL_REQUIRE(!(flags & AVL_LIVE_FILTER) || (Hm > 1 && Wm > 1), "the box filter reflects at the grid's edge: grid %d x %d", Hm, Wm);
    AVL_REQUIRE(!(flags & AVL_LIVE_THRESHOLDS) || thresholds_host, "AVL_LIVE_THRESHOLDS without thresholds_host");
    for (int c = 0; c <= C; ++c)
        AVL_REQUIRE(cost_host[c] >= -1 && cost_host[c] <= AVL_COST_LETHAL, "cost_host[%d] = %d (-1, 0..%d)", c, cost_host[c], AVL_COST_LETHAL);
    AVL_REQUIRE(infl_host[0] == AVL_COST_LETHAL, "infl_host[0] = %d: a lethal cell costs %d", infl_host[0], AVL_COST_LETHAL);
    for (int k = 1; k <= R * R; ++k)
        AVL_REQUIRE(infl_host[k] <= infl_host[k - 1], "infl_host[%d] = %d after %d: the table may not increase", k, infl_host[k], infl_host[k - 1]);
    // h * w distinct elements: positive strides, and the axis with the larger stride steps over the whole extent of the other
    AVL_REQUIRE(stride_i >= 1 && stride_j >= 1 && stride_i <= (1LL << 40) && stride_j <= (1LL << 40), "strides %lld, %lld (1..2^40)",
                (long long)stride_i, (long long)stride_j);
    if (h > 1 && w > 1) {
        const bool i_outer = stride_i >= stride_j;
        const int64_t outer = i_outer ? stride_i : stride_j, inner = i_outer ? stride_j : stride_i;
        AVL_REQUIRE(outer >= inner * (i_outer ? w : h), "strides %lld, %lld alias elements of a %d x %d window", (long long)stride_i,
                    (long long)stride_j, h, w);
    }
    const int64_t need = avl_cost_map_scratch_bytes(h, w, R);
    AVL_REQUIRE(scratch_bytes >= need, "scratch of %lld bytes: avl_cost_map_scratch_bytes(%d, %d, %d) = %lld", (long long)scratch_bytes, h, w,
                R, (long long)need);

    BaseParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.Hm = Hm; bp.Wm = Wm; bp.C = C; bp.flags = flags;
    bp.px0 = (long long)x0 - R; bp.py0 = (long long)y0 - R;
    bp.ph = h + 2 * R; bp.pw = w + 2 * R; bp.ld = plane_ld(w, R);
    const uint8_t no_colors[AVL_MAX_MAP_CLASSES * 3] = {0};   // a cost map has no colours; the render parameters carry a table of them
    int rc;
    if ((rc = avl::fill_render_params(bp.rp, "avl_cost_map", C, no_colors, priority_host, thresholds_host))) return rc;
    memcpy(bp.cost, cost_host, (size_t)C + 1);
    if (car_host) {
        bp.has_car = 1;
        memcpy(bp.car, car_host, sizeof(bp.car));
    }
    InflateParams ip;
    memset(&ip, 0, sizeof(ip));
    ip.h = h; ip.w = w; ip.R = R; ip.ld = bp.ld;
    ip.stride_i = stride_i; ip.stride_j = stride_j;
    memcpy(ip.tab, infl_host, (size_t)R * R + 1);

    signed char* plane = static_cast<signed char*>(scratch);
    const dim3 block(kBlock);
    const dim3 bgrid((unsigned)((bp.pw + kBW - 1) / kBW), (unsigned)((bp.ph + kBH - 1) / kBH));
    if (map_dtype == AVL_F64) hipLaunchKernelGGL(k_cost_base<double>, bgrid, block, 0, avl::as_stream(stream), static_cast<const double*>(map), bp, plane);
    else hipLaunchKernelGGL(k_cost_base<float>, bgrid, block, 0, avl::as_stream(stream), static_cast<const float*>(map), bp, plane);
    AVL_LAUNCH_CHECK();
    const dim3 igrid((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kTH - 1) / kTH));
    hipLaunchKernelGGL(k_cost_inflate, igrid, block, 0, avl::as_stream(stream), plane, ip, reinterpret_cast<signed char*>(cost_out),
                       reinterpret_cast<unsigned short*>(d2_out));
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}
