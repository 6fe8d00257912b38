// The prior point map of a site, tiled on the ground and cropped per frame (not in the reference: its SemanticMapping subscribes to
// /reduced_map, src/mapping.py:61-62, and unpacks whatever an outside node crops and republishes, :172-183).  The whole map is put
// on the device once, sorted by ground tile once (vision_semantic_segmentation_amd/points_map.py), and every frame the tiles that
// can hold a voting point are copied into one contiguous float32 [M][4] cloud that the frame entry points take as any other.
//
//   k_tile_keys           one lane per point: the tile key by the tile rule of include/avl_hip.h, -1 for a dropped point.  Runs once,
//                         at load; the stable sort by key, the histogram and its prefix sum are torch's.
//   k_points_map_gather   the per-frame kernel.  The rectangle's rows r0..r1 are runs of the sorted cloud.  Every workgroup reads
//                         the two offsets of each row, scans the run lengths in LDS (kBlock rows per pass: __shfl_up inside a wave,
//                         the four wave totals through LDS, the carry of the earlier passes in a register), then every lane finds
//                         the run of each of its kPtsPerLane output points by bisection of the inclusive prefix in LDS and copies
//                         the point as one 16-byte load and one 16-byte store.  No atomics; every lane reaches every barrier.
//   avl_points_map_window host only: M and the non-empty runs of a rectangle from the HOST copy of the offsets.  The host so knows M
//                         before anything is launched, which is what lets the result go to entry points that take n as a host integer.
//
// Compiled with -ffp-contract=off (MAPFLAGS): the key's subtraction, division and floor are the three float64 operations as written.
#include "avl_common.h"

#include <cstdint>

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kGatherMaxRows = 1024;                     // rows of the rectangle one launch takes; a taller rectangle goes as several
constexpr int kPtsPerLane = 4;
constexpr int kPtsPerWg = kBlock * kPtsPerLane;
constexpr int kMaxTiles = 1 << 24;

__global__ void __launch_bounds__(kBlock) k_tile_keys(const float4* __restrict__ pts, int n, double ox, double oy, double tile_m, int rows,
                                                      int cols, int32_t* __restrict__ keys) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const float4 p = pts[k];
    int32_t key = -1;
    const bool nan = p.x != p.x || p.y != p.y || p.z != p.z || p.w != p.w;
    if (!nan && !__builtin_isinf(p.x) && !__builtin_isinf(p.y)) {
        const double fx = __builtin_floor(((double)p.x - ox) / tile_m);
        const double fy = __builtin_floor(((double)p.y - oy) / tile_m);
        // inside by construction (ox, oy, rows, cols come from the bounds of the kept points); a caller's wrong bounds drop the point
        if (fx >= 0.0 && fx < (double)rows && fy >= 0.0 && fy < (double)cols) key = (int32_t)fx * cols + (int32_t)fy;
    }
    keys[k] = key;
}

// rows ra .. ra + nrows - 1 of the rectangle, columns c0..c1, to dst[0 .. m): m is the host's count of the same runs
__global__ void __launch_bounds__(kBlock) k_points_map_gather(const float4* __restrict__ pts, const int32_t* __restrict__ offsets, int cols,
                                                              int ra, int nrows, int c0, int c1, float4* __restrict__ dst, int m) {
    __shared__ int32_t s_inc[kGatherMaxRows];            // inclusive prefix of the run lengths
    __shared__ int32_t s_start[kGatherMaxRows];          // first point of each run in the sorted cloud
    __shared__ int32_t s_wave[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < nrows; base += kBlock) {   // uniform trip count: the barriers below are reached by every lane
        const int row = base + tid;
        int start = 0, len = 0;
        if (row < nrows) {
            const int64_t o = (int64_t)(ra + row) * cols;
            start = offsets[o + c0];
            len = offsets[o + c1 + 1] - start;
        }
        int inc = len;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int before = carry, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            const int t = s_wave[w];
            if (w < wave) before += t;
            total += t;
        }
        if (row < nrows) {
            s_inc[row] = before + inc;
            s_start[row] = start;
        }
        carry += total;
        __syncthreads();                                 // s_wave is rewritten by the next pass; s_inc is read below
    }
    const int m_dev = carry < m ? carry : m;             // equal unless the two copies of the offsets differ: then the smaller bounds the copy
    const int first = blockIdx.x * kPtsPerWg + tid;
    for (int j = 0; j < kPtsPerLane; ++j) {
        const int i = first + j * kBlock;
        if (i < m_dev) {
            int lo = 0, hi = nrows - 1;                  // the first row whose inclusive prefix exceeds i: it exists, i < s_inc[nrows - 1]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_inc[mid] > i) hi = mid; else lo = mid + 1;
            }
            const int excl = lo > 0 ? s_inc[lo - 1] : 0;
            dst[i] = pts[s_start[lo] + (i - excl)];
        }
    }
}

// M and the non-empty runs of the rows ra..rb; the offsets are checked to be non-decreasing where they are read
int count_runs(const int32_t* offsets, int cols, int ra, int rb, int c0, int c1, int64_t* m, int* runs) {
    int64_t total = 0;
    int nonempty = 0;
    for (int r = ra; r <= rb; ++r) {
        const int64_t o = (int64_t)r * cols;
        const int64_t len = (int64_t)offsets[o + c1 + 1] - (int64_t)offsets[o + c0];
        AVL_REQUIRE(len >= 0 && offsets[o + c0] >= 0, "points map offsets decrease in tile row %d", r);
        total += len;
        nonempty += len > 0;
    }
    *m = total;
    *runs = nonempty;
    return AVL_OK;
}

int check_rect(const char* who, int rows, int cols, int r0, int r1, int c0, int c1, bool* empty) {
    AVL_REQUIRE(rows >= 0 && cols >= 0 && (int64_t)rows * cols <= kMaxTiles, "%s: %d x %d tiles (at most 2^24)", who, rows, cols);
    *empty = r0 > r1 || c0 > c1;
    if (!*empty)
        AVL_REQUIRE(r0 >= 0 && r1 < rows && c0 >= 0 && c1 < cols, "%s: rectangle rows %d..%d, columns %d..%d leaves the %d x %d tiles", who, r0,
                    r1, c0, c1, rows, cols);
    return AVL_OK;
}

}  // namespace

extern "C" {

int avl_points_map_keys(const float* points, int64_t n, double ox, double oy, double tile_m, int rows, int cols, int32_t* keys, void* stream) {
    AVL_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "avl_points_map_keys: n = %lld (0 .. 2^31 - 1)", (long long)n);
    AVL_REQUIRE(tile_m > 0.0 && tile_m == tile_m && !__builtin_isinf(tile_m), "avl_points_map_keys: tile_m = %g", tile_m);
    AVL_REQUIRE(ox == ox && oy == oy && !__builtin_isinf(ox) && !__builtin_isinf(oy), "avl_points_map_keys: origin (%g, %g)", ox, oy);
    AVL_REQUIRE(rows >= 0 && cols >= 0 && (int64_t)rows * cols <= kMaxTiles, "avl_points_map_keys: %d x %d tiles (at most 2^24)", rows, cols);
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(points != nullptr && keys != nullptr, "avl_points_map_keys: points or keys is NULL");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(points) & 15) == 0, "avl_points_map_keys: points is not 16-byte aligned");
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_tile_keys, dim3(blocks), dim3(kBlock), 0, avl::as_stream(stream), reinterpret_cast<const float4*>(points), (int)n, ox,
                       oy, tile_m, rows, cols, keys);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

int avl_points_map_window(const int32_t* offsets_host, int rows, int cols, int r0, int r1, int c0, int c1, int64_t* m_out, int32_t* runs_out) {
    AVL_REQUIRE(m_out != nullptr && runs_out != nullptr, "avl_points_map_window: m_out or runs_out is NULL");
    bool empty = false;
    if (int rc = check_rect("avl_points_map_window", rows, cols, r0, r1, c0, c1, &empty)) return rc;
    *m_out = 0;
    *runs_out = 0;
    if (empty) return AVL_OK;
    AVL_REQUIRE(offsets_host != nullptr, "avl_points_map_window: offsets_host is NULL");
    int runs = 0;
    if (int rc = count_runs(offsets_host, cols, r0, r1, c0, c1, m_out, &runs)) return rc;
    *runs_out = runs;
    return AVL_OK;
}

int avl_points_map_gather(const float* points, const int32_t* offsets_dev, const int32_t* offsets_host, int rows, int cols, int r0, int r1,
                          int c0, int c1, float* dst, int64_t dst_capacity, void* stream) {
    bool empty = false;
    if (int rc = check_rect("avl_points_map_gather", rows, cols, r0, r1, c0, c1, &empty)) return rc;
    if (empty) return AVL_OK;
    AVL_REQUIRE(offsets_host != nullptr, "avl_points_map_gather: offsets_host is NULL");
    int64_t m = 0;
    int runs = 0;
    if (int rc = count_runs(offsets_host, cols, r0, r1, c0, c1, &m, &runs)) return rc;
    AVL_REQUIRE(m < ((int64_t)1 << 31), "avl_points_map_gather: %lld points", (long long)m);
    AVL_REQUIRE(dst_capacity >= m, "avl_points_map_gather: dst holds %lld points, the rectangle has %lld", (long long)dst_capacity, (long long)m);
    if (m == 0) return AVL_OK;
    AVL_REQUIRE(points != nullptr && offsets_dev != nullptr && dst != nullptr, "avl_points_map_gather: points, offsets_dev or dst is NULL");
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(points) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0,
                "avl_points_map_gather: points and dst must be 16-byte aligned");
    int64_t done = 0;
    for (int ra = r0; ra <= r1; ra += kGatherMaxRows) {
        const int rb = ra + kGatherMaxRows - 1 < r1 ? ra + kGatherMaxRows - 1 : r1;
        int64_t mc = 0;
        if (int rc = count_runs(offsets_host, cols, ra, rb, c0, c1, &mc, &runs)) return rc;
        if (mc == 0) continue;
        const unsigned blocks = (unsigned)((mc + kPtsPerWg - 1) / kPtsPerWg);
        hipLaunchKernelGGL(k_points_map_gather, dim3(blocks), dim3(kBlock), 0, avl::as_stream(stream), reinterpret_cast<const float4*>(points),
                           offsets_dev, cols, ra, rb - ra + 1, c0, c1, reinterpret_cast<float4*>(dst) + done, (int)mc);
        AVL_LAUNCH_CHECK();
        done += mc;
    }
    return AVL_OK;
}

}  // extern "C"
