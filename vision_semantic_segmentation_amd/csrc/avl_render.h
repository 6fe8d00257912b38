// The render rule -- which class a cell of the grid shows, and in which colour -- in device code, and what the launch layer needs to
// feed it.  The end-of-run renderer (mapping.hip), the live kernels (seg_livemap.hip), the site overview (seg_overview.hip) and the
// site finish (seg_sitefinish.hip) all call it, so a window of the live map, and the finish of a scrolled site, are bit-equal to
// apply_filter + render_bev_map.  All these translation units are built with -ffp-contract=off.
#pragma once
#include "avl_common.h"

#include <cstdint>

namespace avl {

struct RenderParams {
    unsigned char colors[AVL_MAX_MAP_CLASSES * 3];
    int priority[AVL_MAX_MAP_CLASSES];
    double thresholds[AVL_MAX_MAP_CLASSES];
};

// np.sum(map, axis=2) of one contiguous row, in the map's own type and in NumPy's order (pairwise_sum in NumPy's
// umath/loops_utils.h.src; C <= 16 stays below its 128-element block): fewer than 8 values are a left fold from 0; from 8 up,
// eight accumulators r[j] = a[j], r[j] += a[i + j] for every further whole group of 8, then
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then a left fold of the remainder.  Which cells count as empty (sum == 0)
// and the shares of the thresholds renderer depend on this rounding.  `at(c)` yields element c of the row.
template <typename MapT, typename At>
__device__ __forceinline__ MapT numpy_row_sum_of(int C, At at) {
    if (C < 8) {
        MapT s = (MapT)0;
        for (int c = 0; c < C; ++c) s = s + at(c);
        return s;
    }
    MapT r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = at(j);
    int i = 8;
    for (; i + 8 <= C; i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + at(i + j);
    MapT s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < C; ++i) s = s + at(i);
    return s;
}

// ---------------------------------------------------------------------------------------------- THE RENDER RULE, stated here and
// nowhere else.  Every kernel that colours a cell -- k_render_bev, k_render_thresholds (mapping.hip), k_live_map, k_live_view
// (seg_livemap.hip), k_site_overview (seg_overview.hip), k_site_finish (seg_sitefinish.hip) -- calls these with its own accessor
// `at(c)`, element c of the cell's row: a row in global memory, a row in LDS, or the nine-tap filter of the live kernels.
constexpr int kNoClass = -1;    // the cell stays black

// render_bev_map (renderer.py:32-59): the class of np.argmax -- the first maximum wins, a NaN beats every number and the first NaN
// wins -- or kNoClass where np.sum of the row is 0.  One pass: `at` is called once per channel, in ascending order, by the row sum.
// The two conditions are joined with | and not ||: both are cheap and free of side effects, and the channels then cost selects,
// not a branch each.
template <typename MapT, typename At>
__device__ __forceinline__ int argmax_class(int C, At at) {
    MapT best = (MapT)0;
    int bi = 0;
    const MapT s = numpy_row_sum_of<MapT>(C, [&](int c) -> MapT {
        const MapT v = at(c);
        const bool first_nan = v != v && best == best;
        if (c == 0) best = v;
        else if ((v > best) | first_nan) { best = v; bi = c; }
        return v;
    });
    return s == (MapT)0 ? kNoClass : bi;
}

// render_bev_map_with_thresholds (renderer.py:131-172): the share is a MapT quotient -- np.divide(map, channel_sum) has the map's
// element type -- compared with the threshold in MapT (NumPy compares a float32 array with a Python float in float32); priorities
// run from low to high and later ones overwrite.  `at(ch)` is evaluated again per priority entry: no per-thread array of C values.
template <typename MapT, typename At>
__device__ __forceinline__ int thresholds_class(int C, const RenderParams& rp, At at) {
    const MapT s = numpy_row_sum_of<MapT>(C, at);
    int cls = kNoClass;
    if (s != (MapT)0) {
        for (int k = 0; k < C; ++k) {
            const int ch = rp.priority[k];
            const MapT pn = at(ch) / s;
            if (pn >= (MapT)rp.thresholds[k]) cls = ch;
        }
    }
    return cls;
}

// class -> colour; kNoClass is black
__device__ __forceinline__ void class_colour(int cls, const RenderParams& rp, unsigned char* rgb) {
    unsigned char r = 0, g = 0, b = 0;
    if (cls != kNoClass) { r = rp.colors[3 * cls]; g = rp.colors[3 * cls + 1]; b = rp.colors[3 * cls + 2]; }
    rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// the colour of a contiguous row of C values (global memory or LDS) under either pick
template <typename MapT>
__device__ __forceinline__ void row_colour(const MapT* row, int C, bool thresholds, const RenderParams& rp, unsigned char* rgb) {
    auto at = [row](int c) -> MapT { return row[c]; };
    class_colour(thresholds ? thresholds_class<MapT>(C, rp, at) : argmax_class<MapT>(C, at), rp, rgb);
}

// convert_labels (test/test_semantic_mapping.py:6-19): label 1..5 for the five map colours, exact three-channel match, else 0
__device__ __forceinline__ int colour_label(unsigned char r, unsigned char g, unsigned char b) {
    if (r == 128 && g == 64 && b == 128) return 1;            // road
    if (r == 140 && g == 140 && b == 200) return 2;           // crosswalk
    if (r == 255 && g == 255 && b == 255) return 3;           // lane
    if (r == 244 && g == 35 && b == 232) return 4;            // sidewalk
    if (r == 107 && g == 142 && b == 35) return 5;            // vegetation
    return 0;
}

// apply_filter (renderer.py:175-189) at cell (y, x), channel c of src [Hm][Wm][C]: cv2.filter2D with ones(3,3,float32)/9,
// BORDER_REFLECT_101 at the grid's edge, the nine products accumulated in double (dy outer, dx inner); the caller rounds to MapT.
template <typename MapT>
__device__ __forceinline__ double box_filter3_taps(const MapT* __restrict__ src, int Hm, int Wm, int C, int y, int x, int c) {
    const double k = (double)(1.0f / 9.0f);
    double acc = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        int yy = y + dy;
        yy = yy < 0 ? -yy : (yy >= Hm ? 2 * Hm - 2 - yy : yy);
        for (int dx = -1; dx <= 1; ++dx) {
            int xx = x + dx;
            xx = xx < 0 ? -xx : (xx >= Wm ? 2 * Wm - 2 - xx : xx);
            acc = acc + k * (double)src[((long long)yy * Wm + xx) * C + c];
        }
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------- the launch layer's share
// RenderParams from host arrays, for `who` (the entry point's name, in the message): priority NULL = 0 .. C - 1, thresholds NULL =
// 0.01 each (render_bev_map_with_thresholds' default).  C is in 1 .. AVL_MAX_MAP_CLASSES and colors is not NULL: the callers check.
inline int fill_render_params(RenderParams& rp, const char* who, int C, const uint8_t* colors, const int32_t* priority,
                              const double* thresholds) {
    memset(&rp, 0, sizeof(rp));
    memcpy(rp.colors, colors, 3 * (size_t)C);
    for (int k = 0; k < C; ++k) {
        rp.priority[k] = priority ? priority[k] : k;
        AVL_REQUIRE(rp.priority[k] >= 0 && rp.priority[k] < C, "%s: priority[%d] = %d", who, k, rp.priority[k]);
        rp.thresholds[k] = thresholds ? thresholds[k] : 0.01;
    }
    return AVL_OK;
}

inline int round16(int v) { return (v + 15) & ~15; }

// what avl_site_overview and avl_site_finish ask of a tile table and its rectangle of nh x nw tiles of tile_cells x tile_cells cells
inline int check_tile_table(const char* who, const void* tiles_dev, int n_tiles, int nh, int nw, int tile_cells, int min_cells, int C,
                            int map_dtype) {
    AVL_REQUIRE(tile_cells >= min_cells && tile_cells <= (1 << 14), "%s: tile_cells = %d (%d .. 16384)", who, tile_cells, min_cells);
    AVL_REQUIRE(C >= 1 && C <= AVL_MAX_MAP_CLASSES, "%s: C = %d (1 .. %d)", who, C, AVL_MAX_MAP_CLASSES);
    AVL_REQUIRE(map_dtype == AVL_F64 || map_dtype == AVL_F32, "%s: map dtype %d", who, map_dtype);
    const int es = map_dtype == AVL_F64 ? 8 : 4;
    AVL_REQUIRE((tile_cells * C * es) % 16 == 0, "%s: a tile row of %d cells of %d bytes is no multiple of 16 bytes", who, tile_cells, C * es);
    AVL_REQUIRE(nh > 0 && nw > 0, "%s: a rectangle of nh = %d x nw = %d tiles", who, nh, nw);
    AVL_REQUIRE(n_tiles >= 0 && (long long)n_tiles <= (long long)nh * nw, "%s: n_tiles = %d (0 .. nh * nw = %lld)", who, n_tiles,
                (long long)nh * nw);
    AVL_REQUIRE(n_tiles == 0 || tiles_dev != nullptr, "%s: tiles_dev is NULL for %d tiles", who, n_tiles);
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(tiles_dev) & 7) == 0, "%s: tiles_dev is misaligned", who);
    return AVL_OK;
}

}  // namespace avl
