// Device arithmetic that the end-of-run renderer (mapping.hip), the live-map kernel (seg_livemap.hip), the site overview
// (seg_overview.hip) and the site finish (seg_sitefinish.hip) share, so that a window of the live map, and the finish of a scrolled
// site, are bit-equal to apply_filter + render_bev_map.  All these translation units are built with -ffp-contract=off.
#pragma once
#include "avl_common.h"

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

template <typename MapT>
__device__ __forceinline__ MapT numpy_row_sum(const MapT* row, int C) {
    return numpy_row_sum_of<MapT>(C, [row](int c) { return row[c]; });
}

// the colour of one row of C values that a kernel holds in LDS (the site overview, the site finish): k_render_bev's rule (mapping.hip),
// restated -- first maximum wins, a NaN beats every number and the first NaN wins; black where np.sum of the row is 0
template <typename MapT>
__device__ __forceinline__ void argmax_colour(const MapT* row, int C, const RenderParams& rp, unsigned char* rgb) {
    MapT best = row[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const MapT v = row[c];
        if (v > best || (v != v && best == best)) { best = v; bi = c; }
    }
    unsigned char r = rp.colors[3 * bi], g = rp.colors[3 * bi + 1], b = rp.colors[3 * bi + 2];
    if (numpy_row_sum(row, C) == (MapT)0) r = g = b = 0;
    rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// k_render_thresholds' rule (mapping.hip), restated: the share is a MapT quotient compared with the threshold in MapT, priorities
// from low to high, later ones overwrite
template <typename MapT>
__device__ __forceinline__ void thresholds_colour(const MapT* row, int C, const RenderParams& rp, unsigned char* rgb) {
    const MapT s = numpy_row_sum(row, C);
    unsigned char r = 0, g = 0, b = 0;
    if (s != (MapT)0) {
        for (int i = 0; i < C; ++i) {
            const int ch = rp.priority[i];
            const MapT pn = row[ch] / s;
            if (pn >= (MapT)rp.thresholds[i]) { r = rp.colors[3 * ch]; g = rp.colors[3 * ch + 1]; b = rp.colors[3 * ch + 2]; }
        }
    }
    rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// k_eval_map's colour -> label table (mapping.hip; convert_labels of test/test_semantic_mapping.py:6-19), restated
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

}  // namespace avl
