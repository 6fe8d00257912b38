// Semantic extraction: per-class connected components and convex hulls of a label map
// (src/semantic_convex_hull.py:17-91, called from src/vision_semantic_segmentation_node.py:138-152).
//
// A "plane" is one (label map, class index) pair; P = n * n_classes planes run in the same launches (blockIdx.z, or
// blockIdx.y for the small per-plane kernels).  Stages, all on the caller's stream with no host synchronisation:
//
//   k_ccl_tile     mask (label == class), 3x3 erosion fused into the tile load (:36-45), and an 8-connected union-find of one
//                  64 x 16 tile in LDS (:51).  Every foreground pixel leaves with parent + 1 = 1 + the smallest linear index
//                  y * w + x of its component INSIDE the tile; background is 0.
//   k_ccl_merge    one thread per pixel of a tile's first row / first column: atomicMin unions across the tile borders.
//   k_ccl_flatten  every pixel replaces its parent by its root: label = 1 + smallest linear index of the component.
//   k_hull_area    integer atomic count per root (:59), one atomic per (wave, root).
//   k_hull_topk    per 4096-entry chunk the top_number largest (area descending, label ascending);
//   k_hull_select  merges the chunks' candidates per plane, applies area > area_threshold (:60), resets the row extremes.
//   k_hull_rows    per selected component and row the leftmost / rightmost pixel (atomicMin / atomicMax at run ends only),
//                  without the component's raster-first pixel when drop_first is set (crosswalk_pts[1:], :71).
//   k_hull_chain   one wave per (plane, component): monotone chain over the <= 2h row extremes (:74), strict vertices.
//
// Every loop ends by construction.  A parent is never larger than its child (parent[x] <= x, only atomicMin writes after the
// initialisation), so a root walk visits strictly decreasing indices; a union retries only with a strictly smaller index; the
// wave-aggregation loops retire at least one lane per round; the chain only pops what it pushed.  No kernel waits for another
// workgroup.
//
// Unpinned against the reference's libraries (cv2 and skimage are not available to the tests; tests/_hull_reference.py states
// the same assumptions with scipy):
//   * cv2.erode's default border: pixels outside the image do not erode (BORDER_CONSTANT with the morphology default value);
//   * skimage.measure.label numbers components in raster order of their first pixel; here the label IS that pixel's linear
//     index + 1, which has the same order (Counter.most_common's tie-break, :59, is therefore "smaller label first");
//   * cv2.convexHull's vertex order and start: here the hull starts at the smallest (x, then y) and runs with positive cross
//     products on (x, y) as stored (counter-clockwise with x right, y up).
#include "avl_common.h"

#include <climits>
#include <cstdint>

namespace {

constexpr int kTW = 64, kTH = 16, kTile = kTW * kTH;   // one workgroup's tile
constexpr int kBlock = 256;
constexpr int kChunk = 4096;                            // area entries per k_hull_topk workgroup
constexpr int kMaxTop = 8;
constexpr int kMaxClasses = 64;
constexpr int kLdsStack = 4096;                         // chain stack entries kept in LDS (h <= 2047); larger h: the scratch stack

struct ClassList { unsigned char c[kMaxClasses]; };

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------ union-find pieces
// LDS: parent index inside the tile, -1 = background
__device__ __forceinline__ int lds_find(int* lab, int x) {
    for (;;) {                                                       // lab[x] <= x: strictly decreasing until the root
        const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
    for (;;) {                                                       // a + b strictly decreases from round to round
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                // a > b: hang root a under b
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;                                                     // someone else moved a first: old < a
    }
}
// global: value = parent + 1, 0 = background.  Inside k_ccl_merge other workgroups change parents: agent-scope atomic loads
// (an older parent would still be an ancestor, so even a stale value could only lengthen the walk).
__device__ __forceinline__ int g_find(int* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b + 1) - 1;
        if (old == a) return;
        a = old;
    }
}

// ------------------------------------------------------------------------------------------------ labelling
__global__ void __launch_bounds__(kBlock) k_ccl_tile(const unsigned char* __restrict__ maps, int h, int w, ClassList classes,
                                                     int n_classes, int erode, int* __restrict__ labels) {
    __shared__ unsigned char raw[(kTH + 2) * (kTW + 2)];
    __shared__ int lab[kTile];
    const int plane = blockIdx.z;
    const unsigned char cls = classes.c[plane % n_classes];
    const unsigned char* map = maps + (size_t)(plane / n_classes) * h * w;
    int* L = labels + (size_t)plane * h * w;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    // tile + 1-pixel halo of (label == class); outside the image = 1: such a neighbour does not erode
    for (int i = threadIdx.x; i < (kTH + 2) * (kTW + 2); i += kBlock) {
        const int gy = y0 - 1 + i / (kTW + 2), gx = x0 - 1 + i % (kTW + 2);
        raw[i] = (gy < 0 || gy >= h || gx < 0 || gx >= w) ? 1 : (map[(size_t)gy * w + gx] == cls);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile; i += kBlock) {
        const int ly = i / kTW, lx = i % kTW;
        const unsigned char* r = raw + (ly + 1) * (kTW + 2) + lx + 1;
        int m = r[0];
        if (erode)
            m &= r[-(kTW + 2) - 1] & r[-(kTW + 2)] & r[-(kTW + 2) + 1] & r[-1] & r[1] & r[(kTW + 2) - 1] & r[kTW + 2] & r[(kTW + 2) + 1];
        if (y0 + ly >= h || x0 + lx >= w) m = 0;
        lab[i] = m ? i : -1;
    }
    __syncthreads();
    // links to the four neighbours earlier in raster order.  With N set, W / NW / NE are already tied to N by their own links
    // (NW and NE are N's row neighbours, W has N as its NE), so one union serves.
    for (int i = threadIdx.x; i < kTile; i += kBlock) {
        if (lab[i] < 0) continue;
        const int ly = i / kTW, lx = i % kTW;
        if (ly > 0 && lab[i - kTW] >= 0) { lds_union(lab, i, i - kTW); continue; }
        if (lx > 0 && lab[i - 1] >= 0) lds_union(lab, i, i - 1);
        if (ly > 0 && lx > 0 && lab[i - kTW - 1] >= 0) lds_union(lab, i, i - kTW - 1);
        if (ly > 0 && lx < kTW - 1 && lab[i - kTW + 1] >= 0) lds_union(lab, i, i - kTW + 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile; i += kBlock) {
        const int gy = y0 + i / kTW, gx = x0 + i % kTW;
        if (gy >= h || gx >= w) continue;
        int v = 0;
        if (lab[i] >= 0) {
            const int r = lds_find(lab, i);
            v = (y0 + r / kTW) * w + x0 + r % kTW + 1;
        }
        L[gy * w + gx] = v;
    }
}

// items of one plane: the pixels of every tile's first row (y = kTH, 2 kTH, ...), then of every tile's first column
__global__ void __launch_bounds__(kBlock) k_ccl_merge(int h, int w, int* __restrict__ labels) {
    const int nbr = (h - 1) / kTH, nbc = (w - 1) / kTW;
    const long long item = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long n_row_items = (long long)nbr * w;
    if (item >= n_row_items + (long long)nbc * h) return;
    int* L = labels + (size_t)blockIdx.z * h * w;
    int x, y;
    bool row_item = item < n_row_items;
    if (row_item) { y = ((int)(item / w) + 1) * kTH; x = (int)(item % w); }
    else { const long long j = item - n_row_items; x = ((int)(j / h) + 1) * kTW; y = (int)(j % h); }
    const int i = y * w + x;
    if (L[i] == 0) return;                                            // foreground never changes: a plain load serves
    if (row_item) {                                                   // the three neighbours of the row above
        for (int dx = -1; dx <= 1; ++dx)
            if (x + dx >= 0 && x + dx < w && L[i - w + dx] != 0) g_union(L, i, i - w + dx);
    } else {                                                          // the three neighbours of the column to the left
        for (int dy = -1; dy <= 1; ++dy)
            if (y + dy >= 0 && y + dy < h && L[i + dy * w - 1] != 0) g_union(L, i, i + dy * w - 1);
    }
}

// After the merge no root changes any more.  Writing a root over a parent while other threads still walk is harmless: both are
// ancestors of the pixel, and an aligned 32-bit store is not torn.
__global__ void __launch_bounds__(kBlock) k_ccl_flatten(int hw, int* __restrict__ labels) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= hw) return;
    int* L = labels + (size_t)blockIdx.z * hw;
    if (L[i] == 0) return;
    int x = i;
    for (;;) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
        if (p == x) break;
        x = p;
    }
    __hip_atomic_store(L + i, x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------ areas and selection
__global__ void __launch_bounds__(kBlock) k_hull_area(int hw, const int* __restrict__ labels, int* __restrict__ area) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int v = i < hw ? labels[(size_t)blockIdx.z * hw + i] : 0;
    int* A = area + (size_t)blockIdx.z * hw;
    const int lane = threadIdx.x & 63;
    bool active = v > 0;
    for (int round = 0; round < 64; ++round) {                        // every round retires the leader's root: <= 64 rounds
        const u64 todo = __ballot(active);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int rv = __shfl(v, leader, 64);
        const bool same = active && v == rv;
        const u64 mates = __ballot(same);
        if (lane == leader) atomicAdd(A + rv - 1, (int)__popcll(mates));
        if (same) active = false;
    }
}

// key of a component: larger area first, then the smaller label (Counter.most_common keeps first-seen order among ties)
__device__ __forceinline__ u64 area_key(int area, int index) { return area > 0 ? ((u64)(unsigned)area << 32) | (0xFFFFFFFFu - (unsigned)index) : 0; }

__device__ __forceinline__ u64 block_max(u64 v, u64* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    __syncthreads();                                                  // red[] of the previous round has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 m = red[0];
    for (int k = 1; k < kBlock / 64; ++k) m = red[k] > m ? red[k] : m;
    return m;
}

// the `top` largest keys of key_at(0 .. n-1) in descending order into out[0 .. top-1] (0 = no more); keys are distinct
template <class F>
__device__ __forceinline__ void block_topk(F key_at, int n, int top, u64* out, u64* red) {
    u64 prev = ~0ull;
    for (int t = 0; t < top; ++t) {
        u64 best = 0;
        if (prev != 0)
            for (int i = threadIdx.x; i < n; i += kBlock) {
                const u64 k = key_at(i);
                if (k < prev && k > best) best = k;
            }
        prev = prev != 0 ? block_max(best, red) : 0;
        if (threadIdx.x == 0) out[t] = prev;
    }
}

__global__ void __launch_bounds__(kBlock) k_hull_topk(int hw, const int* __restrict__ area, int top, u64* __restrict__ partial) {
    __shared__ u64 red[kBlock / 64];
    const int* A = area + (size_t)blockIdx.z * hw;
    const int base = blockIdx.x * kChunk;
    const int n = min(kChunk, hw - base);
    block_topk([&](int i) { return area_key(A[base + i], base + i); }, n, top,
               partial + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * kMaxTop, red);
}

__global__ void __launch_bounds__(kBlock) k_hull_select(int h, int n_chunks, int top, int area_threshold, const u64* __restrict__ partial,
                                                        int* __restrict__ roots, int* __restrict__ areas, int* __restrict__ rowmin,
                                                        int* __restrict__ rowmax) {
    __shared__ u64 red[kBlock / 64];
    __shared__ u64 best[kMaxTop];
    const int plane = blockIdx.x;
    const u64* part = partial + (size_t)plane * n_chunks * kMaxTop;
    block_topk([&](int i) { return (i % kMaxTop) < top ? part[i] : 0; }, n_chunks * kMaxTop, top, best, red);
    __syncthreads();
    if (threadIdx.x < top) {
        const u64 k = best[threadIdx.x];
        const int a = (int)(k >> 32);
        const bool keep = a > 0 && a > area_threshold;                // strict (:60)
        roots[plane * top + threadIdx.x] = keep ? (int)(0xFFFFFFFFu - (unsigned)k) + 1 : 0;
        areas[plane * top + threadIdx.x] = keep ? a : 0;
    }
    for (int i = threadIdx.x; i < top * h; i += kBlock) {
        rowmin[(size_t)plane * top * h + i] = INT_MAX;
        rowmax[(size_t)plane * top * h + i] = -1;
    }
}

// ------------------------------------------------------------------------------------------------ hull
// Only the ends of a row's runs can be its leftmost / rightmost pixel, so only they reach for the atomics.
__global__ void __launch_bounds__(kBlock) k_hull_rows(int h, int w, const int* __restrict__ labels, int top, int drop_first,
                                                      const int* __restrict__ roots, int* __restrict__ rowmin, int* __restrict__ rowmax) {
    const int hw = h * w;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= hw) return;
    const int plane = blockIdx.z;
    const int* L = labels + (size_t)plane * hw;
    const int v = L[i];
    if (v == 0) return;
    int k = -1;
    for (int t = 0; t < top; ++t)
        if (roots[plane * top + t] == v) k = t;
    if (k < 0) return;
    if (drop_first && i + 1 == v) return;                             // the raster-first pixel of the component (:71)
    const int y = i / w, x = i - y * w;
    const bool left = x > 0 && L[i - 1] == v && !(drop_first && i == v);
    const bool right = x < w - 1 && L[i + 1] == v;
    const size_t row = ((size_t)plane * top + k) * h + y;
    if (!left) atomicMin(rowmin + row, x);
    if (!right) atomicMax(rowmax + row, x);
}

// One wave per (component, plane); the whole wave runs the chain in lock step (uniform control flow, every lane holds the same
// stack state and stores the same values), 64 rows are fetched at a time and handed round with shuffles.
// The candidates come sorted by (y, x) for free, so the chain runs in that order with the roles of x and y swapped in the turn
// test; the result is then reversed and rotated to the order the header documents.
struct Chain {
    int2* st;
    int size, ax, ay, bx, by;
    __device__ __forceinline__ void push(int px, int py, int floor_size) {
        while (size >= floor_size) {                                  // pops only what was pushed
            const long long turn = (long long)(by - ay) * (px - ax) - (long long)(bx - ax) * (py - ay);
            if (turn > 0) break;
            --size;
            bx = ax; by = ay;
            if (size >= 2) { const int2 a = st[size - 2]; ax = a.x; ay = a.y; }
        }
        st[size] = make_int2(px, py);
        ax = bx; ay = by; bx = px; by = py;
        ++size;
    }
};

__global__ void __launch_bounds__(64) k_hull_chain(int h, int top, const int* __restrict__ roots, const int* __restrict__ rowmin,
                                                   const int* __restrict__ rowmax, int2* __restrict__ stack_scratch,
                                                   int* __restrict__ vertices, int* __restrict__ n_vertices) {
    __shared__ int2 lds_stack[kLdsStack];
    const int slot = blockIdx.y * top + blockIdx.x;                   // plane * top + k
    const int lane = threadIdx.x;
    const int cap = 2 * h + 1;
    if (roots[slot] == 0) { if (lane == 0) n_vertices[slot] = 0; return; }
    const int* mn_row = rowmin + (size_t)slot * h;
    const int* mx_row = rowmax + (size_t)slot * h;
    Chain c;
    c.st = cap <= kLdsStack ? lds_stack : stack_scratch + (size_t)slot * cap;
    c.size = 0; c.ax = c.ay = c.bx = c.by = 0;
    const int n_blocks = (h + 63) / 64;
    for (int blk = 0; blk < n_blocks; ++blk) {                        // rows upwards: (min, y) then (max, y)
        const int y = blk * 64 + lane;
        const int mn = y < h ? mn_row[y] : INT_MAX, mx = y < h ? mx_row[y] : -1;
        u64 has = __ballot(mn <= mx);
        while (has) {
            const int j = __ffsll((long long)has) - 1;
            has &= has - 1;
            const int a = __shfl(mn, j, 64), b = __shfl(mx, j, 64);
            c.push(a, blk * 64 + j, 2);
            if (b > a) c.push(b, blk * 64 + j, 2);
        }
    }
    int m = c.size;                                                   // 0: nothing left after the drop; 1: a single pixel
    if (m >= 2) {
        const int floor_size = c.size + 1;
        bool skip = true;                                             // the last candidate is already on the stack
        for (int blk = n_blocks - 1; blk >= 0; --blk) {               // and back: (max, y) then (min, y)
            const int y = blk * 64 + lane;
            const int mn = y < h ? mn_row[y] : INT_MAX, mx = y < h ? mx_row[y] : -1;
            u64 has = __ballot(mn <= mx);
            while (has) {
                const int j = 63 - __clzll((long long)has);
                has &= ~(1ull << j);
                const int a = __shfl(mn, j, 64), b = __shfl(mx, j, 64);
                if (!skip) c.push(b, blk * 64 + j, floor_size);
                skip = false;
                if (b > a) c.push(a, blk * 64 + j, floor_size);
            }
        }
        m = c.size - 1;                                               // the walk ends on the first candidate again
    }
    // st[0 .. m-1] turns clockwise on (x, y); emit it backwards from the smallest (x, then y)
    u64 best = ~0ull;
    for (int i = lane; i < m; i += 64) {
        const int2 p = c.st[i];
        const u64 key = ((u64)(unsigned)p.x << 42) | ((u64)(unsigned)p.y << 21) | (unsigned)i;   // x, y, i < 2^21 (checked by the caller)
        best = key < best ? key : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    const int start = (int)(best & 0x1FFFFF);
    int* out = vertices + (size_t)slot * cap * 2;
    for (int j = lane; j < m; j += 64) {
        int src = start - j;
        if (src < 0) src += m;
        const int2 p = c.st[src];
        out[2 * j] = p.x;
        out[2 * j + 1] = p.y;
    }
    if (lane == 0) n_vertices[slot] = m;
}

// ------------------------------------------------------------------------------------------------ host side
constexpr size_t kAlign = 256;
size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Scratch {
    size_t labels, area, partial, rowmin, rowmax, stack, total;
    int n_chunks;
};

Scratch scratch_layout(int h, int w, int planes, int top) {
    Scratch s;
    const size_t hw = (size_t)h * w;
    s.n_chunks = (int)((hw + kChunk - 1) / kChunk);
    size_t o = 0;
    s.labels = o;  o += align_up(hw * planes * sizeof(int));
    s.area = o;    o += align_up(hw * planes * sizeof(int));
    s.partial = o; o += align_up((size_t)planes * s.n_chunks * kMaxTop * sizeof(u64));
    s.rowmin = o;  o += align_up((size_t)planes * top * h * sizeof(int));
    s.rowmax = o;  o += align_up((size_t)planes * top * h * sizeof(int));
    s.stack = o;   o += align_up((size_t)planes * top * (2 * (size_t)h + 1) * sizeof(int2));
    s.total = o;
    return s;
}

int check_geometry(const void* maps, int n, int h, int w, const int32_t* classes, int n_classes, ClassList* cl) {
    AVL_REQUIRE(maps, "maps is NULL");
    AVL_REQUIRE(classes, "classes is NULL");
    AVL_REQUIRE(h >= 1 && w >= 1, "h = %d, w = %d (both must be >= 1)", h, w);
    AVL_REQUIRE(h < (1 << 20) && w < (1 << 21) && (long long)h * w < (1ll << 31) - 1, "a %d x %d map is too large", h, w);
    AVL_REQUIRE(n >= 1, "n = %d", n);
    AVL_REQUIRE(n_classes >= 1 && n_classes <= kMaxClasses, "n_classes = %d (1 .. %d)", n_classes, kMaxClasses);
    AVL_REQUIRE((long long)n * n_classes <= 65535, "%d x %d planes (at most 65535)", n, n_classes);
    for (int k = 0; k < n_classes; ++k) {
        AVL_REQUIRE(classes[k] >= 1 && classes[k] <= 255, "class %d: the index must be 1 .. 255 (0 is the background)", classes[k]);
        cl->c[k] = (unsigned char)classes[k];
    }
    return AVL_OK;
}

int launch_labelling(const uint8_t* maps, int planes, int h, int w, const ClassList& cl, int n_classes, int erode, int* labels, hipStream_t s) {
    const int hw = h * w;
    hipLaunchKernelGGL(k_ccl_tile, dim3((w + kTW - 1) / kTW, (h + kTH - 1) / kTH, planes), dim3(kBlock), 0, s, maps, h, w, cl, n_classes,
                       erode, labels);
    AVL_LAUNCH_CHECK();
    const long long items = (long long)((h - 1) / kTH) * w + (long long)((w - 1) / kTW) * h;
    if (items > 0) {
        hipLaunchKernelGGL(k_ccl_merge, dim3((unsigned)((items + kBlock - 1) / kBlock), 1, planes), dim3(kBlock), 0, s, h, w, labels);
        AVL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ccl_flatten, dim3((hw + kBlock - 1) / kBlock, 1, planes), dim3(kBlock), 0, s, hw, labels);
        AVL_LAUNCH_CHECK();
    }
    return AVL_OK;
}

}  // namespace

extern "C" int64_t avl_hull_scratch_bytes(int h, int w, int planes, int top_number) {
    if (h < 1 || w < 1 || planes < 1 || top_number < 1 || top_number > kMaxTop || (long long)h * w >= (1ll << 31) - 1) return 0;
    return (int64_t)scratch_layout(h, w, planes, top_number).total;
}

extern "C" int avl_label_components(const uint8_t* maps, int n, int h, int w, const int32_t* classes, int n_classes, int erode,
                                    int32_t* labels_out, void* scratch, void* stream) {
    (void)scratch;
    ClassList cl = {};
    if (int rc = check_geometry(maps, n, h, w, classes, n_classes, &cl)) return rc;
    AVL_REQUIRE(labels_out, "labels_out is NULL");
    return launch_labelling(maps, n * n_classes, h, w, cl, n_classes, erode != 0, labels_out, avl::as_stream(stream));
}

extern "C" int avl_class_hulls(const uint8_t* maps, int n, int h, int w, const int32_t* classes, int n_classes, int erode, int top_number,
                               int area_threshold, int drop_first, int32_t* vertices, int32_t* n_vertices, int32_t* areas, int32_t* roots,
                               void* scratch, void* stream) {
    ClassList cl = {};
    if (int rc = check_geometry(maps, n, h, w, classes, n_classes, &cl)) return rc;
    AVL_REQUIRE(top_number >= 1 && top_number <= kMaxTop, "top_number = %d (1 .. %d)", top_number, kMaxTop);
    AVL_REQUIRE(vertices && n_vertices && areas && roots, "an output buffer is NULL");
    AVL_REQUIRE(scratch, "scratch is NULL");
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "scratch must be 8-byte aligned");
    const int planes = n * n_classes, hw = h * w;
    const Scratch lay = scratch_layout(h, w, planes, top_number);
    char* base = static_cast<char*>(scratch);
    int* labels = reinterpret_cast<int*>(base + lay.labels);
    int* area = reinterpret_cast<int*>(base + lay.area);
    u64* partial = reinterpret_cast<u64*>(base + lay.partial);
    int* rowmin = reinterpret_cast<int*>(base + lay.rowmin);
    int* rowmax = reinterpret_cast<int*>(base + lay.rowmax);
    int2* stack = reinterpret_cast<int2*>(base + lay.stack);
    hipStream_t s = avl::as_stream(stream);
    if (int rc = launch_labelling(maps, planes, h, w, cl, n_classes, erode != 0, labels, s)) return rc;
    AVL_HIP_CHECK(hipMemsetAsync(area, 0, (size_t)hw * planes * sizeof(int), s));
    const dim3 pixels((hw + kBlock - 1) / kBlock, 1, planes);
    hipLaunchKernelGGL(k_hull_area, pixels, dim3(kBlock), 0, s, hw, labels, area);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hull_topk, dim3(lay.n_chunks, 1, planes), dim3(kBlock), 0, s, hw, area, top_number, partial);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hull_select, dim3(planes), dim3(kBlock), 0, s, h, lay.n_chunks, top_number, area_threshold, partial, roots, areas,
                       rowmin, rowmax);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hull_rows, pixels, dim3(kBlock), 0, s, h, w, labels, top_number, drop_first != 0, roots, rowmin, rowmax);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hull_chain, dim3(top_number, planes), dim3(64), 0, s, h, top_number, roots, rowmin, rowmax, stack, vertices, n_vertices);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}
