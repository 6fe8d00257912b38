// Ground plane from the LiDAR cloud: RANSAC around the reference's plane model (src/plane_3d.py).  The reference ships the model
// half only -- Plane3D.fit(data, "min") (:45-63), normalize (:98-107), eval (:65-80) and distance_to_plane (:82-88); the plane
// itself arrives from another package (vision_semantic_segmentation_node.py:51, :199-201).  Here the cloud that is already on the
// device fixes it: n_hyp point triples are fitted, every hypothesis is scored against every point, the winner is selected and the
// moments of its inliers are summed, all on the caller's stream with no host synchronisation.
//
//   k_plane_prepare   one thread per point: widen, Xv = T [x, y, z, 1] (the fma chain of mapping.hip's dot4), "used" = all three
//                     coordinates finite and inside the roi; recip = 1 / (|x - x0|^norm + 1) (:67-73) for the x-norm weight.  The
//                     point goes to scratch as four doubles (x, y, z, recip), recip = -1 marks an unused point.  max recip (:74) is an
//                     integer atomicMax on the bit pattern (non-negative doubles order like their bits; max is order-free: exact).
//   k_plane_fit       one thread per hypothesis: :47-51 term by term, then :99-106 with IEEE divide and sqrt, and the norm
//                     distance_to_plane takes of the NORMALISED parameters again (:83).
//   k_plane_score     the hot kernel.  A lane keeps kPts points in registers (x, y, z, weight = recip / max recip, :74); a workgroup
//                     walks kHypChunk hypotheses, which every lane reads at the same address; per hypothesis: cost < tolerance
//                     (:75 / :77), __ballot, popcount, one LDS add per wave, and at the end one integer atomicAdd per hypothesis
//                     and workgroup into global memory.
//   k_plane_select    one workgroup: arg-max of the counts, the lowest index among equals, -1 when every count is 0.
//   k_plane_moments   n, sum(delta), sum(delta delta^T) over the winner's inliers, delta = p - p0, p0 = the first point of the
//                     winning triple; per-workgroup partials in a slab (LDS tree in a fixed order),
//   k_plane_moments_final sums the slab in a fixed order.  No float atomics anywhere: two runs give the same bits.
//
// Compiled with -ffp-contract=off (as mapping.hip): every product and sum below rounds once, as NumPy's scalar float64 does.
// Departure from the reference: a point with a NaN / infinite coordinate is left out (step "used"); in the reference one NaN makes
// np.max (:74) NaN and with it every weight.
#include "avl_common.h"

#include <cstdint>

namespace {

constexpr int kBlock = 256;
constexpr int kPts = 4;                                  // points a lane of k_plane_score holds
constexpr int kPtsPerWg = kBlock * kPts;
constexpr int kHypChunk = 64;                            // hypotheses one k_plane_score workgroup walks (blockIdx.y picks the chunk)
constexpr int kMomPerWg = kBlock * 4;                    // points one k_plane_moments workgroup sums
constexpr int kMaxPoints = 1 << 27;                      // keeps every 32-bit point index and grid size far from overflow
constexpr int kMom = 10;                                 // n, 3 x sum(delta), 6 x sum(delta delta^T)

typedef unsigned long long u64;

struct PlanePts {
    const char* base;
    int n, dtype;
    long long point_stride, comp_stride;
    double T[16];
    double roi[6];
    int has_T, has_roi;
    int weight_method, norm;
    double x0;
};

// scratch header: the three cells the kernels accumulate into (cleared by the host call)
struct Header {
    u64 max_recip_bits;
    int used, valid;
};

__device__ __forceinline__ double dot4(const double* r, double a, double b, double c) {   // mapping.hip's dot4 with the constant 1
    double s = r[0] * a;
    s = __builtin_fma(r[1], b, s);
    s = __builtin_fma(r[2], c, s);
    s = __builtin_fma(r[3], 1.0, s);
    return s;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

__global__ void __launch_bounds__(kBlock) k_plane_prepare(PlanePts pv, double4* __restrict__ pts4, Header* __restrict__ hdr) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    bool used = false;
    double recip = 0.0;
    if (k < pv.n) {
        const char* p = pv.base + (long long)k * pv.point_stride;
        double x, y, z;
        if (pv.dtype == AVL_F64) {
            x = *reinterpret_cast<const double*>(p);
            y = *reinterpret_cast<const double*>(p + pv.comp_stride);
            z = *reinterpret_cast<const double*>(p + 2 * pv.comp_stride);
        } else {
            x = (double)*reinterpret_cast<const float*>(p);
            y = (double)*reinterpret_cast<const float*>(p + pv.comp_stride);
            z = (double)*reinterpret_cast<const float*>(p + 2 * pv.comp_stride);
        }
        if (pv.has_T) {
            const double v0 = dot4(pv.T + 0, x, y, z), v1 = dot4(pv.T + 4, x, y, z), v2 = dot4(pv.T + 8, x, y, z);
            x = v0; y = v1; z = v2;
        }
        used = finite3(x, y, z);
        if (used && pv.has_roi)
            used = x >= pv.roi[0] && x <= pv.roi[1] && y >= pv.roi[2] && y <= pv.roi[3] && z >= pv.roi[4] && z <= pv.roi[5];
        if (used) {
            recip = 1.0;
            if (pv.weight_method == AVL_PLANE_W_XNORM) {
                const double dx = x - pv.x0;
                const double x_norm = pv.norm == 1 ? __builtin_fabs(dx) : dx * dx;          // :68 / :70
                recip = 1.0 / (x_norm + 1.0);                                               // :73
            }
        }
        pts4[k] = make_double4(x, y, z, used ? recip : -1.0);
    }
    // one pair of integer atomics per wave
    double m = used ? recip : 0.0;
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    const u64 mask = __ballot(used);
    if ((threadIdx.x & 63) == 0 && mask) {
        atomicMax(&hdr->max_recip_bits, (u64)__double_as_longlong(m));
        atomicAdd(&hdr->used, (int)__popcll(mask));
    }
}

__global__ void __launch_bounds__(kBlock) k_plane_fit(const double4* __restrict__ pts4, int n, const int* __restrict__ triples, int n_hyp,
                                                      double min_c, double4* __restrict__ planes, double* __restrict__ norms,
                                                      Header* __restrict__ hdr) {
    const int h = blockIdx.x * kBlock + threadIdx.x;
    bool valid = false;
    double a = 0.0, b = 0.0, c = 0.0, d = 0.0, norm = 0.0;
    if (h < n_hyp) {
        const int i0 = triples[3 * h], i1 = triples[3 * h + 1], i2 = triples[3 * h + 2];
        if (i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n) {
            const double4 p0 = pts4[i0], p1 = pts4[i1], p2 = pts4[i2];
            const bool same = (p0.x - p1.x == 0.0) && (p0.y - p1.y == 0.0) && (p0.z - p1.z == 0.0);   // :47
            if (p0.w >= 0.0 && p1.w >= 0.0 && p2.w >= 0.0 && !same) {
                a = (p0.y - p1.y) * (p2.z - p1.z) - (p2.y - p1.y) * (p0.z - p1.z);          // :48
                b = (p0.z - p1.z) * (p2.x - p1.x) - (p2.z - p1.z) * (p0.x - p1.x);          // :49
                c = (p0.x - p1.x) * (p2.y - p1.y) - (p2.x - p1.x) * (p0.y - p1.y);          // :50
                d = -a * p1.x - b * p1.y - c * p1.z;                                        // :51
                double s = __builtin_sqrt(a * a + b * b + c * c);                           // :99
                if (s != 0.0 && __builtin_isfinite(s)) {
                    if (c < 0.0) s = -1.0 * s;                                              // :104-105
                    a = a / s; b = b / s; c = c / s; d = d / s;                             // :106
                    norm = __builtin_sqrt(a * a + b * b + c * c);                           // :83
                    valid = c >= min_c && norm > 1e-3;                                      // :84 holds for every unit normal
                }
            }
        }
        if (!valid) { a = b = c = d = 0.0; norm = 0.0; }
        planes[h] = make_double4(a, b, c, d);
        norms[h] = norm;
    }
    const u64 mask = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&hdr->valid, (int)__popcll(mask));
}

// :85 with the matmul as the fma chain mapping.hip uses for NumPy's products, then :75
__device__ __forceinline__ double plane_cost(double a, double b, double c, double d, double norm, double x, double y, double z, double w) {
    double s = x * a;
    s = __builtin_fma(y, b, s);
    s = __builtin_fma(z, c, s);
    return __builtin_fabs(s + d) / norm * w;
}

__global__ void __launch_bounds__(kBlock) k_plane_score(const double4* __restrict__ pts4, int n, const double4* __restrict__ planes,
                                                        const double* __restrict__ norms, int n_hyp, const Header* __restrict__ hdr,
                                                        int weight_method, double tolerance, int* __restrict__ counts) {
    __shared__ int s_count[kHypChunk];
    if (threadIdx.x < kHypChunk) s_count[threadIdx.x] = 0;
    const double max_recip = __longlong_as_double((long long)hdr->max_recip_bits);
    double x[kPts], y[kPts], z[kPts], w[kPts];
#pragma unroll
    for (int j = 0; j < kPts; ++j) {
        const int k = blockIdx.x * kPtsPerWg + j * kBlock + threadIdx.x;
        double4 p = make_double4(0.0, 0.0, 0.0, -1.0);
        if (k < n) p = pts4[k];
        const bool used = p.w >= 0.0;
        x[j] = used ? p.x : 0.0; y[j] = used ? p.y : 0.0; z[j] = used ? p.z : 0.0;
        // NaN keeps an unused point out of every comparison below
        w[j] = !used ? __builtin_nan("") : (weight_method == AVL_PLANE_W_XNORM ? p.w / max_recip : 1.0);       // :74
    }
    __syncthreads();
    const int h0 = blockIdx.y * kHypChunk;
    const int h1 = min(n_hyp, h0 + kHypChunk);
    for (int h = h0; h < h1; ++h) {
        const double norm = norms[h];
        if (norm == 0.0) continue;                                                          // invalid: its count stays 0
        const double4 pl = planes[h];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kPts; ++j)
            cnt += (int)__popcll(__ballot(plane_cost(pl.x, pl.y, pl.z, pl.w, norm, x[j], y[j], z[j], w[j]) < tolerance));
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_count[h - h0], cnt);
    }
    __syncthreads();
    if (threadIdx.x < h1 - h0) {
        const int cnt = s_count[threadIdx.x];
        if (cnt) atomicAdd(counts + h0 + threadIdx.x, cnt);
    }
}

__global__ void __launch_bounds__(kBlock) k_plane_select(const int* __restrict__ counts, int n_hyp, const double4* __restrict__ planes,
                                                         const int* __restrict__ triples, const double4* __restrict__ pts4,
                                                         const Header* __restrict__ hdr, double* __restrict__ result) {
    __shared__ u64 red[kBlock / 64];
    // larger count first, then the smaller index; 0 = no hypothesis with a point
    u64 best = 0;
    for (int h = threadIdx.x; h < n_hyp; h += kBlock) {
        const int cnt = counts[h];
        const u64 key = cnt > 0 ? ((u64)(unsigned)cnt << 32) | (0xFFFFFFFFu - (unsigned)h) : 0;
        best = key > best ? key : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 0; k < kBlock / 64; ++k) best = red[k] > best ? red[k] : best;
    long long* words = reinterpret_cast<long long*>(result);
    const int h = best ? (int)(0xFFFFFFFFu - (unsigned)best) : -1;
    words[0] = h;
    words[1] = (long long)(best >> 32);
    words[2] = hdr->used;
    words[3] = hdr->valid;
    double4 pl = make_double4(0.0, 0.0, 0.0, 0.0), p0 = pl;
    if (h >= 0) { pl = planes[h]; p0 = pts4[triples[3 * h]]; }                              // a counted hypothesis is valid: its indices are in range
    result[4] = pl.x; result[5] = pl.y; result[6] = pl.z; result[7] = pl.w;
    result[8] = p0.x; result[9] = p0.y; result[10] = p0.z;
    for (int k = 11; k < AVL_PLANE_RESULT_WORDS; ++k) result[k] = 0.0;
}

// the values of all kBlock threads summed in one fixed tree; the total is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
    __syncthreads();                                                   // red[] of the previous sum has been read
    red[threadIdx.x] = v;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(kBlock) k_plane_moments(const double4* __restrict__ pts4, int n, const double* __restrict__ norms,
                                                          const Header* __restrict__ hdr, int weight_method, double tolerance,
                                                          const double* __restrict__ result, double* __restrict__ slab) {
    __shared__ double red[kBlock];
    const long long best = reinterpret_cast<const long long*>(result)[0];
    double acc[kMom];
#pragma unroll
    for (int q = 0; q < kMom; ++q) acc[q] = 0.0;
    if (best >= 0) {                                                   // uniform over the grid
        const double a = result[4], b = result[5], c = result[6], d = result[7], norm = norms[best];
        const double px = result[8], py = result[9], pz = result[10];
        const double max_recip = __longlong_as_double((long long)hdr->max_recip_bits);
#pragma unroll
        for (int j = 0; j < kMomPerWg / kBlock; ++j) {
            const int k = blockIdx.x * kMomPerWg + j * kBlock + threadIdx.x;
            if (k >= n) continue;
            const double4 p = pts4[k];
            if (!(p.w >= 0.0)) continue;
            const double w = weight_method == AVL_PLANE_W_XNORM ? p.w / max_recip : 1.0;
            if (!(plane_cost(a, b, c, d, norm, p.x, p.y, p.z, w) < tolerance)) continue;   // the comparison k_plane_score counted
            const double dx = p.x - px, dy = p.y - py, dz = p.z - pz;
            acc[0] += 1.0;
            acc[1] += dx; acc[2] += dy; acc[3] += dz;
            acc[4] += dx * dx; acc[5] += dx * dy; acc[6] += dx * dz;
            acc[7] += dy * dy; acc[8] += dy * dz; acc[9] += dz * dz;
        }
    }
#pragma unroll
    for (int q = 0; q < kMom; ++q) {
        const double total = block_sum(acc[q], red);
        if (threadIdx.x == 0) slab[(size_t)blockIdx.x * kMom + q] = total;
    }
}

__global__ void __launch_bounds__(kBlock) k_plane_moments_final(const double* __restrict__ slab, int n_wg, double* __restrict__ result) {
    __shared__ double red[kBlock];
#pragma unroll 1
    for (int q = 0; q < kMom; ++q) {
        double v = 0.0;
        for (int i = threadIdx.x; i < n_wg; i += kBlock) v += slab[(size_t)i * kMom + q];
        const double total = block_sum(v, red);
        if (threadIdx.x == 0) result[11 + q] = total;
    }
}

// ------------------------------------------------------------------------------------------------ host side
constexpr size_t kAlign = 256;
size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Scratch {
    size_t header, pts4, planes, norms, counts, slab, total;
    int n_mom_wg;
};

Scratch scratch_layout(int n, int n_hyp) {
    Scratch s;
    s.n_mom_wg = (n + kMomPerWg - 1) / kMomPerWg;
    size_t o = 0;
    s.header = o; o += align_up(sizeof(Header));
    s.pts4 = o;   o += align_up((size_t)n * sizeof(double4));
    s.planes = o; o += align_up((size_t)n_hyp * sizeof(double4));
    s.norms = o;  o += align_up((size_t)n_hyp * sizeof(double));
    s.counts = o; o += align_up((size_t)n_hyp * sizeof(int));
    s.slab = o;   o += align_up((size_t)s.n_mom_wg * kMom * sizeof(double));
    s.total = o;
    return s;
}

}  // namespace

extern "C" int64_t avl_plane_scratch_bytes(int n, int n_hyp) {
    if (n < 3 || n > kMaxPoints || n_hyp < 1 || n_hyp > AVL_PLANE_MAX_HYP) return 0;
    return (int64_t)scratch_layout(n, n_hyp).total;
}

extern "C" int avl_plane_ransac(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, const double* T_host,
                                const double* roi_host, const int32_t* triples, int n_hyp, int weight_method, double x0, int norm,
                                double tolerance, double min_c, double* planes_out, int32_t* counts_out, void* result, void* scratch,
                                void* stream) {
    AVL_REQUIRE(pts, "pts is NULL");
    AVL_REQUIRE(n >= 3, "n = %d (a plane needs three points)", n);
    AVL_REQUIRE(n <= kMaxPoints, "n = %d (at most %d points)", n, kMaxPoints);
    AVL_REQUIRE(dtype == AVL_F32 || dtype == AVL_F64, "point dtype %d", dtype);
    const int64_t es = dtype == AVL_F64 ? 8 : 4;
    AVL_REQUIRE(point_stride > 0 && comp_stride > 0 && point_stride % es == 0 && comp_stride % es == 0,
                "point strides %lld/%lld not multiples of %lld", (long long)point_stride, (long long)comp_stride, (long long)es);
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(pts) % es == 0, "pts is not aligned to its element size");
    AVL_REQUIRE(triples, "triples is NULL");
    AVL_REQUIRE(n_hyp >= 1 && n_hyp <= AVL_PLANE_MAX_HYP, "n_hyp = %d (1 .. %d)", n_hyp, AVL_PLANE_MAX_HYP);
    AVL_REQUIRE(weight_method == AVL_PLANE_W_NONE || weight_method == AVL_PLANE_W_XNORM, "weight_method %d", weight_method);
    AVL_REQUIRE(norm == 1 || norm == 2, "norm = %d (1 or 2)", norm);
    AVL_REQUIRE(tolerance > 0.0, "tolerance = %g (must be positive)", tolerance);
    AVL_REQUIRE(result, "result is NULL");
    AVL_REQUIRE(scratch, "scratch is NULL");
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 32 == 0 && reinterpret_cast<uintptr_t>(result) % 8 == 0,
                "scratch must be 32-byte and result 8-byte aligned");
    AVL_REQUIRE(!planes_out || reinterpret_cast<uintptr_t>(planes_out) % 32 == 0, "planes_out must be 32-byte aligned");
    AVL_REQUIRE(!counts_out || reinterpret_cast<uintptr_t>(counts_out) % 4 == 0, "counts_out must be 4-byte aligned");

    PlanePts pv = {};
    pv.base = static_cast<const char*>(pts);
    pv.n = n; pv.dtype = dtype; pv.point_stride = point_stride; pv.comp_stride = comp_stride;
    pv.has_T = T_host != nullptr;
    if (T_host) memcpy(pv.T, T_host, sizeof(pv.T));
    pv.has_roi = roi_host != nullptr;
    if (roi_host) memcpy(pv.roi, roi_host, sizeof(pv.roi));
    pv.weight_method = weight_method; pv.norm = norm; pv.x0 = x0;

    const Scratch lay = scratch_layout(n, n_hyp);
    char* base = static_cast<char*>(scratch);
    Header* hdr = reinterpret_cast<Header*>(base + lay.header);
    double4* pts4 = reinterpret_cast<double4*>(base + lay.pts4);
    double4* planes = planes_out ? reinterpret_cast<double4*>(planes_out) : reinterpret_cast<double4*>(base + lay.planes);
    double* norms = reinterpret_cast<double*>(base + lay.norms);
    int* counts = counts_out ? counts_out : reinterpret_cast<int*>(base + lay.counts);
    double* slab = reinterpret_cast<double*>(base + lay.slab);
    double* res = static_cast<double*>(result);
    hipStream_t s = avl::as_stream(stream);

    AVL_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(Header), s));
    AVL_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_hyp * sizeof(int), s));
    hipLaunchKernelGGL(k_plane_prepare, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pv, pts4, hdr);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_plane_fit, dim3((n_hyp + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pts4, n, triples, n_hyp, min_c, planes, norms, hdr);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_plane_score, dim3((n + kPtsPerWg - 1) / kPtsPerWg, (n_hyp + kHypChunk - 1) / kHypChunk), dim3(kBlock), 0, s, pts4, n,
                       planes, norms, n_hyp, hdr, weight_method, tolerance, counts);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_plane_select, dim3(1), dim3(kBlock), 0, s, counts, n_hyp, planes, triples, pts4, hdr, res);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_plane_moments, dim3(lay.n_mom_wg), dim3(kBlock), 0, s, pts4, n, norms, hdr, weight_method, tolerance, res, slab);
    AVL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_plane_moments_final, dim3(1), dim3(kBlock), 0, s, slab, lay.n_mom_wg, res);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}
