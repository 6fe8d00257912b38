// Full-resolution head of the segmentation network (gfx950): what the reference does with the logits after
// DeepLabV3Plus.forward(x, upsample_pred=True) (deeplab_v3_plus.py:51,67-69), read straight from the plan's fp32 logits
// buffer (NHWC [h*w][K], row stride ld; every plan writes it, the fused k_dwpw_xs<CLS> classifier included).
//   k_upsample_logits: F.interpolate(mode='bilinear', align_corners=True) to fp32 NCHW planes [K][H][W] (the tensor model(x) returns
//                      for a batch of one).
//   k_full_res_eval:   the same interpolation per output pixel, never written out, followed by torch.argmax (uint8 labels), MeanIOU's
//                      confusion matrix (models/metrics.py:29-59) and CrossEntropyLoss(ignore_index) terms (models/loss.py,
//                      models/build.py:20); k_eval_finalize sums the per-workgroup loss partials in a fixed order in fp64.
// One workgroup = a 16 x 64 tile of output pixels; lane (x = tid & 63, row group tid >> 6) owns the four pixels of its column in rows
// r, r + 4, r + 8, r + 12, so every store of a wave is 64 consecutive x.  The low-res window the tile reads (about 6 x 18 source pixels x K
// at 266 x 476 -> 1080 x 1920) is staged in LDS when it fits (32 KB), otherwise (strong down-sampling) the corners are read from global.
#include <algorithm>

#include "seg_types.h"

namespace avl {
namespace {

constexpr int kThreads = 256;
constexpr int kTileH = 16, kTileW = 64;
constexpr int kWinFloats = 8192;           // at most 32 KB of LDS for the staged window
constexpr int kMaxEvalClasses = 64;        // LDS histogram of K x K uint32 bins; labels are uint8

// The source coordinate of k_bilinear (seg_conv.hip): src = dst * (in-1)/(out-1), the scale is 0 when out = 1.
struct Geo {
    const float* logits;
    int h, w, K;
    long long ld;
    int H, W;
    float sy, sx;
    int win_cap;                       // floats of LDS for the staged window (window_capacity(); 0 = read the corners from global)
};

// The product is rounded before the corner and weight are taken from it: torch rounds it too, and the tile's window below must see the
// very same value as every pixel inside it.  The empty asm makes it opaque, so hipcc cannot contract sy * oy - y0 into one FMA (the
// weight would then move by up to an ulp of the source coordinate: 2e-5 relative at 266 -> 1080).
__device__ __forceinline__ float src_coord(float scale, int dst) {
    float p = scale * (float)dst;
    asm("" : "+v"(p));
    return p;
}

struct Corner {
    int y0, y1, x0, x1;
    float ly, lx, hy, hx;
};

__device__ __forceinline__ Corner corner(const Geo& g, int oy, int ox) {
    Corner c;
    const float fy = src_coord(g.sy, oy), fx = src_coord(g.sx, ox);
    c.y0 = min((int)fy, g.h - 1);
    c.x0 = min((int)fx, g.w - 1);
    c.y1 = c.y0 + (c.y0 < g.h - 1 ? 1 : 0);
    c.x1 = c.x0 + (c.x0 < g.w - 1 ? 1 : 0);
    c.ly = fy - c.y0;
    c.lx = fx - c.x0;
    c.hy = 1.f - c.ly;
    c.hx = 1.f - c.lx;
    return c;
}

// The window of source pixels a tile reads, and (when it fits) its copy in LDS: [rows][cols][Kp], Kp odd (no bank conflicts between
// neighbouring source pixels at even K).
struct Window {
    int y0, x0, cols, Kp;
    bool staged;
};

__device__ __forceinline__ Window stage_window(const Geo& g, int oy0, int ox0, float* lds) {
    Window win;
    const int oy1 = min(oy0 + kTileH, g.H) - 1, ox1 = min(ox0 + kTileW, g.W) - 1;
    win.y0 = min((int)src_coord(g.sy, oy0), g.h - 1);
    win.x0 = min((int)src_coord(g.sx, ox0), g.w - 1);
    const int y1 = min((int)src_coord(g.sy, oy1) + 1, g.h - 1), x1 = min((int)src_coord(g.sx, ox1) + 1, g.w - 1);
    const int rows = y1 - win.y0 + 1;
    win.cols = x1 - win.x0 + 1;
    win.Kp = g.K | 1;
    win.staged = (long long)rows * win.cols * win.Kp <= g.win_cap;
    if (win.staged) {
        const int n = rows * win.cols * g.K;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int p = i / g.K, c = i - p * g.K;
            const int yy = win.y0 + p / win.cols, xx = win.x0 + p % win.cols;
            lds[p * win.Kp + c] = g.logits[((long long)yy * g.w + xx) * g.ld + c];
        }
    }
    __syncthreads();
    return win;
}

// The four corner offsets of an output pixel in the staged window (STAGED) or in the global buffer; class k is at offset + k either way.
template <bool STAGED>
__device__ __forceinline__ void corner_offsets(const Geo& g, const Window& win, const Corner& c, long long (&o)[4]) {
    if (STAGED) {
        const int r0 = c.y0 - win.y0, r1 = c.y1 - win.y0, q0 = c.x0 - win.x0, q1 = c.x1 - win.x0;
        o[0] = (long long)(r0 * win.cols + q0) * win.Kp;
        o[1] = (long long)(r0 * win.cols + q1) * win.Kp;
        o[2] = (long long)(r1 * win.cols + q0) * win.Kp;
        o[3] = (long long)(r1 * win.cols + q1) * win.Kp;
    } else {
        o[0] = ((long long)c.y0 * g.w + c.x0) * g.ld;
        o[1] = ((long long)c.y0 * g.w + c.x1) * g.ld;
        o[2] = ((long long)c.y1 * g.w + c.x0) * g.ld;
        o[3] = ((long long)c.y1 * g.w + c.x1) * g.ld;
    }
}

// the interpolated value of class k, weights and order as k_bilinear
__device__ __forceinline__ float lerp4(const float* src, const long long (&o)[4], const Corner& c, int k) {
    return c.hy * (c.hx * src[o[0] + k] + c.lx * src[o[1] + k]) + c.ly * (c.hx * src[o[2] + k] + c.lx * src[o[3] + k]);
}

template <bool STAGED>
__device__ __forceinline__ void upsample_pixel(const Geo& g, const Window& win, const float* src, int oy, int ox, float* __restrict__ out) {
    const Corner c = corner(g, oy, ox);
    long long o[4];
    corner_offsets<STAGED>(g, win, c, o);
    const long long plane = (long long)g.H * g.W;
    float* dst = out + (long long)oy * g.W + ox;
    for (int k = 0; k < g.K; ++k) dst[k * plane] = lerp4(src, o, c, k);
}

__global__ void __launch_bounds__(kThreads) k_upsample_logits(Geo g, float* __restrict__ out) {
    extern __shared__ float lds[];                              // [g.win_cap]
    const int oy0 = blockIdx.y * kTileH, ox0 = blockIdx.x * kTileW;
    const Window win = stage_window(g, oy0, ox0, lds);
    const int ox = ox0 + (threadIdx.x & (kTileW - 1));
    if (ox >= g.W) return;
#pragma unroll 1
    for (int r = threadIdx.x / kTileW; r < kTileH; r += kThreads / kTileW) {
        const int oy = oy0 + r;
        if (oy >= g.H) break;
        if (win.staged) upsample_pixel<true>(g, win, lds, oy, ox, out);
        else upsample_pixel<false>(g, win, g.logits, oy, ox, out);
    }
}

struct EvalOut {
    const unsigned char* gt;           // uint8 [H][W] or NULL
    int ignore_index;
    unsigned char* labels;             // uint8 [H][W] or NULL
    unsigned long long* confusion;     // [K][K] (ground truth, prediction), accumulated; NULL = none
    double* slab_sum;                  // [blocks] loss partials, NULL = no loss
    unsigned* slab_cnt;                // [blocks] pixels that contributed to the loss
    unsigned* slab_inv;                // [blocks] ground-truth values neither in [0, K) nor ignore_index
};

// One output pixel: K interpolated logits -> arg-max (first maximal index wins, a NaN counts as maximal: AVL_OP_ARGMAX) and, with LOSS and a
// ground truth that counts (gt < K, gt != ignore), logsumexp(z) - z[gt] in fp32: a second pass over the classes sums exp(z - max) with the
// maximum the first pass found (a NaN logit makes the term NaN, as in torch).
template <bool STAGED, bool LOSS>
__device__ __forceinline__ int eval_pixel(const Geo& g, const Window& win, const float* src, int oy, int ox, int gt, bool counts, float& term) {
    const Corner c = corner(g, oy, ox);
    long long o[4];
    corner_offsets<STAGED>(g, win, c, o);
    float best = lerp4(src, o, c, 0);
    int bi = 0;
    for (int k = 1; k < g.K; ++k) {
        const float v = lerp4(src, o, c, k);
        if (v > best || (v != v && best == best)) { best = v; bi = k; }
    }
    if (LOSS && counts) {
        float s = 0.f;
        for (int k = 0; k < g.K; ++k) s += __expf(lerp4(src, o, c, k) - best);
        term = best + __logf(s) - lerp4(src, o, c, gt);
    }
    return bi;
}

struct LossPart {
    double sum;
    unsigned cnt, inv;
};

template <bool LOSS>
__device__ __forceinline__ LossPart eval_tile(const Geo& g, const EvalOut& e, const Window& win, const float* lds, unsigned* hist, int oy0, int ox) {
    LossPart lp = {0.0, 0u, 0u};
#pragma unroll 1
    for (int r = threadIdx.x / kTileW; r < kTileH; r += kThreads / kTileW) {
        const int oy = oy0 + r;
        if (oy >= g.H) break;
        const long long pix = (long long)oy * g.W + ox;
        const int gt = e.gt ? (int)e.gt[pix] : -1;
        const bool counts = gt >= 0 && gt < g.K && gt != e.ignore_index;
        float term = 0.f;
        const int pred = win.staged ? eval_pixel<true, LOSS>(g, win, lds, oy, ox, gt, counts, term)
                                    : eval_pixel<false, LOSS>(g, win, g.logits, oy, ox, gt, counts, term);
        if (e.labels) e.labels[pix] = (unsigned char)pred;
        if (e.confusion && gt >= 0 && gt < g.K) atomicAdd(&hist[gt * g.K + pred], 1u);
        if (LOSS) {
            if (counts) { lp.sum += (double)term; ++lp.cnt; }
            else if (gt >= g.K && gt != e.ignore_index) ++lp.inv;
        }
    }
    return lp;
}

__global__ void __launch_bounds__(kThreads) k_full_res_eval(Geo g, EvalOut e) {
    extern __shared__ unsigned smem[];                          // [K * K histogram bins when e.confusion][g.win_cap window floats]
    unsigned* hist = smem;
    float* lds = reinterpret_cast<float*>(smem + (e.confusion ? g.K * g.K : 0));
    __shared__ double red_sum[kThreads / 64];
    __shared__ unsigned red_cnt[kThreads / 64], red_inv[kThreads / 64];
    const int KK = g.K * g.K;
    if (e.confusion)
        for (int i = threadIdx.x; i < KK; i += kThreads) hist[i] = 0u;
    const int oy0 = blockIdx.y * kTileH, ox0 = blockIdx.x * kTileW;
    const Window win = stage_window(g, oy0, ox0, lds);          // (its barrier also orders the histogram's zeroing)
    const int ox = ox0 + (threadIdx.x & (kTileW - 1));
    LossPart lp = {0.0, 0u, 0u};
    if (ox < g.W) lp = e.slab_sum ? eval_tile<true>(g, e, win, lds, hist, oy0, ox) : eval_tile<false>(g, e, win, lds, hist, oy0, ox);
    double lsum = lp.sum;
    unsigned cnt = lp.cnt, inv = lp.inv;
    if (e.confusion) {
        __syncthreads();
        for (int i = threadIdx.x; i < KK; i += kThreads) {
            const unsigned v = hist[i];
            if (v) atomicAdd(&e.confusion[i], (unsigned long long)v);
        }
    }
    if (e.slab_sum) {
        // fixed-order reduction: a shuffle tree inside each wave, then the four waves in order
        for (int d = 32; d > 0; d >>= 1) {
            lsum += __shfl_down(lsum, d);
            cnt += __shfl_down(cnt, d);
            inv += __shfl_down(inv, d);
        }
        const int wave = threadIdx.x / 64;
        if ((threadIdx.x & 63) == 0) { red_sum[wave] = lsum; red_cnt[wave] = cnt; red_inv[wave] = inv; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double sum = 0.0;
            unsigned c = 0u, n = 0u;
            for (int i = 0; i < kThreads / 64; ++i) { sum += red_sum[i]; c += red_cnt[i]; n += red_inv[i]; }
            const int b = blockIdx.y * gridDim.x + blockIdx.x;
            e.slab_sum[b] = sum;
            e.slab_cnt[b] = c;
            e.slab_inv[b] = n;
        }
    }
}

// loss_out[0] = sum of the terms, loss_out[1] = their mean (NaN when no pixel contributed, as torch's cross_entropy);
// counts_out[0] = contributing pixels, counts_out[1] = invalid ground-truth values.  One workgroup, fixed order: bitwise reproducible.
__global__ void __launch_bounds__(kThreads) k_eval_finalize(const double* __restrict__ slab_sum, const unsigned* __restrict__ slab_cnt,
                                                           const unsigned* __restrict__ slab_inv, int nb, double* __restrict__ loss_out,
                                                           unsigned long long* __restrict__ counts_out) {
    __shared__ double s_sum[kThreads];
    __shared__ unsigned long long s_cnt[kThreads], s_inv[kThreads];
    double sum = 0.0;
    unsigned long long cnt = 0, inv = 0;
    for (int i = threadIdx.x; i < nb; i += kThreads) { sum += slab_sum[i]; cnt += slab_cnt[i]; inv += slab_inv[i]; }
    s_sum[threadIdx.x] = sum;
    s_cnt[threadIdx.x] = cnt;
    s_inv[threadIdx.x] = inv;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + d];
            s_inv[threadIdx.x] += s_inv[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss_out[0] = s_sum[0];
        loss_out[1] = s_cnt[0] ? s_sum[0] / (double)s_cnt[0] : __builtin_nan("");
        counts_out[0] = s_cnt[0];
        counts_out[1] = s_inv[0];
    }
}

bool aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

int make_geo(const float* logits, int h, int w, int K, int64_t ld, int H, int W, Geo& g, const char* what) {
    AVL_REQUIRE(logits, "%s: logits is NULL", what);
    AVL_REQUIRE(aligned(logits, 4), "%s: logits is not 4-byte aligned", what);
    AVL_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0, "%s: sizes %d x %d -> %d x %d", what, h, w, H, W);
    AVL_REQUIRE((long long)H * W <= (1ll << 31) - 1 && (long long)h * w <= (1ll << 31) - 1, "%s: image too large", what);
    AVL_REQUIRE(K > 0, "%s: K = %d", what, K);
    AVL_REQUIRE(ld >= K, "%s: row stride %lld < K %d", what, (long long)ld, K);
    g.logits = logits;
    g.h = h; g.w = w; g.K = K; g.ld = ld; g.H = H; g.W = W;
    g.sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    g.sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    // A tile's window spans floor(s * (tile - 1)) + 3 source rows / columns, one more where the rounded products straddle an integer;
    // the LDS is sized to that, so that small windows keep many workgroups per CU.  stage_window() checks every tile's actual window
    // against it (a tile that does not fit reads from global).
    const long long rows = std::min<long long>(h, (long long)(g.sy * (kTileH - 1)) + 4);
    const long long cols = std::min<long long>(w, (long long)(g.sx * (kTileW - 1)) + 4);
    const long long floats = rows * cols * (K | 1);
    g.win_cap = floats <= kWinFloats ? (int)floats : 0;
    return AVL_OK;
}

dim3 tiles(int H, int W) { return dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH)); }

}  // namespace
}  // namespace avl

extern "C" int avl_upsample_logits(const float* logits, int h, int w, int K, int64_t ld, float* out, int H, int W, void* stream) {
    avl::Geo g;
    if (int rc = avl::make_geo(logits, h, w, K, ld, H, W, g, "avl_upsample_logits")) return rc;
    if (K > 256) return avl::set_error(AVL_E_UNSUPPORTED, "avl_upsample_logits: K = %d > 256 classes", K);
    AVL_REQUIRE(out, "avl_upsample_logits: out is NULL");
    AVL_REQUIRE(avl::aligned(out, 4), "avl_upsample_logits: out is not 4-byte aligned");
    hipLaunchKernelGGL(avl::k_upsample_logits, avl::tiles(H, W), dim3(avl::kThreads), g.win_cap * sizeof(float), avl::as_stream(stream), g, out);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

extern "C" int64_t avl_seg_eval_scratch_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return avl::set_error(AVL_E_ARG, "avl_seg_eval_scratch_bytes: size %d x %d", H, W);
    const dim3 t = avl::tiles(H, W);
    return (int64_t)t.x * t.y * (sizeof(double) + 2 * sizeof(unsigned));
}

extern "C" int avl_seg_eval_full_res(const float* logits, int h, int w, int K, int64_t ld, int H, int W, const uint8_t* gt,
                                     int ignore_index, uint8_t* labels_out, unsigned long long* confusion, double* loss_out,
                                     unsigned long long* counts_out, void* scratch, void* stream) {
    avl::Geo g;
    if (int rc = avl::make_geo(logits, h, w, K, ld, H, W, g, "avl_seg_eval_full_res")) return rc;
    if (K > avl::kMaxEvalClasses)
        return avl::set_error(AVL_E_UNSUPPORTED, "avl_seg_eval_full_res: K = %d > %d classes (LDS confusion histogram, uint8 labels)", K,
                              avl::kMaxEvalClasses);
    const bool loss = loss_out || counts_out || scratch;
    AVL_REQUIRE(!loss || (loss_out && counts_out && scratch), "avl_seg_eval_full_res: loss_out, counts_out and scratch go together");
    AVL_REQUIRE(labels_out || confusion || loss, "avl_seg_eval_full_res: nothing to compute (no labels_out, confusion or loss_out)");
    AVL_REQUIRE(gt || (!confusion && !loss), "avl_seg_eval_full_res: the confusion matrix and the loss need a ground truth (gt is NULL)");
    AVL_REQUIRE(!confusion || avl::aligned(confusion, 8), "avl_seg_eval_full_res: confusion is not 8-byte aligned");
    AVL_REQUIRE(!loss || (avl::aligned(loss_out, 8) && avl::aligned(counts_out, 8) && avl::aligned(scratch, 8)),
                "avl_seg_eval_full_res: loss_out, counts_out and scratch must be 8-byte aligned");
    const dim3 grid = avl::tiles(H, W);
    const int nb = (int)(grid.x * grid.y);
    avl::EvalOut e;
    e.gt = gt;
    e.ignore_index = ignore_index;
    e.labels = labels_out;
    e.confusion = confusion;
    e.slab_sum = loss ? static_cast<double*>(scratch) : nullptr;
    e.slab_cnt = loss ? reinterpret_cast<unsigned*>(e.slab_sum + nb) : nullptr;
    e.slab_inv = loss ? e.slab_cnt + nb : nullptr;
    hipStream_t s = avl::as_stream(stream);
    const size_t lds_bytes = ((confusion ? K * K : 0) + g.win_cap) * sizeof(float);
    hipLaunchKernelGGL(avl::k_full_res_eval, grid, dim3(avl::kThreads), lds_bytes, s, g, e);
    AVL_LAUNCH_CHECK();
    if (loss) {
        hipLaunchKernelGGL(avl::k_eval_finalize, dim3(1), dim3(avl::kThreads), 0, s, e.slab_sum, e.slab_cnt, e.slab_inv, nb, loss_out, counts_out);
        AVL_LAUNCH_CHECK();
    }
    return AVL_OK;
}
