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
// A batch of n images is one launch: the image index is blockIdx.z, and at entry a workgroup moves its 64-bit base pointers (logits, gt,
// labels, planes) to its image and writes its loss partial into its image's row of the slab; every per-lane offset stays that of one
// image, so each image computes exactly what a launch on it alone computes.  The confusion matrix is one for the batch;
// k_eval_finalize sums each image's partials in the single-image order and then the image sums in image order.
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
    long long image_stride;            // floats between two images' logits (image_rows * ld); blockIdx.z = image
};

// src_coord (seg_types.h): the product is rounded, and the tile's window below must see the very same value as every pixel inside it.

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

// BATCH: gridDim.z images (a launch for one image is the <false> kernel, which has no image arithmetic at all)
template <bool BATCH>
__global__ void __launch_bounds__(kThreads) k_upsample_logits(Geo g, float* __restrict__ out) {
    extern __shared__ float lds[];                              // [g.win_cap]
    if (BATCH) {
        g.logits += (long long)blockIdx.z * g.image_stride;
        out += (long long)blockIdx.z * g.K * g.H * g.W;
    }
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
    const unsigned char* gt;           // uint8 [n][H][W] or NULL
    int ignore_index;
    unsigned char* labels;             // uint8 [n][H][W] or NULL
    unsigned long long* confusion;     // [K][K] (ground truth, prediction), accumulated over the batch; NULL = none
    double* slab;                      // NULL = no loss; double [n][blocks] loss partials, then unsigned [n][blocks] pixels that contributed
                                       // to the loss, then unsigned [n][blocks] ground-truth values neither in [0, K) nor ignore_index
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

template <bool BATCH>
__global__ void __launch_bounds__(kThreads) k_full_res_eval(Geo g, EvalOut e) {
    extern __shared__ unsigned smem[];                          // [K * K histogram bins when e.confusion][g.win_cap window floats]
    unsigned* hist = smem;
    float* lds = reinterpret_cast<float*>(smem + (e.confusion ? g.K * g.K : 0));
    __shared__ double red_sum[kThreads / 64];
    __shared__ unsigned red_cnt[kThreads / 64], red_inv[kThreads / 64];
    const int KK = g.K * g.K;
    if (BATCH) {   // this workgroup's image
        const long long img = blockIdx.z, pixels = (long long)g.H * g.W;
        g.logits += img * g.image_stride;
        if (e.gt) e.gt += img * pixels;
        if (e.labels) e.labels += img * pixels;
    }
    if (e.confusion)
        for (int i = threadIdx.x; i < KK; i += kThreads) hist[i] = 0u;
    const int oy0 = blockIdx.y * kTileH, ox0 = blockIdx.x * kTileW;
    const Window win = stage_window(g, oy0, ox0, lds);          // (its barrier also orders the histogram's zeroing)
    const int ox = ox0 + (threadIdx.x & (kTileW - 1));
    LossPart lp = {0.0, 0u, 0u};
    if (ox < g.W) lp = e.slab ? eval_tile<true>(g, e, win, lds, hist, oy0, ox) : eval_tile<false>(g, e, win, lds, hist, oy0, ox);
    double lsum = lp.sum;
    unsigned cnt = lp.cnt, inv = lp.inv;
    if (e.confusion) {
        __syncthreads();
        for (int i = threadIdx.x; i < KK; i += kThreads) {
            const unsigned v = hist[i];
            if (v) atomicAdd(&e.confusion[i], (unsigned long long)v);
        }
    }
    if (e.slab) {
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
            const long long blocks = (long long)gridDim.x * gridDim.y * (BATCH ? gridDim.z : 1u);
            const long long b = ((long long)(BATCH ? blockIdx.z : 0u) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
            unsigned* slab_cnt = reinterpret_cast<unsigned*>(e.slab + blocks);
            e.slab[b] = sum;
            slab_cnt[b] = c;
            slab_cnt[blocks + b] = n;
        }
    }
}

// Per image (in order): its nb partials summed by one workgroup in a fixed order (a strided pass, then a tree) -> image_loss[i] = {sum,
// mean (NaN when no pixel contributed, as torch's cross_entropy)}, image_counts[i] = {contributing pixels, invalid ground-truth values}
// (both optional).  Then the batch: loss_out[0] = the image sums added in image order 0 .. n-1 in fp64, loss_out[1] = that sum over the
// batch's contributing pixels (torch's reduction='mean' over the batch; NaN when there is none), counts_out = the counts' totals.
// Bitwise reproducible, and image i's words are those of a launch on image i alone.
__global__ void __launch_bounds__(kThreads) k_eval_finalize(const double* __restrict__ slab_sum, const unsigned* __restrict__ slab_cnt,
                                                           const unsigned* __restrict__ slab_inv, int nb, int n, double* __restrict__ loss_out,
                                                           unsigned long long* __restrict__ counts_out, double* __restrict__ image_loss,
                                                           unsigned long long* __restrict__ image_counts) {
    __shared__ double s_sum[kThreads];
    __shared__ unsigned long long s_cnt[kThreads], s_inv[kThreads];
    double total = 0.0;
    unsigned long long total_cnt = 0, total_inv = 0;
#pragma unroll 1
    for (int img = 0; img < n; ++img) {
        const long long base = (long long)img * nb;
        double sum = 0.0;
        unsigned long long cnt = 0, inv = 0;
        for (int i = threadIdx.x; i < nb; i += kThreads) { sum += slab_sum[base + i]; cnt += slab_cnt[base + i]; inv += slab_inv[base + i]; }
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
            if (image_loss) {
                image_loss[2 * img] = s_sum[0];
                image_loss[2 * img + 1] = s_cnt[0] ? s_sum[0] / (double)s_cnt[0] : __builtin_nan("");
                image_counts[2 * img] = s_cnt[0];
                image_counts[2 * img + 1] = s_inv[0];
            }
            total = img ? total + s_sum[0] : s_sum[0];
            total_cnt += s_cnt[0];
            total_inv += s_inv[0];
        }
        __syncthreads();                                        // s_* are rewritten by the next image
    }
    if (threadIdx.x == 0) {
        loss_out[0] = total;
        loss_out[1] = total_cnt ? total / (double)total_cnt : __builtin_nan("");
        counts_out[0] = total_cnt;
        counts_out[1] = total_inv;
    }
}

bool aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

constexpr int kMaxBatch = 65535;           // gridDim.z

int make_geo(const float* logits, int n, int64_t image_rows, int h, int w, int K, int64_t ld, int H, int W, Geo& g, const char* what) {
    AVL_REQUIRE(logits, "%s: logits is NULL", what);
    AVL_REQUIRE(aligned(logits, 4), "%s: logits is not 4-byte aligned", what);
    AVL_REQUIRE(n >= 1 && n <= kMaxBatch, "%s: n = %d images (1 .. %d)", what, n, kMaxBatch);
    AVL_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0, "%s: sizes %d x %d -> %d x %d", what, h, w, H, W);
    AVL_REQUIRE((long long)H * W <= (1ll << 31) - 1 && (long long)h * w <= (1ll << 31) - 1, "%s: image too large", what);
    AVL_REQUIRE(K > 0, "%s: K = %d", what, K);
    AVL_REQUIRE(ld >= K, "%s: row stride %lld < K %d", what, (long long)ld, K);
    AVL_REQUIRE(image_rows >= (int64_t)h * w, "%s: image_rows %lld < h * w = %lld", what, (long long)image_rows, (long long)h * w);
    AVL_REQUIRE(image_rows <= (1ll << 61) / ld / n, "%s: n * image_rows * row stride (%d * %lld * %lld) too large", what, n,
                (long long)image_rows, (long long)ld);
    g.logits = logits;
    g.h = h; g.w = w; g.K = K; g.ld = ld; g.H = H; g.W = W;
    g.image_stride = (long long)image_rows * ld;
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

dim3 tiles(int H, int W, int n = 1) { return dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)n); }

int upsample(const char* what, const float* logits, int n, int64_t image_rows, int h, int w, int K, int64_t ld, float* out, int H, int W,
             void* stream) {
    Geo g;
    if (int rc = make_geo(logits, n, image_rows, h, w, K, ld, H, W, g, what)) return rc;
    if (K > 256) return set_error(AVL_E_UNSUPPORTED, "%s: K = %d > 256 classes", what, K);
    AVL_REQUIRE(out, "%s: out is NULL", what);
    AVL_REQUIRE(aligned(out, 4), "%s: out is not 4-byte aligned", what);
    if (n > 1) hipLaunchKernelGGL(k_upsample_logits<true>, tiles(H, W, n), dim3(kThreads), g.win_cap * sizeof(float), as_stream(stream), g, out);
    else hipLaunchKernelGGL(k_upsample_logits<false>, tiles(H, W), dim3(kThreads), g.win_cap * sizeof(float), as_stream(stream), g, out);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

int64_t scratch_bytes(const char* what, int n, int H, int W) {
    if (n < 1 || n > kMaxBatch) return set_error(AVL_E_ARG, "%s: n = %d images (1 .. %d)", what, n, kMaxBatch);
    if (H <= 0 || W <= 0) return set_error(AVL_E_ARG, "%s: size %d x %d", what, H, W);
    const dim3 t = tiles(H, W);
    return (int64_t)n * t.x * t.y * (sizeof(double) + 2 * sizeof(unsigned));
}

int eval(const char* what, const float* logits, int n, int64_t image_rows, int h, int w, int K, int64_t ld, int H, int W, const uint8_t* gt,
         int ignore_index, uint8_t* labels_out, unsigned long long* confusion, double* loss_out, unsigned long long* counts_out,
         double* image_loss_out, unsigned long long* image_counts_out, void* scratch, void* stream) {
    Geo g;
    if (int rc = make_geo(logits, n, image_rows, h, w, K, ld, H, W, g, what)) return rc;
    if (K > kMaxEvalClasses)
        return set_error(AVL_E_UNSUPPORTED, "%s: K = %d > %d classes (LDS confusion histogram, uint8 labels)", what, K, kMaxEvalClasses);
    const bool loss = loss_out || counts_out || scratch;
    AVL_REQUIRE(!loss || (loss_out && counts_out && scratch), "%s: loss_out, counts_out and scratch go together", what);
    AVL_REQUIRE(!image_loss_out == !image_counts_out, "%s: image_loss_out and image_counts_out go together", what);
    AVL_REQUIRE(!image_loss_out || loss, "%s: image_loss_out and image_counts_out need loss_out, counts_out and scratch", what);
    AVL_REQUIRE(labels_out || confusion || loss, "%s: nothing to compute (no labels_out, confusion or loss_out)", what);
    AVL_REQUIRE(gt || (!confusion && !loss), "%s: the confusion matrix and the loss need a ground truth (gt is NULL)", what);
    AVL_REQUIRE(!confusion || aligned(confusion, 8), "%s: confusion is not 8-byte aligned", what);
    AVL_REQUIRE(!loss || (aligned(loss_out, 8) && aligned(counts_out, 8) && aligned(scratch, 8)),
                "%s: loss_out, counts_out and scratch must be 8-byte aligned", what);
    AVL_REQUIRE(!image_loss_out || (aligned(image_loss_out, 8) && aligned(image_counts_out, 8)),
                "%s: image_loss_out and image_counts_out must be 8-byte aligned", what);
    const dim3 grid = tiles(H, W, n);
    const int nb = (int)(grid.x * grid.y);
    const long long slabs = (long long)n * nb;
    EvalOut e;
    e.gt = gt;
    e.ignore_index = ignore_index;
    e.labels = labels_out;
    e.confusion = confusion;
    e.slab = loss ? static_cast<double*>(scratch) : nullptr;
    hipStream_t s = as_stream(stream);
    const size_t lds_bytes = ((confusion ? K * K : 0) + g.win_cap) * sizeof(float);
    if (n > 1) hipLaunchKernelGGL(k_full_res_eval<true>, grid, dim3(kThreads), lds_bytes, s, g, e);
    else hipLaunchKernelGGL(k_full_res_eval<false>, grid, dim3(kThreads), lds_bytes, s, g, e);
    AVL_LAUNCH_CHECK();
    if (loss) {
        const unsigned* slab_cnt = reinterpret_cast<const unsigned*>(e.slab + slabs);
        hipLaunchKernelGGL(k_eval_finalize, dim3(1), dim3(kThreads), 0, s, e.slab, slab_cnt, slab_cnt + slabs, nb, n, loss_out, counts_out,
                           image_loss_out, image_counts_out);
        AVL_LAUNCH_CHECK();
    }
    return AVL_OK;
}

}  // namespace
}  // namespace avl

extern "C" int avl_upsample_logits(const float* logits, int h, int w, int K, int64_t ld, float* out, int H, int W, void* stream) {
    return avl::upsample("avl_upsample_logits", logits, 1, (int64_t)h * w, h, w, K, ld, out, H, W, stream);
}

extern "C" int avl_upsample_logits_batch(const float* logits, int n, int64_t image_rows, int h, int w, int K, int64_t ld, float* out, int H,
                                         int W, void* stream) {
    return avl::upsample("avl_upsample_logits_batch", logits, n, image_rows, h, w, K, ld, out, H, W, stream);
}

extern "C" int64_t avl_seg_eval_scratch_bytes(int H, int W) { return avl::scratch_bytes("avl_seg_eval_scratch_bytes", 1, H, W); }

extern "C" int64_t avl_seg_eval_scratch_bytes_batch(int n, int H, int W) {
    return avl::scratch_bytes("avl_seg_eval_scratch_bytes_batch", n, H, W);
}

extern "C" int avl_seg_eval_full_res(const float* logits, int h, int w, int K, int64_t ld, int H, int W, const uint8_t* gt,
                                     int ignore_index, uint8_t* labels_out, unsigned long long* confusion, double* loss_out,
                                     unsigned long long* counts_out, void* scratch, void* stream) {
    return avl::eval("avl_seg_eval_full_res", logits, 1, (int64_t)h * w, h, w, K, ld, H, W, gt, ignore_index, labels_out, confusion, loss_out,
                     counts_out, nullptr, nullptr, scratch, stream);
}

extern "C" int avl_seg_eval_full_res_batch(const float* logits, int n, int64_t image_rows, int h, int w, int K, int64_t ld, int H, int W,
                                           const uint8_t* gt, int ignore_index, uint8_t* labels_out, unsigned long long* confusion,
                                           double* loss_out, unsigned long long* counts_out, double* image_loss_out,
                                           unsigned long long* image_counts_out, void* scratch, void* stream) {
    return avl::eval("avl_seg_eval_full_res_batch", logits, n, image_rows, h, w, K, ld, H, W, gt, ignore_index, labels_out, confusion,
                     loss_out, counts_out, image_loss_out, image_counts_out, scratch, stream);
}
