// Depthwise k x k conv of the decoder's refine blocks for k != 3 (MODEL.DECODER.REFINE_KERNEL_SIZE; decoder.py:16-36):
// stride 1, dilation 1, padding 0, out = in - (k - 1), + bias + ReLU.  AVL_OP_DWCONV with ksize 1..7 other than 3 lands here
// (the 3x3 op keeps k_dwconv / k_dwconv_split / k_dwpw*).  NHWC, fp32 weights [k*k][C] (tap-major, as the 3x3 layout), fp32
// bias, one fmaf chain per output starting from the bias in row-major tap order -- whatever the storage type.
//
// Forms (one per kind of plan that reaches the op):
//   F32   fp32 in / out (the f32 plan)
//   HALF  one bf16 / f16 plane in and out (the f16 / bf16 plans)
//   SPLIT hi + lo f16 planes in and out (the "mixed" and "split16" decoders): the taps are hi + lo (exact in fp32), the result is
//         written as hi = round(acc), lo = acc - hi, as k_dwconv_split writes it.
//
// A workgroup owns an output tile of kTH x kTW pixels x one channel slab (128 B of a pixel in LDS: 64 channels of a 16-bit plane, or
// 32 fp32 channels for F32 / SPLIT, whose taps are staged as fp32).  It stages the input tile plus its k - 1 halo in LDS once
// (consecutive lanes = consecutive 16-byte chunks of a pixel: each pixel's slab is one contiguous read) together with the slab's
// k*k tap weights, so no input pixel is fetched from global memory more than once per workgroup and no lane holds all k*k weights.
// A lane then computes kR = 4 consecutive outputs of a row for 8 channels: per tap row it reads the kR + k - 1 input pixels it needs
// from LDS once and the row's k weight vectors, i.e. k (kR + k - 1) / kR LDS pixel reads per output instead of k*k.
#include "seg_types.h"

namespace avl {
namespace {

constexpr int kThreads = 256;
constexpr int kTW = 32, kTH = 8;       // output tile
constexpr int kR = 4;                  // outputs per lane along x
constexpr int kLX = kTW / kR;          // lanes along a tile row

enum { FORM_F32 = 0, FORM_HALF = 1, FORM_SPLIT = 2 };

struct DwkGeom {
    int H, W, C, in_ld, OH, OW, out_ld, relu;
    int tiles_x;
};

// 8 consecutive elements of a 16-bit plane (raw 16 bytes) -> 8 floats
template <typename T>
__device__ __forceinline__ void half8_to_f32(const uint4& raw, float (&v)[8]) {
    Vec8<T>::load(reinterpret_cast<const T*>(&raw), v);
}

template <typename T, int FORM, int KS>
__global__ void __launch_bounds__(kThreads) k_dwconv_k(const T* __restrict__ in, const T* __restrict__ in_lo, const float* __restrict__ w,
                                                      const float* __restrict__ bias, T* __restrict__ out, T* __restrict__ out_lo, DwkGeom g) {
    constexpr int NCH = FORM == FORM_HALF ? 8 : 4;        // 8-channel chunks per slab (128 B of a pixel in LDS)
    constexpr int CW = NCH * 8;                           // channels per slab
    constexpr int Q = FORM == FORM_HALF ? 1 : 2;          // 16-byte LDS words per chunk (8 x 16 bit, or 8 x fp32)
    constexpr int LY = kThreads / (NCH * kLX);            // lanes along the tile's rows
    constexpr int J = kTH / LY;                           // rows per lane
    constexpr int IW = kTW + KS - 1, IH = kTH + KS - 1;   // input tile with its halo
    static_assert(NCH * Q == 8 && kTH % LY == 0, "slab layout");
    __shared__ uint4 tile[IH * IW * 8];                   // [pixel][chunk][Q] 16-byte words: 128 B per pixel
    __shared__ float4 wl[KS * KS * CW / 4];               // [tap][slab channel]

    {
        const long long ipix = (long long)g.H * g.W, opix = (long long)g.OH * g.OW;
        in = image_base(in, ipix, g.in_ld);
        in_lo = image_base(in_lo, ipix, g.in_ld);
        out = image_base(out, opix, g.out_ld);
        out_lo = image_base(out_lo, opix, g.out_ld);
    }
    const int c0 = blockIdx.y * CW;                       // the slab's first channel
    const int tx0 = (blockIdx.x % g.tiles_x) * kTW, ty0 = (blockIdx.x / g.tiles_x) * kTH;

    // ---- stage the input tile (zeros outside the image: they only feed outputs that are not stored) and the slab's weights
    for (int e = threadIdx.x; e < IH * IW * NCH; e += kThreads) {
        const int p = e / NCH, c = e % NCH;
        const int iy = ty0 + p / IW, ix = tx0 + p % IW;
        uint4 v[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) v[q] = make_uint4(0u, 0u, 0u, 0u);
        if (iy < g.H && ix < g.W) {
            const long long o = ((long long)iy * g.W + ix) * g.in_ld + c0 + c * 8;
            if constexpr (FORM == FORM_HALF) {
                v[0] = *reinterpret_cast<const uint4*>(in + o);
            } else if constexpr (FORM == FORM_F32) {
                v[0] = *reinterpret_cast<const uint4*>(in + o);
                v[1] = *reinterpret_cast<const uint4*>(in + o + 4);
            } else {
                float h[8], l[8];
                Vec8<T>::load(in + o, h);
                Vec8<T>::load(in_lo + o, l);
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] += l[i];                  // exact: hi + lo carry ~22 significant bits
                v[0] = make_uint4(__float_as_uint(h[0]), __float_as_uint(h[1]), __float_as_uint(h[2]), __float_as_uint(h[3]));
                v[1] = make_uint4(__float_as_uint(h[4]), __float_as_uint(h[5]), __float_as_uint(h[6]), __float_as_uint(h[7]));
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) tile[p * 8 + c * Q + q] = v[q];
    }
    for (int e = threadIdx.x; e < KS * KS * CW / 4; e += kThreads) {
        const int t = e / (CW / 4), q = e % (CW / 4);
        wl[e] = *reinterpret_cast<const float4*>(w + (long long)t * g.C + c0 + q * 4);
    }
    __syncthreads();

    // ---- compute: lane = (chunk, run of kR outputs along x, row)
    const int c = threadIdx.x % NCH, slot = threadIdx.x / NCH;
    const int xr = slot % kLX, yl = slot / kLX;
    const int ox0 = tx0 + xr * kR;
    if (ox0 >= g.OW) return;
    float bs[8];
    {
        const float4 b0 = *reinterpret_cast<const float4*>(bias + c0 + c * 8), b1 = *reinterpret_cast<const float4*>(bias + c0 + c * 8 + 4);
        bs[0] = b0.x; bs[1] = b0.y; bs[2] = b0.z; bs[3] = b0.w; bs[4] = b1.x; bs[5] = b1.y; bs[6] = b1.z; bs[7] = b1.w;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int oyl = yl + j * LY, oy = ty0 + oyl;
        if (oy >= g.OH) break;
        float acc[kR][8];
#pragma unroll
        for (int r = 0; r < kR; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[r][i] = bs[i];
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky) {
            // the kR + KS - 1 input pixels of this tap row, read once
            float x[kR + KS - 1][8];
            const uint4* row = tile + ((oyl + ky) * IW + xr * kR) * 8 + c * Q;
#pragma unroll
            for (int p = 0; p < kR + KS - 1; ++p) {
                if constexpr (FORM == FORM_HALF) {
                    half8_to_f32<T>(row[p * 8], x[p]);
                } else {
                    const uint4 a = row[p * 8], b = row[p * 8 + 1];
                    x[p][0] = __uint_as_float(a.x); x[p][1] = __uint_as_float(a.y); x[p][2] = __uint_as_float(a.z); x[p][3] = __uint_as_float(a.w);
                    x[p][4] = __uint_as_float(b.x); x[p][5] = __uint_as_float(b.y); x[p][6] = __uint_as_float(b.z); x[p][7] = __uint_as_float(b.w);
                }
            }
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                const float4 w0 = wl[(ky * KS + kx) * (CW / 4) + c * 2], w1 = wl[(ky * KS + kx) * (CW / 4) + c * 2 + 1];
                const float wt[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                for (int r = 0; r < kR; ++r)
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[r][i] = fmaf(x[r + kx][i], wt[i], acc[r][i]);
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int ox = ox0 + r;
            if (ox >= g.OW) break;
            if (g.relu) {
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[r][i] = fmaxf(acc[r][i], 0.f);
            }
            const long long o = ((long long)oy * g.OW + ox) * g.out_ld + c0 + c * 8;
            Vec8<T>::store(out + o, acc[r]);
            if constexpr (FORM == FORM_SPLIT) {
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[r][i] -= to_f32(from_f32<T>(acc[r][i]));
                Vec8<T>::store(out_lo + o, acc[r]);
            }
        }
    }
}

template <typename T, int FORM>
int launch_form(const avl_seg_op& op, hipStream_t s) {
    DwkGeom g;
    g.H = op.in_h; g.W = op.in_w; g.C = op.in_c; g.in_ld = op.in_ld; g.OH = op.out_h; g.OW = op.out_w; g.out_ld = op.out_ld; g.relu = op.relu;
    g.tiles_x = (op.out_w + kTW - 1) / kTW;
    const int tiles_y = (op.out_h + kTH - 1) / kTH;
    const int cw = FORM == FORM_HALF ? 64 : 32;
    const dim3 grid((unsigned)(g.tiles_x * tiles_y), (unsigned)(op.in_c / cw), (unsigned)op_batch(op));
    const T* in = static_cast<const T*>(op.in);
    const T* in_lo = static_cast<const T*>(op.in_lo);
    T* out = static_cast<T*>(op.out);
    T* out_lo = static_cast<T*>(op.out_lo);
    const float* w = static_cast<const float*>(op.weight);
#define AVL_DWK(KS) hipLaunchKernelGGL((k_dwconv_k<T, FORM, KS>), grid, dim3(kThreads), 0, s, in, in_lo, w, op.bias, out, out_lo, g)
    switch (op.ksize) {
        case 1: AVL_DWK(1); break;
        case 2: AVL_DWK(2); break;
        case 4: AVL_DWK(4); break;
        case 5: AVL_DWK(5); break;
        case 6: AVL_DWK(6); break;
        case 7: AVL_DWK(7); break;
        default: return set_error(AVL_E_UNSUPPORTED, "dwconv ksize %d: built for 1, 2, 4, 5, 6, 7 (3 is k_dwconv)", op.ksize);
    }
#undef AVL_DWK
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

}  // namespace

// the fields the generic checks of validate_conv_op leave to the op (dtype, 16-byte strides, aligned buffers, rows, split planes = f16)
int validate_dwconv_k(const avl_seg_op& op) {
    const int k = op.ksize, es = elem_size(op.dtype);
    AVL_REQUIRE(k >= 1 && k <= 7 && k != 3, "dwconv ksize %d: the k x k kernel is built for ksize 1..7 (3 is the 3x3 op)", k);
    AVL_REQUIRE(op.weight && op.bias, "dwconv ksize %d: weight [k*k][C] and bias [C] are required", k);
    AVL_REQUIRE(op.out_c == op.in_c, "dwconv ksize %d: out_c %d != in_c %d", k, op.out_c, op.in_c);
    AVL_REQUIRE(op.stride == 1, "dwconv ksize %d: stride %d (only 1)", k, op.stride);
    AVL_REQUIRE(op.dil == 1, "dwconv ksize %d: dil %d (only 1)", k, op.dil);
    AVL_REQUIRE(op.pad == 0, "dwconv ksize %d: pad %d (only 0)", k, op.pad);
    AVL_REQUIRE(op.out_h == op.in_h - (k - 1), "dwconv ksize %d: out_h %d != in_h - (k - 1) = %d", k, op.out_h, op.in_h - (k - 1));
    AVL_REQUIRE(op.out_w == op.in_w - (k - 1), "dwconv ksize %d: out_w %d != in_w - (k - 1) = %d", k, op.out_w, op.in_w - (k - 1));
    AVL_REQUIRE(op.out_h >= 1 && op.out_w >= 1, "dwconv ksize %d: empty output (out_h %d, out_w %d)", k, op.out_h, op.out_w);
    AVL_REQUIRE(!op.out_mx, "dwconv ksize %d: out_mx (FP4 copies) is not supported", k);
    AVL_REQUIRE((op.in_lo == nullptr) == (op.out_lo == nullptr), "dwconv ksize %d: in_lo and out_lo must both be set or both unset", k);
    AVL_REQUIRE(op.in_c % (es == 2 ? 64 : 32) == 0, "dwconv ksize %d: channels %d not a multiple of one 128-byte line", k, op.in_c);
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(op.weight) % 16 == 0 && reinterpret_cast<uintptr_t>(op.bias) % 16 == 0,
                "dwconv ksize %d: weight / bias not 16-byte aligned", k);
    return AVL_OK;
}

int launch_dwconv_k(const avl_seg_op& op, hipStream_t s) {
    if (op.dtype == AVL_F32) return launch_form<float, FORM_F32>(op, s);
    if (op.dtype == AVL_BF16) return launch_form<bf16, FORM_HALF>(op, s);
    if (op.in_lo) return launch_form<f16, FORM_SPLIT>(op, s);
    return launch_form<f16, FORM_HALF>(op, s);
}

}  // namespace avl
