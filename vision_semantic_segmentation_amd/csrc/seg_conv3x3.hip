// Dense 3x3 convolution (torchvision Bottleneck.conv2 of the ResNet / wide ResNet / ResNeXt-101 backbones: groups >= 1 with
// cg = C / groups a multiple of 64 channels) on the matrix cores, as an implicit GEMM:
//   M = output pixels, N = the group's output channels, K = 9 taps x cg input channels.
// No im2col buffer exists: a workgroup owns an 8 x 16 output-pixel tile x 64 NQ output channels of one group and walks K in
// chunks of one 128-byte pixel row (64 channels of a 16-bit type, 32 of fp32).  Per chunk the input tile with its dilation halo
// is staged ONCE into LDS by LDS-DMA (zero-filled outside the image, 16-byte slots XOR-swizzled with the pixel index as in
// k_gconv_mfma), and the nine taps are nine shifted reads of it.  Stride 1 with dilation d > 1 cuts the tile from one residue
// class (y mod d, x mod d) of the image, where the taps are one grid step apart: the halo is 10 x 18 pixels at any dilation.
// Stride 2 reads the strided tile directly (17 x 33 pixels at d = 1).
//
// Weights are packed on the host in MFMA fragment order (network.pack_conv3x3): per (group, chunk, tap, 32-channel block nb,
// n-tile nj, part p, K half h) one 1 KB fragment, lane l = kq * 16 + i holding output channel nb * 32 + (i >> 2) * 8 + nj * 4 +
// (i & 3) and the 16 bytes of input channels chunk * CK + (4 h + kq) * E .. + E - 1 (E = 8 for 16-bit types, 4 for fp32).
// They stream from L2 into registers, one tap ahead of the MFMAs.  The product is computed transposed (channels on MFMA rows,
// pixels on columns) so that a lane ends with 8 consecutive output channels of one pixel: bias + ReLU + one 16-byte store.
//
// Variants (template MODE):
//   0  one plane in, one plane out: v_mfma_f32_16x16x32_{bf16,f16}, or v_mfma_f32_16x16x4_f32 on fp32 activations;
//   1  "mixed" f16 hi + lo: weights as f16 pairs, out (+ out_lo) = Wh.xh + Wl.xh (+ Wh.xl when the input has a lo plane, XS).
// Four waves: wave w takes pixel rows 4 (w & 1) .. + 3 of the tile and 32 NQ of its 64 NQ channels ((w >> 1) half).
#include <type_traits>

#include "seg_types.h"

namespace avl {
namespace {

constexpr int C3_TH = 8, C3_TW = 16;       // output tile (pixels)
constexpr int C3_LDS_MAX = 160 * 1024;

template <typename T>
struct C3Args {
    const T* in;
    const T* in_lo;        // XS: the input's lo plane (same shape and stride), else NULL
    const uint4* w;        // fragments (see above)
    const float* bias;     // [C]
    T* out;
    T* out_lo;             // MODE 1: lo plane of the result, or NULL
    int H, W, in_ld, OH, OW, out_ld;
    int cg, nchunks;       // channels per group, K chunks per group (cg / CK)
    int nblk;              // channel blocks (64 NQ channels) per group
    int stride, dil, comb;
    int tiles_x, tiles_y;
    int in_th, in_tw, npix, ngroups, tw_magic;
    int tile_bytes;        // one plane's tile
};

template <typename T, int MODE, bool XS, int NQ>
__global__ void __launch_bounds__(256) k_conv3x3(C3Args<T> p) {
    static_assert(MODE == 0 || (sizeof(T) == 2 && !std::is_same<T, bf16>::value), "split planes are f16");
    static_assert(!XS || MODE == 1, "a split input goes with split weights");
    constexpr int ES = sizeof(T), E = 16 / ES;           // element size, elements per 16-byte slot
    constexpr int P = MODE == 1 ? 2 : 1;                 // weight parts (hi [, lo])
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, kq = lane >> 4;
    const int pw = wave & 1, cw = wave >> 1;

    {   // batch: image blockIdx.z
        const long long ipix = (long long)p.H * p.W, opix = (long long)p.OH * p.OW;
        p.in = image_base(p.in, ipix, p.in_ld);
        p.in_lo = image_base(p.in_lo, ipix, p.in_ld);
        p.out = image_base(p.out, opix, p.out_ld);
        p.out_lo = image_base(p.out_lo, opix, p.out_ld);
    }
    // ---- which tile, which channels
    const int bx = blockIdx.x;
    const int tx = bx % p.tiles_x, r1 = bx / p.tiles_x, ty = r1 % p.tiles_y, cmb = r1 / p.tiles_y;
    const int g = blockIdx.y / p.nblk, blk = blockIdx.y % p.nblk;
    const int s = p.stride;
    const int d = p.comb ? 1 : p.dil;                    // tap distance inside the LDS tile
    const int step = p.comb ? p.dil : 1;                 // image pixels per tile-grid step
    const int ry = p.comb ? cmb / p.dil : 0, rx = p.comb ? cmb % p.dil : 0;
    const int iy0 = ry + (ty * C3_TH * s - d) * step, ix0 = rx + (tx * C3_TW * s - d) * step;
    const int in_c0 = g * p.cg;                          // first input channel of the group
    const int nb0 = blk * 2 * NQ + cw * NQ;              // this wave's first 32-channel block inside the group
    const unsigned lds0 = lds_addr(lds);

    // ---- weights: this wave's fragments of one (chunk, tap) step, prefetched one step ahead
    const int NB = p.cg / 32;
    const long long step_frags = (long long)NB * 2 * P * 2;                  // 1 KB fragments per (chunk, tap)
    const uint4* wg = p.w + (long long)g * p.nchunks * 9 * step_frags * 64 + (long long)nb0 * 2 * P * 2 * 64 + lane;
    uint4 wf[NQ][2][P][2], wn[NQ][2][P][2];
    auto load_w = [&](int st, uint4 (&dst)[NQ][2][P][2]) {
        const uint4* q = wg + (long long)st * step_frags * 64;
#pragma unroll
        for (int a = 0; a < NQ; ++a)
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int pp = 0; pp < P; ++pp)
#pragma unroll
                    for (int h = 0; h < 2; ++h) dst[a][nj][pp][h] = q[(((a * 2 + nj) * P + pp) * 2 + h) * 64];
    };
    load_w(0, wf);

    // ---- accumulators start from the bias
    f32x4 acc[4][NQ][2];
#pragma unroll
    for (int a = 0; a < NQ; ++a)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + in_c0 + (nb0 + a) * 32 + kq * 8 + nj * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j][a][nj] = f32x4{b.x, b.y, b.z, b.w};
        }

    // ---- one chunk of the input tile (+ halo) into LDS: one DMA instruction = 8 pixels x 128 B; out-of-image pixels read a
    // clamped address and are zeroed once the data has landed (bit per instruction in `oob`)
    auto stage = [&](int chunk) -> unsigned long long {
        const int prow = lane >> 3, cphys = lane & 7;
        const T* base = p.in + in_c0 + chunk * E * 8;
        const T* base_lo = XS ? p.in_lo + in_c0 + chunk * E * 8 : nullptr;
        unsigned long long oob = 0;
        int it = 0;
        for (int gi = wave; gi < p.ngroups; gi += 4, ++it) {
            const int pix = gi * 8 + prow;
            const int ly = (pix * p.tw_magic) >> 16, lx = pix - ly * p.in_tw;      // pix / in_tw (exact: checked on the host)
            const int iy = iy0 + ly * step, ix = ix0 + lx * step;
            const unsigned outside = (unsigned)(pix >= p.npix) | (unsigned)((unsigned)iy >= (unsigned)p.H) | (unsigned)((unsigned)ix >= (unsigned)p.W);
            const int cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);
            const unsigned voff = ((unsigned)(cy * p.W + cx) * (unsigned)p.in_ld + (unsigned)((cphys ^ (pix & 7)) * E)) * (unsigned)ES;
            glds16_saddr(base, voff, lds0 + gi * 1024);
            if constexpr (XS) glds16_saddr(base_lo, voff, lds0 + p.tile_bytes + gi * 1024);
            oob |= (unsigned long long)outside << it;
        }
        return oob;
    };
    auto zero_oob = [&](unsigned long long mask) {
        int it = 0;
        for (int gi = wave; gi < p.ngroups && mask; gi += 4, ++it)
            if ((mask >> it) & 1ull) {
                *reinterpret_cast<uint4*>(lds + gi * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
                if constexpr (XS) *reinterpret_cast<uint4*>(lds + p.tile_bytes + gi * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
            }
    };

    const int nsteps = p.nchunks * 9;
    for (int chunk = 0; chunk < p.nchunks; ++chunk) {
        if (chunk) __syncthreads();                    // every wave is done with the previous chunk's tile
        const unsigned long long oob = stage(chunk);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        zero_oob(oob);
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int st = chunk * 9 + t;
            if (st + 1 < nsteps) load_w(st + 1, wn);
            const int ky = t / 3, kx = t - 3 * (t / 3);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = 4 * h + kq;              // this lane's logical 16-byte slot of the pixel row
                uint4 xb[4], xl[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int pix = ((pw * 4 + j) * s + ky * d) * p.in_tw + fr * s + kx * d;
                    const int off = pix * 128 + ((c ^ (pix & 7)) << 4);
                    xb[j] = *reinterpret_cast<const uint4*>(lds + off);
                    if constexpr (XS) xl[j] = *reinterpret_cast<const uint4*>(lds + p.tile_bytes + off);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int a = 0; a < NQ; ++a)
#pragma unroll
                        for (int nj = 0; nj < 2; ++nj) {
                            if constexpr (ES == 4) {
                                const float4 wv = __builtin_bit_cast(float4, wf[a][nj][0][h]);
                                const float4 xv = __builtin_bit_cast(float4, xb[j]);
                                f32x4 c4 = acc[j][a][nj];
                                c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, xv.x, c4, 0, 0, 0);
                                c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, xv.y, c4, 0, 0, 0);
                                c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, xv.z, c4, 0, 0, 0);
                                c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, xv.w, c4, 0, 0, 0);
                                acc[j][a][nj] = c4;
                            } else {
                                typedef typename Half16<T>::v8 v8;
                                const v8 xv = __builtin_bit_cast(v8, xb[j]);
                                f32x4 c4 = Half16<T>::mfma(__builtin_bit_cast(v8, wf[a][nj][0][h]), xv, acc[j][a][nj]);
                                if constexpr (MODE == 1) {
                                    c4 = Half16<T>::mfma(__builtin_bit_cast(v8, wf[a][nj][P - 1][h]), xv, c4);        // Wl . xh
                                    if constexpr (XS) c4 = Half16<T>::mfma(__builtin_bit_cast(v8, wf[a][nj][0][h]), __builtin_bit_cast(v8, xl[j]), c4);   // Wh . xl
                                }
                                acc[j][a][nj] = c4;
                            }
                        }
            }
            if (st + 1 < nsteps) {
#pragma unroll
                for (int a = 0; a < NQ; ++a)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                        for (int pp = 0; pp < P; ++pp)
#pragma unroll
                            for (int h = 0; h < 2; ++h) wf[a][nj][pp][h] = wn[a][nj][pp][h];
            }
        }
    }

    // ---- epilogue: ReLU, (hi / lo split), one 16-byte store (two for fp32) per lane, pixel and 32-channel block
    const int ox = rx + ((tx * C3_TW) + fr) * step;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = ry + (ty * C3_TH + pw * 4 + j) * step;
        if (oy >= p.OH || ox >= p.OW) continue;
        const long long pix = (long long)oy * p.OW + ox;
#pragma unroll
        for (int a = 0; a < NQ; ++a) {
            const int cb = in_c0 + (nb0 + a) * 32 + kq * 8;
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = fmaxf(acc[j][a][0][r], 0.f);
                v[4 + r] = fmaxf(acc[j][a][1][r], 0.f);
            }
            if constexpr (MODE == 0) {
                Vec8<T>::store(p.out + pix * p.out_ld + cb, v);
            } else {
                f16x8 hv, lv;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    hv[r] = (f16)v[r];
                    lv[r] = (f16)(v[r] - (float)hv[r]);
                }
                *reinterpret_cast<f16x8*>(p.out + pix * p.out_ld + cb) = hv;
                if (p.out_lo) *reinterpret_cast<f16x8*>(p.out_lo + pix * p.out_ld + cb) = lv;
            }
        }
    }
}

struct C3Geom {
    int comb, in_th, in_tw, npix, ngroups, tile_bytes, lds_bytes;
};

C3Geom conv3x3_geom(const avl_seg_op& op) {
    C3Geom q;
    q.comb = (op.stride == 1 && op.dil > 1) ? 1 : 0;
    const int d = q.comb ? 1 : op.dil;
    q.in_th = (C3_TH - 1) * op.stride + 2 * d + 1;
    q.in_tw = (C3_TW - 1) * op.stride + 2 * d + 1;
    q.npix = q.in_th * q.in_tw;
    q.ngroups = (q.npix + 7) / 8;
    q.tile_bytes = q.ngroups * 1024;
    q.lds_bytes = q.tile_bytes * (op.in_lo ? 2 : 1);
    return q;
}

template <typename T, int MODE, bool XS>
int launch_conv3x3_typed(const avl_seg_op& op, hipStream_t s) {
    const C3Geom q = conv3x3_geom(op);
    C3Args<T> a;
    a.in = static_cast<const T*>(op.in);
    a.in_lo = static_cast<const T*>(op.in_lo);
    a.w = static_cast<const uint4*>(op.weight);
    a.bias = op.bias;
    a.out = static_cast<T*>(op.out);
    a.out_lo = static_cast<T*>(op.out_lo);
    a.H = op.in_h; a.W = op.in_w; a.in_ld = op.in_ld; a.OH = op.out_h; a.OW = op.out_w; a.out_ld = op.out_ld;
    a.cg = op.in_c / op.groups;
    a.nchunks = a.cg / (64 * 2 / (int)sizeof(T));
    a.stride = op.stride; a.dil = op.dil; a.comb = q.comb;
    const int gh = q.comb ? (op.out_h + op.dil - 1) / op.dil : op.out_h, gw = q.comb ? (op.out_w + op.dil - 1) / op.dil : op.out_w;
    a.tiles_x = (gw + C3_TW - 1) / C3_TW;
    a.tiles_y = (gh + C3_TH - 1) / C3_TH;
    a.in_th = q.in_th; a.in_tw = q.in_tw; a.npix = q.npix; a.ngroups = q.ngroups; a.tile_bytes = q.tile_bytes;
    a.tw_magic = (65536 + q.in_tw - 1) / q.in_tw;
    const unsigned nx = (unsigned)(a.tiles_x * a.tiles_y * (q.comb ? op.dil * op.dil : 1));
    // 128 output channels per workgroup where the group has them, else 64
    if (a.cg % 128 == 0) {
        a.nblk = a.cg / 128;
        AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv3x3<T, MODE, XS, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, C3_LDS_MAX));
        hipLaunchKernelGGL((k_conv3x3<T, MODE, XS, 2>), dim3(nx, a.nblk * op.groups, op_batch(op)), dim3(256), q.lds_bytes, s, a);
    } else {
        a.nblk = a.cg / 64;
        AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv3x3<T, MODE, XS, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, C3_LDS_MAX));
        hipLaunchKernelGGL((k_conv3x3<T, MODE, XS, 1>), dim3(nx, a.nblk * op.groups, op_batch(op)), dim3(256), q.lds_bytes, s, a);
    }
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

}  // namespace

// AVL_OP_GCONV with w_layout = 2 (called from validate_conv_op after the generic geometry checks)
int validate_conv3x3(const avl_seg_op& op) {
    const int cg = op.in_c / op.groups;
    AVL_REQUIRE(cg % 64 == 0, "dense 3x3 conv (w_layout 2) needs channels per group %% 64 == 0 (got %d)", cg);
    AVL_REQUIRE(op.dtype == AVL_F32 || is_half(op.dtype), "dense 3x3 conv: dtype %d", op.dtype);
    AVL_REQUIRE(op.w_split == 0 || op.w_split == 1, "dense 3x3 conv: w_split %d (0, or 1 = f16 hi + lo weights)", op.w_split);
    AVL_REQUIRE(!op.w_split || op.dtype == AVL_F16, "dense 3x3 conv: split weights need AVL_F16 activations");
    AVL_REQUIRE(!op.in_lo || op.w_split, "dense 3x3 conv: a split input needs split weights (w_split 1)");
    AVL_REQUIRE(!op.out_lo || op.w_split, "dense 3x3 conv: a split output needs split weights (w_split 1)");
    AVL_REQUIRE(!op.in2_lo && !op.out_mx && !op.in_mx && !op.w_mx && !op.mx_flags, "dense 3x3 conv writes and reads no MX-FP4 bundle");
    AVL_REQUIRE(op.relu == 1, "dense 3x3 conv: the ReLU is part of the kernel (relu = 1)");
    AVL_REQUIRE(reinterpret_cast<uintptr_t>(op.weight) % 16 == 0 && reinterpret_cast<uintptr_t>(op.bias) % 16 == 0, "dense 3x3 conv: unaligned weights / bias");
    const C3Geom q = conv3x3_geom(op);
    AVL_REQUIRE(q.lds_bytes <= C3_LDS_MAX && q.ngroups <= 4 * 64, "dense 3x3 conv: the input tile of stride %d, dilation %d does not fit LDS", op.stride, op.dil);
    for (int pix = 0; pix < q.ngroups * 8; ++pix)
        AVL_REQUIRE(((pix * ((65536 + q.in_tw - 1) / q.in_tw)) >> 16) == pix / q.in_tw, "dense 3x3 conv: tile %d x %d too large for the reciprocal division",
                    q.in_th, q.in_tw);
    const int es = elem_size(op.dtype);
    AVL_REQUIRE((long long)op.in_rows * op.in_ld * es < (1LL << 31), "dense 3x3 conv: input plane beyond 2 GB (32-bit DMA offsets)");
    return AVL_OK;
}

int launch_conv3x3(const avl_seg_op& op, hipStream_t s) {
    if (op.w_split) return op.in_lo ? launch_conv3x3_typed<f16, 1, true>(op, s) : launch_conv3x3_typed<f16, 1, false>(op, s);
    if (op.dtype == AVL_F32) return launch_conv3x3_typed<float, 0, false>(op, s);
    if (op.dtype == AVL_F16) return launch_conv3x3_typed<f16, 0, false>(op, s);
    return launch_conv3x3_typed<bf16, 0, false>(op, s);
}

}  // namespace avl
