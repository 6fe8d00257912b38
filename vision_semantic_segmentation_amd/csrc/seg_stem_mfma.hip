// Stem on the matrix cores (bf16): uint8 RGB -> ToTensor/Normalize (semantic_segmentation.py:35-39) ->
// 7x7 stride-2 pad-3 conv 3->64 (torchvision ResNet.conv1) + folded bn1 + ReLU, NHWC bf16 out.
//
// Implicit GEMM with K laid out as [ky 7][kx*3+ci padded 21 -> 24]: inside one kernel row the 21 taps are 21
// CONTIGUOUS bytes of the image row, so a lane's 8-wide K fragment is 8 consecutive values of the normalised
// tile in LDS (the 3 pad positions per row carry zero weights).  K = 7*24 = 168 -> 6 MFMA steps of 32 (the last
// 24 are zero weights).  A workgroup converts an input tile (8x32 outputs -> 21x69 pixels) to normalised bf16 in
// LDS once (zeros outside the image: padding applies to the NORMALISED image), keeps all 24 weight fragments in
// registers and each wave walks 4 sub-tiles of 16 pixels: 21 LDS reads + 24 v_mfma_f32_16x16x32_bf16 per sub-tile.
//
// PRE = the node's pre-processing (vision_semantic_segmentation_node.py:83-98: BGR->RGB, cv2.undistort, INTER_AREA by an
// integer factor) happens in the loader: `img` is then the RAW camera frame and every pixel of the LDS tile is
// preprocessed_rgb() of seg_preprocess.h -- the function k_preprocess applies -- so the RGB network input is never written
// to memory or re-read.  The 5-pixel halo of a tile is recomputed (x1.41 pixels), which costs less than
// the round trip: the undistortion is ~60 double-precision flops per source pixel.  A batch of raw frames (avl_seg_op.raw_batch): image
// blockIdx.z, whose frame, output rows and CAMERA BLOCK (AVL_STEM_CAMERA_BYTES apart) the workgroup moves to at entry; a one-frame
// launch has z = 0.
//
// POOL = the max-pool (3x3 stride 2 pad 1, torchvision ResNet.maxpool) in the epilogue: a workgroup owns 4 x 16 POOLED outputs and computes
// the conv at the 9 x 33 positions their windows cover (rows 2 py0 - 1 .. 2 py0 + 7, columns 2 px0 - 1 .. 2 px0 + 31: 19 sub-tiles of 16
// positions over the four waves, the last one partial; input tile 23 x 71; 297 / 256 = 1.16x the conv work -- with the 8 x 32 conv tile
// pooled in place it would be 1.4x).  The results go through bias, ReLU and the conversion to HT into LDS [9 * 33][64] (16-byte chunks
// XOR-swizzled by position), and after one barrier the 256 lanes pool them with k_maxpool's rule (fmaxf from -INFINITY over the window
// positions inside the conv image, in its order): maxima of the very values the un-pooled stem stores, so the output is that of stem ->
// k_maxpool bit for bit, and the 540 x 960 x 64 conv map is never written or re-read.  Not with SPLIT.
//
// F32IN = an input already normalised by the caller (AVL_IN_F32_CHW: fp32 [3][H][W] planes, DeepLabV3Plus.forward's tensor): the
// loader reads it plane by plane, coalesced along x, and writes (HT)v (SPLIT: and (HT)(v - (float)(HT)v) into tile_lo) -- the
// conversion the uint8 table applies to its fp32 value, so a float equal to that value fills the same tile bits.
#include "seg_types.h"
#include "seg_preprocess.h"

namespace avl {
namespace {

constexpr int S_TH = 8, S_TW = 32;
constexpr int ROW = 224;                                      // bf16 values per LDS row (>= 69*3 + slack for the pad taps)

template <typename HT>
struct StemArgs {
    const unsigned char* img;
    const HT* w;           // [nj 4][step 6][i 16][k 32]; SPLIT: the hi parts, then the same array of lo parts
    const float* bias;    // [64]
    HT* out;
    HT* out_lo;            // SPLIT: the result's lo plane
    int H, W, OH, OW, out_ld, tiles_x;
    int PH, PW;                // POOL: the pooled size, which `out` has then (OH x OW stays the conv's)
    const PreCamera* cam;      // PRE: device memory (one captured graph serves both cameras); one block per image of a batch
    int srcH, srcW, factor;    // PRE: the raw frame; H = srcH / factor, W = srcW / factor
};

// SPLIT (the complete hi + lo pipeline): the NORMALISED image is kept as two f16 tiles (value = hi + lo), the weights are
// f16 pairs, the product runs Wh.xh + Wl.xh + Wh.xl and the result leaves as hi + lo planes: no f16-class rounding anywhere.
template <typename HT, bool PRE, bool SPLIT = false, bool F32IN = false, bool POOL = false>
__global__ void __launch_bounds__(256) k_stem_mfma(StemArgs<HT> p) {
    typedef typename Half16<HT>::v8 v8;
    static_assert(!(POOL && SPLIT), "the pooled epilogue stages one plane");
    constexpr int CTH = POOL ? 9 : S_TH, CTW = POOL ? 33 : S_TW;     // conv positions of a workgroup
    constexpr int ITH = 2 * CTH + 5, ITW = 2 * CTW + 5;              // its input pixels: 21 x 69, POOL 23 x 71
    constexpr int NPOS = CTH * CTW, NSUBT = (NPOS + 15) / 16;
    // a row holds the tile's pixels, and the last position's 24 taps (the 3 pad taps past the pixels read the zeroed slack) stay inside it
    static_assert(ITW * 3 <= ROW && (CTW - 1) * 6 + 24 <= ROW, "LDS row too short for the tile");
    __shared__ __attribute__((aligned(16))) HT tile[(ITH + 1) * ROW];
    __shared__ __attribute__((aligned(16))) HT stage[POOL ? NPOS * 64 : 8];
    __shared__ __attribute__((aligned(16))) HT tile_lo[SPLIT ? (ITH + 1) * ROW : 8];
    __shared__ HT lut[3 * 256];        // normalised value of every (channel, byte): exact divisions, done once
    __shared__ HT lut_lo[SPLIT ? 3 * 256 : 8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
    // first conv position of the tile (POOL: one row and column in front of the 4 x 16 pooled outputs' first window centre)
    const int oy0 = POOL ? ty * 8 - 1 : ty * S_TH, ox0 = POOL ? tx * 32 - 1 : tx * S_TW;
    const long long out_pix = POOL ? (long long)p.PH * p.PW : (long long)p.OH * p.OW;
    if constexpr (!PRE) {       // batch: image blockIdx.z
        p.img = image_base(p.img, (long long)p.H * p.W, F32IN ? 3 * (int)sizeof(float) : 3);     // (F32IN: `img` is the fp32 planes)
        p.out = image_base(p.out, out_pix, p.out_ld);
        p.out_lo = image_base(p.out_lo, out_pix, p.out_ld);
    } else {                    // batch of raw frames (raw_batch): frame blockIdx.z, and ITS camera block (AVL_STEM_CAMERA_BYTES apart)
        p.img = image_base(p.img, (long long)p.srcH * p.srcW, 3);
        p.out = image_base(p.out, out_pix, p.out_ld);
        p.out_lo = image_base(p.out_lo, out_pix, p.out_ld);
        p.cam = reinterpret_cast<const PreCamera*>(reinterpret_cast<const char*>(p.cam) + (long long)blockIdx.z * AVL_STEM_CAMERA_BYTES);
    }
    const int iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    if constexpr (PRE) {
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const float v = ((float)tid / 255.0f - mean[ci]) / stdv[ci];
            lut[ci * 256 + tid] = (HT)v;
            if constexpr (SPLIT) lut_lo[ci * 256 + tid] = (HT)(v - (float)(HT)v);
        }
        // the slack of every row and the extra row (read by the zero-weight pad taps)
        for (int e = tid; e < (ITH + 1) * ROW; e += 256) {
            const int ly = e / ROW, lc = e - ly * ROW;
            if (ly >= ITH || lc >= ITW * 3) { tile[e] = (HT)0.f; if constexpr (SPLIT) tile_lo[e] = (HT)0.f; }
        }
        const PreCamera cam = *p.cam;
        __syncthreads();
        for (int i = tid; i < ITH * ITW; i += 256) {
            const int ly = i / ITW, lx = i - ly * ITW;
            const int iy = iy0 + ly, ix = ix0 + lx;
            const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            int rgb[3] = {0, 0, 0};
            if (ok) preprocessed_rgb(p.img, p.srcH, p.srcW, cam, p.factor, ix, iy, rgb);
            HT* t = tile + ly * ROW + lx * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = ok ? lut[c * 256 + rgb[c]] : (HT)0.f;
            if constexpr (SPLIT) {
                HT* tl = tile_lo + ly * ROW + lx * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) tl[c] = ok ? lut_lo[c * 256 + rgb[c]] : (HT)0.f;
            }
        }
    } else if constexpr (F32IN) {
        // element e of the 3 x 21 x 69 input values: channel plane, then row, then column (consecutive lanes read consecutive floats
        // of one image row); all of a lane's loads are issued before the first conversion, as below
        constexpr int NV = ITH * ITW, NF = (3 * NV + 255) / 256;
        const float* src = reinterpret_cast<const float*>(p.img);
        const long long plane = (long long)p.H * p.W;
        float v[NF];
        unsigned okmask = 0;
    #pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int e = tid + i * 256;
            const int c = e / NV, r = e - c * NV;
            const int ly = r / ITW, lx = r - ly * ITW;
            const int iy = iy0 + ly, ix = ix0 + lx;
            const bool ok = e < 3 * NV && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            const int cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);      // unconditional load, masked below
            v[i] = src[min(c, 2) * plane + (long long)cy * p.W + cx];
            okmask |= (ok ? 1u : 0u) << i;
        }
        // the slack of every row and the extra row (read by the zero-weight pad taps)
        for (int e = tid; e < (ITH + 1) * ROW; e += 256) {
            const int ly = e / ROW, lc = e - ly * ROW;
            if (ly >= ITH || lc >= ITW * 3) { tile[e] = (HT)0.f; if constexpr (SPLIT) tile_lo[e] = (HT)0.f; }
        }
    #pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int e = tid + i * 256;
            if (e < 3 * NV) {
                const int c = e / NV, r = e - c * NV;
                const int ly = r / ITW, lx = r - ly * ITW;
                const float x = ((okmask >> i) & 1u) ? v[i] : 0.f;       // padding applies to the normalised image: 0
                tile[ly * ROW + lx * 3 + c] = (HT)x;
                if constexpr (SPLIT) tile_lo[ly * ROW + lx * 3 + c] = (HT)(x - (float)(HT)x);
            }
        }
    } else {
        // all of a lane's byte loads are issued before the first conversion (the element-at-a-time loop was a chain of
        // ~20 dependent global-load latencies per workgroup and cost more than the MFMAs)
        constexpr int NE = ((ITH + 1) * ROW + 255) / 256;
        unsigned char px[NE];
        unsigned okmask = 0;
    #pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int e = tid + i * 256;
            const int ly = e / ROW, lc = e - ly * ROW;
            const int lx = lc / 3;
            const int iy = iy0 + ly, ix = ix0 + lx;
            const bool ok = ly < ITH && lx < ITW && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            const int cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);      // unconditional load, masked below
            px[i] = p.img[((long long)cy * p.W + cx) * 3 + (lc - lx * 3)];
            okmask |= (ok ? 1u : 0u) << i;
        }
        // while the loads are in flight: the 768-entry table
    #pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const float v = ((float)tid / 255.0f - mean[ci]) / stdv[ci];
            lut[ci * 256 + tid] = (HT)v;
            if constexpr (SPLIT) lut_lo[ci * 256 + tid] = (HT)(v - (float)(HT)v);
        }
        __syncthreads();
    #pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int e = tid + i * 256;
            if (e < (ITH + 1) * ROW) {
                const int ci = (e % ROW) % 3;
                tile[e] = ((okmask >> i) & 1u) ? lut[ci * 256 + px[i]] : (HT)0.f;
                if constexpr (SPLIT) tile_lo[e] = ((okmask >> i) & 1u) ? lut_lo[ci * 256 + px[i]] : (HT)0.f;
            }
        }
    }
    const int fr = lane & 15, kq = lane >> 4;
    v8 wf[4][6];
#pragma unroll
    for (int nj = 0; nj < 4; ++nj)
#pragma unroll
        for (int st = 0; st < 6; ++st)
            wf[nj][st] = *reinterpret_cast<const v8*>(p.w + ((nj * 6 + st) * 16 + fr) * 32 + kq * 8);
    float bias[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 b = *reinterpret_cast<const float4*>(p.bias + kq * 16 + 4 * j);
        bias[4 * j] = b.x; bias[4 * j + 1] = b.y; bias[4 * j + 2] = b.z; bias[4 * j + 3] = b.w;
    }
    __syncthreads();

    for (int sub = wave; sub < NSUBT; sub += 4) {
        int sy, sx;
        if constexpr (POOL) {      // 16 consecutive positions of the 9 x 33 block; the last sub-tile's spare lanes redo the last position
            const int pos = min(sub * 16 + fr, NPOS - 1);
            sy = pos / CTW;
            sx = pos - sy * CTW;
        } else {
            sy = sub >> 1;
            sx = (sub & 1) * 16 + fr;
        }
        f32x4 acc[4];
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) acc[nj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 6; ++st) {
            // chunk index q = st*4 + kq in [0,24): kernel row ky = q/3, 8-wide piece (q%3) of its 24 taps
            const int q = st * 4 + kq;
            const int ky = q / 3, piece = q - ky * 3;
            v8 a;
            if (q < 21) {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(tile + (sy * 2 + ky) * ROW + sx * 6 + piece * 8);
                uint32_t u[4] = {src[0], src[1], src[2], src[3]};
                __builtin_memcpy(&a, u, 16);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) a[i] = (HT)0.f;
            }
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) acc[nj] = Half16<HT>::mfma(wf[nj][st], a, acc[nj]);
            if constexpr (SPLIT) {
                v8 al;
                if (q < 21) {
                    const uint32_t* src = reinterpret_cast<const uint32_t*>(tile_lo + (sy * 2 + ky) * ROW + sx * 6 + piece * 8);
                    uint32_t u[4] = {src[0], src[1], src[2], src[3]};
                    __builtin_memcpy(&al, u, 16);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) al[i] = (HT)0.f;
                }
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) {
                    // the lo parts of the weights are not kept in registers (96 more): 24 L1-resident 16-byte loads per sub-tile
                    const v8 wl = *reinterpret_cast<const v8*>(p.w + 4 * 6 * 16 * 32 + ((nj * 6 + st) * 16 + fr) * 32 + kq * 8);
                    acc[nj] = Half16<HT>::mfma(wf[nj][st], al, acc[nj]);
                    acc[nj] = Half16<HT>::mfma(wl, a, acc[nj]);
                }
            }
        }
        if constexpr (POOL) {
            if (sub * 16 + fr < NPOS) {      // (positions outside the conv image are staged too; the pool never looks at them)
                float lo[8], hi[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    lo[r] = fmaxf(acc[0][r] + bias[r], 0.f);
                    lo[4 + r] = fmaxf(acc[1][r] + bias[4 + r], 0.f);
                    hi[r] = fmaxf(acc[2][r] + bias[8 + r], 0.f);
                    hi[4 + r] = fmaxf(acc[3][r] + bias[12 + r], 0.f);
                }
                const int pos = sy * CTW + sx;
                HT* sp = stage + pos * 64;
                Vec8<HT>::store(sp + (((kq * 2) ^ (pos & 7)) << 3), lo);
                Vec8<HT>::store(sp + (((kq * 2 + 1) ^ (pos & 7)) << 3), hi);
            }
            continue;
        }
        const int oy = oy0 + sy, ox = ox0 + sx;
        if (oy < p.OH && ox < p.OW) {
            float lo[8], hi[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                lo[r] = fmaxf(acc[0][r] + bias[r], 0.f);
                lo[4 + r] = fmaxf(acc[1][r] + bias[4 + r], 0.f);
                hi[r] = fmaxf(acc[2][r] + bias[8 + r], 0.f);
                hi[4 + r] = fmaxf(acc[3][r] + bias[12 + r], 0.f);
            }
            HT* op = p.out + ((long long)oy * p.OW + ox) * p.out_ld + kq * 16;
            if constexpr (SPLIT) {
                float l0[8], l1[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float h0 = (float)(HT)lo[r], h1 = (float)(HT)hi[r];
                    l0[r] = lo[r] - h0; l1[r] = hi[r] - h1;
                    lo[r] = h0; hi[r] = h1;
                }
                HT* ol = p.out_lo + ((long long)oy * p.OW + ox) * p.out_ld + kq * 16;
                Vec8<HT>::store(ol, l0);
                Vec8<HT>::store(ol + 8, l1);
            }
            Vec8<HT>::store(op, lo);
            Vec8<HT>::store(op + 8, hi);
        }
    }
    if constexpr (POOL) {
        __syncthreads();
        // one lane = 8 channels of one pooled pixel: 4 x 16 pixels x 8 chunks over the 256 lanes, 16-byte stores, a pixel's 128 bytes together
        for (int i = tid; i < 4 * 16 * 8; i += 256) {
            const int c = i & 7, lpy = i >> 7, lpx = (i >> 3) & 15;
            const int py = ty * 4 + lpy, px = tx * 16 + lpx;
            if (py >= p.PH || px >= p.PW) continue;
            float m[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
            for (int ky = 0; ky < 3; ++ky) {
                const int cy = py * 2 - 1 + ky;
                if (cy < 0 || cy >= p.OH) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int cx = px * 2 - 1 + kx;
                    if (cx < 0 || cx >= p.OW) continue;
                    const int pos = (lpy * 2 + ky) * CTW + lpx * 2 + kx;         // = (cy - oy0) * CTW + (cx - ox0)
                    float v[8];
                    Vec8<HT>::load(stage + pos * 64 + ((c ^ (pos & 7)) << 3), v);
#pragma unroll
                    for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], v[j]);
                }
            }
            Vec8<HT>::store(p.out + ((long long)py * p.PW + px) * p.out_ld + c * 8, m);
        }
    }
}

}  // namespace

template <typename HT>
int launch_stem_typed(const avl_seg_op& op, hipStream_t s) {
    StemArgs<HT> a;
    a.img = static_cast<const unsigned char*>(op.in);
    a.w = static_cast<const HT*>(op.weight);
    a.bias = op.bias;
    a.out = static_cast<HT*>(op.out);
    a.out_lo = static_cast<HT*>(op.out_lo);
    a.H = op.in_h; a.W = op.in_w; a.OH = op.out_h; a.OW = op.out_w; a.out_ld = op.out_ld;
    // stride 4 (validate_conv_op): the max-pool in the epilogue, out_h x out_w is the pooled size; a workgroup owns 4 x 16 pooled outputs
    const bool pool = op.stride == 4;
    a.PH = op.out_h; a.PW = op.out_w;
    if (pool) { a.OH = (op.in_h + 6 - 7) / 2 + 1; a.OW = (op.in_w + 6 - 7) / 2 + 1; }
    a.tiles_x = pool ? (op.out_w + 15) / 16 : (op.out_w + S_TW - 1) / S_TW;
    const int tiles_y = pool ? (op.out_h + 3) / 4 : (op.out_h + S_TH - 1) / S_TH;
    a.cam = static_cast<const PreCamera*>(op.in2);
    a.srcW = op.in2_ld;
    a.srcH = op.in2_ld > 0 ? op.in_rows / op_batch(op) / op.in2_ld : 0;      // (in_rows counts the frames of a raw batch)
    a.factor = op.in_w > 0 ? a.srcW / op.in_w : 1;
    const dim3 grid(a.tiles_x * tiles_y, 1, op_batch(op));
    if (pool) {                                 // (validated: never split)
        if (op.in_format == AVL_IN_F32_CHW) hipLaunchKernelGGL((k_stem_mfma<HT, false, false, true, true>), grid, dim3(256), 0, s, a);
        else if (op.in2) hipLaunchKernelGGL((k_stem_mfma<HT, true, false, false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_stem_mfma<HT, false, false, false, true>), grid, dim3(256), 0, s, a);
    } else if (op.in_format == AVL_IN_F32_CHW) {       // (validated: never with in2)
        if (op.w_split) {
            if (!op.out_lo) return set_error(AVL_E_ARG, "split stem (w_split = 1): out_lo is NULL");
            hipLaunchKernelGGL((k_stem_mfma<HT, false, true, true>), grid, dim3(256), 0, s, a);
        } else {
            hipLaunchKernelGGL((k_stem_mfma<HT, false, false, true>), grid, dim3(256), 0, s, a);
        }
    } else if (op.w_split) {
        if (!op.out_lo) return set_error(AVL_E_ARG, "split stem (w_split = 1): out_lo is NULL");
        if (op.in2)
            hipLaunchKernelGGL((k_stem_mfma<HT, true, true>), grid, dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((k_stem_mfma<HT, false, true>), dim3(a.tiles_x * tiles_y, 1, op_batch(op)), dim3(256), 0, s, a);
    } else if (op.in2)
        hipLaunchKernelGGL((k_stem_mfma<HT, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_stem_mfma<HT, false>), dim3(a.tiles_x * tiles_y, 1, op_batch(op)), dim3(256), 0, s, a);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

int launch_stem_mfma(const avl_seg_op& op, hipStream_t s) {
    return op.dtype == AVL_F16 ? launch_stem_typed<f16>(op, s) : launch_stem_typed<bf16>(op, s);
}

}  // namespace avl
