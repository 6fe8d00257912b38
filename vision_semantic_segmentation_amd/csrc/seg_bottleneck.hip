// One torchvision Bottleneck (backbone/resnet.py:24-43 over torchvision's Bottleneck: conv1 1x1 -> BN -> ReLU -> grouped 3x3 ->
// BN -> ReLU -> conv3 1x1 -> BN -> (+ identity | + downsample 1x1) -> ReLU) as ONE persistent kernel, "mixed" precision.
//
// What the three-launch form pays for in layer1 (width 128, 129 600 pixels at 1080p) is bytes: conv1's output, the 3x3's output as two
// planes, the block input a second time for the residual -- 0.35 ms for 8 % of the frame's flops, every launch HBM-bound.  Here a
// workgroup owns an 8 x 16 output-pixel tile for ALL channels and the intermediates never leave the CU:
//   conv1   on the 10 x 18 halo (180 pixels, 12 MFMA row tiles): X tile [192 px][CIN] f16 in LDS (LDS-DMA, 64-channel slabs of 128-byte
//           rows, XOR-swizzled on the DMA source), weights as f16 pairs hi + lo in MFMA fragment order straight from L2 into
//           registers.  Wave w owns output channels 16 w .. 16 w + 15 for all 12 row tiles.
//   t1      = ReLU(conv1 + b1), zero outside the image (the 3x3 pads t1, not x), f16 hi (+ lo plane where LDS allows) in LDS as
//           [halo px][128 ch], 256-byte rows, 16-byte chunks XOR-swizzled with px & 15.
//   conv2   grouped 3x3 as dense block-diagonal 16-CHANNEL windows: K = 32 = TWO TAPS x 16 channels, so nine taps are 5 MFMAs per
//           window and row tile (the 32-channel windows of k_gconv_mfma need 18).  Window w is exactly the 16 channels wave w
//           produced in conv1, for all pixels: conv1 -> conv2 needs NO barrier, a wave reads back only what it wrote itself.
//   t2      = ReLU(conv2 + b2) as hi + lo f16 planes, written IN PLACE over the wave's own t1 entries (its results sit in
//           registers by then).
//   conv3   [256 out][128] + bias + residual (the block input re-read from L2 in accumulator layout) or + the downsample 1x1 as
//           two more K steps on the X tile still in LDS; wave w owns 32 output channels (two interleaved n-tiles: a lane holds 8
//           consecutive channels of one pixel = one 16-byte store per plane).
// Per tile: two barriers (t2 visible | t2 read + next X tile landed).  The next tile's X DMA is issued right behind the first
// barrier and has all of conv3 to land.  Every product runs Wh.xh + Wl.xh (+ Wh.xl where the operand has a lo plane) on
// v_mfma_f32_16x16x32_f16 with fp32 accumulation.
#include "seg_types.h"

namespace avl {
namespace {

constexpr int BT_H = 8, BT_W = 16;                  // output tile
constexpr int BH_W = BT_W + 2, BH_H = BT_H + 2;     // halo tile
constexpr int BN_HALO = BH_W * BH_H;                // 180 pixels
constexpr int BN_M1 = 12;                           // conv1 row tiles (192 rows, the last 12 are padding)
constexpr int BN_WIDTH = 128, BN_COUT = 256;
constexpr int XSLAB = 192 * 128;                    // one 64-channel slab of the X tile
constexpr int PLANE1 = 192 * 256;                   // t1 plane (hi or lo)
constexpr int PLANE2 = 128 * 256;                   // t2 plane

struct BnArgs {
    const f16* x;        // block input [rows][in_ld], hi plane
    const f16* x_lo;     // its lo plane (enters the residual sum only) or NULL
    f16* out;
    f16* out_lo;         // NULL: single plane
    const f16* w1;       // [n 8][ks CIN/32][hi, lo][lane 64][8]
    const f16* w2;       // [window 8][ks 5][hi, lo][lane 64][8]
    const f16* w3;       // [wave 8][ks 4 (+ CIN/32 downsample steps)][nj 2][hi, lo][lane 64][8]
    const float* b1;     // [128]
    const float* b2;     // [128]
    const float* b3;     // [256] (downsample bias folded in)
    int H, W, in_ld, out_ld;
    int tiles_x, ntiles;
    int out_bytes;       // one output plane (buffer stores are range-checked against it)
};

template <int CIN, bool DS, bool T1LO>
struct BnLayout {
    static constexpr int NCH = CIN / 64;                          // 64-channel slabs of the X tile
    static constexpr int XTILE = NCH * XSLAB;
    static constexpr int XBYTES = (DS ? 2 : 1) * XTILE;           // DS: the X tile stays for conv3's downsample steps -> two of them
    static constexpr int T1LO_OFF = PLANE1;
    static constexpr int T2LO_OFF = T1LO ? PLANE1 : PLANE2;
    static constexpr int ABYTES = T1LO ? 2 * PLANE1 : 2 * PLANE2;
    static constexpr int LDS = XBYTES + ABYTES;
    static_assert(LDS <= 160 * 1024, "bottleneck tile does not fit the LDS");
};

typedef f16 h2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ReLU on fp32 as ONE instruction (v_med3_f32; fmaxf costs a canonicalising v_max first)
__device__ __forceinline__ float relu_f32(float v) { return __builtin_amdgcn_fmed3f(v, 0.f, 3.0e38f); }

// four fp32 -> packed f16 with ReLU applied on the packed halves (v_cvt_pk_f16_f32 + v_pk_max_f16: rounding is monotone and keeps the sign)
__device__ __forceinline__ uint2 relu_pack4(f32x4 v) {
    const h2v z = {(f16)0.f, (f16)0.f};
    const h2v a = __builtin_elementwise_max(h2v{(f16)v[0], (f16)v[1]}, z), b = __builtin_elementwise_max(h2v{(f16)v[2], (f16)v[3]}, z);
    return make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
}

// f16(v - hi_half) in ONE instruction (v_fma_mixlo / mixhi_f16: an fma whose first operand is an f16 half, rounded once to f16), written into
// the low / high half of `d`.  hipcc does not form these from (f16)(v - (float)h): it emits cvt, sub, cvt.  The inputs must come from ordinary
// vector instructions (here: v_med3 / v_cvt_pk), never straight from an MFMA: hipcc pads MFMA -> VALU hazards only for instructions it knows.
__device__ __forceinline__ unsigned lo_pair(unsigned hipk, float v0, float v1) {
    unsigned d;
    asm("v_fma_mixlo_f16 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(hipk), "v"(v0));
    asm("v_fma_mixhi_f16 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(d) : "v"(hipk), "v"(v1));
    return d;
}

// four (already rectified) fp32 -> packed f16 hi parts and the packed f16 lo parts of what the rounding dropped
__device__ __forceinline__ void split4(const float (&v)[4], uint2& hi, uint2& lo) {
    const h2v a = {(f16)v[0], (f16)v[1]}, b = {(f16)v[2], (f16)v[3]};
    hi = make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
    lo = make_uint2(lo_pair(hi.x, v[0], v[1]), lo_pair(hi.y, v[2], v[3]));
}

template <int CIN, bool DS, bool T1LO, bool XLO, bool OLO>
__global__ void __launch_bounds__(512) k_bottleneck(BnArgs p) {
    typedef BnLayout<CIN, DS, T1LO> L;
    constexpr int KS1 = CIN / 32;                 // conv1 K steps
    constexpr int KS3 = 4 + (DS ? CIN / 32 : 0);  // conv3 K steps (+ downsample)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    const unsigned lds0 = lds_addr(lds);
    char* const A = lds + L::XBYTES;

    {   // batch: image blockIdx.z (its planes; the store range shrinks by what lies in front of the image)
        const long long ipix = (long long)p.H * p.W;
        p.x = image_base(p.x, ipix, p.in_ld);
        p.x_lo = image_base(p.x_lo, ipix, p.in_ld);
        p.out = image_base(p.out, ipix, p.out_ld);
        p.out_lo = image_base(p.out_lo, ipix, p.out_ld);
        p.out_bytes -= (int)((long long)blockIdx.z * ipix * p.out_ld * 2);
    }
    int bid = blockIdx.x;
    {   // XCD-aware bijective remap: the workgroups of one XCD take a contiguous run of tiles (neighbours share halo rows in one L2)
        const int nwg = gridDim.x, xcd = bid & 7, local = bid >> 3, qq = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + local;
    }

    // ---- X tile by LDS-DMA: one wave-instruction = 8 halo pixels x 128 B of one slab; lane -> (pixel, physical chunk), the swizzle
    // goes on the source address.  Pixels outside the image come from a clamped address: conv1 of them is never used (t1 is zeroed there).
    auto stage_group = [&](int tile, unsigned xbase, int j) __attribute__((always_inline)) {
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        int lo_ = lane;
        asm volatile("" : "+v"(lo_));            // (keeps the per-lane source offsets out of the loop preheader)
        const int gi = wave + 8 * j;
        const int pix = gi * 8 + (lo_ >> 3);
        const int hy = (pix * 3641) >> 16, hx = pix - hy * BH_W;          // pix / 18 for pix < 192
        const int iy = min(max(ty * BT_H - 1 + hy, 0), p.H - 1), ix = min(max(tx * BT_W - 1 + hx, 0), p.W - 1);
        const unsigned voff = ((unsigned)(iy * p.W + ix) * (unsigned)p.in_ld + (unsigned)(((lo_ & 7) ^ (pix & 7)) << 3)) * 2u;
#pragma unroll
        for (int kc = 0; kc < L::NCH; ++kc) glds16_saddr(p.x + kc * 64, voff, xbase + kc * XSLAB + gi * 1024);
    };
    auto stage = [&](int tile, unsigned xbase) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) stage_group(tile, xbase, j);
    };

    int tile = bid;
    int it = 0;                                   // tiles done by this workgroup (DS: X tile slot = it & 1)
    if (tile < p.ntiles) stage(tile, lds0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // lane constants
    const unsigned x_rd = (unsigned)(c * 128) + (unsigned)((q ^ (c & 7)) << 4);                        // + m * 2048 (+ 64 with bit flip for the second K step of a slab)
    const unsigned a_wr = (unsigned)(c * 256) + (unsigned)((((2 * wave) | (q >> 1)) ^ c) << 4) + (unsigned)((q & 1) * 8);   // t1 / t2 store: + m * 4096
    const unsigned t2_rd = (unsigned)(c * 256) + (unsigned)((q ^ c) << 4);                              // conv3 read: ^ (ks << 6), + m * 4096

    // weight fragments by BUFFER loads: wave-uniform resource (SGPRs) + 32-bit lane offset + scalar fragment offset -- per-request 64-bit
    // VGPR pointers were what hipcc hoisted out of the tile loop and spilled
    const __amdgpu_buffer_rsrc_t w1r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.w1)) + (size_t)wave * (KS1 * 2 * 1024), 0, KS1 * 2 * 1024, 0x00020000);
    const __amdgpu_buffer_rsrc_t w2r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.w2)) + (size_t)wave * (5 * 2 * 1024), 0, 5 * 2 * 1024, 0x00020000);
    const __amdgpu_buffer_rsrc_t w3r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.w3)) + (size_t)wave * (KS3 * 4 * 1024), 0, KS3 * 4 * 1024, 0x00020000);
    const int wlane = lane * 16;
    auto wfrag = [&](__amdgpu_buffer_rsrc_t r, int frag) __attribute__((always_inline)) {
        return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, wlane, frag * 1024, 0));
    };
    const int ch0 = 32 * wave + 8 * q;                     // conv3: this lane's 8 output channels
    // conv1's weights stay in registers for the whole tile (row tiles outside, K steps inside); requested at the top of the tile.
    // (Requesting the NEXT tile's during conv3, so that their L2 round trip is not exposed at the top of the tile, was measured: -1 us on
    // the single-plane variant, +8 us with a split output -- the 64 registers are missed in conv3 -- and spills with a split residual.)
    f16x8 w1f[KS1][2];

    for (; tile < p.ntiles; tile += gridDim.x, ++it) {
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        const char* X = lds + (DS ? (it & 1) * L::XTILE : 0);
        // (opaque copies of the lane coordinates: hipcc would otherwise hoist the ~70 tile-invariant LDS offsets and pixel masks out of
        // the tile loop and spill them)
        int co = c, qo = q;
        asm volatile("" : "+v"(co), "+v"(qo));
        const bool more = tile + (int)gridDim.x < p.ntiles;
        f16x8 w2f[5][2];
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) { w1f[ks][0] = wfrag(w1r, 2 * ks); w1f[ks][1] = wfrag(w1r, 2 * ks + 1); }
#pragma unroll
        for (int k2 = 0; k2 < 5; ++k2) { w2f[k2][0] = wfrag(w2r, 2 * k2); w2f[k2][1] = wfrag(w2r, 2 * k2 + 1); }
        // DS: two X tiles, the other one is free from the top of the tile on; the weight requests above go first, so nothing waits
        // behind the DMA burst before conv3's preloads -- a whole conv1 + conv2 later
        if (DS && more) stage(tile + gridDim.x, lds0 + ((it & 1) ^ 1) * L::XTILE);

        // ================================================= conv1 + t1 -> LDS + conv2 + t2 -> LDS as ONE software-pipelined stream
        // conv1 walks the 12 halo row tiles (K steps inside, weights in registers): the X fragments of row tile m + 1 are read while the 16
        // MFMAs of tile m run.  Output row r of the 3x3 reads halo pixels up to 18 r + 53, i.e. t1 row tiles 0 .. (18 r + 53) / 16: it is
        // issued as soon as those are stored, so the 3x3's MFMAs and all the vector work (ReLU, f16 split, masks, LDS addresses) run
        // beside conv1's MFMAs instead of in a phase of their own.  t2 row r goes IN PLACE over t1 rows 16 r .. 16 r + 15 of this wave's
        // own channels, which no later output row reads (those start at 18 (r + 1)).
        auto store_t1 = [&](int m, f32x4 acc) __attribute__((always_inline)) {
            const int h = m * 16 + co;
            const int hy = (h * 3641) >> 16, hx = h - hy * BH_W;
            const int iy = ty * BT_H - 1 + hy, ix = tx * BT_W - 1 + hx;
            const bool valid = ((unsigned)(h < BN_HALO) & (unsigned)((unsigned)iy < (unsigned)p.H) & (unsigned)((unsigned)ix < (unsigned)p.W)) != 0u;   // (branch-free)
            const unsigned vm = valid ? 0xffffffffu : 0u;
            if constexpr (T1LO) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = relu_f32(acc[k]);
                uint2 hi, lo;
                split4(v, hi, lo);
                *reinterpret_cast<uint2*>(A + a_wr + m * 4096) = make_uint2(hi.x & vm, hi.y & vm);
                *reinterpret_cast<uint2*>(A + L::T1LO_OFF + a_wr + m * 4096) = make_uint2(lo.x & vm, lo.y & vm);
            } else {
                const uint2 hi = relu_pack4(acc);
                *reinterpret_cast<uint2*>(A + a_wr + m * 4096) = make_uint2(hi.x & vm, hi.y & vm);
            }
        };
        uint2 t2lo[T1LO ? 1 : BT_H];                       // no t1 lo plane: the t2 lo plane shares LDS with t1 rows >= 128 -> stored after the last row
        const float4 bias1 = *reinterpret_cast<const float4*>(p.b1 + 16 * wave + 4 * q);
        const float4 bias2 = *reinterpret_cast<const float4*>(p.b2 + 16 * wave + 4 * q);
        const unsigned cw16 = (unsigned)(((2 * wave) | (qo & 1)) << 4);
        unsigned hk[5];
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) {
            const int t = min(2 * ks + (qo >> 1), 8);      // this lane's tap in the K step (the tenth "tap" has zero weights)
            hk[ks] = (unsigned)((t / 3) * BH_W + (t % 3) + co);         // halo pixel of output row 0
        }
        auto conv2_row = [&](int r) __attribute__((always_inline)) {
            f32x4 acc = f32x4{bias2.x, bias2.y, bias2.z, bias2.w};
            f16x8 th[5], tl[T1LO ? 5 : 1];
#pragma unroll
            for (int ks = 0; ks < 5; ++ks) {
                const unsigned h = hk[ks] + 18u * r;
                const unsigned off = (h << 8) + (cw16 ^ ((h & 15u) << 4));
                th[ks] = *reinterpret_cast<const f16x8*>(A + off);
                if constexpr (T1LO) tl[ks] = *reinterpret_cast<const f16x8*>(A + L::T1LO_OFF + off);
            }
            __builtin_amdgcn_sched_barrier(0);      // all of the row's fragments are requested before its first MFMA (hipcc otherwise pairs them up: one LDS round trip per two MFMAs; same-box A/B: -1.5 .. -4 us per block)
#pragma unroll
            for (int ks = 0; ks < 5; ++ks) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2f[ks][0], th[ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2f[ks][1], th[ks], acc, 0, 0, 0);
                if constexpr (T1LO) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2f[ks][0], tl[ks], acc, 0, 0, 0);
            }
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = relu_f32(acc[k]);
            uint2 hi, lo;
            split4(v, hi, lo);
            *reinterpret_cast<uint2*>(A + a_wr + r * 4096) = hi;
            if constexpr (T1LO) *reinterpret_cast<uint2*>(A + L::T2LO_OFF + a_wr + r * 4096) = lo;
            else t2lo[r] = lo;
        };
        // everything conv3 needs from global memory is requested BEFORE the X DMA of the next tile goes out (vmcnt counts in issue order: a load
        // behind the DMA burst would wait for the burst's HBM round trip at its first use) -- and as early as registers allow
        f16x8 w3f[KS3][4];
        uint4 resh[DS ? 1 : BT_H], resl[XLO ? BT_H : 1];
        static_assert(!(DS && XLO), "the downsample variant has no identity residual");
        auto preload_conv3 = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int ks = 0; ks < KS3; ++ks)
#pragma unroll
                for (int f = 0; f < 4; ++f) w3f[ks][f] = wfrag(w3r, ks * 4 + f);
            if constexpr (!DS) {
                // identity: the block input at the tile's own pixels, in accumulator layout (16 B per lane; L2 / MALL hits: the tile was staged from there)
#pragma unroll
                for (int rr = 0; rr < BT_H; ++rr) {
                    const int oy = min(ty * BT_H + rr, p.H - 1), ox = min(tx * BT_W + co, p.W - 1);
                    const unsigned roff = (unsigned)(oy * p.W + ox) * (unsigned)p.in_ld + (unsigned)ch0;
                    resh[rr] = *reinterpret_cast<const uint4*>(p.x + roff);
                    if constexpr (XLO) resl[rr] = *reinterpret_cast<const uint4*>(p.x_lo + roff);
                }
            }
        };
        {
            // X fragment addresses: slab pair (0,1 | 2,3) x K-step parity -> immediate offsets stay below 64 KB
            const char* xb[KS1 > 4 ? 4 : 2];
#pragma unroll
            for (int i = 0; i < (KS1 > 4 ? 4 : 2); ++i) xb[i] = X + (i >> 1) * 2 * XSLAB + (x_rd ^ ((i & 1) << 6));
            auto read_x = [&](int m, f16x8 (&xf)[KS1]) __attribute__((always_inline)) {
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks)
                    xf[ks] = *reinterpret_cast<const f16x8*>(xb[(ks >> 2) * 2 + (ks & 1)] + ((ks >> 1) & 1) * XSLAB + m * 2048);
            };
            f16x8 xf[2][KS1];
            read_x(0, xf[0]);
            int next_row = 0;
#pragma unroll
            for (int m = 0; m < BN_M1; ++m) {
                if (m + 1 < BN_M1) read_x(m + 1, xf[(m + 1) & 1]);
                f32x4 acc = f32x4{bias1.x, bias1.y, bias1.z, bias1.w};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1f[ks][0], xf[m & 1][ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1f[ks][1], xf[m & 1][ks], acc, 0, 0, 0);
                }
                // the 3x3's output rows whose t1 row tiles (0 .. m - 1 are stored at this point) are complete
#pragma unroll
                for (int r = 0; r < BT_H; ++r)
                    if (r >= next_row && (18 * r + 53) / 16 + 1 <= m) conv2_row(r);
#pragma unroll
                for (int r = 0; r < BT_H; ++r)
                    if (r >= next_row && (18 * r + 53) / 16 + 1 <= m) next_row = r + 1;
                store_t1(m, acc);
            }
            preload_conv3();                   // conv1's weight registers are free from here on: beside the last output rows of the 3x3
#pragma unroll
            for (int r = 0; r < BT_H; ++r)
                if (r >= next_row) conv2_row(r);
        }
        if constexpr (!T1LO) {
#pragma unroll
            for (int r = 0; r < BT_H; ++r) *reinterpret_cast<uint2*>(A + L::T2LO_OFF + a_wr + r * 4096) = t2lo[r];
        }
        __syncthreads();                                   // B2: t2 visible; every wave is done with the X tile it read in conv1

        // ================================================= conv3 (+ downsample) + residual, row by row; results packed in registers
        // The rows' results leave as they are produced, by BUFFER stores: a pixel outside the image gets an offset past the buffer's end
        // and the hardware drops it -- no branch, so the NUMBER of vector-memory instructions behind the last DMA instruction is fixed and
        // the landing of the next X tile can be awaited by count (vmcnt(N) passes once all but the N youngest have completed) without
        // waiting for these stores.
        const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t olrsrc = __builtin_amdgcn_make_buffer_rsrc(OLO ? p.out_lo : p.out, 0, p.out_bytes, 0x00020000);
        {
            const float4 b0 = *reinterpret_cast<const float4*>(p.b3 + ch0), b1 = *reinterpret_cast<const float4*>(p.b3 + ch0 + 4);
            auto read_t2 = [&](int r, f16x8 (&tf)[8]) __attribute__((always_inline)) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const unsigned base = t2_rd ^ (unsigned)(ks << 6);
                    tf[2 * ks] = *reinterpret_cast<const f16x8*>(A + base + r * 4096);
                    tf[2 * ks + 1] = *reinterpret_cast<const f16x8*>(A + L::T2LO_OFF + base + r * 4096);
                }
            };
            f16x8 tf[2][8];
            read_t2(0, tf[0]);
#pragma unroll
            for (int r = 0; r < BT_H; ++r) {
                if (!DS && r < 3 && more) stage_group(tile + gridDim.x, lds0, r);       // the next X tile, one third per row: B2 is behind us
                if (r + 1 < BT_H) read_t2(r + 1, tf[(r + 1) & 1]);                        // next row's fragments beside this row's MFMAs
                f32x4 a0 = f32x4{b0.x, b0.y, b0.z, b0.w}, a1 = f32x4{b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const f16x8 th = tf[r & 1][2 * ks], tl = tf[r & 1][2 * ks + 1];
                    a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks][0], th, a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks][2], th, a1, 0, 0, 0);
                    a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks][1], th, a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks][3], th, a1, 0, 0, 0);
                    a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks][0], tl, a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks][2], tl, a1, 0, 0, 0);
                }
                if constexpr (DS) {
                    // downsample 1x1 (stride 1) on the tile's own pixels of the X tile: KS1 more K steps
                    const int h = (r + 1) * BH_W + 1 + co;
#pragma unroll
                    for (int ks = 0; ks < KS1; ++ks) {
                        const f16x8 xb = *reinterpret_cast<const f16x8*>(X + (ks >> 1) * XSLAB + h * 128 + ((((ks & 1) * 4 + qo) ^ (h & 7)) << 4));
                        a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[4 + ks][0], xb, a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[4 + ks][2], xb, a1, 0, 0, 0);
                        a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[4 + ks][1], xb, a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[4 + ks][3], xb, a1, 0, 0, 0);
                    }
                }
                const int oy = ty * BT_H + r, ox = tx * BT_W + co;
                const bool live = ((unsigned)(oy < p.H) & (unsigned)(ox < p.W)) != 0u;
                const unsigned ooff = live ? ((unsigned)(oy * p.W + ox) * (unsigned)p.out_ld + (unsigned)ch0) * 2u : 0x80000000u;
                float v0[4] = {a0[0], a0[1], a0[2], a0[3]}, v1[4] = {a1[0], a1[1], a1[2], a1[3]};
                if constexpr (!DS) {
                    // + identity.  Plain C (cvt + add): an inline-asm v_fma_mix_f32 reading the MFMA result directly is NOT safe -- hipcc
                    // inserts the MFMA -> VALU wait states only for instructions it knows (measured: garbage sums)
                    const f16x8 rh = __builtin_bit_cast(f16x8, resh[r]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { v0[k] += (float)rh[k]; v1[k] += (float)rh[4 + k]; }
                    if constexpr (XLO) {
                        const f16x8 rl = __builtin_bit_cast(f16x8, resl[r]);
#pragma unroll
                        for (int k = 0; k < 4; ++k) { v0[k] += (float)rl[k]; v1[k] += (float)rl[4 + k]; }
                    }
                }
                if constexpr (OLO) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) { v0[k] = relu_f32(v0[k]); v1[k] = relu_f32(v1[k]); }
                    uint2 h0, l0, h1, l1;
                    split4(v0, h0, l0);
                    split4(v1, h1, l1);
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{h0.x, h0.y, h1.x, h1.y}, orsrc, ooff, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{l0.x, l0.y, l1.x, l1.y}, olrsrc, ooff, 0, 0);
                } else {
                    const uint2 h0 = relu_pack4(f32x4{v0[0], v0[1], v0[2], v0[3]}), h1 = relu_pack4(f32x4{v1[0], v1[1], v1[2], v1[3]});
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{h0.x, h0.y, h1.x, h1.y}, orsrc, ooff, 0, 0);
                }
            }
        }
        // the next X tile has landed: behind its last DMA instruction this wave issued the stores of rows 2 .. 7 (all 8 rows where the DMA went
        // out at the top of the tile) -- at least; anything hipcc adds only makes the wait stricter
        {
            constexpr int NTAIL = (DS ? BT_H : BT_H - 2) * (OLO ? 2 : 1);
            if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NTAIL) : "memory");
        }
        __syncthreads();                                       // B3: ... for every wave; t2 (and, DS, this X tile) is read
    }
}

int device_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

template <int CIN, bool DS, bool T1LO, bool XLO, bool OLO>
int launch_bn(const BnArgs& a, int nimg, hipStream_t s) {
    typedef BnLayout<CIN, DS, T1LO> L;
    AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bottleneck<CIN, DS, T1LO, XLO, OLO>), hipFuncAttributeMaxDynamicSharedMemorySize, L::LDS));
    const int grid = a.ntiles < device_cus() ? a.ntiles : device_cus();
    hipLaunchKernelGGL((k_bottleneck<CIN, DS, T1LO, XLO, OLO>), dim3(grid, 1, nimg), dim3(512), L::LDS, s, a);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// ======================================================================================================== layer2's identity blocks
// The same block at width 256, 512 -> 512 channels (ResNeXt-50 32x4d layer2.1 .. 2.3, 135 x 240 pixels at 1080p), trunk in and out in
// the MX form the MX GEMMs use (hi f16 plane + the bundle: FP4 copies of hi and lo with E8M0 scales, the lo part ONLY as FP4).
//   tile    4 x 16 output pixels (510 tiles at 1080p: two per CU), halo 6 x 18 = 108 pixels padded to 128 DMA rows / 112 MFMA rows.
//   X       does not fit beside t1 at 512 channels: it streams through a ring of three 64-channel slabs (LDS-DMA, 16 KB each), slab
//           s + 2 is requested while slab s is multiplied.  conv1's weights (hi + lo, 1 KB fragments) come from L2 per slab, one slab
//           ahead: 512 KB per tile, conv2's 160 KB, conv3's 512 KB -- 1.2 MB of L2 reads per 64 output pixels (the X tile: 128 KB).
//   conv1   wave w owns t1 channels 32 w .. 32 w + 31 (two 16-channel windows) for all 7 row tiles: 14 accumulators; Wh.xh + Wl.xh.
//   t1      [112 px][256 ch] f16 (512-byte rows, 16-byte chunks XOR-swizzled with px & 15), zero outside the image.
//   conv2   block-diagonal 16-channel windows as in layer1 (the wave's own two windows: no barrier after conv1); t2 hi in place over
//           t1, t2 lo in a plane of its own.
//   conv3   wave w owns output channels 64 w .. 64 w + 63: four n-tiles whose rows are permuted so that a lane holds 16 consecutive
//           channels of one pixel -- with its partner lane ^ 16 exactly one MX block, quantised as mx_epilogue does.  Wh.th + Wl.th +
//           Wh.tl; the residual (hi plane + FP4 lo part) comes from L2.
// Nothing waits on a hand-counted vmcnt across the epilogue's stores (the top of a tile drains to vmcnt(0)): pixels outside the image store nothing.
constexpr int B2_TH = 4, B2_TW = 16;
constexpr int B2_HW = B2_TW + 2, B2_HH = B2_TH + 2;
constexpr int B2_HALO = B2_HW * B2_HH;              // 108 pixels
constexpr int B2_M1 = 7;                            // conv1 row tiles
constexpr int B2_CIN = 512, B2_WIDTH = 256, B2_COUT = 512;
constexpr int B2_NSLAB = B2_CIN / 64;
constexpr int B2_SLAB = 128 * 128;                  // one 64-channel slab: 128 DMA rows x 128 B
constexpr int B2_RING = 3 * B2_SLAB;
constexpr int B2_T1 = B2_RING;                      // t1 (and t2 hi in place): 112 x 512 B
constexpr int B2_T2LO = B2_T1 + 112 * 512;          // t2 lo: 64 x 512 B
constexpr int B2_FLAG = B2_T2LO + 64 * 512;        // one word: "t1 overflowed f16" in this tile
constexpr int B2_LDS = B2_FLAG + 16;
static_assert(B2_LDS <= 160 * 1024, "layer2 bottleneck tile does not fit the LDS");

struct Bn2Args {
    const f16* x;            // block input hi plane [rows][in_ld]
    const char* xq;          // its bundle: the FP4 lo part + scales are read (residual)
    f16* out;                // output hi plane [rows][out_ld]
    char* oq;                // output bundle (Q4(hi), scales, Q4(lo), scales)
    const f16* w1;           // [n 16][ks 16][hi, lo][lane 64][8]
    const f16* w2;           // [window 16][ks 5][hi, lo][lane 64][8]
    const f16* w3;           // [wave 8][ks 8][nj 4][hi, lo][lane 64][8]
    const float* b;          // [b1 256 | b2 256 | b3 512] (one pointer: SGPRs)
    int H, W, in_ld, out_ld;
    int tiles_x, ntiles;
    int in_rows, out_rows;   // rows of the planes / bundles (the scale arrays are [K/256][rows][8])
};

__global__ void __launch_bounds__(512) k_bottleneck_w256(Bn2Args p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    const unsigned lds0 = lds_addr(lds);
    char* const T1 = lds + B2_T1;
    char* const T2L = lds + B2_T2LO;
    const int ipix = p.H * p.W;
    const int row0 = (int)blockIdx.z * ipix;      // the image's first row in every plane and bundle

    int bid = blockIdx.x;
    {   // XCD-aware bijective remap, as in k_bottleneck
        const int nwg = gridDim.x, xcd = bid & 7, local = bid >> 3, qq = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + local;
    }

    // slab s of a tile's X: two wave-instructions per wave (16 x 8 DMA rows; rows >= 108 read a clamped pixel and are never used)
    auto stage = [&](int tile, int s) __attribute__((always_inline)) {
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        int lo_ = lane;
        asm volatile("" : "+v"(lo_));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gi = wave + 8 * j;
            const int pix = gi * 8 + (lo_ >> 3);
            const int hy = min(pix / B2_HW, B2_HH - 1), hx = pix - (pix / B2_HW) * B2_HW;
            const int iy = min(max(ty * B2_TH - 1 + hy, 0), p.H - 1), ix = min(max(tx * B2_TW - 1 + hx, 0), p.W - 1);
            const unsigned voff = ((unsigned)(row0 + iy * p.W + ix) * (unsigned)p.in_ld + (unsigned)(s * 64) + (unsigned)(((lo_ & 7) ^ (pix & 7)) << 3)) * 2u;
            glds16_saddr(p.x, voff, lds0 + (s % 3) * B2_SLAB + gi * 1024);
        }
    };

    const __amdgpu_buffer_rsrc_t w1r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.w1)) + (size_t)wave * (2 * 16 * 2 * 1024), 0, 2 * 16 * 2 * 1024, 0x00020000);
    const __amdgpu_buffer_rsrc_t w3r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.w3)) + (size_t)wave * (8 * 4 * 2 * 1024), 0, 8 * 4 * 2 * 1024, 0x00020000);
    const int wlane = lane * 16;
    // (the fragment offset goes to the VGPR offset, not the scalar one: sixty-odd distinct scalar constants spill SGPRs)
    auto wfrag = [&](__amdgpu_buffer_rsrc_t r, int frag) __attribute__((always_inline)) {
        return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r, wlane + frag * 1024, 0, 0));
    };
    // conv1 weights of slab s: [nt 2][kk 2][hi, lo]; the wave's n-tiles 2 w, 2 w + 1 are contiguous in the pack
    auto load_w1 = [&](int s, f16x8 (&wf)[2][2][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int hl = 0; hl < 2; ++hl) wf[nt][kk][hl] = wfrag(w1r, (nt * 16 + 2 * s + kk) * 2 + hl);
    };

    const unsigned x_rd = (unsigned)(c * 128) + (unsigned)((q ^ (c & 7)) << 4);
    const int ch0 = 64 * wave + 16 * q;                    // conv3: this lane's 16 output channels

    int tile = bid;
    volatile int* const ovf = reinterpret_cast<volatile int*>(lds + B2_FLAG);
    f16x8 w1f[2][2][2][2];                                 // [slab parity][nt][kk][hi, lo]
    if (tile < p.ntiles) { stage(tile, 0); stage(tile, 1); load_w1(0, w1f[0]); }

    for (; tile < p.ntiles; tile += gridDim.x) {
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        int co = c, qo = q;
        asm volatile("" : "+v"(co), "+v"(qo));
        const bool more = tile + (int)gridDim.x < p.ntiles;

        // ================================================= conv1: slabs outside, row tiles inside
        f32x4 acc1[B2_M1][2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float4 b = *reinterpret_cast<const float4*>(p.b + 16 * (2 * wave + nt) + 4 * qo);
#pragma unroll
            for (int m = 0; m < B2_M1; ++m) acc1[m][nt] = f32x4{b.x, b.y, b.z, b.w};
        }
        f16x8 w2f[2][5][2];
#pragma unroll
        for (int s = 0; s < B2_NSLAB; ++s) {
            // slab s and its weights have landed (younger than the weights: slab s + 1's two DMA instructions)
            if (s == 0 || s + 1 >= B2_NSLAB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            __syncthreads();                           // ... for every wave; every wave is done with slab s - 1 (its ring slot is free)
            if (s == 0 && tid == 0) *ovf = 0;          // (every wave is past the last tile's epilogue; the word is set after the last slab)
            if (s + 1 < B2_NSLAB) load_w1(s + 1, w1f[(s + 1) & 1]);
            else {
                // (conv2's weights: plain loads -- one more buffer resource held across the tile loop spills SGPRs)
                const f16x8* w2p = reinterpret_cast<const f16x8*>(p.w2 + (size_t)wave * (2 * 5 * 2 * 512)) + (co + 16 * qo);   // (opaque lane id: hoisted, the pointer spills)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int k2 = 0; k2 < 5; ++k2) { w2f[j][k2][0] = w2p[(j * 5 + k2) * 128]; w2f[j][k2][1] = w2p[(j * 5 + k2) * 128 + 64]; }
            }
            if (s + 2 < B2_NSLAB) stage(tile, s + 2);
            const char* X = lds + (s % 3) * B2_SLAB;
            f16x8 xf[2][2];
            auto read_x = [&](int m, f16x8 (&f)[2]) __attribute__((always_inline)) {
                f[0] = *reinterpret_cast<const f16x8*>(X + x_rd + m * 2048);
                f[1] = *reinterpret_cast<const f16x8*>(X + (x_rd ^ 64u) + m * 2048);
            };
            read_x(0, xf[0]);
#pragma unroll
            for (int m = 0; m < B2_M1; ++m) {
                if (m + 1 < B2_M1) read_x(m + 1, xf[(m + 1) & 1]);
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc1[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1f[s & 1][nt][kk][0], xf[m & 1][kk], acc1[m][nt], 0, 0, 0);
                        acc1[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1f[s & 1][nt][kk][1], xf[m & 1][kk], acc1[m][nt], 0, 0, 0);
                    }
            }
        }
        // t1 = ReLU(conv1 + b1), zero outside the image and on the padding rows.  A conv1 result beyond f16's range never reaches
        // memory here: the tile's output is made +Inf instead, so that the plan's non-finite screen sees the block that overflowed.
        unsigned hmax = 0u;                                // largest stored f16 bit pattern (non-negative: >= 0x7c00 is Inf)
#pragma unroll
        for (int m = 0; m < B2_M1; ++m) {
            const int h = m * 16 + co;
            const int hy = h / B2_HW, hx = h - hy * B2_HW;
            const int iy = ty * B2_TH - 1 + hy, ix = tx * B2_TW - 1 + hx;
            const bool valid = ((unsigned)(h < B2_HALO) & (unsigned)((unsigned)iy < (unsigned)p.H) & (unsigned)((unsigned)ix < (unsigned)p.W)) != 0u;
            const unsigned vm = valid ? 0xffffffffu : 0u;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int n = 2 * wave + nt;
                const uint2 hi = relu_pack4(acc1[m][nt]);
                hmax = max(hmax, max(max((hi.x & vm) & 0xffffu, (hi.x & vm) >> 16), max((hi.y & vm) & 0xffffu, (hi.y & vm) >> 16)));
                const unsigned off = (unsigned)(h * 512) + (unsigned)((((2 * n) | (qo >> 1)) ^ co) << 4) + (unsigned)((qo & 1) * 8);
                *reinterpret_cast<uint2*>(T1 + off) = make_uint2(hi.x & vm, hi.y & vm);
            }
        }
        // ================================================= conv2: the wave's two windows, output row by output row; t2 hi in place
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = 2 * wave + j;
            const float4 bias2 = *reinterpret_cast<const float4*>(p.b + B2_WIDTH + 16 * n + 4 * qo);
            const unsigned cw16 = (unsigned)(((2 * n) | (qo & 1)) << 4);
#pragma unroll
            for (int r = 0; r < B2_TH; ++r) {
                f32x4 acc = f32x4{bias2.x, bias2.y, bias2.z, bias2.w};
                f16x8 th[5];
#pragma unroll
                for (int ks = 0; ks < 5; ++ks) {
                    const int t = min(2 * ks + (qo >> 1), 8);
                    const unsigned h = (unsigned)((r + t / 3) * B2_HW + (t % 3) + co);
                    th[ks] = *reinterpret_cast<const f16x8*>(T1 + (h << 9) + (cw16 ^ ((h & 15u) << 4)));
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 5; ++ks) {
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2f[j][ks][0], th[ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2f[j][ks][1], th[ks], acc, 0, 0, 0);
                }
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = relu_f32(acc[k]);
                uint2 hi, lo;
                split4(v, hi, lo);
                const unsigned px = (unsigned)(r * 16 + co);
                const unsigned off = (px << 9) + (unsigned)((((2 * n) | (qo >> 1)) ^ co) << 4) + (unsigned)((qo & 1) * 8);
                *reinterpret_cast<uint2*>(T1 + off) = hi;
                *reinterpret_cast<uint2*>(T2L + off) = lo;
            }
        }
        if (hmax >= 0x7c00u) *ovf = 1;
        __syncthreads();                                   // B2: t2 visible; the ring is free; the overflow word is final

        // the next tile's first two slabs, beside conv3
        if (more) { stage(tile + gridDim.x, 0); stage(tile + gridDim.x, 1); }

        // ================================================= conv3 + residual: K steps outside, the 4 output rows inside
        f32x4 acc3[B2_TH][4];
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) {
            const float4 b = *reinterpret_cast<const float4*>(p.b + 2 * B2_WIDTH + ch0 + 4 * nj);
#pragma unroll
            for (int r = 0; r < B2_TH; ++r) acc3[r][nj] = f32x4{b.x, b.y, b.z, b.w};
        }
        f16x8 w3f[2][4][2];
        auto load_w3 = [&](int ks, f16x8 (&wf)[4][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) { wf[nj][0] = wfrag(w3r, (ks * 4 + nj) * 2); wf[nj][1] = wfrag(w3r, (ks * 4 + nj) * 2 + 1); }
        };
        uint4 resh[B2_TH][2];
        uint2 resq[B2_TH];
        unsigned ress[B2_TH];
        // the identity at the tile's own pixels in accumulator layout (hi plane + FP4 lo part: L2 hits, the tile was staged from there)
        auto load_res = [&]() __attribute__((always_inline)) {
            const long long P = (long long)p.in_rows * (B2_CIN / 2), S = (long long)(B2_CIN / 256) * p.in_rows * 8;
            const char* const rq = p.xq + P + S;
            const unsigned char* const rs = reinterpret_cast<const unsigned char*>(p.xq + 2 * P + S);
#pragma unroll
            for (int r = 0; r < B2_TH; ++r) {
                const unsigned grow = (unsigned)(row0 + min(ty * B2_TH + r, p.H - 1) * p.W + min(tx * B2_TW + co, p.W - 1));
                resh[r][0] = *reinterpret_cast<const uint4*>(p.x + (grow * (unsigned)p.in_ld + (unsigned)ch0));
                resh[r][1] = *reinterpret_cast<const uint4*>(p.x + (grow * (unsigned)p.in_ld + (unsigned)ch0 + 8u));
                resq[r] = *reinterpret_cast<const uint2*>(rq + (grow * (unsigned)(B2_CIN / 2) + (unsigned)(ch0 / 2)));
                ress[r] = rs[(unsigned)(ch0 >> 8) * (unsigned)p.in_rows * 8u + grow * 8u + (unsigned)((ch0 >> 5) & 7)];
            }
        };
        load_res();
        load_w3(0, w3f[0]);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks + 1 < 8) load_w3(ks + 1, w3f[(ks + 1) & 1]);
            f16x8 th[B2_TH], tl[B2_TH];
#pragma unroll
            for (int r = 0; r < B2_TH; ++r) {
                const unsigned off = (unsigned)((r * 16 + co) << 9) + (unsigned)((((4 * ks) + qo) ^ co) << 4);
                th[r] = *reinterpret_cast<const f16x8*>(T1 + off);
                tl[r] = *reinterpret_cast<const f16x8*>(T2L + off);
            }
#pragma unroll
            for (int r = 0; r < B2_TH; ++r)
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) {
                    acc3[r][nj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks & 1][nj][0], th[r], acc3[r][nj], 0, 0, 0);
                    acc3[r][nj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks & 1][nj][1], th[r], acc3[r][nj], 0, 0, 0);
                    acc3[r][nj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3f[ks & 1][nj][0], tl[r], acc3[r][nj], 0, 0, 0);
                }
        }
        // the next tile's first conv1 weights: conv3's weight registers are free
        if (more) load_w1(0, w1f[0]);

        // ---- epilogue: + identity, ReLU, hi plane, FP4 copies of hi and lo + their scales
        const unsigned OP = (unsigned)p.out_rows * (B2_COUT / 2), OS = (unsigned)(B2_COUT / 256) * (unsigned)p.out_rows * 8u;
#pragma unroll
        for (int r = 0; r < B2_TH; ++r) {
            const int oy = ty * B2_TH + r, ox = tx * B2_TW + co;
            const bool live = ((unsigned)(oy < p.H) & (unsigned)(ox < p.W)) != 0u;
            const unsigned grow = (unsigned)(row0 + min(oy, p.H - 1) * p.W + min(ox, p.W - 1));
            const uint4 rh0 = resh[r][0], rh1 = resh[r][1];
            const uint2 pk = resq[r];
            const unsigned sb = ress[r];
            float v[16];
#pragma unroll
            for (int nj = 0; nj < 4; ++nj)
#pragma unroll
                for (int k = 0; k < 4; ++k) v[nj * 4 + k] = acc3[r][nj][k];
            {
                const f16x8 h0 = __builtin_bit_cast(f16x8, rh0), h1 = __builtin_bit_cast(f16x8, rh1);
                float rl[16];
                typedef float v2f __attribute__((ext_vector_type(2)));
                const float sc = __uint_as_float(sb << 23);
#define AVL_FP4_DEC(w, sel, o) { const v2f d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, sel); rl[o] = d.x; rl[o + 1] = d.y; }
                AVL_FP4_DEC(pk.x, 0, 0) AVL_FP4_DEC(pk.x, 1, 2) AVL_FP4_DEC(pk.x, 2, 4) AVL_FP4_DEC(pk.x, 3, 6)
                AVL_FP4_DEC(pk.y, 0, 8) AVL_FP4_DEC(pk.y, 1, 10) AVL_FP4_DEC(pk.y, 2, 12) AVL_FP4_DEC(pk.y, 3, 14)
#undef AVL_FP4_DEC
                // hi + lo first (exact in fp32), then the accumulator: the order of mx_epilogue
#pragma unroll
                for (int i = 0; i < 8; ++i) { v[i] += (float)h0[i] + rl[i]; v[8 + i] += (float)h1[i] + rl[8 + i]; }
            }
            float hi[16], lo[16];
            unsigned hp[8];
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const float a = relu_f32(v[i]), b = relu_f32(v[i + 1]);
                const h2v hh = {(f16)a, (f16)b};
                hp[i / 2] = __builtin_bit_cast(unsigned, hh);
                hi[i] = (float)hh[0]; hi[i + 1] = (float)hh[1];
                lo[i] = a - hi[i]; lo[i + 1] = b - hi[i + 1];
            }
            unsigned q0[2], q1[2];
            const unsigned s0 = quantize_fp4_block(hi, q0), s1 = quantize_fp4_block(lo, q1);
            // t1 overflowed f16 somewhere in the tile: the hi plane's f16 exponents all set -- the whole tile's output is non-finite
            // (the word is final since B2; read here, where it costs no register across conv3)
            const unsigned ovm = *ovf != 0 ? 0x7c007c00u : 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) hp[k] |= ovm;
            if (live) {
                *reinterpret_cast<uint4*>(p.out + (grow * (unsigned)p.out_ld + (unsigned)ch0)) = make_uint4(hp[0], hp[1], hp[2], hp[3]);
                *reinterpret_cast<uint4*>(p.out + (grow * (unsigned)p.out_ld + (unsigned)ch0 + 8u)) = make_uint4(hp[4], hp[5], hp[6], hp[7]);
                const unsigned qoff = grow * (unsigned)(B2_COUT / 2) + (unsigned)(ch0 / 2);
                *reinterpret_cast<uint2*>(p.oq + qoff) = make_uint2(q0[0], q0[1]);
                *reinterpret_cast<uint2*>(p.oq + (qoff + OP + OS)) = make_uint2(q1[0], q1[1]);
                if ((qo & 1) == 0) {         // one scale byte per 32-channel block: the even lane of the pair stores it
                    const unsigned soff = (unsigned)(ch0 >> 8) * (unsigned)p.out_rows * 8u + grow * 8u + (unsigned)((ch0 >> 5) & 7);
                    p.oq[OP + soff] = (char)s0;
                    p.oq[2u * OP + OS + soff] = (char)s1;
                }
            }
        }
    }
}

int launch_bn2(const Bn2Args& a, int nimg, hipStream_t s) {
    AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bottleneck_w256), hipFuncAttributeMaxDynamicSharedMemorySize, B2_LDS));
    const int grid = a.ntiles < device_cus() ? a.ntiles : device_cus();
    hipLaunchKernelGGL(k_bottleneck_w256, dim3(grid, 1, nimg), dim3(512), B2_LDS, s, a);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

}  // namespace

// AVL_OP_BOTTLENECK (include/avl_hip.h): in_c = 64 (with the downsample 1x1 folded into conv3: w_layout = 1) or 256 (identity
// residual: w_layout = 0); w_split = 1: t1 keeps a lo plane too (in_c = 64 only: the LDS has no room for it at 256).
// in_c = 512 (layer2's identity blocks): width 256 -> 512 output channels, trunk in and out in the MX form: in + in_mx (its lo part only
// as FP4: in_lo NULL, mx_flags AVL_MX_IN_LO), out + out_mx with both halves (out_lo NULL, mx_flags AVL_MX_OUT_LO); w_layout = w_split = 0.
static int validate_bottleneck_w256(const avl_seg_op& op) {
    AVL_REQUIRE(op.out_c == B2_COUT && op.in3_c == B2_WIDTH && op.w_layout == 0 && op.w_split == 0,
                "fused bottleneck (512 channels): width %d -> %d output channels, identity residual (got %d -> %d)", B2_WIDTH, B2_COUT, op.in3_c, op.out_c);
    AVL_REQUIRE(op.in_mx && op.out_mx && !op.in_lo && !op.out_lo && op.mx_flags == (AVL_MX_IN_LO | AVL_MX_OUT_LO),
                "fused bottleneck (512 channels): MX trunk in and out (in_mx, out_mx, mx_flags AVL_MX_IN_LO | AVL_MX_OUT_LO, no f16 lo planes)");
    AVL_REQUIRE(op.in_ld == B2_CIN && op.out_ld == B2_COUT, "fused bottleneck (512 channels): dense rows (the bundles have no row stride)");
    AVL_REQUIRE((long long)op.in_rows >= (long long)op.in_h * op.in_w * op_batch(op) && (long long)op.out_rows >= (long long)op.out_h * op.out_w * op_batch(op),
                "fused bottleneck: rows allocated");
    AVL_REQUIRE((long long)op.in_rows * op.in_ld * 2 < (1LL << 31) && (long long)op.out_rows * op.out_ld * 2 < (1LL << 31), "fused bottleneck: planes beyond 2 GB (32-bit offsets)");
    AVL_REQUIRE(op.in && op.out && op.weight && op.in2 && op.in3 && op.bias, "fused bottleneck: in, out, weight (conv1), in2 (conv2 weights), in3 (conv3 weights), bias");
    AVL_REQUIRE(((reinterpret_cast<uintptr_t>(op.in) | reinterpret_cast<uintptr_t>(op.out) | reinterpret_cast<uintptr_t>(op.in_mx) | reinterpret_cast<uintptr_t>(op.out_mx) |
                  reinterpret_cast<uintptr_t>(op.weight) | reinterpret_cast<uintptr_t>(op.in2) | reinterpret_cast<uintptr_t>(op.in3) | reinterpret_cast<uintptr_t>(op.bias)) & 15) == 0,
                "fused bottleneck: 16-byte aligned buffers");
    AVL_REQUIRE(op.in != op.out && op.in_mx != op.out_mx, "fused bottleneck: not in place (tiles read their neighbours' pixels)");
    return AVL_OK;
}

int validate_bottleneck(const avl_seg_op& op) {
    AVL_REQUIRE(op.dtype == AVL_F16, "fused bottleneck: AVL_F16 activations only");
    AVL_REQUIRE(op.groups == 32 && op.ksize == 3 && op.stride == 1 && op.dil == 1 && op.pad == 1, "fused bottleneck: 3x3, 32 groups, stride 1, dilation 1");
    AVL_REQUIRE(op.in_h == op.out_h && op.in_w == op.out_w && op.in_h > 0 && op.in_w > 0, "fused bottleneck: same-size output");
    if (op.in_c == B2_CIN) return validate_bottleneck_w256(op);
    AVL_REQUIRE(op.out_c == BN_COUT && op.in3_c == BN_WIDTH, "fused bottleneck: width %d -> %d output channels only (got %d -> %d)", BN_WIDTH, BN_COUT, op.in3_c, op.out_c);
    AVL_REQUIRE((op.in_c == 64 && op.w_layout == 1) || (op.in_c == 256 && op.w_layout == 0 && op.w_split == 0),
                "fused bottleneck: 64 input channels with the downsample folded in, or 256 with the identity residual and no t1 lo plane");
    AVL_REQUIRE(op.in_h == op.out_h && op.in_w == op.out_w && op.in_h > 0 && op.in_w > 0, "fused bottleneck: same-size output");
    AVL_REQUIRE(op.in_ld >= op.in_c && op.in_ld % 8 == 0 && op.out_ld >= op.out_c && op.out_ld % 8 == 0, "fused bottleneck: row strides");
    AVL_REQUIRE((long long)op.in_rows >= (long long)op.in_h * op.in_w * op_batch(op) && (long long)op.out_rows >= (long long)op.out_h * op.out_w * op_batch(op),
                "fused bottleneck: rows allocated");
    AVL_REQUIRE((long long)op.in_rows * op.in_ld * 2 < (1LL << 31) && (long long)op.out_rows * op.out_ld * 2 < (1LL << 31), "fused bottleneck: planes beyond 2 GB (32-bit offsets)");
    AVL_REQUIRE(op.in && op.out && op.weight && op.in2 && op.in3 && op.bias, "fused bottleneck: in, out, weight (conv1), in2 (conv2 weights), in3 (conv3 weights), bias");
    AVL_REQUIRE(((reinterpret_cast<uintptr_t>(op.in) | reinterpret_cast<uintptr_t>(op.in_lo) | reinterpret_cast<uintptr_t>(op.out) | reinterpret_cast<uintptr_t>(op.out_lo) |
                  reinterpret_cast<uintptr_t>(op.weight) | reinterpret_cast<uintptr_t>(op.in2) | reinterpret_cast<uintptr_t>(op.in3) | reinterpret_cast<uintptr_t>(op.bias)) & 15) == 0,
                "fused bottleneck: 16-byte aligned buffers");
    AVL_REQUIRE(!(op.in_c == 64 && op.in_lo), "fused bottleneck: the 64-channel variant takes a single-plane input");
    AVL_REQUIRE(op.in != op.out && op.in != op.out_lo, "fused bottleneck: not in place (tiles read their neighbours' pixels)");
    return AVL_OK;
}

int launch_bottleneck(const avl_seg_op& op, hipStream_t s) {
    if (op.in_c == B2_CIN) {
        Bn2Args a;
        a.x = static_cast<const f16*>(op.in);
        a.xq = static_cast<const char*>(op.in_mx);
        a.out = static_cast<f16*>(op.out);
        a.oq = static_cast<char*>(op.out_mx);
        a.w1 = static_cast<const f16*>(op.weight);
        a.w2 = static_cast<const f16*>(op.in2);
        a.w3 = static_cast<const f16*>(op.in3);
        a.b = op.bias;
        a.H = op.in_h; a.W = op.in_w; a.in_ld = op.in_ld; a.out_ld = op.out_ld;
        a.tiles_x = (op.in_w + B2_TW - 1) / B2_TW;
        a.ntiles = a.tiles_x * ((op.in_h + B2_TH - 1) / B2_TH);
        a.in_rows = op.in_rows; a.out_rows = op.out_rows;
        return launch_bn2(a, op_batch(op), s);
    }
    BnArgs a;
    a.x = static_cast<const f16*>(op.in);
    a.x_lo = static_cast<const f16*>(op.in_lo);
    a.out = static_cast<f16*>(op.out);
    a.out_lo = static_cast<f16*>(op.out_lo);
    a.w1 = static_cast<const f16*>(op.weight);
    a.w2 = static_cast<const f16*>(op.in2);
    a.w3 = static_cast<const f16*>(op.in3);
    a.b1 = op.bias; a.b2 = op.bias + BN_WIDTH; a.b3 = op.bias + 2 * BN_WIDTH;
    a.H = op.in_h; a.W = op.in_w; a.in_ld = op.in_ld; a.out_ld = op.out_ld;
    a.tiles_x = (op.in_w + BT_W - 1) / BT_W;
    a.ntiles = a.tiles_x * ((op.in_h + BT_H - 1) / BT_H);
    a.out_bytes = (int)((long long)op.out_rows * op.out_ld * 2);
    const int variant = (op.in_c == 64 ? 4 + 2 * (op.w_split ? 1 : 0) : 2 * (a.x_lo ? 1 : 0)) + (a.out_lo ? 1 : 0);
    switch (variant) {
        case 0: return launch_bn<256, false, false, false, false>(a, op_batch(op), s);
        case 1: return launch_bn<256, false, false, false, true>(a, op_batch(op), s);
        case 2: return launch_bn<256, false, false, true, false>(a, op_batch(op), s);
        case 3: return launch_bn<256, false, false, true, true>(a, op_batch(op), s);
        case 4: return launch_bn<64, true, false, false, false>(a, op_batch(op), s);
        case 5: return launch_bn<64, true, false, false, true>(a, op_batch(op), s);
        case 6: return launch_bn<64, true, true, false, false>(a, op_batch(op), s);
        default: return launch_bn<64, true, true, false, true>(a, op_batch(op), s);
    }
}

}  // namespace avl
