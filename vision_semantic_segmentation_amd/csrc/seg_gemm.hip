// 1x1 convolution = GEMM on the matrix cores (gfx950).
//
//   out[m][n] = act( sum_k in[m][k] * w[n][k] + bias[n] (+ res[m][n]) )
//
// in  : NHWC activations, one row per pixel (row stride lda), K = input channels contiguous
// w   : [n][k] (PyTorch's [Cout][Cin] with BatchNorm folded in), K contiguous
// 94 % of the network's MACs run here, so this is the MFMA-bound kernel.
//
// Structure (one workgroup = WM x WN waves, each wave a 64 x 64 output tile, BK = 128 bytes of K):
//   * both operand tiles go HBM/L2 -> LDS with global_load_lds_dwordx4 (no VGPR staging), two LDS
//     buffers, the load of K-step t+1 in flight while step t is multiplied; one barrier per step;
//   * LDS rows are 128 B; the 16-byte chunk index is XOR-ed with (row & 7).  The DMA writes LDS
//     linearly, so the swizzle is applied to the per-lane SOURCE address and again on the read;
//   * the product is computed transposed (D^T = W . in^T): the MFMA "A" operand is the weight
//     fragment, "B" the activation fragment, so a lane ends up holding 16 CONSECUTIVE channels of one
//     pixel (weight rows are permuted inside the 64-wide wave tile to make that so) and the NHWC
//     store / residual load are 32-byte (bf16) or 64-byte (fp32) contiguous per lane;
//   * workgroup ids are remapped so that the tiles sharing an activation panel run on one XCD (L2).
//   * T = bf16 : v_mfma_f32_16x16x32_bf16, fp32 accumulate.
//     T = float: v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain) -- the reference-precision mode.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "seg_types.h"

namespace avl {
namespace {

struct GemmArgs {
    const void* A;
    const void* W;
    const float* bias;
    const void* R;
    void* C;
    int lda, ldr, ldc;
    int M, N, K;
    int relu, out_f32;
    int ntiles;
    // "mixed" precision (f16): nsub = MFMA passes per 64-wide K block.  1: plain.  2: weights split (hi, lo), A used twice.
    // 3: A split as well: (A hi, W hi), (A hi, W lo), (A lo, W hi); a_lo_delta = byte distance from A's hi plane to its lo plane.
    // W rows are K * nsub long and already interleaved in that order by the host.  R_lo / C_lo: low planes of the
    // residual / of the output (NULL = single plane).
    int nsub;
    long long a_lo_delta;
    const void* R_lo;
    void* C_lo;
    // k_gemm with out_f32 and N <= 32 (the classifier) has no low plane: C_lo is then the uint8 label map, torch.argmax over the row's N
    // values (semantic_segmentation.py:56: first maximal index wins, a NaN counts as maximal) written as one byte per row from the very
    // values stored as logits; NULL = not wanted.  (Not a field of its own: MxArgs embeds this struct and k_gemm_mx_pipe keeps every
    // kernel argument in SGPRs.)
};

// What k_gemm_ring<..., EXT = true> takes beside GemmArgs (not fields of GemmArgs: MxArgs embeds that struct, and the MX kernels keep
// their argument layout).  Both parts are optional at run time.
struct RingExt {
    // pixel map of the A rows (s = 0: none): row m of the product = pixel (oy * s, ox * s) of image m / ohw, (oy, ox) = its place in the
    // ow-wide output image; w, hw = input image width and pixel count.  A stride-s 1x1 conv without the sub-sampled copy of its input.
    int s, ow, ohw, w, hw;
    // second destination (C2 = NULL: none): tiles whose first column is >= n_split write C2 (+ C2_lo) with row stride ldc2, column
    // n_split landing at C2's first.  n_split is a multiple of BN, so a tile has one destination.
    int n_split, ldc2;
    void* C2;
    void* C2_lo;
};

// which sub-steps of a K block bring a NEW activation tile (the others reuse the tile already in LDS)
template <int NSUB> __device__ __forceinline__ bool sub_needs_a(int j) { return NSUB == 1 || j == 0 || (NSUB == 3 && j == 2); }

__device__ __forceinline__ void glds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

template <typename T, int WM, int WN>
__global__ void __launch_bounds__(WM* WN * 64) k_gemm(GemmArgs p) {
    constexpr int NW = WM * WN, BM = WM * 64, BN = WN * 64;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128, BUF = A_BYTES + W_BYTES;
    constexpr int A_INSTR = BM / 8 / NW, W_INSTR = BN / 8 / NW;
    static_assert(A_INSTR >= 1 && W_INSTR >= 1, "tile too small for the wave count");
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware, bijective remap: workgroups b and b+8 share an XCD (and its L2); give each XCD a
    // contiguous run of logical tiles so the WN.. tiles of one activation panel hit the same L2.
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, xcd = bid & 7, local = bid >> 3, q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    const int nt = bid % p.ntiles, mt = bid / p.ntiles;
    const int m0 = mt * BM, n0 = nt * BN;

    // per-lane DMA sources: lane -> (row = lane>>3 of an 8-row group, physical chunk = lane&7)
    const char* a_src[A_INSTR];
    const char* w_src[W_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int r = (i * NW + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ (r & 7);
        a_src[i] = static_cast<const char*>(p.A) + (long long)(m0 + r) * p.lda * (int)sizeof(T) + c * 16;
    }
#pragma unroll
    for (int i = 0; i < W_INSTR; ++i) {
        const int r = (i * NW + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ (r & 7);
        w_src[i] = static_cast<const char*>(p.W) + (long long)(n0 + r) * p.K * p.nsub * (int)sizeof(T) + c * 16;
    }
    auto stage = [&](int buf, int kt) {
        char* base = lds + buf * BUF;
        const int kb = kt / p.nsub, j = kt - kb * p.nsub;                    // K block, pass inside it (see GemmArgs::nsub)
        const long long aoff = (long long)kb * 128 + (j == 2 ? p.a_lo_delta : 0);
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) glds16(a_src[i] + aoff, base + (i * NW + wave) * 1024);
#pragma unroll
        for (int i = 0; i < W_INSTR; ++i) glds16(w_src[i] + (long long)kt * 128, base + A_BYTES + (i * NW + wave) * 1024);
    };

    // fragment addresses (constant over the K loop)
    const int fr = lane & 15, kq = lane >> 4;
    int a_row[4], w_row[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) a_row[mi] = wm * 64 + mi * 16 + fr;
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) w_row[nj] = wn * 64 + (fr >> 2) * 16 + nj * 4 + (fr & 3);

    f32x4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K * (int)sizeof(T) / 128 * p.nsub;
    stage(0, 0);
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of tile kt has landed
        __syncthreads();                                     // everyone's has; buffer cur^1 is free again
        if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
        const char* ab = lds + cur * BUF;
        const char* wb = ab + A_BYTES;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int chunk = kk * 4 + kq;
                typedef typename Half16<T>::v8 v8;
                v8 af[4], wf[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    af[mi] = *reinterpret_cast<const v8*>(ab + a_row[mi] * 128 + ((chunk ^ (a_row[mi] & 7)) << 4));
#pragma unroll
                for (int nj = 0; nj < 4; ++nj)
                    wf[nj] = *reinterpret_cast<const v8*>(wb + w_row[nj] * 128 + ((chunk ^ (w_row[nj] & 7)) << 4));
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = Half16<T>::mfma(wf[nj], af[mi], acc[mi][nj]);
            }
        } else {
            // fp32: lane kq owns k = 8*kq .. 8*kq+7 of the 32-wide step; MFMA step s sums k-set {s, 8+s, 16+s, 24+s}
            f32x4 af[4][2], wf[4][2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int chunk = kq * 2 + h;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    af[mi][h] = *reinterpret_cast<const f32x4*>(ab + a_row[mi] * 128 + ((chunk ^ (a_row[mi] & 7)) << 4));
#pragma unroll
                for (int nj = 0; nj < 4; ++nj)
                    wf[nj][h] = *reinterpret_cast<const f32x4*>(wb + w_row[nj] * 128 + ((chunk ^ (w_row[nj] & 7)) << 4));
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 4; ++nj)
                        acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[nj][s >> 2][s & 3], af[mi][s >> 2][s & 3],
                                                                           acc[mi][nj], 0, 0, 0);
        }
        cur ^= 1;
    }

    // epilogue: lane = (pixel fr of each 16-pixel sub-tile, channel block kq): 16 consecutive channels
    const int nbase = n0 + wn * 64 + kq * 16;
    float bias[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 b = *reinterpret_cast<const float4*>(p.bias + nbase + 4 * j);
        bias[4 * j] = b.x; bias[4 * j + 1] = b.y; bias[4 * j + 2] = b.z; bias[4 * j + 3] = b.w;
    }
    unsigned char* const labels = p.out_f32 ? static_cast<unsigned char*>(p.C_lo) : nullptr;
    if (labels) {
        // the classifier's arg-max (N <= 32: channel blocks kq = 0 and 1 of a row sit 16 lanes apart), on the values stored below; every lane
        // takes part in the exchange, so this runs in front of the loop whose lanes drop out individually
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int m = m0 + wm * 64 + mi * 16 + fr;
            float best = acc[mi][0][0] + bias[0];
            int bi = nbase;
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                const float val = acc[mi][i >> 2][i & 3] + bias[i];
                if (nbase + i < p.N && (val > best || (val != val && best == best))) { best = val; bi = nbase + i; }
            }
            const float ob = __shfl_down(best, 16);
            const int oi = __shfl_down(bi, 16);
            if (nbase + 16 < p.N && (ob > best || (ob != ob && best == best))) { best = ob; bi = oi; }
            if (kq == 0 && m < p.M) labels[m] = (unsigned char)bi;
        }
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int m = m0 + wm * 64 + mi * 16 + fr;
        if (m >= p.M || nbase >= p.N) continue;
        float v[16];
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[nj * 4 + r] = acc[mi][nj][r] + bias[nj * 4 + r];
        const bool full = nbase + 16 <= p.N;
        if (p.R) {
            const T* rp = static_cast<const T*>(p.R) + (long long)m * p.ldr + nbase;
            if (full) {
                float r0[8], r1[8];
                Vec8<T>::load(rp, r0);
                Vec8<T>::load(rp + 8, r1);
#pragma unroll
                for (int i = 0; i < 8; ++i) { v[i] += r0[i]; v[8 + i] += r1[i]; }
            } else {
                for (int i = 0; i < 16; ++i)
                    if (nbase + i < p.N) v[i] += to_f32(rp[i]);
            }
        }
        if (p.relu) {
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        if (p.out_f32) {
            float* cp = static_cast<float*>(p.C) + (long long)m * p.ldc + nbase;
            for (int i = 0; i < 16; ++i)
                if (nbase + i < p.N) cp[i] = v[i];
        }
        if (!p.out_f32) {
            T* cp = static_cast<T*>(p.C) + (long long)m * p.ldc + nbase;
            if (full) {
                float lo[8], hi[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) { lo[i] = v[i]; hi[i] = v[8 + i]; }
                Vec8<T>::store(cp, lo);
                Vec8<T>::store(cp + 8, hi);
            } else {
                for (int i = 0; i < 16; ++i)
                    if (nbase + i < p.N) cp[i] = from_f32<T>(v[i]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// v2 (16-bit types): persistent workgroups, 256 x 128 or 256 x 256 tile (8 waves = 2 per SIMD), LDS ring.
//   * one workgroup per CU walks tiles t = vb, vb + grid, ...; the K-steps of all its tiles form one
//     stream, so the DMA for the NEXT tile's first steps is already in flight during the epilogue;
//   * the ring keeps STAGES - 1 steps ahead in flight: counted `s_waitcnt vmcnt(N)` + raw s_barrier
//     (a __syncthreads() would drain the LDS-DMA queue with vmcnt(0));
//   * weight-tile swizzle key is built from the row bits the permuted fragment rows actually vary in
//     (conflict-free ds_read_b128 for both operands).
//
// The vmcnt invariant: the only inline-asm memory operations are LDS-DMAs (no register outputs) and they
// retire in issue order.  At the top of step g the wave needs every DMA of steps <= g landed; the DMAs it may leave in
// flight are exactly those of step g+1 (STAGES = 3; none for STAGES = 2), so it waits for vmcnt(N) with N = the number
// of DMA instructions this wave issued for step g+1.  Compiler-visible loads/stores (bias in init_acc, the residual
// loads and the output stores of the epilogue) share the counter; they are all YOUNGER than step g+1's DMAs only when
// issued after them, and an s_waitcnt vmcnt(N) with extra younger operations outstanding merely waits for more than
// it needs (in-order retirement: "all but the N youngest" then still covers every DMA of steps <= g).  hipcc's own
// waits for those loads are vmcnt(0)-style and only over-wait as well.  So the count can over-wait, never under-wait.
//
// NSUB ("mixed" precision, f16): MFMA passes per 64-wide K block, see GemmArgs::nsub.  The activation ring and the weight
// ring advance independently: a sub-step always brings a weight tile, an activation tile only when it changes
// (sub_needs_a), so W hi/lo cost 1.5x the L2->LDS bytes of the plain GEMM for 2x the MFMAs.
// IO: the epilogue may read a split residual (R + R_lo) and write a split result (C + C_lo), both optional at run time.
// STAGES = weight tiles in the ring (the producer runs STAGES - 1 sub-steps ahead); AST = activation tiles in the ring:
// = STAGES for the plain GEMM; 2 is enough for NSUB = 2 at any depth because an activation tile lives for two sub-steps
// (256 x 256 tile: 2 x 32 KB + 3 x 32 KB = the whole 160 KB of LDS, two sub-steps of DMA in flight instead of one).
// EXT: the loader may read its rows through a pixel map and the epilogue may write a second destination (RingExt); the plain
// instantiations (EXT = false) never look at `x`.
template <typename H, int WM, int WN, int MI, int STAGES, int NSUB = 1, int IO = 0, int AST = STAGES, bool EXT = false>
__global__ void __launch_bounds__(WM* WN * 64) k_gemm_ring(GemmArgs p, int mtiles, RingExt x) {
    typedef typename Half16<H>::v8 v8;
    constexpr int NW = WM * WN, BM = WM * MI * 16, BN = WN * 64;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128;
    constexpr int W_REGION = AST * A_BYTES;                    // LDS: [AST activation tiles][STAGES weight tiles]
    static_assert(AST == STAGES || (NSUB == 2 && AST == 2), "activation ring too short for this pass pattern");
    constexpr int A_INSTR = BM / 8 / NW, W_INSTR = BN / 8 / NW;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int nwg = gridDim.x;
    int vb;
    {
        const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3, q = nwg >> 3, r = nwg & 7;
        vb = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    const int total = mtiles * p.ntiles;
    const int nkb = p.K / 64;                  // K blocks per tile; NSUB sub-steps each
    const unsigned lds_base = lds_addr(lds);

    // ---- producer side: per-lane DMA sources of the tile whose stages are being issued
    const int srow = lane >> 3, schunk = lane & 7;
    const char* a_src[A_INSTR];
    const char* w_src[W_INSTR];
    int pt = vb, pk = 0;                       // tile and K block being issued next
    int issued = 0, issued_a = 0;              // sub-steps / activation tiles issued so far (ring positions)
    auto set_tile = [&](int t) {
        const int nt = t % p.ntiles, mt = t / p.ntiles;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            const int r = (i * NW + wave) * 8 + srow;
            long long row = mt * BM + r;
            if constexpr (EXT) {
                if (x.s) {         // (rows at or past M, which the last tile reads and never stores, take row M - 1's pixel: inside the image)
                    const int m = min(mt * BM + r, p.M - 1), img = m / x.ohw, rem = m - img * x.ohw, oy = rem / x.ow, ox = rem - oy * x.ow;
                    row = (long long)img * x.hw + (long long)(oy * x.s) * x.w + ox * x.s;
                }
            }
            a_src[i] = static_cast<const char*>(p.A) + row * p.lda * 2 + ((schunk ^ (r & 7)) << 4);
        }
#pragma unroll
        for (int i = 0; i < W_INSTR; ++i) {
            const int r = (i * NW + wave) * 8 + srow;
            const int key = ((r >> 1) & 1) | (((r >> 4) & 3) << 1);
            w_src[i] = static_cast<const char*>(p.W) + (long long)(nt * BN + r) * p.K * (2 * NSUB) + ((schunk ^ key) << 4);
        }
    };
    // one sub-step = W_INSTR (+ A_INSTR when the activation tile changes) DMA instructions per wave; issue_part(h, NP, jj)
    // sends the h-th of NP equal shares of sub-step jj of K block pk (so the instructions can be spread between MFMA groups
    // instead of queueing up in front of them).  jj is wave-uniform: the producer runs STAGES - 1 sub-steps ahead of the consumer.
    auto issue_part = [&](int h, int np, int jj) {
        const bool na = sub_needs_a<NSUB>(jj);
        if (na) {
            const unsigned abase = lds_base + (issued_a % AST) * A_BYTES + wave * 1024;
            const long long aoff = (long long)pk * 128 + ((NSUB == 3 && jj == 2) ? p.a_lo_delta : 0);
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i)
                if (i * np / A_INSTR == h) glds16_asm(a_src[i] + aoff, abase + i * NW * 1024);
        }
        const unsigned wbase = lds_base + W_REGION + (issued % STAGES) * W_BYTES + wave * 1024;
        const long long woff = (long long)(pk * NSUB + jj) * 128;
#pragma unroll
        for (int i = 0; i < W_INSTR; ++i)
            if (i * np / W_INSTR == h) glds16_asm(w_src[i] + woff, wbase + i * NW * 1024);
        if (h == np - 1) {
            ++issued;
            if (na) ++issued_a;
            if (jj == NSUB - 1) {
                if (++pk == nkb) {
                    pk = 0;
                    pt += nwg;
                    if (pt < total) set_tile(pt);
                }
            }
        }
    };
    if (pt < total) set_tile(pt);
#pragma unroll
    for (int i = 0; i < STAGES - 1; ++i)
        if (pt < total) issue_part(0, 1, i % NSUB);

    // ---- consumer side
    const int fr = lane & 15, kq = lane >> 4;
    int a_off[MI], w_off[4], a_key[MI], w_key[4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int row = wm * (MI * 16) + mi * 16 + fr;
        a_off[mi] = row * 128;
        a_key[mi] = row & 7;
    }
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
        const int row = wn * 64 + (fr >> 2) * 16 + nj * 4 + (fr & 3);
        w_off[nj] = W_REGION + row * 128;
        w_key[nj] = ((row >> 1) & 1) | (((row >> 4) & 3) << 1);
    }
    // The accumulators start from the bias, so the epilogue issues no load whose result could still be
    // pending when the K loop resumes (hipcc would then put a vmcnt(0) in front of every K-step's ds_reads).
    f32x4 acc[MI][4];
    auto init_acc = [&](int t) {
        const int nb = (t % p.ntiles) * BN + wn * 64 + kq * 16;
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + nb + 4 * nj);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[mi][nj] = f32x4{b.x, b.y, b.z, b.w};
        }
    };
    if (vb < total) init_acc(vb);

    int g = 0;      // sub-steps consumed so far
    int ca = -1;    // activation tiles consumed so far - 1 = ring position of the current one
    for (int t = vb; t < total; t += nwg) {
        const int nt = t % p.ntiles, mt = t / p.ntiles;
        // one loop over the tile's sub-steps; j = sub-step inside the K block (a scalar: every branch on it is uniform)
        for (int q = 0, j = 0; q < nkb * NSUB; ++q, ++g, j = (NSUB == 1 || j + 1 == NSUB) ? 0 : j + 1) {
            if (sub_needs_a<NSUB>(j)) ++ca;
            const int jn = (j + STAGES - 1) % NSUB;           // the sub-step that is issued during this one
            // sub-step g has landed (this wave's share); sub-step g+1 may stay in flight
            if (STAGES >= 3 && issued > g + 1) {
                if (sub_needs_a<NSUB>((j + 1) % NSUB)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_INSTR + W_INSTR) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(W_INSTR) : "memory");
            } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const bool feed = pt < total;                  // sub-step g+STAGES-1 -> the slots consumed in step g-1
            const char* abase = lds + (ca % AST) * A_BYTES;
            const char* wbase = lds + (g % STAGES) * W_BYTES;
            auto rd_w = [&](int kk, int nj) { return *reinterpret_cast<const v8*>(wbase + w_off[nj] + (((kk * 4 + kq) ^ w_key[nj]) << 4)); };
            auto rd_a = [&](int kk, int mi) { return *reinterpret_cast<const v8*>(abase + a_off[mi] + (((kk * 4 + kq) ^ a_key[mi]) << 4)); };
            // The step is cut into 4 MFMA groups; the next stage's DMA instructions and the second K-half's fragment
            // reads are placed BETWEEN the groups (a DMA burst issued in one go in front of the MFMAs was measured to
            // serialise with them: DMA-only 75 us + MFMA-only 65 us = 131 us for layer4.conv1).
            constexpr int HALF = MI / 2;
            // Waves w and w + NW/2 share a SIMD.  The second half issues its DMA at the head of the step, the first
            // half in the middle, so that on every SIMD one wave is in an MFMA group while its partner pays the
            // (100+ cycle per instruction) LDS-DMA issue cost, instead of both doing the same thing at the same time.
            const bool early = MI == 8 && NW >= 8 && wave >= NW / 2;      // measured: +4-7 % on 256x256 tiles, -4 % on 256x128
            if (feed && early) { issue_part(0, 2, jn); issue_part(1, 2, jn); }
            v8 wa[4], wb[4], af[MI];
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) wa[nj] = rd_w(0, nj);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) af[mi] = rd_a(0, mi);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < HALF; ++mi)
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = Half16<H>::mfma(wa[nj], af[mi], acc[mi][nj]);
            __builtin_amdgcn_sched_barrier(0);
            if (feed && !early) issue_part(0, 2, jn);
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) wb[nj] = rd_w(1, nj);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = HALF; mi < MI; ++mi)
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = Half16<H>::mfma(wa[nj], af[mi], acc[mi][nj]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < HALF; ++mi) af[mi] = rd_a(1, mi);
            if (feed && !early) issue_part(1, 2, jn);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < HALF; ++mi)
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = Half16<H>::mfma(wb[nj], af[mi], acc[mi][nj]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = HALF; mi < MI; ++mi) af[mi] = rd_a(1, mi);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = HALF; mi < MI; ++mi)
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = Half16<H>::mfma(wb[nj], af[mi], acc[mi][nj]);
        }
        // ---- epilogue of tile t (the next tile's first stages are already in flight).  All residual loads
        // are issued before the first one is consumed, so their latency is paid once per tile, not per sub-tile.
        const int nbase = nt * BN + wn * 64 + kq * 16;
        const bool ncol_ok = nbase + 16 <= p.N;
        constexpr int EB = IO ? 2 : 4;              // sub-tiles per epilogue batch (residual registers: 8 (16 split) per sub-tile)
        // the tile's destination (wave-uniform): C2 takes the tiles from column n_split on
        H* c_hi = static_cast<H*>(p.C);
        H* c_lo = static_cast<H*>(p.C_lo);
        int ldc = p.ldc, cbase = nbase;
        if constexpr (EXT) {
            if (x.C2 != nullptr && nt * BN >= x.n_split) {
                c_hi = static_cast<H*>(x.C2);
                c_lo = static_cast<H*>(x.C2_lo);
                ldc = x.ldc2;
                cbase = nbase - x.n_split;
            }
        }
        const bool rsplit = IO && p.R_lo != nullptr, csplit = IO && c_lo != nullptr;
#pragma unroll
        for (int b0 = 0; b0 < MI; b0 += EB) {
            v8 res[EB][2], resl[IO ? EB : 1][2];
            if (p.R) {
#pragma unroll
                for (int e = 0; e < EB; ++e) {
                    const int m = mt * BM + wm * (MI * 16) + (b0 + e) * 16 + fr;
                    if (m < p.M && ncol_ok) {
                        const H* rp = static_cast<const H*>(p.R) + (long long)m * p.ldr + nbase;
                        res[e][0] = *reinterpret_cast<const v8*>(rp);
                        res[e][1] = *reinterpret_cast<const v8*>(rp + 8);
                        if constexpr (IO != 0) {
                            if (rsplit) {
                                const H* rl = static_cast<const H*>(p.R_lo) + (long long)m * p.ldr + nbase;
                                resl[e][0] = *reinterpret_cast<const v8*>(rl);
                                resl[e][1] = *reinterpret_cast<const v8*>(rl + 8);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < EB; ++e) {
                const int mi = b0 + e;
                const int m = mt * BM + wm * (MI * 16) + mi * 16 + fr;
                if (m < p.M && ncol_ok) {
                    float v[16];
#pragma unroll
                    for (int nj = 0; nj < 4; ++nj)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[nj * 4 + r] = acc[mi][nj][r];
                    if (p.R) {
                        if constexpr (IO != 0) {
                            if (rsplit) {          // (hi + lo) first: exact in fp32 (lo is below hi's last bit)
#pragma unroll
                                for (int i = 0; i < 8; ++i) {
                                    v[i] += (float)res[e][0][i] + (float)resl[e][0][i];
                                    v[8 + i] += (float)res[e][1][i] + (float)resl[e][1][i];
                                }
                            } else {
#pragma unroll
                                for (int i = 0; i < 8; ++i) { v[i] += (float)res[e][0][i]; v[8 + i] += (float)res[e][1][i]; }
                            }
                        } else {
#pragma unroll
                            for (int i = 0; i < 8; ++i) { v[i] += (float)res[e][0][i]; v[8 + i] += (float)res[e][1][i]; }
                        }
                    }
                    if (p.relu) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) v[i] = fmaxf(v[i], 0.f);
                    }
                    H* cp = c_hi + (long long)m * ldc + cbase;
                    float lo[8], hi[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { lo[i] = v[i]; hi[i] = v[8 + i]; }
                    Vec8<H>::store(cp, lo);
                    Vec8<H>::store(cp + 8, hi);
                    if constexpr (IO != 0) {
                        if (csplit) {              // low plane: what the rounding to the 16-bit type dropped
#pragma unroll
                            for (int i = 0; i < 8; ++i) { lo[i] = v[i] - (float)(H)v[i]; hi[i] = v[8 + i] - (float)(H)v[8 + i]; }
                            H* cl = c_lo + (long long)m * ldc + cbase;
                            Vec8<H>::store(cl, lo);
                            Vec8<H>::store(cl + 8, hi);
                        }
                    }
                }
            }
        }
        if (t + nwg < total) init_acc(t + nwg);
    }
}

// The launchers take tile counts and the grid from the op's route (gemm_route below); a.ntiles is set by launch_gemm.
template <typename H, int WM, int WN, int MI, int STAGES, int NSUB, int IO, int AST, bool EXT>
int launch_ring(const GemmArgs& a, const avl_gemm_route& r, hipStream_t s, const RingExt& x) {
    constexpr int BM = WM * MI * 16, BN = WN * 64, LDS = (AST * BM + STAGES * BN) * 128;
    static_assert(LDS <= 160 * 1024, "ring does not fit LDS");
    // set on every launch: the attribute is per device and this may be called from several threads / for several devices
    AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_ring<H, WM, WN, MI, STAGES, NSUB, IO, AST, EXT>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    hipLaunchKernelGGL((k_gemm_ring<H, WM, WN, MI, STAGES, NSUB, IO, AST, EXT>), dim3(r.workgroups), dim3(WM * WN * 64), LDS, s, a, r.m_tiles, x);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

template <typename T, int WM, int WN>
int launch_plain(const GemmArgs& a, const avl_gemm_route& r, hipStream_t s, const RingExt&) {
    constexpr int LDS = 2 * (WM * 64 + WN * 64) * 128;
    AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm<T, WM, WN>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    hipLaunchKernelGGL((k_gemm<T, WM, WN>), dim3(r.workgroups), dim3(WM * WN * 64), LDS, s, a);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// ---------------------------------------------------------------------------------------------
// MX variant of the 256 x 256 ring GEMM ("mixed" precision, layer3 / layer4 / ASPP 1x1 convs).
//
//   out = W . x   with  W = Wh + Wl,  x = xh (+ xl)   (f16 pairs)
//       ~ Wh.xh                                  main pass:   v_mfma_f32_16x16x32_f16, K blocks of 64
//       + Q4(Wl).Q4(xh)  [+ Q4(Wh).Q4(xl)]       corrections: v_mfma_scale_f32_16x16x128_f8f6f4 on MX-FP4 operands
//
// The correction terms are 2^-11 of the result, so 2-3 significant bits are plenty for them (tools/precision_study.py:
// the logits error does not move): FP4 (e2m1) with one power-of-two scale per 32 values along K, which the CDNA4 matrix
// cores multiply at 4x the f16 rate -- a correction pass costs a quarter of an f16 pass instead of a whole one.
// The scaled MFMA has the same C/D register layout as the f16 one, so all passes accumulate into the same registers.
//
// Data: an FP4 plane is [rows][K/2] bytes (element 2i in the low nibble of byte i); its scales are E8M0 bytes laid out
// [K/256][rows][8] so that a 256-row tile's scales for one sub-step are 2 KB contiguous.  In LDS an FP4 tile is 256 rows
// x 128 B = 256 K-values per row: exactly the geometry (DMA, XOR swizzle, fragment addressing) of an f16 tile with 64.
// One K macro-block of 256 therefore is 4 f16 sub-steps + 1 or 2 FP4 sub-steps, every one of them "DMA a 32 KB
// activation tile and a 32 KB weight tile, 64 MFMAs per wave".  Two ring stages, vmcnt(0) waits (no hand-counted
// immediates here: the scale DMAs make the per-wave instruction count non-uniform).
struct MxArgs {
    GemmArgs g;                 // A = x hi plane (f16), W = W hi [N][K] f16 (plain rows), R / R_lo, C / C_lo as usual
    const char* Aq[2];          // FP4 planes of the input: Q4(x hi), Q4(x lo) (second one only when nmx == 2)
    const char* As[2];          // their scales
    const char* Wq[2];          // FP4 weights paired with them: Q4(W lo), Q4(W hi)
    const char* Ws[2];
    int ldaq;                   // bytes per row of the input FP4 planes
    long long a_srows, w_srows; // rows per K macro-block in the scale arrays (allocated rows)
    char* Cq[2];                // FP4 planes of the OUTPUT (hi part, lo part) and their scales, or NULL
    char* Cs[2];
    int ldcq;
    long long c_srows;
    int nmx;                    // correction passes: 1 (weights only) or 2 (input split as well)
    const char* Rq;             // FP4 plane + scales of the residual's lo part (instead of the f16 plane g.R_lo), or NULL
    const char* Rs;
    int ldrq;
    long long r_srows;
    // second input appended along K (conv3 + downsample in one product): macro-blocks >= nmb1 read it
    int nmb1;
    const void* A2;
    int lda2, ldaq2;
    const char* Aq2[2];
    const char* As2[2];
    long long a_srows2;
    int stagger;                // 1: waves 0-3 issue their LDS-DMAs after the first K half of a sub-step
    // k_gemm_mx_pipe reads of the INPUT side only A, A2, Aq[0], Aq2[0], W, Wq[0], K, nmb1, a_srows and w_srows: rows are dense
    // (lda = K1, lda2 = K - K1, a_srows2 = a_srows) and the other planes lie where mx_bundle_at puts them behind Aq[0] / Aq2[0] /
    // Wq[0]; launch_mx_pipe checks exactly that.  k_gemm_ring_mx reads every field.
};

// The epilogue of an MX GEMM tile (shared by k_gemm_ring_mx and k_gemm_mx_pipe): bias is in the accumulators; residual (one or two
// planes), ReLU, f16 hi [+ lo] planes, and the FP4 planes + scales the next MX GEMM reads.
template <int IO, int MI>
__device__ __forceinline__ void mx_epilogue(const MxArgs& q, f32x4 (&acc)[MI][4], int nt, int mt, int wm, int wn, int fr, int kq) {
    typedef f16 H;
    typedef typename Half16<H>::v8 v8;
    constexpr int BM = 2 * MI * 16, BN = 256;
    const GemmArgs& p = q.g;
    const int nbase = nt * BN + wn * 64 + kq * 16;
    const bool ncol_ok = nbase + 16 <= p.N;
    // The uniform decisions of the eight rounds -- which planes there are -- are taken ONCE, into one flag word that the compiler
    // cannot see through: a round then tests a bit of one scalar register (s_bitcmp) where it used to compare a 64-bit pointer or
    // keep a 64-bit lane mask per decision alive, which is what pushed the kernels' scalar registers into spills.
    enum { F_RES = 1, F_RES_LO16 = 2, F_RES_LOQ = 4, F_OUT_LO16 = 8, F_RELU = 16, F_OUT_Q0 = 32, F_OUT_Q1 = 64 };
    unsigned fl = (p.R ? F_RES : 0) | (p.R_lo ? F_RES_LO16 : 0) | (q.Rq ? F_RES_LOQ : 0) | (p.C_lo ? F_OUT_LO16 : 0) | (p.relu ? F_RELU : 0) |
                  (q.Cq[0] ? F_OUT_Q0 : 0) | (q.Cq[1] ? F_OUT_Q1 : 0);
    asm volatile("" : "+s"(fl));
    // The epilogue is VALU-issue bound (eight rounds of ~250 vector instructions per wave while the matrix pipe idles), so:
    // every address is a 32-bit BYTE offset from a uniform plane base (validate_gemm bounds the planes to 2 GB), the result is
    // converted to f16 ONCE (the packed vector is stored and read back as hi), every lane stores its own 8 FP4 bytes.
    const unsigned m0 = (unsigned)(mt * BM + wm * (MI * 16) + fr);
    const unsigned sc_r = (unsigned)(nbase >> 8) * (unsigned)q.r_srows * 8u + (unsigned)((nbase >> 5) & 7);
    const unsigned sc_c = (unsigned)(nbase >> 8) * (unsigned)q.c_srows * 8u + (unsigned)((nbase >> 5) & 7);
    // the residual of row mi + 1 is requested before row mi is worked on (its loads could otherwise not move above row
    // mi's stores, and eight dependent load -> compute -> store rounds cost more than the K loop of a short-K tile)
    v8 nr0 = {}, nr1 = {};
    uint2 npk = make_uint2(0u, 0u);
    unsigned nsb = 127u;
    auto load_res = [&](int mi) {
        const unsigned m = m0 + mi * 16;
        if ((fl & F_RES) && (int)m < p.M && ncol_ok) {
            const H* rp = reinterpret_cast<const H*>(static_cast<const char*>(p.R) + (m * (unsigned)p.ldr + (unsigned)nbase) * 2u);
            nr0 = *reinterpret_cast<const v8*>(rp);
            nr1 = *reinterpret_cast<const v8*>(rp + 8);
            if (fl & F_RES_LOQ) {       // the lo part as FP4: 16 values = 8 bytes, one scale byte for the lane pair's 32-block
                npk = *reinterpret_cast<const uint2*>(q.Rq + (m * (unsigned)q.ldrq + (unsigned)(nbase / 2)));
                nsb = (unsigned char)q.Rs[sc_r + m * 8u];
            }
        }
    };
    load_res(0);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const unsigned m = m0 + mi * 16;
        const bool live = (int)m < p.M && ncol_ok;
        const v8 r0 = nr0, r1 = nr1;
        const uint2 pk = npk;
        const unsigned sb = nsb;
        if (mi + 1 < MI) load_res(mi + 1);
        float v[16];
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[nj * 4 + r] = acc[mi][nj][r];
        if ((fl & F_RES) && live) {
            float rl[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) rl[i] = 0.f;
            if (fl & F_RES_LO16) {
                const H* rlp = reinterpret_cast<const H*>(static_cast<const char*>(p.R_lo) + (m * (unsigned)p.ldr + (unsigned)nbase) * 2u);
                const v8 l0 = *reinterpret_cast<const v8*>(rlp), l1 = *reinterpret_cast<const v8*>(rlp + 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) { rl[i] = (float)l0[i]; rl[8 + i] = (float)l1[i]; }
            } else if (fl & F_RES_LOQ) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                const float sc = __uint_as_float(sb << 23);
#define AVL_FP4_DEC(w, sel, o) { const v2f d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, sel); rl[o] = d.x; rl[o + 1] = d.y; }
                AVL_FP4_DEC(pk.x, 0, 0) AVL_FP4_DEC(pk.x, 1, 2) AVL_FP4_DEC(pk.x, 2, 4) AVL_FP4_DEC(pk.x, 3, 6)
                AVL_FP4_DEC(pk.y, 0, 8) AVL_FP4_DEC(pk.y, 1, 10) AVL_FP4_DEC(pk.y, 2, 12) AVL_FP4_DEC(pk.y, 3, 14)
#undef AVL_FP4_DEC
            }
            // hi + lo first (exact in fp32), then the accumulator: same order as k_gemm_ring
#pragma unroll
            for (int i = 0; i < 8; ++i) { v[i] += (float)r0[i] + rl[i]; v[8 + i] += (float)r1[i] + rl[8 + i]; }
        }
        if (fl & F_RELU) {
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        v8 h0, h1;
#pragma unroll
        for (int i = 0; i < 8; ++i) { h0[i] = (H)v[i]; h1[i] = (H)v[8 + i]; }
        float hi[16], lo[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            hi[i] = (float)h0[i];
            hi[8 + i] = (float)h1[i];
            lo[i] = v[i] - hi[i];
            lo[8 + i] = v[8 + i] - hi[8 + i];
        }
        const unsigned coff = (m * (unsigned)p.ldc + (unsigned)nbase) * 2u;       // bytes
        if (live) {
            H* cp = reinterpret_cast<H*>(static_cast<char*>(p.C) + coff);
            *reinterpret_cast<v8*>(cp) = h0;
            *reinterpret_cast<v8*>(cp + 8) = h1;
        }
        if (fl & F_OUT_LO16) { // a stored lo plane is f16: its FP4 copy is taken from what it holds
            v8 l0, l1;
#pragma unroll
            for (int i = 0; i < 8; ++i) { l0[i] = (H)lo[i]; l1[i] = (H)lo[8 + i]; }
            if (live) {
                H* cl = reinterpret_cast<H*>(static_cast<char*>(p.C_lo) + coff);
                *reinterpret_cast<v8*>(cl) = l0;
                *reinterpret_cast<v8*>(cl + 8) = l1;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) { lo[i] = (float)l0[i]; lo[8 + i] = (float)l1[i]; }
        }
        if constexpr (IO != 0) {
            // every lane takes part in the block exchange; rows past M quantise whatever they hold and store nothing
            // (the partner lane is the same row, so it is dead as well)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                if (!(fl & (pl == 0 ? F_OUT_Q0 : F_OUT_Q1))) continue;
                unsigned pq[2];
                const unsigned sq = quantize_fp4_block(pl == 0 ? hi : lo, pq);
                if (live) {
                    *reinterpret_cast<uint2*>(q.Cq[pl] + (m * (unsigned)q.ldcq + (unsigned)(nbase / 2))) = make_uint2(pq[0], pq[1]);
                    if ((kq & 1) == 0) q.Cs[pl][sc_c + m * 8u] = (char)sq;
                }
            }
        }
    }
}

// MI = 8: 256 x 256 tiles; MI = 4: 128 x 256 tiles for shapes that would otherwise leave half the CUs without a tile.
template <int IO, int MI>
__global__ void __launch_bounds__(512) k_gemm_ring_mx(MxArgs q, int mtiles) {
    typedef f16 H;
    typedef typename Half16<H>::v8 v8;
    typedef int v8i __attribute__((ext_vector_type(8)));
    constexpr int WM = 2, WN = 4, STAGES = 2;
    constexpr int NW = WM * WN, BM = WM * MI * 16, BN = WN * 64;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128;
    constexpr int W_REGION = STAGES * A_BYTES, S_REGION = W_REGION + STAGES * W_BYTES;      // [A tiles][W tiles][scale blocks]
    constexpr int S_BYTES = 4096;                                                            // A scales 2 KB | W scales 2 KB
    constexpr int A_INSTR = BM / 8 / NW, W_INSTR = BN / 8 / NW;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const GemmArgs& p = q.g;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int nwg = gridDim.x;
    int vb;
    {
        const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3, qq = nwg >> 3, r = nwg & 7;
        vb = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + local;
    }
    const int total = mtiles * p.ntiles;
    const int nmb = p.K / 256;                 // K macro-blocks per tile
    const int nsub = 4 + q.nmx;                // sub-steps per macro-block: 4 f16 + the FP4 corrections
    const unsigned lds_base = lds_addr(lds);

    // ---- producer: SGPR tile base + VGPR offset addressing.  DMA instruction i of this wave covers rows (i * NW + wave) * 8 + srow:
    // the (i, wave) part is uniform and goes into the scalar base, the lane keeps srow * row_bytes + its swizzled chunk
    // ((r & 7) == srow); the weight swizzle key mixes uniform and lane bits, so those offsets stay per instruction.
    const int srow = lane >> 3, schunk = lane & 7;
    const unsigned ct = (unsigned)((schunk ^ srow) << 4);
    const unsigned a_lane16 = (unsigned)srow * (unsigned)(p.lda * 2) + ct, a_laneq = (unsigned)srow * (unsigned)q.ldaq + ct;
    const unsigned a_lane16_2 = (unsigned)srow * (unsigned)(q.lda2 * 2) + ct, a_laneq_2 = (unsigned)srow * (unsigned)q.ldaq2 + ct;
    unsigned w_off16[W_INSTR], w_offq[W_INSTR];
#pragma unroll
    for (int i = 0; i < W_INSTR; ++i) {
        const int r = (i * NW + wave) * 8 + srow;
        const int key = ((r >> 1) & 1) | (((r >> 4) & 3) << 1);
        w_off16[i] = (unsigned)r * (unsigned)(p.K * 2) + ((schunk ^ key) << 4);
        w_offq[i] = (unsigned)r * (unsigned)(p.K / 2) + ((schunk ^ key) << 4);
    }
    int pt = vb, pmb = 0, pj = 0, issued = 0;
    auto issue = [&]() {
        const int nt = pt % p.ntiles, mt = pt / p.ntiles;
        const unsigned abase = lds_base + (issued % STAGES) * A_BYTES + wave * 1024;
        const unsigned wbase = lds_base + W_REGION + (issued % STAGES) * W_BYTES + wave * 1024;
        const bool second = pmb >= q.nmb1;                     // which input this K macro-block comes from
        const int mbl = second ? pmb - q.nmb1 : pmb;
        if (pj < 4) {
            const long long rowb = second ? (long long)q.lda2 * 2 : (long long)p.lda * 2;
            const char* sa = static_cast<const char*>(second ? q.A2 : p.A) + ((long long)mt * BM + wave * 8) * rowb + (long long)(mbl * 4 + pj) * 128;
            const char* sw = static_cast<const char*>(p.W) + (long long)nt * BN * p.K * 2 + (long long)(pmb * 4 + pj) * 128;
            const unsigned al = second ? a_lane16_2 : a_lane16;
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i) glds16_saddr(sa + (long long)i * (NW * 8) * rowb, al, abase + i * NW * 1024);
#pragma unroll
            for (int i = 0; i < W_INSTR; ++i) glds16_saddr(sw, w_off16[i], wbase + i * NW * 1024);
        } else {
            const int t = pj - 4;
            const long long rowb = second ? q.ldaq2 : q.ldaq;
            const char* sa = (second ? q.Aq2[t] : q.Aq[t]) + ((long long)mt * BM + wave * 8) * rowb + (long long)mbl * 128;
            const char* sw = q.Wq[t] + (long long)nt * BN * (p.K / 2) + (long long)pmb * 128;
            const unsigned al = second ? a_laneq_2 : a_laneq;
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i) glds16_saddr(sa + (long long)i * (NW * 8) * rowb, al, abase + i * NW * 1024);
#pragma unroll
            for (int i = 0; i < W_INSTR; ++i) glds16_saddr(sw, w_offq[i], wbase + i * NW * 1024);
            // scales: BM x 8 bytes for the activation rows (waves 0, 1: one KB each), 2 KB for the weight rows (waves 2, 3)
            if (wave < 4 && (wave >= 2 || wave * 128 < BM)) {
                const char* as = second ? q.As2[t] + ((long long)mbl * q.a_srows2 + (long long)mt * BM) * 8
                                        : q.As[t] + ((long long)mbl * q.a_srows + (long long)mt * BM) * 8;
                const char* ss = wave < 2 ? as + wave * 1024
                                          : q.Ws[t] + ((long long)pmb * q.w_srows + (long long)nt * BN) * 8 + (wave - 2) * 1024;
                glds16_saddr(ss, (unsigned)lane * 16u, lds_base + S_REGION + (issued % STAGES) * S_BYTES + wave * 1024);
            }
        }
        ++issued;
        if (++pj == nsub) {
            pj = 0;
            if (++pmb == nmb) { pmb = 0; pt += nwg; }
        }
    };
    if (pt < total) issue();

    // ---- consumer
    // fragment addressing: row r of a tile sits at r * 128 with its 16-byte chunks XOR-swizzled by key(r); the keys and the
    // scale addresses (r * 8) are recomputed from the row offsets instead of being kept in registers (the 128
    // accumulators leave little room: every array here is sized to stay clear of spills)
    const int fr = lane & 15, kq = lane >> 4;
    const int a_row0 = wm * (MI * 16) + fr;                       // + 16 mi
    int w_off[4], w_key[4];
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
        const int row = wn * 64 + (fr >> 2) * 16 + nj * 4 + (fr & 3);
        w_off[nj] = W_REGION + row * 128;
        w_key[nj] = ((row >> 1) & 1) | (((row >> 4) & 3) << 1);
    }
    const int a_key = a_row0 & 7;                                  // (a_row0 + 16 mi) & 7 is the same for every mi
    f32x4 acc[MI][4];
    auto init_acc = [&](int t) {
        const int nb = (t % p.ntiles) * BN + wn * 64 + kq * 16;
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + nb + 4 * nj);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[mi][nj] = f32x4{b.x, b.y, b.z, b.w};
        }
    };
    if (vb < total) init_acc(vb);

    int g = 0;
    static_assert(NW == 8, "the DMA stagger assumes waves w and w + 4 on one SIMD");
    const int late = (wave >= 4 || q.stagger == 0) ? 0 : 1;       // the K half in front of which this wave issues its DMAs
    for (int t = vb; t < total; t += nwg) {
        const int nt = t % p.ntiles, mt = t / p.ntiles;
        // two plain loops per macro-block (f16 sub-steps, then FP4 sub-steps) rather than one loop with an if / else on the
        // sub-step kind: the accumulators then have ONE definition chain (an if / else made hipcc keep two copies of them)
        for (int mb = 0; mb < nmb; ++mb) {
            for (int j = 0; j < 4; ++j, ++g) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // sub-step g has landed (this wave's share)
                __builtin_amdgcn_s_barrier();
                // sub-step g+1 -> the slots read during step g-1.  Waves w and w + 4 share a SIMD: one issues its LDS-DMAs (100+
                // cycles of issue each) at the head of the step, the other after its first K half, so that the SIMD's matrix pipe
                // has one wave's MFMAs to run while the other is busy issuing (GEMMs 3.53 -> 3.40 ms per frame; spreading the
                // instructions two at a time between MFMA groups instead: 4.0 ms)
                const char* abase = lds + (g % STAGES) * A_BYTES + a_row0 * 128;
                const char* wbase = lds + (g % STAGES) * W_BYTES;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    if (kk == late && pt < total) issue();
                    v8 wf[4];
#pragma unroll
                    for (int nj = 0; nj < 4; ++nj) wf[nj] = *reinterpret_cast<const v8*>(wbase + w_off[nj] + (((kk * 4 + kq) ^ w_key[nj]) << 4));
                    const int achunk = ((kk * 4 + kq) ^ a_key) << 4;
                    v8 af = *reinterpret_cast<const v8*>(abase + achunk);
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) {
                        const v8 cur = af;
                        if (mi + 1 < MI) af = *reinterpret_cast<const v8*>(abase + (mi + 1) * 2048 + achunk);
#pragma unroll
                        for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = Half16<H>::mfma(wf[nj], cur, acc[mi][nj]);
                    }
                }
            }
            for (int u = 0; u < q.nmx; ++u, ++g) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                const char* abase = lds + (g % STAGES) * A_BYTES + a_row0 * 128;
                const char* wbase = lds + (g % STAGES) * W_BYTES;
                const char* sbase = lds + (g % STAGES) * S_BYTES + S_REGION;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    if (kk == late && pt < total) issue();
                    int4 wf[4];
                    int ws[4];
#pragma unroll
                    for (int nj = 0; nj < 4; ++nj) {
                        wf[nj] = *reinterpret_cast<const int4*>(wbase + w_off[nj] + (((kk * 4 + kq) ^ w_key[nj]) << 4));
                        {   // weight scales as network.permute_w_scales lays them out: [16-row block][row & 3][kq][nj][kk]
                            const uint2 w8 = *reinterpret_cast<const uint2*>(sbase + 2048 + (wn * 4 + (fr >> 2)) * 128 + ((fr & 3) * 4 + kq) * 8);
                            ws[nj] = (int)(((nj < 2 ? w8.x : w8.y) >> (8 * ((nj & 1) * 2 + kk))) & 0xffu);
                        }
                    }
                    const int achunk = ((kk * 4 + kq) ^ a_key) << 4;
                    int4 af = *reinterpret_cast<const int4*>(abase + achunk);
                    unsigned asw = *reinterpret_cast<const unsigned*>(sbase + a_row0 * 8 + kk * 4);
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) {
                        const int4 cur = af;
                        const int as = (int)((asw >> (8 * kq)) & 0xffu);
                        if (mi + 1 < MI) {
                            af = *reinterpret_cast<const int4*>(abase + (mi + 1) * 2048 + achunk);
                            asw = *reinterpret_cast<const unsigned*>(sbase + (a_row0 + (mi + 1) * 16) * 8 + kk * 4);
                        }
                        const v8i xa = {cur.x, cur.y, cur.z, cur.w, 0, 0, 0, 0};
#pragma unroll
                        for (int nj = 0; nj < 4; ++nj) {
                            const v8i wa = {wf[nj].x, wf[nj].y, wf[nj].z, wf[nj].w, 0, 0, 0, 0};
                            acc[mi][nj] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa, xa, acc[mi][nj], 4, 4, 0, ws[nj], 0, as);
                        }
                    }
                }
            }
        }
        mx_epilogue<IO, MI>(q, acc, nt, mt, wm, wn, fr, kq);
        if (t + nwg < total) init_acc(t + nwg);
    }
}

// ---------------------------------------------------------------------------------------------
// k_gemm_mx_pipe (round 3): the same tile, ring (two stages), LDS image, DMA geometry and epilogue as k_gemm_ring_mx, but the K
// loop is ONE software-pipelined instruction stream per wave instead of "barrier, read, multiply" rounds.
//
// What was wrong with the rounds (ISA of k_gemm_ring_mx, round 2): after the barrier every wave read 6 fragments, waited, issued
// 8 MFMAs, read 2 more, waited, 8 MFMAs ...: a read -> wait -> multiply chain with the LDS latency exposed every 128 cycles and
// the whole read burst of all 8 waves exposed at every step boundary.
//
// The stream (MI = 8: 16 "steps" of 4 MFMAs per sub-step; step s multiplies activation fragment mi = s % 8 of K half kk = s / 8):
//   * fragments are read D = 3 steps before their MFMAs, one activation fragment per step (a rolling window of four), two sets of
//     weight fragments (the set of the second K half is read during steps 0-3 of the first);
//   * the step boundaries are moved INTO the stream, and there are two per sub-step, one per LDS slot kind ("events"):
//       EW, in front of step 5:  s_waitcnt lgkmcnt(1|2); s_barrier -- every wave has read its last WEIGHT fragment of slot g % 2:
//                                the weight tile of sub-step g + 2 may overwrite it;
//       EV, in front of step 13: s_waitcnt vmcnt(4) lgkmcnt(0); s_barrier -- every wave's DMAs for sub-step g + 1 have landed (only
//                                the 4 instructions of a weight burst sent since may still fly; vmcnt(0) when none was sent) and
//                                every wave has read its last ACTIVATION fragment of slot g % 2.  Right behind it the wave reads
//                                the first fragments of sub-step g + 1 from the other slot -- while it still has the 12 MFMAs of
//                                steps 13 .. 15 in registers to issue: the matrix pipe never waits for a barrier + a cold LDS burst;
//   * one sub-step's DMA is therefore two bursts of 4 instructions per wave (weights; activations + the scale blocks of an FP4
//     sub-step), and the bursts of the two waves of a SIMD are COMPLEMENTARY: waves 4-7 send theirs right behind EW / EV, waves 0-3
//     one event later (right in front of EV / of the next EW), so that one wave of every SIMD issues MFMAs while the other pays
//     the ~150 cycles per LDS-DMA instruction (s_memtime stamps: a 4-instruction burst takes ~600 cycles: the 16
//     instructions of the four waves that burst together queue in the CU's one vector-memory path).
// What bounds it now (stamps): 64 KB per sub-step through that path at ~27 B/clk = ~2400 cycles, against 2048 cycles of MFMA
// issue per SIMD: the 256 x 256 tile is L2 -> LDS bound on this chip; the stream runs at ~3500 cycles per sub-step (was ~4000).
// RAW / WAR on LDS (MI355X_MICROARCH.md, "Read a staged buffer one phase AFTER the wait that retires it"): a slot is read only
// behind the barrier that follows every wave's vmcnt wait for it; it is overwritten only by DMAs issued behind the barrier that
// follows every wave's lgkmcnt wait with all its reads of that slot already issued.  The two hand counts: vmcnt(4) -- younger
// operations (compiler-visible loads / stores, scratch) only make it wait for more; lgkmcnt(1|2) -- at least that many LDS reads
// are issued behind the last weight read (step 4: one fragment, plus its scale byte in an FP4 sub-step).
// Sub-step kinds (f16 / FP4) alternate inside the stream; the fragments carried across a boundary are plain 128-bit values.
// MI = 4 (128 x 256 tiles): one event (both slots) in front of step 5 of 8, vmcnt(0).
template <int IO, int MI, int LATE>
__global__ void __launch_bounds__(512) k_gemm_mx_pipe(MxArgs q, int mtiles) {
    typedef f16 H;
    typedef typename Half16<H>::v8 v8;
    typedef int v8i __attribute__((ext_vector_type(8)));
    constexpr int WM = 2, WN = 4, STAGES = 2;
    constexpr int NW = WM * WN, BM = WM * MI * 16, BN = WN * 64;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128;
    constexpr int W_REGION = STAGES * A_BYTES, S_REGION = W_REGION + STAGES * W_BYTES;
    constexpr int S_BYTES = 4096;
    constexpr int A_INSTR = BM / 8 / NW, W_INSTR = BN / 8 / NW;
    constexpr int NS = 2 * MI, D = 3, EV = NS - D;              // steps per sub-step; fragments are read D steps ahead; the (main) event sits in front of step EV
    constexpr int EW = MI == 8 ? 5 : EV;                         // ... and the weight-slot event (MI = 4: one event for both slots)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const GemmArgs& p = q.g;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int nwg = gridDim.x;
    int vb;
    {
        const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3, qq = nwg >> 3, r = nwg & 7;
        vb = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + local;
    }
    const int ntiles = p.ntiles, nmx = q.nmx;
    const int total = mtiles * ntiles;
    const int nmb = p.K / 256;
    const int nsub = 4 + nmx;
    const unsigned lds_base = lds_addr(lds);

    // ---- producer: SGPR base + VGPR lane offset addressing.  DMA instruction i of this wave covers rows (i * 8 + wave) * 8 + srow
    // of a tile: the (i, wave) part is uniform and goes into the scalar base, the lane keeps srow * row_bytes + its swizzled chunk
    // ((r & 7) == srow for activation rows).  For weight rows the swizzle key ((r >> 1) & 1) | (((r >> 4) & 3) << 1) does not depend
    // on i either (i moves r by 64): ONE lane offset per plane kind.
    // The hot path of issue_w / issue_a works on a handful of scalars (run_*: where the next burst reads each plane of the input the
    // current K macro-block comes from, at this tile and wave) that are set anew only at a tile switch and where the K loop passes
    // from the first input to the second (conv3 + downsample): no scalar (kernarg) loads inside the stream, where their
    // out-of-order lgkmcnt would force `s_waitcnt lgkmcnt(0)` in front of every LDS fragment use, and no spilled scalar either
    // (tests/test_abi_mx_pipe_scalars.py: no v_readlane / v_writelane between the first and the last MFMA).
    // The lane offsets are NOT kept in registers (the K loop has none to spare: hipcc spilled them to scratch, and a scratch reload is a
    // vector-memory operation in the middle of the hand-counted DMA stream): every burst re-derives them from the lane id, ~8 VALU
    // instructions beside 64 MFMAs.  The lane id comes out of a volatile asm so that the arithmetic is not hoisted back out.
    auto lane_now = [&]() __attribute__((always_inline)) {
        unsigned l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
    // The six source pointers RUN: they stand at the piece the next burst fetches and move on by a constant when a sub-step (f16
    // planes: 128 bytes along K) or a K macro-block (FP4 planes: 128 bytes; scale arrays: one block of rows) has been issued, so a
    // burst costs an add pair per instruction and no multiply chain from (tile, macro-block, sub-step) indices.
    int pt = vb, pmb = 0, pj = 0, issued = 0;                   // tile, K macro-block, sub-step being issued next
    // What a switch (to the next tile; from the first input to the second) starts from is kept small, because it stays in scalar
    // registers all through the stream: per operand the f16 plane and the BASE of its MX bundle, the allocated rows and the K split.
    // The input rows are dense (row bytes from the operand's own K) and a bundle's planes lie where mx_bundle_at (seg_types.h) puts
    // them -- FP4 hi, scales hi, FP4 lo, scales lo -- so strides and plane distances are a few multiplies at the switch instead of a
    // dozen more pointers held; launch_mx_pipe refuses arguments that are laid out otherwise.
    unsigned cur_rowb16 = 0;                                     // bytes per row of the f16 input plane (the FP4 plane: a quarter)
    const char *run_a16 = nullptr, *run_aq = nullptr, *run_as = nullptr, *run_w16 = nullptr, *run_wq = nullptr, *run_ws = nullptr;
    unsigned cur_aps = 0;                                        // distance from correction plane 0 to plane 1 of the input
    // These few are what the stream holds of the argument struct.  They are read from the kernel-argument segment at entry AND again
    // behind every epilogue (read_args, through a pointer the compiler cannot see through), so that they are dead while the epilogue
    // runs: it needs the scalar registers for its own dozen planes and strides, which in turn are dead in the stream.
    const char *c_A, *c_A2, *c_Aq, *c_Aq2, *c_W, *c_Wq;
    unsigned K, K1, arows, wrows;
    unsigned asb, wsb;                                           // bytes per K macro-block of the input's / the weights' scales
    unsigned w_pb, wps;                                          // the weights' FP4 plane; distance from correction plane 0 to plane 1
    auto read_args = [&]() __attribute__((always_inline)) {
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();        // `q` is the kernel's first argument: offset 0
        asm volatile("" : "+s"(ka));
        const MxArgs* a = (const MxArgs*)ka;
        c_A = static_cast<const char*>(a->g.A); c_A2 = static_cast<const char*>(a->A2); c_Aq = a->Aq[0]; c_Aq2 = a->Aq2[0];
        c_W = static_cast<const char*>(a->g.W); c_Wq = a->Wq[0];
        K = (unsigned)a->g.K; K1 = (unsigned)a->nmb1 * 256u; arows = (unsigned)a->a_srows; wrows = (unsigned)a->w_srows;
        // the values are used HERE: the wait for the scalar loads stands here and not at their first use inside the stream
        asm volatile("" : "+s"(c_A), "+s"(c_A2), "+s"(c_Aq), "+s"(c_Aq2), "+s"(c_W), "+s"(c_Wq), "+s"(K), "+s"(K1), "+s"(arows), "+s"(wrows));
        asb = arows * 8u; wsb = wrows * 8u;
        w_pb = (unsigned)mx_plane_bytes(wrows, K); wps = w_pb + (unsigned)mx_scale_bytes(wrows, K);
    };
    read_args();
    int p_mt = 0;
    auto set_input = [&](bool second) __attribute__((always_inline)) {     // rare: tile switch, first -> second input
        const long long rows0 = (long long)p_mt * BM + wave * 8;
        const unsigned kin = second ? K - K1 : K1;                         // this input's share of K
        const char* a16 = second ? c_A2 : c_A;
        const char* aq = second ? c_Aq2 : c_Aq;
        const unsigned a_pb = (unsigned)mx_plane_bytes(arows, kin);
        cur_rowb16 = kin * 2u;
        run_a16 = a16 + rows0 * cur_rowb16;
        run_aq = aq + rows0 * (kin / 2u);
        run_as = aq + a_pb + (unsigned)(p_mt * BM * 8);
        cur_aps = a_pb + (unsigned)mx_scale_bytes(arows, kin);
    };
    auto set_tile = [&]() __attribute__((always_inline)) {                  // rare: once per tile
        const int nt_ = pt % ntiles;
        p_mt = pt / ntiles;
        run_w16 = c_W + (long long)nt_ * BN * K * 2;
        run_wq = c_Wq + (long long)nt_ * BN * (K / 2u);
        run_ws = c_Wq + w_pb + (unsigned)(nt_ * BN * 8);
        set_input(false);
    };
    // One sub-step's DMA is issued in two bursts (see the events below): the weight tile, then the activation tile (+ the scale
    // blocks of an FP4 sub-step, so that a weight burst is W_INSTR instructions for EVERY wave: the hand count at the event).
    auto issue_w = [&]() __attribute__((always_inline)) {
        const unsigned wbase = lds_base + W_REGION + (issued & 1) * W_BYTES + wave * 1024;
        // weight row of instruction i: r = (i * 8 + wave) * 8 + srow; its swizzle key ((r >> 1) & 1) | (((r >> 4) & 3) << 1) =
        // ((srow >> 1) & 1) | (((wave >> 1) & 3) << 1) does not depend on i
        const unsigned l = lane_now(), srow = l >> 3, cw = ((l & 7u) ^ (((srow >> 1) & 1u) | (((unsigned)(wave >> 1) & 3u) << 1))) << 4;
        const unsigned wr0 = (unsigned)wave * 8u + srow;
        // (instruction i + 1 reads NW * 8 rows further on: an unsigned add to the running pointer)
        if (pj < 4) {
            const char* sw = run_w16;
            const unsigned rb = K * 2u, wl = wr0 * rb + cw;
#pragma unroll
            for (int i = 0; i < W_INSTR; ++i, sw += rb * (NW * 8))
                glds16_saddr_m0(sw, wl, wbase + i * NW * 1024);
        } else {
            const char* sw = run_wq + (pj == 4 ? 0u : wps);
            const unsigned rb = K / 2u, wl = wr0 * rb + cw;
#pragma unroll
            for (int i = 0; i < W_INSTR; ++i, sw += rb * (NW * 8))
                glds16_saddr_m0(sw, wl, wbase + i * NW * 1024);
        }
    };
    // (the last piece also brings the scale blocks of an FP4 sub-step and moves the producer on to the next sub-step)
    auto issue_a = [&]() __attribute__((always_inline)) {
        const unsigned abase = lds_base + (issued & 1) * A_BYTES + wave * 1024;
        const unsigned l = lane_now(), srow = l >> 3, ct = ((l & 7u) ^ srow) << 4;        // activation rows: key = r & 7 = srow
        if (pj < 4) {
            const char* sa = run_a16;
            const unsigned al = srow * cur_rowb16 + ct;
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i, sa += cur_rowb16 * (NW * 8))
                glds16_saddr_m0(sa, al, abase + i * NW * 1024);
            run_a16 += 128;
            run_w16 += 128;
        } else {
            const unsigned ta = pj == 4 ? 0u : cur_aps, tw = pj == 4 ? 0u : wps;        // which correction pass
            const char* sa = run_aq + ta;
            const unsigned cur_rowbq = cur_rowb16 >> 2, a_lq = srow * cur_rowbq + ct;
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i, sa += cur_rowbq * (NW * 8))
                glds16_saddr_m0(sa, a_lq, abase + i * NW * 1024);
            // scales: BM x 8 bytes for the activation rows (waves 0, 1: one KB each), 2 KB for the weight rows (waves 2, 3)
            if (wave < 4 && (wave >= 2 || wave * 128 < BM)) {
                const char* ss = wave < 2 ? run_as + ta + wave * 1024 : run_ws + tw + (wave - 2) * 1024;
                glds16_saddr_m0(ss, l * 16u, lds_base + S_REGION + (issued & 1) * S_BYTES + wave * 1024);
            }
        }
        ++issued;
        if (++pj == nsub) {
            pj = 0;
            run_aq += 128; run_as += asb;                        // the next K macro-block
            run_wq += 128; run_ws += wsb;
            if (++pmb == nmb) {
                pmb = 0;
                pt += nwg;
                if (pt < total) set_tile();
            } else if (pmb * 256u == K1) set_input(true);
        }
    };
    if (pt < total) set_tile();
    static_assert(NW == 8, "the DMA stagger assumes waves w and w + 4 on one SIMD");
    const bool early = wave >= 4 || q.stagger == 0;             // issues its bursts right behind the events; the others LATE steps later
    if (pt < total) { issue_w(); issue_a(); }                    // sub-step 0 -> slots 0
    if (pt < total) { issue_w(); issue_a(); }                    // sub-step 1 -> slots 1

    // ---- consumer addressing: byte offsets inside a slot (the slot base is uniform and added per sub-step)
    const int fr = lane & 15, kq = lane >> 4;
    const int a_row0 = wm * (MI * 16) + fr;
    // weight row of n-tile nj: wrow0 + 4 nj; its swizzle key ((row >> 1) & 1) | (((row >> 4) & 3) << 1) does not depend on nj, and the
    // second K half is chunk ^ 4: one base register per operand, the rest is immediate offsets and one XOR
    const int wrow0 = wn * 64 + (fr >> 2) * 16 + (fr & 3);
    const int wkey_r = ((wrow0 >> 1) & 1) | (((wrow0 >> 4) & 3) << 1);
    const unsigned a_v0 = (unsigned)(a_row0 * 128 + ((kq ^ (a_row0 & 7)) << 4));
    const unsigned w_v0 = (unsigned)(W_REGION + wrow0 * 128 + ((kq ^ wkey_r) << 4));
    const unsigned sa_v = (unsigned)(S_REGION + a_row0 * 8 + kq);
    const unsigned sw_v = (unsigned)(S_REGION + 2048 + (wn * 4 + (fr >> 2)) * 128 + ((fr & 3) * 4 + kq) * 8);

    f32x4 acc[MI][4];
    auto init_acc = [&](const float* bias, int t) {
        const int nb = (t % ntiles) * BN + wn * 64 + kq * 16;
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) {
            const float4 b = *reinterpret_cast<const float4*>(bias + nb + 4 * nj);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[mi][nj] = f32x4{b.x, b.y, b.z, b.w};
        }
    };
    if (vb < total) init_acc(p.bias, vb);

    // fragments: step s of a sub-step uses Af[s] (and its scale byte As[s]) with the weight set Wf[s / MI]
    int4 Af[NS], Wf[2][4];
    unsigned As[NS];
    uint2 Wsc = make_uint2(0u, 0u), Wsn = make_uint2(0u, 0u);    // weight scales of this / the next FP4 sub-step: byte 2 nj + kk
    auto rdA = [&](const char* slot, int kk, int mi) { return *reinterpret_cast<const int4*>(slot + (a_v0 ^ (unsigned)(kk * 64)) + mi * 2048); };
    auto rdW = [&](const char* slot, int kk, int nj) { return *reinterpret_cast<const int4*>(slot + (w_v0 ^ (unsigned)(kk * 64)) + nj * 512); };
    // activation scales: the array keeps [row][8 K-blocks]; this lane's block of a 128-wide MFMA is kq + 4 kk: a byte read
    auto rdAs = [&](const char* slot, int kk, int mi) { return (unsigned)*reinterpret_cast<const unsigned char*>(slot + sa_v + mi * 128 + kk * 4); };
    // weight scales: the host lays them out per 16-row block as [row & 3][kq][n-tile nj][kk] (network.permute_w_scales), so the
    // eight bytes a lane needs in a sub-step are ONE 8-byte read and the MFMA picks its byte with op_sel: no VALU, two registers
    auto rdWs = [&](const char* slot) { return *reinterpret_cast<const uint2*>(slot + sw_v); };

    int g = 0;                                                   // sub-steps consumed so far (ring position)
    bool w_sent = false;                                         // this wave has issued the weight burst of the current sub-step
    // KIND: 0 = f16 sub-step (K = 64), 1 = FP4 sub-step (K = 256, block scales); next_q: the sub-step that follows is an FP4 one
    // (run-time, uniform: it only decides whether scales are read ahead with the fragments -- TWO loop bodies in all, as in
    // k_gemm_ring_mx: with a body per (kind, next kind) pair hipcc moved the accumulators between two register sets).
    // One step = 4 MFMAs; S is a compile-time constant (op_sel immediates, static register indices).
    auto step = [&](auto kind_c, auto s_c, const bool next_q) __attribute__((always_inline)) {
        constexpr int KIND = decltype(kind_c)::value, S = decltype(s_c)::value;
        constexpr int kk = S / MI, mi = S % MI;
        const char* ab = lds + (g & 1) * A_BYTES;                // a_v0 / w_v0 / s*_v carry the region offsets
        const char* wb = lds + (g & 1) * W_BYTES;
        const char* sb = lds + (g & 1) * S_BYTES;
        const char* abn = lds + ((g + 1) & 1) * A_BYTES;
        const char* wbn = lds + ((g + 1) & 1) * W_BYTES;
        const char* sbn = lds + ((g + 1) & 1) * S_BYTES;
        auto readA = [&](int t) {                                // fragment (and scale byte) of step t of THIS sub-step
            Af[t] = rdA(ab, t / MI, t % MI);
            if (KIND == 1) As[t] = rdAs(sb, t / MI, t % MI);
        };
        auto readAn = [&](int t) {                               // ... of the NEXT sub-step (its slot, its kind)
            Af[t] = rdA(abn, t / MI, t % MI);
            As[t] = rdAs(sbn, t / MI, t % MI);                   // (unconditional: see Wsn below)
        };
        if (EW != EV && S == EW) {
            // complementary bursts: waves 0-3 send the ACTIVATION tile of the sub-step after next here, one event after waves 4-7
            // did (its slot was released at the previous main event; not in the very first sub-step: that tile is already in flight)
            if (LATE == 0 && !early && g > 0 && pt < total) issue_a();
            // weight-slot event: the last weight fragment of this slot was read at step 3, in front of at least one younger LDS
            // read (step 4: one fragment, and its scale byte in an FP4 sub-step), so lgkmcnt(1 / 2) retires every weight read
            if (KIND == 0) asm volatile("s_waitcnt lgkmcnt(1)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(2)\n\ts_barrier" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (early && pt < total) { issue_w(); w_sent = true; }
        }
        if (EW != EV && LATE != 0 && !early && S == EW + LATE && pt < total) {
            issue_w();
            w_sent = true;
        }
        if (S == EV) {
            // every read of this slot was issued >= 2 steps ago.  DMA: the only operations this wave may still have in flight
            // are the W_INSTR of the weight burst it issued a few steps ago (for the sub-step after next); everything older
            // -- both tiles of the next sub-step, epilogue stores -- is waited for
            if (EW != EV && LATE == 0 && !early && pt < total) {
                issue_w();
                w_sent = true;
            }
            // (no weight burst once the work has run out: then nothing may stay in flight)
            if (EW != EV && w_sent) asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(W_INSTR) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            w_sent = false;
            __builtin_amdgcn_sched_barrier(0);
            if (early && pt < total) { if (EW == EV) issue_w(); issue_a(); }
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) Wf[0][nj] = rdW(wbn, 0, nj);
            // Scales are read ahead whether or not the next sub-step is an FP4 one (then they are whatever the slot holds and nothing
            // uses them): a read under the run-time flag would keep Wsn / Wsc / As[0 .. 2] LIVE through every f16 sub-step (seven
            // registers hipcc spilled to scratch and reloaded inside the hand-counted stream); four LDS reads per sub-step are free.
            Wsn = rdWs(sbn);
            readAn(0);
        }
        if (!early && (EW == EV || LATE != 0) && S == EV + LATE && pt < total) {
            if (EW == EV) issue_w();
            issue_a();
        }
        // activation fragments: D steps ahead, one per step -- the last one of the slot at step EV - 1, the first of the next slot
        // right behind the event
        if (S + D < NS) readA(S + D);
        if (S >= EV && S + 1 < NS) readAn(S - EV + 1);
        // weight fragments of the second K half
        if constexpr (MI == 8 && S < 4) Wf[1][S] = rdW(wb, 1, S);
        if constexpr (MI == 4 && S < 2) { Wf[1][2 * S] = rdW(wb, 1, 2 * S); Wf[1][2 * S + 1] = rdW(wb, 1, 2 * S + 1); }
        if (KIND == 0) {
            const v8 af = __builtin_bit_cast(v8, Af[S]);
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = Half16<H>::mfma(__builtin_bit_cast(v8, Wf[kk][nj]), af, acc[mi][nj]);
        } else {
            const v8i xa = {Af[S].x, Af[S].y, Af[S].z, Af[S].w, 0, 0, 0, 0};
            const int as = (int)As[S];
#define AVL_QMFMA(NJ)                                                                                                              \
    do {                                                                                                                           \
        const v8i wa = {Wf[kk][NJ].x, Wf[kk][NJ].y, Wf[kk][NJ].z, Wf[kk][NJ].w, 0, 0, 0, 0};                                       \
        const int ws = (int)((NJ) < 2 ? Wsc.x : Wsc.y);                                                                            \
        acc[mi][NJ] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa, xa, acc[mi][NJ], 4, 4, ((NJ) & 1) * 2 + kk, ws, 0, as);      \
    } while (0)
            AVL_QMFMA(0); AVL_QMFMA(1); AVL_QMFMA(2); AVL_QMFMA(3);
#undef AVL_QMFMA
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto substep = [&](auto kind_c, const bool next_q) __attribute__((always_inline)) {
#define AVL_STEP(N) step(kind_c, std::integral_constant<int, N>(), next_q)
        AVL_STEP(0); AVL_STEP(1); AVL_STEP(2); AVL_STEP(3); AVL_STEP(4); AVL_STEP(5); AVL_STEP(6); AVL_STEP(7);
        if constexpr (NS == 16) { AVL_STEP(8); AVL_STEP(9); AVL_STEP(10); AVL_STEP(11); AVL_STEP(12); AVL_STEP(13); AVL_STEP(14); AVL_STEP(15); }
#undef AVL_STEP
        Wsc = Wsn;                                               // (a move only where the next sub-step is an FP4 one)
        ++g;
    };
    typedef std::integral_constant<int, 0> F16;
    typedef std::integral_constant<int, 1> FP4;

    // prologue: this wave's share of sub-step 0 (and 1) has landed, then everyone's
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int t = vb; t < total; t += nwg) {
        const int nt = t % ntiles, mt = t / ntiles;
        {   // cold start of the tile: the first fragments of its first sub-step (an f16 one; its slot was certified by the previous
            // event, or by the prologue barrier).  The fragments the last sub-step of the previous tile read ahead are not kept
            // across the epilogue (registers), they are simply read again.
            const char* ab = lds + (g & 1) * A_BYTES;
            const char* wb = lds + (g & 1) * W_BYTES;
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) Wf[0][nj] = rdW(wb, 0, nj);
#pragma unroll
            for (int s = 0; s < D; ++s) Af[s] = rdA(ab, 0, s);
        }
        for (int mb = 0; mb < nmb; ++mb) {
            for (int j = 0; j < 4; ++j) substep(F16(), j == 3);
            for (int u = 0; u < nmx; ++u) substep(FP4(), u + 1 < nmx);
        }
        // What only the epilogue uses (output and residual planes, their FP4 planes, scale slabs and strides, the bias) is not held
        // in scalar registers across the stream -- with the producer's state that is more than the 100-odd a wave has, and hipcc
        // then keeps the excess in the lanes of two vector registers and reads them back one v_readlane at a time, inside the stream
        // too.  The tile's epilogue reads the argument struct again, from the kernel-argument segment it was passed in (`q` is the
        // kernel's first argument: offset 0), through a pointer the compiler cannot see through, so the scalar loads stay here,
        // behind the last MFMA in program text (tests/test_abi.py forbids them inside the stream).
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        // (a COPY, made here: every field the epilogue uses is loaded once per tile, in front of the eight rounds -- through the bare
        // pointer hipcc may not read ahead of the rounds' conditions and would load fields again in every round)
        const MxArgs qe = *(const MxArgs*)ka;
        mx_epilogue<IO, MI>(qe, acc, nt, mt, wm, wn, fr, kq);
        if (t + nwg < total) init_acc(qe.g.bias, t + nwg);
        read_args();
    }
}

template <int MI> constexpr int MX_LDS = 2 * (2 * MI * 16 + 256) * 128 + 2 * 4096;

template <int IO, int MI>
int launch_ring_mx(const MxArgs& a, const avl_gemm_route& r, hipStream_t s) {
    AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_ring_mx<IO, MI>), hipFuncAttributeMaxDynamicSharedMemorySize, MX_LDS<MI>));
    hipLaunchKernelGGL((k_gemm_ring_mx<IO, MI>), dim3(r.workgroups), dim3(512), MX_LDS<MI>, s, a, r.m_tiles);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// LATE: how many steps behind the event(s) waves 0-3 issue their bursts (waves 4-7: right behind them)
template <int IO, int MI, int LATE>
int launch_mx_pipe(const MxArgs& a, const avl_gemm_route& r, hipStream_t s) {
    // k_gemm_mx_pipe finds strides and planes from each operand's K and the base of its bundle (see its set_input / set_tile)
    const long long K = a.g.K, K1 = (long long)a.nmb1 * 256, K2 = K - K1;
    auto bundle_ok = [&](const char* const* bq, const char* const* bs, long long rows, long long ch) {
        const long long P = mx_plane_bytes(rows, ch), S = mx_scale_bytes(rows, ch);
        return bs[0] - bq[0] == P && (a.nmx < 2 || (bq[1] - bq[0] == P + S && bs[1] - bq[0] == 2 * P + S)) && 2 * (P + S) < (1LL << 32);
    };
    AVL_REQUIRE(a.g.lda == K1 && a.ldaq == K1 / 2 && bundle_ok(a.Aq, a.As, a.a_srows, K1), "MX GEMM: first input is not dense rows + a bundle");
    AVL_REQUIRE(K2 == 0 || (a.lda2 == K2 && a.ldaq2 == K2 / 2 && a.a_srows2 == a.a_srows && bundle_ok(a.Aq2, a.As2, a.a_srows, K2)),
                "MX GEMM: second input is not dense rows + a bundle of the first input's rows");
    AVL_REQUIRE(bundle_ok(a.Wq, a.Ws, a.w_srows, K), "MX GEMM: weights are not a bundle");
    AVL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_mx_pipe<IO, MI, LATE>), hipFuncAttributeMaxDynamicSharedMemorySize, MX_LDS<MI>));
    hipLaunchKernelGGL((k_gemm_mx_pipe<IO, MI, LATE>), dim3(r.workgroups), dim3(512), MX_LDS<MI>, s, a, r.m_tiles);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

// A GEMM with a per-image bias runs as one batch-1 GEMM per image: the op of image n (pointers at its first row, the rows that
// follow it, its bias vector).
avl_seg_op gemm_image_op(const avl_seg_op& op, int n) {
    avl_seg_op v = op;
    const long long m = (long long)op.out_h * op.out_w * n;
    const int es = elem_size(op.dtype), oes = op.out_f32 ? 4 : es;
    auto at = [](const void* p, long long bytes) -> const void* { return p ? static_cast<const char*>(p) + bytes : p; };
    v.in = at(op.in, m * op.in_ld * es);
    v.in_lo = at(op.in_lo, m * op.in_ld * es);
    v.in2 = at(op.in2, m * op.in2_ld * es);
    v.in2_lo = at(op.in2_lo, m * op.in2_ld * es);
    v.out = const_cast<void*>(at(op.out, m * op.out_ld * oes));
    v.out_lo = const_cast<void*>(at(op.out_lo, m * op.out_ld * es));
    if (op.out_f32) v.out_mx = const_cast<void*>(at(op.out_mx, m));         // the uint8 labels of the fused arg-max
    v.bias = op.bias + (long long)n * op.w_rows;
    v.in_rows = (int)(op.in_rows - m);
    v.out_rows = (int)(op.out_rows - m);
    v.batch = 1;
    v.bias_per_image = 0;
    return v;
}

inline bool per_image_launches(const avl_seg_op& op) { return op.bias_per_image && op_batch(op) > 1; }

// Which kernel an op runs, on which tiles and grid: the ONE place that decides it.  validate_gemm and launch_gemm both start here,
// avl_seg_gemm_route hands it out, and include/avl_hip.h states the rule as a table (keep the two in step).  Why the thresholds:
//   * tile choices count ONE image's rows, so that a batch runs the kernel its batch-1 plan runs;
//   * MX: 128-row tiles where 256-row tiles would leave more than a quarter of the 256 CUs idle or give a ragged second wave.  The
//     software-pipelined stream wins where the K loop is long (K >= 1024: -2...-9 % on layer4 / layer3 conv1 and conv3 + downsample),
//     the ring kernel (two plain barriers per sub-step, a cheaper tile switch) where a tile is only 1-2 K macro-blocks (K = 256 /
//     512: layer2, layer3 conv3, the decoder's pointwise convs: the stream is +2...+19 % there); profiles/r03/gemm_mx_pipe_vs_ring_ab.log;
//   * ring: 256 x 256 halves the L2->LDS bytes per flop (the measured limiter) but needs >= ~200 tiles to fill 256 CUs.
avl_gemm_route gemm_route(const avl_seg_op& op0) {
    const avl_seg_op op = per_image_launches(op0) ? gemm_image_op(op0, 0) : op0;
    avl_gemm_route r;
    memset(&r, 0, sizeof(r));
    r.launches = per_image_launches(op0) ? op0.batch : 1;
    r.ext = op.stride > 1 || op.out2 != nullptr || op.out2_lo != nullptr || op.n_split != 0;
    const int m_image = op.out_h * op.out_w, M = m_image * op_batch(op), N = op.out_c;
    const long long t256 = (long long)((m_image + 255) / 256) * (N / 256);
    const bool can256 = N % 256 == 0 && op.w_rows % 256 == 0;
    if (op.w_split != 2) r.nsub = op.w_split ? (op.in_lo ? 3 : 2) : 1;      // passes per K block: weights split, input split too
    if (op.w_split == 2) {
        const int K = op.in_c + (op.in3 ? op.in3_c : 0);
        r.kernel = K >= 1024 ? AVL_GEMM_MX_PIPE : AVL_GEMM_RING_MX;
        r.dtype = AVL_F16;
        r.io = op.out_mx != nullptr;
        r.mi = (t256 < 192 || (t256 > 256 && t256 < 384)) ? 4 : 8;
        r.late = (r.kernel == AVL_GEMM_MX_PIPE && r.mi == 4) ? 1 : 0;
        r.tile_m = r.mi * 32;
        r.tile_n = 256;
    } else if (is_half(op.dtype) && op.w_layout != 1 && N > 64 && !op.out_f32 && N % 128 == 0 && op.in_rows >= (M + 255) / 256 * 256) {
        r.kernel = AVL_GEMM_RING;
        r.io = r.nsub > 1;
        r.dtype = r.nsub > 1 ? AVL_F16 : op.dtype;
        int v = op.w_layout;        // 0 = by shape, 2 = 256 x 128, 3 = 256 x 256, 4 = 256 x 128 on four waves
        if (v == 0) v = (can256 && t256 >= 192) ? 3 : 2;
        if (v == 3) v = can256 ? 3 : 2;
        if (v == 3) { r.wm = 2; r.wn = 4; r.mi = 8; r.stages = r.nsub == 2 ? 3 : 2; r.ast = 2; }
        else if (v == 4 && r.nsub == 1) { r.wm = 2; r.wn = 2; r.mi = 8; r.stages = 3; r.ast = 3; }
        else { r.wm = 4; r.wn = 2; r.mi = 4; r.stages = 3; r.ast = 3; }
        r.tile_m = r.wm * r.mi * 16;
        r.tile_n = r.wn * 64;
    } else {
        r.kernel = AVL_GEMM_PLAIN;
        r.dtype = is_half(op.dtype) ? op.dtype : AVL_F32;
        r.wm = N <= 64 ? 4 : 2;
        r.wn = N <= 64 ? 1 : 2;
        r.tile_m = r.wm * 64;
        r.tile_n = r.wn * 64;
    }
    r.m_tiles = (M + r.tile_m - 1) / r.tile_m;
    r.n_tiles = (N + r.tile_n - 1) / r.tile_n;
    const long long total = (long long)r.m_tiles * r.n_tiles;
    r.workgroups = (int)(r.kernel != AVL_GEMM_PLAIN && total > 256 ? 256 : total);
    return r;
}

// Every instantiation the library holds, once: the route's kernel, element type and template arguments, and its launcher.  A ring
// kernel stands with its EXT twin (strided input rows / a second destination), which the four-wave configuration does not have.
// (The rows' order is the order hipcc lays the kernels out in the code object; it is the one they had before this table existed, so
// that tools/device_code_diff.py shows the library's device code unmoved, the kernels' places in it included.)
typedef int (*GemmLauncher)(const GemmArgs&, const avl_gemm_route&, hipStream_t, const RingExt&);
typedef int (*MxLauncher)(const MxArgs&, const avl_gemm_route&, hipStream_t);
struct GemmKernel {
    int kernel, dtype, wm, wn, mi, stages, nsub, io, ast, late;
    GemmLauncher launch, launch_ext;
    MxLauncher launch_mx;
};
template <typename T> constexpr int DTYPE = std::is_same<T, float>::value ? AVL_F32 : std::is_same<T, bf16>::value ? AVL_BF16 : AVL_F16;
template <typename H, int WM, int WN, int MI, int STAGES, int NSUB, int IO, int AST, bool TWIN>
constexpr GemmKernel ring_kernel() {
    GemmLauncher ext = nullptr;
    if constexpr (TWIN) ext = &launch_ring<H, WM, WN, MI, STAGES, NSUB, IO, AST, true>;
    return {AVL_GEMM_RING, DTYPE<H>, WM, WN, MI, STAGES, NSUB, IO, AST, 0, &launch_ring<H, WM, WN, MI, STAGES, NSUB, IO, AST, false>, ext, nullptr};
}
template <typename T, int WM, int WN>
constexpr GemmKernel plain_kernel() { return {AVL_GEMM_PLAIN, DTYPE<T>, WM, WN, 0, 0, 0, 0, 0, 0, &launch_plain<T, WM, WN>, nullptr, nullptr}; }
template <int IO, int MI>
constexpr GemmKernel ring_mx_kernel() { return {AVL_GEMM_RING_MX, AVL_F16, 0, 0, MI, 0, 0, IO, 0, 0, nullptr, nullptr, &launch_ring_mx<IO, MI>}; }
template <int IO, int MI, int LATE>
constexpr GemmKernel mx_pipe_kernel() { return {AVL_GEMM_MX_PIPE, AVL_F16, 0, 0, MI, 0, 0, IO, 0, LATE, nullptr, nullptr, &launch_mx_pipe<IO, MI, LATE>}; }

const GemmKernel GEMM_KERNELS[] = {
    //             IO MI LATE                      IO MI
    mx_pipe_kernel<1, 4, 1>(), ring_mx_kernel<1, 4>(), mx_pipe_kernel<0, 4, 1>(), ring_mx_kernel<0, 4>(),       // 128 x 256
    mx_pipe_kernel<1, 8, 0>(), ring_mx_kernel<1, 8>(), mx_pipe_kernel<0, 8, 0>(), ring_mx_kernel<0, 8>(),       // 256 x 256
    //          T     WM WN MI STAGES NSUB IO AST  EXT twin
    ring_kernel<f16,  2, 4, 8, 3,     2,   1, 2,   true>(),     // split operands: 256 x 256 and 256 x 128, two passes, then three
    ring_kernel<f16,  4, 2, 4, 3,     2,   1, 3,   true>(),
    ring_kernel<f16,  2, 4, 8, 2,     3,   1, 2,   true>(),
    ring_kernel<f16,  4, 2, 4, 3,     3,   1, 3,   true>(),
    ring_kernel<bf16, 2, 4, 8, 2,     1,   0, 2,   true>(),     // one plane: 256 x 256
    ring_kernel<f16,  2, 4, 8, 2,     1,   0, 2,   true>(),
    ring_kernel<bf16, 2, 2, 8, 3,     1,   0, 3,   false>(),    // 256 x 128 on four waves
    ring_kernel<f16,  2, 2, 8, 3,     1,   0, 3,   false>(),
    ring_kernel<bf16, 4, 2, 4, 3,     1,   0, 3,   true>(),     // 256 x 128
    ring_kernel<f16,  4, 2, 4, 3,     1,   0, 3,   true>(),
    //           T      WM WN: 256 x 64, 128 x 128
    plain_kernel<bf16,  4, 1>(), plain_kernel<bf16,  2, 2>(),
    plain_kernel<f16,   4, 1>(), plain_kernel<f16,   2, 2>(),
    plain_kernel<float, 4, 1>(), plain_kernel<float, 2, 2>(),
};

const GemmKernel* find_kernel(const avl_gemm_route& r) {
    for (const GemmKernel& k : GEMM_KERNELS)
        if (k.kernel == r.kernel && k.dtype == r.dtype && k.wm == r.wm && k.wn == r.wn && k.mi == r.mi && k.stages == r.stages &&
            (k.kernel != AVL_GEMM_RING || k.nsub == r.nsub) && k.io == r.io && k.ast == r.ast && k.late == r.late && (!r.ext || k.launch_ext))
            return &k;
    return nullptr;
}

}  // namespace

int validate_gemm(const avl_seg_op& op) {
    const int es = elem_size(op.dtype);
    const avl_gemm_route route = gemm_route(op);
    AVL_REQUIRE(is_half(op.dtype) || op.dtype == AVL_F32, "GEMM dtype %d", op.dtype);
    AVL_REQUIRE(op.in && op.out && op.weight && op.bias, "GEMM has NULL buffers");
    // (checked here, not only at launch: a plan that cannot run is refused when it is created)
    AVL_REQUIRE(op.w_layout >= 0 && op.w_layout <= 4, "GEMM w_layout %d (0 = by shape, 1 .. 4 = a forced 16-bit tile configuration)", op.w_layout);
    AVL_REQUIRE(op.w_layout == 0 || is_half(op.dtype), "GEMM w_layout %d forces a tile configuration of the 16-bit kernels: dtype %d", op.w_layout, op.dtype);
    if (per_image_launches(op)) {
        AVL_REQUIRE(op.w_split != 2 && !op.in3, "GEMM: a per-image bias is not supported by the MX GEMM");
        // (gemm_image_op moves neither out2 nor a strided input to image n)
        AVL_REQUIRE(!route.ext, "GEMM: a per-image bias goes with neither strided input rows (stride %d) nor a second destination", op.stride);
        for (int n = 0; n < op.batch; ++n) {
            const avl_seg_op v = gemm_image_op(op, n);
            AVL_REQUIRE(v.in_rows >= (op.out_h * op.out_w + 255) / 256 * 256,
                        "GEMM with a per-image bias: image %d has %d input rows behind its first (the last image needs whole 256-row tiles)", n, v.in_rows);
            const int rc = validate_gemm(v);
            if (rc) return rc;
        }
        return AVL_OK;
    }
    const int M = op.out_h * op.out_w * op_batch(op), K = op.in_c, N = op.out_c;      // a batch is one long run of rows
    AVL_REQUIRE(M > 0 && N > 0 && K > 0, "GEMM M/N/K = %d/%d/%d", M, N, K);
    if (route.ext) {        // strided input rows / a second destination: the ring GEMM of the 16-bit types only
        AVL_REQUIRE(op.w_split != 2 && !op.in3, "GEMM: the MX GEMM takes neither strided input rows (stride %d) nor a second destination", op.stride);
        AVL_REQUIRE(is_half(op.dtype) && !op.out_f32, "GEMM: strided input rows (stride %d) / a second destination need a 16-bit GEMM (dtype %d, out_f32 %d)",
                    op.stride, op.dtype, op.out_f32);
        AVL_REQUIRE(route.kernel == AVL_GEMM_RING && op.w_layout != 4, "GEMM: strided input rows (stride %d) / a second destination need the ring GEMM "
                    "(N %% 128 == 0, N > 64, rows padded to 256, w_layout 0, 2 or 3): N %d, in_rows %d, w_layout %d", op.stride, N, op.in_rows, op.w_layout);
    }
    if (op.stride > 1) {
        AVL_REQUIRE(op.out_h == (op.in_h - 1) / op.stride + 1 && op.out_w == (op.in_w - 1) / op.stride + 1,
                    "GEMM stride %d: output %d x %d is not the sub-sampled %d x %d input", op.stride, op.out_h, op.out_w, op.in_h, op.in_w);
        AVL_REQUIRE((long long)op.in_rows >= (long long)op.in_h * op.in_w * op_batch(op), "GEMM stride %d reads %lld rows, input has %d allocated",
                    op.stride, (long long)op.in_h * op.in_w * op_batch(op), op.in_rows);
    } else
        AVL_REQUIRE(op.in_h * op.in_w == op.out_h * op.out_w, "GEMM in/out pixel counts differ (%d vs %d)", op.in_h * op.in_w, op.out_h * op.out_w);
    AVL_REQUIRE((K * es) % 128 == 0, "GEMM K = %d is not a multiple of %d", K, 128 / es);
    AVL_REQUIRE(op.in_ld >= K && (op.in_ld * es) % 16 == 0, "GEMM in_ld %d", op.in_ld);
    int n1 = N;             // columns that go to `out`
    if (op.out2 || op.out2_lo || op.n_split) {
        const int bn = route.tile_n;
        AVL_REQUIRE(op.out2, "GEMM: n_split %d / out2_lo without a second destination (out2 is NULL)", op.n_split);
        AVL_REQUIRE(op.n_split > 0 && op.n_split < N && op.n_split % bn == 0,
                    "GEMM: n_split %d must be a multiple of the N tile (%d) inside (0, N = %d)", op.n_split, bn, N);
        AVL_REQUIRE(!op.in2, "GEMM: a second destination takes no residual");
        AVL_REQUIRE(op.out2_ld >= N - op.n_split && (op.out2_ld * es) % 16 == 0, "GEMM out2_ld %d (second destination of %d columns)", op.out2_ld, N - op.n_split);
        AVL_REQUIRE(!op.out2_lo || (op.dtype == AVL_F16 && op.w_split == 1), "GEMM: out2_lo needs AVL_F16 activations and w_split = 1");
        AVL_REQUIRE((reinterpret_cast<uintptr_t>(op.out2) | reinterpret_cast<uintptr_t>(op.out2_lo)) % 16 == 0, "GEMM second destination must be 16-byte aligned");
        n1 = op.n_split;
    }
    AVL_REQUIRE(op.out_ld >= n1, "GEMM out_ld %d < N %d", op.out_ld, n1);
    const int rows_read = route.m_tiles * route.tile_m, w_rows_read = route.n_tiles * route.tile_n;
    AVL_REQUIRE(op.in_rows >= rows_read, "GEMM reads %d rows, input has %d allocated", rows_read, op.in_rows);
    AVL_REQUIRE(op.w_rows >= w_rows_read, "GEMM reads %d weight rows, %d allocated", w_rows_read, op.w_rows);
    AVL_REQUIRE(op.out_rows >= M, "GEMM writes %d rows, output has %d", M, op.out_rows);
    if (!op.out_f32) AVL_REQUIRE((op.out_ld * es) % 16 == 0 && N % 16 == 0, "GEMM out_ld %d / N %d not 16-aligned", op.out_ld, N);
    if (op.in2) AVL_REQUIRE(op.in2_ld >= N && (op.in2_ld * es) % 16 == 0, "GEMM residual ld %d", op.in2_ld);
    if (op.out_f32) AVL_REQUIRE(!op.out_lo, "GEMM: an fp32 output has no low plane");
    if (op.out_f32 && op.out_mx)      // the fused arg-max (labels through out_mx): the small-N kernel, plain logits
        AVL_REQUIRE(N <= 32 && !op.in2 && !op.relu && route.kernel == AVL_GEMM_PLAIN && route.tile_n == 64,
                    "GEMM: an arg-max output (out_f32 with out_mx = uint8 labels[rows]) needs N <= 32, no residual, no ReLU (N %d)", N);
    if (op.w_split == 2) {
        AVL_REQUIRE(op.dtype == AVL_F16 && op.w_mx && op.in_mx, "MX GEMM needs AVL_F16 activations and the w_mx / in_mx bundles");
        AVL_REQUIRE(K % 256 == 0 && N % 256 == 0 && op.w_rows % 256 == 0 && op.w_rows >= N, "MX GEMM: K %d, N %d, w_rows %d must be multiples of 256", K, N, op.w_rows);
        AVL_REQUIRE(op.in_ld == K && op.in_rows % 256 == 0 && op.in_rows >= M, "MX GEMM input must be dense rows padded to 256 (ld %d, rows %d)", op.in_ld, op.in_rows);
        AVL_REQUIRE(!op.out_f32 && op.out_ld >= N && (op.out_ld * 2) % 16 == 0, "MX GEMM output");
        AVL_REQUIRE(!op.out_mx || op.out_ld == N, "MX GEMM can only quantise a dense output (out_ld %d, N %d)", op.out_ld, N);
        AVL_REQUIRE(!(op.mx_flags & AVL_MX_RES_LO) || (op.in2 && op.in2_mx && !op.in2_lo && op.in2_ld == N),
                    "AVL_MX_RES_LO needs in2, in2_mx (bundle of a dense [out_rows][N] residual) and no in2_lo");
        AVL_REQUIRE(!(op.mx_flags & AVL_MX_OUT_LO) || op.out_mx, "AVL_MX_OUT_LO without out_mx");
        AVL_REQUIRE(!(op.mx_flags & AVL_MX_IN_LO) || !op.in_lo, "AVL_MX_IN_LO together with in_lo");
        if (op.in3) {
            AVL_REQUIRE(op.in3_mx && op.in3_c > 0 && op.in3_c % 256 == 0 && op.in3_ld == op.in3_c,
                        "second GEMM input: in3_mx, in3_c %d (multiple of 256), dense rows (in3_ld %d)", op.in3_c, op.in3_ld);
            AVL_REQUIRE(!op.in_lo || (op.mx_flags & AVL_MX_IN_LO), "a second GEMM input needs both inputs' lo parts in their bundles (AVL_MX_IN_LO) or none");
            AVL_REQUIRE((reinterpret_cast<uintptr_t>(op.in3) | reinterpret_cast<uintptr_t>(op.in3_mx)) % 16 == 0, "second GEMM input must be 16-byte aligned");
        }
        AVL_REQUIRE((long long)op.in_rows * K * 2 < 0xffffff00LL && (long long)op.w_rows * K * 2 < 0xffffff00LL, "MX GEMM operand larger than 4 GB");
        AVL_REQUIRE((long long)op.out_rows * op.out_ld * 2 < (1LL << 31) && (!op.in2 || (long long)op.out_rows * op.in2_ld * 2 < (1LL << 31)) &&
                    (long long)(N / 256 + 1) * op.out_rows * 8 < (1LL << 31), "MX GEMM output / residual plane beyond 2 GB (32-bit epilogue addressing)");
        AVL_REQUIRE((reinterpret_cast<uintptr_t>(op.w_mx) | reinterpret_cast<uintptr_t>(op.in_mx) | reinterpret_cast<uintptr_t>(op.out_mx) |
                     reinterpret_cast<uintptr_t>(op.in_lo) | reinterpret_cast<uintptr_t>(op.in2_lo) | reinterpret_cast<uintptr_t>(op.out_lo)) % 16 == 0,
                    "MX GEMM bundles / low planes must be 16-byte aligned");
    } else if (op.w_split || op.in_lo || op.in2_lo || op.out_lo) {
        AVL_REQUIRE(op.dtype == AVL_F16 && op.w_split == 1, "split (hi + lo) operands need AVL_F16 activations and w_split = 1");
        AVL_REQUIRE(!op.in2_lo || op.in2, "in2_lo without in2");
        AVL_REQUIRE((reinterpret_cast<uintptr_t>(op.in_lo) | reinterpret_cast<uintptr_t>(op.in2_lo) | reinterpret_cast<uintptr_t>(op.out_lo)) % 16 == 0,
                    "GEMM low planes must be 16-byte aligned");
        if (op.in2_lo || op.out_lo)
            AVL_REQUIRE(route.kernel == AVL_GEMM_RING, "split residual / output need the ring GEMM (N %% 128 == 0, 16-bit output, rows padded to 256)");
    }
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(op.in) | reinterpret_cast<uintptr_t>(op.weight) | reinterpret_cast<uintptr_t>(op.out) |
                 reinterpret_cast<uintptr_t>(op.bias) | reinterpret_cast<uintptr_t>(op.in2)) % 16 == 0,
                "GEMM buffers must be 16-byte aligned");
    return AVL_OK;
}

int launch_gemm(const avl_seg_op& op, hipStream_t s) {
    if (per_image_launches(op)) {
        for (int n = 0; n < op.batch; ++n) {
            const int rc = launch_gemm(gemm_image_op(op, n), s);
            if (rc) return rc;
        }
        return AVL_OK;
    }
    const avl_gemm_route route = gemm_route(op);
    const GemmKernel* kernel = find_kernel(route);
    if (!kernel) return set_error(AVL_E_UNSUPPORTED, "GEMM: the library holds no kernel for this op's route (kernel %d, dtype %d, w_layout %d, ext %d)",
                                  route.kernel, route.dtype, op.w_layout, route.ext);
    GemmArgs a;
    a.A = op.in; a.W = op.weight; a.bias = op.bias; a.R = op.in2; a.C = op.out;
    a.lda = op.in_ld; a.ldr = op.in2_ld; a.ldc = op.out_ld;
    a.M = op.out_h * op.out_w * op_batch(op); a.N = op.out_c; a.K = op.in_c;
    a.relu = op.relu; a.out_f32 = op.out_f32;
    a.ntiles = route.n_tiles;
    if (kernel->launch_mx) {
        MxArgs mx;
        memset(&mx, 0, sizeof(mx));
        a.nsub = 1;
        a.a_lo_delta = 0;
        a.R_lo = op.in2_lo; a.C_lo = op.out_lo;
        mx.g = a;
        mx.stagger = 1;     // a kernel argument, not a constant: folding it into the kernels changes their code (SGPR spills)
        // (with a second input appended along K: K1 = op.in_c comes from `in`, the rest from in3; weights span the whole K)
        const long long K1 = op.in_c, K2 = op.in3 ? op.in3_c : 0;
        const auto x = mx_bundle(op.in_mx, op.in_rows, K1);
        mx.Aq[0] = x.q[0]; mx.As[0] = x.s[0]; mx.Aq[1] = x.q[1]; mx.As[1] = x.s[1];
        mx.ldaq = x.ldq; mx.a_srows = x.srows;
        mx.nmb1 = (int)(K1 / 256);
        mx.lda2 = mx.g.lda; mx.ldaq2 = x.ldq;
        if (K2) {
            a.K = (int)(K1 + K2);
            mx.g.K = a.K;
            const auto x2 = mx_bundle(op.in3_mx, op.in_rows, K2);
            mx.A2 = op.in3; mx.lda2 = op.in3_ld; mx.ldaq2 = x2.ldq;
            mx.Aq2[0] = x2.q[0]; mx.As2[0] = x2.s[0]; mx.Aq2[1] = x2.q[1]; mx.As2[1] = x2.s[1];
            mx.a_srows2 = x2.srows;
        }
        const auto w = mx_bundle(op.w_mx, op.w_rows, K1 + K2);
        mx.Wq[0] = w.q[0]; mx.Ws[0] = w.s[0]; mx.Wq[1] = w.q[1]; mx.Ws[1] = w.s[1];
        mx.w_srows = w.srows;
        mx.nmx = (op.in_lo || (op.mx_flags & AVL_MX_IN_LO)) ? 2 : 1;
        if (op.mx_flags & AVL_MX_RES_LO) {
            const auto r = mx_bundle(op.in2_mx, op.out_rows, a.N);
            mx.Rq = r.q[1]; mx.Rs = r.s[1];
            mx.ldrq = r.ldq; mx.r_srows = r.srows;
        }
        if (op.out_mx) {
            const auto c = mx_bundle(op.out_mx, op.out_rows, a.N);
            mx.Cq[0] = c.q[0]; mx.Cs[0] = c.s[0];
            if (op.out_lo || (op.mx_flags & AVL_MX_OUT_LO)) { mx.Cq[1] = c.q[1]; mx.Cs[1] = c.s[1]; }
            mx.ldcq = c.ldq; mx.c_srows = c.srows;
        }
        return kernel->launch_mx(mx, route, s);
    }
    a.nsub = route.nsub;
    a.a_lo_delta = op.in_lo ? static_cast<const char*>(op.in_lo) - static_cast<const char*>(op.in) : 0;
    a.R_lo = op.in2_lo;
    a.C_lo = op.out_f32 ? op.out_mx : op.out_lo;      // (out_f32 ops have neither a low plane nor an MX bundle: out_mx carries the label map)
    // strided input rows and / or a second destination: the EXT twin of the same ring configuration
    RingExt ext;
    memset(&ext, 0, sizeof(ext));
    if (op.stride > 1) { ext.s = op.stride; ext.ow = op.out_w; ext.ohw = op.out_h * op.out_w; ext.w = op.in_w; ext.hw = op.in_h * op.in_w; }
    if (op.out2) { ext.n_split = op.n_split; ext.ldc2 = op.out2_ld; ext.C2 = op.out2; ext.C2_lo = op.out2_lo; }
    return (route.ext ? kernel->launch_ext : kernel->launch)(a, route, s, ext);
}

}  // namespace avl

extern "C" int avl_seg_gemm_route(const avl_seg_op* op, avl_gemm_route* out) {
    AVL_REQUIRE(op && out, "avl_seg_gemm_route: NULL argument");
    AVL_REQUIRE(op->kind == AVL_OP_GEMM, "avl_seg_gemm_route: op kind %d is not AVL_OP_GEMM", op->kind);
    *out = avl::gemm_route(*op);
    return AVL_OK;
}
