// Merging sites: a table of tile jobs, executed by one kernel (not in the reference: it has one grid and one run).  A frame's
// contribution never reads the grid, so the sum of two sites is the site of all their frames; what the scrolling grid
// lacked is an operation that accumulates a tile into a tile where the tiles live -- the window buffer, a slab of the store -- instead
// of assembling rectangles (vision_semantic_segmentation_amd/scroll.py builds and validates the tables; the rule: struct
// avl_tile_job in include/avl_hip.h).
//
//   k_tile_merge<OP>   one job = one destination tile of T rows, split over `split` workgroups by rows, shaped like k_tile_copy: a wave
//                      takes one tile row at a time and its lanes walk it contiguously, 16 bytes per lane and memory instruction; the
//                      trip count is the same for every lane and the tail of a row is predicated.  The lane that loads a destination
//                      vector is the lane that stores it, so the destination is merged in place without any ordering.  A fresh job
//                      does not read its destination: the accumulator is the fill word.  In AVL_MERGE_ADD_F32_TO_F64 a lane's one
//                      16-byte source vector (four float32) feeds two destination vectors (four float64).  The flag (some 32-bit word of
//                      the RESULT differs from the fill word) is OR-ed in registers, reduced per wave by a ballot, and reaches memory as
//                      one integer atomic OR per wave that has something to say.  No LDS, no barrier, no ordering between workgroups.
//
// Every op is one IEEE or two's-complement operation per element; the translation unit is built with -ffp-contract=off like the other
// map kernels, although an add alone leaves nothing to contract.
#include "avl_tile_table.h"

namespace {

using namespace avl_tile_table;

__device__ __forceinline__ uint2 bits_of(double v) { return __builtin_bit_cast(uint2, v); }
__device__ __forceinline__ double f64_of(uint32_t lo, uint32_t hi) { return __builtin_bit_cast(double, make_uint2(lo, hi)); }
__device__ __forceinline__ uint32_t add_f32(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b));
}
__device__ __forceinline__ uint2 add_i64(uint32_t alo, uint32_t ahi, uint32_t blo, uint32_t bhi) {
    const uint64_t s = ((uint64_t)ahi << 32 | alo) + ((uint64_t)bhi << 32 | blo);          // two's complement: it wraps
    return make_uint2((uint32_t)s, (uint32_t)(s >> 32));
}

// acc (+) src for the ops whose source and destination elements have the same size
template <int OP>
__device__ __forceinline__ uint4 merge_vec(uint4 a, uint4 s) {
    if constexpr (OP == AVL_MERGE_ADD_F64) {
        const uint2 lo = bits_of(f64_of(a.x, a.y) + f64_of(s.x, s.y)), hi = bits_of(f64_of(a.z, a.w) + f64_of(s.z, s.w));
        return make_uint4(lo.x, lo.y, hi.x, hi.y);
    } else if constexpr (OP == AVL_MERGE_ADD_F32) {
        return make_uint4(add_f32(a.x, s.x), add_f32(a.y, s.y), add_f32(a.z, s.z), add_f32(a.w, s.w));
    } else if constexpr (OP == AVL_MERGE_ADD_I64) {
        const uint2 lo = add_i64(a.x, a.y, s.x, s.y), hi = add_i64(a.z, a.w, s.z, s.w);
        return make_uint4(lo.x, lo.y, hi.x, hi.y);
    } else if constexpr (OP == AVL_MERGE_ADD_I32) {
        return make_uint4(a.x + s.x, a.y + s.y, a.z + s.z, a.w + s.w);                      // unsigned: the wrap is defined
    } else if constexpr (OP == AVL_MERGE_MIN_I32) {
        return make_uint4((uint32_t)min((int32_t)a.x, (int32_t)s.x), (uint32_t)min((int32_t)a.y, (int32_t)s.y),
                          (uint32_t)min((int32_t)a.z, (int32_t)s.z), (uint32_t)min((int32_t)a.w, (int32_t)s.w));
    } else {
        static_assert(OP == AVL_MERGE_MAX_I32, "merge_vec: an op without a same-size form");
        return make_uint4((uint32_t)max((int32_t)a.x, (int32_t)s.x), (uint32_t)max((int32_t)a.y, (int32_t)s.y),
                          (uint32_t)max((int32_t)a.z, (int32_t)s.z), (uint32_t)max((int32_t)a.w, (int32_t)s.w));
    }
}

// acc + (double)src for two float32 of the source: one destination vector of AVL_MERGE_ADD_F32_TO_F64
__device__ __forceinline__ uint4 widen_vec(uint4 a, uint32_t s0, uint32_t s1) {
    const uint2 lo = bits_of(f64_of(a.x, a.y) + (double)__builtin_bit_cast(float, s0));
    const uint2 hi = bits_of(f64_of(a.z, a.w) + (double)__builtin_bit_cast(float, s1));
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// row_vecs: the 16-byte vectors of a SOURCE row (for AVL_MERGE_ADD_F32_TO_F64 the destination row has twice as many)
template <int OP>
__global__ void __launch_bounds__(kBlock) k_tile_merge(const avl_tile_job* __restrict__ jobs, int n_jobs, int split, int rows, int row_vecs,
                                                       uint32_t fill, int32_t* __restrict__ flags, int n_flags) {
    const int job_idx = (int)(blockIdx.x / (unsigned)split);
    const int part = (int)(blockIdx.x % (unsigned)split);
    if (job_idx >= n_jobs) return;
    const avl_tile_job job = jobs[job_idx];
    if (job.src == nullptr || job.dst == nullptr) return;                     // no such job in a validated table; wave-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const char* src = static_cast<const char*>(job.src);
    char* dst = static_cast<char*>(job.dst);
    const bool fresh = job.fresh != 0;                                         // wave-uniform: the job is
    const uint4 fill4 = make_uint4(fill, fill, fill, fill);
    bool differs = false;
    for (int r = part * kWaves + wave; r < rows; r += split * kWaves) {      // wave-uniform
        const uint4* s = reinterpret_cast<const uint4*>(src + (int64_t)r * job.src_pitch);
        uint4* d = reinterpret_cast<uint4*>(dst + (int64_t)r * job.dst_pitch);
        for (int c0 = 0; c0 < row_vecs; c0 += 64) {                           // the same trip count for every lane
            const int c = c0 + lane;
            if (c < row_vecs) {
                const uint4 v = s[c];
                if constexpr (OP == AVL_MERGE_ADD_F32_TO_F64) {
                    uint4 a0 = fill4, a1 = fill4;
                    if (!fresh) {
                        a0 = d[2 * c];
                        a1 = d[2 * c + 1];
                    }
                    a0 = widen_vec(a0, v.x, v.y);
                    a1 = widen_vec(a1, v.z, v.w);
                    differs |= differs_from(a0, fill);
                    differs |= differs_from(a1, fill);
                    d[2 * c] = a0;
                    d[2 * c + 1] = a1;
                } else {
                    uint4 a = fill4;
                    if (!fresh) a = d[c];
                    a = merge_vec<OP>(a, v);
                    differs |= differs_from(a, fill);
                    d[c] = a;
                }
            }
        }
    }
    if (job.flag >= 0 && job.flag < n_flags) {                                // wave-uniform: the job is
        const bool any = __ballot(differs) != 0ull;
        if (any && lane == 0) atomicOr(&flags[job.flag], 1);
    }
}

template <int OP>
void launch(const avl_tile_job* jobs_dev, int n_jobs, int split, int rows, int row_vecs, uint32_t fill, int32_t* flags, int n_flags,
            hipStream_t stream) {
    hipLaunchKernelGGL(k_tile_merge<OP>, dim3((unsigned)n_jobs * (unsigned)split), dim3(kBlock), 0, stream, jobs_dev, n_jobs, split, rows,
                       row_vecs, fill, flags, n_flags);
}

}  // namespace

extern "C" {

int avl_tile_merge(const avl_tile_job* jobs_dev, int n_jobs, int op, int tile_cells, int bytes_per_cell, uint32_t fill, int32_t* flags,
                   int n_flags, void* stream) {
    // this call's own conditions first, on the raw arguments: begin() zeroes the flags, and a refused call does no GPU work.  A
    // destination row that is no multiple of 16 bytes is begin()'s to name.
    AVL_REQUIRE(op >= AVL_MERGE_ADD_F64 && op <= AVL_MERGE_MAX_I32, "avl_tile_merge: op = %d (AVL_MERGE_ADD_F64 .. AVL_MERGE_MAX_I32)", op);
    const bool wide = op == AVL_MERGE_ADD_F64 || op == AVL_MERGE_ADD_I64 || op == AVL_MERGE_ADD_F32_TO_F64;
    AVL_REQUIRE(!wide || bytes_per_cell % 8 == 0, "avl_tile_merge: bytes_per_cell = %d is no multiple of 8, the element of op %d",
                bytes_per_cell, op);
    const int64_t dst_row = (int64_t)tile_cells * bytes_per_cell;
    const int64_t src_row = op == AVL_MERGE_ADD_F32_TO_F64 ? dst_row / 2 : dst_row;
    AVL_REQUIRE(dst_row % 16 != 0 || src_row % 16 == 0,
                "avl_tile_merge: a float32 source tile row of %d bytes (%d cells of %d / 2 bytes) is no multiple of 16 bytes", (int)src_row,
                tile_cells, bytes_per_cell);
    hipStream_t st = avl::as_stream(stream);
    int split;
    const int rc = avl_tile_table::begin("avl_tile_merge", jobs_dev, n_jobs, tile_cells, bytes_per_cell, flags, n_flags, st, &split);
    if (rc != AVL_OK || split == 0) return rc;
    const int row_vecs = (int)(src_row / 16);
    switch (op) {
        case AVL_MERGE_ADD_F64: launch<AVL_MERGE_ADD_F64>(jobs_dev, n_jobs, split, tile_cells, row_vecs, fill, flags, n_flags, st); break;
        case AVL_MERGE_ADD_F32: launch<AVL_MERGE_ADD_F32>(jobs_dev, n_jobs, split, tile_cells, row_vecs, fill, flags, n_flags, st); break;
        case AVL_MERGE_ADD_F32_TO_F64:
            launch<AVL_MERGE_ADD_F32_TO_F64>(jobs_dev, n_jobs, split, tile_cells, row_vecs, fill, flags, n_flags, st);
            break;
        case AVL_MERGE_ADD_I64: launch<AVL_MERGE_ADD_I64>(jobs_dev, n_jobs, split, tile_cells, row_vecs, fill, flags, n_flags, st); break;
        case AVL_MERGE_ADD_I32: launch<AVL_MERGE_ADD_I32>(jobs_dev, n_jobs, split, tile_cells, row_vecs, fill, flags, n_flags, st); break;
        case AVL_MERGE_MIN_I32: launch<AVL_MERGE_MIN_I32>(jobs_dev, n_jobs, split, tile_cells, row_vecs, fill, flags, n_flags, st); break;
        default: launch<AVL_MERGE_MAX_I32>(jobs_dev, n_jobs, split, tile_cells, row_vecs, fill, flags, n_flags, st); break;
    }
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

}  // extern "C"
