// The scrolling grid's one device operation: a table of tile jobs, executed by one kernel (not in the reference: its grid is the fixed
// rectangle of MAPPING.BOUNDARY, src/mapping.py:106-117, and a point outside it is dropped, :410-411).  A scroll of the window, the
// reload of stored tiles, the assembly of a site and a save all move whole tiles between the window's two buffers, the slabs of the
// tile store and an output region (vision_semantic_segmentation_amd/scroll.py builds and validates the tables; the rule: struct
// avl_tile_job in include/avl_hip.h).
//
//   k_tile_copy   one job = one tile of T rows of T * bytes_per_cell bytes, split over `split` workgroups by rows.  A wave takes one
//                 tile row at a time and its lanes walk the row contiguously, 16 bytes per lane (one global_load_dwordx4 and one
//                 global_store_dwordx4), 1024 bytes per wave and step; the trip count is the same for every lane and the tail of a
//                 row that is no multiple of 1024 bytes is predicated.  A job without a source stores the fill word.  The emptiness
//                 flag (some 32-bit word of the SOURCE differs from the fill word) is OR-ed in registers, reduced per wave by a
//                 ballot, and reaches memory as one integer atomic OR per wave that has something to say: the result does not depend
//                 on which workgroup finishes first.  No LDS, no barrier, no ordering between workgroups -- source and destination
//                 never alias (the window is double-buffered).
//
// The kernel does no arithmetic on the payload: a tile arrives byte for byte, a -0.0 is a non-fill word like any other.
#include "avl_tile_table.h"

namespace {

using namespace avl_tile_table;

__global__ void __launch_bounds__(kBlock) k_tile_copy(const avl_tile_job* __restrict__ jobs, int n_jobs, int split, int rows, int row_vecs,
                                                      uint32_t fill, int32_t* __restrict__ flags, int n_flags) {
    const int job_idx = (int)(blockIdx.x / (unsigned)split);
    const int part = (int)(blockIdx.x % (unsigned)split);
    if (job_idx >= n_jobs) return;
    const avl_tile_job job = jobs[job_idx];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const char* src = static_cast<const char*>(job.src);
    char* dst = static_cast<char*>(job.dst);
    const uint4 fill4 = make_uint4(fill, fill, fill, fill);
    bool differs = false;
    for (int r = part * kWaves + wave; r < rows; r += split * kWaves) {      // wave-uniform
        const uint4* s = src != nullptr ? reinterpret_cast<const uint4*>(src + (int64_t)r * job.src_pitch) : nullptr;
        uint4* d = reinterpret_cast<uint4*>(dst + (int64_t)r * job.dst_pitch);
        for (int c0 = 0; c0 < row_vecs; c0 += 64) {                           // the same trip count for every lane
            const int c = c0 + lane;
            if (c < row_vecs) {
                uint4 v = fill4;
                if (s != nullptr) {
                    v = s[c];
                    differs |= (v.x != fill) | (v.y != fill) | (v.z != fill) | (v.w != fill);   // differs_from, spelled out: the call swaps two ORs' operands
                }
                d[c] = v;
            }
        }
    }
    if (job.flag >= 0 && job.flag < n_flags) {                                // wave-uniform: the job is
        const bool any = __ballot(differs) != 0ull;
        if (any && lane == 0) atomicOr(&flags[job.flag], 1);
    }
}

}  // namespace

extern "C" {

int avl_tile_copy(const avl_tile_job* jobs_dev, int n_jobs, int tile_cells, int bytes_per_cell, uint32_t fill, int32_t* flags, int n_flags,
                  void* stream) {
    int split;
    const int rc = avl_tile_table::begin("avl_tile_copy", jobs_dev, n_jobs, tile_cells, bytes_per_cell, flags, n_flags, avl::as_stream(stream), &split);
    if (rc != AVL_OK || split == 0) return rc;
    const int row_vecs = tile_cells * bytes_per_cell / 16;
    hipLaunchKernelGGL(k_tile_copy, dim3((unsigned)n_jobs * (unsigned)split), dim3(kBlock), 0, avl::as_stream(stream), jobs_dev, n_jobs, split,
                       tile_cells, row_vecs, fill, flags, n_flags);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

}  // extern "C"
