// What avl_tile_copy (seg_scroll.hip) and avl_tile_merge (seg_sitemerge.hip) share: a table of struct avl_tile_job on the device, one
// job = one tile of T rows split over `split` workgroups by rows, a wave per row, 16 bytes per lane, flags zeroed before the kernel.
#pragma once
#include "avl_common.h"

#include <cstdint>

namespace avl_tile_table {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTargetWorkgroups = 2048;                  // a one-tile-row scroll (20 jobs) is split until the machine is full
constexpr int kMaxBytesPerCell = 128;

__device__ __forceinline__ bool differs_from(uint4 v, uint32_t fill) { return (v.x != fill) | (v.y != fill) | (v.z != fill) | (v.w != fill); }

// The host-side start of both calls, `who` the caller's name: AVL_E_ARG for an argument outside what include/avl_hip.h states for
// avl_tile_copy, else flags[0 .. n_flags) zeroed on `stream` and *split = the workgroups per tile, 0 for a table without jobs (nothing
// to launch).
inline int begin(const char* who, const avl_tile_job* jobs_dev, int n_jobs, int tile_cells, int bytes_per_cell, int32_t* flags, int n_flags,
                 hipStream_t stream, int* split) {
    *split = 0;
    AVL_REQUIRE(n_jobs >= 0 && n_jobs <= (1 << 20), "%s: n_jobs = %d (0 .. 2^20)", who, n_jobs);
    AVL_REQUIRE(n_flags >= 0, "%s: n_flags = %d", who, n_flags);
    AVL_REQUIRE(tile_cells >= 1 && tile_cells <= (1 << 14), "%s: tile_cells = %d (1 .. 16384)", who, tile_cells);
    AVL_REQUIRE(bytes_per_cell >= 4 && bytes_per_cell <= kMaxBytesPerCell && bytes_per_cell % 4 == 0,
                "%s: bytes_per_cell = %d (a multiple of 4, 4 .. %d)", who, bytes_per_cell, kMaxBytesPerCell);
    AVL_REQUIRE((tile_cells * bytes_per_cell) % 16 == 0, "%s: a destination tile row of %d cells of %d bytes is no multiple of 16 bytes", who,
                tile_cells, bytes_per_cell);
    AVL_REQUIRE(n_jobs == 0 || jobs_dev != nullptr, "%s: jobs_dev is NULL for %d jobs", who, n_jobs);
    AVL_REQUIRE(n_flags == 0 || flags != nullptr, "%s: flags is NULL for %d flags", who, n_flags);
    AVL_REQUIRE((reinterpret_cast<uintptr_t>(jobs_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(flags) & 3) == 0,
                "%s: jobs_dev or flags is misaligned", who);
    if (n_flags > 0) AVL_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)n_flags * sizeof(int32_t), stream));
    if (n_jobs == 0) return AVL_OK;
    // workgroups per tile: enough that few jobs still fill the machine, never more than the tile has groups of kWaves rows
    const int want = (kTargetWorkgroups + n_jobs - 1) / n_jobs;
    const int max_split = (tile_cells + kWaves - 1) / kWaves;
    *split = want < 1 ? 1 : (want > max_split ? max_split : want);
    return AVL_OK;
}

}  // namespace avl_tile_table
