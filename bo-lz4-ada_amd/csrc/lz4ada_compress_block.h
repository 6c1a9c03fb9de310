// lz4ada_compress_block.h -- what the three block compressors share (DESIGN.md
// §17, §18, §21): the history policy CompHist, the seeding loop's constants,
// put_ext, and the kernels' declarations.  The matching rule itself, the one
// device body of k_compress_blocks, k_compress_blocks_dict and
// k_compress_blocks_linked, is lz4ada_compress_block.inc.  Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_compress.h"
#include "lz4ada_dev.h"
#include "lz4ada_internal.h"

namespace lz4ada {

enum class CompHist { None, Dict, Linked };

constexpr uint32_t SEED_DEPTH = 8;  // steps of 64 positions whose loads are issued before the first insert
constexpr uint32_t SEED_LAST = uint32_t(COMP_LINK_WINDOW) - 4;  // index of q = -4, the last seeded position
static_assert(COMP_LINK_WINDOW % (64 * SEED_DEPTH) == 0, "the seeding loop covers the window in whole rounds");

// 255* and the rest of a length v >= 15 at dst[o ..) -> the bytes written
// (comp_ext_len(v)); the caller has checked them against the slot's end.
__device__ __forceinline__ int32_t put_ext(g8* dst, int32_t o, int32_t v, uint32_t lane)
{
	if (v < 15)
		return 0;
	const int32_t k = (v - 15) / 255;
	for (int32_t i = int32_t(lane); i < k; i += 64)
		dst[o + i] = 255;
	if (lane == 0)
		dst[o + k] = uint8_t((v - 15) - 255 * k);
	return k + 1;
}

// The three kernels of that body, a translation unit each (lz4ada_compress.hip,
// lz4ada_compress_dict.hip, lz4ada_compress_linked.hip).  Declared here only for
// the host's launch_compress_blocks (lz4ada_compress.hip), which chooses among
// them; no device code calls them.
__global__ __launch_bounds__(64) void k_compress_blocks(const uint8_t* __restrict__ d_in,
                                                         const CompBlock* __restrict__ blk, uint32_t nblocks,
                                                         uint8_t* __restrict__ slots, uint32_t* __restrict__ csize);
__global__ __launch_bounds__(64) void k_compress_blocks_dict(const uint8_t* __restrict__ d_in,
                                                              const CompBlock* __restrict__ blk, uint32_t nblocks,
                                                              const uint8_t* __restrict__ d_tail, uint32_t dict_len,
                                                              const uint32_t* __restrict__ seed,
                                                              uint8_t* __restrict__ slots,
                                                              uint32_t* __restrict__ csize);
__global__ __launch_bounds__(64) void k_compress_blocks_linked(const uint8_t* __restrict__ d_in,
                                                                const CompBlock* __restrict__ blk,
                                                                const CompJob* __restrict__ jobs, uint32_t nblocks,
                                                                const uint8_t* __restrict__ d_tail, uint32_t dict_len,
                                                                const uint32_t* __restrict__ seed,
                                                                uint8_t* __restrict__ slots,
                                                                uint32_t* __restrict__ csize);

}  // namespace lz4ada
