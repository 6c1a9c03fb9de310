// lz4ada_frames.hip -- gfx950 kernels that lay out and judge a pass of many
// frames (lz4ada_bulk_frames.cpp) from the block statuses the
// decoders left on the device, so the host needs no round trip between the
// decode and the compaction:
//  * k_frames_scan_tiles / k_frames_scan_carry -- the exclusive prefix sum
//    of the blocks' decoded lengths in two levels: a workgroup scans a tile
//    of PLAN_TILE blocks (four per thread, a DPP scan per wave, the waves'
//    totals through LDS) and one workgroup then scans the tiles' totals;
//  * k_frames_plan -- adds the two levels into dst_off[] (what k_compact
//    reads) and gives every frame its span, its first failing block and its
//    content-size verdict.
// A pass holds from no block to about a million (the scan itself has no
// limit below 2^32 blocks).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"

namespace lz4ada {

constexpr uint32_t PLAN_WG = 256;                     // threads per workgroup
constexpr uint32_t PLAN_PER = PLAN_TILE / PLAN_WG;    // blocks per thread
static_assert(PLAN_PER * PLAN_WG == PLAN_TILE, "a tile is a whole number of blocks per thread");

// The frame that holds block b: the last one whose first block is <= b
// (frames without blocks share their `first` with the frame after them).
__device__ __forceinline__ uint32_t frame_of_block(const FrameRec* fr, uint32_t nframes, uint32_t b)
{
	uint32_t lo = 0, hi = nframes;  // fr[lo].first <= b < fr[hi].first
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (fr[mid].first <= b)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// Level 1: tile-relative exclusive offsets into loc[], the tile's total
// into part[tile]; a failing block counts 0 bytes and tells its frame.
__global__ __launch_bounds__(PLAN_WG) void k_frames_scan_tiles(
        const lz4ada_block_desc* __restrict__ desc, lz4ada_block_status* __restrict__ st,
        uint32_t nblocks, FrameRec* __restrict__ fr, uint32_t nframes, uint64_t* __restrict__ loc,
        uint64_t* __restrict__ part)
{
	__shared__ uint64_t wsum[PLAN_WG / 64];
	const uint32_t b0 = blockIdx.x * PLAN_TILE + threadIdx.x * PLAN_PER;
	uint32_t len[PLAN_PER];
	uint64_t sum = 0;
#pragma unroll
	for (uint32_t k = 0; k < PLAN_PER; ++k) {
		const uint32_t b = b0 + k;
		len[k] = 0;
		if (b < nblocks) {
			const lz4ada_block_desc d = desc[b];
			const lz4ada_block_status s = st[b];
			// the block checksum is checked before decoding (lz4ada.adb:672-676)
			const bool bad = s.code != DS_OK || s.out_len > d.out_cap ||
			                 ((d.flags & LZ4ADA_BLOCK_HAS_CKSUM) && s.cksum != d.cksum);
			if (bad) {
				st[b].out_len = 0;  // k_compact copies nothing of it
				const uint32_t f = frame_of_block(fr, nframes, b);
				atomicMin(reinterpret_cast<uint32_t*>(&fr[f].fail), b - fr[f].first);
			} else {
				len[k] = s.out_len;
			}
		}
		sum += len[k];
	}
	uint64_t total;
	uint64_t off = wg_excl_scan<PLAN_WG>(sum, wsum, &total);
#pragma unroll
	for (uint32_t k = 0; k < PLAN_PER; ++k) {
		if (b0 + k < nblocks)
			loc[b0 + k] = off;
		off += len[k];
	}
	if (threadIdx.x == 0)
		part[blockIdx.x] = total;
}

// Level 2, one workgroup: part[t] becomes the bytes before tile t and
// part[ntiles] the pass's total.
__global__ __launch_bounds__(PLAN_WG) void k_frames_scan_carry(uint64_t* __restrict__ part,
                                                               uint32_t ntiles)
{
	__shared__ uint64_t wsum[PLAN_WG / 64];
	uint64_t carry = 0;
	for (uint32_t t0 = 0; t0 < ntiles; t0 += PLAN_WG) {
		const uint32_t t = t0 + threadIdx.x;
		const uint64_t v = t < ntiles ? part[t] : 0;
		uint64_t total;
		const uint64_t off = wg_excl_scan<PLAN_WG>(v, wsum, &total);
		if (t < ntiles)
			part[t] = carry + off;
		carry += total;
	}
	if (threadIdx.x == 0)
		part[ntiles] = carry;
}

__device__ __forceinline__ uint64_t plan_off(const uint64_t* loc, const uint64_t* part,
                                             uint32_t nblocks, uint32_t b)
{
	return b < nblocks ? part[b / PLAN_TILE] + loc[b] : part[plan_tiles(nblocks)];
}

// Thread i: dst_off[i] for i <= nblocks, and frame i's span and verdict.
__global__ __launch_bounds__(PLAN_WG) void k_frames_plan(const uint64_t* __restrict__ loc,
                                                         const uint64_t* __restrict__ part,
                                                         uint32_t nblocks, FrameRec* __restrict__ fr,
                                                         uint32_t nframes,
                                                         uint64_t* __restrict__ dst_off)
{
	const uint32_t i = blockIdx.x * PLAN_WG + threadIdx.x;
	if (i <= nblocks)
		dst_off[i] = plan_off(loc, part, nblocks, i);
	if (i < nframes) {
		const uint32_t first = fr[i].first, n = fr[i].nblocks;
		const uint64_t lo = plan_off(loc, part, nblocks, first);
		const uint64_t len = plan_off(loc, part, nblocks, first + n) - lo;
		fr[i].out_off = lo;
		fr[i].out_len = len;
		fr[i].verdict = ((fr[i].flags & FRAME_HAS_SIZE) && len != fr[i].content_size) ? FRAME_SIZE_BAD : 0;
	}
}

hipError_t launch_frames_plan(const lz4ada_block_desc* d_desc, lz4ada_block_status* d_status,
                              uint32_t nblocks, FrameRec* d_frames, uint32_t nframes,
                              uint64_t* d_dst_off, uint64_t* d_loc, uint64_t* d_part,
                              hipStream_t stream)
{
	const uint32_t ntiles = plan_tiles(nblocks);
	if (ntiles)
		hipLaunchKernelGGL(k_frames_scan_tiles, dim3(ntiles), dim3(PLAN_WG), 0, stream, d_desc,
		                   d_status, nblocks, d_frames, nframes, d_loc, d_part);
	hipLaunchKernelGGL(k_frames_scan_carry, dim3(1), dim3(PLAN_WG), 0, stream, d_part, ntiles);
	const uint32_t n = nblocks + 1 > nframes ? nblocks + 1 : nframes;
	hipLaunchKernelGGL(k_frames_plan, dim3((n + PLAN_WG - 1) / PLAN_WG), dim3(PLAN_WG), 0, stream,
	                   d_loc, d_part, nblocks, d_frames, nframes, d_dst_off);
	return hipGetLastError();
}

}  // namespace lz4ada
