// lz4ada_frames_index.hip -- gfx950 kernels that index many frames where
// they lie, in device memory (lz4ada_bulk_frames_device.cpp),
// so that a pass over device-resident frames needs no payload byte on the
// host:
//  * k_frames_walk -- one lane per frame runs frame_walk (lz4ada_frame_walk.h:
//    the header checks and the serial walk of the size words) and records the
//    verdict and the frame's sums;
//  * k_frames_scan -- one workgroup, the exclusive prefix sums of the accepted
//    frames' block counts and slot bytes (the 64-bit DPP scan, a carry between
//    rounds of WG frames);
//  * k_frames_fill -- one lane per frame walks an accepted frame again and
//    writes its block descriptors and its FrameRec where the scan put them.
// The walk is a chain of dependent loads (a size word gives the next word's
// place), so a lane's speed is HBM / L2 latency per block; N frames are N
// independent chains, one wave per workgroup to spread them over the CUs.
// Loads are byte loads through frame_walk: a frame starts at any byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"
#include "lz4ada_frame_walk.h"

namespace lz4ada {

constexpr uint32_t WALK_WG = 64;   // one wave: 64 frames per workgroup
constexpr uint32_t SCAN_WG = 256;  // frames per round of the scan

__global__ __launch_bounds__(WALK_WG) void k_frames_walk(const uint8_t* __restrict__ in,
                                                         const FrameSpan* __restrict__ span,
                                                         uint32_t nframes, bool no_lone, uint64_t budget,
                                                         bool take_linked, uint64_t linked_max,
                                                         FrameWalkRec* __restrict__ walk)
{
	const uint32_t i = blockIdx.x * WALK_WG + threadIdx.x;
	if (i >= nframes)
		return;
	lz4ada_frame_info info;
	WalkSums sums;
	int v = frame_walk(in + span[i].off, int64_t(span[i].len), no_lone, &info, &sums, nullptr, take_linked,
	                   linked_max);
	if (v == LZ4ADA_BATCH_OK && sums.slots > budget)
		v = LZ4ADA_BATCH_OVER_BUDGET;
	FrameWalkRec r;
	r.verdict = v;
	r.flags = (info.has_content_size ? FRAME_HAS_SIZE : 0u) | (info.content_checksum ? FRAME_HAS_CKSUM : 0u) |
	          (info.format == LZ4ADA_FORMAT_MODERN && !info.independent ? FRAME_LINKED : 0u);
	r.nblocks = uint64_t(info.nblocks);
	r.slots = sums.slots;
	r.caps = sums.caps;
	r.frame_len = info.frame_len;
	r.content_size = info.content_size;
	r.cksum = info.content_checksum_declared;
	r.format = v == LZ4ADA_BATCH_NOT_INDEXED ? 0 : info.format;
	walk[i] = r;
}

__global__ __launch_bounds__(SCAN_WG) void k_frames_scan(const FrameWalkRec* __restrict__ walk,
                                                         uint32_t nframes, uint64_t* __restrict__ first,
                                                         uint64_t* __restrict__ slot)
{
	__shared__ uint64_t wsum[SCAN_WG / 64];
	uint64_t carry_b = 0, carry_s = 0;
	for (uint32_t f0 = 0; f0 < nframes; f0 += SCAN_WG) {
		const uint32_t f = f0 + threadIdx.x;
		const bool take = f < nframes && walk[f].verdict == LZ4ADA_BATCH_OK;
		const uint64_t nb = take ? walk[f].nblocks : 0, sl = take ? walk[f].slots : 0;
		uint64_t total_b, total_s;
		const uint64_t off_b = wg_excl_scan<SCAN_WG>(nb, wsum, &total_b);
		const uint64_t off_s = wg_excl_scan<SCAN_WG>(sl, wsum, &total_s);
		if (f < nframes) {
			first[f] = carry_b + off_b;
			slot[f] = carry_s + off_s;
		}
		carry_b += total_b;
		carry_s += total_s;
	}
	if (threadIdx.x == 0) {
		first[nframes] = carry_b;
		slot[nframes] = carry_s;
	}
}

__global__ __launch_bounds__(WALK_WG) void k_frames_fill(const uint8_t* __restrict__ in,
                                                         const FrameSpan* __restrict__ span,
                                                         const FrameWalkRec* __restrict__ walk,
                                                         const uint64_t* __restrict__ first,
                                                         const uint64_t* __restrict__ slot, uint32_t nframes,
                                                         bool no_lone, bool take_linked, uint64_t linked_max,
                                                         lz4ada_block_desc* __restrict__ desc,
                                                         FrameRec* __restrict__ rec)
{
	const uint32_t i = blockIdx.x * WALK_WG + threadIdx.x;
	if (i >= nframes)
		return;
	const FrameWalkRec w = walk[i];
	FrameRec r;
	r.first = uint32_t(first[i]);
	r.nblocks = 0;
	r.flags = 0;
	r.hash = 0;
	r.content_size = 0;
	r.out_off = r.out_len = 0;
	r.fail = -1;
	r.verdict = 0;
	if (w.verdict == LZ4ADA_BATCH_OK) {
		r.nblocks = uint32_t(w.nblocks);
		r.flags = w.flags;
		r.content_size = w.content_size;
		lz4ada_frame_info info;
		WalkSums sums;
		WalkEmit e;
		e.descs = desc + first[i];
		e.cap = int64_t(w.nblocks);
		e.slots = true;
		e.in_base = span[i].off;
		e.out_base = slot[i];
		e.out_limit = slot[i] + w.slots;
		e.written = 0;
		const int v = frame_walk(in + span[i].off, int64_t(span[i].len), no_lone, &info, &sums, &e, take_linked,
		                         linked_max);
		if (v != LZ4ADA_BATCH_OK || e.written != int64_t(w.nblocks) || sums.slots != w.slots) {
			// the input changed between the walks: the frame fails, and the
			// decoders find nothing to do in what is left of its descriptors
			r.fail = 0;
			lz4ada_block_desc none;
			none.in_off = span[i].off;
			none.in_len = 0;
			none.flags = LZ4ADA_BLOCK_STORED;
			none.out_off = slot[i];
			none.out_cap = 0;
			none.cksum = 0;
			for (int64_t k = e.written; k < int64_t(w.nblocks); ++k)
				e.descs[k] = none;
		}
	}
	rec[i] = r;
}

hipError_t launch_frames_walk(const uint8_t* d_in, const FrameSpan* d_span, uint32_t nframes, bool no_lone,
                              uint64_t budget, bool take_linked, uint64_t linked_max, FrameWalkRec* d_walk,
                              hipStream_t stream)
{
	if (nframes == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_frames_walk, dim3((nframes + WALK_WG - 1) / WALK_WG), dim3(WALK_WG), 0, stream,
	                   d_in, d_span, nframes, no_lone, budget, take_linked, linked_max, d_walk);
	return hipGetLastError();
}

hipError_t launch_frames_scan(const FrameWalkRec* d_walk, uint32_t nframes, uint64_t* d_first,
                              uint64_t* d_slot, hipStream_t stream)
{
	hipLaunchKernelGGL(k_frames_scan, dim3(1), dim3(SCAN_WG), 0, stream, d_walk, nframes, d_first, d_slot);
	return hipGetLastError();
}

hipError_t launch_frames_fill(const uint8_t* d_in, const FrameSpan* d_span, const FrameWalkRec* d_walk,
                              const uint64_t* d_first, const uint64_t* d_slot, uint32_t nframes,
                              bool no_lone, bool take_linked, uint64_t linked_max, lz4ada_block_desc* d_desc,
                              FrameRec* d_rec, hipStream_t stream)
{
	if (nframes == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_frames_fill, dim3((nframes + WALK_WG - 1) / WALK_WG), dim3(WALK_WG), 0, stream,
	                   d_in, d_span, d_walk, d_first, d_slot, nframes, no_lone, take_linked, linked_max, d_desc,
	                   d_rec);
	return hipGetLastError();
}

}  // namespace lz4ada
