// lz4ada_sizes.hip -- gfx950 kernels that find the exact decoded sizes of
// device-resident frames without decoding them, so that a
// many-frame pass can be laid out by what its blocks decode to and not by
// what they could at most (lz4ada_bulk_frames_device.cpp):
//  * k_block_sizes -- one wave per block, after a launch_index over the same
//    descriptors: a block pass 1 accepted is the sum of its records' output
//    counts; one it declined is walked by the wave (block_decoded_size,
//    lz4ada_block_size.h, stated for 64 lanes); a stored one is its payload;
//  * k_frame_sizes -- one lane per frame adds its blocks up, judges the frame
//    and leaves what the passes need: the frame's first block among the sizes
//    and a copy of its walk record whose slots are the tight ones;
//  * k_frames_refit -- one lane per frame turns the nominal slots that
//    k_frames_fill wrote into the tight ones.
// No kernel here writes a payload or output byte, and k_block_sizes needs no
// LDS (the compiler keeps k_frame_sizes' record copy in 1 KiB of it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"
#include "lz4ada_block_size.h"

namespace lz4ada {

namespace {

constexpr uint32_t SIZES_WG = 64;  // one wave: a block, or 64 frames

__device__ __forceinline__ int32_t uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// A length extension at block-relative x (a run of bytes 255 and the byte
// that ends it), 64 bytes per step: lane l looks at byte x + l, a ballot
// finds the first byte that is not 255.  Adds the bytes to len and moves x
// past them; false when the payload ends first.  Reads payload bytes only
// (lanes at or past n load nothing), and x moves by 64 or the loop ends.
__device__ __forceinline__ bool scan_extension(cg8* in, int32_t n, int32_t& x, uint64_t& len)
{
	const int32_t lane = int32_t(lane_id());
	for (;;) {
		const bool valid = x + lane < n;
		const uint32_t c = valid ? uint32_t(in[x + lane]) : 0u;
		const uint64_t ends = __ballot(valid && c != 255u);
		if (ends == 0) {
			// every byte left in this step is 255: another step, or cut off
			if (n - x < 64)
				return false;
			len += 255u * 64u;
			x = uniform(x + 64);
			continue;
		}
		// the bytes before the first end are inside the payload and 255
		const int32_t k = uniform(__builtin_ctzll(ends));
		len += 255u * uint32_t(k) + uint32_t(__builtin_amdgcn_readlane(int32_t(c), k));
		x = uniform(x + k + 1);
		return true;
	}
}

// block_decoded_size for one wave, in wave-uniform control flow: every lane
// holds the same position (readfirstlane makes that provable), a sequence's
// token is read once, its literals and its offset are skipped by arithmetic,
// its length extensions are scanned 64 bytes per step.  i strictly advances
// and never passes n.
__device__ __forceinline__ uint32_t walk_block_size(cg8* in, int32_t n)
{
	uint64_t out = 0;
	int32_t i = 0;
	while (i < n) {
		const uint32_t token = uint32_t(__builtin_amdgcn_readfirstlane(int32_t(in[i])));
		uint64_t lit = token >> 4, ml = token & 15u;
		int32_t x = i + 1;
		if (lit == 15 && !scan_extension(in, n, x, lit))
			return BLOCK_SIZE_UNKNOWN;
		if (lit > uint64_t(n - x))
			return BLOCK_SIZE_UNKNOWN;  // the literal run passes the end
		x += int32_t(lit);
		out += lit;
		if (x == n) {
			if (ml != 0)
				return BLOCK_SIZE_UNKNOWN;
			break;
		}
		if (n - x < 2)
			return BLOCK_SIZE_UNKNOWN;  // the offset is cut in half
		x += 2;
		if (ml == 15 && !scan_extension(in, n, x, ml))
			return BLOCK_SIZE_UNKNOWN;
		out += ml + 4;
		i = uniform(x);
	}
	return out < BLOCK_SIZE_UNKNOWN ? uint32_t(out) : BLOCK_SIZE_UNKNOWN;
}

}  // namespace

__global__ __launch_bounds__(SIZES_WG) void k_block_sizes(const uint8_t* __restrict__ frame, uint64_t frame_len,
                                                          const lz4ada_block_desc* __restrict__ desc,
                                                          const lz4ada_block_status* __restrict__ status,
                                                          uint32_t nblocks, const uint8_t* __restrict__ tab_all,
                                                          uint32_t* __restrict__ size)
{
	const uint32_t b = blockIdx.x;
	if (b >= nblocks)
		return;
	const lz4ada_block_desc d = desc[b];
	const int32_t code = uniform(status[b].code);
	const uint32_t lane = lane_id();
	uint32_t s = BLOCK_SIZE_UNKNOWN;
	if (d.in_off > frame_len || d.in_len > frame_len - d.in_off || d.in_len > uint32_t(INT32_MAX)) {
		// not a block of this input: unknown
	} else if (d.flags & LZ4ADA_BLOCK_STORED) {
		s = d.in_len;
	} else if (code == DS_OK) {
		// pass 1's records: the high word is the output of the sequences that
		// start in the record's 32 payload bytes (8 bytes per lane, coalesced)
		const uint64_t* tab = reinterpret_cast<const uint64_t*>(tab_all) + (((d.in_off >> 8) + b) << 3);
		const uint32_t nrec = (d.in_len + 31u) >> 5;
		uint64_t acc = 0;
		for (uint32_t r = lane; r < nrec; r += 64)
			acc += tab[r] >> 32;
		acc = wave_incl_scan64(acc);
		const uint64_t sum = uint64_t(uint32_t(__builtin_amdgcn_readlane(int32_t(uint32_t(acc)), 63))) |
		                     (uint64_t(uint32_t(__builtin_amdgcn_readlane(int32_t(uint32_t(acc >> 32)), 63))) << 32);
		s = sum < BLOCK_SIZE_UNKNOWN ? uint32_t(sum) : BLOCK_SIZE_UNKNOWN;
	} else if (code == DS_SPARSE || code == DS_RETRY) {
		s = walk_block_size(gptr(frame) + d.in_off, int32_t(d.in_len));
	}
	if (lane == 0)
		size[b] = s;
}

// A frame of many blocks is rare among many small frames, so one lane adds a
// frame's blocks up in a serial loop, as k_frames_fill walks them.
__global__ __launch_bounds__(SIZES_WG) void k_frame_sizes(FrameWalkRec* __restrict__ walk,
                                                          const uint64_t* __restrict__ first, uint32_t nframes,
                                                          uint64_t size_base,
                                                          const lz4ada_block_desc* __restrict__ desc,
                                                          const uint32_t* __restrict__ size,
                                                          FrameSizeRec* __restrict__ rec,
                                                          uint64_t* __restrict__ size_first,
                                                          FrameWalkRec* __restrict__ tight)
{
	const uint32_t i = blockIdx.x * SIZES_WG + threadIdx.x;
	if (i >= nframes)
		return;
	FrameWalkRec w = walk[i];
	FrameSizeRec r;
	r.exact = r.tight = 0;
	r.verdict = w.verdict;
	r.pad = 0;
	if (w.verdict == LZ4ADA_BATCH_OK) {
		const uint64_t f = first[i];
		for (uint64_t k = 0; k < w.nblocks; ++k) {
			const uint32_t s = size[f + k], cap = desc[f + k].out_cap;
			// a linked frame's middle block must fill its slot (k_decode_idx_frames
			// ends the chain at a short one): the sizes say so ahead of the pass
			if (s == BLOCK_SIZE_UNKNOWN || s > cap || ((w.flags & FRAME_LINKED) && k + 1 < w.nblocks && s != cap)) {
				r.verdict = LZ4ADA_DEVFRAME_BLOCK;
				break;
			}
			r.exact += s;
			r.tight += (uint64_t(s) + 255) & ~uint64_t(255);
		}
		if (r.verdict == LZ4ADA_BATCH_OK && (w.flags & FRAME_HAS_SIZE) && r.exact != w.content_size)
			r.verdict = LZ4ADA_DEVFRAME_SIZE;
		if (r.verdict != LZ4ADA_BATCH_OK)
			r.exact = r.tight = 0;
		size_first[i] = size_base + f;
		walk[i].verdict = r.verdict;  // a frame the sizes fail takes no block and no slot
	} else {
		size_first[i] = size_base;
	}
	rec[i] = r;
	w.verdict = r.verdict;
	w.slots = r.tight;
	tight[i] = w;
}

__global__ __launch_bounds__(SIZES_WG) void k_frames_refit(const FrameWalkRec* __restrict__ walk,
                                                           const uint64_t* __restrict__ first,
                                                           const uint64_t* __restrict__ slot,
                                                           const uint64_t* __restrict__ size_first,
                                                           const uint32_t* __restrict__ size, uint32_t nframes,
                                                           lz4ada_block_desc* __restrict__ desc)
{
	const uint32_t i = blockIdx.x * SIZES_WG + threadIdx.x;
	if (i >= nframes || walk[i].verdict != LZ4ADA_BATCH_OK)
		return;
	// first / slot: the scan over the tight records, n + 1 entries each, so the
	// frame's blocks are [first[i], first[i + 1]) and its slots end at slot[i + 1]
	const uint64_t f = first[i], nb = first[i + 1] - f, limit = slot[i + 1];
	uint64_t at = slot[i];
	for (uint64_t k = 0; k < nb; ++k) {
		const uint32_t s = size[size_first[i] + k];
		const uint64_t step = (uint64_t(s) + 255) & ~uint64_t(255);
		lz4ada_block_desc d = desc[f + k];
		if (s == BLOCK_SIZE_UNKNOWN || at + step > limit) {
			// never past the frame's share of the slots (the sizes are the ones
			// the tight total was added up from, so this does not happen)
			d.in_len = 0;
			d.flags = LZ4ADA_BLOCK_STORED;
			d.out_off = at;
			d.out_cap = 0;
		} else {
			d.out_off = at;
			d.out_cap = s;
			at += step;
		}
		desc[f + k] = d;
	}
}

hipError_t launch_block_sizes(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                              const lz4ada_block_status* d_status, uint32_t nblocks, const uint8_t* d_tab,
                              uint32_t* d_size, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_block_sizes, dim3(nblocks), dim3(SIZES_WG), 0, stream, d_frame, frame_len, d_desc,
	                   d_status, nblocks, d_tab, d_size);
	return hipGetLastError();
}

hipError_t launch_frame_sizes(FrameWalkRec* d_walk, const uint64_t* d_first, uint32_t nframes, uint64_t size_base,
                              const lz4ada_block_desc* d_desc, const uint32_t* d_size, FrameSizeRec* d_rec,
                              uint64_t* d_size_first, FrameWalkRec* d_tight, hipStream_t stream)
{
	if (nframes == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_frame_sizes, dim3((nframes + SIZES_WG - 1) / SIZES_WG), dim3(SIZES_WG), 0, stream, d_walk,
	                   d_first, nframes, size_base, d_desc, d_size, d_rec, d_size_first, d_tight);
	return hipGetLastError();
}

hipError_t launch_frames_refit(const FrameWalkRec* d_tight, const uint64_t* d_first, const uint64_t* d_slot,
                               const uint64_t* d_size_first, const uint32_t* d_size, uint32_t nframes,
                               lz4ada_block_desc* d_desc, hipStream_t stream)
{
	if (nframes == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_frames_refit, dim3((nframes + SIZES_WG - 1) / SIZES_WG), dim3(SIZES_WG), 0, stream,
	                   d_tight, d_first, d_slot, d_size_first, d_size, nframes, d_desc);
	return hipGetLastError();
}

}  // namespace lz4ada
