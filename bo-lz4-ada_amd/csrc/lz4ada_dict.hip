// lz4ada_dict.hip -- gfx950 kernels that give the slots of a many-frame pass
// a dictionary (lz4ada_bulk_frames_device.cpp):
//  * k_frames_dictid  -- one lane per frame compares a validated header's
//    dictionary id (LZ4ADA_DICT_CHECK_ID);
//  * k_frames_dictgap -- one lane per block moves the slot up by the gaps
//    before it and marks the gapped blocks (BLOCK_DICT);
//  * k_dict_fill      -- one workgroup per gapped block writes the gap: zeros,
//    then the dictionary's tail, ending at the block's out_off.
// The decoders that read the gaps as history are k_decode_idx_dict and
// k_decode_idx_frames_dict (lz4ada_idx.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"

namespace lz4ada {

constexpr uint32_t DICT_WG = 256;

__global__ __launch_bounds__(64) void k_frames_dictid(const uint8_t* __restrict__ in,
                                                      const FrameSpan* __restrict__ span,
                                                      FrameWalkRec* __restrict__ walk, uint32_t nframes,
                                                      uint32_t dict_id, uint32_t* __restrict__ bad)
{
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	if (i >= nframes)
		return;
	uint32_t b = 0;
	if (walk[i].verdict == LZ4ADA_BATCH_OK && walk[i].format == LZ4ADA_FORMAT_MODERN) {
		// the walk accepted the header: FLG, BD, [size], [id] and HC lie inside the span
		const uint8_t* p = in + span[i].off;
		const uint8_t flg = p[4];
		if (flg & 1u) {
			const uint8_t* q = p + 6 + ((flg & 8u) ? 8 : 0);
			const uint32_t id = uint32_t(q[0]) | (uint32_t(q[1]) << 8) | (uint32_t(q[2]) << 16) |
			                    (uint32_t(q[3]) << 24);
			if (id != dict_id) {
				b = 1;
				walk[i].verdict = LZ4ADA_DEVFRAME_DICT;
			}
		}
	}
	bad[i] = b;
}

// The frame that holds block b: the last one whose first block is <= b (as
// frame_of_block, lz4ada_frames.hip).
__device__ __forceinline__ uint32_t dict_frame_of(const FrameRec* fr, uint32_t nframes, uint32_t b)
{
	uint32_t lo = 0, hi = nframes;
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (fr[mid].first <= b)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

__global__ __launch_bounds__(DICT_WG) void k_frames_dictgap(const FrameRec* __restrict__ rec, uint32_t nframes,
                                                            const uint64_t* __restrict__ kind, uint64_t gap,
                                                            uint64_t limit, lz4ada_block_desc* __restrict__ desc,
                                                            uint32_t nblocks)
{
	const uint32_t b = blockIdx.x * DICT_WG + threadIdx.x;
	if (b >= nblocks || nframes == 0)
		return;
	const uint32_t f = dict_frame_of(rec, nframes, b);
	const uint64_t w = kind[f];
	const uint32_t k = b - rec[f].first, how = uint32_t(w & 3u);
	const uint64_t before = w >> 2;
	const uint64_t count = before + (how == DICT_KIND_INDEP ? uint64_t(k) + 1 : how == DICT_KIND_LINKED ? 1 : 0);
	const bool gapped = how == DICT_KIND_INDEP || (how == DICT_KIND_LINKED && k == 0);
	lz4ada_block_desc d = desc[b];
	d.out_off += gap * count;
	if (gapped)
		d.flags |= BLOCK_DICT;
	if (d.out_off + d.out_cap > limit) {  // never past what the host reserved
		d.in_len = 0;
		d.flags = LZ4ADA_BLOCK_STORED;
		d.out_off = 0;
		d.out_cap = 0;
	}
	desc[b] = d;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(DICT_WG) void k_dict_fill(const lz4ada_block_desc* __restrict__ desc,
                                                       uint32_t nblocks, const uint8_t* __restrict__ dict,
                                                       uint64_t dict_len, uint32_t dict_used,
                                                       uint8_t* __restrict__ slots)
{
	if (blockIdx.x >= nblocks)
		return;
	const lz4ada_block_desc d = desc[blockIdx.x];
	const uint64_t gap = dict_gap(dict_used);
	if (!(d.flags & BLOCK_DICT) || d.out_off < gap || dict_used > dict_len)
		return;
	uint8_t* const dst = slots + (d.out_off - gap);  // 256-aligned: out_off and gap are
	const uint32_t zeros = uint32_t(gap) - dict_used;  // bytes in front of the dictionary's
	const uint8_t* const src = dict + (dict_len - dict_used);
	for (uint32_t x = 16 * threadIdx.x; x < uint32_t(gap); x += 16 * DICT_WG) {
		u32x4 v = { 0u, 0u, 0u, 0u };
		if (x >= zeros) {  // 16 dictionary bytes, at any alignment
			__builtin_memcpy(&v, src + (x - zeros), 16);
		} else if (x + 16 > zeros) {  // the piece where the dictionary begins
			uint8_t t[16];
			for (uint32_t i = 0; i < 16; ++i)
				t[i] = x + i >= zeros ? src[x + i - zeros] : uint8_t(0);
			__builtin_memcpy(&v, t, 16);
		}
		*reinterpret_cast<u32x4*>(dst + x) = v;
	}
}

hipError_t launch_frames_dictid(const uint8_t* d_in, const FrameSpan* d_span, FrameWalkRec* d_walk,
                                uint32_t nframes, uint32_t dict_id, uint32_t* d_bad, hipStream_t stream)
{
	if (nframes == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_frames_dictid, dim3((nframes + 63) / 64), dim3(64), 0, stream, d_in, d_span, d_walk,
	                   nframes, dict_id, d_bad);
	return hipGetLastError();
}

hipError_t launch_frames_dictgap(const FrameRec* d_rec, uint32_t nframes, const uint64_t* d_kind, uint64_t gap,
                                 uint64_t limit, lz4ada_block_desc* d_desc, uint32_t nblocks, hipStream_t stream)
{
	if (nblocks == 0 || nframes == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_frames_dictgap, dim3((nblocks + DICT_WG - 1) / DICT_WG), dim3(DICT_WG), 0, stream, d_rec,
	                   nframes, d_kind, gap, limit, d_desc, nblocks);
	return hipGetLastError();
}

hipError_t launch_dict_fill(const lz4ada_block_desc* d_desc, uint32_t nblocks, const uint8_t* d_dict,
                            uint64_t dict_len, uint32_t dict_used, uint8_t* d_slots, hipStream_t stream)
{
	if (nblocks == 0 || dict_used == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_dict_fill, dim3(nblocks), dim3(DICT_WG), 0, stream, d_desc, nblocks, d_dict, dict_len,
	                   dict_used, d_slots);
	return hipGetLastError();
}

}  // namespace lz4ada
