// lz4ada_compress.hip -- gfx950 kernels that compress device-resident records
// into LZ4 frames (lz4ada_bulk_compress.cpp):
//  * k_compress_blocks -- one wave per block: the one device body
//    (lz4ada_compress_block.inc, the matching rule of lz4ada_compress_host.cpp
//    read 64 positions at a time) with nothing in front of the block,
//    CompHist::None.  The block goes into a scratch slot of its own; a block
//    that would not come out shorter than it went in is marked stored;
//  * k_compress_scan_tiles / k_compress_scan_carry -- the exclusive prefix sum
//    of the blocks' bytes in the output (size word, payload, checksum), two
//    levels as in lz4ada_frames.hip;
//  * k_compress_emit -- a workgroup per block writes the size word and the
//    payload, from the slot or, stored, from the record, aligned dwords to the
//    output, and the descriptor k_xxh32_rows hashes the payload by;
//  * k_compress_block_cksums -- the block checksums behind the payloads;
//  * k_compress_frames -- a thread per job writes the header, the end mark and
//    the content checksum k_xxh32_spans left, and the job's place and length.
// launch_compress_blocks picks the pass's kernel of that one body: a
// dictionary call compresses its blocks with
// k_compress_blocks_dict (lz4ada_compress_dict.hip) and shares the rest; its
// dflags / dict_id reach the emit and the header for the 4 bytes of the id.
// A linked call compresses a pass that holds a continuation
// block with k_compress_blocks_linked (lz4ada_compress_linked.hip); the header
// learns its B.Indep bit from `linked`.
// No kernel waits for another workgroup; every loop is bounded by the block
// length or the block count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_compress_block.h"

namespace lz4ada {

namespace {

constexpr uint32_t COMP_WG = 256;                   // threads per workgroup of the scan and the emit
constexpr uint32_t COMP_PER = PLAN_TILE / COMP_WG;  // blocks per thread of the scan
static_assert(COMP_PER * COMP_WG == PLAN_TILE, "a tile is a whole number of blocks per thread");

// Bytes before block b in the pass's output, block bytes alone (b == nblocks: all of them).
__device__ __forceinline__ uint64_t comp_off(const uint64_t* loc, const uint64_t* part, uint32_t nblocks, uint32_t b)
{
	return b < nblocks ? part[b / PLAN_TILE] + loc[b] : part[plan_tiles(nblocks)];
}

}  // namespace

__global__ __launch_bounds__(64) void k_compress_blocks(const uint8_t* __restrict__ d_in,
                                                         const CompBlock* __restrict__ blk, uint32_t nblocks,
                                                         uint8_t* __restrict__ slots, uint32_t* __restrict__ csize)
{
	constexpr CompHist H = CompHist::None;
	constexpr const CompJob* jobs = nullptr;  // what only a history reads: named, never used
	constexpr const uint8_t* d_tail = nullptr;
	constexpr uint32_t dict_len = 0;
	constexpr const uint32_t* seed = nullptr;
#include "lz4ada_compress_block.inc"
}

// Level 1: tile-relative exclusive offsets into loc[], the tile's total into
// part[tile].  A block's bytes: `extra` (size word, checksum) and its payload.
__global__ __launch_bounds__(COMP_WG) void k_compress_scan_tiles(const CompBlock* __restrict__ blk,
                                                                 const uint32_t* __restrict__ csize,
                                                                 uint32_t nblocks, uint32_t extra,
                                                                 uint64_t* __restrict__ loc,
                                                                 uint64_t* __restrict__ part)
{
	__shared__ uint64_t wsum[COMP_WG / 64];
	const uint32_t b0 = blockIdx.x * PLAN_TILE + threadIdx.x * COMP_PER;
	uint32_t len[COMP_PER];
	uint64_t sum = 0;
#pragma unroll
	for (uint32_t k = 0; k < COMP_PER; ++k) {
		const uint32_t b = b0 + k;
		len[k] = 0;
		if (b < nblocks) {
			const uint32_t c = csize[b];
			len[k] = extra + (c ? c : blk[b].len);
		}
		sum += len[k];
	}
	uint64_t total;
	uint64_t off = wg_excl_scan<COMP_WG>(sum, wsum, &total);
#pragma unroll
	for (uint32_t k = 0; k < COMP_PER; ++k) {
		if (b0 + k < nblocks)
			loc[b0 + k] = off;
		off += len[k];
	}
	if (threadIdx.x == 0)
		part[blockIdx.x] = total;
}

// Level 2, one workgroup: part[t] becomes the bytes before tile t and
// part[ntiles] the pass's total.
__global__ __launch_bounds__(COMP_WG) void k_compress_scan_carry(uint64_t* __restrict__ part, uint32_t ntiles)
{
	__shared__ uint64_t wsum[COMP_WG / 64];
	uint64_t carry = 0;
	for (uint32_t t0 = 0; t0 < ntiles; t0 += COMP_WG) {
		const uint32_t t = t0 + threadIdx.x;
		const uint64_t v = t < ntiles ? part[t] : 0;
		uint64_t total;
		const uint64_t off = wg_excl_scan<COMP_WG>(v, wsum, &total);
		if (t < ntiles)
			part[t] = carry + off;
		carry += total;
	}
	if (threadIdx.x == 0)
		part[ntiles] = carry;
}

// Block b's size word and payload at their place in d_out: base (the pass's
// first byte) + the earlier jobs' headers and trailers + this job's header +
// the earlier blocks' bytes.  The payload goes as aligned dwords of d_out, its
// unaligned ends as bytes.  desc[b]: the payload inside d_out, for the block
// checksums; rec[job].stored counts the stored blocks.
__global__ __launch_bounds__(COMP_WG) void k_compress_emit(const uint8_t* __restrict__ d_in,
                                                           const uint8_t* __restrict__ slots,
                                                           const CompBlock* __restrict__ blk,
                                                           const uint32_t* __restrict__ csize,
                                                           const uint64_t* __restrict__ loc,
                                                           const uint64_t* __restrict__ part,
                                                           const CompJob* __restrict__ jobs, uint32_t nblocks,
                                                           uint32_t flags, uint32_t dflags, uint64_t base,
                                                           uint8_t* __restrict__ d_out,
                                                           lz4ada_block_desc* __restrict__ desc,
                                                           CompJobRec* __restrict__ rec)
{
	const uint32_t b = blockIdx.x;
	if (b >= nblocks)
		return;
	const CompBlock B = blk[b];
	const uint32_t c = csize[b];
	const bool stored = c == 0;
	const uint32_t n = stored ? B.len : c;
	const uint64_t at = base + jobs[B.job].fixed_before + uint64_t(comp_header_len(flags, dflags)) +
	                    comp_off(loc, part, nblocks, b);
	cg8* const s = stored ? gptr(d_in) + B.in_off : gptr(slots) + B.slot_off;
	g8* const t = gptr(d_out) + at + 4;
	if (threadIdx.x < 4)
		t[int32_t(threadIdx.x) - 4] = uint8_t((n | (stored ? 0x80000000u : 0u)) >> (8 * threadIdx.x));
	if (threadIdx.x == 0) {
		lz4ada_block_desc d;
		d.in_off = at + 4;
		d.in_len = n;
		d.flags = LZ4ADA_BLOCK_HAS_CKSUM | (stored ? LZ4ADA_BLOCK_STORED : 0u);
		d.out_off = 0;
		d.out_cap = 0;
		d.cksum = 0;
		desc[b] = d;
		if (stored)
			atomicAdd(&rec[B.job].stored, 1u);
	}
	const uint32_t head = min(n, uint32_t(-reinterpret_cast<uintptr_t>(t)) & 3u);
	const uint32_t words = (n - head) / 4, tail = head + 4 * words;
	if (threadIdx.x < head)
		t[threadIdx.x] = s[threadIdx.x];
	GLOBAL uint32_t* const tw = reinterpret_cast<GLOBAL uint32_t*>(t + head);
	for (uint32_t i = threadIdx.x; i < words; i += COMP_WG)
		tw[i] = ld32u_cached(s + head + 4 * i);
	if (threadIdx.x < n - tail)
		t[tail + threadIdx.x] = s[tail + threadIdx.x];
}

// The block checksums k_xxh32_rows left in st[b].cksum, behind the payloads.
__global__ __launch_bounds__(COMP_WG) void k_compress_block_cksums(const lz4ada_block_desc* __restrict__ desc,
                                                                   const lz4ada_block_status* __restrict__ st,
                                                                   uint32_t nblocks, uint8_t* __restrict__ d_out)
{
	const uint32_t b = blockIdx.x * COMP_WG + threadIdx.x;
	if (b >= nblocks)
		return;
	g8* const t = gptr(d_out) + desc[b].in_off + desc[b].in_len;
	const uint32_t h = st[b].cksum;
	for (int i = 0; i < 4; ++i)
		t[i] = uint8_t(h >> (8 * i));
}

// Job j's header, end mark and content checksum, and where its frame lies.  A
// record over hash_max bytes has no hash in frec yet: the host chain's follows.
__global__ __launch_bounds__(COMP_WG) void k_compress_frames(const CompJob* __restrict__ jobs, uint32_t njobs,
                                                             const uint64_t* __restrict__ loc,
                                                             const uint64_t* __restrict__ part, uint32_t nblocks,
                                                             uint32_t block_id, uint32_t flags, uint32_t dflags,
                                                             uint32_t dict_id, uint32_t linked, uint64_t base,
                                                             const FrameRec* __restrict__ frec,
                                                             uint8_t* __restrict__ d_out, CompJobRec* __restrict__ rec)
{
	const uint32_t j = blockIdx.x * COMP_WG + threadIdx.x;
	if (j >= njobs)
		return;
	const CompJob J = jobs[j];
	const uint64_t lo = comp_off(loc, part, nblocks, J.first);
	const uint64_t body = comp_off(loc, part, nblocks, J.first + J.nblocks) - lo;
	const uint64_t at = base + J.fixed_before + lo;
	uint8_t hdr[19];
	const int hn = comp_header(hdr, block_id, flags, J.in_len, dflags, dict_id, linked != 0);
	g8* t = gptr(d_out) + at;
	for (int i = 0; i < hn; ++i)
		t[i] = hdr[i];
	t += uint64_t(hn) + body;
	for (int i = 0; i < 4; ++i)
		t[i] = 0;
	if ((flags & LZ4ADA_COMP_CONTENT_CHECKSUM) && (frec[j].verdict & FRAME_GPU_HASHED)) {
		const uint32_t h = frec[j].hash;
		for (int i = 0; i < 4; ++i)
			t[4 + i] = uint8_t(h >> (8 * i));
	}
	rec[j].out_off = at;
	rec[j].out_len = uint64_t(hn) + body + uint64_t(comp_trailer_len(flags));
}

hipError_t launch_compress_blocks(const uint8_t* d_in, const CompBlock* d_blk, const CompJob* d_jobs, uint32_t nblocks,
                                  bool cont, const uint8_t* d_tail, uint32_t dl, const uint32_t* d_seed,
                                  uint8_t* d_slots, uint32_t* d_csize, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	if (cont)  // every block of the pass, each with the history its place gives it (read from d_in)
		hipLaunchKernelGGL(k_compress_blocks_linked, dim3(nblocks), dim3(64), 0, stream, d_in, d_blk, d_jobs, nblocks,
		                   d_tail, dl, d_seed, d_slots, d_csize);
	else if (dl)
		hipLaunchKernelGGL(k_compress_blocks_dict, dim3(nblocks), dim3(64), 0, stream, d_in, d_blk, nblocks, d_tail, dl,
		                   d_seed, d_slots, d_csize);
	else
		hipLaunchKernelGGL(k_compress_blocks, dim3(nblocks), dim3(64), 0, stream, d_in, d_blk, nblocks, d_slots,
		                   d_csize);
	return hipGetLastError();
}

hipError_t launch_compress_scan(const CompBlock* d_blk, const uint32_t* d_csize, uint32_t nblocks, uint32_t flags,
                                uint64_t* d_loc, uint64_t* d_part, hipStream_t stream)
{
	const uint32_t ntiles = plan_tiles(nblocks);
	if (ntiles)
		hipLaunchKernelGGL(k_compress_scan_tiles, dim3(ntiles), dim3(COMP_WG), 0, stream, d_blk, d_csize, nblocks,
		                   uint32_t(comp_block_extra(flags)), d_loc, d_part);
	hipLaunchKernelGGL(k_compress_scan_carry, dim3(1), dim3(COMP_WG), 0, stream, d_part, ntiles);
	return hipGetLastError();
}

hipError_t launch_compress_emit(const uint8_t* d_in, const uint8_t* d_slots, const CompBlock* d_blk,
                                const uint32_t* d_csize, const uint64_t* d_loc, const uint64_t* d_part,
                                const CompJob* d_jobs, uint32_t nblocks, uint32_t flags, uint32_t dflags, uint64_t base,
                                uint8_t* d_out, lz4ada_block_desc* d_desc, CompJobRec* d_rec, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_compress_emit, dim3(nblocks), dim3(COMP_WG), 0, stream, d_in, d_slots, d_blk, d_csize, d_loc,
	                   d_part, d_jobs, nblocks, flags, dflags, base, d_out, d_desc, d_rec);
	return hipGetLastError();
}

hipError_t launch_compress_block_cksums(const lz4ada_block_desc* d_desc, const lz4ada_block_status* d_st,
                                        uint32_t nblocks, uint8_t* d_out, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_compress_block_cksums, dim3((nblocks + COMP_WG - 1) / COMP_WG), dim3(COMP_WG), 0, stream,
	                   d_desc, d_st, nblocks, d_out);
	return hipGetLastError();
}

hipError_t launch_compress_frames(const CompJob* d_jobs, uint32_t njobs, const uint64_t* d_loc, const uint64_t* d_part,
                                  uint32_t nblocks, uint32_t block_id, uint32_t flags, uint32_t dflags,
                                  uint32_t dict_id, uint32_t linked, uint64_t base, const FrameRec* d_frec,
                                  uint8_t* d_out, CompJobRec* d_rec, hipStream_t stream)
{
	if (njobs == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_compress_frames, dim3((njobs + COMP_WG - 1) / COMP_WG), dim3(COMP_WG), 0, stream, d_jobs,
	                   njobs, d_loc, d_part, nblocks, block_id, flags, dflags, dict_id, linked, base, d_frec, d_out,
	                   d_rec);
	return hipGetLastError();
}

}  // namespace lz4ada
