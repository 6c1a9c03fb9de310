// lz4ada_compress_index.hip -- gfx950 kernels by which a compress pass writes
// the seek index of its own frames (lz4ada_compress_frames_device_indexed,
// DESIGN.md §22), after launch_compress_emit and the block checksums and
// before the pass's host synchronisation:
//  * k_compress_index_frames -- one workgroup, a lane per job, the jobs in
//    rounds: the rule's per-frame half (comp_index_frame,
//    lz4ada_compress_index.h: verdict, nominal slots, checkpoint group) and the
//    exclusive prefix sums that give every taken frame its place among the
//    index's descriptors, nominal slots and checkpoints, carried on from the
//    totals of the passes before (kernel arguments: the host has them from the
//    earlier pass's record).  Writes the per-job record the other two read and
//    the host replays, and the index's per-frame words: first, kgrp, ckfirst,
//    fkind, and the end entries of start and slotp;
//  * k_compress_index -- one lane per block: its descriptor (comp_index_desc)
//    at the frame's first + i, and its entries of start and slotp, which are
//    i * block_len: every block before it is full;
//  * k_ckpt_from_records -- a linked call: CKPT_SAVE_SPLIT workgroups per block
//    of the pass; those of a group start b copy the 65,536 record bytes in front
//    of block b from d_in to the index's store, 16 bytes per lane, the loads
//    wherever the record lies, the stores aligned (k_ckpt_save's layout).
// None of them reads a frame byte; the first two read the pass's arrays alone.
// Every bound comes from the job array, in_len and the counts the host sized
// the index by.  Plain vector stores only, every loop bounded by the job count,
// WALK_LONE_BLOCKS or a checkpoint's bytes, no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"
#include "lz4ada_compress_index.h"

namespace lz4ada {

namespace {

constexpr uint32_t CIDX_WG = 256;
static_assert(CKPT_BYTES % (CKPT_SAVE_SPLIT * CIDX_WG * 16) == 0, "k_ckpt_from_records's pieces tile a checkpoint");

// 16 bytes at any byte address (lz4ada_ranges.hip): one global_load_dwordx4
typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));

}  // namespace

__global__ __launch_bounds__(CIDX_WG) void k_compress_index_frames(const CompJob* __restrict__ jobs, uint32_t njobs,
                                                                   const uint32_t* __restrict__ csize,
                                                                   uint32_t nblocks, uint64_t block_len,
                                                                   uint32_t linked, uint64_t every, uint32_t no_lone,
                                                                   uint32_t kind, uint32_t f_lo, CompIndexRec base,
                                                                   CompIndexOut o, CompIndexRec* __restrict__ rec)
{
	__shared__ uint64_t wsum[CIDX_WG / 64];
	uint64_t carry_b = base.first, carry_s = base.out_base, carry_c = base.ck;
	for (uint32_t j0 = 0; j0 < njobs; j0 += CIDX_WG) {
		const uint32_t j = j0 + threadIdx.x;
		CompIndexFrame F{};
		F.verdict = LZ4ADA_BATCH_NOT_INDEXED;
		uint64_t n = 0;
		if (j < njobs) {
			const CompJob J = jobs[j];
			// (the host laid the blocks out by the same count: does not fail)
			if (uint64_t(J.first) + J.nblocks <= nblocks &&
			    uint64_t(comp_nblocks(int64_t(J.in_len), int64_t(block_len))) == J.nblocks) {
				F = comp_index_frame(J.in_len, block_len, csize + J.first, linked != 0, every, no_lone != 0);
				n = J.in_len;
			}
		}
		const bool take = F.verdict == LZ4ADA_BATCH_OK;
		const uint64_t nb = take ? F.nblocks : 0, sl = take ? F.slots : 0, nc = take ? F.nckpt : 0;
		uint64_t total_b, total_s, total_c;
		const uint64_t first = carry_b + wg_excl_scan<CIDX_WG>(nb, wsum, &total_b);
		const uint64_t slot = carry_s + wg_excl_scan<CIDX_WG>(sl, wsum, &total_s);
		const uint64_t ck = carry_c + wg_excl_scan<CIDX_WG>(nc, wsum, &total_c);
		const uint64_t f = uint64_t(f_lo) + j;
		if (j < njobs) {
			CompIndexRec r;
			r.first = first;
			r.out_base = slot;
			r.ck = ck;
			r.verdict = F.verdict;
			r.pad = 0;
			rec[j] = r;
			// the index is sized for every frame taken, and a prefix only shrinks: inside it
			if (f < o.nframes && first + nb <= o.nblocks) {
				o.first[f] = first;
				o.start[first + f + nb] = take ? n : 0;
				o.slotp[first + f + nb] = take ? F.tight : 0;
				if (o.kgrp) {
					o.kgrp[f] = F.group;
					o.ckfirst[f] = ck;
				}
				if (o.fkind)
					o.fkind[f] = take && nb ? kind : CHAIN_KIND_NONE;
			}
		}
		carry_b += total_b;
		carry_s += total_s;
		carry_c += total_c;
	}
	if (threadIdx.x == 0) {
		CompIndexRec r;
		r.first = carry_b;
		r.out_base = carry_s;
		r.ck = carry_c;
		r.verdict = LZ4ADA_BATCH_OK;
		r.pad = 0;
		rec[njobs] = r;
		const uint64_t f = uint64_t(f_lo) + njobs;  // the next pass's first frame, or the index's end entries
		if (f <= o.nframes) {
			o.first[f] = carry_b;
			if (o.kgrp)
				o.ckfirst[f] = carry_c;
		}
	}
}

__global__ __launch_bounds__(CIDX_WG) void k_compress_index(const CompBlock* __restrict__ blk,
                                                            const uint32_t* __restrict__ csize,
                                                            const lz4ada_block_desc* __restrict__ emitted,
                                                            const lz4ada_block_status* __restrict__ st,
                                                            const CompJob* __restrict__ jobs,
                                                            const CompIndexRec* __restrict__ rec, uint32_t nblocks,
                                                            uint32_t njobs, uint64_t block_len, uint32_t flags,
                                                            uint32_t f_lo, CompIndexOut o)
{
	const uint32_t b = blockIdx.x * CIDX_WG + threadIdx.x;
	if (b >= nblocks)
		return;
	const uint32_t j = blk[b].job;
	if (j >= njobs)
		return;
	const CompJob J = jobs[j];
	const CompIndexRec R = rec[j];
	const uint64_t i = uint64_t(b) - J.first, f = uint64_t(f_lo) + j;
	if (R.verdict != LZ4ADA_BATCH_OK || b < J.first || i >= J.nblocks || f >= o.nframes ||
	    R.first + J.nblocks > o.nblocks)
		return;
	// the payload's place is the one k_compress_emit wrote it to; the checksum the one behind it
	const bool bck = (flags & LZ4ADA_COMP_BLOCK_CHECKSUM) != 0;
	o.desc[R.first + i] = comp_index_desc(J.in_len, block_len, flags, i, csize[b], emitted[b].in_off,
	                                      bck && st ? st[b].cksum : 0u, R.out_base);
	o.start[R.first + f + i] = i * block_len;
	o.slotp[R.first + f + i] = i * block_len;  // (a multiple of 256)
}

__global__ __launch_bounds__(CIDX_WG) void k_ckpt_from_records(const uint8_t* __restrict__ d_in, uint64_t in_len,
                                                               const CompBlock* __restrict__ blk,
                                                               const CompJob* __restrict__ jobs,
                                                               const CompIndexRec* __restrict__ rec, uint32_t b_lo,
                                                               uint32_t nblocks, uint32_t njobs, uint64_t block_len,
                                                               uint32_t f_lo, CompIndexOut o)
{
	const uint32_t b = b_lo + blockIdx.x / CKPT_SAVE_SPLIT, piece = blockIdx.x % CKPT_SAVE_SPLIT;
	if (b >= nblocks || !o.kgrp)
		return;
	const uint32_t j = blk[b].job;
	if (j >= njobs || uint64_t(f_lo) + j >= o.nframes)
		return;
	const CompJob J = jobs[j];
	const CompIndexRec R = rec[j];
	const uint64_t K = o.kgrp[uint64_t(f_lo) + j];
	const uint64_t i = uint64_t(b) - J.first;
	if (R.verdict != LZ4ADA_BATCH_OK || b < J.first || i >= J.nblocks || !chain_head(K, i))
		return;
	const uint64_t c = R.ck + chain_checkpoint_of(K, i), at = i * block_len;
	// the record bytes [at - 65,536, at): inside the record, and the record inside d_in
	if (c >= o.nckpt || at < CKPT_BYTES || at >= J.in_len || J.in_off > in_len || J.in_len > in_len - J.in_off)
		return;
	constexpr uint32_t PIECE = uint32_t(CKPT_BYTES / CKPT_SAVE_SPLIT);
	cg8* const src = gptr(d_in) + J.in_off + (at - CKPT_BYTES) + piece * PIECE;
	g8* const dst = gptr(o.store) + c * CKPT_BYTES + piece * PIECE;
	for (uint32_t x = 16 * threadIdx.x; x < PIECE; x += 16 * CIDX_WG) {
		const u32x4 w = *reinterpret_cast<const GLOBAL u32x4_any*>(src + x);
		*reinterpret_cast<GLOBAL u32x4*>(dst + x) = w;
	}
}

hipError_t launch_compress_index(const uint8_t* d_in, uint64_t in_len, const CompBlock* d_blk, const CompJob* d_jobs,
                                 uint32_t nblocks, uint32_t njobs, const uint32_t* d_csize,
                                 const lz4ada_block_desc* d_emitted, const lz4ada_block_status* d_st,
                                 uint32_t block_id, uint32_t flags, bool linked, bool ckpts, uint64_t every,
                                 bool no_lone, uint32_t kind, uint32_t f_lo, const CompIndexRec& base,
                                 const CompIndexOut& o, CompIndexRec* d_rec, hipStream_t stream)
{
	if (njobs == 0)
		return hipSuccess;
	const uint64_t block_len = uint64_t(comp_block_len(block_id));
	hipLaunchKernelGGL(k_compress_index_frames, dim3(1), dim3(CIDX_WG), 0, stream, d_jobs, njobs, d_csize, nblocks,
	                   block_len, linked ? 1u : 0u, every, no_lone ? 1u : 0u, kind, f_lo, base, o, d_rec);
	if (nblocks == 0)
		return hipGetLastError();
	hipLaunchKernelGGL(k_compress_index, dim3((nblocks + CIDX_WG - 1) / CIDX_WG), dim3(CIDX_WG), 0, stream, d_blk,
	                   d_csize, d_emitted, d_st, d_jobs, d_rec, nblocks, njobs, block_len, flags, f_lo, o);
	// a launch takes fewer than 2^31 workgroups
	for (uint32_t b = 0; ckpts && b < nblocks;) {
		const uint32_t n = std::min<uint32_t>(nblocks - b, (1u << 30) / CKPT_SAVE_SPLIT);
		hipLaunchKernelGGL(k_ckpt_from_records, dim3(n * CKPT_SAVE_SPLIT), dim3(CIDX_WG), 0, stream, d_in, in_len,
		                   d_blk, d_jobs, d_rec, b, nblocks, njobs, block_len, f_lo, o);
		b += n;
	}
	return hipGetLastError();
}

}  // namespace lz4ada
