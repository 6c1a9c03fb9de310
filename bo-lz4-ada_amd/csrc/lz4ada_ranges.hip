// lz4ada_ranges.hip -- gfx950 kernels of the seek index and the ranged decode
// of device-resident frames (lz4ada_bulk_ranges.cpp).  The
// decoders are the passes' own (launch_decode_checked); these are the pieces
// around them:
//  * k_block_starts -- one wave per frame, at the build: the exclusive prefix
//    sums of the frame's block sizes and of their tight slots, 64 blocks per
//    step (the 64-bit DPP scan, the carried totals read from lane 63);
//  * k_ranges_select -- one wave per range: the blocks it touches
//    (range_blocks, lz4ada_range_blocks.h) as a selection record, or their
//    marks in the pass's mark array, lanes striding;
//  * k_ranges_scan -- one workgroup: the exclusive count and slot bytes of the
//    marked blocks over the pass's block span, a carry between rounds;
//  * k_ranges_fill -- one lane per span block: a marked block's descriptor to
//    its compacted place, its slot by its exact size;
//  * k_ranges_verdict -- one wave per range: its first failing block;
//  * k_ranges_gather -- one workgroup per 16 KiB of a range: from the blocks'
//    slots to the caller's buffer, 16 bytes per lane between bytewise edges.
// Linked frames through history checkpoints add
//  * k_ckpt_save -- at the build: the 64 KiB in front of every group start,
//    from a decode pass's slots to the index's store, 16 bytes per lane;
//  * k_ckpt_fill -- one workgroup per compacted block: a head's checkpoint into
//    the gap in front of its slot, behind 256 zeros;
// and the chain rule (lz4ada_range_chains.h) in select, fill and verdict: the
// marks reach back to the group's start, a head's mark carries RANGE_MARK_GAP,
// the scan turns that bit into the gap's bytes, and the fill writes one chain
// record per compacted block for k_decode_idx_frames_dict.
// An index built with a dictionary adds a second gap, the
// dictionary's: select sets RANGE_MARK_DICT on the marked blocks that read it
// (chain_dict_gapped), the scan lays dict_gap(dict_used) bytes in front of
// them, the fill makes each the start of a chain whose record carries its
// history length, and
//  * k_dictimg_fill -- one workgroup per compacted block: the index's gap
//    image into the gap in front of such a block's slot;
// the chains of all three kinds then decode in one k_decode_idx_chains.
// Every bound is taken from the index's arrays and the host's counts; no
// kernel here reads a frame byte, and none lets a block status steer an
// address.  Plain vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"
#include "lz4ada_block_size.h"
#include "lz4ada_range_blocks.h"
#include "lz4ada_range_chains.h"

namespace lz4ada {

namespace {

constexpr uint32_t WAVE = 64;
constexpr uint32_t RSCAN_WG = 1024;  // span blocks per round of the scan
constexpr uint32_t FILL_WG = 256;
constexpr uint32_t GATHER_WG = 256;
constexpr uint32_t CKPT_WG = 256;
static_assert(CKPT_GAP >= CKPT_BYTES + 32 && CKPT_GAP % 256 == 0 && CKPT_BYTES == DICT_MAX,
              "a checkpoint is a dictionary of DICT_MAX bytes in a gap of dict_gap(DICT_MAX)");
static_assert(CHAIN_KIND_NONE == DICT_KIND_NONE && CHAIN_KIND_LINKED == DICT_KIND_LINKED &&
                  CHAIN_KIND_INDEP == DICT_KIND_INDEP,
              "the chain rule names the frame kinds as a dictionary pass does");
static_assert(CKPT_BYTES % (CKPT_SAVE_SPLIT * CKPT_WG * 16) == 0, "k_ckpt_save's pieces tile a checkpoint");

// 16 bytes at any byte address: one global_load_dwordx4 (gfx950 takes an
// unaligned address; the bytes read are the 16 asked for)
typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));

__device__ __forceinline__ uint64_t wave_last64(uint64_t v)
{
	return uint64_t(uint32_t(wave_last(int32_t(uint32_t(v))))) |
	       (uint64_t(uint32_t(wave_last(int32_t(uint32_t(v >> 32))))) << 32);
}

__device__ __forceinline__ uint64_t r256(uint64_t v) { return (v + 255) & ~uint64_t(255); }

// `n` bytes from src to dst by the whole workgroup, any alignment: bytewise up
// to dst's next 16-byte boundary and after its last, 16 bytes per lane between
// (the store aligned, the load wherever the source lies).
__device__ __forceinline__ void wg_copy(g8* dst, cg8* src, uint64_t n)
{
	const uint32_t t = threadIdx.x;
	const uint64_t lead = (16 - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
	const uint64_t head = lead < n ? lead : n;
	if (t < head)
		dst[t] = src[t];
	const uint64_t body = (n - head) & ~uint64_t(15);
	for (uint64_t i = uint64_t(t) * 16; i < body; i += uint64_t(GATHER_WG) * 16) {
		const u32x4 v = *reinterpret_cast<const GLOBAL u32x4_any*>(src + head + i);
		*reinterpret_cast<GLOBAL u32x4*>(dst + head + i) = v;
	}
	const uint64_t done = head + body;
	if (t < n - done)
		dst[done + t] = src[done + t];
}

}  // namespace

__global__ __launch_bounds__(WAVE) void k_block_starts(const uint64_t* __restrict__ first,
                                                       const uint64_t* __restrict__ size_first,
                                                       const uint32_t* __restrict__ size, uint32_t nframes,
                                                       uint64_t* __restrict__ start, uint64_t* __restrict__ slotp)
{
	const uint32_t k = blockIdx.x;
	if (k >= nframes)
		return;
	const uint64_t f = wave_uniform(first[k]), nb = wave_uniform(first[k + 1]) - f;
	const uint64_t sf = wave_uniform(size_first[k]);
	const uint64_t base = f + k;
	const uint32_t lane = lane_id();
	uint64_t carry_s = 0, carry_t = 0;
	for (uint64_t j0 = 0; j0 < nb; j0 += WAVE) {
		const uint64_t j = j0 + lane;
		// a frame the sizes stage accepted has no unknown size
		uint32_t s32 = j < nb ? size[sf + j] : 0u;
		s32 = s32 == BLOCK_SIZE_UNKNOWN ? 0u : s32;
		const uint64_t s = s32, t = r256(s);
		const uint64_t is = wave_incl_scan64(s), it = wave_incl_scan64(t);
		if (j < nb) {
			start[base + j] = carry_s + is - s;
			slotp[base + j] = carry_t + it - t;
		}
		carry_s += wave_last64(is);
		carry_t += wave_last64(it);
	}
	if (lane == 0) {
		start[base + nb] = carry_s;
		slotp[base + nb] = carry_t;
	}
}

__global__ __launch_bounds__(WAVE) void k_ranges_select(SeekView v, const RangeRec* __restrict__ ranges,
                                                        uint32_t nranges, RangeSel* __restrict__ sel,
                                                        uint32_t* __restrict__ mark, uint64_t span_lo,
                                                        uint32_t span_n)
{
	const uint32_t i = blockIdx.x;
	if (i >= nranges)
		return;
	const uint32_t k = wave_uniform(ranges[i].frame);
	if (k >= v.nframes)
		return;
	const uint64_t off = wave_uniform(ranges[i].off), want = wave_uniform(ranges[i].want);
	const uint64_t f = wave_uniform(v.first[k]), nb = wave_uniform(v.first[k + 1]) - f;
	const uint64_t* const st = v.start + f + k;
	const uint64_t* const sp = v.slotp + f + k;
	// every lane runs the same search over the same addresses
	const RangeBlocks rb = range_blocks(st, nb, off, want);
	const uint64_t b0 = wave_uniform(rb.first), n = wave_uniform(rb.count);
	// the chain: in a linked frame the marks begin at the group's start
	const uint64_t K = v.kgrp ? wave_uniform(v.kgrp[k]) : 0;
	const uint64_t c0 = n ? chain_start(K, b0) : b0;
	// a dictionary index: the frame's kind says which marked blocks read it
	const uint32_t kind = v.dict_used && v.fkind ? uint32_t(wave_uniform(v.fkind[k])) : CHAIN_KIND_NONE;
	if (sel && lane_id() == 0) {
		RangeSel r;
		r.first = uint32_t(b0);
		r.count = uint32_t(n);
		r.slot_lo = sp[c0];
		r.slot_hi = sp[b0 + n];
		r.fail = -1;
		r.pad = 0;
		sel[i] = r;
	}
	if (mark) {
		for (uint64_t j = c0 + lane_id(); j < b0 + n; j += WAVE) {
			const uint64_t b = f + j;
			if (b >= span_lo && b - span_lo < span_n)
				mark[b - span_lo] = (1u + (uint32_t((sp[j + 1] - sp[j]) >> 8) & ~RANGE_MARK_BITS)) |
				                    (chain_head(K, j) ? RANGE_MARK_GAP : 0u) |
				                    (chain_dict_gapped(kind, j) ? RANGE_MARK_DICT : 0u);
		}
	}
}

__global__ __launch_bounds__(RSCAN_WG) void k_ranges_scan(const uint32_t* __restrict__ mark, uint32_t span_n,
                                                          uint64_t gap, uint64_t dgap,
                                                          uint32_t* __restrict__ cnt, uint64_t* __restrict__ slot)
{
	__shared__ uint64_t wsum[RSCAN_WG / 64];
	uint64_t carry_c = 0, carry_s = 0;
	for (uint32_t i0 = 0; i0 < span_n; i0 += RSCAN_WG) {
		const uint32_t i = i0 + threadIdx.x;
		const uint32_t mg = i < span_n ? mark[i] : 0u, m = mg & ~RANGE_MARK_BITS;
		// a head's gap lies in front of its slot: part of what it takes, and of
		// where its own bytes begin; so does the dictionary's (no block has both:
		// should a mark carry both bits, the head's gap alone is laid)
		const uint64_t g = !m ? 0u : (mg & RANGE_MARK_GAP) ? gap : (mg & RANGE_MARK_DICT) ? dgap : 0u;
		const uint64_t c = m ? 1u : 0u, s = m ? (uint64_t(m - 1) << 8) + g : 0u;
		uint64_t total_c, total_s;
		const uint64_t off_c = wg_excl_scan<RSCAN_WG>(c, wsum, &total_c);
		const uint64_t off_s = wg_excl_scan<RSCAN_WG>(s, wsum, &total_s);
		if (i < span_n) {
			cnt[i] = uint32_t(carry_c + off_c);
			slot[i] = carry_s + off_s + g;
		}
		carry_c += total_c;
		carry_s += total_s;
	}
	if (threadIdx.x == 0) {
		cnt[span_n] = uint32_t(carry_c);
		slot[span_n] = carry_s;
	}
}

__global__ __launch_bounds__(FILL_WG) void k_ranges_fill(SeekView v, const uint32_t* __restrict__ mark,
                                                         const uint32_t* __restrict__ cnt,
                                                         const uint64_t* __restrict__ slot, uint64_t span_lo,
                                                         uint32_t span_n, uint32_t nsel, uint64_t slots,
                                                         lz4ada_block_desc* __restrict__ out,
                                                         FrameRec* __restrict__ chain)
{
	const uint32_t i = blockIdx.x * FILL_WG + threadIdx.x;
	if (i >= span_n || (mark[i] & ~RANGE_MARK_BITS) == 0)
		return;
	const uint32_t at = cnt[i];
	if (at >= nsel)  // the host counted the same marks: does not happen
		return;
	const uint64_t b = span_lo + i;
	const uint64_t k = rising_find(v.first, v.nframes, b);
	const uint64_t size = v.start[b + k + 1] - v.start[b + k];
	lz4ada_block_desc d = v.desc[b];
	d.out_off = slot[i];
	if (size > 0xFFFFFFFFull || slot[i] + r256(size) > slots) {
		d.in_len = 0;
		d.flags = LZ4ADA_BLOCK_STORED;
		d.out_cap = 0;
		d.out_off = 0;
	} else {
		d.out_cap = uint32_t(size);
	}
	if (chain) {
		// the block's chain record: a head and a linked frame's marked block 0
		// start a chain of the marked blocks of their group, the others ride
		FrameRec r;
		r.first = at;
		r.nblocks = 0;
		r.flags = 0;
		r.hash = 0;
		r.content_size = 0;
		r.out_off = r.out_len = 0;
		r.fail = -1;
		r.verdict = 0;
		const uint64_t K = v.kgrp ? v.kgrp[k] : 0;
		const uint64_t j = b - v.first[k], nb = v.first[k + 1] - v.first[k];
		const bool head = (mark[i] & RANGE_MARK_GAP) != 0;
		// the dictionary's gap: only where the index has one and the frame's kind agrees
		const uint32_t kind = v.dict_used && v.fkind ? uint32_t(v.fkind[k]) : CHAIN_KIND_NONE;
		const bool dgapped = !head && (mark[i] & RANGE_MARK_DICT) != 0;
		if (dgapped && d.out_cap == size) {
			// a dictionary-gapped block without its gap is an empty block
			if (!chain_dict_gapped(kind, j) || (K != 0) != (kind == CHAIN_KIND_LINKED) ||
			    d.out_off < dict_gap(v.dict_used)) {
				d.in_len = 0;
				d.flags = LZ4ADA_BLOCK_STORED;
				d.out_cap = 0;
				d.out_off = 0;
			} else {
				// block 0 of a linked frame: the marked blocks of its group ride; an
				// independent frame's block: a chain of its own
				uint32_t run = 1;
				if (K) {
					const uint64_t e = chain_group_end(K, nb, j);
					while (j + run < e && i + run < span_n && (mark[i + run] & ~RANGE_MARK_BITS) != 0)
						++run;
				}
				r.flags = FRAME_LINKED;
				r.nblocks = run;
				r.hash = v.dict_used;
				r.content_size = CHAIN_NO_CKPT;
				d.flags |= BLOCK_DICT;
			}
		} else if (K && d.out_cap == size && (head || j == 0)) {
			const uint64_t ck = head ? v.ckfirst[k] + chain_checkpoint_of(K, j) : 0;
			// a head without its gap or its checkpoint is an empty block
			if (head && (!chain_head(K, j) || ck >= v.ckfirst[k + 1] || ck >= v.nckpt || d.out_off < CKPT_GAP)) {
				d.in_len = 0;
				d.flags = LZ4ADA_BLOCK_STORED;
				d.out_cap = 0;
				d.out_off = 0;
			} else {
				const uint64_t e = chain_group_end(K, nb, j);
				uint32_t run = 1;
				while (j + run < e && i + run < span_n && (mark[i + run] & ~RANGE_MARK_BITS) != 0)
					++run;
				r.flags = FRAME_LINKED;
				r.nblocks = run;
				r.content_size = ck;
				if (head) {
					r.hash = uint32_t(CKPT_BYTES);
					d.flags |= BLOCK_DICT;
				}
			}
		}
		chain[chain_slot(at, nsel)] = r;
	}
	out[at] = d;
}

__global__ __launch_bounds__(CKPT_WG) void k_ckpt_fill(SeekView v, const lz4ada_block_desc* __restrict__ desc,
                                                       const FrameRec* __restrict__ chain, uint32_t nsel,
                                                       uint8_t* __restrict__ slots_p, uint64_t slots)
{
	if (blockIdx.x >= nsel)
		return;
	const lz4ada_block_desc d = desc[blockIdx.x];
	const FrameRec r = chain[chain_slot(blockIdx.x, nsel)];
	if (!(d.flags & BLOCK_DICT) || !(r.flags & FRAME_LINKED) || r.content_size >= v.nckpt || d.out_off < CKPT_GAP ||
	    d.out_off > slots)
		return;
	// 256-aligned on both sides: out_off and CKPT_GAP are, and the store's entries
	g8* const dst = gptr(slots_p) + (d.out_off - CKPT_GAP);
	cg8* const src = gptr(v.store) + r.content_size * CKPT_BYTES;
	constexpr uint32_t ZEROS = uint32_t(CKPT_GAP - CKPT_BYTES);
	const uint32_t t = threadIdx.x;
	if (t < ZEROS / 16) {
		const u32x4 z = { 0u, 0u, 0u, 0u };
		*reinterpret_cast<GLOBAL u32x4*>(dst + 16 * t) = z;
	}
	for (uint32_t x = 16 * t; x < uint32_t(CKPT_BYTES); x += 16 * CKPT_WG) {
		const u32x4 w = *reinterpret_cast<const GLOBAL u32x4*>(src + x);
		*reinterpret_cast<GLOBAL u32x4*>(dst + ZEROS + x) = w;
	}
}

__global__ __launch_bounds__(CKPT_WG) void k_dictimg_fill(SeekView v, const lz4ada_block_desc* __restrict__ desc,
                                                          const FrameRec* __restrict__ chain, uint32_t nsel,
                                                          uint8_t* __restrict__ slots_p, uint64_t slots)
{
	if (blockIdx.x >= nsel || !v.dict || v.dict_used == 0 || v.dict_used > DICT_MAX)
		return;
	const lz4ada_block_desc d = desc[blockIdx.x];
	const FrameRec r = chain[chain_slot(blockIdx.x, nsel)];
	const uint64_t gap = dict_gap(v.dict_used);
	if (!(d.flags & BLOCK_DICT) || !(r.flags & FRAME_LINKED) || r.content_size != CHAIN_NO_CKPT || d.out_off < gap ||
	    d.out_off > slots)
		return;
	// 256-aligned on both sides: out_off and the gap are, and the image is an allocation
	g8* const dst = gptr(slots_p) + (d.out_off - gap);
	cg8* const src = gptr(v.dict);
	for (uint32_t x = 16 * threadIdx.x; x < uint32_t(gap); x += 16 * CKPT_WG) {
		const u32x4 w = *reinterpret_cast<const GLOBAL u32x4*>(src + x);
		*reinterpret_cast<GLOBAL u32x4*>(dst + x) = w;
	}
}

__global__ __launch_bounds__(CKPT_WG) void k_ckpt_save(const uint64_t* __restrict__ kgrp,
                                                       const uint64_t* __restrict__ ckfirst, uint32_t f_lo,
                                                       uint32_t nf, uint64_t ck_lo, uint32_t nck, uint64_t nckpt,
                                                       const lz4ada_block_desc* __restrict__ desc,
                                                       uint32_t nblocks, FrameRec* __restrict__ rec,
                                                       const uint8_t* __restrict__ slots_p, uint64_t slots,
                                                       uint8_t* __restrict__ store)
{
	const uint32_t c_local = blockIdx.x / CKPT_SAVE_SPLIT, piece = blockIdx.x % CKPT_SAVE_SPLIT;
	if (c_local >= nck || nf == 0)
		return;
	const uint64_t c = ck_lo + c_local;
	// its frame among the pass's: the last one whose first checkpoint is not past c
	const uint64_t* const cf = ckfirst + f_lo;
	if (c >= nckpt || c < cf[0] || c >= cf[nf])
		return;
	const uint32_t f = uint32_t(rising_find(cf, nf, c));
	const uint64_t K = kgrp[f_lo + f];
	const FrameRec r = rec[f];
	const uint64_t b = K ? (c - cf[f] + 1) * K : 0;
	bool ok = K && (r.flags & FRAME_LINKED) && b < r.nblocks && uint64_t(r.first) + r.nblocks <= nblocks;
	uint64_t at = 0;
	if (ok) {
		// the frame's chain is contiguous when it decoded (k_decode_idx_frames ends
		// it otherwise), so the bytes in front of block b are the frame's own
		// once there are enough of them
		at = desc[r.first + b].out_off;
		ok = at >= desc[r.first].out_off + CKPT_BYTES && at <= slots;
	}
	if (!ok) {
		if (threadIdx.x == 0 && piece == 0)
			rec[f].fail = 0;
		return;
	}
	constexpr uint32_t PIECE = uint32_t(CKPT_BYTES / CKPT_SAVE_SPLIT);
	cg8* const src = gptr(slots_p) + (at - CKPT_BYTES) + piece * PIECE;
	g8* const dst = gptr(store) + c * CKPT_BYTES + piece * PIECE;
	for (uint32_t x = 16 * threadIdx.x; x < PIECE; x += 16 * CKPT_WG) {
		const u32x4 w = *reinterpret_cast<const GLOBAL u32x4*>(src + x);
		*reinterpret_cast<GLOBAL u32x4*>(dst + x) = w;
	}
}

__global__ __launch_bounds__(WAVE) void k_ranges_verdict(SeekView v, const RangeRec* __restrict__ ranges,
                                                         uint32_t nranges, RangeSel* __restrict__ sel,
                                                         const uint32_t* __restrict__ cnt, uint64_t span_lo,
                                                         uint32_t span_n,
                                                         const lz4ada_block_desc* __restrict__ desc,
                                                         const lz4ada_block_status* __restrict__ status,
                                                         uint32_t nsel)
{
	const uint32_t i = blockIdx.x;
	if (i >= nranges)
		return;
	const uint32_t k = wave_uniform(ranges[i].frame);
	if (k >= v.nframes)
		return;
	const uint64_t f = wave_uniform(v.first[k]);
	const uint32_t t0 = wave_uniform(sel[i].first), tn = wave_uniform(sel[i].count);
	// the range's chain: a block in front of the touched ones fails it too
	const uint64_t K = v.kgrp ? wave_uniform(v.kgrp[k]) : 0;
	const uint32_t b0 = tn ? uint32_t(chain_start(K, t0)) : t0, n = t0 - b0 + tn;
	int32_t fail = -1;
	for (uint32_t j0 = 0; j0 < n; j0 += WAVE) {
		const uint32_t j = j0 + lane_id();
		bool bad = false;
		if (j < n) {
			const uint64_t b = f + b0 + j;
			bad = true;  // a block the pass did not decode fails
			if (b >= span_lo && b - span_lo < span_n) {
				const uint32_t at = cnt[b - span_lo];
				if (at < nsel) {
					const lz4ada_block_desc d = desc[at];
					const lz4ada_block_status s = status[at];
					const uint64_t size = v.start[b + k + 1] - v.start[b + k];
					bad = s.code != DS_OK || s.out_len != size || d.out_cap != size ||
					      ((d.flags & LZ4ADA_BLOCK_HAS_CKSUM) && s.cksum != d.cksum);
				}
			}
		}
		const uint64_t any = __ballot(bad);
		if (any) {
			fail = int32_t(b0 + j0 + uint32_t(__builtin_ctzll(any)));
			break;
		}
	}
	if (lane_id() == 0)
		sel[i].fail = fail;
}

__global__ __launch_bounds__(GATHER_WG) void k_ranges_gather(SeekView v, const RangeRec* __restrict__ ranges,
                                                             uint32_t nranges, const RangeSel* __restrict__ sel,
                                                             uint64_t tile_lo, const uint32_t* __restrict__ mark,
                                                             const uint64_t* __restrict__ slot, uint64_t span_lo,
                                                             uint32_t span_n, const uint8_t* __restrict__ slots_p,
                                                             uint64_t slots, uint8_t* __restrict__ out)
{
	const uint64_t tile = tile_lo + blockIdx.x;
	// the range of this tile: the last one whose tile0 is not past it
	uint32_t lo = 0, hi = nranges;
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (ranges[mid].tile0 <= tile)
			lo = mid;
		else
			hi = mid;
	}
	const RangeRec r = ranges[lo];
	if (r.frame >= v.nframes || tile < r.tile0)
		return;
	const uint64_t done = (tile - r.tile0) * GATHER_TILE;
	if (done >= r.want)
		return;
	uint64_t rem = r.want - done < GATHER_TILE ? r.want - done : GATHER_TILE;
	uint64_t x = r.off + done;  // frame-relative decoded offset of the next byte
	const uint64_t f = v.first[r.frame], nb = v.first[r.frame + 1] - f;
	const uint64_t* const st = v.start + f + r.frame;
	if (x + rem > st[nb])  // the host clipped the range to the frame: does not happen
		return;
	const uint64_t last = uint64_t(sel[lo].first) + sel[lo].count;  // past the range's blocks
	g8* dst = gptr(out) + r.out_off + done;
	cg8* const src = gptr(slots_p);
	for (uint64_t j = rising_find(st, nb, x); rem > 0 && j < nb && j < last; ++j) {
		const uint64_t in_block = x - st[j], avail = st[j + 1] - x;
		const uint64_t take = avail < rem ? avail : rem;
		const uint64_t b = f + j;
		if (take && b >= span_lo && b - span_lo < span_n && (mark[b - span_lo] & ~RANGE_MARK_BITS)) {
			const uint64_t at = slot[b - span_lo] + in_block;
			if (at + take <= slots)
				wg_copy(dst, src + at, take);
		}
		dst += take;
		x += take;
		rem -= take;
	}
}

hipError_t launch_block_starts(const uint64_t* d_first, const uint64_t* d_size_first, const uint32_t* d_size,
                               uint32_t nframes, uint64_t* d_start, uint64_t* d_slotp, hipStream_t stream)
{
	if (nframes == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_block_starts, dim3(nframes), dim3(WAVE), 0, stream, d_first, d_size_first, d_size,
	                   nframes, d_start, d_slotp);
	return hipGetLastError();
}

hipError_t launch_ranges_select(const SeekView& v, const RangeRec* d_ranges, uint32_t nranges, RangeSel* d_sel,
                                uint32_t* d_mark, uint64_t span_lo, uint32_t span_n, hipStream_t stream)
{
	if (nranges == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_ranges_select, dim3(nranges), dim3(WAVE), 0, stream, v, d_ranges, nranges, d_sel, d_mark,
	                   span_lo, span_n);
	return hipGetLastError();
}

hipError_t launch_ranges_scan(const uint32_t* d_mark, uint32_t span_n, uint64_t gap, uint64_t dict_gap,
                              uint32_t* d_cnt, uint64_t* d_slot, hipStream_t stream)
{
	hipLaunchKernelGGL(k_ranges_scan, dim3(1), dim3(RSCAN_WG), 0, stream, d_mark, span_n, gap, dict_gap, d_cnt,
	                   d_slot);
	return hipGetLastError();
}

hipError_t launch_ranges_fill(const SeekView& v, const uint32_t* d_mark, const uint32_t* d_cnt,
                              const uint64_t* d_slot, uint64_t span_lo, uint32_t span_n, uint32_t nsel,
                              uint64_t slots, lz4ada_block_desc* d_desc, FrameRec* d_chain, hipStream_t stream)
{
	if (span_n == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_ranges_fill, dim3((span_n + FILL_WG - 1) / FILL_WG), dim3(FILL_WG), 0, stream, v, d_mark,
	                   d_cnt, d_slot, span_lo, span_n, nsel, slots, d_desc, d_chain);
	return hipGetLastError();
}

hipError_t launch_ckpt_fill(const SeekView& v, const lz4ada_block_desc* d_desc, const FrameRec* d_chain,
                            uint32_t nsel, uint8_t* d_slots, uint64_t slots, hipStream_t stream)
{
	if (nsel == 0 || v.nckpt == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_ckpt_fill, dim3(nsel), dim3(CKPT_WG), 0, stream, v, d_desc, d_chain, nsel, d_slots, slots);
	return hipGetLastError();
}

hipError_t launch_dictimg_fill(const SeekView& v, const lz4ada_block_desc* d_desc, const FrameRec* d_chain,
                               uint32_t nsel, uint8_t* d_slots, uint64_t slots, hipStream_t stream)
{
	if (nsel == 0 || v.dict_used == 0 || !v.dict)
		return hipSuccess;
	hipLaunchKernelGGL(k_dictimg_fill, dim3(nsel), dim3(CKPT_WG), 0, stream, v, d_desc, d_chain, nsel, d_slots, slots);
	return hipGetLastError();
}

hipError_t launch_ckpt_save(const uint64_t* d_kgrp, const uint64_t* d_ckfirst, uint32_t f_lo, uint32_t nf,
                            uint64_t ck_lo, uint32_t nck, uint64_t nckpt, const lz4ada_block_desc* d_desc,
                            uint32_t nblocks, FrameRec* d_rec, const uint8_t* d_slots, uint64_t slots,
                            uint8_t* d_store, hipStream_t stream)
{
	if (nck == 0 || nf == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_ckpt_save, dim3(nck * CKPT_SAVE_SPLIT), dim3(CKPT_WG), 0, stream, d_kgrp, d_ckfirst, f_lo, nf,
	                   ck_lo, nck, nckpt, d_desc, nblocks, d_rec, d_slots, slots, d_store);
	return hipGetLastError();
}

hipError_t launch_ranges_verdict(const SeekView& v, const RangeRec* d_ranges, uint32_t nranges, RangeSel* d_sel,
                                 const uint32_t* d_cnt, uint64_t span_lo, uint32_t span_n,
                                 const lz4ada_block_desc* d_desc, const lz4ada_block_status* d_status,
                                 uint32_t nsel, hipStream_t stream)
{
	if (nranges == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_ranges_verdict, dim3(nranges), dim3(WAVE), 0, stream, v, d_ranges, nranges, d_sel, d_cnt,
	                   span_lo, span_n, d_desc, d_status, nsel);
	return hipGetLastError();
}

hipError_t launch_ranges_gather(const SeekView& v, const RangeRec* d_ranges, uint32_t nranges,
                                const RangeSel* d_sel, uint64_t tile_lo, uint32_t ntiles, const uint32_t* d_mark,
                                const uint64_t* d_slot, uint64_t span_lo, uint32_t span_n, const uint8_t* d_slots,
                                uint64_t slots, uint8_t* d_out, hipStream_t stream)
{
	if (nranges == 0 || ntiles == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_ranges_gather, dim3(ntiles), dim3(GATHER_WG), 0, stream, v, d_ranges, nranges, d_sel,
	                   tile_lo, d_mark, d_slot, span_lo, span_n, d_slots, slots, d_out);
	return hipGetLastError();
}

}  // namespace lz4ada
