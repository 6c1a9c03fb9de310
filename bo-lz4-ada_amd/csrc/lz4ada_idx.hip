// lz4ada_idx.hip -- index-driven bulk decoder for independent blocks.
//
// Replaces the same reference path as k_decode_pc (lib/lz4ada.adb:716-904:
// Decompress_Full_Block / Decompress_Sequence / Write_Output /
// Output_With_History) with two passes that keep every lane busy instead of
// parsing one sequence chain per wave:
//
//  * k_index (pass 1, one wave per block).  The compressed payload is cut
//    into 256-byte segments, 64 per 16 KiB LDS-staged chunk, one per lane.
//    Every lane walks the sequence chain of its segment from a guessed
//    entry (its segment start; lane 0 from the exact entry carried from the
//    previous chunk), then each lane re-walks from the exit of the lane
//    before it, until no entry changes.  LZ4 chains started at a wrong byte
//    merge with the true chain within a few sequences, so this converges in
//    2-4 walks per segment.  The walk records, for every 32-byte
//    sub-segment, where the first sequence starting inside it begins
//    (1 byte; 0xFF = none).  Any malformed sequence marks the block
//    DS_RETRY.
//  * k_decode_idx (pass 2, one wave per block).  Batches of 64 sub-segments
//    (2 KiB of input): lane i walks the sequences starting in sub-segment i
//    from its index entry (LDS-staged input), a wave prefix sum places them
//    in the output, literals and matches whose source lies before the batch
//    are copied at once, lane-parallel, straight to HBM; long runs and
//    matches reading this batch's own output follow in output order
//    (a leader loop: the first pending item always runs, every other whose
//    source is already final runs with it).
//
//  * k_decode_idx_frames, k_decode_idx_frames_dict, k_decode_idx_chains (pass 2
//    of linked blocks, one wave per chain): the chain's blocks in order, each
//    reading the earlier output as history.  The walk is stated once, in
//    decode_chain; the kernels differ in where the history starts (DESIGN.md
//    §12, §15, §19, §20).
//
// Blocks either pass declines (DS_RETRY: malformed data, a back-reference
// before the block start, an oversize block) are redone by k_decode_pc,
// which produces the exact statuses; so this pair never changes a result,
// only the speed.
//
// One translation unit in parts, included below in order:
// lz4ada_idx_input.inc (input access, sequence parsing), lz4ada_idx_pass1.inc
// (pass 1), lz4ada_idx_window.inc (pass 2's LDS output window and
// ring-sourced matches) and lz4ada_idx_pair.inc (k_decode_pp2).  This file
// keeps the straight-to-HBM path, the stages both block decoders share,
// decode_block, decode_chain, the k_decode_idx* kernels and the launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"

namespace lz4ada {
namespace idx {

// Stored-block copies without a block checksum: nontemporal loads and
// stores (2; 1 = stores only, 0 = neither).  With a block checksum the copy
// stays cached: the checksum kernel beside it reads the same payload.  A/B, 2048 x 4 MiB stored blocks, twice (tools/st_ab.sh,
// DESIGN §3): 3.62 / 3.84 ms plain, 3.71 / 3.77 ms NT stores, 3.39 / 3.48 ms
// NT loads and stores (with block checksums beside: 9.32 / 9.71, 9.49 /
// 9.82, 8.68 / 8.73 ms).
#ifndef LZ4ADA_STORED_NT
#define LZ4ADA_STORED_NT 2
#endif
constexpr int CHUNK = 16384;        // pass-1 staged chunk (16 KiB)
constexpr int SUB = 32;             // pass-2 sub-segment per lane
constexpr int BATCH = 64 * SUB;     // pass-2 batch (2 KiB of input)
constexpr int RING = 4 * BATCH;     // pass-2 staging ring
constexpr int LONG = 256;           // runs longer than this are copied by the whole wave
constexpr int32_t MAX_RUN = 1 << 28;  // length guard (block_max <= 4 MiB in the bulk path)
// Pass-1 lead-in (k_index): each lane first walks from this many bytes
// before its segment: about LEAD_SEQ sequences at the previous chunk's
// density (the first chunk: LEAD_IN0 bytes).
#ifndef LZ4ADA_LEAD_SEQ
#define LZ4ADA_LEAD_SEQ 60
#endif
constexpr int32_t LEAD_SEQ = LZ4ADA_LEAD_SEQ;
#ifndef LZ4ADA_LEAD_MAX
#define LZ4ADA_LEAD_MAX 1024
#endif
constexpr int32_t LEAD_IN0 = 256, LEAD_MIN = 256, LEAD_MAX = LZ4ADA_LEAD_MAX;
// Blocks with more than RLE_RATIO output bytes (slot capacity) per input
// byte are declined as sparse before any walk: few sequences with huge
// matches (runs), whose length extensions of hundreds of 255-bytes make the
// speculative walks crawl a lane per fixed-point iteration (53 per chunk,
// ~125k cycles each) -- k_decode_sparse's case (it declines dense data
// itself, so no result changes).
// (RLE_MIN_IN: the slot capacity overstates a short block's output, e.g. a
// frame's last block, and small blocks cost pass 1 little either way.)
constexpr uint64_t RLE_RATIO = 64;
constexpr uint32_t RLE_MIN_IN = 4096;

// vmcnt(0) through the builtin, so the compiler's wait pass sees it (an asm
// wait leaves the loads pending in its model: later register reuse on any
// path merging with this one then waits again)
__device__ __forceinline__ void vm_wait()
{
	asm volatile("" ::: "memory");
	__builtin_amdgcn_s_waitcnt(0x0F70);
	asm volatile("" ::: "memory");
}

// Diagnostic build only (-DLZ4ADA_IDX_STAMPS): cycles per phase, summed over
// waves (each stamp drains the wave's memory counters: read shares).
enum IdxPhase { I_STAGE, I_WALK0, I_ITER, I_CHUNKS, I_ITERS,
	            D_STAGE, D_WALK1, D_WALK2, D_TLDS, D_LIT, D_MFAR, D_NEAR, D_FLUSH, D_GLOBAL,
	            D_BATCHES, D_GBATCHES, D_ROUNDS, D_TASKS, D_LANES, I_STEPS, I_MAXST, I_LEAD,
	            // pieces dealt past the wave's 64 lanes: batches whose dealt HBM pieces exceed 64, those
	            // pieces, the batches left to M's load-and-wait path and their pieces; ring_pieces calls
	            // with more than 64 pieces, the pieces beyond, and its 64-piece chunk passes
	            D_HOVF_B, D_HOVF_P, D_HSLOW_B, D_HSLOW_P, D_ROVF_B, D_ROVF_P, D_RCHUNKS, IDX_NST };
#ifdef LZ4ADA_IDX_STAMPS
__device__ unsigned long long g_idx_stamps[IDX_NST];
#define ISTAMP_DECL uint64_t ist[IDX_NST] = {}; uint64_t ist_t = __builtin_amdgcn_s_memtime()
#define ISTAMP(ph)                                                           \
	do {                                                                     \
		asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");          \
		const uint64_t _n = __builtin_amdgcn_s_memtime();                    \
		ist[ph] += _n - ist_t;                                               \
		ist_t = _n;                                                          \
	} while (0)
#define ICOUNT(ph, v) (ist[ph] += uint64_t(v))
#define ISTAMP_FLUSH()                                                       \
	do {                                                                     \
		if (lane_id() == 0)                                                  \
			for (int _i = 0; _i < IDX_NST; ++_i)                             \
				atomicAdd(&g_idx_stamps[_i], (unsigned long long)ist[_i]);   \
	} while (0)
#else
#define ISTAMP_DECL
#define ISTAMP(ph)
#define ICOUNT(ph, v)
#define ISTAMP_FLUSH()
#endif

// Diagnostic build only (-DLZ4ADA_IDX_GATHERS): the 16-byte HBM loads of
// k_decode_idx's HBM-sourced matches: loads, 128-byte line touches (a load
// crossing a line boundary touches two; no de-duplication), batches -- to
// price the gather share of FETCH_SIZE.
#ifdef LZ4ADA_IDX_GATHERS
__device__ unsigned long long g_idx_gathers[4];  // loads, line touches, batches, input stagings
#define GCOUNT(i, v)                                                         \
	do {                                                                     \
		const uint64_t _v = uint64_t(v);                                     \
		if (lane_id() == 0 && _v)                                            \
			atomicAdd(&g_idx_gathers[i], (unsigned long long)_v);            \
	} while (0)
#else
#define GCOUNT(i, v)
#endif

#include "lz4ada_idx_input.inc"   // Src, fetch4 / fetch16 / ring16, Seq, parse_*, gload16, gstore_n
#include "lz4ada_idx_pass1.inc"   // Pass1, IdxLds, walk_segment, walk_first, the lead-in, index_block, k_index

// ------------------------------------------------------------------ pass 2

// Matches: copy len bytes to ob[dst] from ob[dst - off] (Output_With_History,
// lz4ada.adb:845-904, for an in-block source).  One lane, exact stores.
// Sources must be final; for off < len the lane reads back its own first
// 16 bytes (made visible by a wave-wide wait) or fills an off < 16 pattern.
__device__ __forceinline__ void lane_match(g8* ob, uintptr_t olim, int32_t dst, int32_t off,
                                           int32_t len)
{
	const uintptr_t base = reinterpret_cast<uintptr_t>(ob);
	if (off < 16 && off < len) {
		const u32x4 s = gload16(base + uintptr_t(dst - off), olim);
		u32x4 pv;
		int32_t width, stp;
		make_pattern(uint64_t(s.x) | (uint64_t(s.y) << 32), uint64_t(s.z) | (uint64_t(s.w) << 32),
		             off, pv, width, stp);
		for (int32_t k = 0; k < len; k += stp)
			gstore_n(ob + dst + k, pv, min(width, len - k));
		return;
	}
	int32_t r = 0;
	for (int32_t k = 0; k < len; k += 16) {
		const u32x4 v = gload16(base + uintptr_t(dst - off + r), olim);
		gstore_n(ob + dst + k, v, min(16, len - k));
		if (k == 0 && off < len)
			vm_wait();  // bytes [dst, dst+16) are read back by later chunks
		r += 16;
		if (r >= off)
			r -= off;
	}
}

// Whole-wave copy of one match (any length).
__device__ __forceinline__ void wave_match(g8* ob, uintptr_t olim, int32_t dst, int32_t off,
                                           int32_t len)
{
	const int32_t lane = int32_t(lane_id());
	const uintptr_t base = reinterpret_cast<uintptr_t>(ob);
	if (off < 16 && off < len) {
		const u32x4 s = gload16(base + uintptr_t(dst - off), olim);
		u32x4 pv;
		int32_t width, stp;
		make_pattern(uint64_t(s.x) | (uint64_t(s.y) << 32), uint64_t(s.z) | (uint64_t(s.w) << 32),
		             off, pv, width, stp);
		for (int32_t c = 0; c < len; c += 64 * stp) {
			const int32_t k = c + lane * stp;
			if (k < len)
				gstore_n(ob + dst + k, pv, min(width, len - k));
		}
		return;
	}
	// each step copies span <= off bytes, so it reads only bytes already final
	const int32_t span = off >= 1024 ? 1024 : (off & ~15);
	for (int32_t c = 0; c < len; c += span) {
		const int32_t k = c + 16 * lane;
		if (16 * lane < span && k < len) {
			const u32x4 v = gload16(base + uintptr_t(dst + k - off), olim);
			gstore_n(ob + dst + k, v, min(16, len - k));
		}
		if (off < len)
			vm_wait();
	}
}

// Whole-wave copy of one literal run from the compressed input.  NT
// (stored blocks, experiment LZ4ADA_STORED_NT): 1 = nontemporal stores,
// 2 = nontemporal loads too.
template <int NT = 0>
__device__ __forceinline__ void wave_literal(g8* ob, int32_t dst, const Src& S, int32_t src,
                                             int32_t len)
{
	const int32_t lane = int32_t(lane_id());
	// 8 KiB per step, every load issued before the first store (a stored
	// block is pure copy: one memory round trip per 8 KiB, not per 1 KiB)
	constexpr int U = 8;
	for (int32_t c = 0; c < len; c += 1024 * U) {
		u32x4 v[U];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const int32_t k = c + 1024 * u + 16 * lane;
			const uintptr_t a = reinterpret_cast<uintptr_t>(S.in) + uintptr_t(src + k);
			if (NT >= 2 && k + 16 <= len && a + 16 <= S.lim)
				v[u] = __builtin_nontemporal_load(reinterpret_cast<const GLOBAL u32x4*>(a));
			else if (k < len)
				v[u] = gload16(a, S.lim);
		}
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const int32_t k = c + 1024 * u + 16 * lane;
			if (NT >= 1 && k + 16 <= len)
				__builtin_nontemporal_store(v[u], reinterpret_cast<GLOBAL u32x4*>(ob + dst + k));
			else if (k < len)
				gstore_n(ob + dst + k, v[u], min(16, len - k));
		}
	}
}

// Deferred work item of one lane: a long literal run (src >= 0: input
// position) or a match (src = -offset) that is long or reads this batch.
struct Item {
	int32_t dst, len, src;
};

// Next deferred item of this lane from cursor (p, o, part); part 0 = the
// sequence's literals are next, 1 = its match.  far_end: output position
// before which every byte is final (the batch start).
__device__ __forceinline__ bool next_item(const Src& S, int32_t& p, int32_t& o, int32_t& part,
                                          int32_t sub_end, int32_t n, int32_t far_end, Item& it)
{
	while (p < sub_end) {
		Seq q;
		parse_seq(S, p, n, q);  // validated by the first walk of this batch
		if (part == 0) {
			part = 1;
			if (q.L > LONG) {
				it.dst = o;
				it.len = q.L;
				it.src = q.lit;
				return true;
			}
		}
		const int32_t mdst = o + q.L;
		p = q.next;
		o = mdst + q.ml;
		part = 0;
		if (q.ml > 0) {
			const int32_t dep_end = mdst - q.off + min(q.off, q.ml);
			if (q.ml > LONG || dep_end > far_end) {
				it.dst = mdst;
				it.len = q.ml;
				it.src = -q.off;
				return true;
			}
		}
	}
	return false;
}

// Oversized batches (a lane whose sequences decode to more than the LDS
// window, e.g. long RLE runs): the batch goes straight to HBM.  Literals
// and matches reading output older than the batch are copied at once;
// long runs and matches reading the batch itself follow in output order
// through a leader loop (the first pending item always runs; any other
// whose source is already final runs with it), with a wave-wide wait
// between rounds.  Returns false on a reference before the block start
// (hb: history bytes before it, linked frames).
__device__ __forceinline__ bool batch_global(const Src& S, g8* ob, uintptr_t olim, int32_t p0,
                                          int32_t sub_end, int32_t n, int32_t o_lane,
                                          int32_t o_batch, int32_t hb)
{
	const int32_t lane = int32_t(lane_id());
	int32_t cp = 0, co = 0, cpart = 0;
	bool has = false, pre = false;
	{
		int32_t o = o_lane;
		for (int32_t p = p0; p < sub_end;) {
			Seq q;
			parse_seq(S, p, n, q);
			if (q.L > LONG) {
				if (!has) {
					has = true;
					cp = p;
					co = o;
					cpart = 0;
				}
			} else {
				for (int32_t c = 0; c < q.L; c += 16)
					gstore_n(ob + o + c, fetch16(S, q.lit + c), min(16, q.L - c));
			}
			const int32_t mdst = o + q.L;
			if (q.ml > 0) {
				if (q.off > mdst + hb)
					pre = true;  // reference before the block start (D2)
				if (hb > 0 && q.off > mdst && q.off >= D1_OFF)
					pre = true;  // a possible quirk-D1 read: P flags / emulates those, so decline
				const int32_t dep_end = mdst - q.off + min(q.off, q.ml);
				if (q.ml > LONG || dep_end > o_batch) {
					if (!has) {
						has = true;
						cp = p;
						co = o;
						cpart = 1;
					}
				} else if (!pre) {
					lane_match(ob, olim, mdst, q.off, q.ml);
				}
			}
			o = mdst + q.ml;
			p = q.next;
		}
	}
	if (__any(pre))
		return false;
	Item it = {0, 0, 0};
	if (has)
		has = next_item(S, cp, co, cpart, sub_end, n, o_batch, it);
	if (__any(has)) {
		vm_wait();  // everything above is final
		for (;;) {
			const uint64_t m = __ballot(has);
			if (m == 0)
				break;
			const int32_t leader = __builtin_ctzll(m);
			const int32_t ldst = __shfl(it.dst, leader);
			const int32_t llen = __shfl(it.len, leader);
			const int32_t lsrc = __shfl(it.src, leader);
			bool ready;
			if (llen > LONG) {
				if (lsrc >= 0)
					wave_literal(ob, ldst, S, lsrc, llen);
				else
					wave_match(ob, olim, ldst, -lsrc, llen);
				ready = (lane == leader);
			} else {
				ready = has && it.len <= LONG &&
				        (it.src >= 0 || it.dst + it.src + min(-it.src, it.len) <= ldst);
				if (ready) {
					if (it.src >= 0)
						for (int32_t c = 0; c < it.len; c += 16)
							gstore_n(ob + it.dst + c, fetch16(S, it.src + c), min(16, it.len - c));
					else
						lane_match(ob, olim, it.dst, -it.src, it.len);
				}
			}
			vm_wait();
			if (ready)
				has = next_item(S, cp, co, cpart, sub_end, n, o_batch, it);
		}
	}
	return true;
}

#include "lz4ada_idx_window.inc"  // DecLds and its accessors, ostore*, oload16, patterns, owner searches, ring_*

// 2 KiB input chunk c (aligned address abase + c*BATCH), 32 bytes per lane
__device__ __forceinline__ void load_chunk2(uintptr_t abase, int32_t c, uintptr_t lim, u32x4& v0,
                                            u32x4& v1)
{
	const uintptr_t g = abase + uintptr_t(c) * BATCH + 16u * lane_id();
	if (abase + uintptr_t(c + 1) * BATCH <= lim) {
		__builtin_memcpy(&v0, reinterpret_cast<cg8*>(g), 16);
		__builtin_memcpy(&v1, reinterpret_cast<cg8*>(g + 1024), 16);
	} else {
		v0 = gload16(g, lim);
		v1 = gload16(g + 1024, lim);
	}
}

// Quirk D1 under the host's predicted round state (BLOCK_D1_ROUND: the
// last round ended at OPH in [65536, 65542] and this block starts at round
// position n1).  A match reading before the round start within 7 bytes of
// where that round ended (OPH - off < 8) reads what the reference's last
// wild copy (lib/lz4ada.adb:811-817) left past its frontier, not history:
// * after literals (L > 0): the payload bytes after them -- emulated when
//   their last chunk was wild (8 payload bytes left, k_lone_words' rule);
// * with no literals: the previous match's last Write_Output call
//   (:845-904), i.e. the output bytes right after that match's source --
//   emulated when the match was one call (no repeating part; from history,
//   no intermediate part either) whose tail read only final bytes (in the
//   round: its source ends pad bytes before its output; from history: the
//   tail stays in the previous round, and that match is no D1 read
//   itself).  `lit` then carries that position (block-relative, + D1_QBIAS,
//   << 3) and the overshoot length pad (low 3 bits) for M.
// Either way the match must read nothing of the current round.  false: a
// D1 read it does not emulate (the block is declined).  The rule was
// checked against the oracle's output over 256-block linked frames of the
// generator's uniform-offset kinds (tools/d1_model.py).
constexpr int32_t D1_QBIAS = 1 << 17;
__device__ __forceinline__ bool d1_emulable(int32_t mdst, int32_t L, int32_t& lit, int32_t off, int32_t ml,
                                            int32_t pmd, int32_t pof, int32_t pml, int32_t n1, int32_t oph,
                                            int32_t n)
{
	if (!(n1 + mdst < off && oph - off < 8))
		return true;  // no D1 read
	if (n1 + mdst + ml > off)
		return false;  // it also reads the current round
	if (L > 0)
		return lit + 8 * ((L - 1) >> 3) + 8 <= n;
	if (n1 + mdst == 0) {  // the round's first output: nothing written past its frontier yet,
		lit = D1_QBIAS << 3;  // the read is the previous round's bytes -- plain history (pad 0)
		return true;
	}
	if (pml <= 0)
		return false;  // the previous match is not known here
	const int32_t f = n1 + pmd, raw = f - pof, pad = (8 - (pml & 7)) & 7;
	bool ok = raw >= 0 ? pml <= pof && pof - pml >= pad
	                   : pof - f >= pml && oph - pof >= 8 && raw + pml + pad <= 0;
	const int32_t q = pmd - pof + pml;  // the previous match's source end
	if (ok)
		lit = ((q + D1_QBIAS) << 3) | pad;
	return ok;
}

// The status of a block with nothing to report but its code and, when that
// is DS_OK, its output length (written by one lane).
__device__ __forceinline__ void put_status(lz4ada_block_status& st, int32_t code, int32_t len)
{
	st.code = code;
	st.aux = 0;
	st.detail = 0;
	st.err_out_pos = 0;
	st.out_len = code == DS_OK ? uint32_t(len) : 0u;
}

// Block b's descriptor (b wave-uniform) in SGPRs.  It is one per wave, but
// pass 2 loads it with a vector load (the kernel may have stored to HBM
// before, which rules a scalar load out), and from VGPRs every bound, base
// address and cursor of the batch loop computed from it would run on the
// VALU in 64 copies.
__device__ __forceinline__ lz4ada_block_desc wave_desc(const lz4ada_block_desc* __restrict__ desc, uint32_t b)
{
	lz4ada_block_desc d = desc[b];
	d.in_off = wave_uniform(d.in_off);
	d.in_len = wave_uniform(d.in_len);
	d.flags = wave_uniform(d.flags);
	d.out_off = wave_uniform(d.out_off);
	d.out_cap = wave_uniform(d.out_cap);
	return d;
}

// ------------------------------------------------ pass 2's shared stages
// The steps of a batch that decode_block (one wave per block) and
// decode_block_pp2 (the pipelined pair) both take, each stated once over
// the LDS layout: DecLds, or a pair wave's view WP2.  What the decoders do
// differently stays in them: the pair's token and done[] hand-offs, its
// split of a match at the HBM threshold (hml) and its glo from the other
// wave's flush; quirk D1, the zero plane and the borrowed slots in
// decode_block.
//
// Left in both decoders, because as a function the same text compiled to
// other machine code for the k_decode_idx family or for k_decode_pp2 in
// every form tried (bench.kernel_code_hash): the
// two-round parse, the fill of the sequence starts into cst, the chunk
// loads ahead of staging (decode_block's own, beside stage_chunk, where
// the pair has pp_load_chunk), and the [&] lambdas through which
// decode_block reaches deal_pack.  The window reload after an oversized
// batch is two statements on purpose: decode_block's reaches back into the
// history in front of the block (hb) with cached loads, the pair's has no
// history, reads past the L1 (nontemporal) and checks each piece against
// cap -- one function would take a flag that says which decoder calls.

// Staging: input chunk c (2 KiB, 32 bytes per lane: v0, v1) into the input
// ring (four chunks; the ring's first 16 bytes mirrored past its end) and
// the pass-1 records of its 64 sub-segments into rrec.
template <class LD>
__device__ __forceinline__ void stage_chunk(LD& L, int32_t c, const u32x4& v0, const u32x4& v1, uint64_t r)
{
	const uint32_t lane = lane_id();
	const uint32_t a = uint32_t(c * BATCH) & (RING - 1);
	*reinterpret_cast<u32x4*>(&ring_of(L)[a + 16 * lane]) = v0;
	*reinterpret_cast<u32x4*>(&ring_of(L)[a + 1024 + 16 * lane]) = v1;
	if (a == 0 && lane == 0)
		*reinterpret_cast<u32x4*>(&ring_of(L)[RING]) = v0;
	rrec_of(L)[64 * (c & 3) + lane] = r;
}

// The batch cut, from the staged records of the 64 sub-segments from k0, one
// per lane: lanes [0, m) form a batch of at most `ow` output bytes and at
// most `seqs` sequences (OW and MAXSEQ; decode_block's experiment macros
// pass a smaller cut).  m == 0: the first sub-segment alone exceeds a limit
// -- an oversized batch, the 64 sub-segments go straight to HBM.
struct BatchCut {
	uint32_t bm;           // this lane's sequence starts (pass 1's bitmap of its sub-segment)
	int32_t cnt, nseq;     // its output bytes (at most 2^24: above any cap, which the caller checks) and sequences
	int32_t incl, incl_s;  // their inclusive sums over the wave
	int32_t m;
};
template <class LD>
__device__ __forceinline__ BatchCut batch_cut(LD& L, int32_t k0, int32_t nsub, int32_t ow, int32_t seqs)
{
	const int32_t k = k0 + int32_t(lane_id());
	const uint64_t rec = (k < nsub) ? rrec_of(L)[k & 255] : 0;
	BatchCut c;
	c.bm = uint32_t(rec);
	c.cnt = int32_t(min(uint32_t(rec >> 32), 1u << 24));
	c.nseq = __popc(c.bm);
	c.incl = wave_incl_scan(c.cnt);
	c.incl_s = wave_incl_scan(c.nseq);
	c.m = __popcll(__ballot(c.incl <= ow && c.incl_s <= seqs));
	return c;
}

// The flush: whole 16-byte units of output bytes [from, to) from the window
// to HBM (the first may start before `from`: those bytes are in the window
// too; a partial last unit goes with the next batch).  Always FLUSH_ST store
// instructions, so that a later vmcnt wait can count them.
__device__ __forceinline__ void flush_units(g8* ob, const uint8_t* window, uint32_t mask, int32_t from, int32_t to)
{
	const int32_t lane = int32_t(lane_id());
	const int32_t u0 = from >> 4, u1 = to >> 4;
#pragma unroll
	for (int i = 0; i < FLUSH_ST; ++i) {
		const int32_t u = u0 + lane + 64 * i;
		if (u < u1)
			*reinterpret_cast<GLOBAL u32x4*>(ob + (u << 4)) =
			    *reinterpret_cast<const u32x4*>(&window[(u << 4) & mask]);
	}
}

// The window's unflushed tail, the partial unit below output position o, to
// HBM by one lane: before an oversized batch, and at the block's end.
template <class LD>
__device__ __forceinline__ void flush_tail(LD& L, g8* ob, int32_t o)
{
	const int32_t a0 = o & ~15;
	if (lane_id() == 0 && o > a0)
		gstore_n(ob + a0, *reinterpret_cast<const u32x4*>(&oring_of(L)[uint32_t(a0) & omask_of(L)]), o - a0);
}

// Dealing two rounds' pieces over the wave (HBM-sourced match pieces,
// literal pieces): lane i has nc0 pieces in round 0 and nc1 in round 1; the
// batch's pieces are numbered round 0's first, in lane order.
struct Deal2 {
	int32_t inc0, tot0;  // round 0: inclusive sum, total
	int32_t inc1, tot;   // both rounds: tot0 + round 1's inclusive sum, total
};
__device__ __forceinline__ Deal2 deal2(int32_t nc0, int32_t nc1)
{
	Deal2 d;
	d.inc0 = wave_incl_scan(nc0);
	d.tot0 = wave_last(d.inc0);
	d.inc1 = d.tot0 + wave_incl_scan(nc1);
	d.tot = wave_last(d.inc1);
	return d;
}
// A run's descriptor, which its dealt pieces read from ldesc (lane i writes
// round 0's at [i] and round 1's at [64 + i]): 4 x 16 bits.
struct DealRun {
	int32_t src;   // a match: its batch-relative destination; literals: their input position in the batch
	int32_t aux;   // a match: its offset; literals: their batch-relative destination
	int32_t len;   // the run's bytes
	int32_t excl;  // the batch's pieces before the run's first
};
__device__ __forceinline__ uint64_t deal_pack(int32_t src, int32_t aux, int32_t len, int32_t excl)
{
	return uint64_t(uint16_t(src)) | (uint64_t(uint16_t(aux)) << 16) | (uint64_t(uint16_t(len)) << 32) |
	       (uint64_t(uint16_t(excl)) << 48);
}
__device__ __forceinline__ DealRun deal_unpack(uint64_t dd)
{
	return DealRun{ int32_t(dd & 0xffffu), int32_t((dd >> 16) & 0xffffu), int32_t((dd >> 32) & 0xffffu),
	                int32_t(dd >> 48) };
}
// One block.  hist: output bytes right before this block's slot that its
// matches may read -- 0 for independent blocks; in a linked frame, the
// earlier blocks' output, contiguous when every one of them is full.
// Returns the block's status code; out_len gets its output length.
//
// ZL (the linked path's second plane, k_decode_idx_zl; a constant at each
// inlined call site, so the other decoders' code has none of it): every literal byte
// is written as 0, so an output byte is nonzero only where it came from
// the synthetic history (whose bytes there hold the history position's
// high byte); a match reading history positions below 256 (more than
// 65,280 bytes before the block: their high byte is 0 too) sets
// AUX_DEEP_HIST; a stored block is all zeros; an oversized batch (literals
// straight to HBM) declines the block, which then takes the three-plane
// decode (lz4ada_bulk_linked.cpp).
__device__ __forceinline__ int32_t decode_block(DecLds& D, const uint8_t* __restrict__ frame,
                                                uint64_t frame_len,
                                                const lz4ada_block_desc* __restrict__ desc,
                                                uint32_t b, const uint8_t* __restrict__ tab_all,
                                                uint8_t* __restrict__ out,
                                                lz4ada_block_status* __restrict__ status,
                                                int64_t hist, int32_t& out_len, const bool ZL = false,
                                                const bool D1E = false)
{
	const int32_t lane = int32_t(lane_id());
	const lz4ada_block_desc d = wave_desc(desc, b);
	out_len = 0;
	if (wave_uniform(int32_t(status[b].code)) != DS_OK)
		return DS_RETRY;  // pass 1 declined it
	cg8* in = gptr(frame) + d.in_off;
	g8* ob = gptr(out) + d.out_off;
	const int32_t n = int32_t(d.in_len);
	const int32_t cap = int32_t(d.out_cap);
	const uintptr_t lim = reinterpret_cast<uintptr_t>(frame) + frame_len;
	const uintptr_t olim = reinterpret_cast<uintptr_t>(ob) + uintptr_t(cap);

	if (d.flags & LZ4ADA_BLOCK_STORED) {
		int32_t code = DS_OK;
		if (n > cap) {
			code = DS_OUT_OVERFLOW;
		} else if (ZL) {  // every byte a literal: zeros
			for (int32_t x = 16 * lane; x < n; x += 64 * 16)
				gstore_n(ob + x, u32x4{ 0u, 0u, 0u, 0u }, min(16, n - x));
		} else {
			Src S0;
			S0.in = in;
			S0.lim = lim;
			// nontemporal copy unless the block checksum kernel beside this
			// one reads the same payload (it then finds it in the caches)
			if (d.flags & LZ4ADA_BLOCK_HAS_CKSUM)
				wave_literal<0>(ob, 0, S0, 0, n);
			else
				wave_literal<LZ4ADA_STORED_NT>(ob, 0, S0, 0, n);
		}
		if (lane == 0)
			put_status(status[b], code, n);
		out_len = code == DS_OK ? n : 0;
		return code;
	}

	const int32_t mis = int32_t(reinterpret_cast<uintptr_t>(in) & 15u);
	const int32_t hb = int32_t(min(hist, int64_t(65535)));  // reachable history
	pattern_lut_init(D.plut);  // (LDS shared with pass 1: written per block)
	if (hb > 0) {
		// the ring's history: the previous block's last bytes
		for (int32_t x = (-min(hb + 16, ORING - 16)) & ~15; x < 0; x += 64 * 16)
			if (x + 16 * lane < 0)
				*reinterpret_cast<u32x4*>(&D.oring[uint32_t(x + 16 * lane) & OMASK]) =
				    gload16(reinterpret_cast<uintptr_t>(ob) + uintptr_t(intptr_t(x + 16 * lane)), olim);
		__builtin_amdgcn_s_waitcnt(0x0F70);  // settled before the batch loop (see fetch4)
		wave_lds_fence();
	}
	const uint64_t* tab = reinterpret_cast<const uint64_t*>(tab_all) + (((d.in_off >> 8) + b) << 3);
	const int32_t nsub = (n + SUB - 1) / SUB;
	const uintptr_t abase = reinterpret_cast<uintptr_t>(in) - uintptr_t(mis);

	Src S;
	S.lds = D.ring;
	S.mask = RING - 1;
	S.mis = mis;
	S.in = in;
	S.lim = lim;

	// input chunks staged: [hi - 4, hi) are in the ring, and the records of
	// sub-segments [64 (hi - 4), 64 hi) in rrec (loaded with the input: a
	// record load of its own per batch would wait on the previous flush)
	int32_t hi = 0;
	u32x4 pf0, pf1;  // chunk hi, loaded ahead
	load_chunk2(abase, 0, lim, pf0, pf1);
	auto load_rec = [&](int32_t c) -> uint64_t {
		const int32_t k = 64 * c + lane;
		return k < nsub ? __builtin_nontemporal_load(tab + k) : 0;
	};
	uint64_t pr = load_rec(0);
	// settled before the loop: left pending, the loop head's merge would
	// make every batch's staging wait vmcnt(0) (flush stores included)
	vm_wait();

	ISTAMP_DECL;
	int32_t o_batch = 0;  // output position of the current batch
	bool bad = false;
	bool d1 = false;  // a match with offset >= D1_OFF reads before the block start
	// the host's prediction of the round state (linked bulk path): quirk D1
	// emulated under it (d1x: a D1 match it cannot emulate declines the
	// block; the status says AUX_D1_EMU: decoded under the prediction)
	const bool d1p = D1E && (d.flags & BLOCK_D1_ROUND) != 0;  // (D1E: the linked planes' kernels)
	const int32_t oph = int32_t(HISTORY_SIZE) + int32_t((d.flags >> BLOCK_D1_OPH_SHIFT) & 7u);
	const int32_t n1 = int32_t(d.flags >> BLOCK_N1_SHIFT);
	bool d1x = false;
	// the previous batch's last match (block-relative output start, offset,
	// length; pml = 0: none known) for a D1 match without literals in lane 0
	int32_t pmd_b = 0, pof_b = 0, pml_b = 0;
	bool deep = false;  // ZL: a match reads history positions below 256
	int32_t hcnt = 0;   // ZL: match bytes read straight from the history region
	for (int32_t k0 = 0; k0 < nsub && !bad;) {
		// stage input so that [k0*SUB, k0*SUB + 4 KiB) is readable
		const int32_t cf = (k0 * SUB + mis) / BATCH;
		bool staged = false;
		if (hi < cf + 3) {
			staged = true;
			auto stage_one = [&]() {
				stage_chunk(D, hi, pf0, pf1, pr);
				++hi;
				load_chunk2(abase, hi, lim, pf0, pf1);
				pr = load_rec(hi);
			};
			// the first chunk outside the loop: its prefetch is settled (M's
			// wait), and inside a loop the wait pass would put a vmcnt(0) --
			// the previous batch's flush stores included -- before it too
			stage_one();
			while (hi < cf + 3)  // the block's first batch (and rarely later)
				stage_one();
			wave_lds_fence();
		}
		S.lo = max(hi - 4, 0) * BATCH - mis;
		S.hi = hi * BATCH - mis;

		ISTAMP(D_STAGE);
		ICOUNT(D_BATCHES, 1);
		const int32_t sub_s = (k0 + lane) * SUB;  // this lane's sub-segment
		const int32_t sub_end = min(sub_s + SUB, n);
		const BatchCut c = batch_cut(D, k0, nsub, LZ4ADA_OW_CUT, LZ4ADA_SEQ_CUT);
		const int32_t m = c.m;  // lanes [0, m) form an LDS batch
		const int32_t p0 = c.bm ? sub_s + __builtin_ctz(c.bm) : n;
		const int32_t o_lane = o_batch + c.incl - c.cnt;
		ISTAMP(D_WALK1);

		if (m == 0) {
			if (ZL) {  // (literals straight to HBM: the three-plane decode takes the block)
				bad = true;
				break;
			}
			// oversized: all 64 sub-segments straight to HBM
			const int32_t total = wave_last(c.incl);
			if (o_batch + total > cap) {
				bad = true;
				break;
			}
			flush_tail(D, ob, o_batch);
			vm_wait();
			if (!batch_global(S, ob, olim, p0, sub_end, n, o_lane, o_batch, hb)) {
				bad = true;
				break;
			}
			o_batch += total;
			pml_b = 0;  // (its sequences are not tracked for quirk D1)
			vm_wait();
			ICOUNT(D_GBATCHES, 1);
			// reload the ring's history from HBM
			const int32_t x0 = max(o_batch - ORING + 16, -((hb + 15) & ~15)) & ~15;
			for (int32_t x = x0 + 16 * lane; x < o_batch + 15; x += 64 * 16)
				*reinterpret_cast<u32x4*>(&D.oring[uint32_t(x) & OMASK]) =
				    gload16(reinterpret_cast<uintptr_t>(ob) + uintptr_t(intptr_t(x)), olim);
			wave_lds_fence();
			ISTAMP(D_GLOBAL);
			k0 += 64;
			continue;
		}

		const int32_t o_end = o_batch + wave_get(c.incl, m - 1);
		if (o_end > cap) {
			bad = true;
			break;
		}
		// the batch's sequence starts, in output order
		const int32_t base = k0 * SUB;
		if (lane < m) {
			int32_t e = c.incl_s - c.nseq;
			const uint16_t rel = uint16_t(sub_s - base);
			for (uint32_t bm = c.bm; bm; bm &= bm - 1)
				D.cst[e++] = uint16_t(rel + __builtin_ctz(bm));
		}
		wave_lds_fence();
		const int32_t N = wave_get(c.incl_s, m - 1);
		// HBM holds every byte below align_down(o_batch, 16) (earlier
		// flushes); a match reading below glo reads HBM (its source ends
		// before o_batch - 16), anything newer is in the ring
		const int32_t glo = o_batch - OW - 16;

		// P: parse 64 sequences per round, place them by a prefix sum
		int32_t rL[RMAX], rlit[RMAX], roff[RMAX], rml[RMAX], rdst[RMAX], rbeg[RMAX];
		bool pre = false, anyg = false;
		{
			int32_t o_round = o_batch;
			// both rounds' sequences parsed first (their starts are known, so
			// the four dependent LDS reads of the two rounds overlap), the
			// rare shapes the branch-free form rejects after, then placement
			// (mixed / dense / text -0.5..-0.9% against one round at a time,
			// profiles/r06u_psplit_ab.txt; 189 VGPRs)
			bool fok[RMAX];
#pragma unroll
			for (int r = 0; r < RMAX; ++r) {
				rL[r] = rlit[r] = roff[r] = rml[r] = 0;
				fok[r] = true;
				const int32_t idx = 64 * r + lane;
				if (idx < N) {
					Seq q;
					fok[r] = parse_fast_try(S, base + int32_t(D.cst[idx]), n, q);
					rL[r] = q.L;
					rlit[r] = q.lit;
					roff[r] = q.off;
					rml[r] = q.ml;
				}
			}
#pragma unroll
			for (int r = 0; r < RMAX; ++r) {
				if (__builtin_expect(__any(!fok[r]), 0)) {
					if (!fok[r]) {
						Seq q;
						parse_seq(S, base + int32_t(D.cst[64 * r + lane]), n, q);
						rL[r] = q.L;
						rlit[r] = q.lit;
						roff[r] = q.off;
						rml[r] = q.ml;
					}
				}
			}
#pragma unroll
			for (int r = 0; r < RMAX; ++r) {
				rbeg[r] = o_round;
				if (64 * r < N) {
					const int32_t len = rL[r] + rml[r];
					const int32_t inc = wave_incl_scan(len);
					rdst[r] = o_round + inc - len;  // literal destination
					o_round += wave_last(inc);
					const int32_t mdst = rdst[r] + rL[r];
					if (d1p) {
						// the previous sequence's match: lane - 1, lane 0 the
						// previous round's lane 63 or the previous batch's last
						int32_t pmd = __shfl(mdst, (lane + 63) & 63), pof = __shfl(roff[r], (lane + 63) & 63),
						        pml = __shfl(rml[r], (lane + 63) & 63);
						if (r > 0) {
							// (round 0 is full here: lane 63 parsed a sequence)
							const int32_t a = wave_last(rdst[0] + rL[0]), b = wave_last(roff[0]),
							              c = wave_last(rml[0]);
							if (lane == 0) {
								pmd = a;
								pof = b;
								pml = c;
							}
						} else if (lane == 0) {
							pmd = pmd_b;
							pof = pof_b;
							pml = pml_b;
						}
						if (rml[r] > 0 && !d1_emulable(mdst, rL[r], rlit[r], roff[r], rml[r], pmd, pof, pml, n1,
						                               oph, n))
							d1x = true;
					}
					if (rml[r] > 0) {
						if (roff[r] > mdst + hb)
							pre = true;  // reference before the block start (D2) / history
						if (roff[r] > mdst && roff[r] >= D1_OFF)
							d1 = true;
						if (ZL && roff[r] > mdst + 65280)
							deep = true;
						if (ZL && roff[r] > mdst)
							hcnt += min(rml[r], roff[r] - mdst);
						if (mdst - roff[r] < glo)
							anyg = true;
					}
				}
			}
		}
		if (__any(pre || d1x)) {
			bad = true;
			break;
		}
		if (d1p) {  // the batch's last sequence, for the next batch's lane 0
			const int32_t l = (N - 1) & 63;
			const bool r1 = N > 64;
			pmd_b = wave_get(r1 ? rdst[1] + rL[1] : rdst[0] + rL[0], l);
			pof_b = wave_get(r1 ? roff[1] : roff[0], l);
			pml_b = wave_get(r1 ? rml[1] : rml[0], l);
		}
		ISTAMP(D_WALK2);

		// HBM-sourced matches: every load in flight before the first use.  A
		// match's last 16-byte piece, the only one that can be short, loads
		// in its own lane; the pieces before it (long matches) of both
		// rounds are dealt over the wave, one per lane, through the LDS
		// match descriptors, and are stored whole (no in-batch HBM match
		// overlaps its source: that lies more than OW back, and a batch
		// holds at most OW bytes).  More than 64 is common
		// where matches are long and far (over a third of the mixed class's
		// batches, by about 7 pieces): the pieces beyond load here too, in
		// lanes whose own slot vg[r][0] is idle because their match is not
		// HBM-sourced (BORROW rounds' slots; off under quirk D1's prediction
		// and in the zero plane).  Only what finds no idle slot loads in M.
		const int BORROW = (D1E || ZL) ? 0 : BORROW_SLOTS;
		u32x4 vg[RMAX][GC], vr = u32x4{0u, 0u, 0u, 0u};
		int32_t rtot[RMAX], rfirst[RMAX];  // pieces beyond GC per round; the first not dealt here
		int32_t rpd = 0;                   // this lane's dealt piece (16 whole bytes)
		bool rph = false;                  // ... and whether it has one
		// a piece beyond the 64 dealt ones, loaded into this lane's idle
		// vg[r][0]: batch-relative output position (12 bits: a batch is at
		// most OW bytes), its 16 bytes' length << 12 (0: none)
		static_assert(OW <= 4096, "a borrowed piece's position takes 12 bits");
		int32_t bpc[RMAX];
#pragma unroll
		for (int r = 0; r < RMAX; ++r)
			rtot[r] = rfirst[r] = bpc[r] = 0;
		if (__any(anyg)) {
			// the previous batch's flush (FLUSH_ST store instructions) and
			// the input and record prefetch (3 loads, when this batch
			// staged) may stay in flight; everything older -- earlier
			// flushes -- is complete
			if (staged)
				asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FLUSH_ST + 3) : "memory");
			else
				asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FLUSH_ST) : "memory");
			int32_t nc[RMAX];
#pragma unroll
			for (int r = 0; r < RMAX; ++r) {
				nc[r] = 0;
				if (64 * r < N) {
					const int32_t src = rdst[r] + rL[r] - roff[r];
					const bool g = rml[r] > 0 && src < glo;
					// the own piece is the match's last (1..16 bytes; the load
					// reads up to 15 bytes past the source's end: still below
					// the match's own destination, and never stored)
					static_assert(GC == 1, "one own HBM piece per match: its last");
					if (g)
						__builtin_memcpy(&vg[r][0], ob + src + (((rml[r] - 1) >> 4) << 4), 16);
					nc[r] = g ? max(((rml[r] + 15) >> 4) - GC, 0) : 0;
					GCOUNT(0, __popcll(__ballot(g)));
					GCOUNT(1, __popcll(__ballot(g)) + __popcll(__ballot(g && ((src & 127) > 112))));
				}
			}
			GCOUNT(2, 1);
			static_assert(RMAX == 2, "HBM piece dealing pairs two rounds");
			if (__any(nc[0] > 0 || nc[1] > 0)) {
				const Deal2 dl = deal2(nc[0], nc[1]);
				rtot[0] = dl.tot0;
				rtot[1] = dl.tot - dl.tot0;
				rfirst[0] = 64;
				rfirst[1] = max(64 - dl.tot0, 0);
				auto pack = [&](int32_t md, int32_t of, int32_t m, int32_t excl) -> uint64_t {
					return deal_pack(md - o_batch, of, m, excl);
				};
				D.ldesc[lane] = pack(rdst[0] + rL[0], roff[0], rml[0], dl.inc0 - nc[0]);
				D.ldesc[64 + lane] = pack(rdst[1] + rL[1], roff[1], rml[1], dl.inc1 - nc[1]);
				const int32_t lo = min(chunk_owner2(D, dl.inc0, nc[0], dl.inc1, nc[1], 0), 127);
				const DealRun u = deal_unpack(D.ldesc[lo]);
				const int32_t od = o_batch + u.src, ooff = u.aux;
				// (a match's dealt pieces are its pieces 0 .. K - 2, whole; its
				// last is its own lane's)
				const int32_t k = lane - u.excl;
				GCOUNT(0, __popcll(__ballot(lane < dl.tot)));
				GCOUNT(1, __popcll(__ballot(lane < dl.tot)) +
				              __popcll(__ballot(lane < dl.tot && ((od - ooff + 16 * k) & 127) > 112)));
				if (lane < dl.tot) {
					rpd = od + 16 * k;
					rph = true;
					__builtin_memcpy(&vr, ob + (od - ooff) + 16 * k, 16);
				}
				if (dl.tot > 64) {
					ICOUNT(D_HOVF_B, 1);
					ICOUNT(D_HOVF_P, dl.tot - 64);
				}
				if (BORROW && dl.tot > 64) {
					// pieces 64 ..: one each to the lanes whose own-piece slot
					// vg[r][0] is idle (the round's match is not HBM-sourced),
					// round 0's idle lanes first, in lane order.  The idle lane
					// of rank i takes piece first + i; its owner is entry i -
					// 64 + first of the second chunk's owners.
					const int32_t own2 = min(chunk_owner2(D, dl.inc0, nc[0], dl.inc1, nc[1], 64), 127);
					int32_t first = 64;
#pragma unroll
					for (int r = 0; r < RMAX; ++r) {
						if (r >= BORROW)
							break;
						const bool idle = 64 * r < N && !(rml[r] > 0 && rdst[r] + rL[r] - roff[r] < glo);
						const uint64_t im = __ballot(idle);
						const int32_t t = first + int32_t(__builtin_amdgcn_mbcnt_hi(
						                              uint32_t(im >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(im), 0u)));
						const int32_t bo = __shfl(own2, (t - 64) & 63);
						if (idle && t < min(dl.tot, 128)) {
							const DealRun bu = deal_unpack(D.ldesc[bo]);
							const int32_t bk = t - bu.excl;
							bpc[r] = (bu.src + 16 * bk) | (16 << 12);  // (a dealt piece: whole)
							__builtin_memcpy(&vg[r][0], ob + (o_batch + bu.src - bu.aux) + 16 * bk, 16);
						}
						first = min(first + __popcll(im), min(dl.tot, 128));
					}
					rfirst[0] = first;
					rfirst[1] = max(first - dl.tot0, 0);
				}
				wave_lds_fence();  // ldesc / own[] are written again later
			}
		}
		ISTAMP(D_TLDS);

		// L: literals (input ring -> output ring).  A run of K 16-byte
		// pieces stores its last one, the only one that can be short, in
		// its own lane with the exact-length store; the K - 1 pieces before
		// it (runs over 16 bytes) of both rounds are dealt over the wave
		// together, each piece reading its run from an LDS descriptor and
		// storing 16 whole bytes that lie inside its run.  (Storing a short
		// last piece as 16 bytes that spill into its own match, rewritten
		// in M, measured no faster.)
		static_assert(RMAX == 2, "literal dealing pairs two rounds");
		{
			const int32_t nc0 = rL[0] > 16 ? (rL[0] - 1) >> 4 : 0;
			const int32_t nc1 = rL[1] > 16 ? (rL[1] - 1) >> 4 : 0;
#pragma unroll
			for (int r = 0; r < RMAX; ++r) {  // (rL = 0 also where a round has no sequence: n = 0)
				const int32_t c = 16 * (r == 0 ? nc0 : nc1);  // the last piece's place in the run
				ostore(D, rdst[r] + c, ZL ? u32x4{ 0u, 0u, 0u, 0u } : fetch16(S, rL[r] > 0 ? rlit[r] + c : S.lo),
				       rL[r] - c);
			}
			if (__any(nc0 > 0 || nc1 > 0)) {
				const Deal2 dl = deal2(nc0, nc1);
				auto pack = [&](int32_t lit, int32_t dst, int32_t L, int32_t excl) -> uint64_t {
					return deal_pack(lit - base, dst - o_batch, L, excl);
				};
				D.ldesc[lane] = pack(rlit[0], rdst[0], rL[0], dl.inc0 - nc0);
				D.ldesc[64 + lane] = pack(rlit[1], rdst[1], rL[1], dl.inc1 - nc1);
				for (int32_t t0 = 0; t0 < dl.tot; t0 += 64) {
					const int32_t t = t0 + lane;
					const int32_t lo = min(chunk_owner2(D, dl.inc0, nc0, dl.inc1, nc1, t0), 127);
					const DealRun u = deal_unpack(D.ldesc[lo]);
					const int32_t lit = base + u.src, dst = o_batch + u.aux;
					const int32_t k = t - u.excl;  // pieces 0 .. K - 2 (the last went in-lane)
					const bool has = t < dl.tot;
					ostore16(D, dst + 16 * k, ZL ? u32x4{ 0u, 0u, 0u, 0u } : fetch16(S, has ? lit + 16 * k : S.lo),
					         has);
				}
			}
		}
		wave_lds_fence();
		ISTAMP(D_LIT);

		// M: matches.  HBM-sourced matches store the pieces loaded in P,
		// both rounds first.  Every match whose source is in the LDS ring --
		// before the batch, in its own literals, or in this batch's match
		// output (near) -- is then cut into pieces dealt over the wave, both
		// rounds together in output order, 16 bytes each (a period-off
		// pattern: stp bytes, so every piece starts at phase 0), so a batch
		// costs its piece count / 64, not its longest match.  A piece
		// reading this chunk's output runs once every lower lane it reads
		// from has stored (one AND against a ballot per step; pieces of one
		// match never read each other: match byte i is source byte i mod
		// off).
		int32_t mring[RMAX], oring[RMAX], lring[RMAX];  // the rounds' ring-sourced matches
		// settle the HBM match loads in every lane: their first uses below
		// are lane-divergent, and a load left pending on the path that skips
		// them makes each later reuse of its registers wait vmcnt(0) (one
		// showed up inside the near-match loop)
		__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
		// pieces of HBM-sourced matches before their last, dealt and loaded
		// in P (the first 64 of the batch): 16 whole bytes inside their match
		ostore16(D, rpd, vr, rph);
#pragma unroll
		for (int r = 0; r < RMAX; ++r) {
			mring[r] = oring[r] = lring[r] = 0;
			if (64 * r < N) {
				const int32_t mdst = rdst[r] + rL[r], off = roff[r], ml = rml[r];
				const bool hbm = ml > 0 && mdst - off < glo;
				static_assert(GC == 1, "one own HBM piece per match");
				// the match's last piece, the one that can be short, loaded in
				// its own lane (the slot of a match that is not HBM-sourced may
				// hold a borrowed whole piece of another match instead: bpc,
				// set in P)
				const int32_t mc = ((ml - 1) >> 4) << 4;
				ostore(D, hbm ? mdst + mc : o_batch + (bpc[r] & 0xfff), vg[r][0], hbm ? ml - mc : bpc[r] >> 12);
				// dealt pieces that found no lane in P load now and are waited
				// for on the spot (over a third of the mixed class's batches
				// without BORROW)
				if (rtot[r] > rfirst[r]) {
					ICOUNT(D_HSLOW_B, r == 0 || rtot[0] <= rfirst[0]);
					ICOUNT(D_HSLOW_P, rtot[r] - rfirst[r]);
					const int32_t nc = hbm ? max(((ml + 15) >> 4) - GC, 0) : 0;
					const int32_t inc = wave_incl_scan(nc);
					for (int32_t t0 = rfirst[r]; t0 < rtot[r]; t0 += 64) {
						const int32_t t = t0 + lane;
						const int32_t lo = piece_owner(inc, t);
						const int32_t k = t - (__shfl(inc, lo) - __shfl(nc, lo));
						const int32_t osrc = __shfl(mdst - off, lo), odst = __shfl(mdst, lo);
						const bool has = t < rtot[r];
						u32x4 v = u32x4{ 0u, 0u, 0u, 0u };
						if (has)
							__builtin_memcpy(&v, ob + osrc + 16 * k, 16);
						ostore16(D, odst + 16 * k, v, has);
					}
					// settle this rare path's loads (see fetch4)
					__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
				}
				int32_t xoff = off, xml = (ml > 0 && !hbm) ? ml : 0;  // its ring copy, if any
				// (after every store of this round's HBM pieces, the loop
				// above included: the D1 bytes overwrite the start of piece 0
				// of their match, which is a dealt piece when the match is
				// over 16 bytes, and a wave's LDS stores take effect in the
				// order they are issued)
				if (d1p) {
					// quirk D1 (d1_emulable): the match's first k1 bytes are
					// what the last wild copy left past the frontier, from d =
					// OPH - off on -- the payload bytes after its literals, or
					// (no literals) the output bytes after the previous
					// match's source, which P put in rlit (a D1 match reads
					// >= 65,529 back: always HBM-sourced, stored above).  Those
					// output bytes: from HBM when flushed (below glo), else a
					// ring copy of their own (offset mdst - q, k1 bytes) among
					// the batch's ring matches, which orders it after the
					// bytes' producers and before their readers
					int32_t k1 = 0, sp = S.lo, gq = 0;
					bool fo = false;
					if (ml > 0 && n1 + mdst < off && oph - off < 8) {
						const int32_t dd = oph - off;
						const int32_t ovs = rL[r] > 0 ? 8 * ((rL[r] + 7) >> 3) - rL[r] : rlit[r] & 7;
						if (dd < ovs) {
							k1 = min(ovs - dd, ml);
							if (rL[r] > 0) {
								sp = rlit[r] + rL[r] + dd;
							} else {
								gq = (rlit[r] >> 3) - D1_QBIAS + dd;
								fo = true;
							}
						}
					}
					if (fo && gq >= glo) {
						xoff = mdst - gq;
						xml = k1;
						k1 = 0;
						fo = false;
					}
					u32x4 v = ZL ? u32x4{ 0u, 0u, 0u, 0u } : fetch16(S, sp);
					if (fo)
						__builtin_memcpy(&v, ob + gq, 16);
					ostore(D, mdst, v, k1);
				}
				mring[r] = mdst;
				oring[r] = xoff;
				lring[r] = xml;
			}
		}
		// every HBM-sourced match of the batch is stored before the ring
		// matches run (none reads another's output: their sources are in HBM)
		wave_lds_fence();
		ISTAMP(D_MFAR);
		// ring-sourced matches: with a long one (over RING_LANE_MAX bytes) in
		// the batch, the pieces of both rounds are dealt over the wave
		// together; rounds of short ones only (e.g. dense data) keep one lane
		// per match -- the dealing's fixed cost (owner search, dependency
		// masks) would dominate there
		static_assert(RMAX == 2, "ring dealing pairs two rounds");
		if (__any(lring[0] > RING_LANE_MAX || lring[1] > RING_LANE_MAX)) {
			const int32_t st = ring_pieces(D, mring, oring, lring, o_batch);
			ICOUNT(D_TASKS, 1);
			ICOUNT(D_ROUNDS, st);
#ifdef LZ4ADA_IDX_STAMPS
			{
				const int32_t tot = wave_last(wave_incl_scan(ring_piece_count(oring[0], lring[0]) +
				                                             ring_piece_count(oring[1], lring[1])));
				ICOUNT(D_RCHUNKS, (tot + 63) >> 6);
				ICOUNT(D_ROVF_B, tot > 64);
				ICOUNT(D_ROVF_P, max(tot - 64, 0));
			}
#endif
			(void)st;
		} else {
#pragma unroll
			for (int r = 0; r < RMAX; ++r) {
				if (64 * r < N) {
					const int32_t st = ring_lanes(D, mring[r], oring[r], lring[r], rbeg[r], rL[r], glo);
					ICOUNT(D_GBATCHES, 1);
					ICOUNT(D_LANES, st);
					(void)st;
				}
			}
		}
		ISTAMP(D_NEAR);

		flush_units(ob, D.oring, OMASK, o_batch, o_end);  // (P's vmcnt wait counts its stores)
		o_batch = o_end;
		k0 += m;
		ISTAMP(D_FLUSH);
	}
	d1 = __any(d1);
	deep = __any(deep);
	if (ZL)
		hcnt = wave_last(wave_incl_scan(hcnt));
	if (!bad && lane == 0 && (o_batch & 15))  // last partial unit
		gstore_n(ob + (o_batch & ~15), *reinterpret_cast<const u32x4*>(&D.oring[(o_batch & ~15) & OMASK]),
		         o_batch & 15);
	if (lane == 0) {
		if (bad) {
			status[b].code = DS_RETRY;
		} else {
			status[b].code = DS_OK;
			status[b].aux = (d1 ? AUX_D1_RISK : 0) | (d1p ? AUX_D1_EMU : 0) | (deep ? AUX_DEEP_HIST : 0);
			status[b].detail = ZL ? hcnt : 0;  // ZL: the linked path's density estimate
			status[b].err_out_pos = 0;
			status[b].out_len = uint32_t(o_batch);
		}
	}
	ISTAMP_FLUSH();
	out_len = bad ? 0 : o_batch;
	return bad ? DS_RETRY : DS_OK;
}

// What k_decode_idx runs (its runtime argument).
enum KIdxMode : int {
	K_PASS2 = 0,   // pass 2 of independent blocks, one wave per block
	K_SERIAL = 1,  // a linked frame in contiguous slots, launched as one workgroup
	K_HIST = 2,    // K_PASS2 with LINK_HIST history bytes before each slot: no launcher passes it
	               // (k_decode_idx_lk took over); kept because the bench ran slower without the arm
	K_FUSED = 3,   // K_PASS2 after pass 1 of the same block by the same wave
};

// Independent blocks (K_PASS2, K_FUSED): one wave per block.  Linked frames
// in contiguous slots (K_SERIAL, launched as one workgroup): the blocks in
// order, each reading the previous ones' output as history while every
// block so far is full (its slot then continues the previous one); a
// declined or short block leaves every later block DS_RETRY for the exact
// path.  (Linked frames in the history layout of lz4ada_linked.hip have the
// two kernels below.)  Pinned to two waves per SIMD (at most 256 registers,
// so the allocator never reaches for AGPRs): LDS allows 8 waves per CU, and
// the bench's 2048 blocks are all resident.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_decode_idx(const uint8_t* __restrict__ frame,
                                                    uint64_t frame_len,
                                                    const lz4ada_block_desc* __restrict__ desc,
                                                    uint32_t nblocks, uint8_t* __restrict__ tab_all,
                                                    uint8_t* __restrict__ out,
                                                    lz4ada_block_status* __restrict__ status,
                                                    int mode)
{
	__shared__ union {
		DecLds d;
		IdxLds<1> x;
	} U;
	DecLds& D = U.d;
	if (mode == K_FUSED) {
		// pass 1 of this block first (its table and status, read
		// below by this same wave, made visible to it first), so a block's pass 2
		// starts when its own pass 1 is done, not when every block's is
		if (blockIdx.x < nblocks)
			index_block<1>(U.x, frame, frame_len, desc, blockIdx.x, tab_all, status);
		// workgroup scope is enough (the same wave reads it back); an agent
		// fence here wrote the whole L2 back once per block
		vm_wait();
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
		__syncthreads();
		mode = K_PASS2;
	}
	// one call site of decode_block for every mode (code size)
	const bool serial = mode == K_SERIAL;
	int64_t hist = mode == K_HIST ? LINK_HIST : 0;
	uint32_t b = serial ? 0u : blockIdx.x;
	const uint32_t bend = serial ? nblocks : min(blockIdx.x + 1u, nblocks);
	for (; b < bend; ++b) {
		int32_t len;
		const int32_t code = decode_block(D, frame, frame_len, desc, b, tab_all, out, status,
		                                  hist, len);
		if (!serial)
			return;
		vm_wait();  // the next block reads this output as history
		__syncthreads();
		if (code != DS_OK)
			break;
		if (b + 1 < nblocks && (uint32_t(len) != desc[b].out_cap ||
		                        desc[b + 1].out_off != desc[b].out_off + uint64_t(len))) {
			++b;  // the next block's history would not be contiguous
			break;
		}
		hist += len;
	}
	if (!serial)
		return;
	for (uint32_t r = b + lane_id(); r < nblocks; r += 64)
		if (status[r].code == DS_OK || r > b)
			status[r].code = DS_RETRY;
}


// The linked path's literal-zero plane (decode_block<true>): pass 2 of every
// block in the history layout, one wave per block.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_decode_idx_zl(
        const uint8_t* __restrict__ frame, uint64_t frame_len, const lz4ada_block_desc* __restrict__ desc,
        uint32_t nblocks, uint8_t* __restrict__ tab_all, uint8_t* __restrict__ out,
        lz4ada_block_status* __restrict__ status)
{
	__shared__ DecLds D;
	if (blockIdx.x >= nblocks)
		return;
	int32_t len;
	decode_block(D, frame, frame_len, desc, blockIdx.x, tab_all, out, status, LINK_HIST, len, true, true);
}

// The linked path's byte planes (x, and y / h when a block needs them):
// pass 2 of every block in the history layout with quirk D1 emulated under
// the host's predicted round state (decode_block's D1E).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_decode_idx_lk(
        const uint8_t* __restrict__ frame, uint64_t frame_len, const lz4ada_block_desc* __restrict__ desc,
        uint32_t nblocks, uint8_t* __restrict__ tab_all, uint8_t* __restrict__ out,
        lz4ada_block_status* __restrict__ status)
{
	__shared__ DecLds D;
	if (blockIdx.x >= nblocks)
		return;
	int32_t len;
	decode_block(D, frame, frame_len, desc, blockIdx.x, tab_all, out, status, LINK_HIST, len, false, true);
}

// One chain of linked blocks [first, bend), walked by one wave: pass 2 over
// them in order, as K_SERIAL does for one frame.  Each block reads `hist` bytes
// in front of its slot as history: what the caller starts with (nothing, a
// dictionary's tail, a checkpoint) and the earlier blocks' output, while every
// block so far is full and its slot continues the previous one.  The walk ends
// before `stop` (the caller passes bend, or first when it refuses the chain's
// layout) and at the first block that is declined, short or not followed by a
// contiguous slot; the blocks before that one keep DS_OK, its own status is
// pass 2's, and every later block of the chain gets DS_RETRY.  Pass 1 is an
// ordinary launch_index over the same descriptors, ahead of the kernel.  The
// caller clamps [first, bend) to the launch's blocks, so no status and no slot
// outside the chain is written whatever its record says.
//
// D1: quirk D1 from the real round state.  The wave knows every decoded
// length, so it replays Output_Pos / Output_Pos_History as the host does for one
// linked frame (lz4ada_bulk_linked.cpp: opos = 0 when >= 65536 at a block's
// start, opos += len, oph = opos when >= 65536).  A block that pass 2 flagged
// AUX_D1_RISK while oph is in [65536, 65542] gets DS_RETRY and ends the chain
// (nothing is emulated here: D1E stays false); outside that state the flagged
// match reads plain history.  Without D1 the semantics are the LZ4
// specification's and the flag is ignored.
//
// (The pointers are the kernels' __restrict__ parameters; saying it here again
// cost k_decode_idx_frames three VGPRs.)
template <bool D1>
__device__ __forceinline__ void decode_chain(DecLds& D, const uint8_t* frame, uint64_t frame_len,
                                             const lz4ada_block_desc* desc, uint8_t* tab_all, uint8_t* out,
                                             lz4ada_block_status* status, uint32_t first, uint32_t bend,
                                             uint32_t stop, int64_t hist)
{
	int64_t opos = 0, oph = 0;
	for (uint32_t b = first; b < stop; ++b) {
		if (D1 && opos >= HISTORY_SIZE)
			opos = 0;
		const bool in_d1 = D1 && oph >= HISTORY_SIZE && oph <= HISTORY_SIZE + 6;
		int32_t len;
		const int32_t code = decode_block(D, frame, frame_len, desc, b, tab_all, out, status, hist, len);
		vm_wait();  // the next block reads this output as history
		__syncthreads();
		if (code != DS_OK) {
			stop = b + 1;  // (its own status is non-zero already)
			break;
		}
		if (in_d1) {
			// the flag lane 0 has just stored (complete: vm_wait), read past
			// the L1 line this wave filled when it read the status before
			const int32_t aux = __builtin_amdgcn_readfirstlane(
			    __hip_atomic_load(&status[b].aux, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
			if (aux & AUX_D1_RISK) {
				stop = b;
				break;
			}
		}
		if (D1) {
			opos += len;
			if (opos >= HISTORY_SIZE)
				oph = opos;
		}
		if (b + 1 < bend && (uint32_t(len) != desc[b].out_cap ||
		                     desc[b + 1].out_off != desc[b].out_off + uint64_t(len))) {
			stop = b + 1;  // the next block's history would not be contiguous
			break;
		}
		hist += len;
	}
	for (uint32_t r = stop + lane_id(); r < bend; r += 64)
		status[r].code = DS_RETRY;
}

// Many linked frames side by side (a many-frame pass): one wave
// per frame of the pass.  Workgroup f takes the blocks [first, first + nblocks)
// of frames[f] when the record carries FRAME_LINKED (any other frame is
// another launch's) and walks them as one chain without history in front, with
// quirk D1's round state (decode_chain<true>).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_decode_idx_frames(
        const uint8_t* __restrict__ frame, uint64_t frame_len, const lz4ada_block_desc* __restrict__ desc,
        uint32_t nblocks, uint8_t* __restrict__ tab_all, uint8_t* __restrict__ out,
        lz4ada_block_status* __restrict__ status, const FrameRec* __restrict__ frames, uint32_t nframes)
{
	__shared__ DecLds D;
	if (blockIdx.x >= nframes)
		return;
	const uint32_t flags = frames[blockIdx.x].flags;
	if (!(flags & FRAME_LINKED))
		return;
	const uint32_t first = min(frames[blockIdx.x].first, nblocks);
	const uint32_t bend = first + min(frames[blockIdx.x].nblocks, nblocks - first);
	decode_chain<true>(D, frame, frame_len, desc, tab_all, out, status, first, bend, bend, 0);
}

// Dictionary frames.  A block whose descriptor carries
// BLOCK_DICT has `G` bytes in front of its slot whose last dict_used are the
// dictionary's last (k_dict_fill, lz4ada_dict.hip): to decode_block they are
// history like a linked frame's earlier output.  The semantics are the LZ4
// specification's: no quirk-D1 round state, AUX_D1_RISK is ignored.  One
// caution of decode_block's remains, because the function is shared with the
// other decoders as it is (a parameter for it changed their code): an
// oversized batch (batch_global) declines a match that starts before the block
// with an offset of D1_OFF or more, so such a block fails its frame and the
// caller's host decode takes it.

// Independent blocks against the dictionary: one wave per block, pass 2 over a
// table from launch_index over the same descriptors.  A block without
// BLOCK_DICT (a legacy frame's) reads no history.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_decode_idx_dict(
        const uint8_t* __restrict__ frame, uint64_t frame_len, const lz4ada_block_desc* __restrict__ desc,
        uint32_t nblocks, uint8_t* __restrict__ tab_all, uint8_t* __restrict__ out,
        lz4ada_block_status* __restrict__ status, uint32_t dict_used)
{
	__shared__ DecLds D;
	if (blockIdx.x >= nblocks)
		return;
	const uint32_t fl = wave_uniform(desc[blockIdx.x].flags);
	int32_t len;
	decode_block(D, frame, frame_len, desc, blockIdx.x, tab_all, out, status,
	                   (fl & BLOCK_DICT) ? int64_t(dict_used) : 0, len);
}

// k_decode_idx_frames with the dictionary before each linked frame's first
// block: the chain starts with dict_used bytes of history when that block
// carries BLOCK_DICT, with none when it does not (decode_chain<false>).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_decode_idx_frames_dict(
        const uint8_t* __restrict__ frame, uint64_t frame_len, const lz4ada_block_desc* __restrict__ desc,
        uint32_t nblocks, uint8_t* __restrict__ tab_all, uint8_t* __restrict__ out,
        lz4ada_block_status* __restrict__ status, const FrameRec* __restrict__ frames, uint32_t nframes,
        uint32_t dict_used)
{
	__shared__ DecLds D;
	if (blockIdx.x >= nframes)
		return;
	const uint32_t flags = frames[blockIdx.x].flags;
	if (!(flags & FRAME_LINKED))
		return;
	const uint32_t first = min(frames[blockIdx.x].first, nblocks);
	const uint32_t bend = first + min(frames[blockIdx.x].nblocks, nblocks - first);
	if (first >= bend)
		return;
	const int64_t hist = (wave_uniform(desc[first].flags) & BLOCK_DICT) ? int64_t(dict_used) : 0;
	decode_chain<false>(D, frame, frame_len, desc, tab_all, out, status, first, bend, bend, hist);
}

// The chains of a ranged pass over a dictionary index: the
// starting history is read from the chain's record (`hash`, which chain records
// otherwise leave unused) instead of a launch argument, so one launch decodes
// chains that start from a checkpoint (65,536 bytes) beside chains that start
// from the dictionary (dict_used).  The history is clamped to DICT_MAX, and it
// is believed only where the layout can hold it: the chain's first block must
// carry BLOCK_DICT and lie at least dict_gap(hist) into the slots, else the
// chain's blocks get DS_RETRY and nothing is decoded (stop = first).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_decode_idx_chains(
        const uint8_t* __restrict__ frame, uint64_t frame_len, const lz4ada_block_desc* __restrict__ desc,
        uint32_t nblocks, uint8_t* __restrict__ tab_all, uint8_t* __restrict__ out,
        lz4ada_block_status* __restrict__ status, const FrameRec* __restrict__ chains, uint32_t nchains)
{
	__shared__ DecLds D;
	if (blockIdx.x >= nchains)
		return;
	const uint32_t flags = chains[blockIdx.x].flags;
	if (!(flags & FRAME_LINKED))
		return;
	const uint32_t first = min(chains[blockIdx.x].first, nblocks);
	const uint32_t bend = first + min(chains[blockIdx.x].nblocks, nblocks - first);
	if (first >= bend)
		return;
	const uint32_t h0 = min(wave_uniform(chains[blockIdx.x].hash), DICT_MAX);
	const bool holds = (wave_uniform(desc[first].flags) & BLOCK_DICT) && wave_uniform(desc[first].out_off) >= dict_gap(h0);
	decode_chain<false>(D, frame, frame_len, desc, tab_all, out, status, first, bend, holds ? bend : first,
	                    int64_t(h0));
}

#include "lz4ada_idx_pair.inc"    // PpLds2 / WP2, the LDS hand-offs, decode_block_pp2, k_decode_pp2

}  // namespace idx

#ifdef LZ4ADA_IDX_STAMPS
extern "C" int lz4ada_idx_stamps(unsigned long long* out, int reset)
{
	if (hipMemcpyFromSymbol(out, HIP_SYMBOL(idx::g_idx_stamps),
	                        sizeof(unsigned long long) * idx::IDX_NST) != hipSuccess)
		return -1;
	if (reset) {
		unsigned long long z[idx::IDX_NST] = {};
		if (hipMemcpyToSymbol(HIP_SYMBOL(idx::g_idx_stamps), z, sizeof z) != hipSuccess)
			return -1;
	}
	return idx::IDX_NST;
}
#endif

#ifdef LZ4ADA_IDX_GATHERS
extern "C" int lz4ada_idx_gathers(unsigned long long* out, int reset)
{
	if (hipMemcpyFromSymbol(out, HIP_SYMBOL(idx::g_idx_gathers), sizeof(unsigned long long) * 4) != hipSuccess)
		return -1;
	if (reset) {
		unsigned long long z[4] = {};
		if (hipMemcpyToSymbol(HIP_SYMBOL(idx::g_idx_gathers), z, sizeof z) != hipSuccess)
			return -1;
	}
	return 4;
}
#endif

// index table: 8 records of 8 bytes per 256-byte segment, per block at
// record ((in_off >> 8) + b) * 8
size_t index_table_bytes(uint64_t frame_len, uint32_t nblocks)
{
	return ((size_t(frame_len) >> 8) + size_t(nblocks) + 2) * 64;
}

hipError_t launch_index(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                        uint32_t nblocks, uint8_t* d_tab, lz4ada_block_status* d_status,
                        hipStream_t stream, int waves)
{
	if (waves != 1 && waves != 2)
		return hipErrorInvalidValue;
	if (nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(waves == 2 ? idx::k_index<2> : idx::k_index<1>, dim3(nblocks), dim3(64 * waves), 0,
	                   stream, d_frame, frame_len, d_desc, nblocks, d_tab, d_status);
	return hipGetLastError();
}

hipError_t launch_decode_idx_tab(const uint8_t* d_frame, uint64_t frame_len,
                                 const lz4ada_block_desc* d_desc, uint32_t nblocks,
                                 const uint8_t* d_tab, uint8_t* d_out,
                                 lz4ada_block_status* d_status, IdxMode mode, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	uint8_t* tab = const_cast<uint8_t*>(d_tab);
	if (mode == IdxMode::PASS2 || mode == IdxMode::LINKED_SERIAL || mode == IdxMode::FUSED_ONE) {
		const bool serial = mode == IdxMode::LINKED_SERIAL;  // one workgroup, the blocks in order
		hipLaunchKernelGGL(idx::k_decode_idx, dim3(serial ? 1 : nblocks), dim3(64), 0, stream, d_frame,
		                   frame_len, d_desc, nblocks, tab, d_out, d_status,
		                   int(serial ? idx::K_SERIAL : (mode == IdxMode::PASS2 ? idx::K_PASS2 : idx::K_FUSED)));
	} else {
		const auto k = mode == IdxMode::LINKED_LK   ? idx::k_decode_idx_lk
		               : mode == IdxMode::LINKED_ZL ? idx::k_decode_idx_zl
		                                            : idx::k_decode_pp2;
		hipLaunchKernelGGL(k, dim3(nblocks), dim3(mode == IdxMode::FUSED_PAIR ? 128 : 64), 0, stream, d_frame,
		                   frame_len, d_desc, nblocks, tab, d_out, d_status);
	}
	return hipGetLastError();
}

hipError_t launch_decode_idx_frames(const uint8_t* d_frame, uint64_t frame_len,
                                    const lz4ada_block_desc* d_desc, uint32_t nblocks, const uint8_t* d_tab,
                                    uint8_t* d_out, lz4ada_block_status* d_status, const FrameRec* d_frames,
                                    uint32_t nframes, hipStream_t stream)
{
	if (nframes == 0 || nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(idx::k_decode_idx_frames, dim3(nframes), dim3(64), 0, stream, d_frame, frame_len, d_desc,
	                   nblocks, const_cast<uint8_t*>(d_tab), d_out, d_status, d_frames, nframes);
	return hipGetLastError();
}

hipError_t launch_decode_idx_dict(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                                  uint32_t nblocks, const uint8_t* d_tab, uint8_t* d_out,
                                  lz4ada_block_status* d_status, uint32_t dict_used, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(idx::k_decode_idx_dict, dim3(nblocks), dim3(64), 0, stream, d_frame, frame_len, d_desc,
	                   nblocks, const_cast<uint8_t*>(d_tab), d_out, d_status, dict_used);
	return hipGetLastError();
}

hipError_t launch_decode_idx_frames_dict(const uint8_t* d_frame, uint64_t frame_len,
                                         const lz4ada_block_desc* d_desc, uint32_t nblocks, const uint8_t* d_tab,
                                         uint8_t* d_out, lz4ada_block_status* d_status, const FrameRec* d_frames,
                                         uint32_t nframes, uint32_t dict_used, hipStream_t stream)
{
	if (nframes == 0 || nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(idx::k_decode_idx_frames_dict, dim3(nframes), dim3(64), 0, stream, d_frame, frame_len,
	                   d_desc, nblocks, const_cast<uint8_t*>(d_tab), d_out, d_status, d_frames, nframes, dict_used);
	return hipGetLastError();
}

hipError_t launch_decode_idx_chains(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                                    uint32_t nblocks, const uint8_t* d_tab, uint8_t* d_out,
                                    lz4ada_block_status* d_status, const FrameRec* d_chains, uint32_t nchains,
                                    hipStream_t stream)
{
	if (nchains == 0 || nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(idx::k_decode_idx_chains, dim3(nchains), dim3(64), 0, stream, d_frame, frame_len, d_desc,
	                   nblocks, const_cast<uint8_t*>(d_tab), d_out, d_status, d_chains, nchains);
	return hipGetLastError();
}

// The fused launch for independent blocks.  One wave per block
// (k_decode_idx) while the blocks fill the chip's SIMDs twice; two waves per
// block pipelining batches (k_decode_pp2) for at most 4 blocks per CU
// (measured, docs/DESIGN_LOG.md §3: 1,024 x 4 MiB mixed 12.0 -> 8.7 ms, but
// at 2,048 blocks 13.3 -> 18.0 ms).  LZ4ADA_IDX_WAVES=1 / p (or 2) forces
// one or the other.
IdxMode idx_fused_mode(uint32_t nblocks)
{
	static const char forced = [] {
		const char* e = getenv("LZ4ADA_IDX_WAVES");
		return e ? e[0] : '\0';
	}();
	if (forced == '1')
		return IdxMode::FUSED_ONE;
	if (forced == '2' || forced == 'p')
		return IdxMode::FUSED_PAIR;
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess)
		(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	return nblocks <= uint32_t(4 * cus) ? IdxMode::FUSED_PAIR : IdxMode::FUSED_ONE;
}

const char* idx_fused_kernel_name(uint32_t nblocks)
{
	return idx_fused_mode(nblocks) == IdxMode::FUSED_PAIR ? "k_decode_pp2" : "k_decode_idx";
}

hipError_t launch_decode_idx(const uint8_t* d_frame, uint64_t frame_len,
                             const lz4ada_block_desc* d_desc, uint32_t nblocks, uint8_t* d_out,
                             lz4ada_block_status* d_status, hipStream_t stream, IdxRun run)
{
	if (nblocks == 0)
		return hipSuccess;
	void* tab = nullptr;
	hipError_t err = hipMallocAsync(&tab, index_table_bytes(frame_len, nblocks), stream);
	if (err != hipSuccess)
		return err;
	// pass 1 as a launch of its own, or inside the FUSED modes' one launch
	const bool two = run == IdxRun::SPLIT || run == IdxRun::LINKED_SERIAL;
	const IdxMode mode = run == IdxRun::SPLIT           ? IdxMode::PASS2
	                     : run == IdxRun::LINKED_SERIAL ? IdxMode::LINKED_SERIAL
	                     : run == IdxRun::FUSED_ONE     ? IdxMode::FUSED_ONE
	                     : run == IdxRun::FUSED_PAIR    ? IdxMode::FUSED_PAIR
	                                                    : idx_fused_mode(nblocks);
	if (two)
		err = launch_index(d_frame, frame_len, d_desc, nblocks, static_cast<uint8_t*>(tab), d_status,
		                   stream);
	if (err == hipSuccess)
		err = launch_decode_idx_tab(d_frame, frame_len, d_desc, nblocks, static_cast<const uint8_t*>(tab),
		                            d_out, d_status, mode, stream);
	const hipError_t e2 = hipFreeAsync(tab, stream);
	return err != hipSuccess ? err : e2;
}

}  // namespace lz4ada
