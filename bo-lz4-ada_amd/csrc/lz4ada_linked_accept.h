// lz4ada_linked_accept.h -- the host decisions of the linked bulk path
// (lz4ada_bulk_linked.cpp) that touch no device: how a batch's
// blocks are laid into slots and which round state each is predicted to
// decode under, which blocks of a decoded batch the path accepts, and which
// planes the accepted ones need.  Standard library only, so a plain C++
// program can include it (tools/linked_accept_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "lz4ada_hip.h"
#include "lz4ada_round_state.h"

namespace lz4ada {

// Output slot capacity of one block: a stored block is its payload; a
// compressed one decodes to at most 255 bytes per payload byte (a length
// extension byte adds <= 255 to a match; everything else expands less), so
// a frame of many small flushed blocks does not reserve block_max each.
inline uint32_t slot_cap(const lz4ada_block_desc& d, int64_t bmax)
{
	if (d.flags & LZ4ADA_BLOCK_STORED)
		return d.in_len;
	return uint32_t(std::min<uint64_t>(uint64_t(bmax), 255ull * d.in_len + 64));
}

inline uint64_t round256(uint64_t v) { return (v + 255) & ~uint64_t(255); }

// A block status's code 0 is DS_OK (lz4ada_internal.h; "0 = ok" in lz4ada_hip.h).
inline bool status_ok(const lz4ada_block_status& s) { return s.code == 0; }

// A round state as a descriptor's flags carry it to the index decoder, which
// emulates quirk D1 under it: nothing outside a D1 round.
inline uint32_t d1_flags(const RoundState& at_start)
{
	if (!at_start.in_d1())
		return 0;
	return BLOCK_D1_ROUND | (uint32_t(at_start.history - HISTORY_SIZE) << BLOCK_D1_OPH_SHIFT) |
	       (uint32_t(at_start.pos) << BLOCK_N1_SHIFT);
}

// Laying a batch: every block's slot (out_cap) behind HISTORY_SIZE bytes of
// history region (out_off is the slot's), slots rounded to 256 bytes; the
// batch's bytes are returned.  Each block's flags get quirk D1's round state
// predicted from `rs`, the state before the batch, with every block filling
// its slot; accept_blocks takes a block decoded under a prediction only if
// the real state is the predicted one.
inline uint64_t lay_batch(std::vector<lz4ada_block_desc>& d, int64_t block_max, RoundState rs)
{
	uint64_t bytes = 0;
	for (auto& x : d) {
		x.out_cap = slot_cap(x, block_max);
		x.out_off = bytes + uint64_t(HISTORY_SIZE);
		bytes += uint64_t(HISTORY_SIZE) + round256(x.out_cap);
		rs.start();
		x.flags = (x.flags & (LZ4ADA_BLOCK_STORED | LZ4ADA_BLOCK_HAS_CKSUM)) | d1_flags(rs);
		rs.advance(int64_t(x.out_cap));
	}
	return bytes;
}

// Accepting blocks: the batch's leading blocks that the bulk path keeps,
// [0, count), `bytes` in all, block i starting at A[i]; rs moves over them.
// Block `count`, if there is one, is the first the exact path has to take: a
// block error, a checksum mismatch, or quirk D1 (a match
// reaching >= D1_OFF back into the history right after a block that ended at
// 65536..65542).  The blocks before it only point backwards, so they resolve
// on their own and the exact path resumes at it.
//
// Quirk D1: a block with a match >= D1_OFF back before its start
// (AUX_D1_RISK) in a round after one that ended at 65536..65542 is the
// decoders' only if the index decoder (which emulates D1) decoded it under
// the real round state; one decoded under a D1 prediction the real state does
// not have goes too (without such a match, neither the quirk nor the
// emulation changes a byte).  Where plane z declined, planes y and h come
// from k_decode_pc, which does not emulate D1 -- the planes would disagree.
//
// seen(i, rs, d1_bad) is called for every block looked at, the stopping one
// included, with the state at its start (the trace's line).
struct Accepted {
	uint32_t count = 0;
	int64_t bytes = 0;
};
template <class Seen>
inline Accepted accept_blocks(const std::vector<lz4ada_block_desc>& d, const std::vector<lz4ada_block_status>& stx,
                              const std::vector<lz4ada_block_status>& stz, RoundState& rs, int64_t* A, Seen&& seen)
{
	Accepted a;
	for (; a.count < d.size(); ++a.count) {
		const lz4ada_block_desc& x = d[a.count];
		const lz4ada_block_status& s = stx[a.count];
		rs.start();
		const bool emu = (s.aux & AUX_D1_EMU) != 0;
		const bool pred_ok = emu && rs.in_d1() && (x.flags & BLOCK_D1_ROUND) && status_ok(stz[a.count]) &&
		                     int64_t((x.flags >> BLOCK_D1_OPH_SHIFT) & 7u) == rs.history - HISTORY_SIZE &&
		                     int64_t(x.flags >> BLOCK_N1_SHIFT) == rs.pos;
		const bool d1_bad = (s.aux & AUX_D1_RISK) && (rs.in_d1() ? !pred_ok : emu);
		seen(a.count, rs, d1_bad);
		if (!status_ok(s) || ((x.flags & LZ4ADA_BLOCK_HAS_CKSUM) && s.cksum != x.cksum) || d1_bad)
			break;
		rs.advance(s.out_len);
		A[a.count] = a.bytes;
		a.bytes += s.out_len;
	}
	return a;
}

// Plane modes: what each accepted block needs beside planes x and z.  A block
// that reads history positions below 256 (AUX_DEEP_HIST: their high byte is 0,
// like a literal's) takes plane y too, mode 1 (x != y marks a history byte,
// k = x | z << 8); one z's decoder declined (oversized batches, anything pass 1
// declined) takes y and h, mode 2 -- the three-plane rule.  ny blocks take
// plane y, nh of them plane h.
struct PlaneCounts {
	uint32_t ny = 0, nh = 0;
};
inline PlaneCounts plane_modes(const std::vector<lz4ada_block_status>& stz, uint32_t count, uint8_t* mode)
{
	PlaneCounts c;
	for (uint32_t i = 0; i < count; ++i) {
		mode[i] = !status_ok(stz[i]) ? 2 : (stz[i].aux & AUX_DEEP_HIST) ? 1 : 0;
		c.ny += mode[i] != 0;
		c.nh += mode[i] == 2;
	}
	return c;
}

}  // namespace lz4ada
