// lz4ada_range_chains.h -- which blocks of a linked frame a ranged decode has
// to decode besides the ones its ranges touch, as host/device code (DESIGN.md
// §16).  A linked frame of nb blocks is cut into groups of K blocks; the seek
// index keeps, for every group start b = K, 2K, ... < nb, the 65,536 decoded
// bytes in front of block b (a history checkpoint).  A range that touches the
// blocks [a, z] (range_blocks, lz4ada_range_blocks.h) marks its *chain*: the
// blocks [chain_start(K, a), z].  A marked block b > 0 with b % K == 0 is a
// *head*: it is decoded with its checkpoint as history, in a wave of its own;
// a marked block 0 starts a chain without history; every other marked block
// continues the chain of the block before it.
//
// Why that suffices: the marks of one range are an interval that begins at a
// group start, so the marked blocks of any group, over any set of ranges, are
// a prefix of the group -- a marked block that is neither a head nor block 0
// always has its predecessor marked, and its history is decoded output.
//
// K == 0 stands for a frame of independent blocks: the chain is the touched
// blocks, and no block is a head.
//
// It is the one statement of the rule: k_ranges_select, k_ranges_fill and
// k_ranges_verdict (lz4ada_ranges.hip) and the host's sweep (plan_pass,
// lz4ada_bulk_ranges.cpp) call it, the host states it through
// lz4ada_range_chains_host, and tests/test_ranges_linked_cpu.py and
// tools/range_chains_asan.cpp pin it to a brute-force definition.  The gap
// count of an interval (chain_heads, and for a dictionary index
// chain_dict_gaps) goes through lz4ada_range_gaps_host, pinned likewise by
// tests/test_ranges_dict_cpu.py and tools/range_gaps_asan.cpp.
//
// Depends on nothing, so a plain C++ program can include it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4ADA_RC_HD __host__ __device__
#else
#define LZ4ADA_RC_HD
#endif

namespace lz4ada {

// Decoded bytes a checkpoint holds: the largest LZ4 offset plus one.
constexpr uint64_t CKPT_BYTES = 65536;

// The first block a range whose first touched block is `a` has to decode.
LZ4ADA_RC_HD inline uint64_t chain_start(uint64_t K, uint64_t a) { return K ? a / K * K : a; }

// Block b, when marked, is decoded from its checkpoint.
LZ4ADA_RC_HD inline bool chain_head(uint64_t K, uint64_t b) { return K && b > 0 && b % K == 0; }

// The heads among the blocks [lo, hi).
LZ4ADA_RC_HD inline uint64_t chain_heads(uint64_t K, uint64_t lo, uint64_t hi)
{
	if (!K || hi <= lo)
		return 0;
	return (hi - 1) / K - (lo ? (lo - 1) / K : 0);
}

// A seek index over dictionary frames knows a second kind of
// gap: the dictionary in front of a block that reads it.  Which blocks those
// are depends on the frame's kind alone (the values of DICT_KIND_*,
// lz4ada_internal.h): every block of an independent modern frame, block 0 of a
// linked one, none of a legacy frame's or in an index without a dictionary.
constexpr uint32_t CHAIN_KIND_NONE = 0, CHAIN_KIND_LINKED = 1, CHAIN_KIND_INDEP = 2;

// Block b, when marked, is decoded with the dictionary in front of it.
LZ4ADA_RC_HD inline bool chain_dict_gapped(uint32_t kind, uint64_t b)
{
	return kind == CHAIN_KIND_INDEP || (kind == CHAIN_KIND_LINKED && b == 0);
}

// The dictionary-gapped blocks among the blocks [lo, hi).  With chain_heads
// the gap count of an interval: no block takes both gaps (a head is not block
// 0, and an independent frame has no head).
LZ4ADA_RC_HD inline uint64_t chain_dict_gaps(uint32_t kind, uint64_t lo, uint64_t hi)
{
	if (hi <= lo)
		return 0;
	return kind == CHAIN_KIND_INDEP ? hi - lo : kind == CHAIN_KIND_LINKED && lo == 0 ? 1 : 0;
}

// Past the last block of b's group in a frame of nb blocks.
LZ4ADA_RC_HD inline uint64_t chain_group_end(uint64_t K, uint64_t nb, uint64_t b)
{
	if (!K)
		return b + 1 < nb ? b + 1 : nb;
	const uint64_t e = (b / K + 1) * K;
	return e < nb ? e : nb;
}

// The checkpoints of a frame of nb blocks: its group starts past block 0.
LZ4ADA_RC_HD inline uint64_t chain_checkpoints(uint64_t K, uint64_t nb) { return K && nb ? (nb - 1) / K : 0; }

// The checkpoint of head b among its frame's.
LZ4ADA_RC_HD inline uint64_t chain_checkpoint_of(uint64_t K, uint64_t b) { return b / K - 1; }

// The block maximum of a linked frame of nb >= 2 blocks that decodes to `size`
// bytes and whose blocks but the last are full: the only one of LZ4F's four
// with (nb - 1) * max <= size <= nb * max (the next larger one is four times
// as large, and 4 * (nb - 1) > nb).  With fewer than two blocks there is no
// checkpoint and the answer is not used.
LZ4ADA_RC_HD inline uint64_t chain_block_max(uint64_t nb, uint64_t size)
{
	uint64_t m = uint64_t(64) << 10;
	while (m < (uint64_t(4) << 20) && size > nb * m)
		m *= 4;
	return m;
}

// K: blocks per group for `checkpoint_bytes` decoded bytes between checkpoints.
LZ4ADA_RC_HD inline uint64_t chain_group(uint64_t checkpoint_bytes, uint64_t block_max)
{
	const uint64_t k = (checkpoint_bytes + block_max - 1) / block_max;
	return k ? k : 1;
}

// Where the chain record of compacted block `at` of a pass of nsel lies among
// the chain_slots(nsel) records that k_decode_idx_frames_dict's workgroups read
// in order.  Workgroups are dealt round-robin over the chip's 8 XCDs, and with
// equal frames the chains' first blocks lie a fixed stride apart: records in
// block order put every chain of a stride that is a multiple of 8 on one XCD
// (measured: DESIGN.md §16).  So the records are dealt out instead: workgroup w
// gets block (w % 8) * q + w / 8, each XCD an eighth of the pass in order.
constexpr uint64_t CHAIN_DEAL = 8;
LZ4ADA_RC_HD inline uint64_t chain_slots(uint64_t nsel) { return (nsel + CHAIN_DEAL - 1) / CHAIN_DEAL * CHAIN_DEAL; }
LZ4ADA_RC_HD inline uint64_t chain_slot(uint64_t at, uint64_t nsel)
{
	const uint64_t q = (nsel + CHAIN_DEAL - 1) / CHAIN_DEAL;
	return q ? (at % q) * CHAIN_DEAL + at / q : 0;
}

// The union of the chains of one frame's ranges, taken in rising first
// touched block: add() returns what a range marks that no earlier one did.
struct ChainSweep {
	uint64_t K;
	uint64_t end;  // past the last marked block so far
	bool open;
	struct Added {
		uint64_t lo, hi;  // blocks [lo, hi), empty when hi <= lo
	};
	LZ4ADA_RC_HD explicit ChainSweep(uint64_t k) : K(k), end(0), open(false) {}
	// touched blocks [a, z]
	LZ4ADA_RC_HD Added add(uint64_t a, uint64_t z)
	{
		Added r;
		r.lo = chain_start(K, a);
		r.hi = z + 1;
		if (open && r.lo < end)
			r.lo = end;
		if (r.hi <= r.lo) {
			r.hi = r.lo;
			return r;
		}
		end = r.hi;
		open = true;
		return r;
	}
};

// The rule for one frame of nb blocks and the touched intervals [first[i],
// first[i] + count[i]) of n ranges, in any order (count 0: none), as the host
// states it (lz4ada_range_chains_host): marked[b] / head[b] (nb entries, 0 or
// 1) by the sweep in rising first block, and the chains as k_ranges_fill
// numbers them -- from a head or a marked block 0 (K == 0: from every marked
// block) over the marked blocks of its group -- as chain_first / chain_count
// (room for nb).  Returns the number of chains.  The intervals must lie inside
// [0, nb).  Allocates nothing: the next interval is searched for each time.
inline int64_t range_chains(uint64_t nb, uint64_t K, const int64_t* first, const int64_t* count, int64_t n,
                            uint8_t* marked, uint8_t* head, int64_t* chain_first, int64_t* chain_count)
{
	for (uint64_t b = 0; b < nb; ++b)
		marked[b] = head[b] = 0;
	ChainSweep sweep(K);
	int64_t last_first = -1, last_i = -1;  // the interval taken last: the order is (first, index)
	for (;;) {
		int64_t pick = -1;
		for (int64_t i = 0; i < n; ++i) {
			if (count[i] <= 0 || first[i] < last_first || (first[i] == last_first && i <= last_i))
				continue;
			if (pick < 0 || first[i] < first[pick])
				pick = i;
		}
		if (pick < 0)
			break;
		last_first = first[pick];
		last_i = pick;
		const ChainSweep::Added a = sweep.add(uint64_t(first[pick]), uint64_t(first[pick] + count[pick] - 1));
		for (uint64_t b = a.lo; b < a.hi; ++b) {
			marked[b] = 1;
			head[b] = chain_head(K, b) ? 1 : 0;
		}
	}
	int64_t nc = 0;
	for (uint64_t b = 0; b < nb; ++b) {
		if (!marked[b] || (K && !head[b] && b != 0))
			continue;
		const uint64_t e = chain_group_end(K, nb, b);
		uint64_t run = 1;
		while (b + run < e && marked[b + run])
			++run;
		chain_first[nc] = int64_t(b);
		chain_count[nc] = int64_t(run);
		++nc;
	}
	return nc;
}

}  // namespace lz4ada
