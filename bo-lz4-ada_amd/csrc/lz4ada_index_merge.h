// lz4ada_index_merge.h -- the rule by which lz4ada_seek_index_concat lays the
// seek indexes of several compress calls (or builds) into one, as host/device
// code.  Every piece an index holds is either relative to its
// frame (start, slotp, kgrp, fkind) or an offset that one constant per part
// rebases (desc.in_off, desc.out_off, first, ckfirst), so the merge is five
// exclusive prefix sums over the parts and, per merged element, the part it
// belongs to.  It is the one statement of both: the host validates and sums
// with it (lz4ada_bulk_ranges.cpp), the k_index_merge_* kernels
// (lz4ada_index_merge.hip) look every element's part up with merge_part_of, the
// host states all of it through lz4ada_index_merge_plan_host, which
// tests/test_index_merge_cpu.py pins to numpy.cumsum and a linear scan, and
// tools/index_merge_asan.cpp runs it over exact-size heap blocks.
//
// Prefixes repeat in ordinary use: a part without frames repeats all five, a
// part whose records are all 0 bytes long holds frames but no block and repeats
// the block and checkpoint prefixes.  merge_part_of is rising_find
// (lz4ada_range_blocks.h), which passes equal neighbours over, so an element is
// never given to a part that holds none.
//
// The rule depends on lz4ada_range_blocks.h and the standard library alone, so
// a plain C++ program can include it; the part table and the launches below it
// are declared for hipcc only.
#pragma once

#include <stdint.h>

#include "lz4ada_range_blocks.h"

namespace lz4ada {

// What the rule needs to know of one part.
struct MergePart {
	int64_t n;       // its jobs (= frames)
	int64_t nb;      // the blocks of the frames it took
	int64_t nck;     // its checkpoints
	int64_t in_len;  // the input it was made over
	int64_t slots;   // its nominal slots: where the out_off of a next frame's first block would lie
};

// The five exclusive prefixes, nparts + 1 entries each; entry nparts is the total.
enum MergePrefix { MERGE_FRAMES, MERGE_BLOCKS, MERGE_WORDS, MERGE_CKPTS, MERGE_SLOTS, MERGE_PREFIXES };

// What merge_validate says: 0, or which rule of lz4ada_seek_index_concat the
// arguments break (all of them misuse).
enum MergeFault {
	MERGE_OK,
	MERGE_NEGATIVE_COUNT,  // nparts < 0 or in_len < 0
	MERGE_NULL_ARRAY,      // nparts > 0 without parts or bases
	MERGE_NEGATIVE_BASE,
	MERGE_BAD_PART,  // a part with a negative count or length (an index never has one)
	MERGE_NOT_RISING,  // in_base[p] < in_base[p - 1] + in_len of part p - 1
	MERGE_PAST_END,    // a part ends past in_len
};

// The parts lie in rising order of place and apart (touching is fine, and so
// are gaps), inside [0, in_len).  *at: the part that breaks the rule.
LZ4ADA_RB_HD inline MergeFault merge_validate(const MergePart* part, const int64_t* in_base, int64_t nparts,
                                              int64_t in_len, int64_t* at)
{
	*at = 0;
	if (nparts < 0 || in_len < 0)
		return MERGE_NEGATIVE_COUNT;
	if (nparts > 0 && (!part || !in_base))
		return MERGE_NULL_ARRAY;
	int64_t end = 0;  // of the part before
	for (int64_t p = 0; p < nparts; ++p) {
		*at = p;
		if (in_base[p] < 0)
			return MERGE_NEGATIVE_BASE;
		const MergePart& m = part[p];
		if (m.n < 0 || m.nb < 0 || m.nck < 0 || m.in_len < 0 || m.slots < 0)
			return MERGE_BAD_PART;
		if (in_base[p] < end)
			return MERGE_NOT_RISING;
		if (m.in_len > in_len || in_base[p] > in_len - m.in_len)
			return MERGE_PAST_END;
		end = in_base[p] + m.in_len;  // (at most in_len: no overflow)
	}
	return MERGE_OK;
}

// The prefixes of validated parts into pre[MERGE_PREFIXES][nparts + 1], laid
// out prefix by prefix.  False when the jobs or the blocks reach 2^31, the
// limit of every index (sums up to there cannot overflow: checked as they grow).
LZ4ADA_RB_HD inline bool merge_plan(const MergePart* part, int64_t nparts, uint64_t* pre)
{
	const uint64_t stride = uint64_t(nparts) + 1, limit = uint64_t(1) << 31;
	uint64_t acc[MERGE_PREFIXES] = { 0, 0, 0, 0, 0 };
	for (int64_t p = 0; p <= nparts; ++p) {
		for (int k = 0; k < MERGE_PREFIXES; ++k)
			pre[uint64_t(k) * stride + uint64_t(p)] = acc[k];
		if (p == nparts)
			break;
		const MergePart& m = part[p];
		if (uint64_t(m.n) >= limit - acc[MERGE_FRAMES] || uint64_t(m.nb) >= limit - acc[MERGE_BLOCKS])
			return false;
		acc[MERGE_FRAMES] += uint64_t(m.n);
		acc[MERGE_BLOCKS] += uint64_t(m.nb);
		acc[MERGE_WORDS] += uint64_t(m.nb) + uint64_t(m.n);
		acc[MERGE_CKPTS] += uint64_t(m.nck);
		acc[MERGE_SLOTS] += uint64_t(m.slots);
	}
	return true;
}

// The part that merged element i of one kind belongs to, by that kind's prefix
// (nparts + 1 entries, 0 <= i < prefix[nparts]): the last p with prefix[p] <= i,
// so prefix[p + 1] > i and the part holds the element however many parts
// before or after it hold none.
LZ4ADA_RB_HD inline uint64_t merge_part_of(const uint64_t* prefix, uint64_t nparts, uint64_t i)
{
	return rising_find(prefix, nparts, i);
}

}  // namespace lz4ada

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "lz4ada_hip.h"

namespace lz4ada {

// One part as the kernels read it: its device arrays (SeekView's; all null in a
// part without frames, kgrp / ckfirst / store null without checkpoint arrays,
// fkind / dict null without a dictionary) and where its input lies in the result's.
struct MergePartDev {
	const lz4ada_block_desc* desc;
	const uint64_t *first, *start, *slotp;
	const uint64_t *kgrp, *ckfirst, *fkind;
	const uint8_t *store, *dict;
	uint64_t in_base;
};
// The part table, one device block that one copy fills: nparts MergePartDev,
// then the five prefixes of merge_plan.
struct MergeTable {
	const MergePartDev* part;
	const uint64_t* pre;  // pre + k * (nparts + 1): prefix k
	uint32_t nparts;
};
// The result's arrays and the counts they were allocated by (alloc_index,
// alloc_checkpoints): nblocks descriptors, nblocks + nframes words of start and
// of slotp, nframes + 1 of first; with kgrp not null nframes of it, nframes + 1
// of ckfirst and nckpt checkpoints in store; with fkind not null nframes of it.
struct MergeOut {
	lz4ada_block_desc* desc;
	uint64_t *first, *start, *slotp;
	uint64_t *kgrp, *ckfirst, *fkind;
	uint8_t* store;
	uint64_t nblocks, nckpt;
	uint32_t nframes;
};
// The four launches that fill a result of nframes > 0 (k_index_merge_blocks,
// _words, _frames, _store; those over no element are left out), whatever nparts
// is.  No kernel writes at or past the counts in `o`, whatever the table says.
hipError_t launch_index_merge(const MergeTable& t, const MergeOut& o, hipStream_t stream);
// k_index_merge_dict_eq: *d_flag (zeroed by the caller) becomes 1 when the gap
// image (gap bytes, a multiple of 16) of any part that has one differs from
// part `ref`'s.
hipError_t launch_index_merge_dict_eq(const MergeTable& t, uint32_t ref, uint64_t gap, uint32_t* d_flag,
                                      hipStream_t stream);

}  // namespace lz4ada
#endif
