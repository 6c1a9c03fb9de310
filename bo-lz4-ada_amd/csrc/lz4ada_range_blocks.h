// lz4ada_range_blocks.h -- which blocks of a frame a range of its decoded
// bytes touches, as host/device code.  A frame of nb blocks
// is given by start[0 .. nb]: start[b] is the decoded offset at which block b
// begins (the exclusive prefix sum of the block sizes) and start[nb] the
// frame's decoded size.  It is the one statement of the rule: k_ranges_select
// and k_ranges_gather (lz4ada_ranges.hip) call it, the host states it through
// lz4ada_range_blocks_host, and tests/test_range_blocks_cpu.py pins it to a
// brute-force definition.
//
// A block is touched when it shares at least one byte with the clipped range,
// so a block of size 0 (a stored block without payload, a compressed block
// that decodes to nothing) is never the first or the last block of a range;
// between two touched blocks it rides along.
//
// Depends on nothing, so a plain C++ program can include it
// (tools/range_blocks_asan.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4ADA_RB_HD __host__ __device__
#else
#define LZ4ADA_RB_HD
#endif

namespace lz4ada {

// The largest i in [0, n) with a[i] <= x, for a rising a[0 .. n] with
// a[0] <= x < a[n]: the block that holds byte x when a is a frame's start[],
// the frame that holds block x when a is the index's first[].  Equal
// neighbours (empty blocks, frames without blocks) are passed over: a[i + 1] > x
// for the i returned.  Reads a[1 .. n - 1] only.
LZ4ADA_RB_HD inline uint64_t rising_find(const uint64_t* a, uint64_t n, uint64_t x)
{
	uint64_t lo = 0, hi = n;  // a[lo] <= x < a[hi]
	while (hi - lo > 1) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (a[mid] <= x)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// What is left of [off, off + len) inside a frame of `size` decoded bytes.
LZ4ADA_RB_HD inline uint64_t range_clip(uint64_t size, uint64_t off, uint64_t len)
{
	return off < size ? (len < size - off ? len : size - off) : 0;
}

struct RangeBlocks {
	uint64_t first, count;  // blocks [first, first + count); count 0: the clipped range is empty
};

// The blocks that [off, off + len), clipped to the frame, touches.  Reads
// start[0 .. nb] only; nb may be 0 (start[0] is then the size, 0).
LZ4ADA_RB_HD inline RangeBlocks range_blocks(const uint64_t* start, uint64_t nb, uint64_t off, uint64_t len)
{
	RangeBlocks r;
	r.first = r.count = 0;
	const uint64_t want = range_clip(start[nb], off, len);
	if (want == 0)
		return r;
	// 0 = start[0] <= off <= off + want - 1 < start[nb]
	r.first = rising_find(start, nb, off);
	r.count = rising_find(start, nb, off + want - 1) - r.first + 1;
	return r;
}

}  // namespace lz4ada
