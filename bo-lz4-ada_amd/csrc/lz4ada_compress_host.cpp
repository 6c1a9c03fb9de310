// lz4ada_compress_host.cpp -- the compressor stated serially:
// the matching rule of one block, and one record as one frame.  What
// k_compress_blocks and the emit kernels (lz4ada_compress.hip) write is tested
// against these bytes, so the rule below is the rule; the kernel is its
// 64-lane reading.  The compressor is this library's own (the reference has
// none).  Plain serial C++, no HIP call; depends on lz4ada_hip.h,
// lz4ada_frame_walk.h and lz4ada_compress.h alone, so a plain C++ program can
// compile it (tools/compress_host_asan.cpp).
//
// The rule.  The block is walked in windows of 64 consecutive positions, the
// first at 0.  Every position of a window hashes its four bytes and reads the
// table's entry for that hash -- the latest position inserted under it --
// before any position of the window is inserted, so a candidate always lies
// before the window.  A candidate is valid when it is at most 65,535 back and
// its four bytes are equal.  The lowest position with a valid candidate wins;
// the positions of the window up to and including it are inserted (all of
// them when none won, and the next window follows this one), the match is
// extended as far as n - 5 allows, one sequence is emitted, and the next
// window starts at the match's end.  Positions inside a match are never
// inserted.  No window reaches past n - 12, the last place a match may start.
#include <stdint.h>
#include <string.h>

#include "lz4ada_compress.h"

namespace lz4ada {
namespace {

void store32(uint8_t* p, uint32_t v)
{
	p[0] = uint8_t(v), p[1] = uint8_t(v >> 8), p[2] = uint8_t(v >> 16), p[3] = uint8_t(v >> 24);
}

// A token's nibble for length v, and the 255* + rest that follows from 15 on.
uint8_t nibble(int64_t v) { return uint8_t(v < 15 ? v : 15); }
int64_t put_ext(uint8_t* dst, int64_t op, int64_t v)
{
	if (v < 15)
		return op;
	for (v -= 15; v >= 255; v -= 255)
		dst[op++] = 255;
	dst[op++] = uint8_t(v);
	return op;
}

int64_t compress_block(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap)
{
	uint32_t table[COMP_TABLE];  // position + 1; 0: none
	memset(table, 0, sizeof table);
	int64_t op = 0, anchor = 0;
	if (n >= COMP_MIN_BLOCK) {
		const int64_t mlast = n - COMP_MFLIMIT;       // the last position a match may start at
		const int64_t mend = n - COMP_LAST_LITERALS;  // where a match ends at the latest
		int64_t w = 0;
		while (w <= mlast) {
			const int64_t wn = mlast - w + 1 < COMP_WINDOW ? mlast - w + 1 : COMP_WINDOW;
			int64_t win = -1, cand = 0;
			for (int64_t p = w; p < w + wn; ++p) {
				const uint32_t v = walk_load32(src + p), e = table[comp_hash(v)];
				if (e && p - int64_t(e - 1) <= COMP_MAX_OFF && walk_load32(src + (e - 1)) == v) {
					win = p;
					cand = int64_t(e - 1);
					break;
				}
			}
			for (int64_t p = w; p <= (win < 0 ? w + wn - 1 : win); ++p)
				table[comp_hash(walk_load32(src + p))] = uint32_t(p + 1);
			if (win < 0) {
				w += wn;
				continue;
			}
			int64_t ml = 4;
			while (win + ml < mend && src[cand + ml] == src[win + ml])
				++ml;
			const int64_t lit = win - anchor;
			if (op + comp_seq_len(lit, ml) > cap)
				return 0;
			dst[op++] = uint8_t((nibble(lit) << 4) | nibble(ml - 4));
			op = put_ext(dst, op, lit);
			memcpy(dst + op, src + anchor, size_t(lit));
			op += lit;
			dst[op++] = uint8_t(win - cand);
			dst[op++] = uint8_t((win - cand) >> 8);
			op = put_ext(dst, op, ml - 4);
			w = anchor = win + ml;
		}
	}
	const int64_t lit = n - anchor;
	if (op + comp_last_len(lit) > cap)
		return 0;
	dst[op++] = uint8_t(nibble(lit) << 4);
	op = put_ext(dst, op, lit);
	if (lit)
		memcpy(dst + op, src + anchor, size_t(lit));
	return op + lit;
}

}  // namespace
}  // namespace lz4ada

using namespace lz4ada;

extern "C" {

int64_t lz4ada_compress_block_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap)
{
	if (n < 0 || cap < 0 || (n > 0 && !src) || (cap > 0 && !dst) || n > COMP_MAX_INPUT)
		return -1;
	return compress_block(src, n, dst, cap);
}

int64_t lz4ada_compress_frames_bound(const lz4ada_compress_job* jobs, int64_t njobs,
                                     const lz4ada_compress_options* opt)
{
	const uint32_t id = opt ? opt->block_id : 0, flags = opt ? opt->flags : 0;
	if (njobs < 0 || (njobs > 0 && !jobs) || !comp_options_ok(id, flags))
		return -1;
	int64_t bound = 0;
	for (int64_t i = 0; i < njobs; ++i) {
		if (jobs[i].in_len < 0 || jobs[i].in_len > (int64_t(1) << 56))
			return -1;
		bound += comp_frame_bound(jobs[i].in_len, id, flags);
		if (bound < 0 || bound > (int64_t(1) << 60))
			return -1;
	}
	return bound;
}

int64_t lz4ada_compress_frame_host(const uint8_t* src, int64_t n, const lz4ada_compress_options* opt, uint8_t* dst,
                                   int64_t cap)
{
	const uint32_t id = opt ? opt->block_id : 0, flags = opt ? opt->flags : 0;
	if (n < 0 || cap < 0 || (n > 0 && !src) || (cap > 0 && !dst) || !comp_options_ok(id, flags) ||
	    n > (int64_t(1) << 56))
		return -int64_t(LZ4ADA_ASSERTION_ERROR);
	if (cap < comp_frame_bound(n, id, flags))
		return -int64_t(LZ4ADA_TOO_LITTLE_MEMORY);
	const int64_t blen = comp_block_len(id);
	int64_t pos = comp_header(dst, id, flags, uint64_t(n));
	for (int64_t at = 0; at < n; at += blen) {
		const int64_t len = n - at < blen ? n - at : blen;
		// compressed only when shorter than the block
		int64_t c = compress_block(src + at, len, dst + pos + 4, len - 1);
		const bool stored = c == 0;
		if (stored) {
			memcpy(dst + pos + 4, src + at, size_t(len));
			c = len;
		}
		store32(dst + pos, uint32_t(c) | (stored ? 0x80000000u : 0u));
		pos += 4 + c;
		if (flags & LZ4ADA_COMP_BLOCK_CHECKSUM) {
			store32(dst + pos, walk_xxh32(dst + pos - c, c));
			pos += 4;
		}
	}
	store32(dst + pos, 0);
	pos += 4;
	if (flags & LZ4ADA_COMP_CONTENT_CHECKSUM) {
		store32(dst + pos, walk_xxh32(src, n));
		pos += 4;
	}
	return pos;
}

}  // extern "C"
