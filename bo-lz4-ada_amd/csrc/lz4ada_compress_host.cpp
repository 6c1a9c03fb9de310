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
//
// With a dictionary.  dl = min(dict_len, 65,536) and D is the
// dictionary's last dl bytes.  Positions are virtual: the block is [0, n) and
// D is [-dl, 0), immediately in front of every block of every record, so every
// block starts from the dictionary afresh.  The table holds virtual position +
// dl + 1.  Before the first window every q of [-dl, -4] -- the positions whose
// four bytes lie wholly inside D -- is inserted in ascending order (dl < 4
// seeds nothing).  A candidate c may then be negative; it is valid when
// p - c <= 65,535 and its four bytes, D's when c < 0, are equal.  The extension
// reads virtual bytes, so a match that starts in D runs on across position 0
// into the block; it still ends at n - 5.  The offset is p - c.  D and the block
// are indexed as two arrays, never as a concatenated copy.  With dl == 0 this
// is the statement above, byte for byte.
//
// Linked blocks.  Block 0 of a record is compressed as above,
// against the dictionary or nothing.  Block i >= 1 at `at` is the same
// function with D = src + at - 65,536 and dl = 65,536, the record's own bytes
// in front of it, whether or not there is a dictionary (it has slid out of
// the window).  Nothing else differs: position -65,536 is seeded and never
// valid, and the two arrays happen to be one.
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

int64_t compress_block(const uint8_t* src, int64_t n, const uint8_t* D, int64_t dl, uint8_t* dst, int64_t cap)
{
	uint32_t table[COMP_TABLE];  // virtual position + dl + 1; 0: none
	memset(table, 0, sizeof table);
	int64_t op = 0, anchor = 0;
	if (n >= COMP_MIN_BLOCK) {
		const int64_t mlast = n - COMP_MFLIMIT;       // the last position a match may start at
		const int64_t mend = n - COMP_LAST_LITERALS;  // where a match ends at the latest
		for (int64_t q = -dl; q <= -4; ++q)           // the dictionary's positions, a later one over an earlier
			table[comp_hash(walk_load32(D + (dl + q)))] = uint32_t(q + dl + 1);
		// the four bytes at a candidate (never astride position 0: -4 < c < 0 is not seeded)
		auto load_at = [&](int64_t c) { return c < 0 ? walk_load32(D + (dl + c)) : walk_load32(src + c); };
		auto byte_at = [&](int64_t x) { return x < 0 ? D[dl + x] : src[x]; };
		int64_t w = 0;
		while (w <= mlast) {
			const int64_t wn = mlast - w + 1 < COMP_WINDOW ? mlast - w + 1 : COMP_WINDOW;
			int64_t win = -1, cand = 0;
			for (int64_t p = w; p < w + wn; ++p) {
				const uint32_t v = walk_load32(src + p), e = table[comp_hash(v)];
				if (e && p - (int64_t(e - 1) - dl) <= COMP_MAX_OFF && load_at(int64_t(e - 1) - dl) == v) {
					win = p;
					cand = int64_t(e - 1) - dl;
					break;
				}
			}
			for (int64_t p = w; p <= (win < 0 ? w + wn - 1 : win); ++p)
				table[comp_hash(walk_load32(src + p))] = uint32_t(p + dl + 1);
			if (win < 0) {
				w += wn;
				continue;
			}
			int64_t ml = 4;
			while (win + ml < mend && byte_at(cand + ml) == src[win + ml])
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

// One record as one frame; dl bytes at D in front of every block, or, linked,
// in front of block 0 alone, and the record's own 65,536 bytes in front of
// every later block.
int64_t compress_frame(const uint8_t* src, int64_t n, const lz4ada_compress_options* opt, const uint8_t* D, int64_t dl,
                       uint32_t dict_id, uint32_t dflags, uint8_t* dst, int64_t cap, bool linked = false)
{
	const uint32_t id = opt ? opt->block_id : 0, flags = opt ? opt->flags : 0;
	if (n < 0 || cap < 0 || (n > 0 && !src) || (cap > 0 && !dst) || !comp_options_ok(id, flags) ||
	    (dflags & ~COMP_DICT_FLAGS_ALL) || n > (int64_t(1) << 56))
		return -int64_t(LZ4ADA_ASSERTION_ERROR);
	if (cap < comp_frame_bound(n, id, flags, dflags))
		return -int64_t(LZ4ADA_TOO_LITTLE_MEMORY);
	const int64_t blen = comp_block_len(id);
	int64_t pos = comp_header(dst, id, flags, uint64_t(n), dflags, dict_id, linked);
	for (int64_t at = 0; at < n; at += blen) {
		const int64_t len = n - at < blen ? n - at : blen;
		const bool cont = linked && at > 0;  // at >= blen >= COMP_LINK_WINDOW
		// compressed only when shorter than the block
		int64_t c = compress_block(src + at, len, cont ? src + at - COMP_LINK_WINDOW : D, cont ? COMP_LINK_WINDOW : dl,
		                           dst + pos + 4, len - 1);
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

int64_t frames_bound(const lz4ada_compress_job* jobs, int64_t njobs, const lz4ada_compress_options* opt,
                     uint32_t dflags)
{
	const uint32_t id = opt ? opt->block_id : 0, flags = opt ? opt->flags : 0;
	if (njobs < 0 || (njobs > 0 && !jobs) || !comp_options_ok(id, flags) || (dflags & ~COMP_DICT_FLAGS_ALL))
		return -1;
	int64_t bound = 0;
	for (int64_t i = 0; i < njobs; ++i) {
		if (jobs[i].in_len < 0 || jobs[i].in_len > (int64_t(1) << 56))
			return -1;
		bound += comp_frame_bound(jobs[i].in_len, id, flags, dflags);
		if (bound < 0 || bound > (int64_t(1) << 60))
			return -1;
	}
	return bound;
}

}  // namespace
}  // namespace lz4ada

using namespace lz4ada;

extern "C" {

int64_t lz4ada_compress_block_host(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap)
{
	if (n < 0 || cap < 0 || (n > 0 && !src) || (cap > 0 && !dst) || n > COMP_MAX_INPUT)
		return -1;
	return compress_block(src, n, nullptr, 0, dst, cap);
}

int64_t lz4ada_compress_block_dict_host(const uint8_t* src, int64_t n, const uint8_t* dict, int64_t dict_len,
                                        uint8_t* dst, int64_t cap)
{
	if (n < 0 || cap < 0 || (n > 0 && !src) || (cap > 0 && !dst) || n > COMP_MAX_INPUT || dict_len < 0 ||
	    (dict_len > 0 && !dict))
		return -1;
	const int64_t dl = dict_len < COMP_DICT_MAX ? dict_len : COMP_DICT_MAX;
	return compress_block(src, n, dl ? dict + (dict_len - dl) : nullptr, dl, dst, cap);
}

int64_t lz4ada_compress_frames_bound(const lz4ada_compress_job* jobs, int64_t njobs,
                                     const lz4ada_compress_options* opt)
{
	return frames_bound(jobs, njobs, opt, 0);
}

int64_t lz4ada_compress_frames_bound_dict(const lz4ada_compress_job* jobs, int64_t njobs,
                                          const lz4ada_compress_options* opt, const lz4ada_compress_dict* dict)
{
	return frames_bound(jobs, njobs, opt, dict ? dict->flags : 0);
}

int64_t lz4ada_compress_frame_host(const uint8_t* src, int64_t n, const lz4ada_compress_options* opt, uint8_t* dst,
                                   int64_t cap)
{
	return compress_frame(src, n, opt, nullptr, 0, 0, 0, dst, cap);
}

int64_t lz4ada_compress_frame_dict_host(const uint8_t* src, int64_t n, const lz4ada_compress_options* opt,
                                        const uint8_t* dict, int64_t dict_len, uint32_t dict_id, uint32_t dict_flags,
                                        uint8_t* dst, int64_t cap)
{
	if (dict_len < 0 || (dict_len > 0 && !dict))
		return -int64_t(LZ4ADA_ASSERTION_ERROR);
	const int64_t dl = dict_len < COMP_DICT_MAX ? dict_len : COMP_DICT_MAX;
	return compress_frame(src, n, opt, dl ? dict + (dict_len - dl) : nullptr, dl, dict_id, dict_flags, dst, cap);
}

int64_t lz4ada_compress_frame_linked_host(const uint8_t* src, int64_t n, const lz4ada_compress_options* opt,
                                          const uint8_t* dict, int64_t dict_len, uint32_t dict_id, uint32_t dict_flags,
                                          uint8_t* dst, int64_t cap)
{
	if (dict_len < 0 || (dict_len > 0 && !dict))
		return -int64_t(LZ4ADA_ASSERTION_ERROR);
	const int64_t dl = dict_len < COMP_DICT_MAX ? dict_len : COMP_DICT_MAX;
	return compress_frame(src, n, opt, dl ? dict + (dict_len - dl) : nullptr, dl, dict_id, dict_flags, dst, cap, true);
}

}  // extern "C"
