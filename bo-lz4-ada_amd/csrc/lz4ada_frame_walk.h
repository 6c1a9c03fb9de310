// lz4ada_frame_walk.h -- one frame's header checks and size-word walk as
// host/device code: what index_frame (lz4ada_bulk.cpp, from
// lib/lz4ada.adb:155-375, 525-585) and classify (lz4ada_bulk_frames.cpp)
// decide about a frame, stated a second time without strings or exceptions
// so that a GPU lane can run it over a frame that lies in device memory
// (lz4ada_frames_index.hip) and the host over one in host memory
// (lz4ada_frame_walk_host).  index_frame and classify own the reference's
// error texts; tests/test_frame_walk_cpu.py pins this statement to them.
//
// Depends on lz4ada_hip.h alone, so a plain C++ program can include it
// (tools/frame_walk_asan.cpp).
#pragma once

#include <stdint.h>
#include <string.h>

#include "lz4ada_hip.h"

#if defined(__HIPCC__)
#define LZ4ADA_HD __host__ __device__
#else
#define LZ4ADA_HD
#endif

namespace lz4ada {

// The lone-block rule's numbers, for few_large_blocks (lz4ada_host_common.cpp)
// and the walk below: a frame of at most WALK_LONE_BLOCKS blocks whose largest
// payload is in [WALK_LONE_MIN_IN, WALK_LONE_MAX_IN] decodes faster one block
// at a time.
constexpr int64_t WALK_LONE_BLOCKS = 24;
constexpr uint32_t WALK_LONE_MIN_IN = 512u << 10;
constexpr int64_t WALK_LONE_MAX_IN = int64_t(16) << 20;  // LONE_MAX_IN (lz4ada_internal.h)
// The bulk decoders take blocks whose slot is at most this (MAX_RUN,
// lz4ada_idx.hip); a legacy frame may declare more.  For classify
// (lz4ada_bulk_frames.cpp) and the walk below.
constexpr uint32_t WALK_SLOT_MAX = 4u << 20;

// What the walk adds up over a frame's blocks.
struct WalkSums {
	uint64_t slots;   // sum of round256(slot_cap): its slots as a pass lays them out
	uint64_t caps;    // sum of slot_cap: what it can decode to
	uint32_t max_in;  // largest payload
	uint32_t pad;
};

// Where the walk writes descriptors (descs null: nowhere).  At most `cap` are
// written, whatever the frame holds.  slots false: as lz4ada_frame_index lays
// them out (in_off frame-relative, out_off = block * block_max, out_cap =
// block_max).  slots true: as a pass needs them (in_off + in_base, out_off
// from out_base in steps of round256(slot_cap) and never past out_limit,
// out_cap = slot_cap).  `written` counts them.
struct WalkEmit {
	lz4ada_block_desc* descs;
	int64_t cap;
	bool slots;
	uint64_t in_base, out_base, out_limit;
	int64_t written;
};

LZ4ADA_HD inline uint32_t walk_load32(const uint8_t* p)
{
	return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

LZ4ADA_HD inline uint32_t walk_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// XXH32, seed 0, of the n < 16 bytes of a frame descriptor (lz4ada.adb:351-361).
LZ4ADA_HD inline uint32_t walk_descriptor_xxh32(const uint8_t* p, int64_t n)
{
	uint32_t h = uint32_t(n) + 374761393u;
	int64_t d = 0;
	for (; d + 4 <= n; d += 4)
		h = walk_rotl(h + walk_load32(p + d) * 3266489917u, 17) * 668265263u;
	for (; d < n; ++d)
		h = walk_rotl(h + uint32_t(p[d]) * 374761393u, 11) * 2654435761u;
	h = (h ^ (h >> 15)) * 2246822519u;
	h = (h ^ (h >> 13)) * 3266489917u;
	return h ^ (h >> 16);
}

// XXH32, seed 0, of n bytes, serially: the block and content checksums of the
// host statements (lz4ada_dict_host.cpp, lz4ada_compress_host.cpp).
inline uint32_t walk_xxh32(const uint8_t* p, int64_t n)
{
	constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
	const uint8_t* const end = p + n;
	uint32_t h;
	if (n >= 16) {
		uint32_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0u - P1;
		for (; end - p >= 16; p += 16) {
			v1 = walk_rotl(v1 + walk_load32(p) * P2, 13) * P1;
			v2 = walk_rotl(v2 + walk_load32(p + 4) * P2, 13) * P1;
			v3 = walk_rotl(v3 + walk_load32(p + 8) * P2, 13) * P1;
			v4 = walk_rotl(v4 + walk_load32(p + 12) * P2, 13) * P1;
		}
		h = walk_rotl(v1, 1) + walk_rotl(v2, 7) + walk_rotl(v3, 12) + walk_rotl(v4, 18);
	} else {
		h = P5;
	}
	h += uint32_t(n);
	for (; end - p >= 4; p += 4)
		h = walk_rotl(h + walk_load32(p) * P3, 17) * P4;
	for (; p < end; ++p)
		h = walk_rotl(h + uint32_t(*p) * P5, 11) * P1;
	h = (h ^ (h >> 15)) * P2;
	h = (h ^ (h >> 13)) * P3;
	return h ^ (h >> 16);
}

LZ4ADA_HD inline bool walk_is_any_magic(uint32_t v)
{
	return v == 0x184d2204u || v == 0x184c2102u || (v >= 0x184d2a50u && v <= 0x184d2a5fu);
}

// slot_cap (lz4ada_linked_accept.h)
LZ4ADA_HD inline uint32_t walk_slot_cap(uint32_t in_len, bool stored, int64_t bmax)
{
	if (stored)
		return in_len;
	const uint64_t grown = 255ull * in_len + 64;
	return uint32_t(grown < uint64_t(bmax) ? grown : uint64_t(bmax));
}

// The lone-block rule over a frame of nb blocks whose largest payload is max_in
// (the numbers above), as the walk below ends with it; stated here for the
// compressor's own index (lz4ada_compress_index.h), which knows its blocks
// without walking them.  tests/test_compress_index_cpu.py pins the two to
// each other.
LZ4ADA_HD inline bool walk_lone(bool no_lone, int64_t nb, uint32_t max_in)
{
	return !no_lone && nb >= 1 && nb <= WALK_LONE_BLOCKS && max_in >= WALK_LONE_MIN_IN &&
	       int64_t(max_in) <= WALK_LONE_MAX_IN;
}

// The frame at [p, p + len) under Single_Frame semantics (the frame and
// whatever follows it).  Returns LZ4ADA_BATCH_OK for exactly the frames that
// pass index_frame and leave classify as LZ4ADA_BATCH_OK (skippable ones
// included), else LZ4ADA_BATCH_LINKED, _BIG_BLOCK or _NOT_INDEXED as classify
// would say (_OVER_BUDGET is the caller's: compare sums->slots).  *info is
// filled as index_frame fills it whenever the result is not _NOT_INDEXED.
// no_lone: LZ4ADA_NO_LONE is set (few_large_blocks then never applies).
// take_linked (LZ4ADA_FRAMES_LINKED): a modern frame with
// B.Indep clear is judged by the other rules too and is LZ4ADA_BATCH_OK when
// it passes them and its slots sum to at most linked_max bytes (one wave walks
// the whole frame), else LZ4ADA_BATCH_LINKED; info->independent stays 0, which
// tells the engine the decoder the frame takes.  Off: today's verdicts.
// Reads no byte outside [p, p + len); ends with the input, since every block
// takes at least 4 bytes of it.
LZ4ADA_HD inline int frame_walk(const uint8_t* p, int64_t len, bool no_lone, lz4ada_frame_info* info,
                                WalkSums* sums, WalkEmit* emit, bool take_linked = false,
                                uint64_t linked_max = 0)
{
	memset(info, 0, sizeof *info);
	sums->slots = sums->caps = 0;
	sums->max_in = sums->pad = 0;
	if (emit)
		emit->written = 0;
	if (len < 7)
		return LZ4ADA_BATCH_NOT_INDEXED;
	const uint32_t magic = walk_load32(p);
	int64_t pos, bmax;
	int cklen = 0;  // block checksum bytes
	bool legacy = false;
	if (magic == 0x184d2204u) {
		const uint8_t flg = p[4], bd = p[5];
		if (((flg & 0xc0u) >> 6) != 1)
			return LZ4ADA_BATCH_NOT_INDEXED;  // version
		if ((flg & 2u) || (bd & 0x8fu))
			return LZ4ADA_BATCH_NOT_INDEXED;  // reserved bits
		const unsigned code = (bd & 0x70u) >> 4;
		if (code < 4)
			return LZ4ADA_BATCH_NOT_INDEXED;  // BD table: 4..7
		bmax = int64_t(65536) << (2 * (code - 4));
		// the descriptor: FLG, BD, the content size, the dictionary id (skipped: quirk Q7)
		const int64_t dlen = 2 + ((flg & 8u) ? 8 : 0) + ((flg & 1u) ? 4 : 0);
		pos = 4 + dlen + 1;
		if (pos > len)
			return LZ4ADA_BATCH_NOT_INDEXED;
		if (p[4 + dlen] != uint8_t((walk_descriptor_xxh32(p + 4, dlen) >> 8) & 0xffu))
			return LZ4ADA_BATCH_NOT_INDEXED;
		info->format = LZ4ADA_FORMAT_MODERN;
		info->flg = flg;
		info->bd = bd;
		info->block_checksum = (flg & 16u) ? 1 : 0;
		info->content_checksum = (flg & 4u) ? 1 : 0;
		info->has_content_size = (flg & 8u) ? 1 : 0;
		info->independent = (flg & 0x20u) ? 1 : 0;
		if (flg & 8u)
			info->content_size = uint64_t(walk_load32(p + 6)) | (uint64_t(walk_load32(p + 10)) << 32);
		cklen = (flg & 16u) ? 4 : 0;
	} else if (magic == 0x184c2102u) {
		legacy = true;
		pos = 4;
		bmax = int64_t(8) << 20;
		info->format = LZ4ADA_FORMAT_LEGACY;
		info->independent = 1;
	} else if (magic >= 0x184d2a50u && magic <= 0x184d2a5fu) {
		if (len < 8)
			return LZ4ADA_BATCH_NOT_INDEXED;
		info->format = LZ4ADA_FORMAT_SKIPPABLE;
		info->block_max = 65536;  // quirk Q3
		info->header_len = 8;
		info->frame_len = 8 + int64_t(walk_load32(p + 4));
		return info->frame_len > len ? LZ4ADA_BATCH_NOT_INDEXED : LZ4ADA_BATCH_OK;
	} else {
		return LZ4ADA_BATCH_NOT_INDEXED;
	}
	info->header_len = pos;
	info->block_max = bmax;

	int64_t nb = 0;
	uint64_t slot_at = emit ? emit->out_base : 0;
	bool big = false;
	for (;;) {
		if (pos + 4 > len) {
			if (legacy && pos == len)
				break;  // a legacy frame ends with the input
			return LZ4ADA_BATCH_NOT_INDEXED;
		}
		uint32_t word = walk_load32(p + pos);
		if (!legacy && word == 0) {  // the end mark
			pos += 4;
			if (info->content_checksum) {
				if (pos + 4 > len)
					return LZ4ADA_BATCH_NOT_INDEXED;
				info->content_checksum_declared = walk_load32(p + pos);
				pos += 4;
			}
			break;
		}
		if (legacy && walk_is_any_magic(word))
			break;  // the next frame starts here
		bool stored = false;
		if (!legacy) {
			stored = (word & 0x80000000u) != 0;
			word &= 0x7ffffffu;  // quirk Q2
		}
		if (int64_t(word) > bmax)  // word + additional > inbuf
			return LZ4ADA_BATCH_NOT_INDEXED;
		const int64_t payload = pos + 4;
		const int64_t end = payload + int64_t(word) + cklen;
		if (end > len)
			return LZ4ADA_BATCH_NOT_INDEXED;
		const uint32_t cap = walk_slot_cap(word, stored, bmax);
		big = big || cap > WALK_SLOT_MAX;
		const uint64_t slot = (uint64_t(cap) + 255) & ~uint64_t(255);
		if (emit && emit->descs && emit->written < emit->cap &&
		    (!emit->slots || slot_at + slot <= emit->out_limit)) {
			lz4ada_block_desc d;
			d.in_off = uint64_t(payload) + (emit->slots ? emit->in_base : 0);
			d.in_len = word;
			d.flags = (stored ? LZ4ADA_BLOCK_STORED : 0u) | (cklen ? LZ4ADA_BLOCK_HAS_CKSUM : 0u);
			d.out_off = emit->slots ? slot_at : uint64_t(nb) * uint64_t(bmax);
			d.out_cap = emit->slots ? cap : uint32_t(bmax);
			d.cksum = cklen ? walk_load32(p + payload + word) : 0u;
			emit->descs[emit->written++] = d;
			slot_at += slot;
		}
		sums->slots += slot;
		sums->caps += cap;
		sums->max_in = word > sums->max_in ? word : sums->max_in;
		++nb;
		pos = end;
	}
	info->nblocks = nb;
	info->frame_len = pos;
	if (!info->independent && !take_linked)
		return LZ4ADA_BATCH_LINKED;
	const bool lone = !no_lone && nb >= 1 && nb <= WALK_LONE_BLOCKS && sums->max_in >= WALK_LONE_MIN_IN &&
	                  int64_t(sums->max_in) <= WALK_LONE_MAX_IN;
	if (big || lone)
		return LZ4ADA_BATCH_BIG_BLOCK;
	return !info->independent && sums->slots > linked_max ? LZ4ADA_BATCH_LINKED : LZ4ADA_BATCH_OK;
}

}  // namespace lz4ada
