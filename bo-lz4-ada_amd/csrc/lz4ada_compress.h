// lz4ada_compress.h -- what the three statements of the compressor share
// (DESIGN.md §17): the frame arithmetic and the header bytes, as host/device
// code, and the matching rule's constants.  lz4ada_compress_host.cpp states
// the rule serially, in one compress_block that a dictionary or a linked
// record calls with another history; lz4ada_compress_block.inc is its 64-lane
// reading, one device body with one wave per block, compiled once per history
// as k_compress_blocks, k_compress_blocks_dict and k_compress_blocks_linked;
// lz4ada_bulk_compress.cpp lays the jobs out.
//
// Depends on lz4ada_hip.h and lz4ada_frame_walk.h alone, so a plain C++ program
// can include it (tools/compress_host_asan.cpp).
#pragma once

#include <stdint.h>

#include "lz4ada_frame_walk.h"
#include "lz4ada_hip.h"

namespace lz4ada {

// ---- the matching rule (stated in lz4ada_compress_host.cpp) ----
// A window of COMP_WINDOW consecutive positions looks up a table of
// 2^COMP_HASH_BITS entries (position + 1 of the latest inserted position with
// that hash, 0: none) before any of them is inserted.
constexpr int COMP_HASH_BITS = 12;
constexpr uint32_t COMP_TABLE = 1u << COMP_HASH_BITS;
constexpr int64_t COMP_WINDOW = 64;
constexpr int64_t COMP_MAX_OFF = 65535;
// The LZ4 end-of-block rules: a block under COMP_MIN_BLOCK bytes is one literal
// run, a match starts at or before n - COMP_MFLIMIT and ends at or before
// n - COMP_LAST_LITERALS.
constexpr int64_t COMP_MIN_BLOCK = 13, COMP_MFLIMIT = 12, COMP_LAST_LITERALS = 5;
constexpr int64_t COMP_MAX_INPUT = 0x7E000000;  // LZ4_MAX_INPUT_SIZE
// With a dictionary positions are virtual: its last
// min(dict_len, COMP_DICT_MAX) bytes D lie at [-dl, 0) in front of every block,
// and the table holds virtual position + dl + 1.
constexpr int64_t COMP_DICT_MAX = 65536;
// In a linked frame block i >= 1 of a record has the
// COMP_LINK_WINDOW record bytes in front of it in the dictionary's place.
constexpr int64_t COMP_LINK_WINDOW = 65536;

LZ4ADA_HD inline uint32_t comp_hash(uint32_t four_bytes)
{
	return (four_bytes * 2654435761u) >> (32 - COMP_HASH_BITS);
}

// Bytes of a length's extension: none below 15, else 255* and a rest.
LZ4ADA_HD inline int64_t comp_ext_len(int64_t v) { return v < 15 ? 0 : (v - 15) / 255 + 1; }
// One sequence: token, literal extension, literals, offset, match extension (ml >= 4).
LZ4ADA_HD inline int64_t comp_seq_len(int64_t lit, int64_t ml)
{
	return 1 + comp_ext_len(lit) + lit + 2 + comp_ext_len(ml - 4);
}
// The last sequence: token, literal extension, literals.
LZ4ADA_HD inline int64_t comp_last_len(int64_t lit) { return 1 + comp_ext_len(lit) + lit; }

// ---- the frame ----
constexpr uint32_t COMP_FLAGS_ALL =
        LZ4ADA_COMP_BLOCK_CHECKSUM | LZ4ADA_COMP_CONTENT_CHECKSUM | LZ4ADA_COMP_CONTENT_SIZE;

LZ4ADA_HD inline bool comp_options_ok(uint32_t block_id, uint32_t flags)
{
	return (block_id == 0 || (block_id >= 4 && block_id <= 7)) && !(flags & ~COMP_FLAGS_ALL);
}
LZ4ADA_HD inline uint32_t comp_block_id(uint32_t block_id) { return block_id ? block_id : 4; }
LZ4ADA_HD inline int64_t comp_block_len(uint32_t block_id)
{
	return int64_t(65536) << (2 * (comp_block_id(block_id) - 4));
}
LZ4ADA_HD inline int64_t comp_nblocks(int64_t n, int64_t block_len) { return (n + block_len - 1) / block_len; }
// dflags: a dictionary call's LZ4ADA_COMP_DICT_* (DESIGN.md §18), 0 without one.
constexpr uint32_t COMP_DICT_FLAGS_ALL = LZ4ADA_COMP_DICT_WRITE_ID;
LZ4ADA_HD inline int64_t comp_header_len(uint32_t flags, uint32_t dflags = 0)
{
	return 7 + ((flags & LZ4ADA_COMP_CONTENT_SIZE) ? 8 : 0) + ((dflags & LZ4ADA_COMP_DICT_WRITE_ID) ? 4 : 0);
}
LZ4ADA_HD inline int64_t comp_trailer_len(uint32_t flags)
{
	return 4 + ((flags & LZ4ADA_COMP_CONTENT_CHECKSUM) ? 4 : 0);
}
// A block's bytes besides its payload: the size word and the checksum.
LZ4ADA_HD inline int64_t comp_block_extra(uint32_t flags) { return 4 + ((flags & LZ4ADA_COMP_BLOCK_CHECKSUM) ? 4 : 0); }
// The bound of include/lz4ada_hip.h: every block stored.
LZ4ADA_HD inline int64_t comp_frame_bound(int64_t n, uint32_t block_id, uint32_t flags, uint32_t dflags = 0)
{
	return comp_header_len(flags, dflags) + comp_nblocks(n, comp_block_len(block_id)) * comp_block_extra(flags) + n +
	       comp_trailer_len(flags);
}
// Magic, FLG, BD, the content size when asked for, the dictionary id under
// LZ4ADA_COMP_DICT_WRITE_ID, HC (over all of them) into h[0 .. 19) -> comp_header_len.
// linked: a frame of linked blocks, FLG 0x20 (B.Indep) clear.
LZ4ADA_HD inline int comp_header(uint8_t* h, uint32_t block_id, uint32_t flags, uint64_t content_size,
                                 uint32_t dflags = 0, uint32_t dict_id = 0, bool linked = false)
{
	h[0] = 0x04, h[1] = 0x22, h[2] = 0x4d, h[3] = 0x18;
	h[4] = uint8_t(0x40 | (linked ? 0 : 0x20) | ((flags & LZ4ADA_COMP_BLOCK_CHECKSUM) ? 0x10 : 0) |
	               ((flags & LZ4ADA_COMP_CONTENT_SIZE) ? 0x08 : 0) | ((flags & LZ4ADA_COMP_CONTENT_CHECKSUM) ? 0x04 : 0) |
	               ((dflags & LZ4ADA_COMP_DICT_WRITE_ID) ? 0x01 : 0));
	h[5] = uint8_t(comp_block_id(block_id) << 4);
	int n = 6;
	if (flags & LZ4ADA_COMP_CONTENT_SIZE)
		for (int i = 0; i < 8; ++i)
			h[n++] = uint8_t(content_size >> (8 * i));
	if (dflags & LZ4ADA_COMP_DICT_WRITE_ID)
		for (int i = 0; i < 4; ++i)
			h[n++] = uint8_t(dict_id >> (8 * i));
	h[n] = uint8_t(walk_descriptor_xxh32(h + 4, n - 4) >> 8);
	return n + 1;
}

}  // namespace lz4ada
