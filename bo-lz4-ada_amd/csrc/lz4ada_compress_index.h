// lz4ada_compress_index.h -- what the compressor knows about the seek index of
// the frames it writes, as host/device code: the one statement
// of the rule by which lz4ada_compress_frames_device_indexed turns a record's
// length and its blocks' written sizes into what lz4ada_seek_index_build*
// would find by walking and sizing the frame.  k_compress_index_frames and
// k_compress_index (lz4ada_compress_index.hip) call it on the device, the host
// replays its per-frame half after a pass (lz4ada_bulk_ranges.cpp) and states
// all of it through lz4ada_compress_index_host, which
// tests/test_compress_index_cpu.py pins to frame_walk, to block_decoded_size
// and to the chain rule, and tools/compress_index_asan.cpp runs over exact-size
// heap blocks.
//
// What makes it arithmetic: the writer cuts a record of n bytes into
// comp_nblocks(n, block_len) blocks, all of block_len bytes but the last, so
// block i decodes to comp_index_block_len bytes and starts at i * block_len.
// A payload of c bytes decodes to at most 255 * c + 64 bytes (walk_slot_cap),
// so a full block's slot capacity is the block maximum whatever it compressed
// to, and the nominal slot of block i lies i * block_len past the frame's
// first; only the last block's capacity depends on its written size.
//
// Depends on lz4ada_hip.h, lz4ada_frame_walk.h, lz4ada_compress.h and
// lz4ada_range_chains.h alone, so a plain C++ program can include it.
#pragma once

#include <stdint.h>

#include "lz4ada_compress.h"
#include "lz4ada_frame_walk.h"
#include "lz4ada_range_chains.h"

namespace lz4ada {

// Decoded bytes of block i of a record of n bytes (i < comp_nblocks(n, block_len)).
LZ4ADA_HD inline uint32_t comp_index_block_len(uint64_t n, uint64_t block_len, uint64_t i)
{
	const uint64_t left = n - i * block_len;
	return uint32_t(left < block_len ? left : block_len);
}

// Payload bytes of a block whose written size is csize (0: stored, its len bytes as they are).
LZ4ADA_HD inline uint32_t comp_index_payload(uint32_t csize, uint32_t len) { return csize ? csize : len; }

// Block i's descriptor as frame_walk emits it with slots == true: its payload
// at `payload_at` (absolute in d_out, past the size word), csize as above,
// cksum the written block checksum (read only under LZ4ADA_COMP_BLOCK_CHECKSUM),
// out_base the nominal slot of the frame's first block.
LZ4ADA_HD inline lz4ada_block_desc comp_index_desc(uint64_t n, uint64_t block_len, uint32_t flags, uint64_t i,
                                                   uint32_t csize, uint64_t payload_at, uint32_t cksum,
                                                   uint64_t out_base)
{
	const bool stored = csize == 0, bck = (flags & LZ4ADA_COMP_BLOCK_CHECKSUM) != 0;
	lz4ada_block_desc d;
	d.in_off = payload_at;
	d.in_len = comp_index_payload(csize, comp_index_block_len(n, block_len, i));
	d.flags = (stored ? LZ4ADA_BLOCK_STORED : 0u) | (bck ? LZ4ADA_BLOCK_HAS_CKSUM : 0u);
	d.out_off = out_base + i * block_len;  // round256(block_len) per earlier block: a full block's capacity
	d.out_cap = walk_slot_cap(d.in_len, stored, int64_t(block_len));
	d.cksum = bck ? cksum : 0u;
	return d;
}

// What the rule says about a whole frame.
struct CompIndexFrame {
	int32_t verdict;   // LZ4ADA_BATCH_OK, or LZ4ADA_BATCH_BIG_BLOCK by frame_walk's lone and big-slot rules
	uint32_t nblocks;  // as written, whatever the verdict
	uint64_t slots;    // its nominal slots: the sum of round256(out_cap)
	uint64_t tight;    // the sum of round256(decoded size), slotp's end entry
	uint64_t group;    // K, the blocks per checkpoint group (a linked frame with blocks; else 0)
	uint64_t nckpt;    // its checkpoints
};

// The frame of a record of n bytes whose blocks' written sizes are csize[0 ..
// nblocks).  linked: a frame of linked blocks, a checkpoint every `every`
// decoded bytes.  no_lone: LZ4ADA_NO_LONE (frame_walk's).  Reads csize only
// where the verdict or the last block's capacity depends on it: at most
// WALK_LONE_BLOCKS + 1 entries.
LZ4ADA_HD inline CompIndexFrame comp_index_frame(uint64_t n, uint64_t block_len, const uint32_t* csize, bool linked,
                                                 uint64_t every, bool no_lone)
{
	CompIndexFrame f;
	const uint64_t nb = uint64_t(comp_nblocks(int64_t(n), int64_t(block_len)));
	f.nblocks = uint32_t(nb);
	f.verdict = LZ4ADA_BATCH_OK;
	f.slots = f.tight = f.group = f.nckpt = 0;
	if (nb == 0)
		return f;
	// a slot capacity is at most the block maximum: the big-slot rule needs a maximum past WALK_SLOT_MAX
	const bool big = block_len > WALK_SLOT_MAX;
	// the lone rule asks for a payload of WALK_LONE_MIN_IN bytes, and no payload exceeds the block length
	uint32_t max_in = 0;
	if (!no_lone && nb <= uint64_t(WALK_LONE_BLOCKS) && block_len >= WALK_LONE_MIN_IN)
		for (uint64_t i = 0; i < nb; ++i) {
			const uint32_t in = comp_index_payload(csize[i], comp_index_block_len(n, block_len, i));
			max_in = in > max_in ? in : max_in;
		}
	if (big || walk_lone(no_lone, int64_t(nb), max_in))
		f.verdict = LZ4ADA_BATCH_BIG_BLOCK;
	const uint32_t last = comp_index_block_len(n, block_len, nb - 1);
	const uint32_t cap = walk_slot_cap(comp_index_payload(csize[nb - 1], last), csize[nb - 1] == 0, int64_t(block_len));
	f.slots = (nb - 1) * block_len + ((uint64_t(cap) + 255) & ~uint64_t(255));
	f.tight = (nb - 1) * block_len + ((uint64_t(last) + 255) & ~uint64_t(255));
	if (linked && f.verdict == LZ4ADA_BATCH_OK) {
		f.group = chain_group(every, chain_block_max(nb, n));
		f.nckpt = chain_checkpoints(f.group, nb);
	}
	return f;
}

}  // namespace lz4ada
