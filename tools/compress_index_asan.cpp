// compress_index_asan.cpp -- the rule by which a compress call writes the seek
// index of its own frames (csrc/lz4ada_compress_index.h: comp_index_frame,
// comp_index_desc, comp_index_block_len; what k_compress_index_frames and
// k_compress_index run and lz4ada_compress_index_host states) under
// AddressSanitizer and UBSan, host code only, against frame_walk
// (csrc/lz4ada_frame_walk.h) over a frame put together here from the same
// written sizes: for every block maximum, record lengths around 0 .. 3 blocks
// and, for 1 MiB and 4 MiB blocks, around the lone-block rule's 24 blocks, with
// every block stored, every block about as short as LZ4 can make it, and sizes
// from a generator -- the verdict (with and without LZ4ADA_NO_LONE), the block count,
// every descriptor as the walk emits it with slots == true, the slots' sum, and
// the checkpoint count against the group starts counted one by one.  The size
// array, the descriptors and the frame are heap arrays of exactly the bytes they
// hold, so a read or write of one entry outside them stops the run.  The frame's
// payload bytes are zeros: neither side reads them.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/compress_index_asan.cpp -o tools/_build/compress_index_asan
//   tools/_build/compress_index_asan > profiles/compress_index_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lz4ada_compress_index.h"

using namespace lz4ada;

static uint64_t rng = 88172645463325252ull;
static uint32_t next()
{
	rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
	return uint32_t(rng >> 16);
}

static long frames = 0, blocks = 0, lone = 0;

// kind 0: every block stored, 1: every block near the shortest, 2: mixed
static bool one(uint64_t n, uint32_t id, uint32_t flags, uint32_t dflags, int kind, bool linked, uint64_t every)
{
	const uint64_t blen = uint64_t(comp_block_len(id));
	const size_t nb = size_t(comp_nblocks(int64_t(n), int64_t(blen)));
	std::unique_ptr<uint32_t[]> csize(new uint32_t[nb]);
	size_t frame_len = size_t(comp_header_len(flags, dflags) + comp_trailer_len(flags));
	for (size_t i = 0; i < nb; ++i) {
		const uint32_t len = comp_index_block_len(n, blen, i);
		// a written size: shorter than the block, and no shorter than LZ4 can make it
		// (a payload of c bytes decodes to at most 255 * c + 64)
		const uint32_t least = len / 255 + 1;
		uint32_t c = kind == 0 ? 0 : kind == 1 ? least + next() % 300 : (next() & 1) ? 0 : least + next() % len;
		if (c >= len)
			c = 0;
		csize[i] = c;
		frame_len += size_t(comp_block_extra(flags)) + comp_index_payload(c, len);
	}
	// the frame the sizes stand for: header, size words, zero payloads, checksums, end mark
	std::unique_ptr<uint8_t[]> frame(new uint8_t[frame_len]);
	memset(frame.get(), 0, frame_len);
	size_t pos = size_t(comp_header(frame.get(), id, flags, n, dflags, 0x1234, linked));
	for (size_t i = 0; i < nb; ++i) {
		const uint32_t len = comp_index_block_len(n, blen, i), in = comp_index_payload(csize[i], len);
		const uint32_t word = in | (csize[i] ? 0u : 0x80000000u);
		for (int k = 0; k < 4; ++k)
			frame[pos + k] = uint8_t(word >> (8 * k));
		pos += 4 + in;
		if (flags & LZ4ADA_COMP_BLOCK_CHECKSUM) {
			const uint32_t ck = 0xC0000000u + uint32_t(i);
			for (int k = 0; k < 4; ++k)
				frame[pos + k] = uint8_t(ck >> (8 * k));
			pos += 4;
		}
	}
	if (pos + size_t(comp_trailer_len(flags)) != frame_len)
		return false;
	bool ok = true;
	for (int no_lone = 0; no_lone < 2; ++no_lone) {
		const uint64_t in_base = 1000003, out_base = 256 * 77;
		std::unique_ptr<lz4ada_block_desc[]> want(new lz4ada_block_desc[nb]);
		lz4ada_frame_info info;
		WalkSums sums;
		WalkEmit e{};
		e.descs = want.get();
		e.cap = int64_t(nb);
		e.slots = true;
		e.in_base = in_base;
		e.out_base = out_base;
		e.out_limit = ~uint64_t(0);
		const int v = frame_walk(frame.get(), int64_t(frame_len), no_lone != 0, &info, &sums, &e, true, ~uint64_t(0));
		const CompIndexFrame f = comp_index_frame(n, blen, csize.get(), linked, every, no_lone != 0);
		ok = ok && v == f.verdict && uint64_t(info.nblocks) == nb && f.nblocks == nb && e.written == int64_t(nb) &&
		     sums.slots == f.slots && info.frame_len == int64_t(frame_len);
		lone += f.verdict == LZ4ADA_BATCH_BIG_BLOCK;
		uint64_t tight = 0, at = size_t(comp_header_len(flags, dflags));
		for (size_t i = 0; i < nb; ++i) {
			const uint32_t len = comp_index_block_len(n, blen, i);
			const lz4ada_block_desc d = comp_index_desc(n, blen, flags, i, csize[i], in_base + at + 4,
			                                            0xC0000000u + uint32_t(i), out_base);
			const lz4ada_block_desc& w = want[i];
			ok = ok && d.in_off == w.in_off && d.in_len == w.in_len && d.flags == w.flags && d.out_off == w.out_off &&
			     d.out_cap == w.out_cap && d.cksum == w.cksum;
			at += uint64_t(comp_block_extra(flags)) + d.in_len;
			tight += (uint64_t(len) + 255) & ~uint64_t(255);
		}
		ok = ok && tight == f.tight;
		uint64_t heads = 0;
		for (uint64_t b = 1; b < nb; ++b)
			heads += f.group && b % f.group == 0;
		const bool lk = linked && nb && f.verdict == LZ4ADA_BATCH_OK;
		ok = ok && f.nckpt == (lk ? heads : 0) && (f.group != 0) == lk &&
		     (!lk || nb < 2 || f.group == (every + blen - 1) / blen);
	}
	++frames;
	blocks += long(nb);
	return ok;
}

int main()
{
	bool ok = true;
	const uint64_t everies[3] = { 65536, 131072, uint64_t(1) << 20 };
	for (uint32_t id : { 0u, 4u, 5u, 6u, 7u }) {
		const uint64_t blen = uint64_t(comp_block_len(id));
		long before = frames, lone_before = lone;
		uint64_t lens[64];
		int nl = 0;
		for (uint64_t base : { uint64_t(0), blen, 2 * blen, 3 * blen })
			for (int64_t d : { -13, -1, 0, 1, 12, 13, 300 })
				if (int64_t(base) + d >= 0)
					lens[nl++] = uint64_t(int64_t(base) + d);
		if (id == 6)  // the lone rule's block count (4 MiB blocks: 24 of them are 96 MiB, left out)
			for (int64_t d : { -1, 0, 1 })
				lens[nl++] = uint64_t(int64_t(24 * blen) + d);
		for (int i = 0; i < nl; ++i)
			for (uint32_t flags = 0; flags < 8; ++flags)
				for (int kind = 0; kind < 3; ++kind) {
					const bool linked = ((flags + kind + i) & 1) != 0;
					const uint32_t dflags = (i & 1) ? LZ4ADA_COMP_DICT_WRITE_ID : 0;
					if (!one(lens[i], id, flags, dflags, kind, linked, everies[(i + kind) % 3])) {
						printf("MISMATCH block id %u, %llu bytes, flags %u, kind %d\n", id,
						       (unsigned long long)lens[i], flags, kind);
						ok = false;
					}
				}
		printf("block id %u (%llu bytes): %ld frames, %ld of them (counted with and without LZ4ADA_NO_LONE) "
		       "LZ4ADA_BATCH_BIG_BLOCK\n",
		       id, (unsigned long long)blen, frames - before, lone - lone_before);
	}
	printf("total %ld frames, %ld blocks -- %s\n", frames, blocks,
	       ok ? "no sanitizer report, the rule is the walk's on every one" : "MISMATCH");
	return ok ? 0 : 1;
}
