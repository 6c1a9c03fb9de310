// frame_walk_asan.cpp -- the frame walk (csrc/lz4ada_frame_walk.h) under
// AddressSanitizer and UBSan, host code only: every truncation of a few
// frames is copied into a heap block of exactly its length and walked, with
// and without descriptors, so a read of one byte outside [p, p + len) or a
// write past the descriptor capacity stops the run.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/frame_walk_asan.cpp -o tools/_build/frame_walk_asan
//   tools/_build/frame_walk_asan > profiles/frame_walk_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lz4ada_frame_walk.h"

using namespace lz4ada;
using Bytes = std::vector<uint8_t>;

static void put32(Bytes& b, uint32_t v)
{
	for (int i = 0; i < 4; ++i)
		b.push_back(uint8_t(v >> (8 * i)));
}

static void put_payload(Bytes& b, uint32_t n, uint32_t seed)
{
	for (uint32_t i = 0; i < n; ++i)
		b.push_back(uint8_t((seed = seed * 1664525u + 1013904223u) >> 24));
}

// A modern frame of stored blocks: FLG bits as given (version 01 added), BD
// code 4..7, the header checksum computed by the walk's own XXH32.
static Bytes modern(uint8_t flg_bits, unsigned bd_code, const std::vector<uint32_t>& blocks)
{
	Bytes f;
	put32(f, 0x184d2204u);
	const uint8_t flg = uint8_t(0x40 | flg_bits);
	f.push_back(flg);
	f.push_back(uint8_t(bd_code << 4));
	if (flg & 8) {
		uint64_t total = 0;
		for (uint32_t n : blocks)
			total += n;
		put32(f, uint32_t(total));
		put32(f, uint32_t(total >> 32));
	}
	if (flg & 1)
		put32(f, 0x11223344u);
	f.push_back(uint8_t((walk_descriptor_xxh32(f.data() + 4, int64_t(f.size()) - 4) >> 8) & 0xff));
	uint32_t seed = 7;
	for (uint32_t n : blocks) {
		put32(f, 0x80000000u | n);
		put_payload(f, n, seed++);
		if (flg & 16)
			put32(f, 0xdeadbeefu);  // the walk records it, the decoders judge it
	}
	put32(f, 0);
	if (flg & 4)
		put32(f, 0xcafef00du);
	return f;
}

static Bytes legacy(const std::vector<uint32_t>& blocks)
{
	Bytes f;
	put32(f, 0x184c2102u);
	uint32_t seed = 99;
	for (uint32_t n : blocks) {
		put32(f, n);
		put_payload(f, n, seed++);
	}
	return f;
}

static Bytes skippable(uint32_t n)
{
	Bytes f;
	put32(f, 0x184d2a53u);
	put32(f, n);
	put_payload(f, n, 5);
	return f;
}

static Bytes cat(Bytes a, const Bytes& b)
{
	a.insert(a.end(), b.begin(), b.end());
	return a;
}

struct Tally {
	long walks = 0, verdict[5] = { 0, 0, 0, 0, 0 };
};

// Every prefix of f (of a large one: the `ends` shortest and longest) in an
// exact-size heap block; the whole frame must give `want`.
static bool run(const char* name, const Bytes& f, int want, int64_t want_len, Tally& all, size_t ends = SIZE_MAX)
{
	Tally t;
	bool ok = true;
	for (size_t n = 0; n <= f.size(); ++n) {
		if (n > ends && n + ends < f.size())
			continue;
		uint8_t* p = static_cast<uint8_t*>(malloc(n ? n : 1));
		if (n)
			memcpy(p, f.data(), n);
		lz4ada_frame_info info, info2;
		WalkSums sums, sums2;
		const int v = frame_walk(p, int64_t(n), false, &info, &sums, nullptr);
		// again with exactly as many descriptors as it counted, then with one fewer
		const int64_t nb = v == LZ4ADA_BATCH_NOT_INDEXED ? 0 : info.nblocks;
		for (int64_t cap = nb; cap >= 0 && cap >= nb - 1; --cap) {
			lz4ada_block_desc* d = static_cast<lz4ada_block_desc*>(malloc(cap ? size_t(cap) * sizeof *d : 1));
			WalkEmit e{};
			e.descs = d;
			e.cap = cap;
			const int v2 = frame_walk(p, int64_t(n), false, &info2, &sums2, &e);
			if (v2 != v || (v != LZ4ADA_BATCH_NOT_INDEXED && (e.written != cap || info2.frame_len != info.frame_len)))
				ok = false;
			for (int64_t k = 0; k < e.written; ++k)  // in_off / in_len stay inside the input
				if (d[k].in_off + d[k].in_len > n)
					ok = false;
			free(d);
			t.walks++;
		}
		if (nb) {  // as a pass lays them out: slots from 512 on, never past the frame's share
			lz4ada_block_desc* d = static_cast<lz4ada_block_desc*>(malloc(size_t(nb) * sizeof *d));
			WalkEmit e{};
			e.descs = d;
			e.cap = nb;
			e.slots = true;
			e.in_base = 1000;
			e.out_base = 512;
			e.out_limit = 512 + sums.slots;
			if (frame_walk(p, int64_t(n), false, &info2, &sums2, &e) != v || e.written != nb)
				ok = false;
			for (int64_t k = 0; k < e.written; ++k)
				if (d[k].in_off < 1000 || d[k].in_off - 1000 + d[k].in_len > n ||
				    d[k].out_off + d[k].out_cap > e.out_limit)
					ok = false;
			e.out_limit -= 256;  // a share one slot short: the last block is left out
			if (frame_walk(p, int64_t(n), false, &info2, &sums2, &e) != v || e.written != nb - 1)
				ok = false;
			free(d);
			t.walks += 2;
		}
		t.walks++;
		t.verdict[v]++;
		if (n == f.size() && (v != want || (v != LZ4ADA_BATCH_NOT_INDEXED && info.frame_len != want_len)))
			ok = false;
		free(p);
	}
	printf("%-28s %7zu bytes %8ld walks  ok %ld linked %ld big %ld not-indexed %ld  %s\n", name, f.size(),
	       t.walks, t.verdict[0], t.verdict[1], t.verdict[2], t.verdict[4], ok ? "pass" : "FAIL");
	all.walks += t.walks;
	for (int i = 0; i < 5; ++i)
		all.verdict[i] += t.verdict[i];
	return ok;
}

int main()
{
	Tally all;
	bool ok = true;
	const Bytes plain = modern(0x20, 4, { 300, 17, 1, 2000 });
	const Bytes full = modern(0x20 | 16 | 8 | 4 | 1, 7, { 1, 0, 700, 3 });
	const Bytes linked = modern(4, 5, { 100, 200 });
	const Bytes lg = legacy({ 500, 3, 700 });
	ok &= run("modern 64 KiB", plain, LZ4ADA_BATCH_OK, int64_t(plain.size()), all);
	ok &= run("modern all options 4 MiB", full, LZ4ADA_BATCH_OK, int64_t(full.size()), all);
	ok &= run("modern linked", linked, LZ4ADA_BATCH_LINKED, int64_t(linked.size()), all);
	ok &= run("empty frame", modern(0x20 | 4, 4, {}), LZ4ADA_BATCH_OK, 15, all);
	ok &= run("legacy", lg, LZ4ADA_BATCH_OK, int64_t(lg.size()), all);
	ok &= run("legacy then modern", cat(lg, plain), LZ4ADA_BATCH_OK, int64_t(lg.size()), all);
	ok &= run("skippable then modern", cat(skippable(33), plain), LZ4ADA_BATCH_OK, 41, all);
	ok &= run("modern then junk", cat(plain, Bytes{ 1, 2, 3 }), LZ4ADA_BATCH_OK, int64_t(plain.size()), all);
	ok &= run("one 600 KiB block", modern(0x20, 7, { 600u << 10 }), LZ4ADA_BATCH_BIG_BLOCK, 7 + 4 + (600 << 10) + 4,
	          all, 300);
	printf("total %ld walks: ok %ld linked %ld big %ld not-indexed %ld -- %s\n", all.walks, all.verdict[0],
	       all.verdict[1], all.verdict[2], all.verdict[4],
	       ok ? "no sanitizer report, every verdict as expected" : "FAILED");
	return ok ? 0 : 1;
}
