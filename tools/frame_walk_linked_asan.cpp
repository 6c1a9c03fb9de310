// frame_walk_linked_asan.cpp -- tools/frame_walk_asan.cpp with the walk's
// take_linked option under AddressSanitizer and UBSan, host
// code only: every truncation of a few frames is copied into a heap block of
// exactly its length and walked with the option off and on (the cap below,
// at and above a linked frame's slots), with and without descriptors, so a
// read of one byte outside [p, p + len) or a write past the descriptor
// capacity stops the run; with the option off every verdict is the plain
// walk's.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan
//       -fno-sanitize-recover=all -Iinclude -Ibo-lz4-ada_amd/csrc tools/frame_walk_linked_asan.cpp -o tools/_build/frame_walk_linked_asan
//   tools/_build/frame_walk_linked_asan > profiles/frame_walk_linked_asan.txt
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
// exact-size heap block, walked with take_linked = take and the cap lmax; the
// whole frame must give `want`.
static bool run(const char* name, const Bytes& f, bool take, uint64_t lmax, int want, int64_t want_len,
                Tally& all, size_t ends = SIZE_MAX)
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
		const int v = frame_walk(p, int64_t(n), false, &info, &sums, nullptr, take, lmax);
		if (!take) {  // off: today's verdict, info and sums
			lz4ada_frame_info i0;
			WalkSums s0;
			if (frame_walk(p, int64_t(n), false, &i0, &s0, nullptr) != v || memcmp(&i0, &info, sizeof i0) ||
			    memcmp(&s0, &sums, sizeof s0))
				ok = false;
		} else if (v != LZ4ADA_BATCH_NOT_INDEXED) {  // on: only a linked verdict may change, to ok within the cap
			lz4ada_frame_info i0;
			WalkSums s0;
			const int v0 = frame_walk(p, int64_t(n), false, &i0, &s0, nullptr);
			if (memcmp(&i0, &info, sizeof i0) || memcmp(&s0, &sums, sizeof s0))
				ok = false;
			if (v0 != LZ4ADA_BATCH_LINKED ? v != v0
			                              : (v == LZ4ADA_BATCH_OK) != (sums.slots <= lmax) &&
			                                    v != LZ4ADA_BATCH_BIG_BLOCK)
				ok = false;
		}
		// again with exactly as many descriptors as it counted, then with one fewer
		const int64_t nb = v == LZ4ADA_BATCH_NOT_INDEXED ? 0 : info.nblocks;
		for (int64_t cap = nb; cap >= 0 && cap >= nb - 1; --cap) {
			lz4ada_block_desc* d = static_cast<lz4ada_block_desc*>(malloc(cap ? size_t(cap) * sizeof *d : 1));
			WalkEmit e{};
			e.descs = d;
			e.cap = cap;
			const int v2 = frame_walk(p, int64_t(n), false, &info2, &sums2, &e, take, lmax);
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
			if (frame_walk(p, int64_t(n), false, &info2, &sums2, &e, take, lmax) != v || e.written != nb)
				ok = false;
			for (int64_t k = 0; k < e.written; ++k)
				if (d[k].in_off < 1000 || d[k].in_off - 1000 + d[k].in_len > n ||
				    d[k].out_off + d[k].out_cap > e.out_limit)
					ok = false;
			e.out_limit -= 256;  // a share one slot short: the last block is left out
			if (frame_walk(p, int64_t(n), false, &info2, &sums2, &e, take, lmax) != v || e.written != nb - 1)
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
	const Bytes linked = modern(4, 5, { 100, 200 });           // slots: 256 + 256
	const Bytes linked_ck = modern(16 | 8 | 4, 4, { 1, 0, 700, 3 });  // slots: 256 + 0 + 768 + 256
	const Bytes lg = legacy({ 500, 3, 700 });
	const int64_t big_len = 7 + 4 + (600 << 10) + 4;
	for (int take = 0; take < 2; ++take) {
		const int lk = take ? LZ4ADA_BATCH_OK : LZ4ADA_BATCH_LINKED;
		printf("take_linked %s\n", take ? "on" : "off");
		ok &= run("modern 64 KiB", plain, take, 1 << 20, LZ4ADA_BATCH_OK, int64_t(plain.size()), all);
		ok &= run("linked, cap above", linked, take, 513, lk, int64_t(linked.size()), all);
		ok &= run("linked, cap at", linked, take, 512, lk, int64_t(linked.size()), all);
		ok &= run("linked, cap below", linked, take, 511, LZ4ADA_BATCH_LINKED, int64_t(linked.size()), all);
		ok &= run("linked, cap 0", linked, take, 0, LZ4ADA_BATCH_LINKED, int64_t(linked.size()), all);
		ok &= run("linked all options, at", linked_ck, take, 1280, lk, int64_t(linked_ck.size()), all);
		ok &= run("linked all options, below", linked_ck, take, 1279, LZ4ADA_BATCH_LINKED,
		          int64_t(linked_ck.size()), all);
		ok &= run("linked empty frame", modern(4, 4, {}), take, 0, lk, 15, all);
		ok &= run("legacy", lg, take, 0, LZ4ADA_BATCH_OK, int64_t(lg.size()), all);
		ok &= run("skippable then linked", cat(skippable(33), linked), take, 1 << 20, LZ4ADA_BATCH_OK, 41, all);
		ok &= run("linked then junk", cat(linked, Bytes{ 1, 2, 3 }), take, 1 << 20, lk, int64_t(linked.size()), all);
		// the lone-block rule comes before the cap
		ok &= run("linked one 600 KiB block", modern(0, 7, { 600u << 10 }), take, uint64_t(1) << 30,
		          take ? LZ4ADA_BATCH_BIG_BLOCK : LZ4ADA_BATCH_LINKED, big_len, all, 300);
	}
	printf("total %ld walks: ok %ld linked %ld big %ld not-indexed %ld -- %s\n", all.walks, all.verdict[0],
	       all.verdict[1], all.verdict[2], all.verdict[4],
	       ok ? "no sanitizer report, every verdict as expected" : "FAILED");
	return ok ? 0 : 1;
}
