// compress_dict_host_asan.cpp -- the compressor's serial statement with a
// dictionary (csrc/lz4ada_compress_host.cpp: lz4ada_compress_block_dict_host,
// lz4ada_compress_frame_dict_host, lz4ada_compress_frames_bound_dict) under
// AddressSanitizer and UBSan, host code only.  The dictionary, the record and
// the destination are heap blocks of exactly their lengths, and the statement
// indexes the dictionary and the block as two arrays, so a read one byte past
// the dictionary's end, in front of its used tail's allocation or outside the
// record stops the run.  Covered: text records of 1 KiB against dictionaries of
// 1, 3, 4, 5, 63, 64, 65, 1,000, 65,535, 65,536, 65,537 and 100,000 bytes (with
// and without the id, every frame decoded again by
// lz4ada_decode_frame_dict_host); the crafted edges of
// tests/test_compress_dict_host_cpu.py -- eight bytes 65,536 and 65,535 in
// front of record position 0, matches that start 5 .. 11, 64 and 261 .. 263
// bytes before the dictionary's end and run 0 .. 40 bytes into the record, a
// repeat of period 3 from 6 bytes before the end into its own output, the same
// string in the dictionary and earlier in the block, records of 65,537 and
// 131,073 bytes; every record length from 0 to 300 against a 64-byte and a
// 1,000-byte dictionary; every destination capacity below the bound.  No GPU,
// no library, nothing loaded into Python:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/compress_dict_host_asan.cpp
//       bo-lz4-ada_amd/csrc/lz4ada_compress_host.cpp bo-lz4-ada_amd/csrc/lz4ada_dict_host.cpp
//       -o tools/_build/compress_dict_host_asan
//   tools/_build/compress_dict_host_asan > profiles/compress_dict_host_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lz4ada_hip.h"

namespace lz4ada {
static std::string g_msg;
void set_thread_error(const std::string& msg) { g_msg = msg; }  // the library's, for lz4ada_dict_host.cpp
}  // namespace lz4ada

using Bytes = std::vector<uint8_t>;

static uint32_t g_rng = 1;
static uint32_t rnd()
{
	g_rng ^= g_rng << 13, g_rng ^= g_rng >> 17, g_rng ^= g_rng << 5;
	return g_rng;
}

// noise without a zero byte: the crafted dictionaries are zeros with planted strings
static Bytes noise(size_t n, uint32_t seed)
{
	g_rng = seed * 2654435761u + 1;
	Bytes b(n);
	for (auto& x : b)
		x = uint8_t(rnd() >> 11) | 1;
	return b;
}

static Bytes text(size_t n, uint32_t seed)
{
	static const char* words[] = { "alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta", "iota", "kappa",
		                       "lambda", "mu", "nu", "xi", "omicron", "pi", "rho", "sigma", "tau", "upsilon" };
	g_rng = seed * 2654435761u + 1;
	Bytes b;
	while (b.size() < n) {
		const char* w = words[rnd() % 20];
		b.insert(b.end(), w, w + strlen(w));
		b.push_back(uint8_t(" ,.\n"[rnd() % 4]));
	}
	b.resize(n);
	return b;
}

static uint8_t* exact(const Bytes& b)
{
	uint8_t* q = static_cast<uint8_t*>(malloc(b.size() ? b.size() : 1));
	if (!b.empty())
		memcpy(q, b.data(), b.size());
	return q;
}

static long g_calls = 0;
static void fail(const char* what, long a = 0, long b = 0)
{
	printf("FAIL: %s (%ld, %ld)\n", what, a, b);
	exit(1);
}

struct Id {
	bool write;
	uint32_t id;
};

// One record as one frame into a destination of exactly `cap` bytes -> the call's result.
static int64_t frame(const Bytes& rec, const lz4ada_compress_options& opt, const Bytes& dict, Id id, size_t cap,
                     Bytes* got)
{
	uint8_t *src = exact(rec), *d = exact(dict), *dst = static_cast<uint8_t*>(malloc(cap ? cap : 1));
	const int64_t n = lz4ada_compress_frame_dict_host(rec.empty() ? nullptr : src, int64_t(rec.size()), &opt,
	                                                  dict.empty() ? nullptr : d, int64_t(dict.size()), id.id,
	                                                  id.write ? LZ4ADA_COMP_DICT_WRITE_ID : 0u, cap ? dst : nullptr,
	                                                  int64_t(cap));
	++g_calls;
	if (n > int64_t(cap))
		fail("a frame longer than its capacity", long(n), long(cap));
	if (got && n >= 0)
		got->assign(dst, dst + n);
	free(dst);
	free(d);
	free(src);
	return n;
}

static Bytes block(const Bytes& rec, const Bytes& dict)
{
	const size_t cap = rec.size() + rec.size() / 255 + 16;
	uint8_t *src = exact(rec), *d = exact(dict), *dst = static_cast<uint8_t*>(malloc(cap));
	const int64_t n = lz4ada_compress_block_dict_host(rec.empty() ? nullptr : src, int64_t(rec.size()),
	                                                  dict.empty() ? nullptr : d, int64_t(dict.size()), dst,
	                                                  int64_t(cap));
	++g_calls;
	if (n <= 0 || n > int64_t(cap))
		fail("a block does not fit its worst case", long(n), long(cap));
	Bytes out(dst, dst + n);
	// and into exactly its length, and refused one below
	uint8_t* tight = static_cast<uint8_t*>(malloc(size_t(n)));
	if (lz4ada_compress_block_dict_host(rec.empty() ? nullptr : src, int64_t(rec.size()), dict.empty() ? nullptr : d,
	                                    int64_t(dict.size()), tight, n) != n ||
	    memcmp(tight, dst, size_t(n)) ||
	    lz4ada_compress_block_dict_host(rec.empty() ? nullptr : src, int64_t(rec.size()), dict.empty() ? nullptr : d,
	                                    int64_t(dict.size()), tight, n - 1) != 0)
		fail("a block into exactly its length", long(n));
	g_calls += 2;
	free(tight);
	free(dst);
	free(d);
	free(src);
	return out;
}

static int64_t bound_of(size_t n, const lz4ada_compress_options& opt, Id id)
{
	lz4ada_compress_job j{};
	j.in_len = int64_t(n);
	const lz4ada_compress_dict cd{ nullptr, 0, id.id, id.write ? LZ4ADA_COMP_DICT_WRITE_ID : 0u };
	return lz4ada_compress_frames_bound_dict(&j, 1, &opt, &cd);
}

// The frame at exactly its bound, decoded again from blocks of exactly their lengths.
static size_t round_trip(const Bytes& rec, const lz4ada_compress_options& opt, const Bytes& dict, Id id = { false, 0 })
{
	const int64_t bound = bound_of(rec.size(), opt, id);
	Bytes f;
	if (bound < 0 || frame(rec, opt, dict, id, size_t(bound), &f) <= 0)
		fail("a frame at its bound is refused", long(rec.size()), long(bound));
	if (bound > 0 && frame(rec, opt, dict, id, size_t(bound - 1), nullptr) != -int64_t(LZ4ADA_TOO_LITTLE_MEMORY))
		fail("a capacity below the bound is accepted", long(bound));
	if (((f[4] & 1) != 0) != id.write)
		fail("FLG bit 0 and the id disagree", f[4]);
	uint8_t *in = exact(f), *d = exact(dict), *out = static_cast<uint8_t*>(malloc(rec.size() ? rec.size() : 1));
	int64_t olen = -1, used = -1;
	const int st = lz4ada_decode_frame_dict_host(in, int64_t(f.size()), dict.empty() ? nullptr : d, int64_t(dict.size()),
	                                             rec.empty() ? nullptr : out, int64_t(rec.size()), &olen, &used);
	if (st != LZ4ADA_OK || size_t(olen) != rec.size() || size_t(used) != f.size() ||
	    (rec.size() && memcmp(out, rec.data(), rec.size())))
		fail("a frame does not decode to its record", st, long(rec.size()));
	free(out);
	free(d);
	free(in);
	return f.size();
}

static Bytes cat(std::initializer_list<Bytes> parts)
{
	Bytes b;
	for (const Bytes& p : parts)
		b.insert(b.end(), p.begin(), p.end());
	return b;
}

static Bytes slice(const Bytes& b, size_t lo, size_t hi) { return Bytes(b.begin() + lo, b.begin() + hi); }
static Bytes tail_of(const Bytes& b, size_t n) { return slice(b, b.size() - n, b.size()); }

int main()
{
	const lz4ada_compress_options none{ 4, 0 }, all{ 4, 7 };
	const Bytes none_dict;

	// dictionary lengths around 4 and 65,536, text records of 1 KiB
	const Bytes dtext = text(100000, 7);
	for (size_t dl : { 1, 3, 4, 5, 63, 64, 65, 1000, 65535, 65536, 65537, 100000 }) {
		const Bytes d = tail_of(dtext, dl);
		size_t with = 0, without = 0;
		for (uint32_t seed = 1; seed <= 3; ++seed) {
			const Bytes rec = text(1024, 100 + seed);
			with += round_trip(rec, none, d);
			round_trip(rec, all, d, { true, 0xC0FFEE42u });
			without += round_trip(rec, none, none_dict);
			const Bytes b = block(rec, d);
			if (dl <= 3 && b != block(rec, none_dict))
				fail("a dictionary under 4 bytes changes the block", long(dl));
			if (dl > 65536) {
				Bytes other = d;
				for (size_t i = 0; i < dl - 65536; ++i)
					other[i] ^= 0x55;
				if (block(rec, other) != b || block(rec, tail_of(d, 65536)) != b)
					fail("bytes in front of the last 65,536 change the block", long(dl));
			}
		}
		printf("dictionary of %6zu bytes: 3 x 1 KiB of text give %zu bytes, %zu without\n", dl, with, without);
	}

	// every record length from 0 to 300 against a 64-byte and a 1,000-byte dictionary
	for (size_t dl : { 64, 1000 }) {
		const Bytes d = tail_of(dtext, dl);
		for (size_t n = 0; n <= 300; ++n) {
			const Bytes rec = n % 2 ? text(n, uint32_t(n)) : cat({ slice(d, dl - n % 50 - 8, dl), text(n, uint32_t(n)) });
			round_trip(slice(rec, 0, n), none, d);
			round_trip(slice(rec, 0, n), all, d, { true, uint32_t(n) });
			if (n)
				block(slice(rec, 0, n), d);
		}
	}
	printf("lengths 0..300 against 64 and 1,000 bytes: %ld calls so far\n", g_calls);

	// every destination capacity from 0 to the bound, with the id
	{
		const Bytes rec = text(300, 9), d = tail_of(dtext, 1000);
		long refused = 0;
		for (const lz4ada_compress_options& opt : { none, all }) {
			const int64_t bound = bound_of(rec.size(), opt, { true, 5 });
			if (bound != bound_of(rec.size(), opt, { false, 5 }) + 4)
				fail("the id adds other than 4 bytes to the bound", long(bound));
			for (int64_t cap = 0; cap < bound; ++cap, ++refused)
				if (frame(rec, opt, d, { true, 5 }, size_t(cap), nullptr) != -int64_t(LZ4ADA_TOO_LITTLE_MEMORY))
					fail("a capacity below the bound is accepted", long(cap), long(bound));
		}
		printf("record of 300 bytes with the id: %ld frame capacities refused\n", refused);
	}

	// crafted: eight bytes 65,536 and 65,535 in front of record position 0
	const Bytes S = noise(8, 41), tail = noise(20, 42);
	const Bytes rec_s = cat({ S, tail });
	const Bytes far = block(rec_s, cat({ S, Bytes(65536 - 8, 0) }));
	const Bytes near = block(rec_s, cat({ Bytes(1, 0), S, Bytes(65536 - 9, 0) }));
	const Bytes near_long = block(rec_s, cat({ noise(34464, 43), Bytes(1, 0), S, Bytes(65536 - 9, 0) }));
	if (far.size() != 30 || far[0] != 0xF0)
		fail("eight bytes 65,536 back are matched", long(far.size()));
	if (near.size() != 25 || near[0] != 0x04 || near[1] != 0xFF || near[2] != 0xFF || near_long != near)
		fail("eight bytes 65,535 back are not matched", long(near.size()));
	round_trip(rec_s, none, cat({ S, Bytes(65536 - 8, 0) }));
	round_trip(rec_s, none, cat({ Bytes(1, 0), S, Bytes(65536 - 9, 0) }));
	// matches that start k bytes before the dictionary's end and run m bytes into the record
	const Bytes R0 = noise(40, 44), fill = noise(30, 45);
	long crossings = 0;
	for (size_t k : { 5, 6, 7, 8, 9, 10, 11, 64, 261, 262, 263 })
		for (size_t m : { 0, 1, 2, 3, 7, 40 }) {
			const Bytes U = noise(k, 46), d = cat({ Bytes(1000, 0), U });
			Bytes end = noise(20, 47);
			end[0] = uint8_t((m < 40 ? R0[m] : fill[0]) ^ 0x80);
			const Bytes rec = cat({ R0, fill, U, slice(R0, 0, m), end });
			const Bytes b = block(rec, d);
			// 70 literals (token, one extension byte), offset 70 + k, then 20 literals
			const size_t ext = k + m - 4 < 15 ? 0 : (k + m - 4 - 15) / 255 + 1;
			if (b.size() != 2 + 70 + 2 + ext + 2 + 20 || b[72] != uint8_t(70 + k) || b[73] != uint8_t((70 + k) >> 8))
				fail("a match across the dictionary's end has another shape", long(k), long(m));
			round_trip(rec, none, d);
			round_trip(rec, all, d, { true, 1 });
			++crossings;
		}
	// a repeat of period 3 from 6 bytes before the dictionary's end into its own output
	{
		Bytes abc;
		for (int i = 0; i < 100; ++i)
			abc.insert(abc.end(), { 'a', 'b', 'c' });
		Bytes end = noise(20, 48);
		end[0] = 'x';
		const Bytes d = cat({ Bytes(500, 0), slice(abc, 0, 60) }), rec = cat({ abc, end });
		const Bytes b = block(rec, d);
		if (b[0] != 0x0F || b[1] != 6 || b[2] != 0)
			fail("the period-3 repeat does not begin 6 bytes back", b[1]);
		round_trip(rec, none, d);
	}
	// the same string in the dictionary and earlier in the block
	{
		const Bytes T = noise(16, 49), a = noise(50, 50), gap = noise(33, 51);
		Bytes end = noise(20, 52);
		end[0] = uint8_t(gap[0] ^ 0x80);
		const Bytes d = cat({ Bytes(1000, 0), T, Bytes(40, 0) }), rec = cat({ a, T, gap, T, end });
		round_trip(rec, none, d);
		block(rec, d);
	}
	// records of 65,537 and 131,073 bytes: the dictionary lies in front of every block
	{
		const Bytes d = tail_of(dtext, 65536), t = text(131073, 8);
		round_trip(slice(t, 0, 65537), all, d, { true, 2 });
		round_trip(cat({ slice(t, 0, 65536), tail_of(d, 100), slice(t, 65636, 131073) }), none, d);
		round_trip(t, lz4ada_compress_options{ 5, 7 }, d);
	}
	// misuse
	{
		uint8_t buf[64];
		const uint8_t abc[4] = { 'a', 'b', 'c', 'd' };
		if (lz4ada_compress_frame_dict_host(abc, 3, &none, abc, -1, 0, 0, buf, 64) != -int64_t(LZ4ADA_ASSERTION_ERROR) ||
		    lz4ada_compress_frame_dict_host(abc, 3, &none, nullptr, 4, 0, 0, buf, 64) != -int64_t(LZ4ADA_ASSERTION_ERROR) ||
		    lz4ada_compress_frame_dict_host(abc, 3, &none, abc, 4, 0, 2, buf, 64) != -int64_t(LZ4ADA_ASSERTION_ERROR) ||
		    lz4ada_compress_block_dict_host(abc, 3, nullptr, 4, buf, 64) != -1)
			fail("misuse is accepted");
	}
	printf("crafted: 65,536 back gives %zu bytes and 65,535 back %zu, %ld crossings, period 3, block wins, blocks\n",
	       far.size(), near.size(), crossings);
	printf("total %ld calls -- no sanitizer report, every short capacity refused, every frame decodes to its record\n",
	       g_calls);
	return 0;
}
