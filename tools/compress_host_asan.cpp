// compress_host_asan.cpp -- the compressor's serial statement
// (csrc/lz4ada_compress_host.cpp: lz4ada_compress_block_host,
// lz4ada_compress_frame_host, lz4ada_compress_frames_bound) under
// AddressSanitizer and UBSan, host code only.  Every source and destination is
// a heap block of exactly its length, so a read of one byte outside the record
// or a write past the capacity stops the run.  Covered: every record length
// from 0 to 300 of three kinds of data under no flag and all three, each frame
// decoded again by lz4ada_decode_frame_dict_host; every destination capacity
// from 0 to the bound for three records (frames) and from 0 to the block's
// length (blocks); the crafted cases of tests/test_compress_host_cpu.py --
// literal runs and match lengths at the token and extension edges, a repeat
// 65,535 and 65,536 back in a block of 256 KiB, a repeat inside the last 12
// bytes.  No GPU, no library, nothing loaded into Python:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/compress_host_asan.cpp
//       bo-lz4-ada_amd/csrc/lz4ada_compress_host.cpp bo-lz4-ada_amd/csrc/lz4ada_dict_host.cpp
//       -o tools/_build/compress_host_asan
//   tools/_build/compress_host_asan > profiles/compress_host_asan.txt
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

static Bytes noise(size_t n, uint32_t seed)
{
	g_rng = seed * 2654435761u + 1;
	Bytes b(n);
	for (auto& x : b)
		x = uint8_t(rnd() >> 11);
	return b;
}

static Bytes text(size_t n, uint32_t seed)
{
	static const char* words[] = { "alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta", "iota", "kappa",
		                       "lambda", "mu" };
	g_rng = seed * 2654435761u + 1;
	Bytes b;
	while (b.size() < n) {
		const char* w = words[rnd() % 12];
		b.insert(b.end(), w, w + strlen(w));
		b.push_back(uint8_t(" ,.\n"[rnd() % 4]));
	}
	b.resize(n);
	return b;
}

static uint8_t* exact(const uint8_t* p, size_t n)
{
	uint8_t* q = static_cast<uint8_t*>(malloc(n ? n : 1));
	if (n)
		memcpy(q, p, n);
	return q;
}

static long g_calls = 0;
static void fail(const char* what, long a = 0, long b = 0)
{
	printf("FAIL: %s (%ld, %ld)\n", what, a, b);
	exit(1);
}

// One record as one frame into a destination of exactly `cap` bytes -> the call's result.
static int64_t frame(const Bytes& rec, const lz4ada_compress_options& opt, size_t cap, Bytes* got)
{
	uint8_t* src = exact(rec.data(), rec.size());
	uint8_t* dst = static_cast<uint8_t*>(malloc(cap ? cap : 1));
	const int64_t n = lz4ada_compress_frame_host(rec.empty() ? nullptr : src, int64_t(rec.size()), &opt,
	                                             cap ? dst : nullptr, int64_t(cap));
	++g_calls;
	if (n > int64_t(cap))
		fail("a frame longer than its capacity", long(n), long(cap));
	if (got && n >= 0)
		got->assign(dst, dst + n);
	free(dst);
	free(src);
	return n;
}

static int64_t block(const Bytes& rec, size_t cap, Bytes* got)
{
	uint8_t* src = exact(rec.data(), rec.size());
	uint8_t* dst = static_cast<uint8_t*>(malloc(cap ? cap : 1));
	const int64_t n = lz4ada_compress_block_host(rec.empty() ? nullptr : src, int64_t(rec.size()), cap ? dst : nullptr,
	                                             int64_t(cap));
	++g_calls;
	if (n < 0 || n > int64_t(cap))
		fail("a block longer than its capacity", long(n), long(cap));
	if (got)
		got->assign(dst, dst + n);
	free(dst);
	free(src);
	return n;
}

static int64_t bound_of(size_t n, const lz4ada_compress_options& opt)
{
	lz4ada_compress_job j{};
	j.in_len = int64_t(n);
	return lz4ada_compress_frames_bound(&j, 1, &opt);
}

// The frame at exactly its bound, decoded again from a block of exactly its length.
static size_t round_trip(const Bytes& rec, const lz4ada_compress_options& opt)
{
	const int64_t bound = bound_of(rec.size(), opt);
	Bytes f;
	if (bound < 0 || frame(rec, opt, size_t(bound), &f) <= 0)
		fail("a frame at its bound is refused", long(rec.size()), long(bound));
	uint8_t* in = exact(f.data(), f.size());
	uint8_t* out = static_cast<uint8_t*>(malloc(rec.size() ? rec.size() : 1));
	int64_t olen = -1, used = -1;
	const int st = lz4ada_decode_frame_dict_host(in, int64_t(f.size()), nullptr, 0, rec.empty() ? nullptr : out,
	                                             int64_t(rec.size()), &olen, &used);
	if (st != LZ4ADA_OK || size_t(olen) != rec.size() || size_t(used) != f.size() ||
	    (rec.size() && memcmp(out, rec.data(), rec.size())))
		fail("a frame does not decode to its record", st, long(rec.size()));
	free(out);
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

int main()
{
	const lz4ada_compress_options none{ 4, 0 }, all{ 4, 7 }, id5{ 5, 7 };
	// every record length from 0 to 300, three kinds
	long frames = 0;
	for (size_t n = 0; n <= 300; ++n)
		for (int kind = 0; kind < 3; ++kind) {
			const Bytes rec = kind == 0 ? Bytes(n, 0) : kind == 1 ? noise(n, uint32_t(n)) : text(n, uint32_t(n));
			round_trip(rec, none);
			round_trip(rec, all);
			Bytes b;
			const int64_t len = block(rec, n + n / 255 + 16, &b);
			if (len <= 0 || block(rec, size_t(len), nullptr) != len)  // and into exactly its length
				fail("a block into exactly its length is refused", long(n), long(len));
			frames += 2;
		}
	printf("lengths 0..300 x zeros, noise, text: %ld frames round trip, %ld calls\n", frames, g_calls);

	// every destination capacity from 0 to the bound, three records
	const Bytes recs[3] = { text(300, 7), Bytes(300, 0), text(1500, 8) };
	for (const Bytes& rec : recs) {
		long refused = 0, zero = 0;
		for (const lz4ada_compress_options& opt : { none, all }) {
			const int64_t bound = bound_of(rec.size(), opt);
			for (int64_t cap = 0; cap < bound; ++cap) {
				if (frame(rec, opt, size_t(cap), nullptr) != -int64_t(LZ4ADA_TOO_LITTLE_MEMORY))
					fail("a capacity below the bound is accepted", long(cap), long(bound));
				++refused;
			}
			if (frame(rec, opt, size_t(bound), nullptr) <= 0)
				fail("the bound is refused", long(bound));
		}
		Bytes b;
		const int64_t len = block(rec, rec.size() + 16, &b);
		for (int64_t cap = 0; cap < len; ++cap, ++zero)
			if (block(rec, size_t(cap), nullptr) != 0)
				fail("a block fits a capacity below its length", long(cap), long(len));
		printf("record of %4zu bytes: %ld frame capacities refused, block of %lld bytes: %ld capacities give 0\n",
		       rec.size(), refused, (long long)len, zero);
	}

	// crafted: literal runs and match lengths at the token and extension edges
	const Bytes A = noise(448, 11);
	for (size_t lit : { 14, 15, 16, 269, 270, 271 })
		for (size_t ml : { 18, 19, 20, 273, 274 }) {
			const Bytes rec = cat({ A, slice(A, 0, 32), noise(lit, uint32_t(300 + lit)), slice(A, 64, 64 + ml),
				                noise(20, uint32_t(200 + ml)) });
			round_trip(rec, none);
			round_trip(rec, all);
		}
	// a repeat whose only earlier copy lies 65,535 / 65,536 back, in a block of 256 KiB
	size_t far[2];
	for (int k = 0; k < 2; ++k) {
		const Bytes s = noise(32, 31);
		const Bytes rec = cat({ Bytes(70000, 0), noise(16, 23), s, noise(16, 24), Bytes(65535 + k - 48, 0), s,
			                noise(20, 22) });
		far[k] = round_trip(rec, id5);
	}
	// a repeat that begins 11 and 12 bytes before the end
	for (size_t k : { 11, 12 }) {
		round_trip(cat({ A, slice(A, 0, k) }), none);
		Bytes b;
		block(cat({ A, slice(A, 0, k) }), 600, &b);
	}
	// a block maximum of every id, one record over two blocks of the smallest
	for (uint32_t id : { 0u, 4u, 5u, 6u, 7u })
		round_trip(text(70000, id), lz4ada_compress_options{ id, 7 });
	const lz4ada_compress_options bad{ 3, 0 };
	if (frame(text(10, 1), bad, 64, nullptr) != -int64_t(LZ4ADA_ASSERTION_ERROR))
		fail("block id 3 is accepted");
	printf("crafted: 30 planted repeats, the repeat 65,535 back gives %zu bytes and 65,536 back %zu, ends, ids\n",
	       far[0], far[1]);
	printf("total %ld calls -- no sanitizer report, every short capacity refused, every frame decodes to its record\n",
	       g_calls);
	return 0;
}
