// compress_linked_host_asan.cpp -- the serial statement of a frame of linked
// blocks (csrc/lz4ada_compress_host.cpp: lz4ada_compress_frame_linked_host)
// under AddressSanitizer and UBSan, host code only.  The record, the
// dictionary and the destination are heap blocks of exactly their lengths, and
// a continuation block's history is the record itself, so a read in front of
// the record (a window that reaches before position 0 of block 1's 65,536
// bytes), past its end or outside the dictionary stops the run.  Covered: every
// record length from 65,536 to 65,536 + 300, text and a repeat of the bytes in
// front of the boundary; the crafted records of
// tests/_compress_linked_cases.py -- eight bytes 65,536 and 65,535 in front of a
// position of block 1, matches that start 4 .. 11 bytes before the boundary and
// run 0 .. 40 bytes into the block, four bytes astride the boundary that are not
// seeded, a repeat of period 3 from 6 bytes before the boundary into its own
// output, the same string in the history and earlier in the block, a stored
// block of noise in front of a compressible one, last blocks of 13 and 12
// bytes; records of 131,072 and 131,073 bytes; 300,000 bytes in blocks of
// 256 KiB; a dictionary in front of block 0; every destination capacity below
// the bound of a short two-block record.  Every frame is decoded again by
// lz4ada_decode_frame_dict_host.  No GPU, no library, nothing loaded into
// Python:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/compress_linked_host_asan.cpp
//       bo-lz4-ada_amd/csrc/lz4ada_compress_host.cpp bo-lz4-ada_amd/csrc/lz4ada_dict_host.cpp
//       -o tools/_build/compress_linked_host_asan
//   tools/_build/compress_linked_host_asan > profiles/compress_linked_host_asan.txt
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

static const size_t B = 65536;

static uint32_t g_rng = 1;
static uint32_t rnd()
{
	g_rng ^= g_rng << 13, g_rng ^= g_rng >> 17, g_rng ^= g_rng << 5;
	return g_rng;
}

// noise without a zero byte: the crafted first blocks are zeros with planted strings
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

// One record as one linked frame into a destination of exactly `cap` bytes -> the call's result.
static int64_t frame(const Bytes& rec, const lz4ada_compress_options& opt, const Bytes& dict, size_t cap, Bytes* got)
{
	uint8_t *src = exact(rec), *d = exact(dict), *dst = static_cast<uint8_t*>(malloc(cap ? cap : 1));
	const int64_t n = lz4ada_compress_frame_linked_host(rec.empty() ? nullptr : src, int64_t(rec.size()), &opt,
	                                                    dict.empty() ? nullptr : d, int64_t(dict.size()), 0, 0u,
	                                                    cap ? dst : nullptr, int64_t(cap));
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

static int64_t bound_of(size_t n, const lz4ada_compress_options& opt)
{
	lz4ada_compress_job j{};
	j.in_len = int64_t(n);
	return lz4ada_compress_frames_bound_dict(&j, 1, &opt, nullptr);
}

// The frame at exactly its bound, B.Indep clear, decoded again from blocks of
// exactly their lengths -> its length.
static size_t round_trip(const Bytes& rec, const lz4ada_compress_options& opt, const Bytes& dict = Bytes())
{
	const int64_t bound = bound_of(rec.size(), opt);
	Bytes f;
	if (bound < 0 || frame(rec, opt, dict, size_t(bound), &f) <= 0)
		fail("a frame at its bound is refused", long(rec.size()), long(bound));
	if (frame(rec, opt, dict, size_t(bound - 1), nullptr) != -int64_t(LZ4ADA_TOO_LITTLE_MEMORY))
		fail("a capacity below the bound is accepted", long(bound));
	if (f[4] & 0x20)
		fail("B.Indep is set", f[4]);
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

// 65,536 zeros with s planted so that its first byte lies k bytes before the end
static Bytes block0(size_t k, const Bytes& s)
{
	Bytes b(B, 0);
	memcpy(b.data() + (B - k), s.data(), s.size());
	return b;
}

// Block 1 of the frame of rec (no checksums, no size): its size word and the bytes behind it.
static Bytes block1(const Bytes& rec)
{
	const lz4ada_compress_options none{ 4, 0 };
	Bytes f;
	frame(rec, none, Bytes(), size_t(bound_of(rec.size(), none)), &f);
	const uint32_t w0 = uint32_t(f[7]) | uint32_t(f[8]) << 8 | uint32_t(f[9]) << 16 | uint32_t(f[10]) << 24;
	const size_t at = 7 + 4 + (w0 & 0x7FFFFFFFu);
	return slice(f, at, f.size() - 4);
}

int main()
{
	const lz4ada_compress_options none{ 4, 0 }, all{ 4, 7 };

	// every record length from 65,536 to 65,536 + 300: text, and a last block
	// that repeats what lies in front of the boundary
	{
		const Bytes t = text(B + 300, 3);
		size_t linked = 0;
		for (size_t n = B; n <= B + 300; ++n) {
			linked += round_trip(slice(t, 0, n), none);
			round_trip(cat({ slice(t, 0, B), slice(t, B - (n - B) % 97 - 8, B - (n - B) % 97 - 8 + (n - B)) }), all);
		}
		printf("lengths 65,536 .. 65,836: %ld calls so far, %zu bytes of frames\n", g_calls, linked);
	}

	// every destination capacity from 0 to the bound of a two-block record
	{
		const Bytes rec = text(B + 13, 9);
		const int64_t bound = bound_of(rec.size(), all);
		long refused = 0;
		for (int64_t cap = 0; cap < bound; ++cap, ++refused)
			if (frame(rec, all, Bytes(), size_t(cap), nullptr) != -int64_t(LZ4ADA_TOO_LITTLE_MEMORY))
				fail("a capacity below the bound is accepted", long(cap), long(bound));
		printf("record of 65,549 bytes: %ld frame capacities below %ld refused\n", refused, long(bound));
	}

	// crafted: eight bytes 65,536 and 65,535 in front of a position of block 1
	const Bytes S = noise(8, 41), tail = noise(20, 42), lead = noise(7, 43);
	{
		const Bytes far = block1(cat({ block0(B, S), S, tail })), near = block1(cat({ block0(B - 1, S), S, tail }));
		const Bytes far7 = block1(cat({ block0(B - 7, S), lead, S, tail }));
		const Bytes near7 = block1(cat({ block0(B - 8, S), lead, S, tail }));
		// a literal run is not shorter than the block: stored
		if (far.size() != 4 + 28 || far[3] != 0x80 || far7.size() != 4 + 35 || far7[3] != 0x80)
			fail("eight bytes 65,536 back are matched", long(far.size()), long(far7.size()));
		if (near.size() != 4 + 25 || near[4] != 0x04 || near[5] != 0xFF || near[6] != 0xFF)
			fail("eight bytes 65,535 back are not matched", long(near.size()));
		if (near7.size() != 4 + 32 || near7[4] != 0x74 || near7[12] != 0xFF || near7[13] != 0xFF)
			fail("eight bytes 65,535 back of position 7 are not matched", long(near7.size()));
		round_trip(cat({ block0(B, S), S, tail }), all);
		round_trip(cat({ block0(B - 1, S), S, tail }), all);
		round_trip(cat({ block0(B - 7, S), lead, S, tail }), none);
		round_trip(cat({ block0(B - 8, S), lead, S, tail }), none);
	}
	// matches that start k bytes before the boundary and run m bytes into the block
	const Bytes R0 = noise(40, 44), fill = noise(30, 45);
	long crossings = 0;
	for (size_t k : { 4, 5, 6, 7, 8, 9, 10, 11 })
		for (size_t m : { 0, 1, 2, 3, 7, 9, 40 }) {
			const Bytes U = noise(k, 46);
			Bytes end = noise(20, 47);
			end[0] = uint8_t((m < 40 ? R0[m] : fill[0]) ^ 0x80);
			const Bytes rec = cat({ block0(k, U), R0, fill, U, slice(R0, 0, m), end });
			const Bytes b = block1(rec);
			// 70 literals (token, one extension byte), offset 70 + k, then 20 literals
			// -- 96 bytes and the extension, which a match under 7 bytes does not undercut: stored
			const size_t ext = k + m - 4 < 15 ? 0 : (k + m - 4 - 15) / 255 + 1, len = 70 + k + m + 20;
			if (96 + ext >= len ? b.size() != 4 + len || b[3] != 0x80
			                    : b.size() != 4 + 96 + ext || b[4 + 72] != uint8_t(70 + k) || b[4 + 73] != 0)
				fail("a match across the boundary has another shape", long(k), long(m));
			round_trip(rec, none);
			round_trip(rec, all);
			++crossings;
		}
	// -3 .. -1 are not seeded: four bytes astride the boundary come again and are not found
	{
		const Bytes T3 = noise(3, 48), first = noise(1, 49);
		Bytes mid = noise(30, 50), end = noise(20, 51);
		end[0] = uint8_t(mid[0] ^ 0x80);
		const Bytes rec = cat({ block0(3, T3), first, mid, T3, first, end });
		if (block1(rec)[3] != 0x80)
			fail("four bytes astride the boundary are found");
		round_trip(rec, none);
	}
	// a repeat of period 3 from 6 bytes before the boundary into its own output
	{
		Bytes abc;
		for (int i = 0; i < 100; ++i)
			abc.insert(abc.end(), { 'a', 'b', 'c' });
		Bytes end = noise(20, 52);
		end[0] = 'x';
		const Bytes rec = cat({ block0(60, slice(abc, 0, 60)), abc, end });
		const Bytes b = block1(rec);
		if (b[4] != 0x0F || b[5] != 6 || b[6] != 0)
			fail("the period-3 repeat does not begin 6 bytes back", b[5]);
		round_trip(rec, none);
	}
	// the same string in the history and earlier in the block
	{
		const Bytes T = noise(16, 53), a = noise(50, 54), gap = noise(33, 55);
		Bytes end = noise(20, 56);
		end[0] = uint8_t(gap[0] ^ 0x80);
		const Bytes rec = cat({ block0(56, T), a, T, gap, T, end });
		const Bytes b = block1(rec);
		if (b[4 + 2 + 50] != 50 + 40 + 16)
			fail("the history's position wins over the block's", b[4 + 2 + 50]);
		round_trip(rec, none);
	}
	// last blocks of 13 and 12 bytes; a stored block of noise in front of a compressible one
	{
		const Bytes P = noise(13, 57);
		const Bytes b13 = block1(cat({ block0(500, slice(P, 0, 8)), P }));
		if (b13.size() != 4 + 9 || b13[4] != 0x04)
			fail("a last block of 13 bytes holds no match", long(b13.size()));
		if (block1(cat({ block0(500, slice(P, 0, 8)), slice(P, 0, 12) }))[3] != 0x80)
			fail("a last block of 12 bytes is not stored");
		round_trip(cat({ block0(500, slice(P, 0, 8)), P }), all);
		round_trip(cat({ block0(500, slice(P, 0, 8)), slice(P, 0, 12) }), all);
		g_rng = 61;
		Bytes nz(B);
		for (auto& x : nz)
			x = uint8_t(rnd() >> 9);
		const Bytes rec = cat({ text(B, 62), nz, slice(nz, B - 1000, B), text(3000, 63) });
		const size_t with = round_trip(rec, all);
		printf("text, noise, the noise's last 1,000 bytes and text: %zu bytes of %zu\n", with, rec.size());
	}
	// records of 131,072 and 131,073 bytes; 300,000 bytes in blocks of 256 KiB; a dictionary in front of block 0
	{
		const Bytes t = text(300000, 8), d = text(100000, 7);
		round_trip(slice(t, 0, 2 * B), none);
		round_trip(slice(t, 0, 2 * B + 1), all);
		round_trip(t, lz4ada_compress_options{ 5, 7 });
		round_trip(slice(t, 0, 2 * B + 1), all, d);
		round_trip(cat({ slice(t, 0, B), slice(d, d.size() - 100, d.size()), slice(t, B + 100, 2 * B + 1) }), none, d);
		round_trip(t, lz4ada_compress_options{ 5, 0 }, slice(d, 0, 1000));
	}
	// misuse
	{
		uint8_t buf[64];
		const uint8_t abc[4] = { 'a', 'b', 'c', 'd' };
		const lz4ada_compress_options closed{ 4, 0x20 };
		if (lz4ada_compress_frame_linked_host(abc, 3, &none, abc, -1, 0, 0, buf, 64) != -int64_t(LZ4ADA_ASSERTION_ERROR) ||
		    lz4ada_compress_frame_linked_host(abc, 3, &none, nullptr, 4, 0, 0, buf, 64) != -int64_t(LZ4ADA_ASSERTION_ERROR) ||
		    lz4ada_compress_frame_linked_host(abc, 3, &none, abc, 4, 0, 2, buf, 64) != -int64_t(LZ4ADA_ASSERTION_ERROR) ||
		    lz4ada_compress_frame_linked_host(abc, 3, &closed, nullptr, 0, 0, 0, buf, 64) != -int64_t(LZ4ADA_ASSERTION_ERROR))
			fail("misuse is accepted");
	}
	printf("crafted: 65,536 back stored and 65,535 back matched, %ld crossings, astride, period 3, block wins, "
	       "last 13 and 12, stored history, blocks\n",
	       crossings);
	printf("total %ld calls -- no sanitizer report, every short capacity refused, every frame decodes to its record\n",
	       g_calls);
	return 0;
}
