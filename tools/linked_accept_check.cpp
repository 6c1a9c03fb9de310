// linked_accept_check.cpp -- the round state (lz4ada_round_state.h) and the
// linked bulk path's host decisions (lz4ada_linked_accept.h: laying a batch,
// accepting blocks, plane modes) against a plain restatement of
// their rules, under AddressSanitizer and UBSan, host code only.  No GPU, no
// library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan
//       -fno-sanitize-recover=all -Iinclude -Ibo-lz4-ada_amd/csrc tools/linked_accept_check.cpp
//       -o tools/_build/linked_accept_check
//
// The rules as restated here: a block starts at 0 once the position has reached
// 65536, else at the position; the position advances by the decoded length, and
// the history position follows it when it has reached 65536; quirk D1 is live
// while the history position lies in 65536..65542.  A batch's blocks are
// accepted up to the first one with a status code, with a stored checksum that
// differs, or with a D1-risk match that either lies in a D1 round and was not
// decoded under exactly that round's state with plane z's decode good, or lies
// outside one and was decoded under a prediction.
//
// Inputs, random with a fixed seed: both positions from {0, 1, 65535, 65536,
// 65539, 65542, 65543, 131072}; 1 to 6 blocks of lengths from {0, 1, 65535,
// 65536, 65542, 65543}; per block a code or none, a checksum equal, different or
// absent, the risk and emulation bits, plane z good or declined, and prediction
// flags that match the real state or are off by one in either field.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "lz4ada_linked_accept.h"

using namespace lz4ada;

static const int64_t POS[8] = { 0, 1, 65535, 65536, 65539, 65542, 65543, 131072 };
static const uint32_t LEN[6] = { 0, 1, 65535, 65536, 65542, 65543 };

// ---- the restatement (none of the headers' functions or constants)
struct Plain {
	int64_t pos, hist;
};
static int64_t plain_start(Plain& s) { return s.pos = s.pos >= 65536 ? 0 : s.pos; }
static void plain_advance(Plain& s, int64_t len)
{
	s.pos += len;
	if (s.pos >= 65536)
		s.hist = s.pos;
}
static bool plain_d1(const Plain& s) { return s.hist >= 65536 && s.hist <= 65542; }
// descriptor flags: bit 3 a D1 round, bits 4-6 the history position - 65536, bits 16.. the start
static uint32_t plain_flags(uint32_t oph3, int64_t n1) { return 8u | (oph3 << 4) | (uint32_t(n1) << 16); }

enum Outcome { ALL, STOP_CODE, STOP_CKSUM, STOP_D1_ROUND, STOP_EMU, HELD, STOP_AT_0, N_OUT };
static const char* const OUT_NAME[N_OUT] = { "all blocks accepted",
	                                     "stop on a block code",
	                                     "stop on a block checksum",
	                                     "stop in a D1 round without a valid prediction",
	                                     "stop outside a D1 round on an emulated block",
	                                     "accepted because the prediction held",
	                                     "stop at block 0" };

[[noreturn]] static void fail(const char* what, long c)
{
	printf("FAIL: %s (case %ld)\n", what, c);
	exit(1);
}

static void check_round_state()
{
	for (int64_t p : POS)
		for (int64_t h : POS)
			for (uint32_t len : LEN) {
				RoundState r;
				r.pos = p;
				r.history = h;
				Plain s{ p, h };
				if (r.in_d1() != plain_d1(s))
					fail("in_d1", p);
				const int64_t ns = r.next_start();
				if (r.pos != p || ns != plain_start(s) || r.start() != ns || r.pos != s.pos || r.history != h)
					fail("start", p);
				r.advance(len);
				plain_advance(s, len);
				if (r.pos != s.pos || r.history != s.hist || r.in_d1() != plain_d1(s))
					fail("advance", p);
			}
}

int main()
{
	check_round_state();
	std::mt19937 rng(0x4C5A3441u);
	auto pick = [&](uint32_t n) { return uint32_t(rng() % n); };
	long counts[N_OUT] = {};
	const long CASES = 400000;
	for (long c = 0; c < CASES; ++c) {
		const Plain s0{ POS[pick(8)], POS[pick(8)] };
		const uint32_t nb = 1 + pick(6);

		// ---- laying: stored blocks decode to their length, compressed ones to at most 255 x + 64
		const int64_t bmax = pick(2) ? 65536 : int64_t(4) << 20;
		std::vector<lz4ada_block_desc> d(nb);
		for (auto& x : d) {
			x = lz4ada_block_desc{};
			x.in_len = pick(2) ? LEN[pick(6)] : pick(600);
			x.flags = pick(4) | (pick(2) ? 0xfffffffcu & rng() : 0u);  // stale bits above the public two
			x.cksum = rng();
		}
		std::vector<lz4ada_block_desc> laid(d);
		const uint64_t bytes = lay_batch(laid, bmax, RoundState{ s0.pos, s0.hist });
		{
			Plain s = s0;
			uint64_t at = 0;
			for (uint32_t i = 0; i < nb; ++i) {
				uint64_t cap = (d[i].flags & 1u) ? d[i].in_len : 255ull * d[i].in_len + 64;
				if (!(d[i].flags & 1u) && cap > uint64_t(bmax))
					cap = uint64_t(bmax);
				plain_start(s);
				const uint32_t want = (d[i].flags & 3u) | (plain_d1(s) ? plain_flags(uint32_t(s.hist - 65536), s.pos) : 0u);
				if (laid[i].out_cap != cap || laid[i].out_off != at + 65536 || laid[i].flags != want ||
				    laid[i].in_len != d[i].in_len || laid[i].cksum != d[i].cksum)
					fail("lay_batch: a block's slot or predicted flags", c);
				at += 65536 + (cap + 255) / 256 * 256;
				plain_advance(s, int64_t(cap));
			}
			if (bytes != at)
				fail("lay_batch: the batch's bytes", c);
		}

		// ---- accepting: statuses and prediction flags drawn around the real state
		std::vector<lz4ada_block_status> stx(nb), stz(nb);
		std::vector<int64_t> want_A;
		std::vector<Plain> want_at;  // per block looked at: the state at its start, its D1 verdict
		std::vector<bool> want_d1;
		Plain s = s0;
		uint32_t want_count = nb;
		int64_t want_bytes = 0;
		int stop = ALL;
		bool held = false;
		for (uint32_t i = 0; i < nb; ++i) {
			lz4ada_block_desc& x = d[i];
			lz4ada_block_status &sx = stx[i], &sz = stz[i];
			sx = sz = lz4ada_block_status{};
			sx.code = pick(8) ? 0 : 1 + int32_t(pick(11));
			sx.out_len = LEN[pick(6)];
			const bool risk = pick(2), emu = pick(2), z_ok = pick(4) != 0;
			sx.aux = (risk ? 1 : 0) | (emu ? 4 : 0);
			sz.code = z_ok ? 0 : 10;
			sz.aux = pick(2) ? 2 : 0;
			const uint32_t ck = pick(8);  // mostly equal or absent
			x.flags = (x.flags & 1u) | (ck < 6 ? 2u : 0u);
			sx.cksum = ck == 5 ? x.cksum ^ 0x10u : x.cksum;
			const bool ck_bad = ck == 5;
			// the real state at this block (only while no earlier block stopped)
			Plain at = s;
			plain_start(at);
			const bool in_d1 = plain_d1(at);
			const uint32_t oph3 = in_d1 ? uint32_t(at.hist - 65536) : 0u;
			const uint32_t pred = pick(4);  // 0, 1: the real state; 2: OPH off by one; 3: N1 off by one
			bool matches = pred < 2 && in_d1;
			if (pred < 2)
				x.flags |= in_d1 ? plain_flags(oph3, at.pos) : 0u;
			else if (pred == 2)
				x.flags |= plain_flags((oph3 + 1) & 7u, at.pos);
			else
				x.flags |= plain_flags(oph3, (at.pos + 1) & 0xffff);
			if (want_count != nb)
				continue;  // past the stop: the acceptor must not look here
			const bool valid = emu && matches && z_ok;  // decoded under exactly this D1 round's state
			const bool d1_stop = risk && (in_d1 ? !valid : emu);
			const int why = sx.code != 0 ? STOP_CODE : ck_bad ? STOP_CKSUM : !d1_stop ? ALL : in_d1 ? STOP_D1_ROUND : STOP_EMU;
			s = at;
			want_at.push_back(at);
			want_d1.push_back(d1_stop);
			if (why != ALL) {
				want_count = i;
				stop = why;
				continue;
			}
			held |= risk && in_d1;
			want_A.push_back(want_bytes);
			want_bytes += sx.out_len;
			plain_advance(s, sx.out_len);
		}
		std::vector<int64_t> A(nb, -1);
		RoundState rs{ s0.pos, s0.hist };
		uint32_t seen_n = 0;
		const Accepted a = accept_blocks(d, stx, stz, rs, A.data(), [&](uint32_t i, const RoundState& at, bool d1_bad) {
			if (i != seen_n++ || i >= want_at.size())
				fail("accept_blocks: looks at every block up to the stopping one, once, in order", c);
			if (at.pos != want_at[i].pos || at.history != want_at[i].hist || d1_bad != want_d1[i])
				fail("accept_blocks: a block's state at its start and its D1 verdict", c);
		});
		if (a.count != want_count || a.bytes != want_bytes)
			fail("accept_blocks: count and bytes", c);
		if (seen_n != want_at.size())
			fail("accept_blocks: looks at the stopping block", c);
		for (uint32_t i = 0; i < nb; ++i)
			if (A[i] != (i < want_count ? want_A[i] : -1))
				fail("accept_blocks: A[] holds the accepted blocks' starts, nothing after", c);
		if (rs.pos != s.pos || rs.history != s.hist)
			fail("accept_blocks: the state after the accepted blocks", c);
		++counts[stop];
		counts[HELD] += held;
		counts[STOP_AT_0] += want_count == 0;

		// ---- plane modes of the accepted blocks
		std::vector<uint8_t> mode(nb, 9);
		const PlaneCounts pc = plane_modes(stz, a.count, mode.data());
		uint32_t ny = 0, nh = 0;
		for (uint32_t i = 0; i < nb; ++i) {
			const uint8_t want = i >= a.count ? 9 : stz[i].code != 0 ? 2 : (stz[i].aux & 2) ? 1 : 0;
			if (mode[i] != want)
				fail("plane_modes: a block's mode", c);
			ny += want == 1 || want == 2;
			nh += want == 2;
		}
		if (pc.ny != ny || pc.nh != nh)
			fail("plane_modes: ny and nh", c);
	}
	for (int o = 0; o < N_OUT; ++o)
		printf("%-48s %ld\n", OUT_NAME[o], counts[o]);
	for (int o = 0; o < N_OUT; ++o)
		if (!counts[o]) {
			printf("FAIL: no case reached: %s\n", OUT_NAME[o]);
			return 1;
		}
	printf("%ld batches: no sanitizer report, every stage as restated\n", CASES);
	return 0;
}
