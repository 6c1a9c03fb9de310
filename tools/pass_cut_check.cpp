// pass_cut_check.cpp -- pass_cut (lz4ada_pass_runs.h) against a
// brute-force statement of its rules, under AddressSanitizer and UBSan, host
// code only: every sequence of up to 6 frames, each not taken or taken with 1 or
// 3 blocks at a cost below, equal to or above the budget, cut from every start;
// and block counts that reach 2^31.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan
//       -fno-sanitize-recover=all -Ibo-lz4-ada_amd/csrc tools/pass_cut_check.cpp -o tools/_build/pass_cut_check
#include <cstdio>

#include "lz4ada_pass_runs.h"

using namespace lz4ada;

static const uint64_t BUDGET = 10, END = uint64_t(1) << 31;
static const PassCost KINDS[7] = { { false, 11, 3 }, { true, 4, 1 },  { true, 10, 1 }, { true, 11, 1 },
	                           { true, 4, 3 },   { true, 10, 3 }, { true, 11, 3 } };

// The rules, each sum taken anew: [lo, h) is a pass when every taken frame in it
// leaves the blocks so far below 2^31 and either has no byte before it or keeps
// the bytes so far within the budget.  A frame that is not taken asks nothing.
static bool is_pass(const std::vector<PassCost>& fr, size_t lo, size_t h)
{
	for (size_t j = lo; j < h; ++j) {
		if (!fr[j].taken)
			continue;
		uint64_t before = 0, blocks = 0;
		for (size_t i = lo; i <= j; ++i)
			if (fr[i].taken) {
				before += i < j ? fr[i].bytes : 0;
				blocks += fr[i].blocks;
			}
		if (blocks >= END || (before && before + fr[j].bytes > BUDGET))
			return false;
	}
	return true;
}

// nullptr, or what the cut from lo gets wrong: it is the longest pass.
static const char* check(const std::vector<PassCost>& fr, size_t lo)
{
	const PassCut c = pass_cut(lo, fr.size(), BUDGET, [&](size_t k) { return fr[k]; });
	size_t hi = fr.size();
	while (!is_pass(fr, lo, hi))
		--hi;  // ([lo, lo) is a pass)
	if (c.hi != hi)
		return "hi ends the longest pass from lo";
	uint64_t bytes = 0, blocks = 0;
	for (size_t k = lo; k < hi; ++k)
		if (fr[k].taken) {
			bytes += fr[k].bytes;
			blocks += fr[k].blocks;
		}
	if (c.bytes != bytes || c.blocks != blocks)
		return "bytes and blocks are the taken frames' sums";
	return nullptr;
}

int main()
{
	long cases = 0;
	for (uint32_t nf = 0; nf <= 6; ++nf) {
		uint32_t count = 1;
		for (uint32_t i = 0; i < nf; ++i)
			count *= 7;
		for (uint32_t code = 0; code < count; ++code, ++cases) {
			std::vector<PassCost> fr;
			for (uint32_t i = 0, c = code; i < nf; ++i, c /= 7)
				fr.push_back(KINDS[c % 7]);
			for (size_t lo = 0; lo <= nf; ++lo)
				if (const char* rule = check(fr, lo)) {
					printf("FAIL: %s (nf %u, code %u, lo %zu)\n", rule, nf, code, lo);
					return 1;
				}
		}
	}
	// a pass holds fewer than 2^31 blocks: one short of it fits, the block that
	// reaches it does not, and a frame that holds as many alone gives hi == lo,
	// also behind a frame that is not taken
	const std::vector<PassCost> big[4] = { { { true, 1, END - 2 }, { true, 1, 1 }, { true, 1, 1 } },
		                               { { true, 1, END - 1 }, { false, 1, 1 }, { true, 1, 1 } },
		                               { { true, 1, END }, { true, 1, 1 } },
		                               { { false, 1, 1 }, { true, 20, END }, { true, 1, 1 } } };
	const size_t big_hi[4] = { 2, 2, 0, 1 };
	for (int i = 0; i < 4; ++i, ++cases) {
		const char* rule = check(big[i], 0);
		if (!rule && pass_cut(0, big[i].size(), BUDGET, [&](size_t k) { return big[i][k]; }).hi != big_hi[i])
			rule = "a pass holds fewer than 2^31 blocks";
		if (rule) {
			printf("FAIL: %s (large case %d)\n", rule, i);
			return 1;
		}
	}
	printf("%ld sequences: no sanitizer report, every cut as the rules state\n", cases);
	return 0;
}
