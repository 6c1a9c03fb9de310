// pass_runs_check.cpp -- pass_runs (lz4ada_pass_runs.h) against
// its definition, under AddressSanitizer and UBSan, host code only: every
// sequence of up to 8 frames, each blockless, independent with 1 or 3 blocks
// or linked with 1 or 3 blocks.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan
//       -fno-sanitize-recover=all -Ibo-lz4-ada_amd/csrc tools/pass_runs_check.cpp -o tools/_build/pass_runs_check
#include <cstdio>

#include "lz4ada_pass_runs.h"

using namespace lz4ada;

static const PassFrame KINDS[5] = { { 0, false }, { 1, false }, { 3, false }, { 1, true }, { 3, true } };

// The kind of the first frame with blocks in [f0, f1): 0 independent, 1 linked,
// -1 none; *at gets its position.
static int first_kind(const std::vector<PassFrame>& fr, uint32_t f0, uint32_t f1, uint32_t* at)
{
	for (uint32_t k = f0; k < f1; ++k)
		if (fr[k].nblocks) {
			*at = k;
			return int(fr[k].linked);
		}
	return -1;
}

// nullptr, or the rule the runs break.
static const char* check(const std::vector<PassFrame>& fr, const std::vector<PassRun>& runs)
{
	const uint32_t nf = uint32_t(fr.size());
	std::vector<uint32_t> prefix(nf + 1, 0);
	for (uint32_t k = 0; k < nf; ++k)
		prefix[k + 1] = prefix[k] + fr[k].nblocks;
	if (nf == 0)
		return runs.empty() ? nullptr : "no frames give no run";
	if (runs.empty() || runs.front().f0 != 0 || runs.back().f1 != nf)
		return "the runs cover [0, nf)";
	if (prefix[nf] == 0 && (runs.size() != 1 || runs[0].b0 != runs[0].b1))
		return "blockless frames alone give one run with b0 == b1";
	for (size_t i = 0; i < runs.size(); ++i) {
		const PassRun& r = runs[i];
		if (r.f0 >= r.f1 || r.f1 > nf || (i && r.f0 != runs[i - 1].f1))
			return "the runs tile the frames in order, without gaps";
		if (r.b0 != prefix[r.f0] || r.b1 != prefix[r.f1])
			return "b0 / b1 are the prefix sums at f0 / f1";
		for (uint32_t k = r.f0; k < r.f1; ++k)
			if (fr[k].nblocks && fr[k].linked != r.linked)
				return "every frame with blocks has its run's kind";
		uint32_t at = 0;
		const int kind = first_kind(fr, r.f0, r.f1, &at);
		if (kind < 0 && r.linked)
			return "a run without blocks is not linked";
		if (i && (kind < 0 || at != r.f0 || (kind == 1) == runs[i - 1].linked))
			return "a later run starts at a frame with blocks of the other kind";
	}
	return nullptr;
}

int main()
{
	long cases = 0;
	for (uint32_t nf = 0; nf <= 8; ++nf) {
		uint32_t count = 1;
		for (uint32_t i = 0; i < nf; ++i)
			count *= 5;
		for (uint32_t code = 0; code < count; ++code, ++cases) {
			std::vector<PassFrame> fr;
			for (uint32_t i = 0, c = code; i < nf; ++i, c /= 5)
				fr.push_back(KINDS[c % 5]);
			if (const char* rule = check(fr, pass_runs(fr))) {
				printf("FAIL: %s (nf %u, code %u)\n", rule, nf, code);
				return 1;
			}
		}
	}
	printf("%ld sequences: no sanitizer report, every run as defined\n", cases);
	return 0;
}
