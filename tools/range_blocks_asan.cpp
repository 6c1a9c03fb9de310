// range_blocks_asan.cpp -- the block search of the ranged decode
// (csrc/lz4ada_range_blocks.h) under AddressSanitizer and UBSan, host code
// only, against a brute-force definition: every start[] built from 0 to 5
// blocks of the sizes {0, 1, 2, 255, 256, 257}, every off in 0 .. size + 2 and
// every len in {0, 1, 2, size, size + 1}.  start[] is a heap array of exactly
// nb + 1 entries, so a read of one entry outside it stops the run.  A block is
// touched when it shares a byte with the clipped range; the selected interval
// must begin and end with a touched block and be empty exactly when the
// clipped length is 0.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibo-lz4-ada_amd/csrc tools/range_blocks_asan.cpp -o tools/_build/range_blocks_asan
//   tools/_build/range_blocks_asan > profiles/range_blocks_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "lz4ada_range_blocks.h"

using namespace lz4ada;

static const uint64_t SIZES[6] = { 0, 1, 2, 255, 256, 257 };

int main()
{
	long total = 0, empty_total = 0;
	bool ok = true;
	for (int nb = 0; nb <= 5; ++nb) {
		long arrays = 0, calls = 0, empty = 0, bad = 0;
		int pick[5] = { 0, 0, 0, 0, 0 };
		for (;;) {
			uint64_t* start = static_cast<uint64_t*>(malloc(size_t(nb + 1) * sizeof(uint64_t)));
			start[0] = 0;
			for (int b = 0; b < nb; ++b)
				start[b + 1] = start[b] + SIZES[pick[b]];
			const uint64_t size = start[nb];
			const uint64_t lens[5] = { 0, 1, 2, size, size + 1 };
			++arrays;
			for (uint64_t off = 0; off <= size + 2; ++off)
				for (uint64_t len : lens) {
					const RangeBlocks r = range_blocks(start, uint64_t(nb), off, len);
					// the definition: the clipped range, and the blocks that share a byte with it
					const uint64_t end = off + len < size ? off + len : size, want = end > off ? end - off : 0;
					int64_t lo = -1, hi = -1;
					for (int b = 0; b < nb; ++b)
						if (want > 0 && start[b + 1] > start[b] && start[b] < off + want && start[b + 1] > off) {
							lo = lo < 0 ? b : lo;
							hi = b;
						}
					const bool same = want == 0 ? (r.count == 0 && r.first == 0 && lo < 0)
					                            : (lo >= 0 && r.first == uint64_t(lo) &&
					                               r.count == uint64_t(hi - lo + 1));
					if (range_clip(size, off, len) != want || !same)
						++bad;
					++calls;
					empty += r.count == 0;
				}
			free(start);
			int b = 0;
			while (b < nb && ++pick[b] == 6)
				pick[b++] = 0;
			if (b == nb)
				break;
		}
		printf("%d blocks %6ld start arrays %10ld ranges  empty %9ld  wrong %ld  %s\n", nb, arrays, calls, empty, bad,
		       bad ? "FAIL" : "pass");
		ok &= bad == 0;
		total += calls;
		empty_total += empty;
	}
	printf("total %ld ranges, %ld empty -- %s\n", total, empty_total,
	       ok ? "no sanitizer report, every interval is the brute-force one" : "FAILED");
	return ok ? 0 : 1;
}
