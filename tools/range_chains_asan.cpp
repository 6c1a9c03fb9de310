// range_chains_asan.cpp -- the chain rule of the ranged decode of linked
// frames (csrc/lz4ada_range_chains.h: range_chains, what
// lz4ada_range_chains_host runs, over ChainSweep and the chain_* functions the
// kernels share) under AddressSanitizer and UBSan, host code only, against the
// brute-force definition: every frame of nb = 1 .. 9 blocks, every group size
// K = 1 .. 4 and every set of up to three touched intervals [a, z] of the
// frame.  The definition: a range marks floor(a / K) * K .. z; a marked block
// b > 0 with b % K == 0 is a head; the chains are the maximal runs of marked
// blocks, cut in front of every head.  Also per set: chain_heads against a
// count, chain_checkpoints, and that every chain begins at a group start.  All
// arrays are heap arrays of exactly the size the call may touch, so a read or
// write of one entry outside them stops the run.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibo-lz4-ada_amd/csrc tools/range_chains_asan.cpp -o tools/_build/range_chains_asan
//   tools/_build/range_chains_asan > profiles/range_chains_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "lz4ada_range_chains.h"

using namespace lz4ada;

template <class T>
static T* exact(size_t n)
{
	return static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
}

int main()
{
	long total = 0;
	bool ok = true;
	for (int nb = 1; nb <= 9; ++nb) {
		// the intervals of the frame
		int ia[45], iz[45], ni = 0;
		for (int a = 0; a < nb; ++a)
			for (int z = a; z < nb; ++z) {
				ia[ni] = a;
				iz[ni] = z;
				++ni;
			}
		for (int K = 1; K <= 4; ++K) {
			long sets = 0, bad = 0, chains = 0;
			for (int n = 0; n <= 3; ++n) {
				int pick[3] = { 0, 1, 2 };  // a combination of n intervals
				for (;;) {
					if (n > ni)
						break;
					int64_t* first = exact<int64_t>(size_t(n));
					int64_t* count = exact<int64_t>(size_t(n));
					for (int i = 0; i < n; ++i) {  // in falling order: the call sorts for itself
						first[n - 1 - i] = ia[pick[i]];
						count[n - 1 - i] = iz[pick[i]] - ia[pick[i]] + 1;
					}
					uint8_t* marked = exact<uint8_t>(size_t(nb));
					uint8_t* head = exact<uint8_t>(size_t(nb));
					int64_t* cf = exact<int64_t>(size_t(nb));
					int64_t* cc = exact<int64_t>(size_t(nb));
					const int64_t nc = range_chains(uint64_t(nb), uint64_t(K), first, count, n, marked, head, cf, cc);
					// the definition
					bool m[9], h[9];
					for (int b = 0; b < nb; ++b) {
						m[b] = false;
						for (int i = 0; i < n; ++i)
							m[b] |= b >= ia[pick[i]] / K * K && b <= iz[pick[i]];
						h[b] = m[b] && b > 0 && b % K == 0;
					}
					int64_t wf[9], wc[9], wn = 0;
					for (int b = 0; b < nb; ++b) {
						if (!m[b])
							continue;
						if (h[b] || b == 0 || !m[b - 1]) {
							wf[wn] = b;
							wc[wn] = 1;
							++wn;
						} else {
							++wc[wn - 1];
						}
					}
					bool same = nc == wn;
					uint64_t nheads = 0;
					for (int b = 0; b < nb; ++b) {
						same &= (marked[b] != 0) == m[b] && (head[b] != 0) == h[b];
						nheads += h[b];
					}
					for (int64_t c = 0; same && c < nc; ++c)
						same &= cf[c] == wf[c] && cc[c] == wc[c] && cf[c] % K == 0 &&
						        uint64_t(cf[c] + cc[c]) <= chain_group_end(uint64_t(K), uint64_t(nb), uint64_t(cf[c]));
					// the heads of a marked run [lo, hi), as the host's sweep charges their gaps
					for (int lo = 0; lo < nb; ++lo)
						for (int hi = lo; hi <= nb; ++hi) {
							uint64_t want = 0;
							for (int b = lo; b < hi; ++b)
								want += b > 0 && b % K == 0;
							same &= chain_heads(uint64_t(K), uint64_t(lo), uint64_t(hi)) == want;
						}
					uint64_t ck = 0;
					for (int b = K; b < nb; b += K)
						++ck;
					same &= chain_checkpoints(uint64_t(K), uint64_t(nb)) == ck && nheads <= ck;
					bad += !same;
					chains += nc;
					++sets;
					free(first);
					free(count);
					free(marked);
					free(head);
					free(cf);
					free(cc);
					// the next combination
					int i = n - 1;
					while (i >= 0 && pick[i] == ni - n + i)
						--i;
					if (i < 0)
						break;
					++pick[i];
					for (int j = i + 1; j < n; ++j)
						pick[j] = pick[j - 1] + 1;
				}
			}
			printf("%d blocks K %d %6ld sets of intervals %8ld chains  wrong %ld  %s\n", nb, K, sets, chains, bad,
			       bad ? "FAIL" : "pass");
			ok &= bad == 0;
			total += sets;
		}
	}
	// the block maximum from a frame's block count and size, and K from it
	long bm_bad = 0;
	const uint64_t maxes[4] = { 64u << 10, 256u << 10, 1u << 20, 4u << 20 };
	for (uint64_t bm : maxes)
		for (uint64_t nb = 2; nb <= 40; ++nb)
			for (uint64_t last : { uint64_t(0), uint64_t(1), bm - 1, bm })
				bm_bad += chain_block_max(nb, (nb - 1) * bm + last) != bm;
	bm_bad += chain_group(0, 65536) != 1 || chain_group(65536, 65536) != 1 || chain_group(65537, 65536) != 2 ||
	          chain_group(1 << 20, 4 << 20) != 1 || chain_group(1 << 20, 65536) != 16;
	printf("block maximum and group size: wrong %ld  %s\n", bm_bad, bm_bad ? "FAIL" : "pass");
	ok &= bm_bad == 0;
	printf("total %ld sets -- %s\n", total,
	       ok ? "no sanitizer report, every marked set, head and chain is the brute-force one" : "FAILED");
	return ok ? 0 : 1;
}
