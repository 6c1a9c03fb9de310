// range_gaps_asan.cpp -- the gap count of the ranged decode over a dictionary
// index (csrc/lz4ada_range_chains.h: chain_dict_gapped, chain_dict_gaps beside
// chain_heads, what lz4ada_range_gaps_host runs and the kernels and the host's
// sweep share) under AddressSanitizer and UBSan, host code only, against the
// brute-force definition: every frame of nb = 1 .. 9 blocks, every group size
// K = 0 .. 4, all three frame kinds and every interval [lo, hi) of the frame.
// The definition: a block b > 0 with b % K == 0 has a checkpoint's gap; the
// dictionary's gap lies in front of every block of an independent modern frame
// and of block 0 of a linked one.  Also, as the host's sweep (plan_pass)
// charges a pass: for every set of up to three touched intervals the gaps of
// what ChainSweep::add returns add up to the gaps of the marked set counted
// block by block, and no block of a consistent frame takes both gaps.  The
// mark arrays are heap arrays of exactly nb entries, so a read or write of one
// entry outside them stops the run.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibo-lz4-ada_amd/csrc tools/range_gaps_asan.cpp -o tools/_build/range_gaps_asan
//   tools/_build/range_gaps_asan > profiles/range_gaps_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "lz4ada_range_chains.h"

using namespace lz4ada;

static bool def_head(int K, int b) { return K && b > 0 && b % K == 0; }
static bool def_gapped(uint32_t kind, int b) { return kind == CHAIN_KIND_INDEP || (kind == CHAIN_KIND_LINKED && b == 0); }

int main()
{
	bool ok = true;
	long total = 0;
	const uint32_t kinds[3] = { CHAIN_KIND_NONE, CHAIN_KIND_LINKED, CHAIN_KIND_INDEP };
	for (int nb = 1; nb <= 9; ++nb) {
		for (int K = 0; K <= 4; ++K) {
			for (uint32_t kind : kinds) {
				long bad = 0, intervals = 0, sets = 0;
				for (int lo = 0; lo <= nb; ++lo)
					for (int hi = lo; hi <= nb; ++hi) {
						uint64_t heads = 0, gaps = 0;
						for (int b = lo; b < hi; ++b) {
							heads += def_head(K, b);
							gaps += def_gapped(kind, b);
							bad += chain_dict_gapped(kind, uint64_t(b)) != def_gapped(kind, b);
							bad += chain_head(uint64_t(K), uint64_t(b)) != def_head(K, b);
						}
						bad += chain_heads(uint64_t(K), uint64_t(lo), uint64_t(hi)) != heads;
						bad += chain_dict_gaps(kind, uint64_t(lo), uint64_t(hi)) != gaps;
						++intervals;
					}
				// a frame's kind and its K agree in an index: linked <=> K != 0
				const bool consistent = (kind == CHAIN_KIND_LINKED) == (K != 0);
				if (consistent) {
					// the sweep over up to three touched intervals [a, z], in rising a
					int ia[45], iz[45], ni = 0;
					for (int a = 0; a < nb; ++a)
						for (int z = a; z < nb; ++z) {
							ia[ni] = a;
							iz[ni] = z;
							++ni;
						}
					for (int i = 0; i < ni; ++i)
						for (int j = i; j < ni; ++j)
							for (int k = j; k < ni; ++k) {
								uint8_t* marked = static_cast<uint8_t*>(calloc(size_t(nb), 1));
								ChainSweep sweep{ uint64_t(K) };
								uint64_t heads = 0, gaps = 0;
								for (int r : { i, j, k }) {  // (i <= j <= k: rising first block)
									const ChainSweep::Added a = sweep.add(uint64_t(ia[r]), uint64_t(iz[r]));
									heads += chain_heads(uint64_t(K), a.lo, a.hi);
									gaps += chain_dict_gaps(kind, a.lo, a.hi);
									for (uint64_t b = a.lo; b < a.hi; ++b) {
										bad += marked[b] != 0;  // the sweep returns a block once
										marked[b] = 1;
									}
								}
								uint64_t wh = 0, wg = 0;
								for (int b = 0; b < nb; ++b) {
									bool m = false;
									for (int r : { i, j, k })
										m |= b >= int(chain_start(uint64_t(K), uint64_t(ia[r]))) && b <= iz[r];
									bad += m != (marked[b] != 0);
									wh += m && def_head(K, b);
									wg += m && def_gapped(kind, b);
									bad += def_head(K, b) && def_gapped(kind, b);  // never both gaps
								}
								bad += wh != heads || wg != gaps;
								free(marked);
								++sets;
							}
				}
				printf("%d blocks K %d kind %u %4ld intervals %7ld sets of intervals  wrong %ld  %s\n", nb, K, kind,
				       intervals, sets, bad, bad ? "FAIL" : "pass");
				ok &= bad == 0;
				total += intervals + sets;
			}
		}
	}
	printf("total %ld cases -- %s\n", total,
	       ok ? "no sanitizer report, every gap count is the brute-force one" : "FAILED");
	return ok ? 0 : 1;
}
