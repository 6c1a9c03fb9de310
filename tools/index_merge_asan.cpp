// index_merge_asan.cpp -- the merge rule of lz4ada_seek_index_concat
// (csrc/lz4ada_index_merge.h: merge_validate, merge_plan, merge_part_of; what
// the host sums by, the k_index_merge_* kernels look parts up with and
// lz4ada_index_merge_plan_host states) under AddressSanitizer and UBSan, host
// code only.  Part lists from a generator -- runs of parts without jobs at the
// front, in the middle and at the end, parts with frames and no block, one
// part, 300 parts -- are planned, every prefix is compared with a running sum,
// and for every merged element of the four counted kinds the part is compared
// with a linear scan.  Then a merge is replayed as the kernels do it: every
// part's arrays (first, the start words, a checkpoint tag per checkpoint) are
// heap blocks of exactly the entries the part holds, the result's are blocks
// of exactly the summed counts, and every element is fetched from
// part[merge_part_of(...)] at i - prefix[part]; a part chosen wrongly where
// prefixes repeat reads or writes outside a block and stops the run.  The
// validation is run over lists that break each of its rules.  No GPU, no
// library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/index_merge_asan.cpp -o tools/_build/index_merge_asan
//   tools/_build/index_merge_asan > profiles/index_merge_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lz4ada_index_merge.h"

using namespace lz4ada;

static uint64_t rng = 88172645463325252ull;
static uint32_t next()
{
	rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
	return uint32_t(rng >> 16);
}

static long lists = 0, parts_seen = 0, elements = 0, repeats = 0;

// A part's own arrays, each of exactly its entries.
struct Part {
	std::unique_ptr<uint64_t[]> first;  // n + 1
	std::unique_ptr<uint64_t[]> words;  // nb + n
	std::unique_ptr<uint64_t[]> ckpt;   // nck tags
};

static bool one(int64_t nparts, int mode)
{
	std::unique_ptr<MergePart[]> shape(new MergePart[size_t(nparts)]);
	std::unique_ptr<int64_t[]> base(new int64_t[size_t(nparts)]);
	std::unique_ptr<Part[]> part(new Part[size_t(nparts)]);
	int64_t at = int64_t(next() % 7);
	for (int64_t p = 0; p < nparts; ++p) {
		MergePart& m = shape[size_t(p)];
		const uint32_t roll = next() % 10;
		const bool run = nparts > 8 && (p < 3 || p >= nparts - 2 || (p >= nparts / 2 && p < nparts / 2 + 3));
		m = MergePart{ 0, 0, 0, int64_t(next() % 50), 0 };
		if (mode == 1 || (mode == 0 && !run && roll >= 3)) {
			m.n = 1 + int64_t(next() % 8);
			m.in_len = 15 * m.n;
			if (mode == 1 || roll >= 5) {
				m.nb = 1 + int64_t(next() % 40);
				m.nck = roll >= 7 ? int64_t(next() % uint32_t(m.nb)) : 0;
				m.in_len += int64_t(next() % 100000);
				m.slots = 256 * (m.nb + int64_t(next() % 1000));
			}
		}
		at += int64_t(next() % 3) * int64_t(next() % 5000);
		base[size_t(p)] = at;
		at += m.in_len;
		Part& q = part[size_t(p)];
		q.first.reset(new uint64_t[size_t(m.n) + 1]);
		q.words.reset(new uint64_t[size_t(m.nb + m.n)]);
		q.ckpt.reset(new uint64_t[size_t(m.nck)]);
		// the blocks dealt over the frames, some frames without any
		uint64_t b = 0;
		for (int64_t k = 0; k < m.n; ++k) {
			q.first[size_t(k)] = b;
			const uint64_t left = uint64_t(m.nb) - b;
			b += k == m.n - 1 ? left : (left ? next() % (left + 1) : 0);
		}
		q.first[size_t(m.n)] = uint64_t(m.nb);
		for (int64_t w = 0; w < m.nb + m.n; ++w)
			q.words[size_t(w)] = (uint64_t(p) << 32) | uint64_t(w);
		for (int64_t c = 0; c < m.nck; ++c)
			q.ckpt[size_t(c)] = (uint64_t(p) << 32) | uint64_t(c) | (uint64_t(1) << 63);
	}
	int64_t bad = 0;
	if (merge_validate(shape.get(), base.get(), nparts, at, &bad) != MERGE_OK)
		return false;
	const size_t stride = size_t(nparts) + 1;
	std::unique_ptr<uint64_t[]> pre(new uint64_t[MERGE_PREFIXES * stride]);
	if (!merge_plan(shape.get(), nparts, pre.get()))
		return false;
	bool ok = true;
	uint64_t sum[MERGE_PREFIXES] = { 0, 0, 0, 0, 0 };
	for (int64_t p = 0; p <= nparts; ++p) {
		for (int k = 0; k < MERGE_PREFIXES; ++k)
			ok = ok && pre[size_t(k) * stride + size_t(p)] == sum[k];
		if (p == nparts)
			break;
		const MergePart& m = shape[size_t(p)];
		sum[MERGE_FRAMES] += uint64_t(m.n);
		sum[MERGE_BLOCKS] += uint64_t(m.nb);
		sum[MERGE_WORDS] += uint64_t(m.nb + m.n);
		sum[MERGE_CKPTS] += uint64_t(m.nck);
		sum[MERGE_SLOTS] += uint64_t(m.slots);
		for (int k = 0; k < MERGE_PREFIXES - 1; ++k)
			repeats += pre[size_t(k) * stride + size_t(p)] == sum[k];
	}
	// the part of every element, against a linear scan
	for (int k = 0; k < MERGE_PREFIXES - 1; ++k) {
		const uint64_t* const a = pre.get() + size_t(k) * stride;
		uint64_t lin = 0;
		for (uint64_t i = 0; i < a[nparts]; ++i) {
			while (a[lin + 1] <= i)
				++lin;
			ok = ok && merge_part_of(a, uint64_t(nparts), i) == lin;
			++elements;
		}
	}
	// the merge as the kernels run it, into blocks of exactly the summed counts
	const uint64_t *const pf = pre.get(), *const pb = pre.get() + stride, *const pw = pre.get() + 2 * stride,
	               *const pc = pre.get() + 3 * stride;
	const uint64_t n = pf[nparts], nb = pb[nparts], nck = pc[nparts];
	std::unique_ptr<uint64_t[]> first(new uint64_t[size_t(n) + 1]), words(new uint64_t[size_t(nb + n)]),
	    ckpt(new uint64_t[size_t(nck)]);
	for (uint64_t f = 0; f < n; ++f) {
		const uint64_t p = merge_part_of(pf, uint64_t(nparts), f);
		first[size_t(f)] = part[size_t(p)].first[size_t(f - pf[p])] + pb[p];
	}
	first[size_t(n)] = nb;
	for (uint64_t w = 0; w < nb + n; ++w) {
		const uint64_t p = merge_part_of(pw, uint64_t(nparts), w);
		words[size_t(w)] = part[size_t(p)].words[size_t(w - pw[p])];
	}
	for (uint64_t c = 0; c < nck; ++c) {
		const uint64_t p = merge_part_of(pc, uint64_t(nparts), c);
		ckpt[size_t(c)] = part[size_t(p)].ckpt[size_t(c - pc[p])];
	}
	// what a reader of the result finds: frame f's words begin at first[f] + f
	uint64_t f = 0, c = 0;
	for (int64_t p = 0; p < nparts; ++p) {
		const MergePart& m = shape[size_t(p)];
		for (int64_t k = 0; k < m.n; ++k, ++f) {
			const uint64_t lo = part[size_t(p)].first[size_t(k)], hi = part[size_t(p)].first[size_t(k) + 1];
			ok = ok && first[size_t(f)] == pb[p] + lo && first[size_t(f) + 1] >= first[size_t(f)];
			for (uint64_t i = 0; i <= hi - lo; ++i)
				ok = ok && words[size_t(first[size_t(f)] + f + i)] == ((uint64_t(p) << 32) | (lo + uint64_t(k) + i));
		}
		for (int64_t k = 0; k < m.nck; ++k, ++c)
			ok = ok && ckpt[size_t(c)] == ((uint64_t(p) << 32) | uint64_t(k) | (uint64_t(1) << 63));
	}
	ok = ok && f == n && c == nck;
	++lists;
	parts_seen += long(nparts);
	return ok;
}

static bool faults()
{
	const MergePart a{ 3, 5, 2, 1000, 1280 }, e{ 0, 0, 0, 10, 0 }, neg{ -1, 0, 0, 10, 0 };
	int64_t at = 0;
	bool ok = true;
	auto is = [&](const MergePart* m, const int64_t* b, int64_t np, int64_t len, MergeFault want) {
		ok = ok && merge_validate(m, b, np, len, &at) == want;
	};
	std::unique_ptr<MergePart[]> two(new MergePart[2]{ a, a }), ea(new MergePart[2]{ e, a }), bad(new MergePart[1]{ neg });
	std::unique_ptr<int64_t[]> b(new int64_t[2]{ 0, 1000 });
	is(two.get(), b.get(), 2, 2000, MERGE_OK);
	is(two.get(), b.get(), 2, 1999, MERGE_PAST_END);
	is(two.get(), b.get(), -1, 2000, MERGE_NEGATIVE_COUNT);
	is(two.get(), b.get(), 2, -1, MERGE_NEGATIVE_COUNT);
	is(nullptr, b.get(), 2, 2000, MERGE_NULL_ARRAY);
	is(two.get(), nullptr, 2, 2000, MERGE_NULL_ARRAY);
	is(nullptr, nullptr, 0, 0, MERGE_OK);
	b[1] = 999;
	is(two.get(), b.get(), 2, 2000, MERGE_NOT_RISING);
	b[0] = -1;
	is(two.get(), b.get(), 2, 2000, MERGE_NEGATIVE_BASE);
	b[0] = 5, b[1] = 14;
	is(ea.get(), b.get(), 2, 2000, MERGE_NOT_RISING);
	b[1] = 15;
	is(ea.get(), b.get(), 2, 2000, MERGE_OK);
	b[0] = INT64_MAX - 3;
	is(ea.get(), b.get(), 1, INT64_MAX, MERGE_PAST_END);
	b[0] = 0;
	is(bad.get(), b.get(), 1, 100, MERGE_BAD_PART);
	// 2^31 jobs or blocks in all
	std::unique_ptr<MergePart[]> big(new MergePart[2]{ { int64_t(1) << 30, 1, 0, 0, 0 }, { int64_t(1) << 30, 1, 0, 0, 0 } });
	std::unique_ptr<uint64_t[]> pre(new uint64_t[MERGE_PREFIXES * 3]);
	ok = ok && merge_plan(big.get(), 1, pre.get()) && !merge_plan(big.get(), 2, pre.get());
	big[0] = big[1] = MergePart{ 1, (int64_t(1) << 30) + 1, 0, 0, 0 };
	ok = ok && merge_plan(big.get(), 1, pre.get()) && !merge_plan(big.get(), 2, pre.get());
	return ok;
}

int main()
{
	bool ok = faults();
	printf("validation and limits: %s\n", ok ? "every rule names its fault" : "MISMATCH");
	const int64_t counts[] = { 1, 2, 3, 7, 31, 300 };
	for (int64_t nparts : counts) {
		const long before = lists, el = elements, rp = repeats;
		for (int round = 0; round < (nparts == 300 ? 6 : 40); ++round)
			for (int mode = 0; mode < 3; ++mode)  // mixed, every part with blocks, every part empty
				if (!one(nparts, mode)) {
					printf("MISMATCH %lld parts, round %d, mode %d\n", (long long)nparts, round, mode);
					ok = false;
				}
		printf("%lld parts: %ld lists, %ld elements looked up, %ld repeated prefix entries\n", (long long)nparts,
		       lists - before, elements - el, repeats - rp);
	}
	printf("total %ld lists, %ld parts, %ld elements -- %s\n", lists, parts_seen, elements,
	       ok ? "no sanitizer report, every element found in the part that holds it" : "MISMATCH");
	return ok ? 0 : 1;
}
