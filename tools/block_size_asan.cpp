// block_size_asan.cpp -- the size rule (csrc/lz4ada_block_size.h) under
// AddressSanitizer and UBSan, host code only: every block of the golden .lz4
// files given on the command line, every truncation of three of them and
// every single-bit flip of the first 64 bytes of two, each copied into a heap
// block of exactly its length, so a read of one byte outside [p, p + n) stops
// the run.  The frames are found with the frame walk (csrc/lz4ada_frame_walk.h);
// a frame that declares its content size must add up to it.  No GPU, no library:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/block_size_asan.cpp -o tools/_build/block_size_asan
//   tools/_build/block_size_asan tests/golden/vectors/*.lz4 tests/golden/lz4f/*.lz4
//       > profiles/block_size_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lz4ada_block_size.h"
#include "lz4ada_frame_walk.h"

using namespace lz4ada;
using Bytes = std::vector<uint8_t>;

// block_decoded_size over an exact-size heap copy of [p, p + n)
static int64_t sized(const uint8_t* p, size_t n, bool stored)
{
	uint8_t* q = static_cast<uint8_t*>(malloc(n ? n : 1));
	if (n)
		memcpy(q, p, n);
	const int64_t s = block_decoded_size(n ? q : q + 1, int64_t(n), stored);  // n = 0: no byte is the block's
	free(q);
	return s;
}

struct Tally {
	long calls = 0, known = 0, unknown = 0;
	void add(int64_t s)
	{
		++calls;
		++(s >= 0 ? known : unknown);
	}
};

int main(int argc, char** argv)
{
	bool ok = true;
	Tally all;
	std::vector<Bytes> kept;  // compressed blocks for the truncations and the flips
	for (int a = 1; a < argc; ++a) {
		FILE* fh = fopen(argv[a], "rb");
		if (!fh) {
			printf("%s: cannot open\n", argv[a]);
			return 1;
		}
		Bytes f;
		uint8_t buf[65536];
		for (size_t n; (n = fread(buf, 1, sizeof buf, fh)) > 0;)
			f.insert(f.end(), buf, buf + n);
		fclose(fh);
		Tally t;
		long frames = 0, declared = 0;
		bool file_ok = true;
		for (size_t at = 0; at < f.size();) {
			lz4ada_frame_info info;
			WalkSums sums;
			// linked frames and large blocks count too: the verdict only says which pass takes them
			if (frame_walk(f.data() + at, int64_t(f.size() - at), true, &info, &sums, nullptr, true, UINT64_MAX) ==
			        LZ4ADA_BATCH_NOT_INDEXED || info.frame_len <= 0)
				break;
			std::vector<lz4ada_block_desc> d(size_t(info.nblocks) + 1);
			WalkEmit e{};
			e.descs = d.data();
			e.cap = info.nblocks;
			frame_walk(f.data() + at, int64_t(f.size() - at), true, &info, &sums, &e, true, UINT64_MAX);
			uint64_t sum = 0;
			for (int64_t k = 0; k < e.written; ++k) {
				const bool stored = (d[k].flags & LZ4ADA_BLOCK_STORED) != 0;
				const uint8_t* p = f.data() + at + d[k].in_off;
				const int64_t s = sized(p, d[k].in_len, stored);
				t.add(s);
				if (s < 0)
					file_ok = false;  // a golden block is never unknown
				else
					sum += uint64_t(s);
				if (!stored && d[k].in_len >= 200 && d[k].in_len <= 6000 && kept.size() < 3)
					kept.emplace_back(p, p + d[k].in_len);
			}
			if (info.has_content_size) {
				++declared;
				if (sum != info.content_size)
					file_ok = false;
			}
			++frames;
			at += size_t(info.frame_len);
		}
		const char* base = strrchr(argv[a], '/');
		printf("%-28s %9zu bytes %3ld frames %6ld blocks  known %6ld unknown %ld  content sizes %ld  %s\n",
		       base ? base + 1 : argv[a], f.size(), frames, t.calls, t.known, t.unknown, declared,
		       file_ok ? "pass" : "FAIL");
		ok &= file_ok;
		all.calls += t.calls;
		all.known += t.known;
		all.unknown += t.unknown;
	}
	if (kept.size() < 3) {
		printf("fewer than three compressed blocks of 200 to 6000 bytes among the files\n");
		return 1;
	}
	for (size_t b = 0; b < 3; ++b) {  // every truncation: a prefix decodes to no more than the block
		Tally t;
		const int64_t whole = sized(kept[b].data(), kept[b].size(), false);
		bool pass = whole >= 0;
		for (size_t n = 0; n <= kept[b].size(); ++n) {
			const int64_t s = sized(kept[b].data(), n, false);
			t.add(s);
			if (s > whole)
				pass = false;
		}
		printf("truncations of block %zu     %9zu bytes %10ld calls  known %6ld unknown %ld  %s\n", b,
		       kept[b].size(), t.calls, t.known, t.unknown, pass ? "pass" : "FAIL");
		ok &= pass;
		all.calls += t.calls;
		all.known += t.known;
		all.unknown += t.unknown;
	}
	for (size_t b = 0; b < 2; ++b) {  // every bit of the first 64 bytes: any verdict, no report
		Tally t;
		for (size_t bit = 0; bit < 64 * 8 && bit / 8 < kept[b].size(); ++bit) {
			Bytes x = kept[b];
			x[bit >> 3] ^= uint8_t(1u << (bit & 7));
			t.add(sized(x.data(), x.size(), false));
		}
		printf("bit flips in block %zu       %9zu bytes %10ld calls  known %6ld unknown %ld  pass\n", b,
		       kept[b].size(), t.calls, t.known, t.unknown);
		all.calls += t.calls;
		all.known += t.known;
		all.unknown += t.unknown;
	}
	printf("total %ld calls: known %ld unknown %ld -- %s\n", all.calls, all.known, all.unknown,
	       ok ? "no sanitizer report, every golden block has a size" : "FAILED");
	return ok ? 0 : 1;
}
