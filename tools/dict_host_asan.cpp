// dict_host_asan.cpp -- lz4ada_decode_frame_dict_host (csrc/lz4ada_dict_host.cpp)
// under AddressSanitizer and UBSan, host code only: every truncation and every
// single-byte corruption of three committed dictionary frames, each input, the
// dictionary and the output in heap blocks of exactly their lengths, so a read
// of one byte outside the frame or the dictionary, or a write past out_cap,
// stops the run.  Every output capacity from 0 to the frame's size is tried on
// the intact frame too.  No GPU, no library, nothing loaded into Python:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Ibo-lz4-ada_amd/csrc tools/dict_host_asan.cpp bo-lz4-ada_amd/csrc/lz4ada_dict_host.cpp
//       -o tools/_build/dict_host_asan
//   tools/_build/dict_host_asan tests/golden/lz4f_dict > profiles/dict_host_asan.txt
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lz4ada_hip.h"

namespace lz4ada {
static std::string g_msg;
void set_thread_error(const std::string& msg) { g_msg = msg; }  // the library's, for the unit under test
}  // namespace lz4ada

using Bytes = std::vector<uint8_t>;

static Bytes slurp(const std::string& path)
{
	Bytes b;
	FILE* f = fopen(path.c_str(), "rb");
	if (!f) {
		fprintf(stderr, "cannot read %s\n", path.c_str());
		exit(2);
	}
	uint8_t buf[65536];
	for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
		b.insert(b.end(), buf, buf + n);
	fclose(f);
	return b;
}

static uint8_t* exact(const uint8_t* p, size_t n)
{
	uint8_t* q = static_cast<uint8_t*>(malloc(n ? n : 1));
	if (n)
		memcpy(q, p, n);
	return q;
}

struct Tally {
	long calls = 0, st[10] = { 0 };
};

static int decode(const uint8_t* f, size_t n, const uint8_t* d, size_t dn, size_t cap, Bytes* got, Tally& t)
{
	uint8_t* in = exact(f, n);
	uint8_t* out = static_cast<uint8_t*>(malloc(cap ? cap : 1));
	int64_t olen = -1, used = -1;
	const int st = lz4ada_decode_frame_dict_host(n ? in : nullptr, int64_t(n), dn ? d : nullptr, int64_t(dn),
	                                             cap ? out : nullptr, int64_t(cap), &olen, &used);
	t.calls++;
	t.st[st < 0 || st > 9 ? 9 : st]++;
	bool ok = st == LZ4ADA_OK ? (olen >= 0 && size_t(olen) <= cap && used >= 0 && size_t(used) <= n)
	                          : (olen == 0 && used == 0 && !lz4ada::g_msg.empty());
	if (!ok) {
		printf("FAIL: status %d olen %lld used %lld\n", st, (long long)olen, (long long)used);
		exit(1);
	}
	if (got && st == LZ4ADA_OK)
		got->assign(out, out + olen);
	free(out);
	free(in);
	return st;
}

static bool run(const std::string& dir, const char* frame, const char* dict, size_t size, Tally& all)
{
	const Bytes f = slurp(dir + "/" + frame), dfile = slurp(dir + "/" + dict);
	uint8_t* d = exact(dfile.data(), dfile.size());
	Tally t;
	Bytes plain;
	bool ok = decode(f.data(), f.size(), d, dfile.size(), size, &plain, t) == LZ4ADA_OK && plain.size() == size;
	// every truncation
	for (size_t n = 0; n < f.size(); ++n)
		ok &= decode(f.data(), n, d, dfile.size(), size, nullptr, t) != LZ4ADA_OK;
	// every single-byte corruption (two patterns): any status, no report; OK only with a plausible result
	long same = 0;
	for (size_t i = 0; i < f.size(); ++i)
		for (uint8_t x : { uint8_t(0x01), uint8_t(0xff) }) {
			Bytes g = f;
			g[i] ^= x;
			Bytes got;
			if (decode(g.data(), g.size(), d, dfile.size(), size + 4096, &got, t) == LZ4ADA_OK && got == plain)
				same++;
		}
	// every output capacity below the size
	for (size_t cap = 0; cap < size; cap += (size > 4096 ? 61 : 1))
		ok &= decode(f.data(), f.size(), d, dfile.size(), cap, nullptr, t) == LZ4ADA_TOO_LITTLE_MEMORY;
	// a dictionary cut short from the front, and none
	for (size_t cut : { size_t(1), dfile.size() / 2, dfile.size() })
		decode(f.data(), f.size(), d + cut, dfile.size() - cut, size, nullptr, t);
	printf("%-10s %-10s %7zu -> %7zu bytes %8ld calls  ok %ld checksum %ld corruption %ld memory %ld unsupported %ld"
	       "  (%ld corruptions decode to the same bytes)  %s\n",
	       frame, dict, f.size(), size, t.calls, t.st[0], t.st[1], t.st[2], t.st[5], t.st[3], same, ok ? "pass" : "FAIL");
	all.calls += t.calls;
	for (int i = 0; i < 10; ++i)
		all.st[i] += t.st[i];
	free(d);
	return ok;
}

int main(int argc, char** argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: dict_host_asan tests/golden/lz4f_dict\n");
		return 2;
	}
	Tally all;
	bool ok = true;
	// (frame, its dictionary, its plaintext's length: tests/golden/lz4f_dict/manifest.json)
	ok &= run(argv[1], "f03.lz4", "dict_b.bin", 512, all);   // small, linked header options
	ok &= run(argv[1], "f06.lz4", "dict_a.bin", 1500, all);  // block and content checksums
	ok &= run(argv[1], "f12.lz4", "dict_a.bin", 7000, all);  // content size
	printf("total %ld calls: ok %ld checksum %ld corruption %ld memory %ld unsupported %ld -- %s\n", all.calls,
	       all.st[0], all.st[1], all.st[2], all.st[5], all.st[3],
	       ok ? "no sanitizer report, every truncation and short capacity refused" : "FAILED");
	return ok ? 0 : 1;
}
