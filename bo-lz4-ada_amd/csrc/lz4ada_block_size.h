// lz4ada_block_size.h -- the decoded length of one block from its payload
// alone, as host/device code: the sequence chain that
// Decompress_Full_Block walks (lib/lz4ada.adb:716-788), stated without
// output, history or exceptions.  It is the serial statement of the rule;
// k_block_sizes (lz4ada_sizes.hip) states it a second time for one wave, and
// tests/test_gpu_frames_sizes.py pins the two to each other and to the
// oracle's lengths.
//
// A chain is accepted exactly when Decompress_Full_Block accepts it as a
// chain: the block may end after a match; a sequence that ends the block with
// its literals must carry a zero match nibble; a literal run may not pass the
// end; a length extension or an offset may not be cut off by it.  Offsets are
// not judged (0, or one that reaches before the output, is the decoders'
// business), so a size says nothing about whether the block decodes.
//
// Depends on nothing, so a plain C++ program can include it
// (tools/block_size_asan.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4ADA_BS_HD __host__ __device__
#else
#define LZ4ADA_BS_HD
#endif

namespace lz4ada {

constexpr uint32_t BLOCK_SIZE_UNKNOWN = 0xFFFFFFFFu;

// The decoded length of the block at [p, p + n), or -1: the chain is
// malformed, or the length does not fit below BLOCK_SIZE_UNKNOWN.  stored:
// the length is n.  Reads no byte outside [p, p + n); every loop ends with
// the input, since each step reads the byte at i and moves past it.
LZ4ADA_BS_HD inline int64_t block_decoded_size(const uint8_t* p, int64_t n, bool stored)
{
	if (n < 0)
		return -1;
	uint64_t out = uint64_t(n);
	if (!stored) {
		out = 0;
		int64_t i = 0;
		while (i < n) {
			const uint8_t token = p[i++];
			uint64_t lit = token >> 4, ml = token & 15u;
			if (lit == 15) {
				uint8_t e;
				do {
					if (i >= n)
						return -1;  // the extension is cut off
					e = p[i++];
					lit += e;
				} while (e == 255);
			}
			if (lit > uint64_t(n - i))
				return -1;  // the literal run passes the end
			i += int64_t(lit);
			out += lit;
			if (i == n) {
				if (ml != 0)
					return -1;  // a match is announced and the block is over
				break;
			}
			if (n - i < 2)
				return -1;  // the offset is cut in half
			i += 2;
			if (ml == 15) {
				uint8_t e;
				do {
					if (i >= n)
						return -1;
					e = p[i++];
					ml += e;
				} while (e == 255);
			}
			out += ml + 4;
		}
	}
	return out < BLOCK_SIZE_UNKNOWN ? int64_t(out) : -1;
}

}  // namespace lz4ada
