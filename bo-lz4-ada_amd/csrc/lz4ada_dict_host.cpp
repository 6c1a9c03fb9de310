// lz4ada_dict_host.cpp -- one modern LZ4 frame decoded against a dictionary on
// the host: the statement the dictionary passes of
// lz4ada_decode_frames_device_dict are tested against, and the caller's way
// for a frame those passes answer with LZ4ADA_EXACT_PATH.  Semantics are the
// LZ4 frame specification's (LZ4F_decompress_usingDict), not the reference's:
// the reference knows no dictionary, so no quirk of it is replayed and every
// message here is this library's own.  Plain serial C++, no HIP call; depends
// on lz4ada_hip.h and lz4ada_frame_walk.h alone, so a plain C++ program can
// compile it (tools/dict_host_asan.cpp, which brings its own
// set_thread_error).
#include <stdint.h>
#include <string.h>

#include <string>

#include "lz4ada_frame_walk.h"
#include "lz4ada_hip.h"

namespace lz4ada {
void set_thread_error(const std::string& msg);  // lz4ada_host_common.cpp

namespace {

struct Fail {
	int code;
	std::string msg;
};

std::string at(int64_t v) { return " " + std::to_string(v); }

// One compressed block at in[0 .. n) decoded to out[pos ..), at most `room`
// bytes (the frame's block maximum, or what is left of out: too_small tells
// which ended it).  Its matches read out[base .. pos) and, before that, the
// last `du` bytes of the dictionary, which end at dict_end.  A block may end
// after a match, as everywhere in this library.
int64_t decode_block_dict(const uint8_t* in, int64_t n, uint8_t* out, int64_t base, int64_t pos, int64_t bmax,
                          int64_t out_cap, const uint8_t* dict_end, int64_t du, Fail& f)
{
	const int64_t start = pos, limit = start + bmax;
	int64_t p = 0;
	auto over = [&](int64_t want) {
		if (want > limit) {
			f = Fail{ LZ4ADA_DATA_CORRUPTION, "dictionary decode: a block decodes to more than the block maximum" };
			return true;
		}
		if (want > out_cap) {
			f = Fail{ LZ4ADA_TOO_LITTLE_MEMORY, "dictionary decode: the output holds" + at(out_cap) + " bytes" };
			return true;
		}
		return false;
	};
	auto ext = [&](int64_t& v) {  // 255* + rest
		for (;;) {
			if (p >= n)
				return false;
			const uint8_t b = in[p++];
			v += b;
			if (b != 255)
				return true;
			if (v > (int64_t(1) << 28))
				return false;
		}
	};
	while (p < n) {
		const uint8_t token = in[p++];
		int64_t L = token >> 4;
		if (L == 15 && !ext(L)) {
			f = Fail{ LZ4ADA_DATA_CORRUPTION, "dictionary decode: a literal length runs past the block" };
			return -1;
		}
		if (L > n - p) {
			f = Fail{ LZ4ADA_DATA_CORRUPTION, "dictionary decode: literals run past the block" };
			return -1;
		}
		if (over(pos + L))
			return -1;
		if (L)
			memcpy(out + pos, in + p, size_t(L));
		pos += L;
		p += L;
		if (p == n)
			break;  // the last sequence holds literals alone
		if (n - p < 2) {
			f = Fail{ LZ4ADA_DATA_CORRUPTION, "dictionary decode: the block ends inside an offset" };
			return -1;
		}
		const int64_t off = int64_t(in[p]) | (int64_t(in[p + 1]) << 8);
		p += 2;
		int64_t ml = token & 15;
		if (ml == 15 && !ext(ml)) {
			f = Fail{ LZ4ADA_DATA_CORRUPTION, "dictionary decode: a match length runs past the block" };
			return -1;
		}
		ml += 4;
		if (off == 0) {
			f = Fail{ LZ4ADA_DATA_CORRUPTION, "dictionary decode: offset 0" };
			return -1;
		}
		if (off > pos - base + du) {
			f = Fail{ LZ4ADA_DATA_CORRUPTION, "dictionary decode: a match at output position" + at(pos) +
				                                  " reaches" + at(off - (pos - base) - du) +
				                                  " bytes before the dictionary's first usable byte" };
			return -1;
		}
		if (over(pos + ml))
			return -1;
		int64_t s = pos - base - off;  // source, relative to out + base
		for (; ml > 0 && s < 0; --ml, ++s)
			out[pos++] = dict_end[s];
		for (; ml > 0; --ml, ++s)
			out[pos++] = out[base + s];
	}
	return pos - start;
}

int decode(const uint8_t* p, int64_t len, const uint8_t* dict, int64_t dict_len, uint8_t* out, int64_t out_cap,
           int64_t* out_len, int64_t* consumed, Fail& f)
{
	auto fail = [&](int code, const std::string& msg) {
		f = Fail{ code, msg };
		return code;
	};
	if (!out_len || !consumed || len < 0 || (len > 0 && !p) || dict_len < 0 || (dict_len > 0 && !dict) ||
	    out_cap < 0 || (out_cap > 0 && !out))
		return fail(LZ4ADA_ASSERTION_ERROR, "lz4ada_decode_frame_dict_host: a NULL pointer or a negative length");
	*out_len = *consumed = 0;
	if (len < 4)
		return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: the frame is truncated");
	const uint32_t magic = walk_load32(p);
	if (magic == 0x184c2102u || (magic >= 0x184d2a50u && magic <= 0x184d2a5fu))
		return fail(LZ4ADA_NOT_SUPPORTED, "dictionary decode: modern frames only (legacy or skippable frame)");
	if (magic != 0x184d2204u)
		return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: not an LZ4 frame");
	if (len < 7)
		return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: the frame is truncated");
	const uint8_t flg = p[4], bd = p[5];
	if (((flg & 0xc0u) >> 6) != 1)
		return fail(LZ4ADA_NOT_SUPPORTED, "dictionary decode: unknown frame version");
	if ((flg & 2u) || (bd & 0x8fu))
		return fail(LZ4ADA_NOT_SUPPORTED, "dictionary decode: reserved header bits are set");
	const unsigned code = (bd & 0x70u) >> 4;
	if (code < 4)
		return fail(LZ4ADA_NOT_SUPPORTED, "dictionary decode: unknown block maximum");
	const int64_t bmax = int64_t(65536) << (2 * (code - 4));
	const int64_t dlen = 2 + ((flg & 8u) ? 8 : 0) + ((flg & 1u) ? 4 : 0);  // the id is not compared here
	int64_t pos = 4 + dlen + 1;
	if (pos > len)
		return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: the frame is truncated");
	if (p[4 + dlen] != uint8_t((walk_descriptor_xxh32(p + 4, dlen) >> 8) & 0xffu))
		return fail(LZ4ADA_CHECKSUM_ERROR, "dictionary decode: header checksum");
	const bool indep = (flg & 0x20u) != 0, bck = (flg & 16u) != 0, cck = (flg & 4u) != 0, has_size = (flg & 8u) != 0;
	const uint64_t content_size =
	    has_size ? uint64_t(walk_load32(p + 6)) | (uint64_t(walk_load32(p + 10)) << 32) : 0;
	const int64_t du = dict_len < 65536 ? dict_len : 65536;
	const uint8_t* const dict_end = dict ? dict + dict_len : nullptr;

	int64_t opos = 0;
	for (;;) {
		if (pos + 4 > len)
			return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: the frame is truncated");
		uint32_t word = walk_load32(p + pos);
		pos += 4;
		if (word == 0)
			break;
		const bool stored = (word & 0x80000000u) != 0;
		word &= 0x7fffffffu;
		if (int64_t(word) > bmax)
			return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: a block is larger than the block maximum");
		if (pos + int64_t(word) + (bck ? 4 : 0) > len)
			return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: the frame is truncated");
		if (bck && walk_xxh32(p + pos, word) != walk_load32(p + pos + word))
			return fail(LZ4ADA_CHECKSUM_ERROR, "dictionary decode: block checksum");
		if (stored) {
			if (int64_t(word) > out_cap - opos)
				return fail(LZ4ADA_TOO_LITTLE_MEMORY, "dictionary decode: the output holds" + at(out_cap) + " bytes");
			if (word)
				memcpy(out + opos, p + pos, word);
			opos += word;
		} else {
			const int64_t got = decode_block_dict(p + pos, word, out, indep ? opos : 0, opos, bmax, out_cap,
			                                      dict_end, du, f);
			if (got < 0)
				return f.code;
			opos += got;
		}
		pos += int64_t(word) + (bck ? 4 : 0);
	}
	if (has_size && uint64_t(opos) != content_size)
		return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: the frame decodes to" + at(opos) +
		                                            " bytes, its header declares" + at(int64_t(content_size)));
	if (cck) {
		if (pos + 4 > len)
			return fail(LZ4ADA_DATA_CORRUPTION, "dictionary decode: the frame is truncated");
		if (walk_xxh32(out, opos) != walk_load32(p + pos))
			return fail(LZ4ADA_CHECKSUM_ERROR, "dictionary decode: content checksum");
		pos += 4;
	}
	*out_len = opos;
	*consumed = pos;
	return LZ4ADA_OK;
}

}  // namespace
}  // namespace lz4ada

extern "C" int lz4ada_decode_frame_dict_host(const uint8_t* frame, int64_t len, const uint8_t* dict, int64_t dict_len,
                                             uint8_t* out, int64_t out_cap, int64_t* out_len,
                                             int64_t* frame_consumed)
{
	lz4ada::Fail f{ LZ4ADA_OK, std::string() };
	const int st = lz4ada::decode(frame, len, dict, dict_len, out, out_cap, out_len, frame_consumed, f);
	if (st != LZ4ADA_OK)
		lz4ada::set_thread_error(f.msg);
	return st;
}
