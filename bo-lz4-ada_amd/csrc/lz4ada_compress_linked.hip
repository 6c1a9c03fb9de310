// lz4ada_compress_linked.hip -- the gfx950 kernel of the compressor for frames
// of linked blocks (lz4ada_bulk_compress.cpp); a unit of its
// own, so that k_compress_blocks and k_compress_blocks_dict keep their code.
//  * k_compress_blocks_linked -- k_compress_blocks_dict with the history given
//    per block, one wave per block.  What lies at [-dl, 0) in front of a block
//    follows from its place in its record and the call's dictionary:
//     - block 0, no dictionary: nothing; the table starts zeroed, dl = 0, the
//       plain rule;
//     - block 0, a dictionary: its used tail D, the table a copy of the seeded
//       one (k_compress_dict_table), as in k_compress_blocks_dict;
//     - block i >= 1: the 65,536 bytes of its own record in front of it in
//       d_in.  The wave seeds its own table: every q of [-65536, -4], 64
//       consecutive positions per step, SEED_DEPTH steps' loads in flight, by
//       atomicMax of q + 65536 + 1 (positions only grow, so the maximum is the
//       latest, as in the serial statement's ascending loop).  The history is
//       contiguous with the block, so a candidate below 0 and the extension
//       read straight through position 0.
// The kernel waits for no other workgroup; every loop is bounded by the block
// length or by 65,536.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4ada_compress.h"
#include "lz4ada_dev.h"
#include "lz4ada_internal.h"

namespace lz4ada {

namespace {

constexpr uint32_t SEED_DEPTH = 8;  // steps of 64 positions whose loads are issued before the first insert
constexpr uint32_t SEED_LAST = uint32_t(COMP_LINK_WINDOW) - 4;  // index of q = -4, the last seeded position
static_assert(COMP_LINK_WINDOW % (64 * SEED_DEPTH) == 0, "the seeding loop covers the window in whole rounds");

// 255* and the rest of a length v >= 15 at dst[o ..) -> the bytes written
// (comp_ext_len(v)); the caller has checked them against the slot's end.
__device__ __forceinline__ int32_t put_ext(g8* dst, int32_t o, int32_t v, uint32_t lane)
{
	if (v < 15)
		return 0;
	const int32_t k = (v - 15) / 255;
	for (int32_t i = int32_t(lane); i < k; i += 64)
		dst[o + i] = 255;
	if (lane == 0)
		dst[o + k] = uint8_t((v - 15) - 255 * k);
	return k + 1;
}

}  // namespace

__global__ __launch_bounds__(64) void k_compress_blocks_linked(const uint8_t* __restrict__ d_in,
                                                                const CompBlock* __restrict__ blk,
                                                                const CompJob* __restrict__ jobs, uint32_t nblocks,
                                                                const uint8_t* __restrict__ d_tail, uint32_t dict_len,
                                                                const uint32_t* __restrict__ seed,
                                                                uint8_t* __restrict__ slots,
                                                                uint32_t* __restrict__ csize)
{
	__shared__ __attribute__((aligned(16))) uint32_t table[COMP_TABLE];  // virtual position + dl + 1; 0: none
	const uint32_t b = blockIdx.x;
	if (b >= nblocks)
		return;
	const uint32_t lane = lane_id();
	const uint64_t in_off = wave_uniform(blk[b].in_off), slot_off = wave_uniform(blk[b].slot_off);
	const int32_t n = wave_uniform(int32_t(blk[b].len));
	// a block that does not begin its record lies a whole number of block
	// lengths (>= 65,536 each) into it
	const bool cont = in_off != wave_uniform(jobs[wave_uniform(blk[b].job)].in_off);
	const int32_t dl = cont ? int32_t(COMP_LINK_WINDOW) : wave_uniform(int32_t(dict_len));  // 0, or 4 .. 65,536
	cg8* const src = gptr(d_in) + in_off;
	// virtual position 0 of the history: hst[x], -dl <= x < 0 (never read when dl == 0)
	cg8* const hst = cont ? src : gptr(d_tail) + dl;
	g8* const dst = gptr(slots) + slot_off;
	const int32_t cap = n - 1;  // compressed only when shorter than the block; the slot holds n bytes
	if (!cont && dl) {
		const GLOBAL u32x4* const s4 = reinterpret_cast<const GLOBAL u32x4*>(gptr(seed));
		u32x4* const t4 = reinterpret_cast<u32x4*>(table);
		for (uint32_t i = lane; i < COMP_TABLE / 4; i += 64)
			t4[i] = s4[i];
	} else {
		for (uint32_t i = lane; i < COMP_TABLE; i += 64)
			table[i] = 0;
	}
	__syncthreads();
	if (cont && n >= COMP_MIN_BLOCK) {  // a block under 13 bytes is one literal run and seeds nothing
		cg8* const h0 = src - COMP_LINK_WINDOW;
		for (uint32_t i0 = 0; i0 < uint32_t(COMP_LINK_WINDOW); i0 += 64 * SEED_DEPTH) {
			uint32_t v[SEED_DEPTH];
#pragma unroll
			for (uint32_t k = 0; k < SEED_DEPTH; ++k) {
				const uint32_t i = i0 + 64 * k + lane;
				v[k] = i <= SEED_LAST ? ld32u_cached(h0 + i) : 0u;
			}
#pragma unroll
			for (uint32_t k = 0; k < SEED_DEPTH; ++k) {
				const uint32_t i = i0 + 64 * k + lane;
				if (i <= SEED_LAST)
					atomicMax(&table[comp_hash(v[k])], i + 1);
			}
		}
		__syncthreads();
	}
	int32_t op = 0, anchor = 0;
	bool stored = false;
	if (n >= COMP_MIN_BLOCK) {
		const int32_t mlast = n - int32_t(COMP_MFLIMIT), mend = n - int32_t(COMP_LAST_LITERALS);
		int32_t w = 0;
		while (w <= mlast) {  // every turn moves w on by a window or a match
			const int32_t wn = min(mlast - w + 1, int32_t(COMP_WINDOW));
			const int32_t p = w + int32_t(lane);
			const bool active = int32_t(lane) < wn;
			const uint32_t v = active ? ld32u_cached(src + p) : 0u;
			const uint32_t h = comp_hash(v);
			const uint32_t e = active ? table[h] : 0u;  // read before any position of the window is inserted
			const int32_t c = int32_t(e) - 1 - dl;      // -dl <= c <= -4 (seeded) or 0 <= c < w
			bool ok = e != 0 && p - c <= int32_t(COMP_MAX_OFF);
			if (ok)
				ok = ld32u_cached(c < 0 ? hst + c : src + c) == v;
			const uint64_t won = __ballot(ok);
			const int32_t wl = won ? int32_t(__builtin_ctzll(won)) : wn - 1;
			if (active && int32_t(lane) <= wl)
				atomicMax(&table[h], uint32_t(p + dl + 1));
			wave_lds_fence();
			if (!won) {
				w += wn;
				continue;
			}
			const int32_t win = w + wl;
			const int32_t cand = wave_uniform(int32_t(__shfl(e, wl))) - 1 - dl;
			// the match's length: 4 bytes per lane, the first lane with a
			// mismatch or at the end (n - 5) ends it
			int32_t ml = 4;
			for (;;) {
				const int32_t q = win + ml + 4 * int32_t(lane);
				const int32_t rem = mend - q;  // bytes of this lane's four the match may still take
				uint32_t x = 1;
				if (rem > 0) {
					// the candidate's dword at virtual position y < q; astride 0 the
					// record's history is read through, the dictionary's bytes come
					// from D below 0 and from src[0 .. 3) (n >= 13) above
					const int32_t y = cand + ml + 4 * int32_t(lane);
					uint32_t cv;
					if (cont || y >= 0 || y <= -4) {
						cv = ld32u_cached(y < 0 ? hst + y : src + y);
					} else {
						cv = 0;
						for (int32_t k = 0; k < 4; ++k)
							cv |= uint32_t(y + k < 0 ? hst[y + k] : src[y + k]) << (8 * k);
					}
					x = ld32u_cached(src + q) ^ cv;
					if (rem < 4)
						x |= 1u << (8 * rem);
				}
				const int32_t same = x ? int32_t(__builtin_ctz(x) >> 3) : 4;
				const uint64_t ends = __ballot(same < 4);
				if (ends) {
					const int32_t fl = int32_t(__builtin_ctzll(ends));
					ml += 4 * fl + wave_uniform(int32_t(__shfl(same, fl)));
					break;
				}
				ml += 256;
			}
			const int32_t lit = win - anchor;
			if (op + int32_t(comp_seq_len(lit, ml)) > cap) {
				stored = true;
				break;
			}
			if (lane == 0)
				dst[op] = uint8_t((min(lit, 15) << 4) | min(ml - 4, 15));
			int32_t o = op + 1;
			o += put_ext(dst, o, lit, lane);
			for (int32_t i = int32_t(lane); i < lit; i += 64)
				dst[o + i] = src[anchor + i];
			o += lit;
			if (lane == 0) {
				dst[o] = uint8_t(win - cand);
				dst[o + 1] = uint8_t((win - cand) >> 8);
			}
			o += 2;
			o += put_ext(dst, o, ml - 4, lane);
			op = o;
			w = anchor = win + ml;
		}
	}
	if (!stored) {
		const int32_t lit = n - anchor;
		if (op + int32_t(comp_last_len(lit)) > cap) {
			stored = true;
		} else {
			if (lane == 0)
				dst[op] = uint8_t(min(lit, 15) << 4);
			int32_t o = op + 1;
			o += put_ext(dst, o, lit, lane);
			for (int32_t i = int32_t(lane); i < lit; i += 64)
				dst[o + i] = src[anchor + i];
			op = o + lit;
		}
	}
	if (lane == 0)
		csize[b] = stored ? 0u : uint32_t(op);
}

hipError_t launch_compress_blocks_linked(const uint8_t* d_in, const CompBlock* d_blk, const CompJob* d_jobs,
                                         uint32_t nblocks, const uint8_t* d_tail, uint32_t dl, const uint32_t* d_seed,
                                         uint8_t* d_slots, uint32_t* d_csize, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_compress_blocks_linked, dim3(nblocks), dim3(64), 0, stream, d_in, d_blk, d_jobs, nblocks,
	                   d_tail, dl, d_seed, d_slots, d_csize);
	return hipGetLastError();
}

}  // namespace lz4ada
