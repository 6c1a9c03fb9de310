// lz4ada_idx_window.inc -- part of lz4ada_idx.hip, which includes it inside namespace
// lz4ada::idx (one translation unit: the text below is that file's, moved):
// pass 2's LDS output window, its pattern helpers and owner searches, and
// the ring-sourced matches (ring_match, ring_pieces, ring_lanes).

// ------------------------------------------------------ LDS output window
// A batch whose output fits in OW bytes is assembled in an LDS ring that
// also keeps the 2+ KiB of output before it, then flushed to HBM with
// aligned 16-byte stores (the partial last 16 bytes go with the next batch).
constexpr int OW = 4080;        // max batch output assembled in LDS (see glo below)
constexpr int ORING = 8192;     // LDS output ring (batch + history)
constexpr int OMASK = ORING - 1;
constexpr int MAXSEQ = 128;     // sequences per batch (2 rounds: 192 VGPRs; 256 took 254 and spilled)
constexpr int RMAX = MAXSEQ / 64;  // rounds of 64 sequences per batch
constexpr int GC = 1;           // 16-byte pieces an HBM-sourced match loads in its own lane (1: fewest registers; the rest are dealt)
constexpr int FLUSH_ST = (OW + 15) / 16 / 64 + 1;  // store instructions per flush (fixed)
static_assert(2 * OW + 16 <= ORING, "batch + its HBM threshold must fit the ring");
// batch cut limits (experiments: a smaller cut with the same ring and HBM threshold)
#ifndef LZ4ADA_OW_CUT
#define LZ4ADA_OW_CUT OW
#endif
#ifndef LZ4ADA_SEQ_CUT
#define LZ4ADA_SEQ_CUT MAXSEQ
#endif

struct alignas(16) DecLds {
	uint8_t ring[RING + 16];      // staged input: 4 chunks of 2 KiB (+ mirror)
	uint8_t oring[ORING];         // output window
	uint16_t cst[MAXSEQ];         // the batch's sequence starts, in order
	uint8_t own[256];             // piece -> owning lane (dealt HBM pieces)
	uint64_t rrec[4 * 64];        // pass-1 records of the staged chunks' sub-segments
	uint64_t ldesc[2 * 64];       // literal runs of both rounds (dealt literal pieces)
	uint32_t plut[16 * 4];        // v_perm selectors of the period-off patterns (pattern_lut_init)
	uint8_t junk[16];             // target of the stores a lane does not need (lds_store_bf)
};
static_assert(sizeof(DecLds) <= 20480, "8 waves per CU: at most 20 KiB of LDS per wave");

// The output window and per-wave scratch of an LDS layout: DecLds (one
// wave per block) holds them directly; a k_decode_pp2 wave's view (WP2,
// below) picks its wave's scratch.
__device__ __forceinline__ uint8_t* oring_of(DecLds& D) { return D.oring; }
__device__ __forceinline__ const uint8_t* oring_of(const DecLds& D) { return D.oring; }
__device__ __forceinline__ uint8_t* own_of(DecLds& D) { return D.own; }
__device__ __forceinline__ uint64_t* ldesc_of(DecLds& D) { return D.ldesc; }
// ... and the staged input with its pass-1 records
__device__ __forceinline__ uint8_t* ring_of(DecLds& D) { return D.ring; }
__device__ __forceinline__ uint64_t* rrec_of(DecLds& D) { return D.rrec; }
// Layouts with junk bytes and the pattern selectors (the one-wave decoder):
// branch-free exact stores (lds_store_bf) and period patterns by v_perm
// (pattern_perm); the two-wave layout keeps the branching forms.
template <class LD>
struct lds_fast {
	static constexpr bool value = false;
};
template <>
struct lds_fast<DecLds> {
	static constexpr bool value = true;
};
__device__ __forceinline__ uint8_t* junk_of(DecLds& D) { return D.junk; }
__device__ __forceinline__ const uint32_t* plut_of(const DecLds& D) { return D.plut; }
template <class LD>
__device__ __forceinline__ uint8_t* junk_of(LD&) { return nullptr; }
template <class LD>
__device__ __forceinline__ const uint32_t* plut_of(const LD&) { return nullptr; }
// the window's size - 1 (a power of two) for a layout: ORING unless the
// layout says otherwise (the pipelined pair's 16 KiB window)
template <class LD>
constexpr uint32_t omask_v = OMASK;
template <class LD>
__device__ __forceinline__ constexpr uint32_t omask_of(const LD&) { return omask_v<LD>; }

// Exact store of n (0..16) bytes of v at p, without branches: each of the
// five stores (16, 8, 4, 2, 1 bytes) goes to its place or, when n does not
// take it, to the 16 junk bytes, so every lane runs the same five ds_write
// instructions (lds_store_n's four divergent branches cost a wave whose
// lanes disagree on n all of them, with their exec-mask bookkeeping).
__device__ __forceinline__ void lds_store_bf(uint8_t* p, uint8_t* junk, u32x4 v, uint32_t n)
{
	const uint64_t lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
	const uint64_t hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
	__builtin_memcpy(n >= 16u ? p : junk, &v, 16);
	__builtin_memcpy((n & 8u) ? p : junk, &lo, 8);
	const uint64_t r8 = (n & 8u) ? hi : lo;
	uint8_t* const p4 = p + (n & 8u);
	const uint32_t w4 = uint32_t(r8);
	__builtin_memcpy((n & 4u) ? p4 : junk, &w4, 4);
	const uint32_t r4 = (n & 4u) ? uint32_t(r8 >> 32) : w4;
	uint8_t* const p2 = p4 + (n & 4u);
	const uint16_t w2 = uint16_t(r4);
	__builtin_memcpy((n & 2u) ? p2 : junk, &w2, 2);
	*((n & 1u) ? p2 + (n & 2u) : junk) = uint8_t((n & 2u) ? (r4 >> 16) : r4);
}

// Exact-length store of n bytes (fast layouts: 0..16; else 1..16) at
// output position x into the ring.
template <class LD>
__device__ __forceinline__ void ostore(LD& L, int32_t x, u32x4 v, int32_t n)
{
	const uint32_t a = uint32_t(x) & omask_of(L);
	if constexpr (lds_fast<LD>::value) {
		// a store wrapping the ring's end (one piece every 8 KiB of output)
		// takes the byte loop below, the wave's other lanes with it
		if (__builtin_expect(!__any(a + uint32_t(n) > omask_of(L) + 1), 1)) {
			lds_store_bf(&oring_of(L)[a], junk_of(L), v, uint32_t(n));
			return;
		}
	}
	if (a + uint32_t(n) <= omask_of(L) + 1) {
		// one ds_write_b128 even when misaligned: 256 cycles against 1579
		// for four ds_write_b32 (each misaligned one is split too) and 384
		// for 16 ds_write_b8 (tools/lds_bench.hip, dependent chain)
		lds_store_n(&oring_of(L)[a], v, n);
		return;
	}
	const uint64_t lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
	const uint64_t hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
#pragma clang loop vectorize(disable) unroll(disable)
	for (int32_t i = 0; i < n; ++i) {
		const uint64_t w = i < 8 ? lo : hi;
		oring_of(L)[(a + uint32_t(i)) & omask_of(L)] = uint8_t(w >> (8 * (i & 7)));
	}
}

// Whole-piece store: v's 16 bytes at output position x where has, else
// nothing.  The fast layouts issue one ds_write_b128, to the piece's place
// or to the junk bytes -- none of lds_store_bf's select network, no second
// to fifth store; a piece wrapping the ring's end sends the wave through
// ostore, as there.  For a dealt piece that is not its run's last: such a
// piece lies wholly inside its own run.
template <class LD>
__device__ __forceinline__ void ostore16(LD& L, int32_t x, u32x4 v, bool has)
{
	if constexpr (lds_fast<LD>::value) {
		const uint32_t a = uint32_t(x) & omask_of(L);
		if (__builtin_expect(!__any(has && a + 16u > omask_of(L) + 1), 1)) {
			__builtin_memcpy(has ? &oring_of(L)[a] : junk_of(L), &v, 16);
			return;
		}
		ostore(L, x, v, has ? 16 : 0);
	} else {
		if (has)
			ostore(L, x, v, 16);
	}
}

template <class LD>
__device__ __forceinline__ u32x4 oload16(const LD& L, int32_t x)
{
	return ring16(oring_of(L), uint32_t(x) & omask_of(L), omask_of(L));
}

// Store steps and phases of period-off patterns without integer division:
// bits 5(o-1).. = o * (16 / o), bits 40 + 2(o-1).. = 8 mod o, for o = 1..8.
constexpr uint64_t pattern_lut()
{
	uint64_t v = 0;
	for (int o = 1; o <= 8; ++o)
		v |= (uint64_t(o * (16 / o)) << (5 * (o - 1))) | (uint64_t(8 % o) << (40 + 2 * (o - 1)));
	return v;
}
constexpr uint64_t PAT_LUT = pattern_lut();

// 16 bytes of the period-off (1..15) sequence whose first off bytes are
// s0|s1's, and the largest multiple of off <= 16: storing it every stp
// bytes keeps the phase.
__device__ __forceinline__ void make_pattern16(uint64_t s0, uint64_t s1, int32_t off, u32x4& pv,
                                               int32_t& stp)
{
	uint64_t x, hi;
	if (off <= 8) {
		x = off == 8 ? s0 : (s0 & ((uint64_t(1) << (8 * off)) - 1));
		// doubling x |= x << 8w for w = off, 2 off, 4 off while w < 8, with
		// selects instead of a lane-divergent loop
#pragma unroll
		for (int i = 0; i < 3; ++i) {
			const int32_t w = off << i;
			x |= w < 8 ? x << (8 * w) : 0;
		}
		const uint32_t sh = uint32_t(off - 1);
		stp = int32_t((PAT_LUT >> (5 * sh)) & 31u);
		const int32_t r = int32_t((PAT_LUT >> (40 + 2 * sh)) & 3u);
		// bytes 8..15: x[r..7], then x from 8 - off on (x is off-periodic)
		hi = r == 0 ? x : (x >> (8 * r)) | ((x >> (8 * (8 - off))) << (8 * (8 - r)));
	} else {
		const int32_t r = off - 8;
		x = s0;
		hi = (s1 & ((uint64_t(1) << (8 * r)) - 1)) | (s0 << (8 * r));
		stp = off;
	}
	pv.x = uint32_t(x);
	pv.y = uint32_t(x >> 32);
	pv.z = uint32_t(hi);
	pv.w = uint32_t(hi >> 32);
}

// a's bytes j < c, b's from c on (c = 1..15)
__device__ __forceinline__ u32x4 merge_at(u32x4 a, u32x4 b, int32_t c)
{
	auto m = [c](int32_t d) -> uint32_t {
		const int32_t t = c - 4 * d;
		return t >= 4 ? ~0u : (t <= 0 ? 0u : (1u << (8 * t)) - 1u);
	};
	u32x4 v;
	v.x = (a.x & m(0)) | (b.x & ~m(0));
	v.y = (a.y & m(1)) | (b.y & ~m(1));
	v.z = (a.z & m(2)) | (b.z & ~m(2));
	v.w = (a.w & m(3)) | (b.w & ~m(3));
	return v;
}

// Store step of a period-off pattern match (make_pattern16's stp).
__device__ __forceinline__ int32_t pattern_step(int32_t off)
{
	return off <= 8 ? int32_t((PAT_LUT >> (5 * (off - 1))) & 31u) : off;
}

// v_perm_b32 selectors of the period-off patterns, off = 1..15 (entry off,
// dword d; entry 0 unused): byte t of output dword d is source byte
// (4d + t) mod off, taken from v.y:v.x (off <= 8, and dwords 0-1 -- v.x and
// v.y themselves -- of every off), v.z:v.x (dword 2, off >= 9) or
// v.w:v.x / v.y:v.x (dword 3, off >= 12 / 9..11): pattern_perm.  Written
// once per block by its wave (lane l: entry l / 4, dword l % 4).
__device__ __forceinline__ void pattern_lut_init(uint32_t* plut)
{
	const uint32_t l = lane_id(), off = l >> 2, d = l & 3u;
	uint32_t sel = 0;
	if (off > 0)
		for (uint32_t t = 0; t < 4; ++t) {
			const uint32_t idx = (4 * d + t) % off;
			uint32_t x = idx;
			if (off > 8 && d == 2 && idx >= 8)
				x = idx - 4;  // v.z byte idx - 8 (v_perm's src0 bytes are 4..7)
			if (off >= 12 && d == 3 && idx >= 12)
				x = idx - 8;  // v.w byte idx - 12
			sel |= x << (8 * t);
		}
	plut[l] = sel;
}

// The phase-0 period-off (1..15) pattern of the 16 source bytes v (the
// first off of them valid): make_pattern16's value in one LDS read, two
// selects and four v_perm_b32 instead of its 64-bit shift network.
// (pattern_sel is the LDS read: it needs off alone, so a caller issues it
// beside the source read and applies it once both have arrived)
__device__ __forceinline__ u32x4 pattern_sel(int32_t off, const uint32_t* plut)
{
	return *reinterpret_cast<const u32x4*>(plut + 4 * off);
}

__device__ __forceinline__ u32x4 pattern_perm(u32x4 v, int32_t off, u32x4 sel)
{
	const uint32_t h2 = off <= 8 ? v.y : v.z, h3 = off <= 11 ? v.y : v.w;
	u32x4 o;
	o.x = __builtin_amdgcn_perm(v.y, v.x, sel.x);
	o.y = __builtin_amdgcn_perm(v.y, v.x, sel.y);
	o.z = __builtin_amdgcn_perm(h2, v.x, sel.z);
	o.w = __builtin_amdgcn_perm(h3, v.x, sel.w);
	return o;
}

// Match with a final source entirely inside the ring (Output_With_History,
// lz4ada.adb:845-904).  Match byte i is source byte i mod off (the overlap
// rule), so no unit reads this match's own output: an off < 16 overlap
// stores a 16-byte period pattern every stp bytes, any other match 16
// source bytes per unit (a unit that wraps the period merges two reads).
// One loop for both forms: a wave runs max(units) over its lanes, not the
// two loops one after the other.
template <class LD>
__device__ __forceinline__ void ring_match(LD& L, int32_t dst, int32_t off, int32_t len)
{
	const int32_t src = dst - off;
	u32x4 pv = oload16(L, src);
	int32_t stp = 16;
	const bool pat = off < 16 && off < len;
	if (pat) {
		if constexpr (lds_fast<LD>::value) {
			pv = pattern_perm(pv, off, pattern_sel(off, plut_of(L)));
			stp = pattern_step(off);
		} else {
			make_pattern16(uint64_t(pv.x) | (uint64_t(pv.y) << 32), uint64_t(pv.z) | (uint64_t(pv.w) << 32),
			               off, pv, stp);
		}
	}
	ostore(L, dst, pv, min(16, len));
	int32_t start = 0;  // unit x of the wide form begins at source byte x mod off
	for (int32_t x = stp; x < len; x += stp) {
		u32x4 v = pv;
		if (!pat) {
			start += 16;
			if (start >= off)
				start -= off;
			v = oload16(L, src + start);
			if (off - start < 16)
				v = merge_at(v, oload16(L, src + start - off), off - start);
		}
		ostore(L, dst + x, v, min(16, len - x));
	}
}

// q = t / d and r = t mod d for 0 <= t < 2^22, 1 <= d < 2^16: float
// reciprocal (error < 1 in q) and one correction step.
__device__ __forceinline__ int32_t div_small(int32_t t, int32_t d, int32_t& r)
{
	int32_t q = int32_t(float(t) * __builtin_amdgcn_rcpf(float(d)));
	r = t - q * d;
	if (r < 0) {
		--q;
		r += d;
	}
	if (r >= d) {
		++q;
		r -= d;
	}
	return q;
}


__device__ __forceinline__ int32_t piece_owner(int32_t inc, int32_t t);

// Owner lane of piece t0 + lane, lane i holding pieces [inc_i - np_i,
// inc_i) (inc: inclusive prefix sum, monotone): each lane marks its first
// piece's slot of the 64-piece chunk in LDS, a prefix maximum fills the
// slots in between, and the chunk's first slot is seeded with the owner of
// piece t0 (the lanes with inc <= t0, counted from a ballot).  Two LDS
// round trips instead of six dependent shuffles of a binary search.
template <class LD>
__device__ __forceinline__ int32_t chunk_owner(LD& D, int32_t inc, int32_t np, int32_t t0)
{
	const int32_t lane = int32_t(lane_id());
	const int32_t seed = __popcll(__ballot(inc <= t0));
	uint8_t* own = own_of(D);
	own[lane] = uint8_t(lane == 0 ? seed : 0);
	const int32_t excl = inc - np;
	if (np > 0 && excl >= t0 && excl < t0 + 64)
		own[excl - t0] = uint8_t(lane);
	wave_lds_fence();
	const int32_t v = own[lane];
	wave_lds_fence();  // own[] is marked again for the next chunk
	return wave_incl_max(v);
}

// chunk_owner over two rounds' entries (round 0's lanes, then round 1's),
// from each entry's first piece e and whether it has any (nz): entry
// 64 r + lane holds pieces [e_r, e_r + its count), owner 0..127; seed is the
// owner of piece t0.
template <class LD>
__device__ __forceinline__ int32_t chunk_owner_marks(LD& D, int32_t seed, int32_t e0, bool nz0, int32_t e1,
                                                     bool nz1, int32_t t0)
{
	const int32_t lane = int32_t(lane_id());
	uint8_t* own = own_of(D);
	own[lane] = uint8_t(lane == 0 ? seed : 0);
	if (nz0 && e0 >= t0 && e0 < t0 + 64)
		own[e0 - t0] = uint8_t(lane);
	if (nz1 && e1 >= t0 && e1 < t0 + 64)
		own[e1 - t0] = uint8_t(64 + lane);
	wave_lds_fence();
	const int32_t v = own[lane];
	wave_lds_fence();  // own[] is marked again for the next chunk
	return wave_incl_max(v);
}

// ... from the inclusive prefix sums and the counts (entry 64 r + lane holds
// pieces [inc_r - np_r, inc_r))
template <class LD>
__device__ __forceinline__ int32_t chunk_owner2(LD& D, int32_t inc0, int32_t np0, int32_t inc1,
                                                int32_t np1, int32_t t0)
{
	const int32_t seed = __popcll(__ballot(inc0 <= t0)) + __popcll(__ballot(inc1 <= t0));
	return chunk_owner_marks(D, seed, inc0 - np0, np0 > 0, inc1 - np1, np1 > 0, t0);
}

// Every lane's match (dst, off, ml; ml = 0: none) with a source in the LDS
// ring, cut into units of which ring_pieces deals two per piece over the
// wave: 16 output bytes each, or stp bytes of a period-off pattern (off <
// 16 < ml would overlap: match byte i is source byte i mod off, so a unit
// never reads its own match's output).  Pieces are in output order; one
// reading output of a lower lane of its chunk waits until that lane has
// stored (ballot per step).
// Units of one match: 16 bytes each, or stp-byte steps of a period-off
// pattern (off < 16 < ml overlaps).
__device__ __forceinline__ int32_t match_pieces(int32_t off, int32_t ml)
{
	if (ml <= 0)
		return 0;
	if (!(off < 16 && off < ml))
		return (ml + 15) >> 4;
	const int32_t stp = pattern_step(off);
	int32_t rr;
	return stp == 16 ? (ml + 15) >> 4 : div_small(ml + stp - 1, stp, rr);
}

// Rounds whose idle own-piece slots take dealt HBM pieces beyond the 64th
// (decode_block's P; 0: none, every such piece loads in M)
#ifndef LZ4ADA_BORROW_SLOTS
#define LZ4ADA_BORROW_SLOTS 2
#endif
constexpr int BORROW_SLOTS = LZ4ADA_BORROW_SLOTS;
static_assert(BORROW_SLOTS >= 0 && BORROW_SLOTS <= 2, "round 0's slots, or both rounds'");

#ifndef LZ4ADA_FWD_ROUNDS
#define LZ4ADA_FWD_ROUNDS 5
#endif
constexpr int FWD_ROUNDS = LZ4ADA_FWD_ROUNDS;  // forwarding rounds of ring_lanes (0: none)
// (forwarding over ring_pieces' dealt pieces was measured and is gone: mixed
// 13.17 -> 13.41 ms with it, dense 37.07 -> 37.38; profiles/r06i_ab.txt)

// Dealt pieces of a ring-sourced match: two of match_pieces' units each
// (32 output bytes, or two steps of a period-off pattern), so a batch of
// mixed data deals ~48 pieces instead of ~71 and nearly always fits one
// 64-piece chunk (ring_pieces' set-up runs once per chunk).
__device__ __forceinline__ int32_t ring_piece_count(int32_t off, int32_t ml)
{
	return (match_pieces(off, ml) + 1) >> 1;
}

// chunk_owner2 from the entries' first pieces alone (e: exclusive prefix sum
// of the piece counts, 16 bits per round in ee; nz: the entry has pieces):
// the entries with inc <= t0 are those after the first with e <= t0 (entry
// 0's e is 0, and piece t0 exists).
template <class LD>
__device__ __forceinline__ int32_t chunk_owner_e(LD& D, uint32_t ee, bool nz0, bool nz1, int32_t t0)
{
	const int32_t e0 = int32_t(ee & 0xffffu), e1 = int32_t(ee >> 16);
	const int32_t seed = __popcll(__ballot(e0 <= t0)) + __popcll(__ballot(e1 <= t0)) - 1;
	return chunk_owner_marks(D, seed, e0, nz0, e1, nz1, t0);
}

// Marks two registers as changed (no instruction): what is computed from
// them after this point stays after it, instead of being hoisted out of the
// loop around it and held in registers across it.
__device__ __forceinline__ void step_state(uint32_t& a, uint32_t& b) { asm volatile("" : "+v"(a), "+v"(b)); }

// Both rounds' ring-sourced matches (round r: mdst[r], off[r], ml[r]; ml 0:
// none), dealt together in output order; a piece finds its match in an LDS
// descriptor (D.ldesc, free after the literals) instead of by shuffles.
// Piece k of a match is its units 2k and 2k + 1 (match_pieces' units: 16
// output bytes, or stp bytes' step of a period-off pattern).  With more
// than 16 bytes left at its start it stores 16 whole bytes there and an
// exact-length second unit ostp further on; else one exact-length unit.
// Neither unit reads its own match's output (ring_match's rule), so a
// piece waits only for the lower pieces of its chunk that write into the
// source of either unit.
template <class LD>
__device__ __forceinline__ int32_t ring_pieces(LD& D, const int32_t (&mdst)[RMAX],
                                               const int32_t (&off)[RMAX], const int32_t (&ml)[RMAX],
                                               int32_t o_batch)
{
	int32_t steps = 0;  // store steps (diagnostic count)
	const int32_t lane = int32_t(lane_id());
	const bool nz0 = ml[0] > 0, nz1 = ml[1] > 0;
	int32_t tot;
	uint32_t ee;  // the entries' first pieces, both rounds (inc* / np* end here)
	{
		const int32_t np0 = ring_piece_count(off[0], ml[0]), np1 = ring_piece_count(off[1], ml[1]);
		const int32_t inc0 = wave_incl_scan(np0);
		const int32_t tot0 = wave_last(inc0);
		const int32_t inc1 = tot0 + wave_incl_scan(np1);
		tot = wave_last(inc1);
		auto pack = [&](int32_t md, int32_t of, int32_t m, int32_t excl) -> uint64_t {
			return uint64_t(uint16_t(md - o_batch)) | (uint64_t(uint16_t(of)) << 16) |
			       (uint64_t(uint16_t(m)) << 32) | (uint64_t(uint16_t(excl)) << 48);
		};
		uint64_t* ldesc = ldesc_of(D);
		ldesc[lane] = pack(mdst[0], off[0], ml[0], inc0 - np0);
		ldesc[64 + lane] = pack(mdst[1], off[1], ml[1], inc1 - np1);
		ee = uint32_t(inc0 - np0) | (uint32_t(inc1 - np1) << 16);
	}
	for (int32_t t0 = 0; t0 < tot; t0 += 64) {
		const int32_t t = t0 + lane;
		const bool act = t < tot;
		const int32_t lo = min(chunk_owner_e(D, ee, nz0, nz1, t0), 127);
		const uint64_t dd = ldesc_of(D)[lo];
		const int32_t od = o_batch + int32_t(dd & 0xffffu);
		const int32_t ooff = int32_t((dd >> 16) & 0xffffu), oml = int32_t((dd >> 32) & 0xffffu);
		const int32_t k = t - int32_t(dd >> 48);
		const bool opat = ooff < 16 && ooff < oml;
		const int32_t ostp = opat ? pattern_step(ooff) : 16;
		const bool wide = !opat && oml > ooff;  // overlap with off >= 16
		const int32_t base = 2 * k * ostp;       // the piece's first output byte in its match
		const int32_t pd = od + base;
		const int32_t left = oml - base;
		const bool two = left > 16;
		// the exact-length store: the second unit's bytes, or the whole piece
		const int32_t pd2 = two ? pd + ostp : pd;
		const int32_t n2 = two ? min(16, left - ostp) : left;
		const int32_t pe_ = pd2 + n2;  // the piece writes [pd, pe_)
		// source bytes read: the whole period for patterns and overlaps
		const int32_t s_lo = (opat || wide) ? od - ooff : od - ooff + base;
		const int32_t s_hi = (opat || wide) ? od : s_lo + (pe_ - pd);
		// lanes of this chunk whose piece [pd, pe_) meets [s_lo, s_hi):
		// pd is monotone over the lanes, so two binary searches -- skipped
		// when every source ends before the chunk's first piece
		// (a piece's real end, not pd + 32: a short last piece must not hold
		// back a source that only starts after it)
		const int32_t pe = act ? pe_ : INT32_MAX, ps = act ? pd : INT32_MAX;
		int32_t fj1 = 64, fj2 = -1;  // the chunk's pieces that write this one's source (none)
		if (!__all(!act || s_hi <= wave_get(ps, 0))) {
			// the first probe's source is lane 31 in every lane: a readlane, not
			// an LDS shuffle.  wave_get's conditions hold: 31 is a constant, and
			// every lane computed pe and ps above (the chunk loop and this
			// branch are wave-uniform)
			int32_t j1 = wave_get(pe, 31) <= s_lo ? 32 : 0, c2 = wave_get(ps, 31) < s_hi ? 32 : 0;
#pragma unroll
			for (int st = 16; st >= 1; st >>= 1) {
				if (__shfl(pe, j1 + st - 1) <= s_lo)
					j1 += st;
				if (__shfl(ps, c2 + st - 1) < s_hi)
					c2 += st;
			}
			fj1 = j1;
			fj2 = min(c2 - 1, lane - 1);
		}
		uint64_t dep = 0;
		if (act && fj1 <= fj2)
			dep = (fj2 == 63 ? ~uint64_t(0) : ((uint64_t(2) << fj2) - 1)) & ~((uint64_t(1) << fj1) - 1);
		// the piece's reads, fixed before the steps: per unit 16 bytes at a
		// and, for an overlap with off >= 16 whose unit wraps the period, the
		// bytes from cut on at a - off.  The second unit begins 16 bytes on
		// in the period: at a1 + 16, or off before that once past its end.
		// The step loop is the kernel's register peak, and every address,
		// select and mask the loads and stores derive from these values
		// would be hoisted out of it, so they cross it packed in two
		// registers the compiler must take as changing (step_state): a step
		// unpacks what it needs.
		//   sa: a1 (ring address, 14 bits) | pd (ring address) << 14 | (ostp - 1) << 28
		//   sb: off | cut1 << 16 | cut2 << 21 | n2 << 26 | (the second unit wraps) << 31
		static_assert(omask_v<LD> < (1u << 14), "ring addresses pack into 14 bits");
		uint32_t sa, sb;
		{
			int32_t rem = 0;
			if (wide)
				div_small(base, ooff, rem);
			const int32_t a1 = opat ? od - ooff : (wide ? od - ooff + rem : s_lo);
			const int32_t cut1 = (wide && ooff - rem < 16) ? ooff - rem : 16;
			const bool wrap2 = wide && rem + 16 >= ooff;
			const int32_t rem2 = rem + 16 - (wrap2 ? ooff : 0);
			const int32_t cut2 = (wide && ooff - rem2 < 16) ? ooff - rem2 : 16;
			sa = (uint32_t(a1) & omask_of(D)) | ((uint32_t(pd) & omask_of(D)) << 14) | (uint32_t(ostp - 1) << 28);
			sb = uint32_t(ooff) | (uint32_t(cut1) << 16) | (uint32_t(cut2) << 21) | (uint32_t(max(n2, 0)) << 26) |
			     (uint32_t(wrap2) << 31);
		}
		const bool ld2 = two && !opat;  // a pattern's second unit is its first
		bool pend = act;
		for (;;) {
			const uint64_t pm = __ballot(pend);
			if (pm == 0)
				break;
			const bool ready = pend && (dep & pm) == 0;
			step_state(sa, sb);
			const int32_t xa1 = int32_t(sa & 0x3fffu), xpd = int32_t((sa >> 14) & 0x3fffu);
			const int32_t xoff = int32_t(sb & 0xffffu), xcut1 = int32_t((sb >> 16) & 31u);
			const int32_t xcut2 = int32_t((sb >> 21) & 31u), xn2 = int32_t((sb >> 26) & 31u);
			const int32_t xa2 = xa1 + 16 - (int32_t(sb) < 0 ? xoff : 0);
			const int32_t xpd2 = two ? xpd + int32_t(sa >> 28) + 1 : xpd;
			// Reads first.  Unit 1's read, unit 2's and the pattern selectors'
			// (their address needs only xoff) are issued here, before the
			// step's first store, and consumed below, so they are in flight
			// together and each use waits for its own (a counted lgkmcnt)
			// instead of paying a round trip of its own behind the store
			// before it.  The rule that makes it valid: no read of a ready
			// lane meets a store of this step.  Not its own piece's --
			// neither unit reads its own match's output (ring_match's rule)
			// -- and not another ready lane's: dep covers the sources of both
			// units, so two lanes ready in one step never read each other's
			// stores of that step.  The compiler cannot prove that two oring
			// addresses differ and would keep unit 2's read behind unit 1's
			// store; hence the order here.  (The wrap-merge reads of an
			// overlap stay where they are used: issued up here under their
			// predicates they measured slower, and so did unit 2's early
			// read in the branching form below, which keeps the plain
			// order; DESIGN.md §4.)
			if constexpr (lds_fast<LD>::value) {
				// every lane loads and stores (a lane not ready stores
				// nothing: its stores go to the junk bytes)
				u32x4 v = oload16(D, xa1);
				u32x4 w = oload16(D, xa2);
				const u32x4 sel = pattern_sel(opat ? xoff : 0, plut_of(D));
				if (ready && xcut1 < 16)
					v = merge_at(v, oload16(D, xa1 - xoff), xcut1);
				if (ready && opat)
					v = pattern_perm(v, xoff, sel);
				// unit 2's bytes are assembled before unit 1's store is issued:
				// placed after it, their wait would count the store as well
				asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(w.z), "+v"(w.w)::"memory");
				// the first unit of two: 16 whole bytes in one store (one wrapping
				// the ring's end takes ostore's byte loop)
				if (__builtin_expect(!__any(ready && two && uint32_t(xpd) + 16u > omask_of(D) + 1), 1))
					__builtin_memcpy((ready && two) ? &oring_of(D)[xpd] : junk_of(D), &v, 16);
				else
					ostore(D, xpd, v, (ready && two) ? 16 : 0);
				if (ready && ld2 && xcut2 < 16)
					w = merge_at(w, oload16(D, xa2 - xoff), xcut2);
				if (ld2)
					v = w;
				ostore(D, xpd2, v, ready ? xn2 : 0);
			} else if (ready) {
				u32x4 v = oload16(D, xa1);
				if (xcut1 < 16)
					v = merge_at(v, oload16(D, xa1 - xoff), xcut1);
				if (opat) {
					int32_t sstp;
					make_pattern16(uint64_t(v.x) | (uint64_t(v.y) << 32),
					               uint64_t(v.z) | (uint64_t(v.w) << 32), xoff, v, sstp);
				}
				if (two)
					ostore(D, xpd, v, 16);
				if (ld2) {
					v = oload16(D, xa2);
					if (xcut2 < 16)
						v = merge_at(v, oload16(D, xa2 - xoff), xcut2);
				}
				ostore(D, xpd2, v, xn2);
			}
			pend = pend && !ready;
			wave_lds_fence();
			++steps;
		}
	}
	return steps;
}

// Ring-sourced matches of a round of short matches, one lane each: those
// whose source is final before the round (or lies in their own literals)
// at once, a near match -- reading this round's match output -- once every
// lane whose output it reads is done (a 64-bit mask from two binary
// searches over the round's monotone match positions, one AND against a
// ballot per step).  rbeg: the round's first output position; L: this
// lane's literal length.
#ifndef LZ4ADA_RING_LANE_MAX
#define LZ4ADA_RING_LANE_MAX 32
#endif
constexpr int RING_LANE_MAX = LZ4ADA_RING_LANE_MAX;
template <class LD>
__device__ __forceinline__ int32_t ring_lanes(LD& D, int32_t mdst, int32_t off, int32_t ml,
                                           int32_t rbeg, int32_t L, int32_t glo = INT32_MIN)
{
	const int32_t lane = int32_t(lane_id());
	const int32_t src = mdst - off;
	const int32_t dep_end = src + min(off, ml);
	const bool far = ml > 0 && (dep_end <= rbeg || off <= L);
	int32_t steps = 0;  // store steps (diagnostic count)
	if (!__any(ml > 0 && !far)) {
		if (far)
			ring_match(D, mdst, off, ml);
		wave_lds_fence();
		return 0;
	}
	// with near matches, the far ones run in the first step with the near
	// ones that are ready (their sources are final: no producers), not in
	// a step of their own
	bool near = ml > 0;
	const int32_t mend = mdst + ml;
	// the first probe by readlane (lane 31 in every lane).  wave_get's
	// conditions hold: every lane holds its mdst and mend -- the caller
	// computes them for all 64 lanes, in wave-uniform control flow
	int32_t j1 = wave_get(mend, 31) <= src ? 32 : 0, c2 = wave_get(mdst, 31) < dep_end ? 32 : 0;
#pragma unroll
	for (int st = 16; st >= 1; st >>= 1) {
		if (__shfl(mend, j1 + st - 1) <= src)
			j1 += st;
		if (__shfl(mdst, c2 + st - 1) < dep_end)
			c2 += st;
	}
	int32_t fj1 = far ? 64 : j1, fj2 = far ? -1 : min(c2 - 1, lane - 1);
	// Forwarding (pointer jumping over the round's near matches): a plain
	// match (off >= ml) whose source lies inside ONE earlier near match P of
	// the round, P itself a plain copy, reads P's source instead -- byte x of
	// it is byte x - off - off_P -- and waits for P's producers instead of
	// for P.  Each round composes every lane's forwarding with its producer's
	// current one, so a chain of k dependent matches (text: matches copying
	// recent matches, ~17 in a row) takes ~log2 k rounds instead of k store
	// steps.  A source forwarded past glo (below the window's kept bytes)
	// stops there.
	int32_t fo = off;
	{
		const int32_t pm = __shfl(mdst, fj1), pe = __shfl(mend, fj1), po = __shfl(off, fj1);
		const bool pn = __shfl(int32_t(near), fj1) != 0;
		bool fw = FWD_ROUNDS > 0 && glo != INT32_MIN && near && off >= ml && fj1 == fj2 && pm <= src &&
		          dep_end <= pe && pn && po >= pe - pm;
		// (the producer's state is read before any lane updates its own:
		// synchronous rounds; P's identity out[y] = out[y - fo_P] holds for
		// whatever forwarding P has reached)
		for (int r = 0; r < FWD_ROUNDS && __any(fw); ++r) {
			const int32_t p = fj1;
			const int32_t qo = __shfl(fo, p), q1 = __shfl(fj1, p), q2 = __shfl(fj2, p);
			const bool qf = __shfl(int32_t(fw), p) != 0;
			if (fw && mdst - fo - qo >= glo) {
				fo += qo;
				fj1 = q1;  // P's producers (none: q1 > q2, the source is final)
				fj2 = q2;
				fw = qf;
			} else {
				fw = false;
			}
		}
	}
	uint64_t dep = 0;
	if (near && fj1 <= fj2)
		dep = (fj2 == 63 ? ~uint64_t(0) : ((uint64_t(2) << fj2) - 1)) & ~((uint64_t(1) << fj1) - 1);
	for (;;) {
		const uint64_t pending = __ballot(near);
		if (pending == 0)
			break;
		const bool ready = near && (dep & pending) == 0;
		if (ready) {
			ring_match(D, mdst, fo, ml);
			near = false;
		}
		wave_lds_fence();
		++steps;
	}
	return steps;
}

// Owner of piece t when lane i holds pieces [inc_i - cnt_i, inc_i) (inc: the
// wave's inclusive prefix sum of piece counts): the first lane with inc > t.
__device__ __forceinline__ int32_t piece_owner(int32_t inc, int32_t t)
{
	int32_t lo = 0;
#pragma unroll
	for (int st = 32; st >= 1; st >>= 1)
		if (__shfl(inc, lo + st - 1) <= t)
			lo += st;
	return lo;
}
