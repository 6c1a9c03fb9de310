// lz4ada_idx_pass1.inc -- part of lz4ada_idx.hip, which includes it inside namespace
// lz4ada::idx (one translation unit: the text below is that file's, moved):
// pass 1, the sequence index (index_block, k_index).

// ------------------------------------------------------------------ pass 1

// the 16-bit output counts of a lane's records: two to a dword, so the
// first walk can add into one with a 32-bit LDS add; read and written as
// halves everywhere else
typedef uint16_t __attribute__((may_alias)) cnt16;
typedef uint32_t __attribute__((may_alias)) cnt32;

// Pass 1 runs on the W waves of a block's workgroup (1: k_index and
// k_decode_idx; 2: k_decode_pp2): 64 * W lanes share each staged chunk.
template <int W>
struct Pass1 {
	static_assert(W == 1 || W == 2, "one or two waves per block");
	static constexpr int SEG = CHUNK / (64 * W);  // segment per lane
	static constexpr int NSUB = SEG / SUB;        // index records per segment
	static constexpr int STRIDE = 16 * 64 * W;    // bytes one 16-byte load per thread covers
	static constexpr int PF = CHUNK / STRIDE;     // 16-byte loads per thread per chunk
};

template <int W>
struct alignas(16) IdxLds {
	uint8_t buf[CHUNK + 16];                     // staged chunk; + mirror of its first 16 bytes
	uint32_t rbm[64 * W][Pass1<W>::NSUB + 1];    // each lane's records from its latest walk: start
	cnt32 rcnt[64 * W][Pass1<W>::NSUB / 2 + 1];  // bitmaps and output bytes (>= 0xFFFF: in HBM)
	// the exchange words of two waves (no bytes with one)
	int32_t xa[W - 1];        // wave 0's largest exit (wave 1's lane-0 entry)
	int32_t xs[W - 1][2][4];  // per wave: largest exit, sequence starts, bad, used sub-segments
};
static_assert(sizeof(IdxLds<1>) <= 20480, "8 waves per CU: at most 20 KiB of LDS per wave");

// a lane's counts as halves (record k: half k)
template <int N>
__device__ __forceinline__ cnt16* halves(cnt32 (&row)[N])
{
	return reinterpret_cast<cnt16*>(row);
}
template <int N>
__device__ __forceinline__ const cnt16* halves(const cnt32 (&row)[N])
{
	return reinterpret_cast<const cnt16*>(row);
}

// Walk the chain from e (an entry at or after this lane's segment start s)
// over the sequences starting before seg_end; returns the exit (first
// chain position >= seg_end, or n).  A malformed sequence sets err (epos:
// its position) and returns seg_end as a guess: from a wrong (speculative)
// entry that is just a dead chain, and a -1 would poison every lane after
// it one iteration at a time.
//
// Every walk rewrites the segment's NS records (sub-segment k = bytes
// [s + 32k, s + 32k + 32)) in LDS: rb[k] bit j = a sequence starts at byte
// j, rc[k] = the output bytes (literals + match) of the sequences starting
// there.  The lane's last walk -- from the true entry -- leaves the exact
// records; k_index writes them to HBM once per chunk.  An output count that
// does not fit 16 bits goes straight to its record's high word in HBM
// (ghi[2k]; long RLE runs).
//
// Re-walk (may_stop: the lane's previous walk, exit y_old, had no error):
// chains are deterministic, so once this walk reaches a position the
// previous walk started a sequence at, the rest is the previous walk.  It
// finishes that sub-segment (its count mixes both walks' sequences) and
// stops: later records and the exit are the previous walk's.  Chains from a
// wrong entry merge within ~14 sequences, so a re-walk costs a fraction of
// a segment.
template <int NS>
__device__ __forceinline__ int32_t walk_segment(const Src& S, int32_t e, int32_t s, int32_t seg_end,
                                                int32_t n, uint32_t* rb, cnt16* rc, uint32_t* ghi,
                                                bool& err, int32_t& epos, int32_t y_old,
                                                bool may_stop, int32_t& nst)
{
	nst = 0;  // sequence steps (diagnostic counts; dead in the product)
	err = false;
	epos = INT32_MAX;
	auto put = [&](int32_t k, uint32_t b, uint32_t c) {
		rb[k] = b;
		rc[k] = uint16_t(min(c, 0xFFFFu));
		if (c >= 0xFFFFu)
			ghi[2 * k] = c;
	};
	// the dword pair at pos, shifted to pos (LDS; a position outside the
	// staged window reads garbage, which parse_fast's window test rejects)
	auto pair_at = [&](int32_t pos) -> uint32_t {
		const uint32_t a = uint32_t(pos + S.mis) & S.mask;
		const uint32_t* wa = reinterpret_cast<const uint32_t*>(S.lds + (a & ~3u));
		return __builtin_amdgcn_alignbyte(wa[1], wa[0], a & 3u);
	};
	int32_t p = e;
	int32_t kc = -1, nxt = 0;  // sub-segment being counted; next record to write
	uint32_t bm = 0, cnt = 0;
	bool merged = false;
	uint32_t w = p < seg_end ? pair_at(p) : 0u;  // token pair of the sequence at p
	while (p < seg_end) {
		const int32_t k = (p - s) >> 5;
		if (k != kc) {
			if (kc >= 0)
				put(kc, bm, cnt);
			if (merged)
				return y_old;
			for (; nxt < k; ++nxt)
				if (nxt != kc)
					put(nxt, 0, 0);
			nxt = k + 1;
			kc = k;
			bm = cnt = 0;
		}
		const uint32_t bit = 1u << ((p - s) & 31);
		if (may_stop && (rb[k] & bit))
			merged = true;  // rb[k] is still the previous walk's record
		bm |= bit;
		++nst;
		// parse_fast from the token pair in hand; the offset pair at x and
		// the next sequence's token pair load together (the next position
		// needs only this token), so a step waits for one LDS round trip
		const uint32_t tk = w & 0xffu, e1 = (w >> 8) & 0xffu;
		const bool x1 = tk >= 0xf0u, x2 = (tk & 15u) == 15u;
		const int32_t L = int32_t(tk >> 4) + (x1 ? int32_t(e1) : 0);
		const int32_t x = p + 1 + (x1 ? 1 : 0) + L;
		const int32_t np = x + 2 + (x2 ? 1 : 0);
		const uint32_t w2 = pair_at(x), wn = pair_at(np);
		const uint32_t e2 = (w2 >> 16) & 0xffu;
		Seq q;
		q.L = L;
		q.ml = int32_t(tk & 15u) + 4 + (x2 ? int32_t(e2) : 0);
		q.next = np;
		const bool ok = p >= S.lo && x + 8 <= S.hi && x + 8 <= n && !(x1 && e1 == 255u) &&
		                !(x2 && e2 == 255u) && (w2 & 0xffffu) != 0;
		if (!ok) {  // rare shapes (and malformed data): the exact parse
			if (!parse_seq(S, p, n, q)) {
				err = true;
				epos = p;
				return seg_end;
			}
		}
		cnt += uint32_t(q.L + q.ml);
		p = q.next;
		w = ok ? wn : pair_at(p);
	}
	if (kc >= 0)
		put(kc, bm, cnt);
	if (!merged)
		for (; nxt < NS; ++nxt)
			put(nxt, 0, 0);
	return p;
}

// A lane's first walk of a chunk: walk_segment(may_stop = false) from an
// entry e >= s, leaving exactly the records it would, with the per-step
// bookkeeping (the sub-segment transition, the zero fill, the merge tests)
// replaced by two LDS read-modify-writes into rows zeroed up front: the
// start bit is OR-ed into rb[k], L + ml added to the 16-bit half k of rc
// (no other lane touches the row, and a wave's LDS operations execute in
// order).  Positions are buffer offsets (the staged chunk is linear here:
// byte p at buf[p - S.lo]), so no read wraps; one past the staged bytes
// returns other LDS contents, which the window test rejects.
//
// A sub-segment starts at most 11 sequences the branch-free parse accepts
// (3 bytes or more each, L <= 269, ml <= 273), so their sum cannot carry
// out of its half.  The first sequence it rejects (a longer length extension, bytes
// past the staged window, the block's last sequences, malformed data) ends
// the adds for its sub-segment: the rest of that sub-segment goes through
// parse_seq with an exact 32-bit count, stored saturated with the exact
// value in HBM as walk_segment's put() does.
template <int NS>
__device__ __forceinline__ int32_t walk_first(const Src& S, int32_t e, int32_t s, int32_t seg_end,
                                              int32_t n, uint32_t* rb, cnt32* rc, uint32_t* ghi,
                                              bool& err, int32_t& epos, int32_t& nst)
{
	static_assert(NS % 2 == 0, "two counts to a dword");
	nst = 0;
	err = false;
	epos = INT32_MAX;
#pragma unroll
	for (int k = 0; k < NS; ++k)
		rb[k] = 0;
#pragma unroll
	for (int k = 0; k < NS / 2; ++k)
		rc[k] = 0;
	const uint8_t* buf = S.lds;
	auto pair_at = [&](int32_t P) -> uint32_t {
		const uint32_t a = uint32_t(P);
		const uint32_t* wa = reinterpret_cast<const uint32_t*>(buf + (a & ~3u));
		return __builtin_amdgcn_alignbyte(wa[1], wa[0], a & 3u);
	};
	const int32_t B = S.lo;
	const int32_t S0 = s - B, END = seg_end - B;
	const int32_t LIM8 = min(S.hi, n) - 8 - B;  // the latest x with 8 staged bytes inside the block
	int32_t P = e - B;                          // e >= s >= S.lo
	uint32_t w = P < END ? pair_at(P) : 0u;
	while (P < END) {
		const uint32_t d = uint32_t(P - S0);
		const uint32_t k = d >> 5, bit = 1u << (d & 31u);
		++nst;
		const uint32_t tk = w & 0xffu, e1 = (w >> 8) & 0xffu;
		const bool x1 = tk >= 0xf0u, x2 = (tk & 15u) == 15u;
		const int32_t L = int32_t(tk >> 4) + (x1 ? int32_t(e1) : 0);
		const int32_t x = P + 1 + (x1 ? 1 : 0) + L;
		const int32_t np = x + 2 + (x2 ? 1 : 0);
		// the offset pair at x and the next token pair load together, before
		// the branch below (left to the compiler, the second read sinks past
		// it and a step waits for two LDS round trips)
		const uint32_t w2 = pair_at(x), wn = pair_at(np);
		asm volatile("" ::"v"(wn));
		const uint32_t e2 = (w2 >> 16) & 0xffu;
		const uint32_t c =uint32_t(L) + (tk & 15u) + 4u + (x2 ? e2 : 0u);
		const bool ok = x <= LIM8 && !(x1 && e1 == 255u) && !(x2 && e2 == 255u) && (w2 & 0xffffu) != 0;
		if (__builtin_expect(!ok, 0)) {
			const uint32_t sh = (k & 1u) * 16u;
			const uint32_t old = (__hip_atomic_load(&rc[k >> 1], __ATOMIC_RELAXED,
			                                        __HIP_MEMORY_SCOPE_WAVEFRONT) >> sh) & 0xffffu;
			uint32_t bm = 0, cnt = old;
			int32_t p = P + B;
			do {
				Seq q;
				if (!parse_seq(S, p, n, q)) {
					err = true;
					epos = p;
					return seg_end;
				}
				bm |= 1u << (uint32_t(p - s) & 31u);
				cnt += uint32_t(q.L + q.ml);
				p = q.next;
				if (p < seg_end && uint32_t(p - s) >> 5 == k)
					++nst;
				else
					break;
			} while (true);
			__hip_atomic_fetch_or(&rb[k], bm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
			__hip_atomic_fetch_add(&rc[k >> 1], (min(cnt, 0xFFFFu) - old) << sh, __ATOMIC_RELAXED,
			                       __HIP_MEMORY_SCOPE_WAVEFRONT);
			if (cnt >= 0xFFFFu)
				ghi[2 * k] = cnt;
			P = p - B;
			w = P < END ? pair_at(P) : 0u;
			continue;
		}
		__hip_atomic_fetch_or(&rb[k], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
		__hip_atomic_fetch_add(&rc[k >> 1], c << ((k & 1u) * 16u), __ATOMIC_RELAXED,
		                       __HIP_MEMORY_SCOPE_WAVEFRONT);
		P = np;
		w = wn;
	}
	return P + B;
}

// The chain position after the sequence at buffer offset P (the staged
// chunk is linear: byte p at buf[p - S.lo]), for the lead-in walk: only a
// guess, so no checks, and every length extension taken as one byte (a
// longer one just makes a wrong guess, which the re-walks fix) -- then the
// token and the byte after it are all a step reads, with no address
// arithmetic: the lead-in keeps P itself.
__device__ __forceinline__ int32_t skip_seq(const uint8_t* buf, int32_t P)
{
	const uint32_t tk = buf[P], e1 = buf[P + 1];
	const int32_t x1 = tk >= 0xf0u ? 1 : 0;
	const int32_t L = int32_t(tk >> 4) + (x1 ? int32_t(e1) : 0);
	return P + 3 + x1 + L + ((tk & 15u) == 15u ? 1 : 0);
}

// The lead-in of a lane whose segment starts at s > C: from `lead` bytes
// before s (inside the staged chunk), the first guessed chain position >= s.
__device__ __forceinline__ int32_t lead_in_walk(const Src& S, int32_t C, int32_t s, int32_t lead)
{
	const int32_t S0 = s - S.lo;
	int32_t P = max(s - lead, C) - S.lo;
	while (P < S0)
		P = skip_seq(S.lds, P);
	return P + S.lo;
}

__device__ __forceinline__ int32_t lead_in_bytes(int32_t starts)
{
	const int32_t l = LEAD_SEQ * (CHUNK / max(starts, 1));
	return __builtin_amdgcn_readfirstlane(min(max(l, LEAD_MIN), LEAD_MAX));
}

// Pass 1 of block b by the W waves of its workgroup (the body of k_index;
// the fused kernels run it before pass 2 of the same block: k_decode_idx
// with one wave, k_decode_pp2 with two).  With two waves, 128 lanes walk
// each chunk, 128 bytes each: wave 0's lane 0 enters at the exact chain
// position, wave 1's lane 0 at its lead-in guess until wave 0's exit is
// known (one LDS exchange per chunk), and the chunk's totals are combined
// through LDS; one wave keeps everything in registers.
template <int W>
__device__ __forceinline__ void index_block(IdxLds<W>& X, const uint8_t* __restrict__ frame,
                                            uint64_t frame_len,
                                            const lz4ada_block_desc* __restrict__ desc, uint32_t b,
                                            uint8_t* __restrict__ tab_all,
                                            lz4ada_block_status* __restrict__ status)
{
	constexpr int SEG = Pass1<W>::SEG, NSUB = Pass1<W>::NSUB, PF = Pass1<W>::PF, STRIDE = Pass1<W>::STRIDE;
	const int32_t tid = int32_t(threadIdx.x) & (64 * W - 1);  // thread of the block's workgroup
	const int32_t w = tid >> 6, lane = tid & 63;               // its wave, its lane
	const lz4ada_block_desc d = desc[b];
	if (d.flags & LZ4ADA_BLOCK_STORED) {
		if (tid == 0)
			status[b].code = DS_OK;
		return;
	}
	if (d.in_len >= RLE_MIN_IN && uint64_t(d.in_len) * RLE_RATIO < uint64_t(d.out_cap)) {
		if (tid == 0)
			status[b].code = DS_SPARSE;
		return;
	}
	cg8* in = gptr(frame) + d.in_off;
	const int32_t n = int32_t(d.in_len);
	const uintptr_t lim = reinterpret_cast<uintptr_t>(frame) + frame_len;
	const int32_t mis = int32_t(reinterpret_cast<uintptr_t>(in) & 15u);
	uint64_t* tab = reinterpret_cast<uint64_t*>(tab_all) + (((d.in_off >> 8) + b) << 3);

	Src S;
	S.lds = X.buf;
	S.mask = CHUNK - 1;
	S.mis = mis;
	S.in = in;
	S.lim = lim;

	// 16 KiB chunk at aligned address a (threads: PF x 16 bytes each), the
	// next one loaded while the current one is walked
	auto load16k = [&](uintptr_t a, u32x4 (&v)[PF]) {
		if (a + CHUNK <= lim) {
#pragma unroll
			for (int r = 0; r < PF; ++r)
				__builtin_memcpy(&v[r], reinterpret_cast<cg8*>(a + uintptr_t(STRIDE * r + 16 * tid)), 16);
		} else {
#pragma unroll
			for (int r = 0; r < PF; ++r)
				v[r] = gload16(a + uintptr_t(STRIDE * r + 16 * tid), lim);
		}
	};
	const uintptr_t abase = reinterpret_cast<uintptr_t>(in) - uintptr_t(mis);
	u32x4 pf[PF];
	if (n > 0)
		load16k(abase, pf);

	ISTAMP_DECL;
	int32_t E = 0;  // exact chain entry of the current chunk
	int32_t lead = LEAD_IN0;  // lead-in bytes (from the previous chunk's density)
	bool bad = false;
	bool sparse = false;  // declined as literal-heavy (k_decode_sparse takes it)
	for (int32_t C = 0; C < n && !bad; C += CHUNK) {
		// stage block-relative [C - mis, C - mis + CHUNK) (16-byte aligned addresses)
#pragma unroll
		for (int r = 0; r < PF; ++r)
			*reinterpret_cast<u32x4*>(&X.buf[STRIDE * r + 16 * tid]) = pf[r];
		if (tid == 0)
			*reinterpret_cast<u32x4*>(&X.buf[CHUNK]) = pf[0];
		__syncthreads();
		if (C + CHUNK < n)
			load16k(abase + uintptr_t(C + CHUNK), pf);
		S.lo = C - mis;
		S.hi = C - mis + CHUNK;
		ISTAMP(I_STAGE);
		ICOUNT(I_CHUNKS, 1);

		const int32_t s = C + SEG * tid;
		const int32_t seg_end = min(s + SEG, n);
		// Entry of lane i = max exit of lanes < i (lane 0: the exact entry E).
		// True exits never decrease along the chunk, so the fixed point is
		// the true chain, and a run of segments a long sequence jumps over
		// is crossed in one step instead of one iteration per segment.
		int32_t ein = (tid == 0) ? E : s;
		if (tid > 0 && s < n) {
			// Lead-in: walk from OV bytes before the segment to find a
			// likelier entry than s itself -- chains from a wrong start merge
			// with the true one within ~14 sequences, so by s this one mostly
			// has, and the re-walk rounds below (most of pass 1's time) are
			// rarely needed.
			ein = lead_in_walk(S, C, s, lead);
		}
		ISTAMP(I_LEAD);
		uint32_t* ghi = reinterpret_cast<uint32_t*>(tab + (C >> 5) + NSUB * tid) + 1;
		int32_t epos = INT32_MAX;
		bool err = false;
		int32_t nst = 0;
		int32_t y = (s < n) ? walk_first<NSUB>(S, ein, s, seg_end, n, X.rbm[tid], X.rcnt[tid], ghi, err,
		                                       epos, nst)
		                    : ein;
		ISTAMP(I_WALK0);
		ICOUNT(I_STEPS, wave_last(wave_incl_scan(nst)));
		ICOUNT(I_MAXST, wave_last(wave_incl_max(nst)));
		// this wave's lane-0 entry: the exact one, but for wave 1 its lead-in
		// guess until wave 0's largest exit is known
		int32_t e0 = E;
		if constexpr (W == 2)
			e0 = __shfl(ein, 0);
		auto converge = [&]() {
			for (int it = 0; it < 64; ++it) {
				int32_t prev = __shfl_up(wave_incl_max(y), 1);
				if (lane == 0)
					prev = e0;
				const bool changed = prev != ein;
				if (!__any(changed))
					break;
				ICOUNT(I_ITERS, 1);
				nst = 0;
				if (changed) {
					ein = prev;
					if (s < n) {
						y = walk_segment<NSUB>(S, ein, s, seg_end, n, X.rbm[tid], halves(X.rcnt[tid]), ghi,
						                       err, epos, y, !err, nst);
					} else {
						y = ein;
						err = false;
					}
				}
				ICOUNT(I_STEPS, wave_last(wave_incl_scan(nst)));
				ICOUNT(I_MAXST, wave_last(wave_incl_max(nst)));
			}
		};
		converge();
		if constexpr (W == 2) {
			const int32_t mx = wave_last(wave_incl_max(y));
			if (tid == 0)
				X.xa[0] = mx;
			__syncthreads();
			if (w == 1) {
				const int32_t ea = X.xa[0];
				if (ea != e0) {  // the guess missed: the lanes it reached walk again
					e0 = ea;
					converge();
				}
			}
		}
		ISTAMP(I_ITER);
		// converged: every entry is the true chain position, and every
		// lane's records are those of its last walk: to HBM, coalesced
		bad = __any(s < n && err);
		wave_lds_fence();
		int32_t starts = 0;  // sequence starts in this chunk (sizes the next lead-in)
#pragma unroll
		for (int i = 0; i < NSUB; ++i) {
			// this wave's record q (segment sg, sub-segment sb), the chunk's record r
			const int32_t q = 64 * i + lane, sg = 64 * w + q / NSUB, sb = q & (NSUB - 1);
			const int32_t r = W == 2 ? q + 256 * w : q;
			if (C + SEG * sg < n) {
				const uint32_t bmv = X.rbm[sg][sb], c16 = halves(X.rcnt[sg])[sb];
				starts += __popc(bmv);
				if (c16 != 0xFFFFu)
					tab[(C >> 5) + r] = uint64_t(bmv) | (uint64_t(c16) << 32);
				else  // the exact count is in the high word already
					*reinterpret_cast<uint32_t*>(tab + (C >> 5) + r) = bmv;
			}
		}
		// Sparse chains (over 64 input bytes per sequence: long literal
		// runs) defeat the speculative walks -- every segment's guess
		// misses and the entries crawl one lane per iteration -- and are
		// the one-wave scalar parse's best case: decline the block (large
		// blocks only: a short one costs a few chunks either way).
		const bool sparse_test = C == 0 && n >= 4 * CHUNK;
		int32_t used = 0;  // sub-segments holding a sequence start
		E = wave_last(wave_incl_max(y));
		starts = wave_last(wave_incl_scan(starts));
		if (sparse_test) {
			if (s < n)
				for (int k = 0; k < NSUB; ++k)
					used += X.rbm[tid][k] ? 1 : 0;
			used = wave_last(wave_incl_scan(used));
		}
		if constexpr (W == 2) {  // the chunk's totals over both waves
			if (lane == 0) {
				X.xs[0][w][0] = E;
				X.xs[0][w][1] = starts;
				X.xs[0][w][2] = bad ? 1 : 0;
				X.xs[0][w][3] = used;
			}
			__syncthreads();  // also: every read of this chunk's staging is done
			E = max(X.xs[0][0][0], X.xs[0][1][0]);
			starts = X.xs[0][0][1] + X.xs[0][1][1];
			bad = (X.xs[0][0][2] | X.xs[0][1][2]) != 0;
			used = X.xs[0][0][3] + X.xs[0][1][3];
		}
		lead = lead_in_bytes(starts);
		if (sparse_test && !bad && used < CHUNK / SUB / 4)
			bad = sparse = true;
		if constexpr (W == 1)
			__syncthreads();  // the next chunk overwrites the staging buffer
	}
	if (E != n)
		bad = true;
	if (tid == 0)
		status[b].code = bad ? (sparse ? DS_SPARSE : DS_RETRY) : DS_OK;
	ISTAMP_FLUSH();
}

// Pass 1 alone, 64 * W threads per block.  The product launches W = 1;
// W = 2 puts k_decode_pp2's pass 1 under the table test.
template <int W>
__global__ __launch_bounds__(64 * W) void k_index(const uint8_t* __restrict__ frame, uint64_t frame_len,
                                                   const lz4ada_block_desc* __restrict__ desc,
                                                   uint32_t nblocks, uint8_t* __restrict__ tab_all,
                                                   lz4ada_block_status* __restrict__ status)
{
	__shared__ IdxLds<W> X;
	if (blockIdx.x < nblocks)
		index_block<W>(X, frame, frame_len, desc, blockIdx.x, tab_all, status);
}
