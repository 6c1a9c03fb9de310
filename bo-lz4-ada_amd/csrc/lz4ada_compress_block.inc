// lz4ada_compress_block.inc -- the matching rule of lz4ada_compress_host.cpp read
// 64 positions at a time, one wave per block: the one device body of
// k_compress_blocks, k_compress_blocks_dict and k_compress_blocks_linked
// (DESIGN.md §17, §18, §21), stated once and included as the body of each.  A
// kernel names its history, `constexpr CompHist H`, and has in scope d_in, blk,
// nblocks, slots, csize and, as parameters or as null constants where its history
// never reads them, jobs, d_tail, dict_len, seed.  (Included, not called: as an
// inlined function the same text compiles to other code, which measured slower
// than the parent's range on five rows, 0.36 % on 4,096 records of 153,600 bytes
// (profiles/compress_one_body_ab.txt); included it compiles to the code each
// kernel had when it held its own copy.)  As on the host, a dictionary or a
// linked record is this body "called with another history"; what lies at
// [-dl, 0) in front of a block is decided at compile time, so a kernel carries
// only what its history needs:
//  * CompHist::None   -- nothing: dl is the constant 0, the table starts zeroed
//    and no history pointer is formed;
//  * CompHist::Dict   -- the dictionary's used tail D (dl = 4 .. 65,536 bytes at
//    d_tail): the table starts as a copy of the seeded one
//    (k_compress_dict_table), a candidate below 0 reads its four bytes from D,
//    and the extension's candidate dword is read at a virtual position -- from
//    the record at y >= 0, from D at y <= -4, byte by byte in between (one lane
//    per step at most lies astride);
//  * CompHist::Linked -- per block, by its place in its record: block 0 as None
//    (dict_len == 0) or Dict; block i >= 1 has the 65,536 bytes of its own
//    record in front of it in d_in.  Its wave seeds its own table: every q of
//    [-65536, -4], 64 consecutive positions per step, SEED_DEPTH steps' loads in
//    flight, by atomicMax of q + 65536 + 1 (positions only grow, so the maximum
//    is the latest, as in the serial statement's ascending loop).  That history
//    is contiguous with the block, so a candidate below 0 and the extension
//    read straight through position 0.
// The window's lookups are one LDS read per lane, the lowest valid lane is a
// ballot, the inserts are ds_max_u32 (two lanes with one hash: the higher
// position stays, as the serial loop's later store), the match is extended 256
// bytes per step.  The block goes into a scratch slot of its own; a block that
// would not come out shorter than it went in stops there and is marked stored.
// The body waits for no other workgroup; every loop is bounded by the block
// length, the dictionary's or 65,536.
	__shared__ __attribute__((aligned(16))) uint32_t table[COMP_TABLE];  // virtual position + dl + 1; 0: none
	const uint32_t b = blockIdx.x;
	if (b >= nblocks)
		return;
	const uint32_t lane = lane_id();
	const uint64_t in_off = wave_uniform(blk[b].in_off), slot_off = wave_uniform(blk[b].slot_off);
	const int32_t n = wave_uniform(int32_t(blk[b].len));
	// a block that does not begin its record lies a whole number of block
	// lengths (>= 65,536 each) into it
	bool cont = false;
	if constexpr (H == CompHist::Linked)
		cont = in_off != wave_uniform(jobs[wave_uniform(blk[b].job)].in_off);
	int32_t dl = 0;  // 0, or 4 .. 65,536
	if constexpr (H != CompHist::None)
		dl = cont ? int32_t(COMP_LINK_WINDOW) : wave_uniform(int32_t(dict_len));
	cg8* const src = gptr(d_in) + in_off;
	// virtual position 0 of the history: hst[x], -dl <= x < 0 (never read when dl == 0)
	cg8* hst = src;
	if constexpr (H != CompHist::None)
		hst = cont ? src : gptr(d_tail) + dl;
	// where virtual position x lies, -dl <= x < n (without a history that is src + x, and is written so)
	auto at = [&](int32_t x) -> cg8* { return x < 0 ? hst + x : src + x; };
	g8* const dst = gptr(slots) + slot_off;
	const int32_t cap = n - 1;  // compressed only when shorter than the block; the slot holds n bytes

	// ---- the table's start: the dictionary's seeded one, or empty and, in a
	// continuation block, seeded by this wave from the record
	if (H == CompHist::Dict || (H == CompHist::Linked && !cont && dl)) {
		const GLOBAL u32x4* const s4 = reinterpret_cast<const GLOBAL u32x4*>(gptr(seed));
		u32x4* const t4 = reinterpret_cast<u32x4*>(table);
		for (uint32_t i = lane; i < COMP_TABLE / 4; i += 64)
			t4[i] = s4[i];
	} else {
		for (uint32_t i = lane; i < COMP_TABLE; i += 64)
			table[i] = 0;
	}
	__syncthreads();
	if constexpr (H == CompHist::Linked) {
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
	}

	int32_t op = 0, anchor = 0;
	bool stored = false;
	if (n >= COMP_MIN_BLOCK) {
		const int32_t mlast = n - int32_t(COMP_MFLIMIT), mend = n - int32_t(COMP_LAST_LITERALS);
		int32_t w = 0;
		while (w <= mlast) {  // every turn moves w on by a window or a match
			// ---- the window's lookup and insert
			const int32_t wn = min(mlast - w + 1, int32_t(COMP_WINDOW));
			const int32_t p = w + int32_t(lane);
			const bool active = int32_t(lane) < wn;
			const uint32_t v = active ? ld32u_cached(src + p) : 0u;
			const uint32_t h = comp_hash(v);
			const uint32_t e = active ? table[h] : 0u;  // read before any position of the window is inserted
			const int32_t c = int32_t(e) - 1 - dl;      // -dl <= c <= -4 (seeded) or 0 <= c < w
			bool ok = e != 0 && p - c <= int32_t(COMP_MAX_OFF);
			if (ok)  // without a history c is e - 1, unsigned: no sign extension in the window's loop
				ok = ld32u_cached(H == CompHist::None ? src + (e - 1) : at(c)) == v;
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
			// ---- the extension: 4 bytes per lane, the first lane with a
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
					if constexpr (H == CompHist::None) {
						x = ld32u_cached(src + q) ^ ld32u_cached(src + y);
					} else {
						uint32_t cv;
						if (cont || y >= 0 || y <= -4) {
							cv = ld32u_cached(at(y));
						} else {
							cv = 0;
							for (int32_t k = 0; k < 4; ++k)
								cv |= uint32_t(*at(y + k)) << (8 * k);
						}
						x = ld32u_cached(src + q) ^ cv;
					}
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
			// ---- the sequence
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
	// ---- the last literals
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
