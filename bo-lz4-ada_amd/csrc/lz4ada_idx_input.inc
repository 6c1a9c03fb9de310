// lz4ada_idx_input.inc -- part of lz4ada_idx.hip, which includes it inside namespace
// lz4ada::idx (one translation unit: the text below is that file's, moved):
// input access (the staged input ring or HBM) and sequence parsing.

// ---------------------------------------------------------------- byte access
// Block-relative byte p comes from LDS when [p, p+8) lies in the staged
// window [lo, hi), else from global memory (guarded by the frame end).
struct Src {
	const uint8_t* lds;  // LDS array; block-relative p at lds[(p + mis) & mask]
	uint32_t mask;       // LDS array size - 1 (power of two; a 16-byte mirror follows)
	int32_t mis;
	int32_t lo, hi;
	cg8* in;
	uintptr_t lim;
};

__device__ __forceinline__ uint32_t fetch4(const Src& S, int32_t p)
{
	if (p >= S.lo && p + 8 <= S.hi) {
		const uint32_t a = uint32_t(p + S.mis) & S.mask;
		const uint32_t* w = reinterpret_cast<const uint32_t*>(S.lds + (a & ~3u));
		const uint32_t w0 = w[0], w1 = w[1];  // w[1] may be in the mirror
		return __builtin_amdgcn_alignbyte(w1, w0, a & 3u);
	}
	const uintptr_t g = reinterpret_cast<uintptr_t>(S.in) + uintptr_t(intptr_t(p));
	uint32_t v = 0;
#pragma unroll
	for (int i = 0; i < 4; ++i)
		if (g + i < S.lim)
			v |= uint32_t(*reinterpret_cast<cg8*>(g + i)) << (8 * i);
	// settle this rare path's loads here: left pending, they make every
	// merge after it (the walk loops' heads) wait for all memory, the
	// in-flight next-chunk prefetch included
	__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
	return v;
}

// 16 bytes at byte a of a power-of-two LDS ring (mask = size - 1): three
// 8-byte-aligned ds_read_b64 (each wrapped on its own), a one-bit dword
// select and four v_alignbyte -- ld16u's select network costs ~4x the VALU.
__device__ __forceinline__ u32x4 ring16(const uint8_t* base, uint32_t a, uint32_t mask)
{
	const uint32_t a8 = a & ~7u;
	const uint64_t q0 = *reinterpret_cast<const uint64_t*>(base + (a8 & mask));
	const uint64_t q1 = *reinterpret_cast<const uint64_t*>(base + ((a8 + 8) & mask));
	const uint64_t q2 = *reinterpret_cast<const uint64_t*>(base + ((a8 + 16) & mask));
	const uint32_t w0 = uint32_t(q0), w1 = uint32_t(q0 >> 32), w2 = uint32_t(q1),
	               w3 = uint32_t(q1 >> 32), w4 = uint32_t(q2), w5 = uint32_t(q2 >> 32);
	const bool s1 = (a & 4u) != 0;
	const uint32_t d0 = s1 ? w1 : w0, d1 = s1 ? w2 : w1, d2 = s1 ? w3 : w2, d3 = s1 ? w4 : w3,
	               d4 = s1 ? w5 : w4;
	const uint32_t sh = a & 3u;
	u32x4 v;
	v.x = __builtin_amdgcn_alignbyte(d1, d0, sh);
	v.y = __builtin_amdgcn_alignbyte(d2, d1, sh);
	v.z = __builtin_amdgcn_alignbyte(d3, d2, sh);
	v.w = __builtin_amdgcn_alignbyte(d4, d3, sh);
	return v;
}

// 16 bytes at block-relative p (literal source): LDS or global.
__device__ __forceinline__ u32x4 fetch16(const Src& S, int32_t p)
{
	if (p >= S.lo && p + 16 <= S.hi)
		return ring16(S.lds, uint32_t(p + S.mis) & S.mask, S.mask);
	const uintptr_t g = reinterpret_cast<uintptr_t>(S.in) + uintptr_t(intptr_t(p));
	u32x4 v;
	if (g + 16 <= S.lim) {
		__builtin_memcpy(&v, reinterpret_cast<cg8*>(g), 16);
	} else {
		uint8_t t[16];
		for (int i = 0; i < 16; ++i)
			t[i] = (g + i < S.lim) ? *reinterpret_cast<cg8*>(g + i) : 0;
		__builtin_memcpy(&v, t, 16);
	}
	// settle the rare global read here (see fetch4): otherwise every use of
	// the LDS path's result waits for all memory -- the batch's in-flight
	// HBM match loads and flush stores included
	__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
	return v;
}

struct Seq {
	int32_t lit, L, off, ml, next;  // ml = 0: literal-only last sequence
};

// One sequence at block-relative p < n (Decompress_Sequence,
// lz4ada.adb:737-777, with the end-of-block rule of :748-764).  False on
// any malformed shape; the caller then declines the block.
__device__ __forceinline__ bool parse_seq(const Src& S, int32_t p, int32_t n, Seq& q)
{
	const uint32_t w = fetch4(S, p);
	const int32_t tk = int32_t(w & 0xffu);
	int32_t L = tk >> 4, M = tk & 15, x = p + 1;
	if (L == 15) {
		uint32_t e, k = 1, ww = w;
		do {
			if (x >= n || L > n)
				return false;
			if (k > 3) {
				ww = fetch4(S, x);
				k = 0;
			}
			e = (ww >> (8 * k)) & 0xffu;
			++k;
			++x;
			L += int32_t(e);
		} while (e == 255u);
	}
	q.lit = x;
	q.L = L;
	x += L;
	if (x >= n) {
		if (x > n || M != 0)
			return false;
		q.off = 0;
		q.ml = 0;
		q.next = n;
		return true;
	}
	if (x + 1 >= n)
		return false;
	uint32_t w2 = fetch4(S, x);
	q.off = int32_t(w2 & 0xffffu);
	if (q.off == 0)
		return false;
	x += 2;
	if (M == 15) {
		uint32_t e, k = 2;
		do {
			if (x >= n || M > MAX_RUN)
				return false;
			if (k > 3) {
				w2 = fetch4(S, x);
				k = 0;
			}
			e = (w2 >> (8 * k)) & 0xffu;
			++k;
			++x;
			M += int32_t(e);
		} while (e == 255u);
	}
	q.ml = M + 4;
	q.next = x;
	return true;
}

// parse_seq for the common shape, without branches: both length
// extensions at most one byte, every byte read in the LDS window, the
// sequence well before the block end.  Anything else (and malformed data)
// takes parse_seq; the result is the same.
__device__ __forceinline__ bool parse_fast(const Src& S, int32_t p, int32_t n, Seq& q)
{
	const uint32_t a = uint32_t(p + S.mis) & S.mask;
	const uint32_t* wa = reinterpret_cast<const uint32_t*>(S.lds + (a & ~3u));
	const uint32_t w = __builtin_amdgcn_alignbyte(wa[1], wa[0], a & 3u);
	const uint32_t tk = w & 0xffu, e1 = (w >> 8) & 0xffu;
	const bool x1 = tk >= 0xf0u, x2 = (tk & 15u) == 15u;
	const int32_t L = int32_t(tk >> 4) + (x1 ? int32_t(e1) : 0);
	const int32_t lit = p + 1 + (x1 ? 1 : 0);
	const int32_t x = lit + L;
	const uint32_t b = uint32_t(x + S.mis) & S.mask;
	const uint32_t* wb = reinterpret_cast<const uint32_t*>(S.lds + (b & ~3u));
	const uint32_t w2 = __builtin_amdgcn_alignbyte(wb[1], wb[0], b & 3u);
	const uint32_t e2 = (w2 >> 16) & 0xffu;
	q.lit = lit;
	q.L = L;
	q.off = int32_t(w2 & 0xffffu);
	q.ml = int32_t(tk & 15u) + 4 + (x2 ? int32_t(e2) : 0);
	q.next = x + 2 + (x2 ? 1 : 0);
	const bool ok = p >= S.lo && x + 8 <= S.hi && x + 8 <= n && !(x1 && e1 == 255u) &&
	                !(x2 && e2 == 255u) && q.off != 0;
	if (__builtin_expect(ok, 1))
		return true;
	return parse_seq(S, p, n, q);
}

// parse_fast's branch-free form alone: false where it does not apply (the
// caller then runs parse_seq for that sequence; q is a placeholder)
__device__ __forceinline__ bool parse_fast_try(const Src& S, int32_t p, int32_t n, Seq& q)
{
	const uint32_t a = uint32_t(p + S.mis) & S.mask;
	const uint32_t* wa = reinterpret_cast<const uint32_t*>(S.lds + (a & ~3u));
	const uint32_t w = __builtin_amdgcn_alignbyte(wa[1], wa[0], a & 3u);
	const uint32_t tk = w & 0xffu, e1 = (w >> 8) & 0xffu;
	const bool x1 = tk >= 0xf0u, x2 = (tk & 15u) == 15u;
	const int32_t L = int32_t(tk >> 4) + (x1 ? int32_t(e1) : 0);
	const int32_t lit = p + 1 + (x1 ? 1 : 0);
	const int32_t x = lit + L;
	const uint32_t b = uint32_t(x + S.mis) & S.mask;
	const uint32_t* wb = reinterpret_cast<const uint32_t*>(S.lds + (b & ~3u));
	const uint32_t w2 = __builtin_amdgcn_alignbyte(wb[1], wb[0], b & 3u);
	const uint32_t e2 = (w2 >> 16) & 0xffu;
	q.lit = lit;
	q.L = L;
	q.off = int32_t(w2 & 0xffffu);
	q.ml = int32_t(tk & 15u) + 4 + (x2 ? int32_t(e2) : 0);
	q.next = x + 2 + (x2 ? 1 : 0);
	return p >= S.lo && x + 8 <= S.hi && x + 8 <= n && !(x1 && e1 == 255u) && !(x2 && e2 == 255u) &&
	       q.off != 0;
}


// 16 bytes from global memory at byte address a, never reading at or past lim.
__device__ __forceinline__ u32x4 gload16(uintptr_t a, uintptr_t lim)
{
	u32x4 v;
	if (a + 16 <= lim) {
		__builtin_memcpy(&v, reinterpret_cast<cg8*>(a), 16);
	} else {
		uint8_t t[16];
		for (int i = 0; i < 16; ++i)
			t[i] = (a + i < lim) ? *reinterpret_cast<cg8*>(a + i) : 0;
		__builtin_memcpy(&v, t, 16);
	}
	return v;
}

// Exact-length store of n (0..16) bytes to global memory.
__device__ __forceinline__ void gstore_n(g8* dst, u32x4 v, int32_t n)
{
	if (n >= 16) {
		__builtin_memcpy(dst, &v, 16);
		return;
	}
	uint64_t lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
	const uint64_t hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
	if (n & 8) {
		__builtin_memcpy(dst, &lo, 8);
		dst += 8;
		lo = hi;
	}
	if (n & 4) {
		const uint32_t x = uint32_t(lo);
		__builtin_memcpy(dst, &x, 4);
		dst += 4;
		lo >>= 32;
	}
	if (n & 2) {
		const uint16_t x = uint16_t(lo);
		__builtin_memcpy(dst, &x, 2);
		dst += 2;
		lo >>= 16;
	}
	if (n & 1)
		*dst = uint8_t(lo);
}
