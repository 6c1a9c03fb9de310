// lz4ada_bulk_linked.cpp -- the linked-frame bulk path of the MI355X LZ4Ada
// decompressor (BASELINE configs[4]): every block of a
// linked frame (B.Indep = 0, the LZ4F default) decoded at once against
// synthetic history, which lz4ada_linked.hip then resolves on the GPU by
// pointer jumping; quirk D1 (lib/lz4ada.adb:811-817, 862-879)
// and references before the frame start go to the exact path.
//
// bulk_linked, at the end, is the batch loop: cut a batch, lay it, decode
// planes x and z, accept, planes y and h if any block needs them, resolve,
// commit.  The stages that touch no device (lay_batch, accept_blocks,
// plane_modes) are lz4ada_linked_accept.h's; the device stages and the trace
// are here, above it.
#include "lz4ada_host_common.h"

namespace lz4ada {
namespace {

static_assert(DS_OK == 0, "status_ok (lz4ada_linked_accept.h) reads code 0 as DS_OK");

// LZ4ADA_TRACE_LINKED=1: phase times (synchronised) to stderr; =2: the
// host's own time between the phases (no synchronisation); =3: a line per
// block the acceptor looks at.
int trace_level()  // read once per process
{
	static const int level = [] {
		const char* e = getenv("LZ4ADA_TRACE_LINKED");
		return e ? std::max(1, atoi(e)) : 0;
	}();
	return level;
}
struct Trace {
	const int level = trace_level();
	hipStream_t stream;
	std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	explicit Trace(hipStream_t s) : stream(s) {}
	void phase(const char* name)
	{
		if (!level)
			return;
		if (level == 1)
			HIP_OK(hipStreamSynchronize(stream));
		const auto t1 = std::chrono::steady_clock::now();
		fprintf(stderr, "[linked] %-10s %8.3f ms\n", name,
		        std::chrono::duration<double, std::milli>(t1 - t0).count());
		t0 = t1;
	}
	BulkResult why(BulkResult r, const char* reason) const  // why the batch loop ends
	{
		if (level)
			fprintf(stderr, "[linked] result %d: %s\n", int(r), reason);
		return r;
	}
	// the acceptor's view of block `blk` of the frame, the round state at its start
	void block(uint32_t blk, const lz4ada_block_desc& d, const lz4ada_block_status& st,
	           const lz4ada_block_status& stz, const RoundState& rs, bool d1_bad) const
	{
		if (level > 2)
			fprintf(stderr, "[linked] block %u: code %d aux %d len %u z %d | opos %lld oph %lld pred %s%u/%u%s\n",
			        blk, st.code, st.aux, st.out_len, stz.code, (long long)rs.pos, (long long)rs.history,
			        (d.flags & BLOCK_D1_ROUND) ? "" : "-", (d.flags >> BLOCK_D1_OPH_SHIFT) & 7u,
			        d.flags >> BLOCK_N1_SHIFT, d1_bad ? " D1 STOP" : "");
	}
	void words(int64_t hbytes, int64_t n, bool full) const
	{
		if (level)
			fprintf(stderr, "[linked] history   %.3f of the bytes read straight from history: %s words\n",
			        double(hbytes) / double(std::max<int64_t>(n, 1)), full ? "full" : "sparse");
	}
	void spans_flagged(const uint8_t* d_act, int64_t ns) const  // spans a round will visit
	{
		if (!level)
			return;
		std::vector<uint8_t> h(static_cast<size_t>(ns));
		d2h(h.data(), d_act, size_t(ns), stream);
		size_t c = 0;
		for (uint8_t v : h)
			c += v != 0;
		fprintf(stderr, "[linked] spans     %zu of %lld flagged\n", c, (long long)ns);
	}
};

// The small per-call buffers -- both history tails, and per batch the
// descriptors, both planes' statuses (x's, then z's: one copy back), A, the
// modes and the round counters -- carved from one thread-cached device buffer
// (SC_LINK), and their host sides from one thread-cached pinned buffer: a
// pooled buffer's release costs a device synchronisation (round 5: ~8 per
// call).  Sized for all the frame's blocks in one batch.
struct LinkScratch {
	uint8_t* d_tail[2] = { nullptr, nullptr };
	lz4ada_block_desc *d_desc = nullptr, *h_desc = nullptr;
	lz4ada_block_status *d_st = nullptr, *h_st = nullptr;
	int64_t *d_A = nullptr, *h_A = nullptr;
	uint8_t *d_mode = nullptr, *h_mode = nullptr;
	uint32_t *d_ctr = nullptr, *h_ctr = nullptr;
	bool carve(size_t nmax)  // false: no device memory
	{
		auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
		const size_t o_desc = 2 * size_t(HISTORY_SIZE), o_st = o_desc + al(nmax * sizeof(lz4ada_block_desc)),
		             o_A = o_st + al(2 * nmax * sizeof(lz4ada_block_status)),
		             o_mode = o_A + al(nmax * sizeof(int64_t)), o_ctr = o_mode + al(nmax), bytes = o_ctr + 256;
		uint8_t* const d = scratch(SC_LINK, bytes);
		if (!d)
			return false;
		PinBuf& pin = scratch_cache().pin;
		pin.reserve(bytes);
		uint8_t* const h = pin.p;  // host twin of d: h + o is the host side of d + o
		auto both = [&](size_t o, auto*& dev, auto*& host) {
			using T = std::remove_reference_t<decltype(*dev)>;
			dev = reinterpret_cast<T*>(d + o);
			host = reinterpret_cast<T*>(h + o);
		};
		d_tail[0] = d;
		d_tail[1] = d + HISTORY_SIZE;
		both(o_desc, d_desc, h_desc);
		both(o_st, d_st, h_st);
		both(o_A, d_A, h_A);
		both(o_mode, d_mode, h_mode);
		both(o_ctr, d_ctr, h_ctr);
		return true;
	}
};

// What a call's stages share: the frame on the device, its stream, the carved
// scratch and the trace.
struct Linked {
	const uint8_t* d_frame;
	uint64_t frame_len;
	int64_t block_max;
	hipStream_t stream;
	LinkScratch s;
	Trace tr;
};

// A batch on its way through the stages.  d: its blocks as lay_batch laid them;
// st, stz: planes x's and z's statuses on the host.  Two planes for every block
// (x: history k -> k & 255; z: literals as zeros, history k -> k >> 8), two more
// (y, h) only for the blocks z cannot serve.  On the device
// plane x's statuses are c.s.d_st[0 .. d.size()), plane z's the d.size() after them.
struct Batch {
	std::vector<lz4ada_block_desc> d;
	uint64_t bytes = 0;
	uint8_t *bx = nullptr, *bz = nullptr, *tab = nullptr, *py = nullptr, *ph = nullptr;
	std::vector<lz4ada_block_status> st, stz;
};

// The history before the first block into d_tail (zeros where there is none);
// returns its valid bytes.
int64_t seed_tail(uint8_t* d_tail, const LinkedHist* hist, hipStream_t stream)
{
	HIP_OK(hipMemsetAsync(d_tail, 0, size_t(HISTORY_SIZE), stream));
	if (!hist)
		return 0;
	if (hist->n1 > 0)
		HIP_OK(hipMemcpyAsync(d_tail + HISTORY_SIZE - hist->n1, hist->h1, size_t(hist->n1),
		                      hipMemcpyDeviceToDevice, stream));
	if (hist->n0 > 0)
		HIP_OK(hipMemcpyAsync(d_tail + HISTORY_SIZE - hist->n1 - hist->n0, hist->h0, size_t(hist->n0),
		                      hipMemcpyDeviceToDevice, stream));
	return std::min<int64_t>(hist->n0 + hist->n1, HISTORY_SIZE);
}

// The blocks [lo, hi) of the next batch: as many as `budget` bytes of slots
// and history regions hold, one at least.
uint32_t cut_batch(const std::vector<lz4ada_block_desc>& descs, uint32_t lo, int64_t block_max, uint64_t budget)
{
	const auto bt = batches_of(std::vector<lz4ada_block_desc>(descs.begin() + lo, descs.end()), block_max,
	                           uint64_t(HISTORY_SIZE), budget);
	return lo + bt[0].second;
}

// Decode planes x and z of every block of the batch; their statuses come back
// in b.st and b.stz.
void decode_xz(Linked& c, Batch& b)
{
	const uint32_t nb = uint32_t(b.d.size());
	lz4ada_block_desc* const d_desc = c.s.d_desc;
	lz4ada_block_status *const sx = c.s.d_st, *const sz = sx + nb;
	const size_t sb = b.d.size() * sizeof(lz4ada_block_status);
	memcpy(c.s.h_desc, b.d.data(), b.d.size() * sizeof(lz4ada_block_desc));
	HIP_OK(hipMemcpyAsync(d_desc, c.s.h_desc, b.d.size() * sizeof(lz4ada_block_desc), hipMemcpyHostToDevice,
	                      c.stream));
	c.tr.phase("desc h2d");
	HIP_OK(hipMemsetAsync(sx, 0, sb, c.stream));
	// the history regions' fill and the checksums ride beside the index
	// (side stream); the decodes wait for the fill, the status read for
	// the checksums
	HIP_OK(launch_link_fill_beside(b.bx, nullptr, b.bz, d_desc, nb, c.stream));
	HIP_OK(launch_block_checksums_beside(c.d_frame, d_desc, nb, sx, c.stream));
	HIP_OK(launch_index(c.d_frame, c.frame_len, d_desc, nb, b.tab, sx, c.stream));
	HIP_OK(join_link_fill(c.stream));
	c.tr.phase("launches");
	HIP_OK(hipMemcpyAsync(sz, sx, sb, hipMemcpyDeviceToDevice, c.stream));
	// plane z's decode on the side stream beside plane x's: each launch
	// has more blocks than resident slots, and the other one's blocks
	// fill the slots its last ones leave idle
	// (LZ4ADA_LINK_SERIAL=1: one after the other, for A/B)
	static const bool serial = getenv("LZ4ADA_LINK_SERIAL") != nullptr;
	hipStream_t side = c.stream;
	if (!serial)
		HIP_OK(side_fork(c.stream, &side));
	HIP_OK(launch_decode_idx_tab(c.d_frame, c.frame_len, d_desc, nb, b.tab, b.bz, sz, IdxMode::LINKED_ZL, side));
	HIP_OK(launch_decode_idx_tab(c.d_frame, c.frame_len, d_desc, nb, b.tab, b.bx, sx, IdxMode::LINKED_LK,
	                             c.stream));
	HIP_OK(launch_decode_pc(c.d_frame, c.frame_len, d_desc, nb, b.bx, sx, 1, LINK_HIST, c.stream));
	HIP_OK(side_join(c.stream));  // plane z and the checksums
	c.tr.phase("decodes");
	d2h(c.s.h_st, sx, 2 * sb, c.stream);
	b.st.assign(c.s.h_st, c.s.h_st + nb);
	b.stz.assign(c.s.h_st + nb, c.s.h_st + 2 * nb);
}

// Decode planes y and (nh != 0) h of the accepted blocks [0, nb) whose mode
// (c.s.h_mode) asks for them; every other block is DS_SKIP in those launches.
// nullptr, or why the frame goes to the exact path.
const char* decode_yh(Linked& c, Batch& b, uint32_t nb, uint32_t nh)
{
	const uint8_t* const mode = c.s.h_mode;
	b.py = scratch(SC_Y, size_t(b.bytes));
	b.ph = b.py && nh ? scratch(SC_H, size_t(b.bytes)) : nullptr;
	if (!b.py || (nh && !b.ph))
		return "plane Y/H alloc";
	HIP_OK(hipMemcpyAsync(c.s.d_mode, mode, nb, hipMemcpyHostToDevice, c.stream));
	HIP_OK(launch_link_fill(nullptr, b.py, b.ph, c.s.d_desc, nb, c.stream));
	// the plane's statuses in plane z's half of the status scratch (free: stz
	// is on the host), not a pooled buffer -- releasing one costs a
	// device-wide synchronisation
	lz4ada_block_status* const s_dev = c.s.d_st + b.d.size();
	for (int k = 0; k < (nh ? 2 : 1); ++k) {
		std::vector<lz4ada_block_status> s_plane(b.stz.begin(), b.stz.begin() + nb);
		for (uint32_t i = 0; i < nb; ++i)
			if (mode[i] <= k)  // y: modes 1 and 2; h: mode 2
				s_plane[i].code = DS_SKIP;
		const size_t sb = s_plane.size() * sizeof(lz4ada_block_status);
		HIP_OK(hipMemcpyAsync(s_dev, s_plane.data(), sb, hipMemcpyHostToDevice, c.stream));
		uint8_t* const buf = k == 0 ? b.py : b.ph;
		HIP_OK(launch_decode_idx_tab(c.d_frame, c.frame_len, c.s.d_desc, nb, b.tab, buf, s_dev, IdxMode::LINKED_LK,
		                             c.stream));
		HIP_OK(launch_decode_pc(c.d_frame, c.frame_len, c.s.d_desc, nb, buf, s_dev, 1, LINK_HIST, c.stream));
		d2h(s_plane.data(), s_dev, sb, c.stream);
		for (uint32_t i = 0; i < nb; ++i)
			if (mode[i] > k && (s_plane[i].code != DS_OK || s_plane[i].out_len != b.st[i].out_len))
				return "never expected: plane x decoded it";
	}
	c.tr.phase("more planes");
	return nullptr;
}

// Resolve the accepted blocks [0, nb), n bytes starting at c.s.h_A[], into
// the sink's buffer (*F) against the history in d_tail (tail_valid bytes of
// it real), and leave the next batch's history in d_tail_next.  nullptr, or
// why the frame goes to the exact path.
const char* resolve(Linked& c, const Batch& b, uint32_t nb, int64_t n, bool more_planes, const uint8_t* d_tail,
                    int64_t tail_valid, uint8_t* d_tail_next, LinkedSink& sink, uint8_t** F_out)
{
	uint32_t* const d_P = reinterpret_cast<uint32_t*>(scratch(SC_P, size_t(std::max<int64_t>(n, 1)) * 4));
	if (!d_P)
		return "scratch P alloc";
	HIP_OK(hipMemcpyAsync(c.s.d_A, c.s.h_A, nb * sizeof(int64_t), hipMemcpyHostToDevice, c.stream));
	// a word per output byte (resolving only the history-derived bytes,
	// round 4's sparse form, measured slower -- three gathers per target
	// instead of one word -- DESIGN §7).  The constant bytes go to F with the
	// words, each round writes the bytes it resolves: the last round leaves
	// the output
	uint8_t* const F = *F_out = sink.dst(n);
	if (!F)
		return "sink has no room";
	// span activity flags, double-buffered across rounds (an init that
	// also stepped every history-derived byte one pointer forward was
	// measured and dropped: mixed 10.32 vs 10.35 ms, chain 13.5 vs
	// 15.4, dense 31.0 vs 23.7 -- its byte gathers cost what the round
	// saves)
	const int64_t ns = link_spans(n);
	uint8_t* const act = scratch(SC_U, size_t(2 * ns + 64));
	uint8_t* const M = act ? scratch(SC_M, size_t(n) + 64) : nullptr;
	if (!M)
		return "scratch U/M alloc";
	// init flags the spans that hold a history-derived byte: the
	// first round reads only those
	HIP_OK(hipMemsetAsync(act + ns, 0, size_t(ns), c.stream));
	// words everywhere (`full`) or only where a byte is still open
	// after init's steps: the latter saves most of init's writes but
	// costs the rounds a gather per word (a source's M), which only
	// pays where few stay open.  The z decoder counts the match bytes
	// each block reads straight from history: above 1/12 of the
	// batch's bytes (measured: dense 0.102, mixed 0.058, chain 0),
	// full.
	// LZ4ADA_LINK_WORDS=full / sparse forces one.
	int64_t hbytes = 0;
	for (uint32_t i = 0; i < nb; ++i)
		hbytes += b.stz[i].detail;
	const char* we = getenv("LZ4ADA_LINK_WORDS");  // (per call: the tests force both)
	const int words_env = we ? (we[0] == 'f' ? 1 : (we[0] == 's' ? 2 : 0)) : 0;
	const bool full = words_env ? words_env == 1 : 12 * hbytes > n;
	c.tr.words(hbytes, n, full);
	HIP_OK(launch_link_init(b.bx, b.bz, b.py, b.ph, more_planes ? c.s.d_mode : nullptr, c.s.d_desc, c.s.d_st,
	                        c.s.d_A, nb, c.block_max, d_tail, tail_valid, d_P, F, M, act + ns, full, c.stream));
	c.tr.phase("init");
	c.tr.spans_flagged(act + ns, ns);
	// the rounds run in pairs, one host round trip per pair (a mixed
	// frame needs two rounds; a round after the last one finds every
	// span flagged 0 and reads only the flags).  The first pair always
	// runs: init's span flags leave it nothing to read when no byte
	// came from history (a count would cost an atomic per wave and a
	// round trip)
	uint32_t left = 1;
	for (int round = 0; left > 0; round += 2) {
		if (round > 64)
			return "never expected: every pointer goes strictly back";
		HIP_OK(hipMemsetAsync(c.s.d_ctr, 0, 4 * sizeof(uint32_t), c.stream));
		for (int k = 0; k < 2; ++k) {
			uint8_t* a_out = act + ((round + k) & 1) * ns;
			const uint8_t* a_in = act + ((round + k + 1) & 1) * ns;
			HIP_OK(launch_link_jump(d_P, M, n, d_tail, tail_valid, F, a_in, a_out, c.s.d_ctr + 2 * k, full,
			                        c.stream));
			c.tr.spans_flagged(a_out, ns);
		}
		// the next batch's history, enqueued before the round trip (a
		// later pair, if any, writes it again)
		HIP_OK(launch_link_tail(F, n, d_tail, d_tail_next, c.stream));
		const uint32_t* c4 = c.s.h_ctr;
		d2h(c.s.h_ctr, c.s.d_ctr, 4 * sizeof(uint32_t), c.stream);
		if (c4[1] || c4[3])
			return "a reference before the frame start: the exact error";
		left = c4[2];  // words still unresolved after the pair's second round
	}
	c.tr.phase("jumps");
	return nullptr;
}

}  // namespace

// Linked frames (and independent ones whose blocks read earlier blocks,
// D2): every block at once with synthetic history, resolved on the GPU
// (lz4ada_linked.hip), batch by batch with the previous batch's last
// 64 KiB carried as real history.  BULK_EXACT: the frame needs the exact
// path (a block error or checksum mismatch, quirk D1, a reference before
// the frame start, no device memory).
BulkResult bulk_linked(const uint8_t* d_frame, uint64_t frame_len, int64_t block_max,
                              const std::vector<lz4ada_block_desc>& descs, LinkedSink& sink,
                              uint64_t& total, std::vector<uint32_t>& lens, int64_t& fail,
                              hipStream_t stream, const LinkedHist* hist)
{
	lens.clear();
	fail = -1;
	// a batch holds 3 decode buffers (slots + 64 KiB regions) and one 4-byte
	// word per output byte: ~7x its slot bytes
	uint64_t budget = uint64_t(env_bytes("LZ4ADA_LINKED_BATCH_BYTES", int64_t(2) << 30));
	Linked c{ d_frame, frame_len, block_max, stream, LinkScratch{}, Trace(stream) };
	Trace& tr = c.tr;
	if (!c.s.carve(descs.size()))
		return tr.why(BULK_EXACT, "scratch LINK alloc");
	int cur = 0;  // c.s.d_tail[cur]: the history before the batch
	const int64_t hist0 = seed_tail(c.s.d_tail[0], hist, stream);  // history bytes before the first block
	RoundState rs = hist ? hist->round : RoundState{};  // for quirk D1
	uint32_t lo = 0;
	total = 0;
	while (lo < descs.size()) {
		const uint32_t hi = cut_batch(descs, lo, block_max, budget);
		Batch b;
		b.d.assign(descs.begin() + lo, descs.begin() + hi);
		tr.phase("batch");
		b.bytes = lay_batch(b.d, block_max, rs);
		b.bx = scratch(SC_X, size_t(b.bytes));
		b.bz = b.bx ? scratch(SC_Z, size_t(b.bytes)) : nullptr;
		b.tab = b.bz ? scratch(SC_TAB, index_table_bytes(frame_len, uint32_t(b.d.size()))) : nullptr;
		if (!b.tab) {
			// no room: a smaller batch from the same start
			if (budget > (uint64_t(64) << 20) && b.d.size() > 1) {
				budget /= 2;
				continue;
			}
			return tr.why(BULK_EXACT, "scratch X/Z/TAB alloc");
		}
		tr.phase("alloc");
		decode_xz(c, b);
		const RoundState rs0 = rs;  // this batch's start (a smaller retry rescans)
		const Accepted a = accept_blocks(b.d, b.st, b.stz, rs, c.s.h_A,
		                                 [&](uint32_t i, const RoundState& at, bool d1_bad) {
			                                 tr.block(lo + i, b.d[i], b.st[i], b.stz[i], at, d1_bad);
		                                 });
		if (a.count < b.d.size()) {
			fail = int64_t(lo) + a.count;
			if (a.count == 0)
				return tr.why(BULK_FAIL_AT, "the batch's first block fails");
		}
		const int64_t n = a.bytes;
		if (n >= (int64_t(1) << 31) - HISTORY_SIZE) {  // words hold positions + 65536 in 31 bits
			if (a.count > 1) {
				// the smaller batch rescans from this batch's start: its own
				// first failing block (if any) and the replayed positions
				budget /= 2;
				fail = -1;
				rs = rs0;
				continue;
			}
			return tr.why(BULK_EXACT, "positions overflow 31 bits");
		}
		const PlaneCounts planes = plane_modes(b.stz, a.count, c.s.h_mode);
		if (planes.ny)
			if (const char* reason = decode_yh(c, b, a.count, planes.nh))
				return tr.why(BULK_EXACT, reason);
		const int64_t tail_valid = std::min<int64_t>(int64_t(total) + hist0, HISTORY_SIZE);
		uint8_t* F = nullptr;
		if (const char* reason = resolve(c, b, a.count, n, planes.ny != 0, c.s.d_tail[cur], tail_valid,
		                                 c.s.d_tail[cur ^ 1], sink, &F))
			return tr.why(BULK_EXACT, reason);
		cur ^= 1;
		tr.phase("emit");
		sink.done(F, n);
		tr.phase("sink");
		total += uint64_t(n);
		for (uint32_t i = 0; i < a.count; ++i)
			lens.push_back(b.st[i].out_len);
		if (fail >= 0)
			return tr.why(BULK_FAIL_AT, "a block fails, the ones before it committed");
		lo = hi;
	}
	return BULK_OK;
}

}  // namespace lz4ada
