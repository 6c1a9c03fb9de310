// lz4ada_bulk_frames.cpp -- many frames in one device pass:
// the stream index (which frames a concatenated stream holds and which of
// them can share a pass), the pass itself (one H2D of the frames, the device
// half that lz4ada_frames_pass.cpp states for this engine and the
// device-to-device one, one D2H of the bytes), and the entries built on it:
// lz4ada_stream_index, lz4ada_decode_frames and the routing of
// lz4ada_decode_stream / _alloc.  A frame the pass does not find good in
// every respect is decoded again by decode_one_frame (lz4ada_bulk.cpp), so
// every error text is the reference's; this unit invents none for a decode.
// With LZ4ADA_FRAMES_LINKED, linked frames up to lz4ada_batch_linked_max()
// share the pass.
#include "lz4ada_frame_walk.h"
#include "lz4ada_host_common.h"

using namespace lz4ada;

namespace lz4ada {
namespace {

// lz4ada_decode_stream takes the pass when the stream holds at least this
// many batchable frames with blocks (profiles/frames_batch_ab.txt).
constexpr int64_t BATCH_MIN_FRAMES = 2;

thread_local std::vector<std::string> g_job_errors;

struct Frame {
	const uint8_t* p = nullptr;  // Single_Frame input: the frame and whatever follows it
	int64_t len = 0;
	lz4ada_frame_info info{};
	std::vector<lz4ada_block_desc> descs;
	int32_t reason = LZ4ADA_BATCH_NOT_INDEXED;
	uint64_t slots = 0;  // its slots as the pass lays them out: sum of round256(slot_cap)
	uint64_t caps = 0;   // sum of slot_cap: what it can decode to
	bool skippable() const { return info.format == LZ4ADA_FORMAT_SKIPPABLE; }
	bool linked() const { return info.format == LZ4ADA_FORMAT_MODERN && !info.independent; }
};

// The switches that pin a frame to one of the single-frame paths pin the
// stream to the per-frame loop too.
bool batch_enabled()
{
	return !getenv("LZ4ADA_NO_BATCH") && !getenv("LZ4ADA_EXACT_ONLY") && !getenv("LZ4ADA_FORCE_LINKED");
}

// Index the frame at fr.p and say whether it can share a pass.  *why (may
// be null) gets the exception of a frame that does not index.  flags:
// LZ4ADA_FRAMES_LINKED lets a linked frame of at most linked_max slot bytes in.
void classify(Frame& fr, uint64_t budget, Error* why, uint32_t flags, uint64_t linked_max)
{
	fr.reason = LZ4ADA_BATCH_NOT_INDEXED;
	fr.descs.clear();
	try {
		index_frame(fr.p, fr.len, fr.info, &fr.descs);
		if (fr.info.frame_len > fr.len)  // index_frame takes a skippable frame's length on trust
			raise(LZ4ADA_DATA_CORRUPTION, "Frame truncated inside a skippable frame.");
	} catch (const Error& e) {
		if (why)
			*why = e;
		return;
	}
	fr.reason = LZ4ADA_BATCH_OK;
	if (fr.skippable())
		return;  // consumed, no output
	if (fr.linked() && !(flags & LZ4ADA_FRAMES_LINKED)) {
		fr.reason = LZ4ADA_BATCH_LINKED;
		return;
	}
	fr.slots = fr.caps = 0;
	for (const auto& d : fr.descs) {
		const uint32_t cap = slot_cap(d, fr.info.block_max);
		if (cap > WALK_SLOT_MAX)
			fr.reason = LZ4ADA_BATCH_BIG_BLOCK;
		fr.slots += round256(cap);
		fr.caps += cap;
	}
	// a few large blocks decode far faster one at a time on the whole GPU
	// (decode_lone_blocks) than as one wave each in a pass
	if (few_large_blocks(fr.descs))
		fr.reason = LZ4ADA_BATCH_BIG_BLOCK;
	if (fr.reason == LZ4ADA_BATCH_OK && fr.linked() && fr.slots > linked_max)
		fr.reason = LZ4ADA_BATCH_LINKED;
	if (fr.reason == LZ4ADA_BATCH_OK && fr.slots > budget)
		fr.reason = LZ4ADA_BATCH_OVER_BUDGET;
}

// ------------------------------------------------------------ the engine

// What became of the frames: per job for lz4ada_decode_frames, else (a
// stream) the first failure propagates.
struct Report {
	lz4ada_frame_job* jobs = nullptr;
	int64_t* committed = nullptr;  // follows out.len after every success
};

void committed_now(const Report& rp, const Sink& out)
{
	if (rp.committed)
		*rp.committed = out.len;
}

// Frame i was committed from a pass: its n bytes lie at `off` of the output.
void report_batched(const Report& rp, const Frame& fr, size_t i, int64_t off, int64_t n)
{
	++batch_stats().frames_batched;
	const int bits = LZ4ADA_PATH_BATCH |
	                 (fr.skippable() ? 0 : fr.linked() ? LZ4ADA_PATH_LINKED : LZ4ADA_PATH_INDEPENDENT);
	add_last_path(bits);
	if (rp.jobs) {
		lz4ada_frame_job& j = rp.jobs[i];
		j.out_off = off;
		j.out_len = n;
		j.consumed = fr.info.frame_len;
		j.status = LZ4ADA_OK;
		j.path = bits;
	}
}

// Frame i on its own, by today's path: the reference's output or exception.
void decode_single(const Report& rp, const Frame& fr, size_t i, Sink& out)
{
	++batch_stats().frames_single;
	int64_t c = 0;
	if (!rp.jobs) {
		decode_one_frame(fr.p, fr.len, out, c);
		committed_now(rp, out);
		if (c <= 0)
			raise(LZ4ADA_CONSTRAINT_ERROR, "decoder made no progress");
		if (fr.reason != LZ4ADA_BATCH_NOT_INDEXED && c != fr.info.frame_len)
			raise(LZ4ADA_CONSTRAINT_ERROR, "a frame's decoded extent differs from its index");
		return;
	}
	const int before = lz4ada_last_path();
	set_last_path(0);
	const int64_t base = out.len;
	std::string msg;
	const int st = guarded(&msg, [&] {
		decode_one_frame(fr.p, fr.len, out, c);
		if (c <= 0)
			raise(LZ4ADA_CONSTRAINT_ERROR, "decoder made no progress");
	});
	const int bits = lz4ada_last_path();
	set_last_path(before | bits);
	if (st == LZ4ADA_DEVICE_ERROR)  // the call itself did not work
		raise(st, msg);
	lz4ada_frame_job& j = rp.jobs[i];
	j.out_off = base;
	j.out_len = out.len - base;  // on failure: what the reference had output before raising
	j.consumed = st == LZ4ADA_OK ? c : 0;
	j.status = st;
	j.path = bits;
	g_job_errors[i] = msg;
}

// One pass over the batchable frames fs[lo, hi).  contiguous: the frames
// lie back to back in the caller's input (a stream).  false: the device has
// no room for it (nothing was committed; the caller decodes them singly).
bool run_pass(const std::vector<Frame>& fs, size_t lo, size_t hi, bool contiguous, Sink& out,
              const Report& rp, uint64_t hash_max)
{
	device_check_or_raise();
	std::vector<PassFrame> frames;
	uint64_t slots = 0, caps = 0, packed = 0;
	for (size_t k = lo; k < hi; ++k) {
		frames.push_back(PassFrame{ uint32_t(fs[k].descs.size()), fs[k].linked() });
		slots += fs[k].slots;
		caps += fs[k].caps;
		packed += uint64_t(fs[k].info.frame_len);
	}

	// Stage: a stream's frames are already back to back, so their covering
	// range is copied as it is; a job array's frames are packed into pinned
	// memory first.  Either way one H2D.
	PinBuf pack;
	const uint8_t* src = fs[lo].p;
	uint64_t stage_len = packed;
	if (contiguous) {
		stage_len = uint64_t(fs[hi - 1].p - src) + uint64_t(fs[hi - 1].info.frame_len);
	} else {
		pack.reserve(size_t(packed));
		uint64_t at = 0;
		for (size_t k = lo; k < hi; ++k) {
			memcpy(pack.p + at, fs[k].p, size_t(fs[k].info.frame_len));
			at += uint64_t(fs[k].info.frame_len);
		}
		src = pack.p;
	}

	// every reservation before the first copy is queued
	uint8_t* const d_in = scratch(SC_FRAME, size_t(stage_len));
	uint8_t* const d_cmp = scratch(SC_BATCH, size_t(std::max<uint64_t>(caps, 1)));
	PassArrays a;
	if (!d_in || !d_cmp || a.reserve(frames, slots, stage_len))
		return false;

	// Descriptors rebased to the staged base, in frame and block order, and
	// stage_len covers the staged range, as decode_pass asks; slots as
	// bulk_independent lays them out.  The records stay in a pinned buffer of
	// this pass: decode_single runs between the reads of them.
	PinBuf hmeta;
	hmeta.reserve(a.desc_b + a.rec_b);
	auto* const h_desc = reinterpret_cast<lz4ada_block_desc*>(hmeta.p);
	auto* const h_rec = reinterpret_cast<FrameRec*>(hmeta.p + a.desc_b);
	uint32_t b = 0;
	uint64_t slot_at = 0, in_at = 0;
	for (size_t k = lo; k < hi; ++k) {
		const Frame& fr = fs[k];
		const uint64_t base = contiguous ? uint64_t(fr.p - src) : in_at;
		in_at += uint64_t(fr.info.frame_len);
		FrameRec r{};
		r.first = b;
		r.nblocks = uint32_t(fr.descs.size());
		r.flags = (fr.info.has_content_size ? FRAME_HAS_SIZE : 0u) |
		          (fr.info.content_checksum ? FRAME_HAS_CKSUM : 0u) | (fr.linked() ? FRAME_LINKED : 0u);
		r.content_size = fr.info.content_size;
		r.fail = -1;
		h_rec[k - lo] = r;
		for (const auto& d : fr.descs) {
			lz4ada_block_desc x = d;
			x.in_off = base + d.in_off;
			x.out_cap = slot_cap(d, fr.info.block_max);
			x.out_off = slot_at;
			slot_at += round256(x.out_cap);
			h_desc[b++] = x;
		}
	}

	hipStream_t stream = nullptr;
	HIP_OK(hipMemcpyAsync(d_in, src, size_t(stage_len), hipMemcpyHostToDevice, stream));
	HIP_OK(hipMemcpyAsync(a.d_desc, hmeta.p, a.desc_b + a.rec_b, hipMemcpyHostToDevice, stream));
	decode_pass(a, d_in, stage_len, d_cmp, hash_max, h_rec, stream);

	const auto rec = [&](size_t k) -> const FrameRec& { return h_rec[k - lo]; };
	std::vector<FrameVerdict> verdict(frames.size());
	for (size_t k = lo; k < hi; ++k) {
		bool hashed = false;
		verdict[k - lo] = frame_verdict(rec(k), fs[k].info.content_checksum_declared, &hashed);
		batch_stats().gpu_hashed += hashed ? 1 : 0;
	}
	size_t k = lo;
	while (k < hi) {
		// good as far as the device can tell: every block, the content size and
		// (when it was hashed there) the content checksum
		if (verdict[k - lo] != FV_GOOD && verdict[k - lo] != FV_HOST_HASH) {
			decode_single(rp, fs[k], k, out);
			++k;
			continue;
		}
		if (verdict[k - lo] == FV_HOST_HASH) {  // over hash_max: hashed while its bytes are copied out
			const FrameRec& r = rec(k);
			uint8_t* dst = out.room(int64_t(r.out_len));
			lz4ada_xxh32_state hs;
			lz4ada_xxh32_reset(&hs, 0);
			content_xxh32_d2h(hs, d_cmp + r.out_off, int64_t(r.out_len), dst, stream);
			++batch_stats().host_hashed;
			if (host_xxh32_final(hs) != fs[k].info.content_checksum_declared) {
				decode_single(rp, fs[k], k, out);  // over the bytes just copied: none was committed
			} else {
				report_batched(rp, fs[k], k, out.len, int64_t(r.out_len));
				out.commit(int64_t(r.out_len));
				committed_now(rp, out);
			}
			++k;
			continue;
		}
		// a run of good frames: adjacent in the compacted output, one D2H
		size_t m = k;
		while (m < hi && verdict[m - lo] == FV_GOOD)
			++m;
		const uint64_t off0 = rec(k).out_off;
		const uint64_t total = rec(m - 1).out_off + rec(m - 1).out_len - off0;
		uint8_t* dst = out.room(int64_t(total));
		if (total)
			HIP_OK(hipMemcpy(dst, d_cmp + off0, size_t(total), hipMemcpyDeviceToHost));
		for (size_t q = k; q < m; ++q)
			report_batched(rp, fs[q], q, out.len + int64_t(rec(q).out_off - off0), int64_t(rec(q).out_len));
		out.commit(int64_t(total));
		committed_now(rp, out);
		k = m;
	}
	return true;
}

// Every frame of fs in order: each maximal run of batchable frames within
// the byte budget in one pass, everything else singly.
void run_frames(const std::vector<Frame>& fs, bool contiguous, Sink& out, const Report& rp)
{
	const uint64_t budget = uint64_t(batch_budget()), hash_max = uint64_t(batch_hash_max());
	const bool enabled = batch_enabled();
	size_t i = 0;
	while (i < fs.size()) {
		size_t j = i;
		uint64_t acc = 0, nb = 0, real = 0;
		while (enabled && j < fs.size() && fs[j].reason == LZ4ADA_BATCH_OK &&
		       (j == i || acc + fs[j].slots <= budget) && nb + fs[j].descs.size() < (uint64_t(1) << 31)) {
			acc += fs[j].slots;
			nb += fs[j].descs.size();
			real += fs[j].skippable() ? 0 : 1;
			++j;
		}
		if (j == i)
			j = i + 1;
		// a pass pays off from two frames with blocks on; fewer go the
		// single way (a skippable frame is consumed on the host either way)
		if (real < 2 || !run_pass(fs, i, j, contiguous, out, rp, hash_max)) {
			for (size_t k = i; k < j; ++k) {
				if (fs[k].reason == LZ4ADA_BATCH_OK && fs[k].skippable() && enabled)
					report_batched(rp, fs[k], k, out.len, 0);
				else
					decode_single(rp, fs[k], k, out);
			}
		}
		i = j;
	}
}

}  // namespace

void decode_stream_frames(const uint8_t* input, int64_t len, Sink& out, int64_t* committed)
{
	batch_stats() = lz4ada_batch_stats{};
	Report rp;
	rp.committed = committed;
	std::vector<Frame> fs;
	int64_t pos = 0;
	// a stream of one frame (the common call) is not indexed twice
	bool several = false;
	if (batch_enabled() && len >= 7) {
		try {
			lz4ada_frame_info first;
			index_frame(input, len, first, nullptr);
			several = first.frame_len < len;
		} catch (const Error&) {
		}
	}
	if (several) {
		const uint64_t budget = uint64_t(batch_budget()), linked_max = uint64_t(batch_linked_max());
		const uint32_t flags = batch_env_flags();
		int64_t real = 0;
		while (pos < len) {
			Frame fr;
			fr.p = input + pos;
			fr.len = len - pos;
			classify(fr, budget, nullptr, flags, linked_max);
			if (fr.reason == LZ4ADA_BATCH_NOT_INDEXED)
				break;  // from here on the per-frame loop, which raises in the reference's order
			pos += fr.info.frame_len;
			real += (fr.reason == LZ4ADA_BATCH_OK && !fr.skippable()) ? 1 : 0;
			fs.push_back(std::move(fr));
		}
		if (real < BATCH_MIN_FRAMES) {
			fs.clear();
			pos = 0;
		}
	}
	if (!fs.empty())
		run_frames(fs, true, out, rp);
	while (pos < len) {
		int64_t c = 0;
		partial_frame_check(len - pos);
		++batch_stats().frames_single;
		decode_one_frame(input + pos, len - pos, out, c);
		committed_now(rp, out);
		if (c <= 0)
			raise(LZ4ADA_CONSTRAINT_ERROR, "decoder made no progress");
		pos += c;
	}
}

}  // namespace lz4ada

extern "C" {

int lz4ada_stream_index(const uint8_t* input, int64_t len, lz4ada_stream_entry* entries, int64_t cap,
                        int64_t* nframes)
{
	return lz4ada_stream_index_opt(input, len, batch_env_flags(), entries, cap, nframes);
}

int lz4ada_stream_index_opt(const uint8_t* input, int64_t len, uint32_t flags, lz4ada_stream_entry* entries,
                            int64_t cap, int64_t* nframes)
{
	*nframes = 0;
	return guarded(nullptr, [&] {
		const uint64_t budget = uint64_t(batch_budget()), linked_max = uint64_t(batch_linked_max());
		int64_t pos = 0;
		while (pos < len) {
			Frame fr;
			fr.p = input + pos;
			fr.len = len - pos;
			Error why{ LZ4ADA_OK, "" };
			classify(fr, budget, &why, flags, linked_max);
			if (fr.reason == LZ4ADA_BATCH_NOT_INDEXED)
				raise(why.code, why.msg);
			if (entries) {
				if (*nframes >= cap)
					raise(LZ4ADA_CONSTRAINT_ERROR, "stream entry capacity exceeded");
				lz4ada_stream_entry& e = entries[*nframes];
				e.offset = pos;
				e.frame_len = fr.info.frame_len;
				e.info = fr.info;
				e.batchable = fr.reason;
				e.pad = 0;
			}
			++*nframes;
			pos += fr.info.frame_len;
		}
	});
}

int lz4ada_decode_frames(lz4ada_frame_job* jobs, int64_t njobs, uint8_t** out, int64_t* out_len)
{
	return lz4ada_decode_frames_opt(jobs, njobs, batch_env_flags(), out, out_len);
}

int lz4ada_decode_frames_opt(lz4ada_frame_job* jobs, int64_t njobs, uint32_t flags, uint8_t** out,
                             int64_t* out_len)
{
	*out = nullptr;
	*out_len = 0;
	batch_stats() = lz4ada_batch_stats{};
	g_job_errors.clear();
	set_last_path(0);
	Sink s;
	s.growable = true;
	const int st = guarded(nullptr, [&] {
		if (!jobs || njobs < 0)
			raise(LZ4ADA_ASSERTION_ERROR, "lz4ada_decode_frames: jobs is NULL or njobs is negative");
		g_job_errors.assign(size_t(njobs), std::string());
		const uint64_t budget = uint64_t(batch_budget()), linked_max = uint64_t(batch_linked_max());
		std::vector<Frame> fs(static_cast<size_t>(njobs));
		for (int64_t i = 0; i < njobs; ++i) {
			lz4ada_frame_job& j = jobs[i];
			j.out_off = j.out_len = j.consumed = 0;
			j.status = LZ4ADA_OK;
			j.path = 0;
			fs[size_t(i)].p = j.frame;
			fs[size_t(i)].len = j.len;
			if (j.frame && j.len >= 7)
				classify(fs[size_t(i)], budget, nullptr, flags, linked_max);
		}
		Report rp;
		rp.jobs = jobs;
		run_frames(fs, false, s, rp);
	});
	if (st != LZ4ADA_OK) {
		free(s.p);
		return st;
	}
	*out = s.p ? s.p : static_cast<uint8_t*>(malloc(1));
	*out_len = s.len;
	return LZ4ADA_OK;
}

const char* lz4ada_frames_error(int64_t i)
{
	return i >= 0 && size_t(i) < g_job_errors.size() ? g_job_errors[size_t(i)].c_str() : "";
}

void lz4ada_last_batch_stats(lz4ada_batch_stats* out) { *out = batch_stats(); }

int64_t lz4ada_batch_hash_max(void) { return batch_hash_max(); }
int64_t lz4ada_batch_linked_max(void) { return batch_linked_max(); }

// Test-only (lz4ada_hip.h): k_index over the marked frames' blocks, then
// k_decode_idx_frames over every record; the unmarked frames' blocks see no
// launch at all.
int lz4ada_decode_idx_frames_debug(const void* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_descs,
                                   int64_t nblocks, const int64_t* first, const uint8_t* linked, int64_t nframes,
                                   void* d_out, lz4ada_block_status* d_status, void* stream)
{
	return guarded(nullptr, [&] {
		if (nblocks < 0 || nblocks >= (int64_t(1) << 31) || nframes < 0 || nframes >= (int64_t(1) << 31) ||
		    !first || (nframes > 0 && !linked))
			raise(LZ4ADA_CONSTRAINT_ERROR, "block or frame count out of range");
		for (int64_t i = 0; i < nframes; ++i)
			if (first[i] < 0 || first[i] > first[i + 1] || first[i + 1] > nblocks)
				raise(LZ4ADA_CONSTRAINT_ERROR, "frame block ranges must rise within the blocks");
		if (nframes == 0 || nblocks == 0)
			return;
		device_check_or_raise();
		hipStream_t s = static_cast<hipStream_t>(stream);
		const auto* const in = static_cast<const uint8_t*>(d_frame);
		std::vector<FrameRec> recs(static_cast<size_t>(nframes));
		std::vector<PassFrame> frames;
		for (int64_t i = 0; i < nframes; ++i) {
			FrameRec& r = recs[size_t(i)];
			r = FrameRec{};
			r.first = uint32_t(first[i]);
			r.nblocks = uint32_t(first[i + 1] - first[i]);
			r.flags = linked[i] ? FRAME_LINKED : 0u;
			r.fail = -1;
			frames.push_back(PassFrame{ r.nblocks, linked[i] != 0 });
		}
		DevBuf<FrameRec> d_rec;
		d_rec.reserve(recs.size());
		DevBuf<uint8_t> tab;
		tab.reserve(index_table_bytes(frame_len, uint32_t(nblocks)));
		vec_h2d(d_rec, recs, s);
		for (const PassRun& r : pass_runs(frames))  // pass 1 per run of marked frames
			if (r.linked)
				HIP_OK(launch_index(in, frame_len, d_descs + first[r.f0], r.b1 - r.b0,
				                    tab.p + size_t(first[r.f0]) * 64, d_status + first[r.f0], s));
		HIP_OK(launch_decode_idx_frames(in, frame_len, d_descs, uint32_t(nblocks), tab.p,
		                                static_cast<uint8_t*>(d_out), d_status, d_rec.p, uint32_t(nframes), s));
		HIP_OK(hipStreamSynchronize(s));
	});
}

int lz4ada_xxh32_spans_device(const void* d_buf, const int64_t* off, const int64_t* len, int64_t nspans,
                              uint32_t* hash, float* kernel_ms)
{
	return guarded(nullptr, [&] {
		if (nspans < 0 || nspans > (int64_t(1) << 30))
			raise(LZ4ADA_CONSTRAINT_ERROR, "span count out of range");
		device_check_or_raise();
		std::vector<FrameRec> recs(static_cast<size_t>(nspans));
		for (int64_t i = 0; i < nspans; ++i) {
			if (off[i] < 0 || len[i] < 0)
				raise(LZ4ADA_CONSTRAINT_ERROR, "negative span");
			FrameRec& r = recs[size_t(i)];
			r = FrameRec{};
			r.flags = FRAME_HAS_CKSUM;
			r.out_off = uint64_t(off[i]);
			r.out_len = uint64_t(len[i]);
			r.fail = -1;
		}
		DevBuf<FrameRec> d_rec;
		d_rec.reserve(recs.size());
		vec_h2d(d_rec, recs, nullptr);
		struct Events {
			hipEvent_t a = nullptr, b = nullptr;
			~Events()
			{
				if (a)
					(void)hipEventDestroy(a);
				if (b)
					(void)hipEventDestroy(b);
			}
		} ev;
		HIP_OK(hipEventCreate(&ev.a));
		HIP_OK(hipEventCreate(&ev.b));
		HIP_OK(hipEventRecord(ev.a, nullptr));
		HIP_OK(launch_xxh32_spans(static_cast<const uint8_t*>(d_buf), d_rec.p, uint32_t(nspans),
		                          ~uint64_t(0), nullptr));
		HIP_OK(hipEventRecord(ev.b, nullptr));
		vec_d2h(recs, d_rec, nullptr);
		if (kernel_ms)
			HIP_OK(hipEventElapsedTime(kernel_ms, ev.a, ev.b));
		for (int64_t i = 0; i < nspans; ++i)
			hash[i] = recs[size_t(i)].hash;
	});
}

}  // extern "C"
