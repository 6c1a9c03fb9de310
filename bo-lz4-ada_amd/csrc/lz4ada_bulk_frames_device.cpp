// lz4ada_bulk_frames_device.cpp -- many frames that already lie in device
// memory, decoded into device memory.  The device half of the
// pass is the host engine's too (decode_pass, lz4ada_frames_pass.cpp); what
// differs is where its index comes from and where its bytes go: the frames are
// indexed where they lie by k_frames_walk / k_frames_scan / k_frames_fill
// (lz4ada_frames_index.hip), the decoders read the caller's d_in itself, and
// the compaction writes into the caller's d_out.  The host sees the per-frame
// walk records (one D2H per call: verdicts and sizes, from which it sizes the
// scratch and splits the passes by the byte budget) and the per-frame pass
// records (one D2H per pass); no payload byte crosses, except that a content
// checksum over more than lz4ada_batch_hash_max() bytes is hashed by the host
// chain (content_xxh32_d2h with no host destination).  A frame the pass does
// not find good in every respect gets LZ4ADA_EXACT_PATH and a reason; this
// unit invents no exception text.  With LZ4ADA_FRAMES_LINKED the walk accepts
// linked frames up to lz4ada_batch_linked_max().  With
// LZ4ADA_FRAMES_EXACT, and in lz4ada_frames_device_sizes, a sizes stage finds
// what every accepted frame decodes to without decoding it (lz4ada_sizes.hip,
// one more D2H of per-frame records per call), and the passes are laid out by
// those sizes instead of the slot capacities.  The _dict calls
// are the same passes with a gap in front of the slots that need one, filled
// with the dictionary's tail, and the dictionary decoders.
#include "lz4ada_block_size.h"
#include "lz4ada_frame_walk.h"
#include "lz4ada_host_common.h"

using namespace lz4ada;

namespace lz4ada {
namespace {

static_assert(WALK_LONE_MAX_IN == LONE_MAX_IN, "the walk states the lone-block rule a second time");

// Blocks per chunk of the sizes stage: its descriptors, statuses and index
// table are temporary, 160 bytes per block (and a quarter of the input for the
// table, whatever the chunk).  LZ4ADA_SIZES_CHUNK_BLOCKS, read per call,
// overrides it (the tests cut a call into many chunks with it).
constexpr int64_t SIZES_CHUNK_BLOCKS = int64_t(1) << 20;

[[noreturn]] void misuse(const char* entry, const std::string& what)
{
	raise(LZ4ADA_ASSERTION_ERROR, std::string(entry) + ": " + what);
}

}  // namespace

// The argument checks (nothing is launched before they pass), the sort, and
// the walk of every job's frame with its one host synchronisation.
void index_jobs(const char* entry, const void* d_in, int64_t in_len, const lz4ada_device_frame_job* jobs,
                int64_t njobs, uint32_t flags, hipStream_t stream, FramesIndex& ix)
{
	ix.take_linked = (flags & LZ4ADA_FRAMES_LINKED) != 0;
	ix.linked_max = uint64_t(batch_linked_max());
	if (njobs < 0 || (njobs > 0 && !jobs) || in_len < 0 || (in_len > 0 && !d_in) ||
	    njobs >= (int64_t(1) << 31))
		misuse(entry, "jobs or d_in is NULL, or a count is out of range");
	const size_t n = size_t(njobs);
	for (size_t i = 0; i < n; ++i)
		if (jobs[i].in_off < 0 || jobs[i].in_len < 0 || jobs[i].in_off > in_len ||
		    jobs[i].in_len > in_len - jobs[i].in_off)
			misuse(entry, "job" + img(int64_t(i)) + " lies outside the input");
	ix.order.resize(n);
	for (size_t i = 0; i < n; ++i)
		ix.order[i] = uint32_t(i);
	std::stable_sort(ix.order.begin(), ix.order.end(),
	                 [&](uint32_t a, uint32_t b) { return jobs[a].in_off < jobs[b].in_off; });
	// Two jobs' ranges may share bytes only when the earlier one runs to the
	// end of the input (the frame and whatever follows it); its frame is
	// checked against the next job once the walk has found its length.
	for (size_t k = 0; k + 1 < n; ++k) {
		const auto &a = jobs[ix.order[k]], &b = jobs[ix.order[k + 1]];
		if (a.in_off + a.in_len > b.in_off && a.in_off + a.in_len != in_len)
			misuse(entry, "jobs" + img(int64_t(ix.order[k])) + " and" + img(int64_t(ix.order[k + 1])) +
			                      " overlap");
	}
	ix.walk.assign(n, FrameWalkRec{});
	ix.span.resize(n);
	if (n == 0)
		return;
	device_check_or_raise();
	const size_t span_b = n * sizeof(FrameSpan), walk_b = n * sizeof(FrameWalkRec), scan_b = (n + 1) * 8;
	uint8_t* const d = scratch(SC_FRAME, span_b + walk_b + 2 * scan_b);
	if (!d)
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the frame index");
	ix.d_span = reinterpret_cast<FrameSpan*>(d);
	ix.d_walk = reinterpret_cast<FrameWalkRec*>(d + span_b);
	ix.d_first = reinterpret_cast<uint64_t*>(d + span_b + walk_b);
	ix.d_slot = reinterpret_cast<uint64_t*>(d + span_b + walk_b + scan_b);
	PinBuf& h = scratch_cache().pin;  // this thread's small pinned transfers
	h.reserve(std::max(span_b, walk_b));
	for (size_t k = 0; k < n; ++k)
		ix.span[k] = FrameSpan{ uint64_t(jobs[ix.order[k]].in_off), uint64_t(jobs[ix.order[k]].in_len) };
	memcpy(h.p, ix.span.data(), span_b);
	HIP_OK(hipMemcpyAsync(ix.d_span, h.p, span_b, hipMemcpyHostToDevice, stream));
	HIP_OK(launch_frames_walk(static_cast<const uint8_t*>(d_in), ix.d_span, uint32_t(n), lone_blocks_disabled(),
	                          uint64_t(batch_budget()), ix.take_linked, ix.linked_max, ix.d_walk, stream));
	// the index's host synchronisation: verdicts and sizes, no frame byte
	HIP_OK(hipMemcpyAsync(h.p, ix.d_walk, walk_b, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	memcpy(ix.walk.data(), h.p, walk_b);
	for (size_t k = 0; k + 1 < n; ++k)
		if (ix.taken(k) && ix.span[k].off + uint64_t(ix.walk[k].frame_len) > ix.span[k + 1].off)
			misuse(entry, "the frame of job" + img(int64_t(ix.order[k])) + " reaches into job" +
			                      img(int64_t(ix.order[k + 1])));
}

// What the index alone says about every job, and the bound: what the frames
// a pass takes can decode to.
int64_t report_index(const FramesIndex& ix, lz4ada_device_frame_job* jobs)
{
	uint64_t bound = 0;
	for (size_t k = 0; k < ix.order.size(); ++k) {
		lz4ada_device_frame_job& j = jobs[ix.order[k]];
		j.out_off = j.out_len = j.consumed = 0;
		j.status = ix.taken(k) ? LZ4ADA_OK : LZ4ADA_EXACT_PATH;
		j.reason = ix.walk[k].verdict;
		if (ix.taken(k))
			bound += ix.walk[k].caps;
	}
	return int64_t(bound);
}

// The sizes stage: the exact decoded size of every block of every accepted
// frame, without decoding (k_index's records added up, or the wave's own walk
// of the chain: lz4ada_sizes.hip), in chunks of whole frames.  A chunk fills
// temporary descriptors with the nominal slots (SC_BATCH_META, which a pass
// lays out anew), indexes them (SC_TAB) and needs no output slot.  What the
// passes need stays in SC_SIZES for the call.  One host synchronisation: the
// per-frame size records.  A frame the sizes fail is no longer taken(), with
// LZ4ADA_DEVFRAME_BLOCK or _SIZE as its verdict, on the host and on the device.
void size_jobs(FramesIndex& ix, const uint8_t* d_in, uint64_t in_len, hipStream_t stream)
{
	const size_t n = ix.order.size();
	ix.sized = true;
	ix.size.assign(n, FrameSizeRec{});
	if (n == 0)
		return;
	// the chunks: sorted jobs [lo, hi) and their blocks
	struct Chunk {
		size_t lo, hi;
		uint64_t nb;
	};
	std::vector<Chunk> chunks;
	const uint64_t chunk_blocks = uint64_t(env_bytes("LZ4ADA_SIZES_CHUNK_BLOCKS", SIZES_CHUNK_BLOCKS));
	uint64_t nb_all = 0, nb_max = 0;
	size_t nf_max = 0;
	for (size_t lo = 0; lo < n;) {
		size_t hi = lo;
		uint64_t nb = 0;
		for (; hi < n; ++hi) {
			const uint64_t add = ix.taken(hi) ? ix.walk[hi].nblocks : 0;
			if (hi > lo && nb + add > chunk_blocks)
				break;
			nb += add;
		}
		if (nb >= (uint64_t(1) << 31))  // one frame of 2^31 blocks or more
			raise(LZ4ADA_CONSTRAINT_ERROR, "a frame holds more blocks than a pass takes");
		chunks.push_back(Chunk{ lo, hi, nb });
		nb_all += nb;
		nb_max = std::max(nb_max, nb);
		nf_max = std::max(nf_max, hi - lo);
		lo = hi;
	}
	const size_t tight_b = n * sizeof(FrameWalkRec), first_b = n * 8, rec_b = n * sizeof(FrameSizeRec);
	uint8_t* const p = scratch(SC_SIZES, tight_b + first_b + rec_b + size_t(nb_all) * 4);
	const size_t desc_b = size_t(nb_max) * sizeof(lz4ada_block_desc), frec_b = nf_max * sizeof(FrameRec);
	uint8_t* const t = scratch(SC_BATCH_META, desc_b + frec_b + size_t(nb_max) * sizeof(lz4ada_block_status));
	uint8_t* const d_tab = nb_max ? scratch(SC_TAB, index_table_bytes(in_len, uint32_t(nb_max))) : nullptr;
	if (!p || !t || (nb_max && !d_tab))
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the sizes stage");
	ix.d_tight = reinterpret_cast<FrameWalkRec*>(p);
	ix.d_size_first = reinterpret_cast<uint64_t*>(p + tight_b);
	FrameSizeRec* const d_rec = reinterpret_cast<FrameSizeRec*>(p + tight_b + first_b);
	ix.d_size = reinterpret_cast<uint32_t*>(p + tight_b + first_b + rec_b);
	lz4ada_block_desc* const d_desc = reinterpret_cast<lz4ada_block_desc*>(t);
	FrameRec* const d_frec = reinterpret_cast<FrameRec*>(t + desc_b);
	lz4ada_block_status* const d_st = reinterpret_cast<lz4ada_block_status*>(t + desc_b + frec_b);
	uint64_t base = 0;  // the chunk's first block among the call's sizes
	for (const Chunk& c : chunks) {
		const uint32_t nf = uint32_t(c.hi - c.lo), nb = uint32_t(c.nb);
		HIP_OK(launch_frames_scan(ix.d_walk + c.lo, nf, ix.d_first, ix.d_slot, stream));
		HIP_OK(launch_frames_fill(d_in, ix.d_span + c.lo, ix.d_walk + c.lo, ix.d_first, ix.d_slot, nf,
		                          lone_blocks_disabled(), ix.take_linked, ix.linked_max, d_desc, d_frec, stream));
		if (nb) {
			HIP_OK(hipMemsetAsync(d_st, 0, size_t(nb) * sizeof(lz4ada_block_status), stream));
			HIP_OK(launch_index(d_in, in_len, d_desc, nb, d_tab, d_st, stream));
			HIP_OK(launch_block_sizes(d_in, in_len, d_desc, d_st, nb, d_tab, ix.d_size + base, stream));
		}
		HIP_OK(launch_frame_sizes(ix.d_walk + c.lo, ix.d_first, nf, base, d_desc, ix.d_size + base, d_rec + c.lo,
		                          ix.d_size_first + c.lo, ix.d_tight + c.lo, stream));
		base += nb;
	}
	// the stage's host synchronisation: sizes and verdicts, no frame byte
	PinBuf& h = scratch_cache().pin;
	h.reserve(rec_b);
	HIP_OK(hipMemcpyAsync(h.p, d_rec, rec_b, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	memcpy(ix.size.data(), h.p, rec_b);
	for (size_t k = 0; k < n; ++k)
		if (ix.taken(k))
			ix.walk[k].verdict = ix.size[k].verdict;
}

// What the sizes stage says about every job: report_index with the exact
// length of every accepted frame, and their sum.
int64_t report_sizes(const FramesIndex& ix, lz4ada_device_frame_job* jobs)
{
	report_index(ix, jobs);
	uint64_t total = 0;
	for (size_t k = 0; k < ix.order.size(); ++k)
		if (ix.taken(k)) {
			jobs[ix.order[k]].out_len = int64_t(ix.size[k].exact);
			total += ix.size[k].exact;
		}
	return int64_t(total);
}

// The blocks of sorted job k that get a gap: every block of an independent
// modern frame, the first of a linked one.
uint64_t gapped_blocks(const FramesIndex& ix, size_t k)
{
	if (!ix.taken(k) || ix.walk[k].format != LZ4ADA_FORMAT_MODERN || ix.walk[k].nblocks == 0)
		return 0;
	return ix.linked(k) ? 1 : ix.walk[k].nblocks;
}

// LZ4ADA_DICT_CHECK_ID: a taken modern frame that names another dictionary id
// is no longer taken(), with LZ4ADA_DEVFRAME_DICT as its verdict, on the host
// and on the device.  One host synchronisation: a word per frame.
void check_dict_ids(FramesIndex& ix, const uint8_t* d_in, uint32_t dict_id, hipStream_t stream)
{
	const size_t n = ix.order.size();
	if (n == 0)
		return;
	uint32_t* const d_bad = reinterpret_cast<uint32_t*>(scratch(SC_DICT, n * 4));
	if (!d_bad)
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the dictionary ids");
	HIP_OK(launch_frames_dictid(d_in, ix.d_span, ix.d_walk, uint32_t(n), dict_id, d_bad, stream));
	PinBuf& h = scratch_cache().pin;
	h.reserve(n * 4);
	HIP_OK(hipMemcpyAsync(h.p, d_bad, n * 4, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	const uint32_t* bad = reinterpret_cast<const uint32_t*>(h.p);
	for (size_t k = 0; k < n; ++k)
		if (bad[k] && ix.taken(k))
			ix.walk[k].verdict = LZ4ADA_DEVFRAME_DICT;
}

// A dictionary pass over the sorted jobs [lo, hi), once its descriptors are
// filled: the gaps (k_frames_dictgap from a word per frame, written to the
// pinned h_kind and sent up from there), their bytes (k_dict_fill), and the
// runs cut again so that legacy frames, which read no dictionary, keep
// launch_decode_checked while modern ones take the dictionary decoders.
// `total`: the pass's slots and gaps, what SC_OUT holds.
void lay_dict_pass(PassArrays& m, const FramesIndex& ix, size_t lo, size_t hi, uint64_t total, uint64_t in_len,
                   const DictCtx& dc, uint64_t* h_kind, hipStream_t stream)
{
	const size_t kind_b = size_t(m.nf) * 8;
	uint64_t* const d_kind = reinterpret_cast<uint64_t*>(scratch(SC_DICT, kind_b));
	if (!d_kind)
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the pass's gaps");
	uint64_t before = 0;
	for (size_t k = lo; k < hi; ++k) {
		const uint64_t g = gapped_blocks(ix, k);
		h_kind[k - lo] = (before << 2) | (g == 0 ? DICT_KIND_NONE : ix.linked(k) ? DICT_KIND_LINKED : DICT_KIND_INDEP);
		before += g;
	}
	HIP_OK(hipMemcpyAsync(d_kind, h_kind, kind_b, hipMemcpyHostToDevice, stream));
	HIP_OK(launch_frames_dictgap(m.d_rec, m.nf, d_kind, dc.gap, total, m.d_desc, m.nb, stream));
	HIP_OK(launch_dict_fill(m.d_desc, m.nb, dc.d_dict, dc.len, dc.used, m.d_slots, stream));
	// the runs: a linked run takes the dictionary as it is; an independent one
	// is cut where legacy and modern frames meet
	std::vector<PassRun> runs;
	for (const PassRun& r : m.runs) {
		if (r.linked) {
			runs.push_back(r);
			runs.back().dict = true;
			continue;
		}
		std::vector<PassFrame> fr;
		for (uint32_t f = r.f0; f < r.f1; ++f) {
			const size_t k = lo + f;
			fr.push_back(PassFrame{ ix.taken(k) ? uint32_t(ix.walk[k].nblocks) : 0u,
			                        ix.walk[k].format == LZ4ADA_FORMAT_MODERN });
		}
		for (PassRun q : pass_runs(fr)) {  // (`linked` there: modern)
			q.dict = q.linked;
			q.linked = false;
			q.b0 += r.b0, q.b1 += r.b0, q.f0 += r.f0, q.f1 += r.f0;
			runs.push_back(q);
		}
	}
	m.runs = runs;
	m.dict_used = dc.used;
	if (!m.d_tab && m.nb && !(m.d_tab = scratch(SC_TAB, index_table_bytes(in_len, m.nb))))
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the pass's sequence index");
}

// Room on the device for a pass over the sorted jobs [lo, hi), their blocks as
// k_frames_scan counts them: a frame the index did not take rides without any.
void reserve_pass(PassArrays& a, const FramesIndex& ix, size_t lo, size_t hi, uint64_t slots,
                  uint64_t in_len)
{
	std::vector<PassFrame> frames;
	for (size_t k = lo; k < hi; ++k)
		frames.push_back(PassFrame{ ix.taken(k) ? uint32_t(ix.walk[k].nblocks) : 0u, ix.linked(k) });
	if (const char* what = a.reserve(frames, slots, in_len))
		raise(LZ4ADA_DEVICE_ERROR, std::string("no device memory for the pass's ") + what);
}

// The scan and the fill over the sorted jobs [lo, hi): descriptors and frame
// records of a pass, on the device.
void fill_pass(const FramesIndex& ix, size_t lo, size_t hi, const uint8_t* d_in, const PassArrays& m,
               hipStream_t stream)
{
	// sized: the scan adds up the tight slots, the fill lays the nominal ones
	// out from each frame's tight base, and the refit puts every block where
	// its size says (out_cap = size, steps of round256(size))
	HIP_OK(launch_frames_scan((ix.sized ? ix.d_tight : ix.d_walk) + lo, m.nf, ix.d_first, ix.d_slot, stream));
	HIP_OK(launch_frames_fill(d_in, ix.d_span + lo, ix.d_walk + lo, ix.d_first, ix.d_slot, m.nf,
	                          lone_blocks_disabled(), ix.take_linked, ix.linked_max, m.d_desc, m.d_rec, stream));
	if (ix.sized)
		HIP_OK(launch_frames_refit(ix.d_tight + lo, ix.d_first, ix.d_slot, ix.d_size_first + lo, ix.d_size, m.nf,
		                           m.d_desc, stream));
}

namespace {

void job_rejected(lz4ada_device_frame_job& j, int reason)
{
	j.out_off = j.out_len = j.consumed = 0;
	j.status = LZ4ADA_EXACT_PATH;
	j.reason = reason;
}

void job_skipped(lz4ada_device_frame_job& j, const FrameWalkRec& w, uint64_t at)
{
	j.out_off = int64_t(at);
	j.consumed = w.frame_len;
	++batch_stats().frames_batched;
	add_last_path(LZ4ADA_PATH_BATCH);
}

// One pass over the sorted jobs [lo, hi) (`slots` slot bytes, a dictionary
// pass's gaps included): their bytes go to d_out from *base on, which then
// moves past them.  The jobs are sorted and their frames disjoint, and in_len
// covers every block, as decode_pass asks.
void run_device_pass(const FramesIndex& ix, size_t lo, size_t hi, uint64_t slots, const uint8_t* d_in,
                     uint64_t in_len, lz4ada_device_frame_job* jobs, uint8_t* d_out, uint64_t* base,
                     uint64_t hash_max, hipStream_t stream, const DictCtx* dc = nullptr)
{
	PassArrays m;
	reserve_pass(m, ix, lo, hi, slots, in_len);
	uint8_t* const dst = d_out + *base;
	fill_pass(ix, lo, hi, d_in, m, stream);
	PinBuf& h = scratch_cache().pin;  // this thread's small pinned transfers
	h.reserve(std::max(m.rec_b, dc ? size_t(m.nf) * 8 : size_t(0)));
	if (dc)
		lay_dict_pass(m, ix, lo, hi, slots, in_len, *dc, reinterpret_cast<uint64_t*>(h.p), stream);
	FrameRec* const rec = reinterpret_cast<FrameRec*>(h.p);
	decode_pass(m, d_in, in_len, dst, hash_max, rec, stream);
	lz4ada_batch_stats& stats = batch_stats();
	for (size_t k = lo; k < hi; ++k) {
		if (!ix.taken(k))
			continue;
		const FrameRec& r = rec[k - lo];
		lz4ada_device_frame_job& j = jobs[ix.order[k]];
		if (ix.skippable(k)) {  // consumed, no output: its place among the others'
			job_skipped(j, ix.walk[k], *base + r.out_off);
			continue;
		}
		bool hashed = false;
		const FrameVerdict v = frame_verdict(r, ix.walk[k].cksum, &hashed);
		int reason = v == FV_HOST_HASH ? LZ4ADA_DEVFRAME_OK : int(v);
		stats.gpu_hashed += hashed && (v == FV_GOOD || v == FV_CHECKSUM) ? 1 : 0;
		if (v == FV_HOST_HASH) {
			// over hash_max: the host chain, the one place where decoded bytes
			// visit the host, and only to be hashed
			lz4ada_xxh32_state hs;
			lz4ada_xxh32_reset(&hs, 0);
			content_xxh32_d2h(hs, dst + r.out_off, int64_t(r.out_len), nullptr, stream);
			++stats.host_hashed;
			if (host_xxh32_final(hs) != ix.walk[k].cksum)
				reason = LZ4ADA_DEVFRAME_CHECKSUM;
		}
		if (reason != LZ4ADA_DEVFRAME_OK) {
			job_rejected(j, reason);
			continue;
		}
		j.out_off = int64_t(*base + r.out_off);
		j.out_len = int64_t(r.out_len);
		j.consumed = ix.walk[k].frame_len;
		j.status = LZ4ADA_OK;
		j.reason = LZ4ADA_DEVFRAME_OK;
		++stats.frames_batched;
		add_last_path(LZ4ADA_PATH_BATCH | (ix.linked(k) ? LZ4ADA_PATH_LINKED : LZ4ADA_PATH_INDEPENDENT));
	}
	*base += rec[m.nf - 1].out_off + rec[m.nf - 1].out_len;
}

}  // namespace

// API misuse of a _dict call's dictionary, before any launch.
void check_dict(const char* entry, const lz4ada_device_dict* dict)
{
	if (!dict)
		return;
	if (dict->dict_len < 0 || (dict->dict_len > 0 && !dict->d_dict))
		misuse(entry, "dict_len is negative, or d_dict is NULL");
	if (dict->flags & ~LZ4ADA_DICT_CHECK_ID)
		misuse(entry, "unknown bits in dict->flags");
}

namespace {

// lz4ada_decode_frames_device_opt, and with a dictionary of dict_len > 0 the
// _dict call: the same index, sizes and passes, the gaps charged against the
// budget, and every pass laid out and decoded with the dictionary.
int decode_frames_device(const char* entry, const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs,
                         int64_t njobs, uint32_t flags, const lz4ada_device_dict* dict, void* d_out,
                         int64_t out_cap, int64_t* out_len, void* stream)
{
	*out_len = 0;
	batch_stats() = lz4ada_batch_stats{};
	set_last_path(0);
	return guarded(nullptr, [&] {
		hipStream_t s = static_cast<hipStream_t>(stream);
		check_dict(entry, dict);
		DictCtx dctx{}, *dc = nullptr;
		if (dict && dict->dict_len > 0) {
			dctx.d_dict = static_cast<const uint8_t*>(dict->d_dict);
			dctx.len = uint64_t(dict->dict_len);
			dctx.used = uint32_t(std::min<uint64_t>(dctx.len, DICT_MAX));
			dctx.gap = dict_gap(dctx.used);
			dc = &dctx;
		}
		FramesIndex ix;
		index_jobs(entry, d_in, in_len, jobs, njobs, flags, s, ix);
		if (dc && (dict->flags & LZ4ADA_DICT_CHECK_ID))
			check_dict_ids(ix, static_cast<const uint8_t*>(d_in), dict->dict_id, s);
		// LZ4ADA_FRAMES_EXACT: the sizes stage, then the frames it passed laid
		// out by their sizes; what suffices is their sum, not the bound
		if (flags & LZ4ADA_FRAMES_EXACT)
			size_jobs(ix, static_cast<const uint8_t*>(d_in), uint64_t(in_len), s);
		const int64_t sizes_total = ix.sized ? report_sizes(ix, jobs) : 0;
		const int64_t index_bound = report_index(ix, jobs);
		const int64_t bound = ix.sized ? sizes_total : index_bound;
		if (out_cap < bound || (bound > 0 && !d_out)) {
			*out_len = bound;
			raise(LZ4ADA_TOO_LITTLE_MEMORY, std::string(entry) + ": the output holds" + img(out_cap) +
			                                        " bytes, the frames may decode to" + img(bound));
		}
		const uint64_t budget = uint64_t(batch_budget()), hash_max = uint64_t(batch_hash_max());
		uint64_t base = 0;
		const size_t n = ix.order.size();
		size_t lo = 0;
		while (lo < n) {
			// the sorted jobs [lo, hi): as many frames as the budget takes
			// (a dictionary pass's gaps are scratch like its slots)
			const PassCut cut = pass_cut(lo, n, budget, [&](size_t k) {
				return PassCost{ ix.taken(k), ix.slots(k) + (dc ? dc->gap * gapped_blocks(ix, k) : 0),
					         ix.walk[k].nblocks };
			});
			const size_t hi = cut.hi;
			if (hi == lo)  // one frame of 2^31 blocks or more
				raise(LZ4ADA_CONSTRAINT_ERROR, "a frame holds more blocks than a pass takes");
			bool real = false;  // a frame that is taken and not skippable
			for (size_t k = lo; k < hi; ++k)
				real |= ix.taken(k) && !ix.skippable(k);
			if (real) {
				run_device_pass(ix, lo, hi, cut.bytes, static_cast<const uint8_t*>(d_in), uint64_t(in_len), jobs,
				                static_cast<uint8_t*>(d_out), &base, hash_max, s, dc);
			} else {  // nothing but skippable frames, if any: no launch
				for (size_t k = lo; k < hi; ++k)
					if (ix.taken(k))
						job_skipped(jobs[ix.order[k]], ix.walk[k], base);
			}
			lo = hi;
		}
		*out_len = int64_t(base);
	});
}

}  // namespace
}  // namespace lz4ada

extern "C" {

int lz4ada_frame_walk_host(const uint8_t* frame, int64_t len, lz4ada_frame_info* info, lz4ada_block_desc* descs,
                           int64_t desc_cap)
{
	WalkSums sums;
	WalkEmit e{};
	e.descs = descs;
	e.cap = desc_cap;
	return frame_walk(frame, len, lone_blocks_disabled(), info, &sums, descs ? &e : nullptr);
}

int lz4ada_frame_walk_host_opt(const uint8_t* frame, int64_t len, uint32_t flags, lz4ada_frame_info* info,
                               lz4ada_block_desc* descs, int64_t desc_cap)
{
	WalkSums sums;
	WalkEmit e{};
	e.descs = descs;
	e.cap = desc_cap;
	return frame_walk(frame, len, lone_blocks_disabled(), info, &sums, descs ? &e : nullptr,
	                  (flags & LZ4ADA_FRAMES_LINKED) != 0, uint64_t(batch_linked_max()));
}

int lz4ada_frames_device_bound(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs, int64_t njobs,
                               int64_t* bound, void* stream)
{
	return lz4ada_frames_device_bound_opt(d_in, in_len, jobs, njobs, batch_env_flags(), bound, stream);
}

int lz4ada_frames_device_bound_opt(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs,
                                   int64_t njobs, uint32_t flags, int64_t* bound, void* stream)
{
	*bound = 0;
	batch_stats() = lz4ada_batch_stats{};
	return guarded(nullptr, [&] {
		FramesIndex ix;
		index_jobs("lz4ada_frames_device_bound", d_in, in_len, jobs, njobs, flags,
		           static_cast<hipStream_t>(stream), ix);
		*bound = report_index(ix, jobs);
	});
}

int lz4ada_frames_device_sizes(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs, int64_t njobs,
                               uint32_t flags, int64_t* total, void* stream)
{
	*total = 0;
	batch_stats() = lz4ada_batch_stats{};
	return guarded(nullptr, [&] {
		hipStream_t s = static_cast<hipStream_t>(stream);
		FramesIndex ix;
		index_jobs("lz4ada_frames_device_sizes", d_in, in_len, jobs, njobs, flags, s, ix);
		size_jobs(ix, static_cast<const uint8_t*>(d_in), uint64_t(in_len), s);
		*total = report_sizes(ix, jobs);
	});
}

int64_t lz4ada_block_size_host(const uint8_t* block, int64_t n, int stored)
{
	return block_decoded_size(block, n, stored != 0);
}

int lz4ada_decode_frames_device(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs, int64_t njobs,
                                void* d_out, int64_t out_cap, int64_t* out_len, void* stream)
{
	return lz4ada_decode_frames_device_opt(d_in, in_len, jobs, njobs, batch_env_flags(), d_out, out_cap, out_len,
	                                       stream);
}

int lz4ada_decode_frames_device_opt(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs,
                                    int64_t njobs, uint32_t flags, void* d_out, int64_t out_cap,
                                    int64_t* out_len, void* stream)
{
	return decode_frames_device("lz4ada_decode_frames_device", d_in, in_len, jobs, njobs, flags, nullptr, d_out,
	                            out_cap, out_len, stream);
}

int lz4ada_frames_device_bound_dict(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs,
                                    int64_t njobs, uint32_t flags, const lz4ada_device_dict* dict,
                                    int64_t* bound, void* stream)
{
	*bound = 0;
	batch_stats() = lz4ada_batch_stats{};
	return guarded(nullptr, [&] {
		check_dict("lz4ada_frames_device_bound_dict", dict);
		hipStream_t s = static_cast<hipStream_t>(stream);
		FramesIndex ix;
		index_jobs("lz4ada_frames_device_bound_dict", d_in, in_len, jobs, njobs, flags, s, ix);
		if (dict && dict->dict_len > 0 && (dict->flags & LZ4ADA_DICT_CHECK_ID))
			check_dict_ids(ix, static_cast<const uint8_t*>(d_in), dict->dict_id, s);
		*bound = report_index(ix, jobs);
	});
}

int lz4ada_decode_frames_device_dict(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs,
                                     int64_t njobs, uint32_t flags, const lz4ada_device_dict* dict, void* d_out,
                                     int64_t out_cap, int64_t* out_len, void* stream)
{
	const bool none = !dict || dict->dict_len == 0;
	return decode_frames_device(none ? "lz4ada_decode_frames_device" : "lz4ada_decode_frames_device_dict", d_in,
	                            in_len, jobs, njobs, flags, dict, d_out, out_cap, out_len, stream);
}

int lz4ada_frames_index_device_debug(const void* d_in, int64_t in_len, const lz4ada_device_frame_job* jobs,
                                     int64_t njobs, int32_t* verdict, int64_t* nblocks, lz4ada_block_desc* descs,
                                     int64_t desc_cap, void* stream)
{
	return guarded(nullptr, [&] {
		hipStream_t s = static_cast<hipStream_t>(stream);
		FramesIndex ix;
		index_jobs("lz4ada_frames_index_device_debug", d_in, in_len, jobs, njobs, batch_env_flags(), s, ix);
		const size_t n = ix.order.size();
		uint64_t nb = 0;
		for (size_t k = 0; k < n; ++k) {
			verdict[ix.order[k]] = ix.walk[k].verdict;
			nblocks[ix.order[k]] = ix.walk[k].format ? int64_t(ix.walk[k].nblocks) : 0;
			nb += ix.taken(k) ? ix.walk[k].nblocks : 0;
		}
		if (nb > uint64_t(std::max<int64_t>(desc_cap, 0)) || nb >= (uint64_t(1) << 31))
			raise(LZ4ADA_CONSTRAINT_ERROR, "descriptor capacity exceeded");
		if (n == 0 || nb == 0)
			return;
		PassArrays m;
		reserve_pass(m, ix, 0, n, 0, uint64_t(in_len));
		fill_pass(ix, 0, n, static_cast<const uint8_t*>(d_in), m, s);
		d2h(descs, m.d_desc, m.desc_b, s);
	});
}

}  // extern "C"
