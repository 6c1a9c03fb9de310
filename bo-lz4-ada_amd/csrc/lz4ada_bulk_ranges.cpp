// lz4ada_bulk_ranges.cpp -- a seek index over device-resident frames and the
// ranged decode that reads through it.  The build is the
// index and sizes stages of lz4ada_bulk_frames_device.cpp (index_jobs,
// size_jobs) and then keeps what they found: the descriptors of every
// accepted frame's blocks (launch_frames_scan / _fill once over all frames)
// and, from k_block_starts, the decoded offset at which each block starts,
// in device memory the index owns.  A ranged call selects the blocks its
// ranges touch (k_ranges_select; one D2H of the selection records), cuts the
// ranges into passes by LZ4ADA_BATCH_BYTES, and per pass compacts the marked
// blocks' descriptors (k_ranges_scan, k_ranges_fill), decodes them with the
// passes' own decoders and block checksums (launch_decode_checked), judges
// every range by the blocks it touches (k_ranges_verdict) and copies its bytes
// to the caller's buffer (k_ranges_gather); one D2H of the records per pass.
// The index is immutable after the build; a ranged call works in the calling
// thread's scratch roles (SC_FRAME: the range records, SC_BATCH_META: the
// pass's arrays, SC_OUT: the slots), so any number of threads may share one.
//
// With LZ4ADA_SEEK_LINKED (lz4ada_seek_index_build_opt) the
// index takes linked frames: the build decodes each once with the linked run
// of §12 (decode_linked_frames: the device engine's own pass stages and
// decode_pass_blocks over a view of the index) and keeps the
// 64 KiB in front of every K-th block in a store of its own (k_ckpt_save).  A range of a linked frame marks
// its chain (lz4ada_range_chains.h): the pass lays a gap in front of every
// head, fills it with the head's checkpoint (k_ckpt_fill) and decodes the
// chains with the dictionary decoder of §15, one wave per chain, beside the
// independent frames' launch_decode_checked; SC_TAB holds the sequence index.
//
// With a dictionary (lz4ada_seek_index_build_dict) the index
// keeps its own copy of the dictionary's used bytes as a gap image, and a word
// per frame that says which of its blocks read it.  A pass lays a second kind
// of gap, the dictionary's, in front of every such marked block
// (k_dictimg_fill), makes each the start of a chain, and decodes the chains of
// all kinds -- from a checkpoint, from the dictionary -- in one launch that
// takes the history length per chain (k_decode_idx_chains).  Legacy frames keep
// launch_decode_checked.
//
// An index may also come from the compress call that wrote the frames
// (lz4ada_compress_frames_device_indexed): comp_index_open / _pass
// / _close below fill the same object from what the writer knows, through the
// allocation layouts and the dictionary image the builds use (alloc_index,
// alloc_checkpoints, lay_dict_image), and the ranged calls cannot tell the two
// apart.
#include <climits>

#include "lz4ada_compress_index.h"
#include "lz4ada_host_common.h"
#include "lz4ada_index_merge.h"
#include "lz4ada_range_blocks.h"
#include "lz4ada_range_chains.h"

using namespace lz4ada;

namespace lz4ada {

// One hipMalloc'd block, freed with its owner.
struct DevMem {
	uint8_t* p = nullptr;
	size_t bytes = 0;
	DevMem() = default;
	DevMem(const DevMem&) = delete;
	DevMem& operator=(const DevMem&) = delete;
	~DevMem()
	{
		if (p)
			(void)hipFree(p);
	}
	// `what`: whose memory, for the text when the device has none
	uint8_t* alloc(size_t n, const char* what)
	{
		void* q = nullptr;
		if (hipMalloc(&q, n) != hipSuccess) {
			(void)hipGetLastError();
			raise(LZ4ADA_DEVICE_ERROR, std::string("no device memory for ") + what);
		}
		p = static_cast<uint8_t*>(q);
		bytes = n;
		return p;
	}
};

}  // namespace lz4ada

struct lz4ada_seek_index {
	int64_t in_len = 0;  // the input it was built over
	DevMem mem;          // desc | first | start | slotp | with a dictionary: fkind
	// LZ4ADA_SEEK_LINKED: store | ckfirst | kgrp, and by sorted position what the
	// last two hold (kgrp: n entries, K or 0; ckfirst: n + 1)
	DevMem ck;
	std::vector<uint64_t> kgrp, ckfirst;
	bool linked = false;  // it holds a linked frame
	// a dictionary index: the gap image (dict.gap bytes: zeros, then the last
	// dict.used bytes of the dictionary) as the passes' dictionary, and by sorted
	// position the frame's CHAIN_KIND_* (empty without a dictionary: every frame
	// CHAIN_KIND_NONE); all zero without one
	DevMem dict_mem;
	DictCtx dict{};
	std::vector<uint8_t> kind;
	SeekView view{};
	uint64_t* d_start = nullptr;
	// by job
	std::vector<uint32_t> pos;  // its sorted position
	std::vector<int32_t> reason;
	std::vector<uint64_t> size;  // decoded bytes; 0 unless accepted
	// by sorted position, n + 1 entries: what view.first holds
	std::vector<uint64_t> first;
	// the nominal slots of the frames taken: where the out_off of a next frame's
	// first block would lie (what a concat rebases a later part's out_off by)
	uint64_t slots = 0;
	bool taken(size_t job) const { return reason[job] == LZ4ADA_DEVFRAME_OK; }
};

namespace lz4ada {
namespace {

[[noreturn]] void misuse(const char* entry, const std::string& what)
{
	raise(LZ4ADA_ASSERTION_ERROR, std::string(entry) + ": " + what);
}

// LZ4ADA_SEEK_LINKED with checkpoint_bytes == 0: a checkpoint per MiB decoded.
// A choice, not a measurement taken beforehand (DESIGN.md §16 has the table): the
// store is then at most 1/16 of the decoded size for any block maximum up to 1 MiB.
constexpr uint64_t SEEK_CHECKPOINT_BYTES = uint64_t(1) << 20;

void check_ranges(const char* entry, const lz4ada_seek_index* idx, const lz4ada_frame_range* ranges,
                  int64_t nranges)
{
	if (!idx || nranges < 0 || (nranges > 0 && !ranges) || nranges >= (int64_t(1) << 31))
		misuse(entry, "idx or ranges is NULL, or a count is out of range");
	const int64_t njobs = int64_t(idx->pos.size());
	for (int64_t i = 0; i < nranges; ++i) {
		const lz4ada_frame_range& r = ranges[i];
		if (r.job < 0 || r.job >= njobs)
			misuse(entry, "range" + img(i) + " names job" + img(r.job) + " of" + img(njobs));
		if (r.off < 0 || r.len < 0 || r.off > INT64_MAX - r.len)
			misuse(entry, "range" + img(i) + " has a negative or overflowing extent");
	}
}

// The ranges with bytes to deliver, sorted by frame and offset, on the device
// with their selection records (this thread's SC_FRAME scratch).
struct Selection {
	std::vector<int64_t> of;  // sorted position -> index in the caller's array
	std::vector<RangeRec> rec;
	std::vector<RangeSel> sel;
	RangeRec* d_rec = nullptr;
	RangeSel* d_sel = nullptr;
	uint64_t tiles = 0;
};

// Clips every range, fixes its place in the output by the caller's order and
// sets the status of those that need no pass; returns the clipped total.
int64_t lay_out(const lz4ada_seek_index& x, lz4ada_frame_range* ranges, int64_t nranges, Selection& s)
{
	uint64_t total = 0;
	for (int64_t i = 0; i < nranges; ++i) {
		lz4ada_frame_range& r = ranges[i];
		r.out_off = int64_t(total);
		r.out_len = 0;
		if (!x.taken(size_t(r.job))) {
			r.status = LZ4ADA_EXACT_PATH;
			r.reason = x.reason[size_t(r.job)];
			continue;
		}
		r.status = LZ4ADA_OK;
		r.reason = LZ4ADA_DEVFRAME_OK;
		const uint64_t want = range_clip(x.size[size_t(r.job)], uint64_t(r.off), uint64_t(r.len));
		if (want > uint64_t(INT64_MAX) - total)
			raise(LZ4ADA_CONSTRAINT_ERROR, "the ranges' bytes do not fit a 64-bit count");
		r.out_len = int64_t(want);
		total += want;
		if (want)
			s.of.push_back(i);
	}
	std::sort(s.of.begin(), s.of.end(), [&](int64_t a, int64_t b) {
		const uint32_t fa = x.pos[size_t(ranges[a].job)], fb = x.pos[size_t(ranges[b].job)];
		return fa != fb ? fa < fb : ranges[a].off != ranges[b].off ? ranges[a].off < ranges[b].off : a < b;
	});
	s.rec.resize(s.of.size());
	for (size_t k = 0; k < s.of.size(); ++k) {
		const lz4ada_frame_range& r = ranges[s.of[k]];
		s.rec[k] = RangeRec{ x.pos[size_t(r.job)], 0u, uint64_t(r.off), uint64_t(r.out_len), uint64_t(r.out_off),
			             s.tiles };
		s.tiles += (uint64_t(r.out_len) + GATHER_TILE - 1) / GATHER_TILE;
	}
	return int64_t(total);
}

// k_ranges_select over s.rec and the call's first host synchronisation: the
// selection records.
void select_ranges(const lz4ada_seek_index& x, Selection& s, hipStream_t stream)
{
	const size_t n = s.rec.size(), rec_b = n * sizeof(RangeRec), sel_b = n * sizeof(RangeSel);
	device_check_or_raise();
	uint8_t* const d = scratch(SC_FRAME, rec_b + sel_b);
	if (!d)
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the range records");
	s.d_rec = reinterpret_cast<RangeRec*>(d);
	s.d_sel = reinterpret_cast<RangeSel*>(d + rec_b);
	PinBuf& h = scratch_cache().pin;  // this thread's small pinned transfers
	h.reserve(std::max(rec_b, sel_b));
	memcpy(h.p, s.rec.data(), rec_b);
	HIP_OK(hipMemcpyAsync(s.d_rec, h.p, rec_b, hipMemcpyHostToDevice, stream));
	HIP_OK(launch_ranges_select(x.view, s.d_rec, uint32_t(n), s.d_sel, nullptr, 0, 0, stream));
	HIP_OK(hipMemcpyAsync(h.p, s.d_sel, sel_b, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	s.sel.resize(n);
	memcpy(s.sel.data(), h.p, sel_b);
}

// The blocks that the sorted ranges [lo, hi) mark, from their records: how
// many once shared ones count once, their slot bytes with the heads' gaps, the
// span of blocks (among all the index's) they lie in, and the compacted blocks
// cut into runs of one kind.  The ranges of a frame come in rising first block,
// and so do their chains' starts, so their union is a sweep (ChainSweep).
struct PassPlan {
	uint32_t nsel = 0, span_n = 0;
	uint64_t slots = 0, span_lo = 0;
	bool chains = false;                          // a run is
	std::vector<std::pair<bool, uint32_t>> runs;  // (of chains, compacted blocks), in order
};
uint64_t frame_k(const lz4ada_seek_index& x, uint32_t f) { return x.kgrp.empty() ? 0 : x.kgrp[f]; }
uint32_t frame_kind(const lz4ada_seek_index& x, uint32_t f) { return x.kind.empty() ? CHAIN_KIND_NONE : x.kind[f]; }
// the gaps in front of the blocks [lo, hi) of frame f: its heads' and the dictionary's
uint64_t gap_bytes(const lz4ada_seek_index& x, uint32_t f, uint64_t lo, uint64_t hi)
{
	return CKPT_GAP * chain_heads(frame_k(x, f), lo, hi) + x.dict.gap * chain_dict_gaps(frame_kind(x, f), lo, hi);
}
// what a range's own chain takes of the budget: its blocks' slots and their gaps
uint64_t range_need(const lz4ada_seek_index& x, const Selection& s, size_t k)
{
	const RangeSel& r = s.sel[k];
	const uint32_t f = s.rec[k].frame;
	return r.slot_hi - r.slot_lo + gap_bytes(x, f, chain_start(frame_k(x, f), r.first), uint64_t(r.first) + r.count);
}
PassPlan plan_pass(const lz4ada_seek_index& x, const Selection& s, size_t lo, size_t hi)
{
	PassPlan p;
	uint64_t run_slot = 0, nsel = 0, span_hi = 0;  // the open frame's sweep, its slots' end
	uint32_t run_frame = UINT32_MAX;
	ChainSweep sweep(0);
	for (size_t k = lo; k < hi; ++k) {
		const RangeSel& r = s.sel[k];
		const uint32_t f = s.rec[k].frame;
		const uint64_t K = frame_k(x, f), c0 = chain_start(K, r.first);
		if (k == lo)
			p.span_lo = x.first[f] + c0;
		if (f != run_frame) {
			sweep = ChainSweep(K);
			run_frame = f;
		}
		const ChainSweep::Added a = sweep.add(r.first, uint64_t(r.first) + r.count - 1);
		span_hi = std::max(span_hi, x.first[f] + r.first + r.count);
		if (a.hi <= a.lo)
			continue;
		// a new run of blocks takes its own slots, one that continues the open run
		// what lies past that (slot_lo is slotp at c0, slot_hi past the last block)
		p.slots += a.lo == c0 ? r.slot_hi - r.slot_lo : r.slot_hi - run_slot;
		p.slots += gap_bytes(x, f, a.lo, a.hi);
		run_slot = r.slot_hi;
		nsel += a.hi - a.lo;
		// chains: a linked frame's blocks, and in a dictionary index every modern one's
		const bool chains = K != 0 || frame_kind(x, f) != CHAIN_KIND_NONE;
		if (!p.runs.empty() && p.runs.back().first == chains)
			p.runs.back().second += uint32_t(a.hi - a.lo);
		else
			p.runs.emplace_back(chains, uint32_t(a.hi - a.lo));
		p.chains |= chains;
	}
	// the index holds fewer than 2^31 blocks
	p.nsel = uint32_t(nsel);
	p.span_n = uint32_t(span_hi - p.span_lo);
	return p;
}

// A pass's device arrays in this thread's scratch.  SC_BATCH_META: descriptors
// | statuses | chain records | slot | mark | cnt.  SC_OUT: the slots.  SC_TAB:
// the sequence index.  The chain records and the sequence index only when the
// pass decodes chains (in_len > 0 says so to reserve()).
struct RangePass {
	lz4ada_block_desc* d_desc = nullptr;
	lz4ada_block_status* d_st = nullptr;
	FrameRec* d_chain = nullptr;
	uint64_t* d_slot = nullptr;
	uint32_t *d_mark = nullptr, *d_cnt = nullptr;
	uint8_t *d_slots = nullptr, *d_tab = nullptr;
	size_t st_b = 0, mark_b = 0, chain_b = 0;
	void reserve(const PassPlan& p, bool chains = false, uint64_t in_len = 0)
	{
		const size_t desc_b = size_t(p.nsel) * sizeof(lz4ada_block_desc), slot_b = (size_t(p.span_n) + 1) * 8;
		chain_b = chains ? size_t(chain_slots(p.nsel)) * sizeof(FrameRec) : 0;
		st_b = size_t(p.nsel) * sizeof(lz4ada_block_status);
		mark_b = size_t(p.span_n) * 4;
		uint8_t* const d = scratch(SC_BATCH_META, desc_b + st_b + chain_b + slot_b + mark_b + mark_b + 4);
		d_slots = scratch(SC_OUT, size_t(std::max<uint64_t>(p.slots, 1)));
		d_tab = chains ? scratch(SC_TAB, index_table_bytes(in_len, p.nsel)) : nullptr;
		if (!d || !d_slots || (chains && !d_tab))
			raise(LZ4ADA_DEVICE_ERROR, "no device memory for a pass over the ranges");
		d_desc = reinterpret_cast<lz4ada_block_desc*>(d);
		d_st = reinterpret_cast<lz4ada_block_status*>(d + desc_b);
		d_chain = chains ? reinterpret_cast<FrameRec*>(d + desc_b + st_b) : nullptr;
		d_slot = reinterpret_cast<uint64_t*>(d + desc_b + st_b + chain_b);
		d_mark = reinterpret_cast<uint32_t*>(d + desc_b + st_b + chain_b + slot_b);
		d_cnt = d_mark + p.span_n;
	}
	// marks, scan: what select_debug needs of a pass, and its first half
	void mark(const lz4ada_seek_index& x, const Selection& s, size_t lo, size_t hi, const PassPlan& p,
	          hipStream_t stream) const
	{
		HIP_OK(hipMemsetAsync(d_mark, 0, std::max<size_t>(mark_b, 4), stream));
		HIP_OK(launch_ranges_select(x.view, s.d_rec + lo, uint32_t(hi - lo), nullptr, d_mark, p.span_lo, p.span_n,
		                            stream));
		HIP_OK(launch_ranges_scan(d_mark, p.span_n, x.linked ? CKPT_GAP : 0, x.dict.gap, d_cnt, d_slot, stream));
	}
};

void range_failed(lz4ada_frame_range& r, int reason)
{
	r.out_len = 0;
	r.status = LZ4ADA_EXACT_PATH;
	r.reason = reason;
}

// One pass over the sorted ranges [lo, hi): their blocks decoded into slots,
// their bytes gathered into d_out, their verdicts into the caller's array.
void run_range_pass(const lz4ada_seek_index& x, Selection& s, size_t lo, size_t hi, const uint8_t* d_in,
                    lz4ada_frame_range* ranges, uint8_t* d_out, hipStream_t stream)
{
	const PassPlan p = plan_pass(x, s, lo, hi);
	RangePass m;
	const uint64_t in_len = uint64_t(x.in_len);
	m.reserve(p, p.chains, in_len);
	const uint32_t nr = uint32_t(hi - lo);
	m.mark(x, s, lo, hi, p, stream);
	if (p.chains)  // a record no block fills has flags 0: its workgroup returns at once
		HIP_OK(hipMemsetAsync(m.d_chain, 0, m.chain_b, stream));
	HIP_OK(launch_ranges_fill(x.view, m.d_mark, m.d_cnt, m.d_slot, p.span_lo, p.span_n, p.nsel, p.slots, m.d_desc,
	                          m.d_chain, stream));
	HIP_OK(hipMemsetAsync(m.d_st, 0, m.st_b, stream));
	if (p.chains) {
		HIP_OK(launch_ckpt_fill(x.view, m.d_desc, m.d_chain, p.nsel, m.d_slots, p.slots, stream));
		HIP_OK(launch_dictimg_fill(x.view, m.d_desc, m.d_chain, p.nsel, m.d_slots, p.slots, stream));
	}
	// the compacted blocks run by run, as the host's sweep cut them: independent
	// frames' with the passes' decoders (in a dictionary index: legacy frames'),
	// chains' with pass 1 and the block checksums as a linked run of a many-frame
	// pass has them; then every chain of the pass in one launch, one wave each,
	// its checkpoint as its dictionary -- or, in a dictionary index, whichever of
	// the two its record names, by the record's own history length
	uint32_t b0 = 0;
	for (const auto& run : p.runs) {
		const uint32_t n = run.second;
		if (!run.first) {
			HIP_OK(launch_decode_checked(d_in, in_len, m.d_desc + b0, n, m.d_slots, m.d_st + b0, stream));
		} else {
			HIP_OK(launch_block_checksums_beside(d_in, m.d_desc + b0, n, m.d_st + b0, stream));
			HIP_OK(launch_index(d_in, in_len, m.d_desc + b0, n, m.d_tab + size_t(b0) * 64, m.d_st + b0, stream));
		}
		b0 += n;
	}
	if (p.chains) {
		if (x.dict.used)
			HIP_OK(launch_decode_idx_chains(d_in, in_len, m.d_desc, p.nsel, m.d_tab, m.d_slots, m.d_st, m.d_chain,
			                                uint32_t(chain_slots(p.nsel)), stream));
		else
			HIP_OK(launch_decode_idx_frames_dict(d_in, in_len, m.d_desc, p.nsel, m.d_tab, m.d_slots, m.d_st,
			                                     m.d_chain, uint32_t(chain_slots(p.nsel)), uint32_t(CKPT_BYTES),
			                                     stream));
		HIP_OK(join_block_checksums(stream));
	}
	HIP_OK(launch_ranges_verdict(x.view, s.d_rec + lo, nr, s.d_sel + lo, m.d_cnt, p.span_lo, p.span_n, m.d_desc,
	                             m.d_st, p.nsel, stream));
	const uint64_t tile_lo = s.rec[lo].tile0, tile_hi = hi < s.rec.size() ? s.rec[hi].tile0 : s.tiles;
	for (uint64_t t = tile_lo; t < tile_hi;) {  // a launch takes fewer than 2^31 workgroups
		const uint32_t n = uint32_t(std::min<uint64_t>(tile_hi - t, uint64_t(1) << 30));
		HIP_OK(launch_ranges_gather(x.view, s.d_rec + lo, nr, s.d_sel + lo, t, n, m.d_mark, m.d_slot, p.span_lo,
		                            p.span_n, m.d_slots, p.slots, d_out, stream));
		t += n;
	}
	// the pass's one host synchronisation: the ranges' records
	PinBuf& h = scratch_cache().pin;
	HIP_OK(hipMemcpyAsync(h.p, s.d_sel + lo, size_t(nr) * sizeof(RangeSel), hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	++batch_stats().passes;
	const RangeSel* const got = reinterpret_cast<const RangeSel*>(h.p);
	for (size_t k = lo; k < hi; ++k) {
		if (got[k - lo].fail >= 0)
			range_failed(ranges[s.of[k]], LZ4ADA_DEVFRAME_BLOCK);
		else
			add_last_path(LZ4ADA_PATH_BATCH |
			              (frame_k(x, s.rec[k].frame) ? LZ4ADA_PATH_LINKED : LZ4ADA_PATH_INDEPENDENT));
	}
}

// LZ4ADA_SEEK_LINKED: every linked frame the sizes stage accepted, decoded once
// with the linked run of a many-frame pass (pass 1, one wave per
// frame with quirk D1's round state, the block checksums beside them), in
// passes under the byte budget, and the checkpoints of each pass saved from its
// slots.  The passes are the device engine's stages over a view of the index
// in which only those frames are taken (its walk records in SC_SEEK: nominal |
// tight), so an independent frame takes no block and no slot and every pass is
// one linked run.  A frame whose chain fails is no longer taken(), on the host
// and on the device, with LZ4ADA_DEVFRAME_BLOCK (_SIZE) as its verdict.  One
// host synchronisation per pass: the frame records.  In a dictionary index
// every frame's first block gets the dictionary's gap from the index's image,
// charged to the pass, and the frames decode against it with the LZ4
// specification's semantics (no quirk-D1 round state).
void decode_linked_frames(FramesIndex& ix, const lz4ada_seek_index& x, uint8_t* d_store, uint64_t* d_ckfirst,
                          uint64_t* d_kgrp, const uint8_t* d_in, uint64_t in_len, hipStream_t stream)
{
	const size_t n = ix.order.size(), walk_b = n * sizeof(FrameWalkRec);
	const size_t ckf_b = (n + 1) * 8, kg_b = n * 8;
	const bool dict = x.dict.used != 0;
	FramesIndex v = ix;  // the view: any other frame rides along
	bool any = false;
	for (size_t k = 0; k < n; ++k) {
		if (ix.taken(k) && ix.linked(k) && ix.walk[k].nblocks > 0)
			any = true;
		else if (ix.taken(k))
			v.walk[k].verdict = LZ4ADA_BATCH_LINKED;
	}
	v.d_walk = reinterpret_cast<FrameWalkRec*>(scratch(SC_SEEK, 2 * walk_b));
	if (!v.d_walk)
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the linked frames' records");
	v.d_tight = v.d_walk + n;
	// pinned: the index's per-frame words and the records going up, and behind
	// them room for a pass's frame records coming down and a dictionary pass's
	// kind words going up (a frame's word is written in its one pass), so that
	// nothing is written while a copy may read it
	PinBuf& h = scratch_cache().pin;
	h.reserve(ckf_b + kg_b + 2 * walk_b + n * sizeof(FrameRec) + (dict ? n * 8 : 0));
	memcpy(h.p, x.ckfirst.data(), ckf_b);
	memcpy(h.p + ckf_b, x.kgrp.data(), kg_b);
	HIP_OK(hipMemcpyAsync(d_ckfirst, h.p, ckf_b + kg_b, hipMemcpyHostToDevice, stream));  // (kgrp follows ckfirst)
	if (!any)
		return;
	FrameWalkRec* const w = reinterpret_cast<FrameWalkRec*>(h.p + ckf_b + kg_b);
	FrameRec* const rec = reinterpret_cast<FrameRec*>(h.p + ckf_b + kg_b + 2 * walk_b);
	uint64_t* const kind = reinterpret_cast<uint64_t*>(rec + n);
	for (size_t k = 0; k < n; ++k) {
		w[k] = w[n + k] = v.walk[k];
		w[n + k].slots = ix.size[k].tight;
	}
	HIP_OK(hipMemcpyAsync(v.d_walk, w, 2 * walk_b, hipMemcpyHostToDevice, stream));
	const uint64_t budget = uint64_t(batch_budget());
	bool failed = false;
	for (size_t lo = 0; lo < n;) {
		// (the gap is scratch like its slots)
		const PassCut cut = pass_cut(lo, n, budget, [&](size_t k) {
			return PassCost{ v.taken(k), ix.size[k].tight + x.dict.gap, ix.walk[k].nblocks };
		});
		const size_t hi = cut.hi;
		if (cut.blocks == 0) {  // nothing of the view's, or one frame of 2^31 blocks or more: skipped
			lo = std::max(hi, lo + 1);
			continue;
		}
		PassArrays m;
		reserve_pass(m, v, lo, hi, cut.bytes, in_len);
		fill_pass(v, lo, hi, d_in, m, stream);
		if (dict)
			lay_dict_pass(m, v, lo, hi, cut.bytes, in_len, x.dict, kind + lo, stream);
		decode_pass_blocks(m, d_in, in_len, stream);
		HIP_OK(launch_ckpt_save(d_kgrp, d_ckfirst, uint32_t(lo), m.nf, x.ckfirst[lo],
		                        uint32_t(x.ckfirst[hi] - x.ckfirst[lo]), x.ckfirst[n], m.d_desc, m.nb, m.d_rec,
		                        m.d_slots, cut.bytes, d_store, stream));
		// the pass's host synchronisation: the frame records
		HIP_OK(hipMemcpyAsync(rec, m.d_rec, m.rec_b, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		++batch_stats().passes;
		for (size_t k = lo; k < hi; ++k) {
			if (!v.taken(k))
				continue;
			const FrameRec& r = rec[k - lo];
			if (r.fail >= 0 || (r.verdict & FRAME_SIZE_BAD)) {
				ix.walk[k].verdict = r.fail >= 0 ? LZ4ADA_DEVFRAME_BLOCK : LZ4ADA_DEVFRAME_SIZE;
				failed = true;
			}
		}
		lo = hi;
	}
	if (failed) {  // the device's records follow the host's, for the scan that fixes the index
		memcpy(w, ix.walk.data(), walk_b);
		HIP_OK(hipMemcpyAsync(ix.d_walk, w, walk_b, hipMemcpyHostToDevice, stream));
	}
}

// The index's own dictionary, queued on s: the gap every pass copies, zeros and
// then the last `used` bytes of the caller's (an allocation: 256-aligned).  For
// the builds and for the index a compress call writes; dict_len > 0.
uint8_t* alloc_dict_image(lz4ada_seek_index& x, uint32_t used)
{
	const uint64_t gap = dict_gap(used);
	uint8_t* const img = x.dict_mem.alloc(size_t(gap), "the seek index's dictionary");
	x.dict = DictCtx{ img, gap, used, gap };
	x.view.dict = img;
	x.view.dict_used = used;
	return img;
}
void lay_dict_image(lz4ada_seek_index& x, const void* d_dict, int64_t dict_len, hipStream_t s)
{
	const uint32_t used = uint32_t(std::min<uint64_t>(uint64_t(dict_len), DICT_MAX));
	uint8_t* const img = alloc_dict_image(x, used);
	const size_t zeros = size_t(x.dict.gap) - used;
	HIP_OK(hipMemsetAsync(img, 0, zeros, s));
	HIP_OK(hipMemcpyAsync(img + zeros, static_cast<const uint8_t*>(d_dict) + (uint64_t(dict_len) - used), used,
	                      hipMemcpyDeviceToDevice, s));
}
// Its sibling for a concat: the image of an index that has one, as it lies.
void copy_dict_image(lz4ada_seek_index& x, const lz4ada_seek_index& from, hipStream_t s)
{
	uint8_t* const img = alloc_dict_image(x, from.dict.used);
	HIP_OK(hipMemcpyAsync(img, from.dict_mem.p, size_t(from.dict.gap), hipMemcpyDeviceToDevice, s));
}

// What the index keeps of nb blocks in n > 0 frames, allocated and named in its
// view: 32 bytes per block, 16 for its two prefixes, 24 per frame (first, and
// the prefixes' end entries), and with a dictionary (lay_dict_image comes
// first) 8 more per frame: its kind.
struct IndexArrays {
	lz4ada_block_desc* d_desc;
	uint64_t *d_first, *d_slotp, *d_kind;
};
IndexArrays alloc_index(lz4ada_seek_index& x, uint64_t nb, size_t n)
{
	const size_t desc_b = size_t(nb) * sizeof(lz4ada_block_desc), first_b = (n + 1) * 8,
	             pre_b = (size_t(nb) + n) * 8, kind_b = x.dict.used ? n * 8 : 0;
	uint8_t* const m = x.mem.alloc(desc_b + first_b + 2 * pre_b + kind_b, "the seek index");
	IndexArrays a;
	a.d_desc = reinterpret_cast<lz4ada_block_desc*>(m);
	a.d_first = reinterpret_cast<uint64_t*>(m + desc_b);
	x.d_start = reinterpret_cast<uint64_t*>(m + desc_b + first_b);
	a.d_slotp = reinterpret_cast<uint64_t*>(m + desc_b + first_b + pre_b);
	a.d_kind = x.dict.used ? reinterpret_cast<uint64_t*>(m + desc_b + first_b + 2 * pre_b) : nullptr;
	x.view.desc = a.d_desc;
	x.view.first = a.d_first;
	x.view.start = x.d_start;
	x.view.slotp = a.d_slotp;
	x.view.nframes = uint32_t(n);
	x.view.fkind = a.d_kind;
	return a;
}

// The checkpoints of a linked index over n > 0 frames: store | ckfirst | kgrp.
struct CkptArrays {
	uint8_t* d_store;
	uint64_t *d_ckfirst, *d_kgrp;
};
CkptArrays alloc_checkpoints(lz4ada_seek_index& x, uint64_t nck, size_t n)
{
	const size_t store_b = size_t(nck) * CKPT_BYTES, ckf_b = (n + 1) * 8, kg_b = n * 8;
	CkptArrays c;
	c.d_store = x.ck.alloc(store_b + ckf_b + kg_b, "the seek index's checkpoints");
	c.d_ckfirst = reinterpret_cast<uint64_t*>(c.d_store + store_b);
	c.d_kgrp = c.d_ckfirst + n + 1;
	x.view.kgrp = c.d_kgrp;
	x.view.ckfirst = c.d_ckfirst;
	x.view.store = c.d_store;
	x.view.nckpt = nck;
	return c;
}

// The one body of the builds.  linked: LZ4ADA_SEEK_LINKED, with a checkpoint
// every `every` decoded bytes.  dict: null, or a dictionary of dict_len > 0 that
// check_dict has passed.
void build_index(const char* entry, const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs, int64_t njobs,
                 bool linked, uint64_t every, const lz4ada_device_dict* dict, lz4ada_seek_index** idx, hipStream_t s)
{
	FramesIndex ix;
	index_jobs(entry, d_in, in_len, jobs, njobs, linked ? LZ4ADA_FRAMES_LINKED : 0, s, ix);
	if (dict && (dict->flags & LZ4ADA_DICT_CHECK_ID))
		check_dict_ids(ix, static_cast<const uint8_t*>(d_in), dict->dict_id, s);
	size_jobs(ix, static_cast<const uint8_t*>(d_in), uint64_t(in_len), s);
	std::unique_ptr<lz4ada_seek_index> x(new lz4ada_seek_index);
	const size_t n = ix.order.size();
	x->in_len = in_len;
	if (dict && n)
		lay_dict_image(*x, dict->d_dict, dict->dict_len, s);
	if (linked && n) {
		// the checkpoints of every linked frame the sizes stage accepted, and the
		// linked frames decoded once into them
		x->kgrp.assign(n, 0);
		x->ckfirst.assign(n + 1, 0);
		for (size_t k = 0; k < n; ++k) {
			const bool lk = ix.taken(k) && ix.linked(k) && ix.walk[k].nblocks > 0;
			if (lk)
				x->kgrp[k] = chain_group(every, chain_block_max(ix.walk[k].nblocks, ix.size[k].exact));
			x->ckfirst[k + 1] = x->ckfirst[k] + (lk ? chain_checkpoints(x->kgrp[k], ix.walk[k].nblocks) : 0);
		}
		const CkptArrays c = alloc_checkpoints(*x, x->ckfirst[n], n);
		// (which also sends the two arrays up, from pinned memory with its records)
		decode_linked_frames(ix, *x, c.d_store, c.d_ckfirst, c.d_kgrp, static_cast<const uint8_t*>(d_in),
		                     uint64_t(in_len), s);
	}
	report_sizes(ix, jobs);
	x->pos.resize(n);
	x->reason.resize(n);
	x->size.assign(n, 0);
	x->first.assign(n + 1, 0);
	for (size_t k = 0; k < n; ++k) {
		const size_t job = ix.order[k];
		x->pos[job] = uint32_t(k);
		x->reason[job] = ix.walk[k].verdict;
		x->size[job] = ix.taken(k) ? ix.size[k].exact : 0;
		x->first[k + 1] = x->first[k] + (ix.taken(k) ? ix.walk[k].nblocks : 0);
		if (linked && n && !ix.taken(k))
			x->kgrp[k] = 0;
		x->linked |= linked && ix.taken(k) && ix.linked(k) && ix.walk[k].nblocks > 0;
		x->slots += ix.taken(k) ? ix.walk[k].slots : 0;
	}
	const uint64_t nb = x->first[n];
	if (nb >= (uint64_t(1) << 31))
		raise(LZ4ADA_CONSTRAINT_ERROR, "the frames hold more blocks than a seek index takes");
	if (n == 0) {
		*idx = x.release();
		return;
	}
	const IndexArrays a = alloc_index(*x, nb, n);
	lz4ada_block_desc* const d_desc = a.d_desc;
	uint64_t *const d_first = a.d_first, *const d_slotp = a.d_slotp;
	const size_t first_b = (n + 1) * 8, kind_b = x->dict.used ? n * 8 : 0;
	if (x->dict.used) {
		// which blocks read the dictionary, by the final verdicts: every block of
		// an independent modern frame, block 0 of a linked one, none of a legacy one
		uint64_t* const d_kind = a.d_kind;
		x->kind.assign(n, uint8_t(CHAIN_KIND_NONE));
		HIP_OK(hipStreamSynchronize(s));  // nothing may still read the pinned buffer
		PinBuf& h = scratch_cache().pin;
		h.reserve(kind_b);
		uint64_t* const w = reinterpret_cast<uint64_t*>(h.p);
		for (size_t k = 0; k < n; ++k) {
			if (ix.taken(k) && ix.walk[k].format == LZ4ADA_FORMAT_MODERN && ix.walk[k].nblocks > 0)
				x->kind[k] = uint8_t(ix.linked(k) ? CHAIN_KIND_LINKED : CHAIN_KIND_INDEP);
			w[k] = x->kind[k];
		}
		HIP_OK(hipMemcpyAsync(d_kind, w, kind_b, hipMemcpyHostToDevice, s));
	}
	FrameRec* const d_rec = reinterpret_cast<FrameRec*>(scratch(SC_BATCH_META, n * sizeof(FrameRec)));
	if (!d_rec)
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the seek index");
	// the descriptors of every frame the sizes stage passed, for good: its
	// verdicts are in d_walk, so the scan counts what x->first counts
	HIP_OK(launch_frames_scan(ix.d_walk, uint32_t(n), ix.d_first, ix.d_slot, s));
	HIP_OK(launch_frames_fill(static_cast<const uint8_t*>(d_in), ix.d_span, ix.d_walk, ix.d_first, ix.d_slot,
	                          uint32_t(n), lone_blocks_disabled(), linked, ix.linked_max, d_desc, d_rec, s));
	HIP_OK(hipMemcpyAsync(d_first, ix.d_first, first_b, hipMemcpyDeviceToDevice, s));
	HIP_OK(launch_block_starts(ix.d_first, ix.d_size_first, ix.d_size, uint32_t(n), x->d_start, d_slotp, s));
	// the index is complete when the call returns, for any stream and thread
	HIP_OK(hipStreamSynchronize(s));
	*idx = x.release();
}

}  // namespace

// ---- the index a compress call writes (lz4ada_bulk_compress.cpp) ----
// The host knows every count before the first pass but one thing: whether a
// frame of at most WALK_LONE_BLOCKS blocks of 1 or 4 MiB falls to the lone-block
// rule, which asks for a written payload of WALK_LONE_MIN_IN bytes.  So the
// index is laid out pass by pass: its two blocks are allocated for every frame
// taken, each pass's kernels place its frames behind those of the passes
// before (k_compress_index_frames), and the host replays the places from the
// pass's records.  Only when the rule did turn a frame down are the arrays, by
// then dense at the front of blocks that are too large, moved into exact ones.

CompIndexSink::~CompIndexSink() { delete x; }

uint64_t seek_checkpoint_every(int64_t checkpoint_bytes)
{
	return checkpoint_bytes ? uint64_t(checkpoint_bytes) : SEEK_CHECKPOINT_BYTES;
}

void comp_index_open(CompIndexSink& k, const lz4ada_compress_job* jobs, size_t n, uint32_t block_id, bool linked,
                     int64_t checkpoint_bytes, const lz4ada_compress_dict* cdict, hipStream_t s)
{
	k.linked = linked;
	k.every = seek_checkpoint_every(checkpoint_bytes);
	k.no_lone = lone_blocks_disabled();
	const bool dict = cdict && cdict->dict_len > 0;
	k.kind = !dict ? CHAIN_KIND_NONE : linked ? CHAIN_KIND_LINKED : CHAIN_KIND_INDEP;
	const uint64_t blen = uint64_t(comp_block_len(block_id));
	uint64_t nb = 0, nck = 0;
	for (size_t i = 0; i < n; ++i) {
		const uint64_t b = uint64_t(comp_nblocks(jobs[i].in_len, int64_t(blen)));
		nb += b;
		if (linked && b)
			nck += chain_checkpoints(chain_group(k.every, chain_block_max(b, uint64_t(jobs[i].in_len))), b);
	}
	if (nb >= (uint64_t(1) << 31))
		raise(LZ4ADA_CONSTRAINT_ERROR, "the frames hold more blocks than a seek index takes");
	std::unique_ptr<lz4ada_seek_index> x(new lz4ada_seek_index);
	x->pos.resize(n);
	for (size_t i = 0; i < n; ++i)
		x->pos[i] = uint32_t(i);  // the frames lie in job order
	x->reason.assign(n, LZ4ADA_DEVFRAME_OK);
	x->size.assign(n, 0);
	x->first.assign(n + 1, 0);
	if (n) {
		if (dict) {
			lay_dict_image(*x, cdict->d_dict, cdict->dict_len, s);
			x->kind.assign(n, uint8_t(CHAIN_KIND_NONE));
		}
		const IndexArrays a = alloc_index(*x, nb, n);
		k.out = CompIndexOut{};
		k.out.desc = a.d_desc;
		k.out.first = a.d_first;
		k.out.start = x->d_start;
		k.out.slotp = a.d_slotp;
		k.out.fkind = a.d_kind;
		k.out.nblocks = nb;
		k.out.nframes = uint32_t(n);
		if (linked) {
			x->kgrp.assign(n, 0);
			x->ckfirst.assign(n + 1, 0);
			const CkptArrays c = alloc_checkpoints(*x, nck, n);
			k.out.kgrp = c.d_kgrp;
			k.out.ckfirst = c.d_ckfirst;
			k.out.store = c.d_store;
			k.out.nckpt = nck;
		}
	}
	k.x = x.release();
}

void comp_index_pass(CompIndexSink& k, const lz4ada_compress_job* jobs, size_t lo, size_t hi, uint32_t block_id,
                     const CompIndexRec* rec)
{
	lz4ada_seek_index& x = *k.x;
	const uint64_t blen = uint64_t(comp_block_len(block_id));
	for (size_t f = lo; f < hi; ++f) {
		const uint64_t n = uint64_t(jobs[f].in_len), nb = uint64_t(comp_nblocks(jobs[f].in_len, int64_t(blen)));
		const bool taken = rec[f - lo].verdict == LZ4ADA_BATCH_OK;
		x.reason[f] = rec[f - lo].verdict;
		x.size[f] = taken ? n : 0;
		x.first[f + 1] = x.first[f] + (taken ? nb : 0);
		if (k.linked) {
			x.kgrp[f] = taken && nb ? chain_group(k.every, chain_block_max(nb, n)) : 0;
			x.ckfirst[f + 1] = x.ckfirst[f] + chain_checkpoints(x.kgrp[f], nb);
			x.linked |= taken && nb > 0;
		}
		if (!x.kind.empty() && taken && nb)
			x.kind[f] = uint8_t(k.kind);
		// the places the kernels wrote by are the ones the ranged calls will read by
		if (rec[f - lo].first != x.first[f] || (k.linked && rec[f - lo].ck != x.ckfirst[f]))
			raise(LZ4ADA_CONSTRAINT_ERROR, "the seek index's places on the device are not the host's");
	}
	k.base = rec[hi - lo];
	if (k.base.first != x.first[hi] || (k.linked && k.base.ck != x.ckfirst[hi]))
		raise(LZ4ADA_CONSTRAINT_ERROR, "the seek index's places on the device are not the host's");
}

lz4ada_seek_index* comp_index_close(CompIndexSink& k, const lz4ada_compress_job* jobs, int64_t out_len,
                                    lz4ada_device_frame_job* frames, hipStream_t s)
{
	lz4ada_seek_index& x = *k.x;
	const size_t n = x.pos.size();
	x.in_len = out_len;
	x.slots = k.base.out_base;
	const uint64_t nb = n ? x.first[n] : 0, nck = k.linked && n ? x.ckfirst[n] : 0;
	if (n && (nb != k.out.nblocks || nck != k.out.nckpt)) {
		// a frame fell to the lone-block rule: the arrays into blocks of the build's
		// sizes (the passes are synchronised; this is the one more)
		lz4ada_seek_index y;
		y.dict = x.dict;  // (alloc_index reads whether there is a dictionary)
		const IndexArrays a = alloc_index(y, nb, n);
		const size_t pre_b = (size_t(nb) + n) * 8;
		HIP_OK(hipMemcpyAsync(a.d_desc, k.out.desc, size_t(nb) * sizeof(lz4ada_block_desc), hipMemcpyDeviceToDevice, s));
		HIP_OK(hipMemcpyAsync(a.d_first, k.out.first, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
		HIP_OK(hipMemcpyAsync(y.d_start, k.out.start, pre_b, hipMemcpyDeviceToDevice, s));
		HIP_OK(hipMemcpyAsync(a.d_slotp, k.out.slotp, pre_b, hipMemcpyDeviceToDevice, s));
		if (a.d_kind)
			HIP_OK(hipMemcpyAsync(a.d_kind, k.out.fkind, n * 8, hipMemcpyDeviceToDevice, s));
		if (k.linked) {
			const CkptArrays c = alloc_checkpoints(y, nck, n);
			if (nck)
				HIP_OK(hipMemcpyAsync(c.d_store, k.out.store, size_t(nck) * CKPT_BYTES, hipMemcpyDeviceToDevice, s));
			HIP_OK(hipMemcpyAsync(c.d_ckfirst, k.out.ckfirst, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
			HIP_OK(hipMemcpyAsync(c.d_kgrp, k.out.kgrp, n * 8, hipMemcpyDeviceToDevice, s));
		}
		HIP_OK(hipStreamSynchronize(s));
		std::swap(x.mem.p, y.mem.p);
		std::swap(x.mem.bytes, y.mem.bytes);
		std::swap(x.ck.p, y.ck.p);
		std::swap(x.ck.bytes, y.ck.bytes);
		const SeekView old = x.view;
		x.view = y.view;
		x.view.dict = old.dict;
		x.view.dict_used = old.dict_used;
		x.d_start = y.d_start;
	}
	for (size_t f = 0; frames && f < n; ++f) {
		lz4ada_device_frame_job& j = frames[f];
		j.in_off = jobs[f].out_off;
		j.in_len = jobs[f].out_len;
		j.out_off = j.consumed = 0;
		j.out_len = int64_t(x.size[f]);
		j.status = x.taken(f) ? LZ4ADA_OK : LZ4ADA_EXACT_PATH;
		j.reason = x.reason[f];
	}
	lz4ada_seek_index* const r = k.x;
	k.x = nullptr;
	return r;
}

// ---- several indexes laid into one (lz4ada_seek_index_concat) ----
// The rule is lz4ada_index_merge.h's: the host validates the parts and sums the
// five prefixes with it, concatenates its own vectors by them, allocates the
// result through the layouts above, sends one part table up and queues the
// kernels of lz4ada_index_merge.hip; one host synchronisation ends the call and
// brings the dictionary comparison's flag down.
namespace {

MergePart merge_shape(const lz4ada_seek_index& x)
{
	const size_t n = x.pos.size();
	return MergePart{ int64_t(n), int64_t(n ? x.first[n] : 0), int64_t(x.view.nckpt), x.in_len, int64_t(x.slots) };
}

void concat_index(const char* entry, const lz4ada_seek_index* const* parts, const int64_t* in_base, int64_t nparts,
                  int64_t in_len, lz4ada_seek_index** idx, hipStream_t s)
{
	if (!idx)
		misuse(entry, "idx is NULL");
	if (nparts > 0 && !parts)
		misuse(entry, "parts is NULL");
	std::vector<MergePart> shape(size_t(std::max<int64_t>(nparts, 0)));
	for (int64_t p = 0; p < nparts; ++p) {
		if (!parts[p])
			misuse(entry, "part" + img(p) + " is NULL");
		shape[size_t(p)] = merge_shape(*parts[p]);
	}
	int64_t at = 0;
	switch (merge_validate(shape.data(), in_base, nparts, in_len, &at)) {
	case MERGE_OK:
		break;
	case MERGE_NEGATIVE_COUNT:
		misuse(entry, "nparts or in_len is negative");
	case MERGE_NULL_ARRAY:
		misuse(entry, "in_base is NULL");
	case MERGE_NEGATIVE_BASE:
		misuse(entry, "the base of part" + img(at) + " is negative");
	case MERGE_BAD_PART:
		misuse(entry, "part" + img(at) + " is not an index");
	case MERGE_NOT_RISING:
		misuse(entry, "part" + img(at) + " begins at" + img(in_base[at]) + ", inside or in front of the part before it");
	case MERGE_PAST_END:
		misuse(entry, "part" + img(at) + " ends past in_len," + img(in_len));
	}
	// one dictionary, or none: by its used length here, by its bytes on the device
	const lz4ada_seek_index* ref = nullptr;  // the first part with frames
	uint32_t ref_at = 0;
	bool anyck = false;
	for (int64_t p = 0; p < nparts; ++p) {
		const lz4ada_seek_index& q = *parts[p];
		if (q.pos.empty())
			continue;
		if (!ref) {
			ref = &q;
			ref_at = uint32_t(p);
		}
		if (q.dict.used != ref->dict.used)
			misuse(entry, "part" + img(p) + " holds a dictionary of" + img(q.dict.used) + " bytes, part" + img(ref_at) +
			                  " one of" + img(ref->dict.used) + ": one dictionary for all parts, or none");
		anyck |= !q.kgrp.empty();
	}
	const size_t np = size_t(nparts), stride = np + 1;
	std::vector<uint64_t> pre(MERGE_PREFIXES * stride);
	if (!merge_plan(shape.data(), nparts, pre.data()))
		raise(LZ4ADA_CONSTRAINT_ERROR, "the parts hold more jobs or blocks than a seek index takes");
	const uint64_t *const pre_f = &pre[MERGE_FRAMES * stride], *const pre_b = &pre[MERGE_BLOCKS * stride],
	               *const pre_c = &pre[MERGE_CKPTS * stride];
	const size_t n = size_t(pre_f[np]);
	const uint64_t nb = pre_b[np], nck = pre_c[np];
	std::unique_ptr<lz4ada_seek_index> x(new lz4ada_seek_index);
	x->in_len = in_len;
	if (n == 0) {  // nothing to hold: no device call
		*idx = x.release();
		return;
	}
	// the host's vectors: by job, and by sorted position (a part's sorted
	// positions are kept, shifted by the frames before it)
	x->slots = pre[MERGE_SLOTS * stride + np];
	x->pos.reserve(n);
	x->reason.reserve(n);
	x->size.reserve(n);
	x->first.reserve(n + 1);
	if (anyck) {
		x->kgrp.reserve(n);
		x->ckfirst.reserve(n + 1);
	}
	if (ref->dict.used)
		x->kind.reserve(n);
	for (size_t p = 0; p < np; ++p) {
		const lz4ada_seek_index& q = *parts[p];
		const size_t m = q.pos.size();
		for (size_t j = 0; j < m; ++j)
			x->pos.push_back(uint32_t(pre_f[p] + q.pos[j]));
		x->reason.insert(x->reason.end(), q.reason.begin(), q.reason.end());
		x->size.insert(x->size.end(), q.size.begin(), q.size.end());
		for (size_t k = 0; k < m; ++k) {
			x->first.push_back(pre_b[p] + q.first[k]);
			if (anyck) {
				x->kgrp.push_back(q.kgrp.empty() ? 0 : q.kgrp[k]);
				x->ckfirst.push_back(pre_c[p] + (q.ckfirst.empty() ? 0 : q.ckfirst[k]));
			}
			if (ref->dict.used)
				x->kind.push_back(q.kind.empty() ? uint8_t(CHAIN_KIND_NONE) : q.kind[k]);
		}
		x->linked |= q.linked;
	}
	x->first.push_back(nb);
	if (anyck)
		x->ckfirst.push_back(nck);
	// the device's arrays, in the builds' layouts
	device_check_or_raise();
	if (ref->dict.used)
		copy_dict_image(*x, *ref, s);
	const IndexArrays a = alloc_index(*x, nb, n);
	MergeOut o{};
	o.desc = a.d_desc;
	o.first = a.d_first;
	o.start = x->d_start;
	o.slotp = a.d_slotp;
	o.fkind = a.d_kind;
	o.nblocks = nb;
	o.nframes = uint32_t(n);
	if (anyck) {
		const CkptArrays c = alloc_checkpoints(*x, nck, n);
		o.kgrp = c.d_kgrp;
		o.ckfirst = c.d_ckfirst;
		o.store = c.d_store;
		o.nckpt = nck;
	}
	// the part table, in one copy: the parts | the prefixes | the comparison's flag
	const size_t part_b = np * sizeof(MergePartDev), pre_b8 = pre.size() * 8, tab_b = part_b + pre_b8 + 8;
	uint8_t* const d_tab = scratch(SC_SEEK, tab_b);
	if (!d_tab)
		raise(LZ4ADA_DEVICE_ERROR, "no device memory for the part table");
	PinBuf& h = scratch_cache().pin;
	h.reserve(tab_b);
	MergePartDev* const w = reinterpret_cast<MergePartDev*>(h.p);
	for (size_t p = 0; p < np; ++p) {
		const lz4ada_seek_index& q = *parts[p];
		MergePartDev d{};
		if (!q.pos.empty()) {
			const SeekView& v = q.view;
			d = MergePartDev{ v.desc, v.first, v.start, v.slotp, v.kgrp, v.ckfirst, v.fkind, v.store, v.dict,
				          uint64_t(in_base[p]) };
		}
		w[p] = d;
	}
	memcpy(h.p + part_b, pre.data(), pre_b8);
	memset(h.p + part_b + pre_b8, 0, 8);
	HIP_OK(hipMemcpyAsync(d_tab, h.p, tab_b, hipMemcpyHostToDevice, s));
	MergeTable t{};
	t.part = reinterpret_cast<const MergePartDev*>(d_tab);
	t.pre = reinterpret_cast<const uint64_t*>(d_tab + part_b);
	t.nparts = uint32_t(np);
	uint32_t* const d_flag = reinterpret_cast<uint32_t*>(d_tab + part_b + pre_b8);
	HIP_OK(launch_index_merge(t, o, s));
	if (ref->dict.used)
		HIP_OK(launch_index_merge_dict_eq(t, ref_at, ref->dict.gap, d_flag, s));
	// the call's one host synchronisation: the index is complete, and the flag
	uint32_t* const flag = reinterpret_cast<uint32_t*>(h.p + part_b + pre_b8);
	HIP_OK(hipMemcpyAsync(flag, d_flag, 4, hipMemcpyDeviceToHost, s));
	HIP_OK(hipStreamSynchronize(s));
	if (*flag)
		misuse(entry, "the parts' dictionaries differ in their bytes: one dictionary for all parts, or none");
	*idx = x.release();
}

}  // namespace
}  // namespace lz4ada

extern "C" {

int lz4ada_seek_index_build(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs, int64_t njobs,
                            uint32_t flags, lz4ada_seek_index** idx, void* stream)
{
	if (idx)
		*idx = nullptr;
	batch_stats() = lz4ada_batch_stats{};
	return guarded(nullptr, [&] {
		const char* const entry = "lz4ada_seek_index_build";
		if (!idx)
			misuse(entry, "idx is NULL");
		if (flags != 0)
			misuse(entry, "flags must be 0");
		build_index(entry, d_in, in_len, jobs, njobs, false, 0, nullptr, idx, static_cast<hipStream_t>(stream));
	});
}

}  // extern "C"

namespace lz4ada {
namespace {

// lz4ada_seek_index_build_opt, and with a dictionary of dict_len > 0 the _dict build.
int seek_index_build_opt(const char* entry, const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs,
                         int64_t njobs, const lz4ada_seek_options* opt, const lz4ada_device_dict* dict,
                         lz4ada_seek_index** idx, void* stream)
{
	if (idx)
		*idx = nullptr;
	batch_stats() = lz4ada_batch_stats{};
	return guarded(nullptr, [&] {
		if (!idx)
			misuse(entry, "idx is NULL");
		if (opt && (opt->flags & ~LZ4ADA_SEEK_LINKED))
			misuse(entry, "unknown bits in opt->flags");
		if (opt && opt->reserved != 0)
			misuse(entry, "opt->reserved must be 0");
		if (opt && opt->checkpoint_bytes < 0)
			misuse(entry, "opt->checkpoint_bytes is negative");
		check_dict(entry, dict);
		const bool linked = opt && (opt->flags & LZ4ADA_SEEK_LINKED);
		const uint64_t every = seek_checkpoint_every(opt ? opt->checkpoint_bytes : 0);
		build_index(entry, d_in, in_len, jobs, njobs, linked, every, dict && dict->dict_len > 0 ? dict : nullptr, idx,
		            static_cast<hipStream_t>(stream));
	});
}

}  // namespace
}  // namespace lz4ada

extern "C" {

int lz4ada_seek_index_build_opt(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs, int64_t njobs,
                                const lz4ada_seek_options* opt, lz4ada_seek_index** idx, void* stream)
{
	return seek_index_build_opt("lz4ada_seek_index_build_opt", d_in, in_len, jobs, njobs, opt, nullptr, idx, stream);
}

int lz4ada_seek_index_build_dict(const void* d_in, int64_t in_len, lz4ada_device_frame_job* jobs, int64_t njobs,
                                 const lz4ada_seek_options* opt, const lz4ada_device_dict* dict,
                                 lz4ada_seek_index** idx, void* stream)
{
	const bool none = !dict || dict->dict_len == 0;
	return seek_index_build_opt(none ? "lz4ada_seek_index_build_opt" : "lz4ada_seek_index_build_dict", d_in, in_len,
	                            jobs, njobs, opt, dict, idx, stream);
}

void lz4ada_seek_index_free(lz4ada_seek_index* idx)
{
	delete idx;  // (its device memory with it)
}

int64_t lz4ada_seek_index_bytes(const lz4ada_seek_index* idx)
{
	return idx ? int64_t(idx->mem.bytes + idx->ck.bytes + idx->dict_mem.bytes) : 0;
}

int lz4ada_decode_ranges_device(const lz4ada_seek_index* idx, const void* d_in, int64_t in_len,
                                lz4ada_frame_range* ranges, int64_t nranges, void* d_out, int64_t out_cap,
                                int64_t* out_len, void* stream)
{
	if (out_len)
		*out_len = 0;
	batch_stats() = lz4ada_batch_stats{};
	set_last_path(0);
	return guarded(nullptr, [&] {
		const char* const entry = "lz4ada_decode_ranges_device";
		if (!out_len)
			misuse(entry, "out_len is NULL");
		check_ranges(entry, idx, ranges, nranges);
		if (in_len != idx->in_len)
			misuse(entry, "in_len is" + img(in_len) + ", the index was built over" + img(idx->in_len));
		if (in_len > 0 && !d_in)
			misuse(entry, "d_in is NULL");
		Selection sel;
		const int64_t total = lay_out(*idx, ranges, nranges, sel);
		*out_len = total;
		if (out_cap < total || (total > 0 && !d_out))
			raise(LZ4ADA_TOO_LITTLE_MEMORY, std::string(entry) + ": the output holds" + img(out_cap) +
			                                        " bytes, the ranges hold" + img(total));
		if (sel.of.empty())  // nothing to deliver: no launch
			return;
		hipStream_t s = static_cast<hipStream_t>(stream);
		select_ranges(*idx, sel, s);
		// the sorted ranges [lo, hi): as many as the budget takes, by the sum of
		// their own chains' slot bytes and gaps (a block two of them share counts twice)
		const uint64_t budget = uint64_t(batch_budget());
		const size_t n = sel.of.size();
		for (size_t lo = 0; lo < n;) {
			size_t hi = lo;
			uint64_t acc = 0;
			for (; hi < n; ++hi) {
				const uint64_t need = range_need(*idx, sel, hi);
				if (need > budget || (acc && acc + need > budget))
					break;
				acc += need;
			}
			if (hi == lo) {  // its blocks alone exceed the budget
				range_failed(ranges[sel.of[lo]], LZ4ADA_BATCH_OVER_BUDGET);
				++lo;
				continue;
			}
			run_range_pass(*idx, sel, lo, hi, static_cast<const uint8_t*>(d_in), ranges,
			               static_cast<uint8_t*>(d_out), s);
			lo = hi;
		}
	});
}

int lz4ada_range_blocks_host(const uint64_t* start, int64_t nblocks, const int64_t* off, const int64_t* len,
                             int64_t n, int64_t* first, int64_t* count, int64_t* want)
{
	if (!start || nblocks < 0 || n < 0 || (n > 0 && (!off || !len || !first || !count || !want)))
		return LZ4ADA_ASSERTION_ERROR;
	for (int64_t i = 0; i < n; ++i) {
		if (off[i] < 0 || len[i] < 0)
			return LZ4ADA_ASSERTION_ERROR;
		const RangeBlocks r = range_blocks(start, uint64_t(nblocks), uint64_t(off[i]), uint64_t(len[i]));
		first[i] = int64_t(r.first);
		count[i] = int64_t(r.count);
		want[i] = int64_t(range_clip(start[nblocks], uint64_t(off[i]), uint64_t(len[i])));
	}
	return LZ4ADA_OK;
}

int lz4ada_range_chains_host(int64_t nblocks, int64_t group, const int64_t* first, const int64_t* count, int64_t n,
                             uint8_t* marked, uint8_t* head, int64_t* chain_first, int64_t* chain_count,
                             int64_t* nchains)
{
	if (nchains)
		*nchains = 0;
	if (nblocks < 0 || group < 0 || n < 0 || !nchains || (n > 0 && (!first || !count)) ||
	    (nblocks > 0 && (!marked || !head || !chain_first || !chain_count)))
		return LZ4ADA_ASSERTION_ERROR;
	for (int64_t i = 0; i < n; ++i)
		if (first[i] < 0 || count[i] < 0 || first[i] > nblocks || count[i] > nblocks - first[i])
			return LZ4ADA_ASSERTION_ERROR;
	*nchains = range_chains(uint64_t(nblocks), uint64_t(group), first, count, n, marked, head, chain_first, chain_count);
	return LZ4ADA_OK;
}

int lz4ada_range_gaps_host(int64_t nblocks, int64_t group, int32_t kind, int64_t lo, int64_t hi, int64_t* heads,
                           int64_t* dict_gaps)
{
	if (!heads || !dict_gaps || nblocks < 0 || group < 0 || kind < 0 || kind > int32_t(CHAIN_KIND_INDEP) || lo < 0 ||
	    hi < lo || hi > nblocks)
		return LZ4ADA_ASSERTION_ERROR;
	*heads = int64_t(chain_heads(uint64_t(group), uint64_t(lo), uint64_t(hi)));
	*dict_gaps = int64_t(chain_dict_gaps(uint32_t(kind), uint64_t(lo), uint64_t(hi)));
	return LZ4ADA_OK;
}

// Test-only (lz4ada_hip.h): k_index over all the blocks, then k_decode_idx_chains
// over chain records in the order given (no dealing), as a ranged pass over a
// dictionary index writes them.
int lz4ada_decode_idx_chains_debug(const void* d_frame, uint64_t frame_len, const lz4ada_block_desc* descs,
                                   int64_t nblocks, const int64_t* first, const int64_t* count, const uint32_t* hist,
                                   const uint8_t* gapped, int64_t nchains, void* d_out,
                                   lz4ada_block_status* d_status, void* stream)
{
	return guarded(nullptr, [&] {
		if (nblocks < 0 || nblocks >= (int64_t(1) << 31) || nchains < 0 || nchains >= (int64_t(1) << 31) ||
		    (nblocks > 0 && (!descs || !d_status)) || (nchains > 0 && (!first || !count || !hist || !gapped)))
			raise(LZ4ADA_CONSTRAINT_ERROR, "block or chain count out of range, or a NULL array");
		for (int64_t i = 0; i < nchains; ++i)
			if (first[i] < 0 || count[i] < 0 || first[i] > nblocks || count[i] > nblocks - first[i] ||
			    (i > 0 && first[i] < first[i - 1] + count[i - 1]))
				raise(LZ4ADA_CONSTRAINT_ERROR, "chains must rise within the blocks and not overlap");
		if (nchains == 0 || nblocks == 0)
			return;
		device_check_or_raise();
		hipStream_t s = static_cast<hipStream_t>(stream);
		const auto* const in = static_cast<const uint8_t*>(d_frame);
		std::vector<lz4ada_block_desc> ds(descs, descs + nblocks);
		std::vector<FrameRec> recs(static_cast<size_t>(nchains));
		for (int64_t i = 0; i < nchains; ++i) {
			FrameRec& r = recs[size_t(i)];
			r = FrameRec{};
			r.first = uint32_t(first[i]);
			r.nblocks = uint32_t(count[i]);
			r.flags = FRAME_LINKED;
			r.hash = hist[i];
			r.content_size = CHAIN_NO_CKPT;
			r.fail = -1;
			if (gapped[i] && count[i] > 0)
				ds[size_t(first[i])].flags |= BLOCK_DICT;
		}
		DevBuf<lz4ada_block_desc> d_desc;
		d_desc.reserve(ds.size());
		DevBuf<FrameRec> d_rec;
		d_rec.reserve(recs.size());
		DevBuf<uint8_t> tab;
		tab.reserve(index_table_bytes(frame_len, uint32_t(nblocks)));
		vec_h2d(d_desc, ds, s);
		vec_h2d(d_rec, recs, s);
		HIP_OK(launch_index(in, frame_len, d_desc.p, uint32_t(nblocks), tab.p, d_status, s));
		HIP_OK(launch_decode_idx_chains(in, frame_len, d_desc.p, uint32_t(nblocks), tab.p, static_cast<uint8_t*>(d_out),
		                                d_status, d_rec.p, uint32_t(nchains), s));
		HIP_OK(hipStreamSynchronize(s));
	});
}

int lz4ada_seek_index_debug(const lz4ada_seek_index* idx, int64_t job, int32_t* reason, int64_t* nblocks,
                            uint64_t* start, int64_t start_cap, void* stream)
{
	return guarded(nullptr, [&] {
		const char* const entry = "lz4ada_seek_index_debug";
		if (!idx || !reason || !nblocks || job < 0 || job >= int64_t(idx->pos.size()))
			misuse(entry, "idx, reason or nblocks is NULL, or job is out of range");
		const size_t k = idx->pos[size_t(job)];
		const uint64_t nb = idx->first[k + 1] - idx->first[k];
		*reason = idx->reason[size_t(job)];
		*nblocks = int64_t(nb);
		if (!start)
			return;
		if (start_cap < int64_t(nb) + 1)
			raise(LZ4ADA_CONSTRAINT_ERROR, "start capacity exceeded");
		d2h(start, idx->d_start + idx->first[k] + k, (size_t(nb) + 1) * 8, static_cast<hipStream_t>(stream));
	});
}

int lz4ada_seek_index_store_debug(const lz4ada_seek_index* idx, void* store, int64_t store_cap, int64_t* nckpt,
                                  void* stream)
{
	return guarded(nullptr, [&] {
		if (!idx || !nckpt)
			misuse("lz4ada_seek_index_store_debug", "idx or nckpt is NULL");
		*nckpt = int64_t(idx->view.nckpt);
		if (!store || idx->view.nckpt == 0)
			return;
		if (store_cap < int64_t(idx->view.nckpt * CKPT_BYTES))
			raise(LZ4ADA_CONSTRAINT_ERROR, "store capacity exceeded");
		d2h(store, idx->view.store, size_t(idx->view.nckpt * CKPT_BYTES), static_cast<hipStream_t>(stream));
	});
}

int lz4ada_seek_index_concat(const lz4ada_seek_index* const* parts, const int64_t* in_base, int64_t nparts,
                             int64_t in_len, lz4ada_seek_index** idx, void* stream)
{
	if (idx)
		*idx = nullptr;
	batch_stats() = lz4ada_batch_stats{};
	return guarded(nullptr, [&] {
		if (nparts >= (int64_t(1) << 31))
			raise(LZ4ADA_CONSTRAINT_ERROR, "lz4ada_seek_index_concat: more parts than a seek index takes jobs");
		concat_index("lz4ada_seek_index_concat", parts, in_base, nparts, in_len, idx, static_cast<hipStream_t>(stream));
	});
}

int lz4ada_index_merge_plan_host(const int64_t* n, const int64_t* nb, const int64_t* nck, const int64_t* part_len,
                                 const int64_t* slots, const int64_t* in_base, int64_t nparts, int64_t in_len,
                                 uint64_t* prefix, const int64_t* kind, const int64_t* elem, int64_t nq,
                                 int64_t* part_of)
{
	if (nparts < 0 || nparts >= (int64_t(1) << 31) || nq < 0 || !prefix ||
	    (nparts > 0 && (!n || !nb || !nck || !part_len || !slots || !in_base)) ||
	    (nq > 0 && (!kind || !elem || !part_of)))
		return LZ4ADA_ASSERTION_ERROR;
	std::vector<MergePart> shape(static_cast<size_t>(nparts));
	for (int64_t p = 0; p < nparts; ++p)
		shape[size_t(p)] = MergePart{ n[p], nb[p], nck[p], part_len[p], slots[p] };
	int64_t at = 0;
	if (merge_validate(shape.data(), in_base, nparts, in_len, &at) != MERGE_OK)
		return LZ4ADA_ASSERTION_ERROR;
	if (!merge_plan(shape.data(), nparts, prefix))
		return LZ4ADA_CONSTRAINT_ERROR;
	const uint64_t stride = uint64_t(nparts) + 1;
	for (int64_t q = 0; q < nq; ++q) {
		if (kind[q] < 0 || kind[q] >= MERGE_PREFIXES || elem[q] < 0)
			return LZ4ADA_ASSERTION_ERROR;
		const uint64_t* const pre = prefix + uint64_t(kind[q]) * stride;
		if (uint64_t(elem[q]) >= pre[nparts])
			return LZ4ADA_ASSERTION_ERROR;
		part_of[q] = int64_t(merge_part_of(pre, uint64_t(nparts), uint64_t(elem[q])));
	}
	return LZ4ADA_OK;
}

int lz4ada_seek_index_arrays_debug(const lz4ada_seek_index* idx, int64_t* nframes, int64_t* nblocks, int64_t* nckpt,
                                   int32_t* has_ckpt, int32_t* has_kind, lz4ada_block_desc* desc, uint64_t* first,
                                   uint64_t* start, uint64_t* slotp, uint64_t* kgrp, uint64_t* ckfirst,
                                   uint64_t* fkind, void* stream)
{
	return guarded(nullptr, [&] {
		if (!idx || !nframes || !nblocks || !nckpt || !has_ckpt || !has_kind)
			misuse("lz4ada_seek_index_arrays_debug", "idx or a count is NULL");
		const size_t n = idx->pos.size();
		const uint64_t nb = n ? idx->first[n] : 0;
		const SeekView& v = idx->view;
		*nframes = int64_t(n);
		*nblocks = int64_t(nb);
		*nckpt = int64_t(v.nckpt);
		*has_ckpt = v.kgrp != nullptr;
		*has_kind = v.fkind != nullptr;
		if (n == 0)
			return;
		hipStream_t s = static_cast<hipStream_t>(stream);
		if (desc && nb)
			d2h(desc, v.desc, size_t(nb) * sizeof(lz4ada_block_desc), s);
		if (first)
			d2h(first, v.first, (n + 1) * 8, s);
		if (start)
			d2h(start, v.start, (size_t(nb) + n) * 8, s);
		if (slotp)
			d2h(slotp, v.slotp, (size_t(nb) + n) * 8, s);
		if (kgrp && v.kgrp)
			d2h(kgrp, v.kgrp, n * 8, s);
		if (ckfirst && v.ckfirst)
			d2h(ckfirst, v.ckfirst, (n + 1) * 8, s);
		if (fkind && v.fkind)
			d2h(fkind, v.fkind, n * 8, s);
	});
}

int lz4ada_ranges_select_debug(const lz4ada_seek_index* idx, lz4ada_frame_range* ranges, int64_t nranges,
                               int64_t* first, int64_t* count, int64_t* marked, void* stream)
{
	if (marked)
		*marked = 0;
	return guarded(nullptr, [&] {
		const char* const entry = "lz4ada_ranges_select_debug";
		if (!marked || (nranges > 0 && (!first || !count)))
			misuse(entry, "first, count or marked is NULL");
		check_ranges(entry, idx, ranges, nranges);
		Selection sel;
		lay_out(*idx, ranges, nranges, sel);
		for (int64_t i = 0; i < nranges; ++i)
			first[i] = count[i] = 0;
		if (sel.of.empty())
			return;
		hipStream_t s = static_cast<hipStream_t>(stream);
		select_ranges(*idx, sel, s);
		for (size_t k = 0; k < sel.of.size(); ++k) {
			first[sel.of[k]] = sel.sel[k].first;
			count[sel.of[k]] = sel.sel[k].count;
		}
		// the marks of all of them as one pass lays them, counted by its scan
		const PassPlan p = plan_pass(*idx, sel, 0, sel.of.size());
		RangePass m;
		m.reserve(p);
		m.mark(*idx, sel, 0, sel.of.size(), p, s);
		uint32_t n = 0;
		d2h(&n, m.d_cnt + p.span_n, 4, s);
		if (n != p.nsel)
			raise(LZ4ADA_CONSTRAINT_ERROR, "the scan counts" + img(n) + " marked blocks, the host" + img(p.nsel));
		*marked = n;
	});
}

}  // extern "C"
