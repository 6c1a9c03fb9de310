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
#include <climits>

#include "lz4ada_host_common.h"
#include "lz4ada_range_blocks.h"

using namespace lz4ada;

struct lz4ada_seek_index {
	int64_t in_len = 0;  // the input it was built over
	void* d_mem = nullptr;
	size_t bytes = 0;  // desc | first | start | slotp
	SeekView view{};
	uint64_t* d_start = nullptr;
	// by job
	std::vector<uint32_t> pos;  // its sorted position
	std::vector<int32_t> reason;
	std::vector<uint64_t> size;  // decoded bytes; 0 unless accepted
	// by sorted position, n + 1 entries: what view.first holds
	std::vector<uint64_t> first;
	bool taken(size_t job) const { return reason[job] == LZ4ADA_DEVFRAME_OK; }
};

namespace lz4ada {
namespace {

[[noreturn]] void misuse(const char* entry, const std::string& what)
{
	raise(LZ4ADA_ASSERTION_ERROR, std::string(entry) + ": " + what);
}

struct IndexDeleter {
	void operator()(lz4ada_seek_index* x) const { lz4ada_seek_index_free(x); }
};

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
// many once shared ones count once, their slot bytes, and the span of blocks
// (among all the index's) they lie in.  The ranges of a frame come in rising
// first block, so their union is a sweep.
struct PassPlan {
	uint32_t nsel = 0, span_n = 0;
	uint64_t slots = 0, span_lo = 0;
};
PassPlan plan_pass(const lz4ada_seek_index& x, const Selection& s, size_t lo, size_t hi)
{
	PassPlan p;
	uint64_t run_end = 0, run_slot = 0, nsel = 0, span_hi = 0;  // the open run: past its last block, its slots' end
	uint32_t run_frame = UINT32_MAX;
	for (size_t k = lo; k < hi; ++k) {
		const RangeSel& r = s.sel[k];
		const uint32_t f = s.rec[k].frame;
		const uint64_t g0 = x.first[f] + r.first, g1 = g0 + r.count;
		if (k == lo)
			p.span_lo = g0;
		if (f != run_frame || g0 >= run_end) {  // a new run
			nsel += r.count;
			p.slots += r.slot_hi - r.slot_lo;
			run_frame = f;
			run_end = g1;
			run_slot = r.slot_hi;
		} else if (g1 > run_end) {  // reaches past the open run
			nsel += g1 - run_end;
			p.slots += r.slot_hi - run_slot;
			run_end = g1;
			run_slot = r.slot_hi;
		}
		span_hi = std::max(span_hi, g1);
	}
	// the index holds fewer than 2^31 blocks
	p.nsel = uint32_t(nsel);
	p.span_n = uint32_t(span_hi - p.span_lo);
	return p;
}

// A pass's device arrays in this thread's scratch.  SC_BATCH_META: descriptors
// | statuses | slot | mark | cnt.  SC_OUT: the slots.
struct RangePass {
	lz4ada_block_desc* d_desc = nullptr;
	lz4ada_block_status* d_st = nullptr;
	uint64_t* d_slot = nullptr;
	uint32_t *d_mark = nullptr, *d_cnt = nullptr;
	uint8_t* d_slots = nullptr;
	size_t st_b = 0, mark_b = 0;
	void reserve(const PassPlan& p)
	{
		const size_t desc_b = size_t(p.nsel) * sizeof(lz4ada_block_desc), slot_b = (size_t(p.span_n) + 1) * 8;
		st_b = size_t(p.nsel) * sizeof(lz4ada_block_status);
		mark_b = size_t(p.span_n) * 4;
		uint8_t* const d = scratch(SC_BATCH_META, desc_b + st_b + slot_b + mark_b + mark_b + 4);
		d_slots = scratch(SC_OUT, size_t(std::max<uint64_t>(p.slots, 1)));
		if (!d || !d_slots)
			raise(LZ4ADA_DEVICE_ERROR, "no device memory for a pass over the ranges");
		d_desc = reinterpret_cast<lz4ada_block_desc*>(d);
		d_st = reinterpret_cast<lz4ada_block_status*>(d + desc_b);
		d_slot = reinterpret_cast<uint64_t*>(d + desc_b + st_b);
		d_mark = reinterpret_cast<uint32_t*>(d + desc_b + st_b + slot_b);
		d_cnt = d_mark + p.span_n;
	}
	// marks, scan: what select_debug needs of a pass, and its first half
	void mark(const lz4ada_seek_index& x, const Selection& s, size_t lo, size_t hi, const PassPlan& p,
	          hipStream_t stream) const
	{
		HIP_OK(hipMemsetAsync(d_mark, 0, std::max<size_t>(mark_b, 4), stream));
		HIP_OK(launch_ranges_select(x.view, s.d_rec + lo, uint32_t(hi - lo), nullptr, d_mark, p.span_lo, p.span_n,
		                            stream));
		HIP_OK(launch_ranges_scan(d_mark, p.span_n, d_cnt, d_slot, stream));
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
	m.reserve(p);
	const uint32_t nr = uint32_t(hi - lo);
	m.mark(x, s, lo, hi, p, stream);
	HIP_OK(launch_ranges_fill(x.view, m.d_mark, m.d_cnt, m.d_slot, p.span_lo, p.span_n, p.nsel, p.slots, m.d_desc,
	                          stream));
	HIP_OK(hipMemsetAsync(m.d_st, 0, m.st_b, stream));
	HIP_OK(launch_decode_checked(d_in, uint64_t(x.in_len), m.d_desc, p.nsel, m.d_slots, m.d_st, stream));
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
			add_last_path(LZ4ADA_PATH_BATCH | LZ4ADA_PATH_INDEPENDENT);
	}
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
		hipStream_t s = static_cast<hipStream_t>(stream);
		FramesIndex ix;
		index_jobs(entry, d_in, in_len, jobs, njobs, 0, s, ix);
		size_jobs(ix, static_cast<const uint8_t*>(d_in), uint64_t(in_len), s);
		report_sizes(ix, jobs);
		std::unique_ptr<lz4ada_seek_index, IndexDeleter> x(new lz4ada_seek_index);
		const size_t n = ix.order.size();
		x->in_len = in_len;
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
		}
		const uint64_t nb = x->first[n];
		if (nb >= (uint64_t(1) << 31))
			raise(LZ4ADA_CONSTRAINT_ERROR, "the frames hold more blocks than a seek index takes");
		if (n == 0) {
			*idx = x.release();
			return;
		}
		// what the index keeps: 32 bytes per block, 16 for its two prefixes,
		// 24 per frame (first, and the prefixes' end entries)
		const size_t desc_b = size_t(nb) * sizeof(lz4ada_block_desc), first_b = (n + 1) * 8,
		             pre_b = (size_t(nb) + n) * 8;
		x->bytes = desc_b + first_b + 2 * pre_b;
		if (hipMalloc(&x->d_mem, x->bytes) != hipSuccess) {
			(void)hipGetLastError();
			x->d_mem = nullptr;
			raise(LZ4ADA_DEVICE_ERROR, "no device memory for the seek index");
		}
		uint8_t* const m = static_cast<uint8_t*>(x->d_mem);
		lz4ada_block_desc* const d_desc = reinterpret_cast<lz4ada_block_desc*>(m);
		uint64_t* const d_first = reinterpret_cast<uint64_t*>(m + desc_b);
		x->d_start = reinterpret_cast<uint64_t*>(m + desc_b + first_b);
		uint64_t* const d_slotp = reinterpret_cast<uint64_t*>(m + desc_b + first_b + pre_b);
		x->view = SeekView{ d_desc, d_first, x->d_start, d_slotp, uint32_t(n) };
		FrameRec* const d_rec = reinterpret_cast<FrameRec*>(scratch(SC_BATCH_META, n * sizeof(FrameRec)));
		if (!d_rec)
			raise(LZ4ADA_DEVICE_ERROR, "no device memory for the seek index");
		// the descriptors of every frame the sizes stage passed, for good: its
		// verdicts are in d_walk, so the scan counts what x->first counts
		HIP_OK(launch_frames_scan(ix.d_walk, uint32_t(n), ix.d_first, ix.d_slot, s));
		HIP_OK(launch_frames_fill(static_cast<const uint8_t*>(d_in), ix.d_span, ix.d_walk, ix.d_first, ix.d_slot,
		                          uint32_t(n), lone_blocks_disabled(), false, ix.linked_max, d_desc, d_rec, s));
		HIP_OK(hipMemcpyAsync(d_first, ix.d_first, first_b, hipMemcpyDeviceToDevice, s));
		HIP_OK(launch_block_starts(ix.d_first, ix.d_size_first, ix.d_size, uint32_t(n), x->d_start, d_slotp, s));
		// the index is complete when the call returns, for any stream and thread
		HIP_OK(hipStreamSynchronize(s));
		*idx = x.release();
	});
}

void lz4ada_seek_index_free(lz4ada_seek_index* idx)
{
	if (!idx)
		return;
	if (idx->d_mem)
		(void)hipFree(idx->d_mem);
	delete idx;
}

int64_t lz4ada_seek_index_bytes(const lz4ada_seek_index* idx) { return idx ? int64_t(idx->bytes) : 0; }

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
		// their own slot bytes (a block two of them share counts twice)
		const uint64_t budget = uint64_t(batch_budget());
		const size_t n = sel.of.size();
		for (size_t lo = 0; lo < n;) {
			size_t hi = lo;
			uint64_t acc = 0;
			for (; hi < n; ++hi) {
				const uint64_t need = sel.sel[hi].slot_hi - sel.sel[hi].slot_lo;
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
