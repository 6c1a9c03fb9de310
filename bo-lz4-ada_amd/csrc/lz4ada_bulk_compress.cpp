// lz4ada_bulk_compress.cpp -- records that lie in device memory compressed
// into LZ4 frames in device memory, the write side of
// lz4ada_bulk_frames_device.cpp.  The host knows every length, so it builds the
// block and job arrays itself (one H2D per pass); the device compresses every
// block into a scratch slot (k_compress_blocks, one wave per block), scans the
// sizes, emits size words and payloads into the caller's d_out, hashes them
// with the existing XXH32 kernels and writes headers, end marks and checksums
// from the job array (lz4ada_compress.hip).  The host sees the per-job results
// (one D2H per pass); no payload byte crosses, except that a content checksum
// over more than lz4ada_batch_hash_max() bytes is hashed by the host chain
// (content_xxh32_d2h with no host destination).  The jobs are cut into passes
// only when their slots exceed LZ4ADA_BATCH_BYTES.  A linked call (DESIGN.md
// §21) differs in the kernel of a pass that holds a continuation block
// (k_compress_blocks_linked, which reads a block's history from d_in, never
// from a slot) and in the header's B.Indep bit.  The indexed call (DESIGN.md
// §22) hands every pass a sink: the pass then also queues the kernels that
// write the frames' seek index (lz4ada_compress_index.hip) in front of its
// synchronisation, which brings their records down with its own.
#include "lz4ada_compress.h"
#include "lz4ada_compress_index.h"
#include "lz4ada_host_common.h"

using namespace lz4ada;

namespace lz4ada {
namespace {

// A call's dictionary: its used tail (dl bytes, 0: none, the plain kernel) and
// the seeded table on the device; the header's flags and id.
struct PassDict {
	const uint8_t* d_tail = nullptr;
	uint32_t dl = 0;
	const uint32_t* d_seed = nullptr;
	uint32_t dflags = 0, dict_id = 0;
};

inline size_t up16(size_t v) { return (v + 15) & ~size_t(15); }

// One pass over the jobs [lo, hi), nb blocks and slot_b slot bytes in all:
// their frames go to d_out from *base on, which then moves past them.  sink:
// null, or the seek index the call writes (in_len: d_in's, for its checkpoints).
void compress_pass(const char* ENTRY, const uint8_t* d_in, lz4ada_compress_job* jobs, size_t lo, size_t hi,
                   uint64_t nb64, uint64_t slot_b, uint32_t id, uint32_t flags, const PassDict& dict, bool linked,
                   uint8_t* d_out, uint64_t* base, uint64_t hash_max, hipStream_t stream,
                   CompIndexSink* sink = nullptr, uint64_t in_len = 0)
{
	const bool bck = (flags & LZ4ADA_COMP_BLOCK_CHECKSUM) != 0, cck = (flags & LZ4ADA_COMP_CONTENT_CHECKSUM) != 0;
	const uint32_t nb = uint32_t(nb64), nj = uint32_t(hi - lo);
	const int64_t blen = comp_block_len(id);
	// what the host fills, in one piece: blocks | jobs | content hash records
	const size_t blk_b = up16(size_t(nb) * sizeof(CompBlock)), job_b = up16(size_t(nj) * sizeof(CompJob)),
	             frec_b = cck ? up16(size_t(nj) * sizeof(FrameRec)) : 0, up_b = blk_b + job_b + frec_b;
	// what the device fills
	const size_t rec_b = up16(size_t(nj) * sizeof(CompJobRec)), csize_b = up16(size_t(nb) * 4),
	             loc_b = up16(size_t(nb) * 8), part_b = up16((size_t(plan_tiles(nb)) + 1) * 8),
	             desc_b = up16(size_t(nb) * sizeof(lz4ada_block_desc)),
	             st_b = bck ? up16(size_t(nb) * sizeof(lz4ada_block_status)) : 0,
	             xrec_b = sink ? up16((size_t(nj) + 1) * sizeof(CompIndexRec)) : 0;
	uint8_t* const m = scratch(SC_BATCH_META, up_b + rec_b + csize_b + loc_b + part_b + desc_b + st_b + xrec_b);
	uint8_t* const d_slots = scratch(SC_OUT, size_t(slot_b));
	if (!m || !d_slots)
		raise(LZ4ADA_DEVICE_ERROR, std::string(ENTRY) + ": no device memory for the pass");
	uint8_t* q = m;
	auto take = [&](size_t b) {
		uint8_t* const p = q;
		q += b;
		return p;
	};
	CompBlock* const d_blk = reinterpret_cast<CompBlock*>(take(blk_b));
	CompJob* const d_jobs = reinterpret_cast<CompJob*>(take(job_b));
	FrameRec* const d_frec = cck ? reinterpret_cast<FrameRec*>(take(frec_b)) : nullptr;
	CompJobRec* const d_rec = reinterpret_cast<CompJobRec*>(take(rec_b));
	uint32_t* const d_csize = reinterpret_cast<uint32_t*>(take(csize_b));
	uint64_t* const d_loc = reinterpret_cast<uint64_t*>(take(loc_b));
	uint64_t* const d_part = reinterpret_cast<uint64_t*>(take(part_b));
	lz4ada_block_desc* const d_desc = reinterpret_cast<lz4ada_block_desc*>(take(desc_b));
	lz4ada_block_status* const d_st = bck ? reinterpret_cast<lz4ada_block_status*>(take(st_b)) : nullptr;
	CompIndexRec* const d_xrec = sink ? reinterpret_cast<CompIndexRec*>(take(xrec_b)) : nullptr;

	PinBuf& h = scratch_cache().pin;  // this thread's small pinned transfers
	h.reserve(up_b + rec_b + xrec_b);
	CompBlock* const blk = reinterpret_cast<CompBlock*>(h.p);
	CompJob* const cj = reinterpret_cast<CompJob*>(h.p + blk_b);
	FrameRec* const frec = reinterpret_cast<FrameRec*>(h.p + blk_b + job_b);
	const CompJobRec* const rec = reinterpret_cast<const CompJobRec*>(h.p + up_b);
	uint64_t fixed = 0, slot = 0;
	uint32_t b = 0;
	bool cont = false;  // a linked pass with a block that has its record in front of it
	for (size_t k = lo; k < hi; ++k) {
		const lz4ada_compress_job& j = jobs[k];
		const uint32_t n = uint32_t(comp_nblocks(j.in_len, blen));
		cont = cont || (linked && n > 1);
		cj[k - lo] = CompJob{ uint64_t(j.in_off), uint64_t(j.in_len), fixed, b, n };
		fixed += uint64_t(comp_header_len(flags, dict.dflags) + comp_trailer_len(flags));
		for (uint32_t i = 0; i < n; ++i, ++b) {
			const int64_t at = int64_t(i) * blen, len = std::min(blen, j.in_len - at);
			blk[b] = CompBlock{ uint64_t(j.in_off + at), slot, uint32_t(len), uint32_t(k - lo) };
			slot += round256(uint64_t(len));
		}
		if (cck) {
			FrameRec r{};
			r.flags = FRAME_HAS_CKSUM;
			r.out_off = uint64_t(j.in_off);
			r.out_len = uint64_t(j.in_len);
			r.fail = -1;
			frec[k - lo] = r;
		}
	}
	HIP_OK(hipMemcpyAsync(m, h.p, up_b, hipMemcpyHostToDevice, stream));
	HIP_OK(hipMemsetAsync(d_rec, 0, rec_b, stream));
	if (cck)  // over the records where they lie; the longer ones are the host chain's
		HIP_OK(launch_xxh32_spans(d_in, d_frec, nj, hash_max, stream));
	HIP_OK(launch_compress_blocks(d_in, d_blk, d_jobs, nb, cont, dict.d_tail, dict.dl, dict.d_seed, d_slots, d_csize,
	                              stream));
	HIP_OK(launch_compress_scan(d_blk, d_csize, nb, flags, d_loc, d_part, stream));
	HIP_OK(launch_compress_emit(d_in, d_slots, d_blk, d_csize, d_loc, d_part, d_jobs, nb, flags, dict.dflags, *base,
	                            d_out, d_desc, d_rec, stream));
	if (bck) {  // over the payloads as written
		HIP_OK(launch_block_checksums(d_out, d_desc, nb, d_st, stream));
		HIP_OK(launch_compress_block_cksums(d_desc, d_st, nb, d_out, stream));
	}
	if (sink) {  // the frames' seek index from what the pass knows, and its records down with the pass's
		HIP_OK(launch_compress_index(d_in, in_len, d_blk, d_jobs, nb, nj, d_csize, d_desc, d_st, id, flags, linked, cont,
		                             sink->every, sink->no_lone, sink->kind, uint32_t(lo), sink->base, sink->out, d_xrec,
		                             stream));
		HIP_OK(hipMemcpyAsync(h.p + up_b + rec_b, d_xrec, xrec_b, hipMemcpyDeviceToHost, stream));
	}
	HIP_OK(launch_compress_frames(d_jobs, nj, d_loc, d_part, nb, id, flags, dict.dflags, dict.dict_id, linked, *base,
	                              d_frec, d_out, d_rec, stream));
	// the pass's host synchronisation: places, lengths and counts, no payload byte
	HIP_OK(hipMemcpyAsync(h.p + up_b, d_rec, rec_b, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	std::vector<uint32_t> late;  // the host chain's checksums, kept until they are copied
	late.reserve(nj);
	for (size_t k = lo; k < hi; ++k) {
		lz4ada_compress_job& j = jobs[k];
		const CompJobRec& r = rec[k - lo];
		j.out_off = int64_t(r.out_off);
		j.out_len = int64_t(r.out_len);
		j.stored_blocks = int32_t(r.stored);
		j.status = LZ4ADA_OK;
		*base = r.out_off + r.out_len;
	}
	if (sink)
		comp_index_pass(*sink, jobs, lo, hi, id, reinterpret_cast<const CompIndexRec*>(h.p + up_b + rec_b));
	for (size_t k = lo; cck && k < hi; ++k) {
		const lz4ada_compress_job& j = jobs[k];
		if (uint64_t(j.in_len) <= hash_max)
			continue;
		lz4ada_xxh32_state hs;
		lz4ada_xxh32_reset(&hs, 0);
		content_xxh32_d2h(hs, d_in + j.in_off, j.in_len, nullptr, stream);
		late.push_back(host_xxh32_final(hs));
		HIP_OK(hipMemcpyAsync(d_out + j.out_off + j.out_len - 4, &late.back(), 4, hipMemcpyHostToDevice, stream));
	}
	if (!late.empty())
		HIP_OK(hipStreamSynchronize(stream));
}

// What the indexed call adds to an entry: its options, the frames' report (may
// be null) and where the index goes.
struct IndexAsk {
	const lz4ada_compress_index_options* xopt;
	lz4ada_device_frame_job* frames;
	lz4ada_seek_index** idx;
};

// Every entry: cdict null is the plain call; linked: frames of linked blocks
// (DESIGN.md §21), with the same slots and the same passes; ask: null, or the
// indexed call's, which adds its own misuse to the checks, the
// index's memory before the first pass and a sink to every pass.
int compress_frames(const char* ENTRY, const void* d_in, int64_t in_len, lz4ada_compress_job* jobs, int64_t njobs,
                    const lz4ada_compress_options* opt, const lz4ada_compress_dict* cdict, bool linked, void* d_out,
                    int64_t out_cap, int64_t* out_len, void* stream, const IndexAsk* ask = nullptr)
{
	if (out_len)
		*out_len = 0;
	if (ask && ask->idx)
		*ask->idx = nullptr;
	return guarded(nullptr, [&] {
		auto misuse = [&](const std::string& what) { raise(LZ4ADA_ASSERTION_ERROR, std::string(ENTRY) + ": " + what); };
		const uint32_t id = opt ? opt->block_id : 0, flags = opt ? opt->flags : 0;
		if (ask && (!ask->idx || (ask->xopt && ((ask->xopt->flags & ~LZ4ADA_COMP_INDEX_LINKED) ||
		                                        ask->xopt->reserved != 0 || ask->xopt->checkpoint_bytes < 0))))
			misuse("idx is NULL, unknown bits in xopt->flags, xopt->reserved is not 0, or checkpoint_bytes is negative");
		if (!out_len || njobs < 0 || (njobs > 0 && !jobs) || in_len < 0 || (in_len > 0 && !d_in) || out_cap < 0 ||
		    njobs >= (int64_t(1) << 31))
			misuse("jobs, d_in or out_len is NULL, or a count is out of range");
		if (!comp_options_ok(id, flags))
			misuse("block_id is not 0 or 4..7, or unknown bits in flags");
		if (cdict && (cdict->dict_len < 0 || (cdict->dict_len > 0 && !cdict->d_dict) ||
		              (cdict->flags & ~COMP_DICT_FLAGS_ALL)))
			misuse("dict_len is negative, d_dict is NULL, or unknown bits in dict->flags");
		for (int64_t i = 0; i < njobs; ++i)
			if (jobs[i].in_off < 0 || jobs[i].in_len < 0 || jobs[i].in_off > in_len ||
			    jobs[i].in_len > in_len - jobs[i].in_off)
				misuse("job" + img(i) + " lies outside the input");
		const int64_t bound = lz4ada_compress_frames_bound_dict(jobs, njobs, opt, cdict);
		if (bound < 0)
			misuse("the jobs' bound is out of range");
		if (bound > 0 && !d_out && out_cap >= bound)
			misuse("d_out is NULL");
		for (int64_t i = 0; i < njobs; ++i) {
			jobs[i].out_off = jobs[i].out_len = 0;
			jobs[i].stored_blocks = 0;
			jobs[i].status = out_cap < bound ? LZ4ADA_TOO_LITTLE_MEMORY : LZ4ADA_OK;
		}
		if (out_cap < bound) {
			*out_len = bound;
			raise(LZ4ADA_TOO_LITTLE_MEMORY, std::string(ENTRY) + ": the output holds" + img(out_cap) +
			                                        " bytes, the frames may take" + img(bound));
		}
		CompIndexSink sink;
		hipStream_t s = static_cast<hipStream_t>(stream);
		if (njobs == 0) {
			if (ask) {  // an empty index, no device call
				comp_index_open(sink, jobs, 0, id, linked, 0, cdict, s);
				*ask->idx = comp_index_close(sink, jobs, 0, ask->frames, s);
			}
			return;
		}
		device_check_or_raise();
		PassDict dict;
		if (cdict) {
			dict.dflags = cdict->flags;
			dict.dict_id = cdict->dict_id;
			const int64_t dl = std::min(cdict->dict_len, COMP_DICT_MAX);
			if (dl >= 4) {  // below 4 bytes nothing is seeded: the plain kernel's bytes
				uint32_t* const d_seed = reinterpret_cast<uint32_t*>(scratch(SC_DICT, COMP_TABLE * sizeof(uint32_t)));
				if (!d_seed)
					raise(LZ4ADA_DEVICE_ERROR, std::string(ENTRY) + ": no device memory for the dictionary's table");
				dict.d_tail = static_cast<const uint8_t*>(cdict->d_dict) + (cdict->dict_len - dl);
				dict.dl = uint32_t(dl);
				dict.d_seed = d_seed;
				HIP_OK(launch_compress_dict_table(dict.d_tail, dict.dl, d_seed, s));  // once per call
			}
		}
		if (ask)
			comp_index_open(sink, jobs, size_t(njobs), id, linked, ask->xopt ? ask->xopt->checkpoint_bytes : 0, cdict, s);
		const uint64_t budget = uint64_t(batch_budget()), hash_max = uint64_t(batch_hash_max());
		const int64_t blen = comp_block_len(id);
		uint64_t base = 0;
		const size_t n = size_t(njobs);
		size_t lo = 0;
		while (lo < n) {
			// the jobs [lo, hi): as many as the budget's slots take, one at least
			size_t hi = lo;
			uint64_t acc = 0, nb = 0;
			for (; hi < n; ++hi) {
				const uint64_t jb = uint64_t(comp_nblocks(jobs[hi].in_len, blen));
				const uint64_t cost = jb ? (jb - 1) * round256(uint64_t(blen)) +
				                                   round256(uint64_t(jobs[hi].in_len - int64_t(jb - 1) * blen))
				                         : 0;
				if (hi > lo && (acc + cost > budget || nb + jb >= (uint64_t(1) << 31)))
					break;
				acc += cost;
				nb += jb;
			}
			if (nb >= (uint64_t(1) << 31))
				raise(LZ4ADA_CONSTRAINT_ERROR, std::string(ENTRY) + ": a record holds more blocks than a pass takes");
			compress_pass(ENTRY, static_cast<const uint8_t*>(d_in), jobs, lo, hi, nb, acc, id, flags, dict, linked,
			              static_cast<uint8_t*>(d_out), &base, hash_max, s, ask ? &sink : nullptr, uint64_t(in_len));
			lo = hi;
		}
		*out_len = int64_t(base);
		if (ask)
			*ask->idx = comp_index_close(sink, jobs, *out_len, ask->frames, s);
	});
}

}  // namespace
}  // namespace lz4ada

extern "C" int lz4ada_compress_frames_device(const void* d_in, int64_t in_len, lz4ada_compress_job* jobs,
                                             int64_t njobs, const lz4ada_compress_options* opt, void* d_out,
                                             int64_t out_cap, int64_t* out_len, void* stream)
{
	return compress_frames("lz4ada_compress_frames_device", d_in, in_len, jobs, njobs, opt, nullptr, false, d_out,
	                       out_cap, out_len, stream);
}

extern "C" int lz4ada_compress_frames_device_dict(const void* d_in, int64_t in_len, lz4ada_compress_job* jobs,
                                                  int64_t njobs, const lz4ada_compress_options* opt,
                                                  const lz4ada_compress_dict* dict, void* d_out, int64_t out_cap,
                                                  int64_t* out_len, void* stream)
{
	return compress_frames("lz4ada_compress_frames_device_dict", d_in, in_len, jobs, njobs, opt, dict, false, d_out,
	                       out_cap, out_len, stream);
}

extern "C" int lz4ada_compress_frames_device_linked(const void* d_in, int64_t in_len, lz4ada_compress_job* jobs,
                                                    int64_t njobs, const lz4ada_compress_options* opt,
                                                    const lz4ada_compress_dict* dict, void* d_out, int64_t out_cap,
                                                    int64_t* out_len, void* stream)
{
	return compress_frames("lz4ada_compress_frames_device_linked", d_in, in_len, jobs, njobs, opt, dict, true, d_out,
	                       out_cap, out_len, stream);
}

extern "C" int lz4ada_compress_frames_device_indexed(const void* d_in, int64_t in_len, lz4ada_compress_job* jobs,
                                                     int64_t njobs, const lz4ada_compress_options* opt,
                                                     const lz4ada_compress_dict* dict,
                                                     const lz4ada_compress_index_options* xopt, void* d_out,
                                                     int64_t out_cap, int64_t* out_len,
                                                     lz4ada_device_frame_job* frames, lz4ada_seek_index** idx,
                                                     void* stream)
{
	const IndexAsk ask{ xopt, frames, idx };
	const bool linked = xopt && (xopt->flags & LZ4ADA_COMP_INDEX_LINKED);
	return compress_frames("lz4ada_compress_frames_device_indexed", d_in, in_len, jobs, njobs, opt, dict, linked, d_out,
	                       out_cap, out_len, stream, &ask);
}

// Test-only (lz4ada_hip.h): the rule of lz4ada_compress_index.h over one frame
// that a _host compress statement wrote, its written sizes read from the frame's
// size words at the places the rule itself gives them.
extern "C" int lz4ada_compress_index_host(const uint8_t* frame, int64_t frame_len, int64_t record_len,
                                          const lz4ada_compress_options* opt, uint32_t dict_flags, uint32_t linked,
                                          int64_t checkpoint_bytes, uint64_t frame_off, uint64_t out_base,
                                          lz4ada_block_desc* descs, uint32_t* sizes, int64_t cap, int64_t* nblocks,
                                          int32_t* verdict, int64_t* group, int64_t* checkpoints)
{
	const uint32_t id = opt ? opt->block_id : 0, flags = opt ? opt->flags : 0;
	if (!frame || frame_len < 0 || record_len < 0 || !comp_options_ok(id, flags) || (dict_flags & ~COMP_DICT_FLAGS_ALL) ||
	    checkpoint_bytes < 0 || cap < 0 || (cap > 0 && (!descs || !sizes)) || !nblocks || !verdict || !group ||
	    !checkpoints)
		return LZ4ADA_ASSERTION_ERROR;
	const uint64_t blen = uint64_t(comp_block_len(id)), n = uint64_t(record_len);
	const int64_t nb = comp_nblocks(record_len, int64_t(blen));
	std::vector<uint32_t> csize(size_t(nb) + 1), cksum(size_t(nb) + 1);
	std::vector<uint64_t> at(size_t(nb) + 1);
	int64_t pos = comp_header_len(flags, dict_flags);
	for (int64_t i = 0; i < nb; ++i) {
		if (pos + 4 > frame_len)
			return LZ4ADA_ASSERTION_ERROR;
		const uint32_t word = walk_load32(frame + pos), len = comp_index_block_len(n, blen, uint64_t(i));
		const uint32_t in = word & 0x7fffffffu;
		if ((word >> 31) ? in != len : (in == 0 || in >= len))  // stored as it is, or shorter than it went in
			return LZ4ADA_ASSERTION_ERROR;
		csize[size_t(i)] = (word >> 31) ? 0u : in;
		at[size_t(i)] = uint64_t(pos) + 4;
		pos += 4 + int64_t(in);
		if (pos + (comp_block_extra(flags) - 4) > frame_len)
			return LZ4ADA_ASSERTION_ERROR;
		if (flags & LZ4ADA_COMP_BLOCK_CHECKSUM) {
			cksum[size_t(i)] = walk_load32(frame + pos);
			pos += 4;
		}
	}
	if (pos + comp_trailer_len(flags) != frame_len)
		return LZ4ADA_ASSERTION_ERROR;
	const CompIndexFrame f =
	        comp_index_frame(n, blen, csize.data(), linked != 0, seek_checkpoint_every(checkpoint_bytes), lone_blocks_disabled());
	*nblocks = int64_t(f.nblocks);
	*verdict = f.verdict;
	*group = int64_t(f.group);
	*checkpoints = int64_t(f.nckpt);
	for (int64_t i = 0; i < nb && i < cap; ++i) {
		descs[i] = comp_index_desc(n, blen, flags, uint64_t(i), csize[size_t(i)], frame_off + at[size_t(i)],
		                           cksum[size_t(i)], out_base);
		sizes[i] = comp_index_block_len(n, blen, uint64_t(i));
	}
	return LZ4ADA_OK;
}
