// lz4ada_frames_pass.cpp -- what the two many-frame engines and the seek
// index's linked build do on the device, stated once (DESIGN.md §10-§12, §20;
// declared in lz4ada_host_common.h): a pass's arrays, the decode launches of
// its runs, the device half of the pass up to its one synchronisation (the
// build's up to k_frames_plan), a frame's verdict, the tuning values and counters.
#include "lz4ada_host_common.h"

namespace lz4ada {
namespace {

// G: a frame's content checksum is hashed by k_xxh32_spans when the frame decodes
// to at most this many bytes, else by the host chain while its bytes are copied
// out.  Measured (profiles/frames_batch_xxh.txt): with 64 spans
// side by side the kernel beats one host core from 4 KiB to 16 MiB, the largest.
constexpr int64_t BATCH_HASH_MAX = int64_t(16) << 20;
// A linked frame shares a pass (LZ4ADA_FRAMES_LINKED) when its slots sum to
// at most this: one wave walks the whole frame, so past some size the frame
// is faster on its own, every block at once (lz4ada_bulk_linked.cpp).
// Measured (profiles/frames_linked_ab.txt): a pass of 2 frames
// of 32 x 64 KiB is still 1.17x faster than the two on their own, one of 2 of
// 64 x 64 KiB is 1.46x slower; sizes in between were not measured.
constexpr int64_t BATCH_LINKED_MAX = int64_t(2) << 20;

thread_local lz4ada_batch_stats g_stats{};

// One run's decode launches.  Independent: launch_decode_checked over its
// blocks.  Linked: the block checksums beside pass 1 over its blocks, one wave
// per frame (k_decode_idx_frames), then the join.  A dictionary run (DESIGN.md
// §15) is the linked arm with the dictionary decoders: one wave per frame
// (linked) or per block (independent: no launch_decode_checked, whose fallback
// decoders know no history, so a block pass 1 declines keeps its code).
void decode_pass_run(const PassArrays& a, const uint8_t* d_in, uint64_t in_len, const PassRun& run,
                     hipStream_t stream)
{
	const uint32_t n = run.b1 - run.b0;
	if (n == 0)
		return;
	if (!run.linked && !run.dict) {
		HIP_OK(launch_decode_checked(d_in, in_len, a.d_desc + run.b0, n, a.d_slots, a.d_st + run.b0, stream));
		return;
	}
	HIP_OK(launch_block_checksums_beside(d_in, a.d_desc + run.b0, n, a.d_st + run.b0, stream));
	HIP_OK(launch_index(d_in, in_len, a.d_desc + run.b0, n, a.d_tab + size_t(run.b0) * 64, a.d_st + run.b0,
	                    stream));
	if (run.dict && run.linked)
		HIP_OK(launch_decode_idx_frames_dict(d_in, in_len, a.d_desc, a.nb, a.d_tab, a.d_slots, a.d_st,
		                                     a.d_rec + run.f0, run.f1 - run.f0, a.dict_used, stream));
	else if (run.dict)
		HIP_OK(launch_decode_idx_dict(d_in, in_len, a.d_desc + run.b0, n, a.d_tab + size_t(run.b0) * 64, a.d_slots,
		                              a.d_st + run.b0, a.dict_used, stream));
	else
		HIP_OK(launch_decode_idx_frames(d_in, in_len, a.d_desc, a.nb, a.d_tab, a.d_slots, a.d_st,
		                                a.d_rec + run.f0, run.f1 - run.f0, stream));
	HIP_OK(join_block_checksums(stream));
}

}  // namespace

int64_t batch_budget() { return env_bytes("LZ4ADA_BATCH_BYTES", int64_t(4) << 30); }
int64_t batch_hash_max() { return env_bytes("LZ4ADA_BATCH_HASH_MAX", BATCH_HASH_MAX); }
int64_t batch_linked_max() { return env_bytes("LZ4ADA_BATCH_LINKED_MAX", BATCH_LINKED_MAX); }
uint32_t batch_env_flags()
{
	const char* e = getenv("LZ4ADA_BATCH_LINKED");
	return e && *e && *e != '0' ? LZ4ADA_FRAMES_LINKED : 0u;
}
lz4ada_batch_stats& batch_stats() { return g_stats; }

const char* PassArrays::reserve(const std::vector<PassFrame>& frames, uint64_t slots, uint64_t in_len)
{
	runs = pass_runs(frames);
	nf = uint32_t(frames.size());
	nb = runs.empty() ? 0u : runs.back().b1;
	desc_b = size_t(nb) * sizeof(lz4ada_block_desc);
	rec_b = size_t(nf) * sizeof(FrameRec);
	st_b = size_t(nb) * sizeof(lz4ada_block_status);
	const size_t words = 2 * size_t(nb) + plan_tiles(nb) + 2;  // dst_off: nb + 1, loc: nb, part: tiles + 1
	uint8_t* const d = scratch(SC_BATCH_META, desc_b + rec_b + st_b + words * 8);
	if (!d)
		return "block arrays";
	d_desc = reinterpret_cast<lz4ada_block_desc*>(d);
	d_rec = reinterpret_cast<FrameRec*>(d + desc_b);
	d_st = reinterpret_cast<lz4ada_block_status*>(d + desc_b + rec_b);
	d_off = reinterpret_cast<uint64_t*>(d + desc_b + rec_b + st_b);
	d_loc = d_off + nb + 1;
	d_part = d_loc + nb;
	if (!(d_slots = scratch(SC_OUT, size_t(std::max<uint64_t>(slots, 1)))))
		return "slots";
	const bool any_linked = std::any_of(runs.begin(), runs.end(), [](const PassRun& r) { return r.linked; });
	d_tab = any_linked ? scratch(SC_TAB, index_table_bytes(in_len, nb)) : nullptr;
	return any_linked && !d_tab ? "sequence index" : nullptr;
}

void decode_pass_blocks(const PassArrays& a, const uint8_t* d_in, uint64_t in_len, hipStream_t stream)
{
	if (a.nb)
		HIP_OK(hipMemsetAsync(a.d_st, 0, a.st_b, stream));
	for (const PassRun& run : a.runs)
		decode_pass_run(a, d_in, in_len, run, stream);
	HIP_OK(launch_frames_plan(a.d_desc, a.d_st, a.nb, a.d_rec, a.nf, a.d_off, a.d_loc, a.d_part, stream));
}

void decode_pass(const PassArrays& a, const uint8_t* d_in, uint64_t in_len, uint8_t* dst, uint64_t hash_max,
                 FrameRec* h_rec, hipStream_t stream)
{
	decode_pass_blocks(a, d_in, in_len, stream);
	HIP_OK(launch_compact(a.d_slots, a.d_desc, a.d_off, a.d_st, a.nb, dst, stream));
	HIP_OK(launch_xxh32_spans(dst, a.d_rec, a.nf, hash_max, stream));
	// the pass's one host synchronisation: the per-frame records
	HIP_OK(hipMemcpyAsync(h_rec, a.d_rec, a.rec_b, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	++g_stats.passes;
}

FrameVerdict frame_verdict(const FrameRec& r, uint32_t declared, bool* gpu_hashed)
{
	*gpu_hashed = (r.verdict & FRAME_GPU_HASHED) != 0;
	if (r.fail >= 0)
		return FV_BLOCK;
	if (r.verdict & FRAME_SIZE_BAD)
		return FV_SIZE;
	if (*gpu_hashed)
		return r.hash == declared ? FV_GOOD : FV_CHECKSUM;
	return (r.flags & FRAME_HAS_CKSUM) ? FV_HOST_HASH : FV_GOOD;
}

}  // namespace lz4ada
