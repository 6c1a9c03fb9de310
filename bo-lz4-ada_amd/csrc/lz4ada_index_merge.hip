// lz4ada_index_merge.hip -- gfx950 kernels by which lz4ada_seek_index_concat
// lays the device arrays of several seek indexes into one.
// One part table (MergeTable, lz4ada_index_merge.h: every part's array
// pointers and base, and the five prefixes of merge_plan) is on the device;
// every lane finds the part of its merged element with merge_part_of and
// copies the element, rebased by that part's constants:
//  * k_index_merge_blocks -- a lane per merged block: its descriptor, in_off
//    grown by the part's base and out_off by the nominal slots before;
//  * k_index_merge_words -- a lane per merged word of start / slotp (a part's
//    nb + n words are one run, and land at blocks before + frames before);
//  * k_index_merge_frames -- a lane per merged frame: first grown by the
//    blocks before, ckfirst by the checkpoints before, kgrp and fkind copied
//    (K = 0 and a flat ckfirst for a part without checkpoint arrays), and one
//    lane more for the end entries of first and ckfirst;
//  * k_index_merge_store -- CKPT_SAVE_SPLIT workgroups per merged checkpoint,
//    16 bytes per lane: source and destination are 65,536-byte entries of
//    stores that begin an allocation, so whole u32x4 loads and stores
//    (k_ckpt_from_records' stores);
//  * k_index_merge_dict_eq -- every other part's dictionary image against one
//    part's, 16 bytes per lane, into one flag word.
// No frame byte is read and nothing is decoded.  Every bound is a count the
// result was allocated by (MergeOut), and a part is read only below the counts
// its own prefixes give, so a table that lies may give wrong words but writes
// nothing outside the result.  Plain vector stores only (the flag: the same
// value from every writer), every loop bounded by a count of the table or a
// checkpoint's bytes, no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lz4ada_internal.h"
#include "lz4ada_dev.h"
#include "lz4ada_range_chains.h"
#include "lz4ada_index_merge.h"

namespace lz4ada {

namespace {

constexpr uint32_t MERGE_WG = 256;
constexpr uint32_t MERGE_DICT_PARTS = 1024;  // the comparison's grid in y: parts beyond it by stride
static_assert(CKPT_BYTES % (CKPT_SAVE_SPLIT * MERGE_WG * 16) == 0, "k_index_merge_store's pieces tile a checkpoint");

__device__ __forceinline__ const uint64_t* merge_pre(const MergeTable& t, int k)
{
	return t.pre + uint64_t(k) * (uint64_t(t.nparts) + 1);
}

}  // namespace

__global__ __launch_bounds__(MERGE_WG) void k_index_merge_blocks(MergeTable t, MergeOut o)
{
	const uint64_t b = uint64_t(blockIdx.x) * MERGE_WG + threadIdx.x;
	const uint64_t* const pre = merge_pre(t, MERGE_BLOCKS);
	if (b >= o.nblocks || b >= pre[t.nparts])
		return;
	const uint64_t p = merge_part_of(pre, t.nparts, b);
	const MergePartDev P = t.part[p];
	if (!P.desc)
		return;
	lz4ada_block_desc d = P.desc[b - pre[p]];
	d.in_off += P.in_base;
	d.out_off += merge_pre(t, MERGE_SLOTS)[p];
	o.desc[b] = d;
}

__global__ __launch_bounds__(MERGE_WG) void k_index_merge_words(MergeTable t, MergeOut o)
{
	const uint64_t w = uint64_t(blockIdx.x) * MERGE_WG + threadIdx.x;
	const uint64_t* const pre = merge_pre(t, MERGE_WORDS);
	if (w >= o.nblocks + o.nframes || w >= pre[t.nparts])
		return;
	const uint64_t p = merge_part_of(pre, t.nparts, w);
	const MergePartDev P = t.part[p];
	if (!P.start || !P.slotp)
		return;
	o.start[w] = P.start[w - pre[p]];
	o.slotp[w] = P.slotp[w - pre[p]];
}

__global__ __launch_bounds__(MERGE_WG) void k_index_merge_frames(MergeTable t, MergeOut o)
{
	const uint64_t f = uint64_t(blockIdx.x) * MERGE_WG + threadIdx.x;
	const uint64_t* const pre = merge_pre(t, MERGE_FRAMES);
	const uint64_t* const pre_b = merge_pre(t, MERGE_BLOCKS);
	const uint64_t* const pre_c = merge_pre(t, MERGE_CKPTS);
	if (f > o.nframes)
		return;
	if (f == o.nframes) {  // the end entries
		o.first[f] = pre_b[t.nparts];
		if (o.ckfirst)
			o.ckfirst[f] = pre_c[t.nparts];
		return;
	}
	if (f >= pre[t.nparts])
		return;
	const uint64_t p = merge_part_of(pre, t.nparts, f), k = f - pre[p];
	const MergePartDev P = t.part[p];
	if (!P.first)
		return;
	o.first[f] = P.first[k] + pre_b[p];
	if (o.kgrp) {
		const bool has = P.kgrp && P.ckfirst;
		o.kgrp[f] = has ? P.kgrp[k] : 0;
		o.ckfirst[f] = pre_c[p] + (has ? P.ckfirst[k] : 0);
	}
	if (o.fkind)
		o.fkind[f] = P.fkind ? P.fkind[k] : uint64_t(CHAIN_KIND_NONE);
}

__global__ __launch_bounds__(MERGE_WG) void k_index_merge_store(MergeTable t, MergeOut o, uint64_t c_lo)
{
	const uint64_t c = c_lo + blockIdx.x / CKPT_SAVE_SPLIT;
	const uint32_t piece = blockIdx.x % CKPT_SAVE_SPLIT;
	const uint64_t* const pre = merge_pre(t, MERGE_CKPTS);
	if (c >= o.nckpt || c >= pre[t.nparts] || !o.store)
		return;
	const uint64_t p = merge_part_of(pre, t.nparts, c);
	const MergePartDev P = t.part[p];
	if (!P.store)
		return;
	constexpr uint32_t PIECE = uint32_t(CKPT_BYTES / CKPT_SAVE_SPLIT);
	cg8* const src = gptr(P.store) + (c - pre[p]) * CKPT_BYTES + piece * PIECE;
	g8* const dst = gptr(o.store) + c * CKPT_BYTES + piece * PIECE;
	for (uint32_t x = 16 * threadIdx.x; x < PIECE; x += 16 * MERGE_WG)
		*reinterpret_cast<GLOBAL u32x4*>(dst + x) = *reinterpret_cast<const GLOBAL u32x4*>(src + x);
}

__global__ __launch_bounds__(MERGE_WG) void k_index_merge_dict_eq(MergeTable t, uint32_t ref, uint64_t gap,
                                                                  uint32_t* __restrict__ flag)
{
	const uint64_t x = 16 * (uint64_t(blockIdx.x) * MERGE_WG + threadIdx.x);
	if (x + 16 > gap || ref >= t.nparts)
		return;
	const uint8_t* const want = t.part[ref].dict;
	if (!want)
		return;
	const u32x4 a = *reinterpret_cast<const GLOBAL u32x4*>(gptr(want) + x);
	bool differ = false;
	for (uint32_t p = blockIdx.y; p < t.nparts; p += gridDim.y) {
		const uint8_t* const img = t.part[p].dict;
		if (!img || img == want)
			continue;
		const u32x4 b = *reinterpret_cast<const GLOBAL u32x4*>(gptr(img) + x);
		differ |= a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w;
	}
	if (differ)
		*flag = 1;
}

hipError_t launch_index_merge(const MergeTable& t, const MergeOut& o, hipStream_t stream)
{
	if (o.nframes == 0 || t.nparts == 0)
		return hipSuccess;
	const auto groups = [](uint64_t n) { return dim3(uint32_t((n + MERGE_WG - 1) / MERGE_WG)); };
	if (o.nblocks)
		hipLaunchKernelGGL(k_index_merge_blocks, groups(o.nblocks), dim3(MERGE_WG), 0, stream, t, o);
	hipLaunchKernelGGL(k_index_merge_words, groups(o.nblocks + o.nframes), dim3(MERGE_WG), 0, stream, t, o);
	hipLaunchKernelGGL(k_index_merge_frames, groups(uint64_t(o.nframes) + 1), dim3(MERGE_WG), 0, stream, t, o);
	// a launch takes fewer than 2^31 workgroups
	for (uint64_t c = 0; o.store && c < o.nckpt;) {
		const uint64_t n = std::min<uint64_t>(o.nckpt - c, (uint64_t(1) << 30) / CKPT_SAVE_SPLIT);
		hipLaunchKernelGGL(k_index_merge_store, dim3(uint32_t(n * CKPT_SAVE_SPLIT)), dim3(MERGE_WG), 0, stream, t, o, c);
		c += n;
	}
	return hipGetLastError();
}

hipError_t launch_index_merge_dict_eq(const MergeTable& t, uint32_t ref, uint64_t gap, uint32_t* d_flag,
                                      hipStream_t stream)
{
	if (t.nparts < 2 || gap < 16)
		return hipSuccess;
	const uint32_t gx = uint32_t((gap / 16 + MERGE_WG - 1) / MERGE_WG);
	hipLaunchKernelGGL(k_index_merge_dict_eq, dim3(gx, std::min(t.nparts, MERGE_DICT_PARTS)), dim3(MERGE_WG), 0, stream,
	                   t, ref, gap, d_flag);
	return hipGetLastError();
}

}  // namespace lz4ada
