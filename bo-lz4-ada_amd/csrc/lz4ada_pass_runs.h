// lz4ada_pass_runs.h -- how the sorted frames of a device call are cut into
// passes by the byte budget (pass_cut), and how the frames of a
// pass are cut into runs of one kind (pass_runs).  Standard
// library only, so a plain C++ program can include it
// (tools/pass_cut_check.cpp, tools/pass_runs_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace lz4ada {

// A frame as the cutter sees it: its blocks in this pass (0 for one that rides
// along: skippable, empty, or not taken by the device index) and its kind.
struct PassFrame {
	uint32_t nblocks;
	bool linked;
};
// A maximal run of frames of one kind: blocks [b0, b1), frames [f0, f1).
struct PassRun {
	uint32_t b0, b1, f0, f1;
	bool linked;
	bool dict = false;  // a dictionary pass's run of modern frames; pass_runs leaves it clear
};

// The runs in order, tiling the frames and their blocks.  A run ends just
// before the first frame with blocks of the other kind; a frame without blocks,
// a leading one included, belongs to the run it falls into, so frames without
// blocks alone are one run with b0 == b1, and no frames are no run.
inline std::vector<PassRun> pass_runs(const std::vector<PassFrame>& fr)
{
	std::vector<PassRun> runs;
	for (uint32_t k = 0, b = 0, nf = uint32_t(fr.size()); k < nf;) {
		int kind = -1;
		PassRun r{ b, b, k, k, false };
		for (; r.f1 < nf; ++r.f1) {
			const int kq = fr[r.f1].nblocks ? int(fr[r.f1].linked) : -1;
			if (kind >= 0 && kq >= 0 && kq != kind)
				break;
			kind = kind >= 0 ? kind : kq;
			r.b1 += fr[r.f1].nblocks;
		}
		r.linked = kind == 1;
		runs.push_back(r);
		b = r.b1;
		k = r.f1;
	}
	return runs;
}

// What a frame asks of the pass that holds it: nothing when it is not taken
// (it rides along), else its scratch bytes (slots, a dictionary's gaps) and
// its blocks.
struct PassCost {
	bool taken;
	uint64_t bytes, blocks;
};
// The next pass over the sorted frames: [lo, hi), and its taken frames' sums.
struct PassCut {
	size_t hi;
	uint64_t bytes, blocks;
};
// As many frames from lo on as `budget` bytes take;
// frame(k) -> PassCost.  A frame that is not taken costs nothing; the first
// taken frame is accepted whatever it costs; a pass holds fewer than 2^31
// blocks, so hi == lo says that frame lo alone holds as many.
template <class F>
inline PassCut pass_cut(size_t lo, size_t n, uint64_t budget, F&& frame)
{
	PassCut c{ lo, 0, 0 };
	for (; c.hi < n; ++c.hi) {
		const PassCost f = frame(c.hi);
		if (!f.taken)
			continue;
		if ((c.bytes && c.bytes + f.bytes > budget) || c.blocks + f.blocks >= (uint64_t(1) << 31))
			break;
		c.bytes += f.bytes;
		c.blocks += f.blocks;
	}
	return c;
}

}  // namespace lz4ada
