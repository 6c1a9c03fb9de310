// lz4ada_compress_linked.hip -- the gfx950 kernel of the compressor for frames
// of linked blocks (lz4ada_bulk_compress.cpp):
//  * k_compress_blocks_linked -- the one body (lz4ada_compress_block.inc) with
//    the history given per block, CompHist::Linked: nothing or the dictionary's
//    used tail in front of a record's block 0, the 65,536 bytes of its own
//    record in d_in in front of every later block, which seeds its own table.
#include "lz4ada_compress_block.h"

namespace lz4ada {

__global__ __launch_bounds__(64) void k_compress_blocks_linked(const uint8_t* __restrict__ d_in,
                                                                const CompBlock* __restrict__ blk,
                                                                const CompJob* __restrict__ jobs, uint32_t nblocks,
                                                                const uint8_t* __restrict__ d_tail, uint32_t dict_len,
                                                                const uint32_t* __restrict__ seed,
                                                                uint8_t* __restrict__ slots,
                                                                uint32_t* __restrict__ csize)
{
	constexpr CompHist H = CompHist::Linked;
#include "lz4ada_compress_block.inc"
}

}  // namespace lz4ada
