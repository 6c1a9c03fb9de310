// lz4ada_compress_dict.hip -- gfx950 kernels of the compressor with a shared
// dictionary (lz4ada_bulk_compress.cpp):
//  * k_compress_dict_table -- once per call: the 4,096-entry table of the
//    dictionary's used tail D, every position whose four bytes lie inside D
//    inserted by atomicMax on position + 1 (positions only grow, so the
//    maximum is the latest, as in the serial statement's ascending loop);
//  * k_compress_blocks_dict -- the one body (lz4ada_compress_block.inc) with D
//    at [-dl, 0) in front of every block, CompHist::Dict: the LDS table starts
//    as a copy of the seeded one.
// No kernel waits for another workgroup; every loop is bounded by the block
// length or the dictionary's.
#include "lz4ada_compress_block.h"

namespace lz4ada {

namespace {

constexpr uint32_t DICT_WG = 256;  // threads per workgroup of the table kernel

}  // namespace

// seed[h]: index + 1 of the last i in [0, dl - 3) with comp_hash(D[i .. i + 4)) == h
// (virtual position i - dl, so virtual position + dl + 1); the caller zeroed seed.
__global__ __launch_bounds__(DICT_WG) void k_compress_dict_table(const uint8_t* __restrict__ d_tail, uint32_t dl,
                                                                 uint32_t* __restrict__ seed)
{
	const uint32_t i = blockIdx.x * DICT_WG + threadIdx.x;
	if (i + 4 > dl)
		return;
	atomicMax(&seed[comp_hash(ld32u_cached(gptr(d_tail) + i))], i + 1);
}

__global__ __launch_bounds__(64) void k_compress_blocks_dict(const uint8_t* __restrict__ d_in,
                                                              const CompBlock* __restrict__ blk, uint32_t nblocks,
                                                              const uint8_t* __restrict__ d_tail, uint32_t dict_len,
                                                              const uint32_t* __restrict__ seed,
                                                              uint8_t* __restrict__ slots,
                                                              uint32_t* __restrict__ csize)
{
	constexpr CompHist H = CompHist::Dict;
	constexpr const CompJob* jobs = nullptr;  // what only a linked record reads: named, never used
#include "lz4ada_compress_block.inc"
}

hipError_t launch_compress_dict_table(const uint8_t* d_tail, uint32_t dl, uint32_t* d_seed, hipStream_t stream)
{
	hipError_t e = hipMemsetAsync(d_seed, 0, COMP_TABLE * sizeof(uint32_t), stream);
	if (e != hipSuccess || dl < 4)
		return e;
	hipLaunchKernelGGL(k_compress_dict_table, dim3((dl - 3 + DICT_WG - 1) / DICT_WG), dim3(DICT_WG), 0, stream, d_tail,
	                   dl, d_seed);
	return hipGetLastError();
}

}  // namespace lz4ada
