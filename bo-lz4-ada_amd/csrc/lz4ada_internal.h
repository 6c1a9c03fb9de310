// lz4ada_internal.h -- what the host units (lz4ada_host_common.h/.cpp,
// lz4ada_facade.cpp, lz4ada_bulk.cpp, lz4ada_bulk_linked.cpp,
// lz4ada_bulk_frames.cpp, lz4ada_bulk_frames_device.cpp, lz4ada_bulk_ranges.cpp,
// lz4ada_multi.cpp)
// share with the gfx950 kernel files (lz4ada_*.hip): the device status codes
// and the launchers' declarations.  Not part of the public C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "lz4ada_hip.h"
#include "lz4ada_round_state.h"

namespace lz4ada {

// XXH32 primes (lz4ada.ads:323-328).
constexpr uint32_t P1 = 2654435761u;
constexpr uint32_t P2 = 2246822519u;
constexpr uint32_t P3 = 3266489917u;
constexpr uint32_t P4 = 668265263u;
constexpr uint32_t P5 = 374761393u;

constexpr int64_t BLOCK_SIZE_BYTES = 4;  // lz4ada.ads:351

// Linked frames (lz4ada_linked.hip): every block slot is preceded by this
// many readable history bytes (the largest LZ4 offset).
constexpr int32_t LINK_HIST = 65535;
// (HISTORY_SIZE, quirk D1's constants and the linked path's aux bits:
// lz4ada_round_state.h)

// Device status codes written by the decode kernels (per block).
enum DevStatus : int32_t {
	DS_OK = 0,
	DS_OFFSET0 = 1,        // lz4ada.adb:769-772
	DS_ML_AFTER_LIT = 2,   // lz4ada.adb:752-762 (aux = Match_Length nibble)
	DS_LIT_OVERRUN = 3,    // D3
	DS_TRUNCATED = 4,      // D4
	DS_OUT_OVERFLOW = 5,   // D5 (bulk: block_max slot; serial: Buffer)
	DS_PRE_BLOCK_REF = 6,  // back-reference before the block start (bulk)
	DS_BACKREF = 7,        // lz4ada.adb:867-874 (detail = H_Offset)
	DS_CONTENT_SIZE = 8,   // lz4ada.adb:830-835
	DS_INTERNAL = 9,       // decoder invariant broken (never expected)
	DS_RETRY = 10,         // a fast decoder declined the block: k_decode_pc (or the exact path) redoes it
	DS_SPARSE = 11,        // pass 1 declined a literal-heavy block: k_decode_sparse takes it
	                       // (k_decode_pc, retry_only, takes it like DS_RETRY)
	DS_SKIP = 12,          // not part of this launch: every decoder leaves the block alone
};

// State of the serial reference-exact block kernel (emulates one
// Decode_Full_Block_With_Trailer step on a device mirror of Buffer).
struct SerialState {
	int64_t output_pos;          // Ctx.Output_Pos
	int64_t output_pos_history;  // Ctx.Output_Pos_History
	int64_t first, last;         // Output_First / Output_Last
	uint64_t size_remaining;     // Ctx.M.Size_Remaining
	int32_t has_content_size;
	int32_t code;   // DevStatus
	int32_t aux;
	int32_t pad;
	int64_t detail;
};

// ---- launchers (lz4ada_kernels.hip) ----
// All launch on `stream` and never synchronise.

// Bulk independent-block decoders (LZ4ADA_DECODE_* in lz4ada_hip.h).
enum DecVariant : int { DEC_PC = 0, DEC_IDX = 3, DEC_IDX_ALONE = 4,
                        DEC_IDX_LINKED = 5, DEC_IDX_SPARSE = 6,
                        // the fused index decoder alone with one / two waves per block
                        DEC_IDX1_ALONE = 7, DEC_IDX2_ALONE = 8,
                        // the pipelined two-wave decoder (k_decode_pp2) alone
                        DEC_PP2_ALONE = 9,
                        // k_index then k_decode_idx's pass 2, two launches (per-pass counters)
                        DEC_IDX_SPLIT = 10 };
// What launch_decode_idx_tab launches (lz4ada_idx.hip).
enum class IdxMode {
	PASS2,          // k_decode_idx: pass 2 of independent blocks over a table from launch_index
	LINKED_SERIAL,  // k_decode_idx as one workgroup: a linked frame's blocks in order (contiguous slots)
	LINKED_LK,      // k_decode_idx_lk: pass 2 of every block at once, LINK_HIST readable history
	                // bytes before each slot, quirk D1 emulated
	LINKED_ZL,      // k_decode_idx_zl: the same layout, literals as zeros
	FUSED_ONE,      // k_decode_idx: both passes of independent blocks, one wave per block (d_tab
	                // is written: no launch_index needed)
	FUSED_PAIR,     // k_decode_pp2: both passes, two waves per block pipelining batches
};
// What a caller of launch_decode_idx asks for.
enum class IdxRun {
	AUTO,           // both passes in one launch, the kernel idx_fused_mode picks
	FUSED_ONE,      // ... k_decode_idx whatever the launch size
	FUSED_PAIR,     // ... k_decode_pp2 whatever the launch size
	SPLIT,          // k_index, then pass 2: two launches (diagnostic: per-pass counters)
	LINKED_SERIAL,  // k_index, then the serial linked workgroup
};
IdxMode idx_fused_mode(uint32_t nblocks);  // FUSED_ONE or FUSED_PAIR, by launch size (lz4ada_idx.hip)
const char* idx_fused_kernel_name(uint32_t nblocks);  // the kernel idx_fused_mode picks

hipError_t launch_decode_variant(const uint8_t* d_frame, uint64_t frame_len,
                                 const lz4ada_block_desc* d_desc, uint32_t nblocks,
                                 uint8_t* d_out, lz4ada_block_status* d_status, int variant,
                                 hipStream_t stream);

// The default decoder: the index-driven decoder, then the literal-heavy and
// two-wave decoders for the blocks it declines; LZ4ADA_DECODER=pc selects
// k_decode_pc alone.
hipError_t launch_decode_blocks(const uint8_t* d_frame, uint64_t frame_len,
                                const lz4ada_block_desc* d_desc, uint32_t nblocks,
                                uint8_t* d_out, lz4ada_block_status* d_status,
                                hipStream_t stream);

// Index-driven decoder alone (lz4ada_idx.hip): k_index + k_decode_idx;
// declined blocks keep status DS_RETRY and are not decoded.
// IdxRun::LINKED_SERIAL: the blocks of one linked frame (slots contiguous),
// decoded in order with the earlier output as history; from the first
// declined or short block on, every block is left DS_RETRY.
hipError_t launch_decode_idx(const uint8_t* d_frame, uint64_t frame_len,
                             const lz4ada_block_desc* d_desc, uint32_t nblocks, uint8_t* d_out,
                             lz4ada_block_status* d_status, hipStream_t stream,
                             IdxRun run = IdxRun::AUTO);

// Two-wave decoder alone (k_decode_pc).  retry_only: only blocks whose
// status is DS_RETRY.  hist: output bytes readable right before every slot
// (0 independent; LINK_HIST in the linked-frame layout).
hipError_t launch_decode_pc(const uint8_t* d_frame, uint64_t frame_len,
                            const lz4ada_block_desc* d_desc, uint32_t nblocks, uint8_t* d_out,
                            lz4ada_block_status* d_status, int retry_only, int32_t hist,
                            hipStream_t stream);

// Pass 1 of the index-driven decoder alone: the sequence-index table of
// every block (index_table_bytes() of device memory at d_tab); declined
// blocks get status DS_RETRY.  waves: 1 (the product's k_index) or 2 (the
// pass 1 k_decode_pp2 runs, for the table test); anything else is
// hipErrorInvalidValue.
size_t index_table_bytes(uint64_t frame_len, uint32_t nblocks);
hipError_t launch_index(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                        uint32_t nblocks, uint8_t* d_tab, lz4ada_block_status* d_status,
                        hipStream_t stream, int waves = 1);
// One launch of the index decoder over the table at d_tab: pass 2 over a
// table from launch_index, or (the FUSED modes) both passes.
hipError_t launch_decode_idx_tab(const uint8_t* d_frame, uint64_t frame_len,
                                 const lz4ada_block_desc* d_desc, uint32_t nblocks,
                                 const uint8_t* d_tab, uint8_t* d_out,
                                 lz4ada_block_status* d_status, IdxMode mode, hipStream_t stream);

// Literal-heavy blocks pass 1 declined (status DS_SPARSE; lz4ada_sparse.hip):
// decoded straight to HBM, one wave per block; anything unusual leaves the
// block DS_RETRY for k_decode_pc.
hipError_t launch_decode_sparse(const uint8_t* d_frame, uint64_t frame_len,
                                const lz4ada_block_desc* d_desc, uint32_t nblocks, uint8_t* d_out,
                                lz4ada_block_status* d_status, hipStream_t stream);

// Per-block XXH32 of the compressed payloads (block checksums).
hipError_t launch_block_checksums(const uint8_t* d_frame,
                                  const lz4ada_block_desc* d_desc, uint32_t nblocks,
                                  lz4ada_block_status* d_status, hipStream_t stream);

// Block checksums and the default decoder together: the checksum kernel
// (latency-bound, no LDS) runs on a side stream beside pass 1 of the
// index-driven decoder, fork and join by events; `stream` sees both done.
hipError_t launch_decode_checked(const uint8_t* d_frame, uint64_t frame_len,
                                 const lz4ada_block_desc* d_desc, uint32_t nblocks,
                                 uint8_t* d_out, lz4ada_block_status* d_status,
                                 hipStream_t stream);

// Per-block XXH32 of decoded output slots (golden checks).
hipError_t launch_output_checksums(const uint8_t* d_out,
                                   const lz4ada_block_desc* d_desc, uint32_t nblocks,
                                   const lz4ada_block_status* d_status,
                                   uint32_t* d_hash, hipStream_t stream);

// Streaming XXH32 update of a device-resident state over device data.
// Also refreshes state->hash with the Final() value.
hipError_t launch_xxh32_update(lz4ada_xxh32_state* d_state, const uint8_t* d_data,
                               uint64_t len, hipStream_t stream);

// Reference-exact serial decode of one block into the Buffer mirror.
hipError_t launch_serial_block(uint8_t* d_buf, int64_t buflen, const uint8_t* d_blk,
                               int64_t raw_len, int64_t data_len, int compressed,
                               SerialState* d_state, hipStream_t stream);

// Linked frames, every block at once (lz4ada_linked.hip).  Slots of the
// three decode buffers are preceded by 64 KiB history regions.
hipError_t launch_link_fill(uint8_t* x, uint8_t* y, uint8_t* h, const lz4ada_block_desc* d_desc,
                            uint32_t nblocks, hipStream_t stream);
// The block checksums on this thread's side stream, forked from stream
// (they write only the statuses' cksum fields, so kernels on stream may
// fill the other fields meanwhile); join_block_checksums makes stream wait
// for them.
hipError_t launch_block_checksums_beside(const uint8_t* d_frame, const lz4ada_block_desc* d_desc,
                                        uint32_t nblocks, lz4ada_block_status* d_status, hipStream_t stream);
hipError_t join_block_checksums(hipStream_t stream);
// k_link_fill on the same side stream (after everything already on
// stream), so it runs beside k_index; join_link_fill makes stream wait for
// it (before the decodes that read the history regions).
hipError_t launch_link_fill_beside(uint8_t* x, uint8_t* y, uint8_t* h, const lz4ada_block_desc* d_desc,
                                   uint32_t nblocks, hipStream_t stream);
hipError_t join_link_fill(hipStream_t stream);
// The same side stream for any launch: side_fork gives it, ordered after
// everything already on stream; side_join makes stream wait for everything
// on it so far (the checksums included).
hipError_t side_fork(hipStream_t stream, hipStream_t* side);
hipError_t side_join(hipStream_t stream);
// Words from the planes: x (history k -> k & 255) and z (literals 0,
// history k -> k >> 8) for every block; d_three (nullable) gives a block's
// mode -- 1: y (~x) as well, 2: x, y and h (k >> 8) instead.
// Each pointer is stepped twice from its source's planes (d_tail: the
// tail_valid bytes before the batch, for sources there).  d_P gets a word
// for every quad with a byte still open and d_M a byte per position (0
// open, 1 final with no word, 2 final with its word) -- or, `full` (batches
// where many words stay open, whose rounds then read a source's word
// alone), every word and no d_M.
hipError_t launch_link_init(const uint8_t* x, const uint8_t* z, const uint8_t* y, const uint8_t* h,
                            const uint8_t* d_three, const lz4ada_block_desc* d_desc,
                            const lz4ada_block_status* d_st, const int64_t* d_A, uint32_t nblocks,
                            int64_t block_max, const uint8_t* d_tail, int64_t tail_valid, uint32_t* d_P,
                            uint8_t* d_F, uint8_t* d_M, uint8_t* d_act, bool full, hipStream_t stream);
// One pointer-jumping round; d_act_in (nullptr: every span) / d_act_out:
// a byte per span of positions, 1 while the span holds an unresolved word.
int64_t link_spans(int64_t n);
hipError_t launch_link_jump(uint32_t* d_P, const uint8_t* d_M, int64_t n, const uint8_t* d_tail,
                            int64_t tail_valid, uint8_t* d_F, const uint8_t* d_act_in, uint8_t* d_act_out,
                            uint32_t* d_ctr, bool full, hipStream_t stream);
hipError_t launch_link_tail(const uint8_t* d_F, int64_t n, const uint8_t* d_tail_old,
                            uint8_t* d_tail_new, hipStream_t stream);

// Gather variable-length slots into a contiguous buffer (short blocks).
// One block decoded by the whole GPU (lz4ada_lone.hip): d_st gets DS_OK and
// out_len, or DS_RETRY (the exact path then decides).  d_scratch holds
// lone_scratch_bytes(n, cap) bytes.  History (a linked frame's block): the
// n0 + n1 <= 65535 bytes before the block, h0 then h1 (device memory; the
// reference's Buffer keeps them in two places), readable by its matches;
// d1: 0; 1 -- a match reaching >= D1_OFF back before the block start
// declines it (quirk D1); or the round's Output_Pos_History (>= 65536) --
// the block follows a round that ended there, and quirk D1's overshoot
// bytes are emulated (lz4ada_lone.hip).  Without history such a match
// declines it.  At most LONE_MAX_IN compressed bytes: the chain step keeps
// every window's entry in one workgroup's registers (16 MiB of windows at
// every window size); larger blocks return hipErrorInvalidValue, and the
// facade sends them to the exact path instead (lone_plan).
constexpr int64_t LONE_MAX_IN = int64_t(16) << 20;
int64_t lone_scratch_bytes(int64_t n, int64_t cap);
hipError_t launch_decode_lone(const uint8_t* d_blk, int64_t n, uint8_t* d_out, int64_t cap,
                              lz4ada_block_status* d_st, void* d_scratch, int64_t scratch_bytes,
                              hipStream_t stream, const uint8_t* d_h0 = nullptr, int32_t n0 = 0,
                              const uint8_t* d_h1 = nullptr, int32_t n1 = 0, int d1 = 0);
// The same in two halves: the parse (steps 1-3: nothing written to d_out,
// the status set to DS_RETRY on a decline) and the emit (step 4: the bytes
// to d_out when the status is still OK).  A caller may check something on
// the host between them, e.g. the block checksum before d_out is touched.
// Zero-copy form (the streaming facade): d_blk may be pinned host memory
// that step 1 reads once and copies to d_copy (ncopy >= n bytes: the
// block's trailer too), which step 3 then reads; d_st may be pinned host
// memory; h_out, when not null, is pinned host memory that step 4 writes
// the bytes to as well -- no DMA copy on the block's critical path.
hipError_t launch_decode_lone_parse(const uint8_t* d_blk, int64_t n, int64_t cap,
                                    lz4ada_block_status* d_st, void* d_scratch, int64_t scratch_bytes,
                                    hipStream_t stream, const uint8_t* d_h0, int32_t n0,
                                    const uint8_t* d_h1, int32_t n1, int d1, uint8_t* d_copy = nullptr,
                                    int64_t ncopy = 0, bool fused = false);
// fused: a small block's chain step runs inside its windows launch, which
// needs the scratch's header zeroed once (lone_scratch_init) before the
// scratch's first fused use; every fused use leaves it zeroed again.
hipError_t lone_scratch_init(void* d_scratch, hipStream_t stream);
hipError_t launch_decode_lone_emit(int64_t n, uint8_t* d_out, int64_t cap, lz4ada_block_status* d_st,
                                   void* d_scratch, hipStream_t stream, int32_t H, uint8_t* h_out = nullptr);

// host side (lz4ada_host_common.cpp): the calling thread's message for
// lz4ada_thread_last_error() and its lz4ada_last_path() bits (set, or
// added to what the call has set so far)
void set_thread_error(const std::string& msg);
void set_last_path(int bits);
void add_last_path(int bits);

hipError_t launch_compact(const uint8_t* d_src, const lz4ada_block_desc* d_desc,
                          const uint64_t* d_dst_off, const lz4ada_block_status* d_status,
                          uint32_t nblocks, uint8_t* d_dst, hipStream_t stream);

// ---- many frames in one pass (lz4ada_frames.hip, lz4ada_xxh32.hip) ----
// One frame of a pass.  The host fills first / nblocks / flags /
// content_size; k_frames_plan fills out_off / out_len / fail / verdict from
// the block statuses, k_xxh32_spans fills hash.
constexpr uint32_t FRAME_HAS_SIZE = 1u;   // content_size is declared
constexpr uint32_t FRAME_HAS_CKSUM = 2u;  // C.Checksum
constexpr uint32_t FRAME_LINKED = 4u;     // B.Indep clear: its blocks are k_decode_idx_frames' 
constexpr int32_t FRAME_SIZE_BAD = 1;     // verdict: out_len != content_size
constexpr int32_t FRAME_GPU_HASHED = 2;   // verdict: hash holds XXH32 of the frame's output
struct FrameRec {
	uint32_t first, nblocks;  // its blocks among the pass's
	uint32_t flags;           // FRAME_HAS_*, FRAME_LINKED
	uint32_t hash;
	uint64_t content_size;
	uint64_t out_off, out_len;  // its bytes in the compacted output
	int32_t fail;               // first failing block (frame-relative), -1: none
	int32_t verdict;            // FRAME_SIZE_BAD | FRAME_GPU_HASHED
};
// Blocks per workgroup of the scan's first level.
constexpr uint32_t PLAN_TILE = 1024;
__host__ __device__ inline uint32_t plan_tiles(uint32_t nblocks)
{
	return (nblocks + PLAN_TILE - 1) / PLAN_TILE;
}
// The pass's layout, from the device-resident statuses: d_dst_off[0 ..
// nblocks] gets the exclusive prefix sum of the blocks' decoded lengths
// (entry nblocks: the total) -- what launch_compact reads -- and every
// frame record its span, first failing block and content-size verdict.  A
// block with a non-zero code, a length over its slot or a block checksum
// unequal to the declared one counts as failing and as 0 bytes (its
// out_len is set to 0, so launch_compact copies nothing of it; the host sets
// every record's fail to -1 beforehand).  Scratch: d_loc, nblocks words, and
// d_part, plan_tiles(nblocks) + 1 words.  nblocks may be 0.
hipError_t launch_frames_plan(const lz4ada_block_desc* d_desc, lz4ada_block_status* d_status,
                              uint32_t nblocks, FrameRec* d_frames, uint32_t nframes,
                              uint64_t* d_dst_off, uint64_t* d_loc, uint64_t* d_part,
                              hipStream_t stream);
// XXH32 of every frame's compacted output that has C.Checksum, no failing
// block and at most hash_max bytes, into its record (FRAME_GPU_HASHED set);
// four frames per wave.
hipError_t launch_xxh32_spans(const uint8_t* d_buf, FrameRec* d_frames, uint32_t nframes,
                              uint64_t hash_max, hipStream_t stream);
// The linked frames of a pass, one wave per frame (k_decode_idx_frames,
// lz4ada_idx.hip): pass 2 over the blocks [first, first + nblocks) of every
// record among d_frames[0 .. nframes) that carries FRAME_LINKED, in order,
// each block reading the frame's earlier output as history; records without
// the flag are left alone.  d_desc / d_status / nblocks are the arrays the
// records' `first` counts in, and d_tab the table of a launch_index over
// those blocks laid out for the same arrays (block b's records at
// ((in_off >> 8) + b)).  A block that is declined, short, not contiguous or in
// quirk D1's round state ends its frame's chain: it and the later blocks of
// the frame get a non-zero code.
hipError_t launch_decode_idx_frames(const uint8_t* d_frame, uint64_t frame_len,
                                    const lz4ada_block_desc* d_desc, uint32_t nblocks, const uint8_t* d_tab,
                                    uint8_t* d_out, lz4ada_block_status* d_status, const FrameRec* d_frames,
                                    uint32_t nframes, hipStream_t stream);

// ---- frames indexed on the device (lz4ada_frames_index.hip) ----
// A job's bytes inside the device input: the frame and whatever follows it.
struct FrameSpan {
	uint64_t off, len;
};
// What k_frames_walk found out about one frame (frame_walk, lz4ada_frame_walk.h).
struct FrameWalkRec {
	int32_t verdict;  // LZ4ADA_BATCH_*; _OVER_BUDGET when its slots alone exceed the budget
	uint32_t flags;   // FRAME_HAS_*, FRAME_LINKED (a modern frame with B.Indep clear)
	uint64_t nblocks;
	uint64_t slots, caps;  // sum of round256(slot_cap), sum of slot_cap
	int64_t frame_len;
	uint64_t content_size;
	uint32_t cksum;  // the declared content checksum
	int32_t format;  // LZ4ADA_FORMAT_*, 0 when the frame does not index
};
// One lane per frame: d_walk[i] from the frame at d_span[i].  Reads no byte
// outside a frame's span.  take_linked / linked_max: frame_walk's option
// (linked frames of at most linked_max slot bytes are accepted).
hipError_t launch_frames_walk(const uint8_t* d_in, const FrameSpan* d_span, uint32_t nframes, bool no_lone,
                              uint64_t budget, bool take_linked, uint64_t linked_max, FrameWalkRec* d_walk,
                              hipStream_t stream);
// One workgroup: d_first[i] / d_slot[i] get the blocks / slot bytes of the
// accepted frames (verdict LZ4ADA_BATCH_OK) before frame i, entry nframes the
// totals.  Frames that are not accepted count as nothing.
hipError_t launch_frames_scan(const FrameWalkRec* d_walk, uint32_t nframes, uint64_t* d_first,
                              uint64_t* d_slot, hipStream_t stream);
// One lane per frame: an accepted frame is walked again and its descriptors
// go to d_desc[d_first[i] ..] as a pass needs them (in_off absolute in d_in,
// out_off from d_slot[i] in steps of round256(slot_cap), out_cap = slot_cap);
// every frame gets its record d_rec[i] (fail -1; a frame that is not accepted
// holds no block).  Never writes past the frame's share of d_desc or of the
// slots: should the second walk differ from the first (the input changed in
// between), the frame's remaining descriptors are empty and its fail is 0.
hipError_t launch_frames_fill(const uint8_t* d_in, const FrameSpan* d_span, const FrameWalkRec* d_walk,
                              const uint64_t* d_first, const uint64_t* d_slot, uint32_t nframes,
                              bool no_lone, bool take_linked, uint64_t linked_max, lz4ada_block_desc* d_desc,
                              FrameRec* d_rec, hipStream_t stream);

// ---- exact decoded sizes (lz4ada_sizes.hip) ----
// What k_frame_sizes found out about one frame.
struct FrameSizeRec {
	uint64_t exact;   // its decoded bytes
	uint64_t tight;   // sum of round256(block size): its slots when a pass lays it out by size
	int32_t verdict;  // the walk's, or LZ4ADA_DEVFRAME_BLOCK / _SIZE; exact = tight = 0 unless 0
	uint32_t pad;
};
// One wave per block, after a launch_index over the same descriptors into
// d_tab and d_status: d_size[b] gets block b's decoded length, 0xFFFFFFFF when
// its chain is malformed (block_decoded_size, lz4ada_block_size.h).  Reads no
// byte outside a block's payload and writes nothing but d_size.
hipError_t launch_block_sizes(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                              const lz4ada_block_status* d_status, uint32_t nblocks, const uint8_t* d_tab,
                              uint32_t* d_size, hipStream_t stream);
// One lane per frame, over the frames of a launch_frames_scan / _fill with the
// nominal slots (d_first, d_desc) and their blocks' d_size: d_rec[i] as above.
// A frame is LZ4ADA_DEVFRAME_BLOCK when a block's size is unknown or over its
// slot_cap, or when a linked frame's middle block does not fill its slot, and
// LZ4ADA_DEVFRAME_SIZE when the sizes do not add up to a declared content
// size; d_walk[i].verdict then says so too, so that later scans and fills
// give the frame no block and no slot.  d_size_first[i]: size_base + its first
// block; d_tight[i]: d_walk[i] with the tight bytes as its slots.
hipError_t launch_frame_sizes(FrameWalkRec* d_walk, const uint64_t* d_first, uint32_t nframes, uint64_t size_base,
                              const lz4ada_block_desc* d_desc, const uint32_t* d_size, FrameSizeRec* d_rec,
                              uint64_t* d_size_first, FrameWalkRec* d_tight, hipStream_t stream);
// One lane per frame, over descriptors from launch_frames_fill whose d_first /
// d_slot come from a launch_frames_scan over d_tight: block k of frame i gets
// out_cap = its size and out_off from d_slot[i] in steps of round256(size).
// Never places a block past d_slot[i + 1].
hipError_t launch_frames_refit(const FrameWalkRec* d_tight, const uint64_t* d_first, const uint64_t* d_slot,
                               const uint64_t* d_size_first, const uint32_t* d_size, uint32_t nframes,
                               lz4ada_block_desc* d_desc, hipStream_t stream);

// ---- dictionary frames (lz4ada_dict.hip, lz4ada_idx.hip) ----
// A descriptor flag of a dictionary pass (bit 2: free beside the public flags
// and the linked path's BLOCK_D1_* bits, which such a pass never sets): the
// block is *gapped* -- DICT_GAP(dict_used) bytes lie in front of its slot and
// their last dict_used are the dictionary's last.
constexpr uint32_t BLOCK_DICT = 4u;
constexpr uint32_t DICT_MAX = 65536;  // dictionary bytes a block can reach (HISTORY_SIZE)
// The gap: the dictionary's used bytes, the 32 that decode_block's ring fill
// may read further back than its history, rounded up to 256 like every slot.
__host__ __device__ inline uint64_t dict_gap(uint32_t dict_used)
{
	return (uint64_t(dict_used) + 32 + 255) & ~uint64_t(255);
}
// How the frames of a dictionary pass take gaps, one word per frame, from the
// host's walk records: kind in the low 2 bits, the gapped blocks before the
// frame above them.
constexpr uint32_t DICT_KIND_NONE = 0;    // not modern, or without blocks: its blocks move, none is gapped
constexpr uint32_t DICT_KIND_LINKED = 1;  // one gap before the frame's first block
constexpr uint32_t DICT_KIND_INDEP = 2;   // a gap before every block
// One lane per block, after launch_frames_fill (and _refit): block k of frame f
// moves up by gap times the gapped blocks before it and including it, and a
// gapped block gets BLOCK_DICT.  A block that would end past `limit` (the
// slots and gaps the host reserved) becomes an empty one at 0 instead.
hipError_t launch_frames_dictgap(const FrameRec* d_rec, uint32_t nframes, const uint64_t* d_kind, uint64_t gap,
                                 uint64_t limit, lz4ada_block_desc* d_desc, uint32_t nblocks, hipStream_t stream);
// One workgroup per block: in front of every BLOCK_DICT block's slot, gap bytes
// whose last dict_used are d_dict[dict_len - dict_used, dict_len) and whose
// others are zeros.  16-byte stores (out_off is a multiple of 256), loads at
// any alignment.  Writes inside [out_off - gap, out_off) only, and nothing for
// a block whose out_off is below gap.
hipError_t launch_dict_fill(const lz4ada_block_desc* d_desc, uint32_t nblocks, const uint8_t* d_dict,
                            uint64_t dict_len, uint32_t dict_used, uint8_t* d_slots, hipStream_t stream);
// One lane per frame (LZ4ADA_DICT_CHECK_ID): a taken modern frame whose FLG bit
// 0 is set and whose dictionary id is not dict_id gets LZ4ADA_DEVFRAME_DICT as
// its walk verdict, so that later scans give it no block, and d_bad[i] = 1
// (else 0).  Reads the 4 id bytes of headers the walk has validated.
hipError_t launch_frames_dictid(const uint8_t* d_in, const FrameSpan* d_span, FrameWalkRec* d_walk,
                                uint32_t nframes, uint32_t dict_id, uint32_t* d_bad, hipStream_t stream);
// k_decode_idx_dict: pass 2 of independent blocks, one wave per block, hist =
// dict_used for a BLOCK_DICT block; d_tab from a launch_index over the same
// descriptors.  A block pass 1 declined keeps its DS_RETRY / DS_SPARSE.
hipError_t launch_decode_idx_dict(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                                  uint32_t nblocks, const uint8_t* d_tab, uint8_t* d_out,
                                  lz4ada_block_status* d_status, uint32_t dict_used, hipStream_t stream);
// k_decode_idx_frames_dict: launch_decode_idx_frames with hist starting at
// dict_used and without the quirk-D1 round state.
hipError_t launch_decode_idx_frames_dict(const uint8_t* d_frame, uint64_t frame_len,
                                         const lz4ada_block_desc* d_desc, uint32_t nblocks, const uint8_t* d_tab,
                                         uint8_t* d_out, lz4ada_block_status* d_status, const FrameRec* d_frames,
                                         uint32_t nframes, uint32_t dict_used, hipStream_t stream);
// k_decode_idx_chains: launch_decode_idx_frames_dict with the starting history
// of every chain in its own record (`hash`, clamped to DICT_MAX) instead of one
// for the launch: a ranged pass over a dictionary index decodes chains from
// checkpoints (65,536) and chains from the dictionary (dict_used) side by side
// (DESIGN.md §19).  A chain whose first block lacks BLOCK_DICT or lies less
// than dict_gap(history) into the slots gets DS_RETRY on its blocks.
hipError_t launch_decode_idx_chains(const uint8_t* d_frame, uint64_t frame_len, const lz4ada_block_desc* d_desc,
                                    uint32_t nblocks, const uint8_t* d_tab, uint8_t* d_out,
                                    lz4ada_block_status* d_status, const FrameRec* d_chains, uint32_t nchains,
                                    hipStream_t stream);

// ---- seek index and ranged decode (lz4ada_ranges.hip) ----
// The device arrays of a seek index over nframes frames in rising in_off, as
// the kernels see them.  first: n + 1 entries, frame k's blocks are
// [first[k], first[k + 1]) among desc (a frame the index did not accept holds
// none).  start / slotp: frame k's nb + 1 entries begin at first[k] + k: the
// decoded offset at which each block starts and the frame's size, and the same
// prefix over round256(size), the blocks' tight slots.
// An index that took linked frames also has kgrp: frame k's K,
// the blocks per checkpoint group, 0 for a frame of independent blocks, and
// ckfirst: n + 1 entries, frame k's checkpoints are [ckfirst[k], ckfirst[k + 1])
// among the nckpt entries of CKPT_BYTES bytes each at store.  All three are
// null / 0 in an index built without LZ4ADA_SEEK_LINKED.
// An index built with a dictionary has dict_used > 0, fkind:
// frame k's DICT_KIND_* (which of its blocks read the dictionary), and dict:
// the index's own copy as a gap image of dict_gap(dict_used) bytes, zeros and
// then the dictionary's last dict_used bytes.  Null / 0 otherwise.
struct SeekView {
	const lz4ada_block_desc* desc;
	const uint64_t* first;
	const uint64_t* start;
	const uint64_t* slotp;
	uint32_t nframes;
	const uint64_t* kgrp;
	const uint64_t* ckfirst;
	const uint8_t* store;
	uint64_t nckpt;
	const uint64_t* fkind;
	const uint8_t* dict;
	uint32_t dict_used;
};
// One range with bytes to deliver, as the host hands it to the kernels.
struct RangeRec {
	uint32_t frame, pad;  // sorted position of its frame
	uint64_t off, want;   // decoded bytes [off, off + want) of it, clipped: want > 0
	uint64_t out_off;     // where they go in d_out
	uint64_t tile0;       // its first tile among the gather's, counted over the call
};
// What k_ranges_select found for it, and k_ranges_verdict after the decode.
struct RangeSel {
	uint32_t first, count;      // the blocks it touches, frame-relative
	uint64_t slot_lo, slot_hi;  // slotp at its chain's start (chain_start: `first` unless linked), at first + count
	int32_t fail;               // first failing block among them (frame-relative), -1: none
	int32_t pad;
};
// Bytes of a range that one workgroup of k_ranges_gather copies.
constexpr uint64_t GATHER_TILE = 16384;
// One wave per frame: start / slotp of SeekView from the sizes stage's arrays
// (d_size_first[k]: frame k's first block among d_size).  d_first: the scan
// over the final verdicts, n + 1 entries.  Writes first[k] + k .. + nb per frame.
hipError_t launch_block_starts(const uint64_t* d_first, const uint64_t* d_size_first, const uint32_t* d_size,
                               uint32_t nframes, uint64_t* d_start, uint64_t* d_slotp, hipStream_t stream);
// One wave per range.  d_sel not null: every range's RangeSel (fail -1).
// d_mark not null: mark[b - span_lo] = 1 + round256(size) / 256 for every block
// b of the range's chain (lz4ada_range_chains.h: the blocks it touches, and in
// a linked frame those from its group's start on) inside [span_lo, span_lo +
// span_n), with RANGE_MARK_GAP added for a head (the same value from every
// writer), and in a dictionary index RANGE_MARK_DICT for a block that reads the
// dictionary (chain_dict_gapped).  Reads the index alone.
constexpr uint32_t RANGE_MARK_GAP = 0x80000000u;
constexpr uint32_t RANGE_MARK_DICT = 0x40000000u;
constexpr uint32_t RANGE_MARK_BITS = RANGE_MARK_GAP | RANGE_MARK_DICT;  // the size field needs 15 bits
// The gap in front of a head's slot: its checkpoint as a dictionary of DICT_MAX bytes.
constexpr uint64_t CKPT_GAP = (uint64_t(DICT_MAX) + 32 + 255) & ~uint64_t(255);
hipError_t launch_ranges_select(const SeekView& v, const RangeRec* d_ranges, uint32_t nranges, RangeSel* d_sel,
                                uint32_t* d_mark, uint64_t span_lo, uint32_t span_n, hipStream_t stream);
// One workgroup: d_cnt[i] / d_slot[i] get the marked blocks before span block i
// and where block i's bytes begin: past the slot bytes of the marked blocks
// before it and past the gaps (`gap` bytes per RANGE_MARK_GAP, `dict_gap` per
// RANGE_MARK_DICT) up to its own; entry span_n the totals.
hipError_t launch_ranges_scan(const uint32_t* d_mark, uint32_t span_n, uint64_t gap, uint64_t dict_gap,
                              uint32_t* d_cnt, uint64_t* d_slot, hipStream_t stream);
// One lane per span block: a marked block's descriptor goes to d_desc[d_cnt[i]]
// with out_off = d_slot[i] and out_cap = its exact size.  Writes no descriptor
// at or past nsel and places no block past slots (an empty one instead).
// d_chain not null (a pass with linked frames): d_chain[chain_slot(d_cnt[i],
// nsel)] (lz4ada_range_chains.h; chain_slots(nsel) records, zeroed by the
// caller) gets the block's chain record -- a head (BLOCK_DICT in its descriptor, its checkpoint's
// number among the store's in content_size) or a marked block 0 of a linked
// frame carries FRAME_LINKED, first = its own place and nblocks = the marked
// blocks of its group from it on (a walk over at most K marks); every other
// record has flags 0.  `hash` holds the chain's starting history: CKPT_BYTES
// for a head.  In a dictionary index a block with RANGE_MARK_DICT starts a
// chain too (BLOCK_DICT, hash = dict_used, content_size = CHAIN_NO_CKPT: of an
// independent frame a chain of that block alone, of a linked one block 0's).
hipError_t launch_ranges_fill(const SeekView& v, const uint32_t* d_mark, const uint32_t* d_cnt,
                              const uint64_t* d_slot, uint64_t span_lo, uint32_t span_n, uint32_t nsel,
                              uint64_t slots, lz4ada_block_desc* d_desc, FrameRec* d_chain, hipStream_t stream);
// One workgroup per compacted block: in front of the slot of every BLOCK_DICT
// block whose chain record names a checkpoint, CKPT_GAP bytes: zeros, then the
// checkpoint.  Writes inside [out_off - CKPT_GAP, out_off) only, and nothing
// where out_off < CKPT_GAP or out_off > slots.
hipError_t launch_ckpt_fill(const SeekView& v, const lz4ada_block_desc* d_desc, const FrameRec* d_chain,
                            uint32_t nsel, uint8_t* d_slots, uint64_t slots, hipStream_t stream);
// A chain record's content_size when its history is the dictionary, not a checkpoint.
constexpr uint64_t CHAIN_NO_CKPT = ~uint64_t(0);
// k_ckpt_fill's sibling for the dictionary: in front of the slot of every
// BLOCK_DICT block whose chain record says CHAIN_NO_CKPT, the index's gap image,
// dict_gap(dict_used) bytes.  Writes inside [out_off - dict_gap, out_off) only,
// and nothing where out_off < dict_gap or out_off > slots.
hipError_t launch_dictimg_fill(const SeekView& v, const lz4ada_block_desc* d_desc, const FrameRec* d_chain,
                               uint32_t nsel, uint8_t* d_slots, uint64_t slots, hipStream_t stream);
// The build: the checkpoints [ck_lo, ck_lo + nck) of the index, which are those
// of the sorted frames [f_lo, f_lo + nf) of one decode pass (d_rec: the pass's
// frame records after launch_frames_plan, d_desc its descriptors), from the
// pass's slots to the store, CKPT_SAVE_SPLIT workgroups per checkpoint.  A
// checkpoint whose frame does not have CKPT_BYTES contiguous decoded bytes in
// front of that block inside [0, slots) sets the frame's fail to 0 instead.
constexpr uint32_t CKPT_SAVE_SPLIT = 4;
hipError_t launch_ckpt_save(const uint64_t* d_kgrp, const uint64_t* d_ckfirst, uint32_t f_lo, uint32_t nf,
                            uint64_t ck_lo, uint32_t nck, uint64_t nckpt, const lz4ada_block_desc* d_desc,
                            uint32_t nblocks, FrameRec* d_rec, const uint8_t* d_slots, uint64_t slots,
                            uint8_t* d_store, hipStream_t stream);
// One wave per range, after the decode: d_sel[i].fail = the first block of the
// range's chain whose status is non-zero, whose length is not its size or
// whose block checksum differs.
hipError_t launch_ranges_verdict(const SeekView& v, const RangeRec* d_ranges, uint32_t nranges, RangeSel* d_sel,
                                 const uint32_t* d_cnt, uint64_t span_lo, uint32_t span_n,
                                 const lz4ada_block_desc* d_desc, const lz4ada_block_status* d_status,
                                 uint32_t nsel, hipStream_t stream);
// One workgroup per GATHER_TILE bytes of a range (tiles tile_lo .. tile_lo +
// ntiles of the call, which are those of d_ranges[0 .. nranges)): the range's
// bytes from the blocks' slots to d_out + out_off.  Reads d_slots inside
// [0, slots) and writes inside [out_off, out_off + want) only.
hipError_t launch_ranges_gather(const SeekView& v, const RangeRec* d_ranges, uint32_t nranges,
                                const RangeSel* d_sel, uint64_t tile_lo, uint32_t ntiles, const uint32_t* d_mark,
                                const uint64_t* d_slot, uint64_t span_lo, uint32_t span_n, const uint8_t* d_slots,
                                uint64_t slots, uint8_t* d_out, hipStream_t stream);

// ---- records compressed into frames (lz4ada_compress.hip) ----
// One block of a pass: its bytes inside d_in, its scratch slot (of at least
// len bytes), the job it belongs to.  The host fills them: it knows every length.
struct CompBlock {
	uint64_t in_off, slot_off;
	uint32_t len, job;
};
// One job of a pass: its record, its blocks among the pass's, and the header
// and trailer bytes of the pass's earlier jobs.
struct CompJob {
	uint64_t in_off, in_len;
	uint64_t fixed_before;
	uint32_t first, nblocks;
};
// What a pass reports per job: its frame inside d_out and its stored blocks
// (counted by atomic adds: zeroed by the caller).
struct CompJobRec {
	uint64_t out_off, out_len;
	uint32_t stored, pad;
};
// One wave per block: block b compressed into its slot, d_csize[b] its length
// there, or 0 for a block to be stored (the compressed form would not be
// shorter).  Writes inside [slot_off, slot_off + len - 1) only.  The pass's
// history picks the kernel (lz4ada_compress_block.inc):
//  * dl == 0, no cont: k_compress_blocks, nothing in front of a block; d_jobs,
//    d_tail and d_seed are not read;
//  * dl != 0, no cont: k_compress_blocks_dict: dl bytes
//    (4 .. 65,536) at d_tail lie in front of every block, d_seed is their table
//    as launch_compress_dict_table left it.  Reads d_tail inside [0, dl);
//  * cont, a linked pass that holds a continuation block:
//    k_compress_blocks_linked.  Block b begins its record when
//    its in_off is d_jobs[d_blk[b].job].in_off and is then compressed as above
//    (dl == 0: no dictionary); any other block has the 65,536 bytes in front of
//    it in d_in as its history and seeds its own table from them.
hipError_t launch_compress_blocks(const uint8_t* d_in, const CompBlock* d_blk, const CompJob* d_jobs, uint32_t nblocks,
                                  bool cont, const uint8_t* d_tail, uint32_t dl, const uint32_t* d_seed,
                                  uint8_t* d_slots, uint32_t* d_csize, hipStream_t stream);
// d_seed[0 .. COMP_TABLE): for every hash the last position + 1 of d_tail[0 .. dl)
// whose four bytes lie inside it, 0 for none (dl < 4: all 0).
hipError_t launch_compress_dict_table(const uint8_t* d_tail, uint32_t dl, uint32_t* d_seed, hipStream_t stream);
// The exclusive prefix sum of the blocks' bytes in the output (size word,
// payload, checksum under `flags`): block b's is d_part[b / PLAN_TILE] +
// d_loc[b], the total d_part[plan_tiles(nblocks)].  nblocks may be 0.
hipError_t launch_compress_scan(const CompBlock* d_blk, const uint32_t* d_csize, uint32_t nblocks, uint32_t flags,
                                uint64_t* d_loc, uint64_t* d_part, hipStream_t stream);
// One workgroup per block: size word and payload into d_out (the pass begins
// at d_out + base), d_desc[b] the payload inside d_out, d_rec[job].stored.
// dflags: a dictionary call's LZ4ADA_COMP_DICT_* (the header's length), else 0.
hipError_t launch_compress_emit(const uint8_t* d_in, const uint8_t* d_slots, const CompBlock* d_blk,
                                const uint32_t* d_csize, const uint64_t* d_loc, const uint64_t* d_part,
                                const CompJob* d_jobs, uint32_t nblocks, uint32_t flags, uint32_t dflags, uint64_t base,
                                uint8_t* d_out, lz4ada_block_desc* d_desc, CompJobRec* d_rec, hipStream_t stream);
// d_st[b].cksum (launch_block_checksums over d_out and d_desc) behind every payload.
hipError_t launch_compress_block_cksums(const lz4ada_block_desc* d_desc, const lz4ada_block_status* d_st,
                                        uint32_t nblocks, uint8_t* d_out, hipStream_t stream);
// One thread per job: header, end mark, the content checksum when d_frec[j]
// carries one (launch_xxh32_spans over d_in; d_frec may be null without
// LZ4ADA_COMP_CONTENT_CHECKSUM), and d_rec[j].out_off / out_len.  dflags and
// dict_id: a dictionary call's, for the header; else 0.  linked: nonzero for
// frames of linked blocks (B.Indep clear).
hipError_t launch_compress_frames(const CompJob* d_jobs, uint32_t njobs, const uint64_t* d_loc, const uint64_t* d_part,
                                  uint32_t nblocks, uint32_t block_id, uint32_t flags, uint32_t dflags,
                                  uint32_t dict_id, uint32_t linked, uint64_t base, const FrameRec* d_frec,
                                  uint8_t* d_out, CompJobRec* d_rec, hipStream_t stream);

// ---- the seek index a compress call writes (lz4ada_compress_index.hip) ----
// The index's device arrays as the pass's kernels fill them (SeekView's, writable)
// and what the host sized them by: nblocks descriptors, nckpt checkpoints in
// store, nframes frames.  kgrp / ckfirst / store: null unless the call is
// linked; fkind: null without a dictionary.
struct CompIndexOut {
	lz4ada_block_desc* desc;
	uint64_t *first, *start, *slotp;
	uint64_t *kgrp, *ckfirst;
	uint8_t* store;
	uint64_t* fkind;
	uint64_t nblocks, nckpt;
	uint32_t nframes;
};
// What k_compress_index_frames says about job j of a pass: its first
// descriptor, its first block's nominal slot and its first checkpoint among the
// index's, and the rule's verdict (LZ4ADA_BATCH_*; a frame not taken holds
// nothing).  Entry njobs: the totals after the pass, the next pass's `base`.
struct CompIndexRec {
	uint64_t first, out_base, ck;
	int32_t verdict;
	uint32_t pad;
};
// The three kernels of a pass over d_jobs[0 .. njobs) / d_blk[0 .. nblocks), the
// call's jobs f_lo .. f_lo + njobs, once launch_compress_emit (d_emitted: its
// descriptors) and the block checksums (d_st; null without them) are queued.
// kind: the CHAIN_KIND_* of a taken frame with blocks (NONE without a
// dictionary).  ckpts: the pass holds a continuation block of a linked call, so
// k_ckpt_from_records runs: it reads d_in inside the jobs' records alone and
// writes checkpoints [base.ck, d_rec[njobs].ck).  d_rec: njobs + 1 records.
hipError_t launch_compress_index(const uint8_t* d_in, uint64_t in_len, const CompBlock* d_blk, const CompJob* d_jobs,
                                 uint32_t nblocks, uint32_t njobs, const uint32_t* d_csize,
                                 const lz4ada_block_desc* d_emitted, const lz4ada_block_status* d_st,
                                 uint32_t block_id, uint32_t flags, bool linked, bool ckpts, uint64_t every,
                                 bool no_lone, uint32_t kind, uint32_t f_lo, const CompIndexRec& base,
                                 const CompIndexOut& o, CompIndexRec* d_rec, hipStream_t stream);

}  // namespace lz4ada
