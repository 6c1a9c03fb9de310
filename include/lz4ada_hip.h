/*
 * lz4ada_hip.h -- C-ABI of the MI355X-native LZ4Ada decompressor.
 *
 * Drop-in boundary for the reference's public Ada API (lib/lz4ada.ads):
 * every entry point below names the reference subprogram it replaces.  An
 * Ada caller binds them with pragma Import (bindings/ada/lz4ada.ads,
 * INTEGRATION.md); Python binds them with ctypes (bo-lz4-ada_amd/lz4ada.py).
 *
 * Plain pointers and sizes only.  Lengths are int64_t so that both the
 * Integer and the Stream_Element_Offset overloads map onto one entry point.
 * Status codes are 1:1 with the reference's exceptions (lz4ada.ads:133-162);
 * the exact Exception_Information message is available from
 * lz4ada_last_error() / lz4ada_thread_last_error().
 *
 * Block decode and block XXH32 run on the GPU (HIP kernels for gfx950).
 * Frame-header parsing, the Update state machine and the serial XXH32 chain
 * over host-resident bytes (content checksums, the XXHash32 API) are host
 * code.  There is no CPU fallback: without a usable GPU,
 * calls that would decode return LZ4ADA_DEVICE_ERROR.
 */
#ifndef LZ4ADA_HIP_H
#define LZ4ADA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZ4ADA_HIP_ABI_VERSION 1

/* ---------------------------------------------------------------- enums */

/* Exceptions (lz4ada.ads:133-162). */
typedef enum {
	LZ4ADA_OK = 0,
	LZ4ADA_CHECKSUM_ERROR = 1,       /* LZ4Ada.Checksum_Error */
	LZ4ADA_DATA_CORRUPTION = 2,      /* LZ4Ada.Data_Corruption */
	LZ4ADA_NOT_SUPPORTED = 3,        /* LZ4Ada.Not_Supported */
	LZ4ADA_TOO_FEW_HEADER_BYTES = 4, /* LZ4Ada.Too_Few_Header_Bytes */
	LZ4ADA_TOO_LITTLE_MEMORY = 5,    /* LZ4Ada.Too_Little_Memory */
	LZ4ADA_ASSERTION_ERROR = 6,      /* Pre/Assert violated (API misuse) */
	LZ4ADA_CONSTRAINT_ERROR = 7,     /* library-internal check */
	LZ4ADA_DEVICE_ERROR = 8,         /* HIP error / no GPU (no reference twin) */
	LZ4ADA_EXACT_PATH = 9            /* device-only call: the frame needs lz4ada_decode_frame */
} lz4ada_status;

/* Flexible_Memory_Reservation (lz4ada.ads:79-106), same order. */
typedef enum {
	LZ4ADA_SZ_64_KIB = 0,
	LZ4ADA_SZ_256_KIB = 1,
	LZ4ADA_SZ_1_MIB = 2,
	LZ4ADA_SZ_4_MIB = 3,
	LZ4ADA_SZ_8_MIB = 4,
	LZ4ADA_USE_FIRST = 5,
	LZ4ADA_SINGLE_FRAME = 6,
	LZ4ADA_FOR_MODERN = LZ4ADA_SZ_4_MIB, /* lz4ada.ads:92 */
	LZ4ADA_FOR_LEGACY = LZ4ADA_SZ_8_MIB, /* lz4ada.ads:100 */
	LZ4ADA_FOR_ALL = LZ4ADA_SZ_8_MIB     /* lz4ada.ads:106 */
} lz4ada_reservation;

/* End_Of_Frame (lz4ada.ads:124). */
typedef enum { LZ4ADA_EOF_YES = 0, LZ4ADA_EOF_NO = 1, LZ4ADA_EOF_MAYBE = 2 } lz4ada_end_of_frame;

/* ------------------------------------------------- streaming decompressor */

/* Opaque Decompressor context (lz4ada.ads:126, 440-449).  Owns device
 * buffers (Buffer mirror holding the 64 KiB history, block staging, content
 * hash state); not copyable; one thread at a time. */
typedef struct lz4ada_decompressor lz4ada_decompressor;

/* LZ4Ada.Init (lz4ada.ads:189-191, 218-220; lz4ada.adb:48-63).
 * reservation: one of LZ4ADA_SZ_*. */
int lz4ada_init(int reservation, int64_t *min_buffer_size, lz4ada_decompressor **ctx);

/* LZ4Ada.Init_With_Header (lz4ada.ads:238-243; lz4ada.adb:79-125).
 * Requires len >= 7 (Pre).  On failure *ctx is NULL and the message is in
 * lz4ada_thread_last_error(). */
int lz4ada_init_with_header(const uint8_t *input, int64_t len, int reservation,
                            int64_t *num_consumed, int64_t *min_buffer_size,
                            lz4ada_decompressor **ctx);

/* LZ4Ada.Init_For_Block (lz4ada.ads:255-258; lz4ada.adb:127-147). */
int lz4ada_init_for_block(int64_t compressed_length, int reservation,
                          int64_t *min_buffer_size, lz4ada_decompressor **ctx);

/* LZ4Ada.Update (lz4ada.ads:211-216, 281-287; lz4ada.adb:383-418).
 * buffer is the caller-owned 0-based Buffer (length >= min_buffer_size);
 * it must not be modified between calls.  At most one block of output is
 * returned, as inclusive indices [*output_first, *output_last]
 * (first = 1, last = 0 when nothing was produced). */
int lz4ada_update(lz4ada_decompressor *ctx, const uint8_t *input, int64_t len,
                  int64_t *num_consumed, uint8_t *buffer, int64_t buffer_len,
                  int64_t *output_first, int64_t *output_last);

/* LZ4Ada.Is_End_Of_Frame (lz4ada.ads:303; lz4ada.adb:906-915). */
int lz4ada_is_end_of_frame(const lz4ada_decompressor *ctx);

/* Exception message of the last failed call on ctx, and the reference
 * exception name for a status ("LZ4ADA.DATA_CORRUPTION"). */
const char *lz4ada_last_error(const lz4ada_decompressor *ctx);
/* Blocks this context sent through the reference-exact single-lane path
 * (k_serial_block: errors, quirk D1, anything the GPU decoders decline);
 * every other block was decoded by the parallel GPU decoders.  Diagnostic,
 * no reference twin. */
int64_t lz4ada_exact_blocks(const lz4ada_decompressor *ctx);
const char *lz4ada_error_name(int status);
/* Message of the last failed context-less call on this thread. */
const char *lz4ada_thread_last_error(void);

void lz4ada_free(lz4ada_decompressor *ctx);

/* LZ4Ada.To_Hex (lz4ada.ads:306-307); writes 3 / 9 bytes incl. NUL. */
void lz4ada_to_hex8(uint8_t v, char out[3]);
void lz4ada_to_hex32(uint32_t v, char out[9]);

/* ---------------------------------------------------------------- XXHash32 */

/* LZ4Ada.XXHash32.Hasher (lz4ada.ads:335-343).  Plain struct so callers can
 * embed it.  Host bytes are hashed on the calling thread (the chain is one
 * serial dependency); device-resident bytes by the GPU kernel or
 * the D2H pipeline below, on the same state.  `hash` caches Final(). */
typedef struct {
	uint32_t state[4];
	uint8_t buffer[16];
	int32_t buffer_size;
	uint32_t hash;
	uint64_t total_length;
} lz4ada_xxh32_state;

/* XXHash32.Init (lz4ada.adb:925-930): Seed is ignored (quirk Q1). */
void lz4ada_xxh32_init(lz4ada_xxh32_state *h, uint32_t seed);
/* XXHash32.Reset (lz4ada.adb:932-940). */
void lz4ada_xxh32_reset(lz4ada_xxh32_state *h, uint32_t seed);
/* XXHash32.Update (lz4ada.adb:942-963) over host bytes (host chain, no
 * device round trip). */
int lz4ada_xxh32_update(lz4ada_xxh32_state *h, const uint8_t *data, int64_t len);
/* Same over device-resident bytes; stream is a hipStream_t (0 = default). */
int lz4ada_xxh32_update_device(lz4ada_xxh32_state *h, const void *d_data, int64_t len,
                               void *stream);
/* Content checksum pipeline: XXHash32.Update over
 * device-resident bytes copied to the host in 32 MiB chunks, each chunk
 * hashed on the calling host thread while the next one is in flight; the
 * bytes also land in host_out when it is not NULL.  The serial chain runs
 * ~5x faster on a host core than on one GPU wave. */
int lz4ada_content_xxh32_d2h(lz4ada_xxh32_state *h, const void *d_data, int64_t len,
                             uint8_t *host_out, void *stream);
/* XXHash32.Final (lz4ada.adb:993-1017). */
uint32_t lz4ada_xxh32_final(const lz4ada_xxh32_state *h);
/* XXHash32.Hash (lz4ada.adb:1019-1024), seed 0, host bytes. */
int lz4ada_xxh32_hash(const uint8_t *data, int64_t len, uint32_t *out);

/* ------------------------------------------------------- bulk frame decode */
/*
 * The hot path.  A whole LZ4 frame is indexed on the host (a serial walk of
 * the 4-byte block size words, lz4ada.adb:525-585) and every block is then
 * decoded by its own wavefront on the GPU, with block checksums
 * (lz4ada.adb:698-707) verified on the GPU.  Output lands in per-block
 * slots of block_max bytes (desc.out_off), contiguous whenever every
 * non-last block is full.  lz4ada_decode_frame() decodes independent
 * blocks this way; linked frames (and independent ones whose blocks read
 * earlier blocks, quirk D2) decode every block at once against a synthetic
 * history that the GPU then resolves (quirk D1
 * emulated there, section 6).  A non-zero block status, a failed checksum,
 * a D1 read the GPU does not emulate or a reference before the frame start
 * sends the frame (from that block on) down the reference-exact serial
 * path, which reproduces the reference's output and exception.
 */

typedef struct {
	uint64_t in_off;  /* payload offset inside the frame */
	uint32_t in_len;  /* payload bytes (size word & 0x7FFFFFF) */
	uint32_t flags;   /* LZ4ADA_BLOCK_* */
	uint64_t out_off; /* output slot offset */
	uint32_t out_cap; /* slot capacity (block_max) */
	uint32_t cksum;   /* declared block checksum (if present) */
} lz4ada_block_desc;

#define LZ4ADA_BLOCK_STORED 1u    /* size word bit 31 set */
#define LZ4ADA_BLOCK_HAS_CKSUM 2u /* FLG.B.Checksum */

typedef struct {
	int32_t code;        /* 0 = ok; else device status */
	int32_t aux;
	int64_t detail;
	int64_t err_out_pos; /* block-relative output count at the error */
	uint32_t out_len;    /* decoded bytes */
	uint32_t cksum;      /* XXH32 of the compressed payload */
} lz4ada_block_status;

#define LZ4ADA_FORMAT_MODERN 1
#define LZ4ADA_FORMAT_LEGACY 2
#define LZ4ADA_FORMAT_SKIPPABLE 3

typedef struct {
	int32_t format;           /* LZ4ADA_FORMAT_* */
	uint8_t flg, bd;          /* frame descriptor bytes (modern) */
	uint8_t block_checksum;   /* FLG bit 4 */
	uint8_t content_checksum; /* FLG bit 2 */
	uint8_t has_content_size; /* FLG bit 3 */
	uint8_t independent;      /* FLG bit 5 (B.Indep; ignored by the reference) */
	uint8_t pad[2];
	int64_t block_max;        /* BD block maximum (8 MiB for legacy) */
	int64_t header_len;
	int64_t nblocks;
	int64_t frame_len;        /* bytes of this frame incl. end mark + checksum */
	uint64_t content_size;
	uint32_t content_checksum_declared;
	uint32_t pad2;
} lz4ada_frame_info;

/* Index one frame starting at frame[0].  descs may be NULL to count blocks
 * (then info->nblocks is set and LZ4ADA_OK returned).  Slots are laid out
 * at i * block_max.  Errors carry the reference's header messages. */
int lz4ada_frame_index(const uint8_t *frame, int64_t len, lz4ada_frame_info *info,
                       lz4ada_block_desc *descs, int64_t desc_cap);

/* Launch the per-block kernels over a device-resident frame: block XXH32
 * (when LZ4ADA_BLOCK_HAS_CKSUM) and decode into d_out.  Asynchronous on
 * `stream` (hipStream_t).  d_frame must stay readable up to frame_len.
 * The checksums run on a library-owned side stream beside the decoder's
 * first pass (forked from and joined back into `stream` by events; set
 * LZ4ADA_NO_OVERLAP to serialise them). */
int lz4ada_decode_blocks_device(const void *d_frame, uint64_t frame_len,
                                const lz4ada_block_desc *d_descs, int64_t nblocks,
                                void *d_out, lz4ada_block_status *d_status,
                                void *stream);

/* Decode-only / checksum-only halves of the above (for profiling). */
int lz4ada_launch_decode(const void *d_frame, uint64_t frame_len,
                         const lz4ada_block_desc *d_descs, int64_t nblocks, void *d_out,
                         lz4ada_block_status *d_status, void *stream);
/* Decoder variants of the bulk path: the two-wave
 * producer/consumer decoder (1, the round-1 one-wave decoder, and 2, the
 * workgroup decoder, are retired: LZ4ADA_DEVICE_ERROR). */
#define LZ4ADA_DECODE_PC 0
/* Index-driven two-pass decoder (k_index + k_decode_idx, lz4ada_idx.hip),
 * then the two-wave decoder for the blocks it declines; _ALONE skips that
 * second step (declined blocks keep status code 10). */
#define LZ4ADA_DECODE_IDX 3
#define LZ4ADA_DECODE_IDX_ALONE 4
/* The blocks of one LINKED frame (slots contiguous, block_max >= 256 KiB):
 * sequence index of every block at once, then the blocks in order with the
 * earlier output as history; from the first declined or short block on,
 * every block is left with status code 10 (the exact path takes over). */
#define LZ4ADA_DECODE_IDX_LINKED 5
/* The index-driven decoder, then the literal-heavy decoder (k_decode_sparse)
 * for the blocks pass 1 declines as sparse; no two-wave pass: blocks either
 * declines keep status code 10 (retry). */
#define LZ4ADA_DECODE_IDX_SPARSE 6
/* The fused index decoder alone with one wave per block (k_decode_idx) or
 * two pipelining batches (k_decode_pp2; _IDX2_ALONE named round 4's
 * k_decode_idx2, retired in round 6, and now runs k_decode_pp2); declined
 * blocks keep status code 10.  The default of LZ4ADA_DECODE_IDX / _ALONE
 * picks by launch size: k_decode_pp2 for at most 4x the CU count in
 * blocks, k_decode_idx above; LZ4ADA_IDX_WAVES=1 / p forces k_decode_idx /
 * k_decode_pp2 (lz4ada_bulk_decoder_kernel() names the one a launch uses). */
#define LZ4ADA_DECODE_IDX1_ALONE 7
#define LZ4ADA_DECODE_IDX2_ALONE 8
/* The pipelined two-wave decoder (k_decode_pp2: two waves per block taking
 * alternate batches) alone; declined blocks keep status code 10 / 11. */
#define LZ4ADA_DECODE_PP2_ALONE 9
/* The index decoder's two passes as two launches (k_index, then
 * k_decode_idx's pass 2): per-pass timing and counters. */
#define LZ4ADA_DECODE_IDX_SPLIT 10

int lz4ada_launch_decode_variant(const void *d_frame, uint64_t frame_len,
                                 const lz4ada_block_desc *d_descs, int64_t nblocks, void *d_out,
                                 lz4ada_block_status *d_status, int variant, void *stream);
/* Test-only, like the variants above: pass 1 of the index decoder alone
 * (k_index, by `waves` = 1 or 2 waves per block: the pass 1 that
 * k_decode_idx and k_decode_pp2 run; any other value is a constraint error)
 * into a scratch table, which is copied to host_out (host_cap
 * bytes; the call fails when the table is larger).  Block b's records
 * start at byte 64 * ((in_off >> 8) + b) of the table: one 8-byte record
 * per 32-byte sub-segment of its payload, start bitmap | output bytes << 32
 * (the low 16 bits of the count saturate at 0xFFFF; the whole high word then
 * holds the exact count).  d_status gets pass 1's verdict per block (code 0
 * accepted, 10 declined, 11 literal-heavy).  Returns after the stream has
 * drained; the table's size in bytes is ((frame_len >> 8) + nblocks + 2) * 64. */
int lz4ada_index_table_debug(const void *d_frame, uint64_t frame_len,
                             const lz4ada_block_desc *d_descs, int64_t nblocks, void *host_out,
                             int64_t host_cap, lz4ada_block_status *d_status, void *stream,
                             int waves);
/* The name of the kernel the fused bulk decode (LZ4ADA_DECODE_IDX, the
 * product call lz4ada_decode_blocks_device) launches for nblocks blocks --
 * it depends on how the block count fills the chip (for benches and
 * profiles; a static string). */
const char *lz4ada_bulk_decoder_kernel(int64_t nblocks);

/* One block (payload d_blk, n bytes, no history) decoded by the whole GPU
 * (lz4ada_lone.hip: every byte position parsed, the sequence chain found by
 * pointer jumping, copies resolved by pointer jumping over one word per
 * output byte) into d_out (cap bytes); *d_status gets code 0 and out_len, or
 * 10 (declined: malformed data, a reference before the block start, an
 * output over cap -- the exact path gives the reference's result).  The
 * streaming facade's decoder for lone blocks.  d_scratch: device memory of
 * lz4ada_lone_scratch_bytes(n, cap) bytes.  Asynchronous on stream. */
int64_t lz4ada_lone_scratch_bytes(int64_t n, int64_t cap);
int lz4ada_launch_decode_lone(const void *d_blk, int64_t n, void *d_out, int64_t cap,
                              lz4ada_block_status *d_status, void *d_scratch,
                              int64_t scratch_bytes, void *stream);

int lz4ada_launch_block_checksums(const void *d_frame, const lz4ada_block_desc *d_descs,
                                  int64_t nblocks, lz4ada_block_status *d_status,
                                  void *stream);

/* XXH32 of each decoded slot (golden checks). */
int lz4ada_output_checksums_device(const void *d_out, const lz4ada_block_desc *d_descs,
                                   const lz4ada_block_status *d_status, int64_t nblocks,
                                   uint32_t *d_hash, void *stream);

/* Decode one complete single frame (Init_With_Header(Single_Frame) + Update
 * semantics, as tool_unlz4ada does per frame) from host memory into host
 * memory.  *frame_consumed = bytes of this frame; *out_len = decoded bytes.
 * On failure the reference's exception message is in
 * lz4ada_thread_last_error().  out_cap must be >= the decoded size. */
int lz4ada_decode_frame(const uint8_t *frame, int64_t len, uint8_t *out, int64_t out_cap,
                        int64_t *out_len, int64_t *frame_consumed);

/* Decode every frame of a concatenated stream (skippable frames skipped). */
int lz4ada_decode_stream(const uint8_t *input, int64_t len, uint8_t *out, int64_t out_cap,
                         int64_t *out_len);

/* The same two calls into a buffer the library allocates and grows, so no
 * bound is needed up front (a stream that fails to index part-way still
 * raises the reference's own exception); release it with
 * lz4ada_buffer_free().  On failure *out is NULL. */
int lz4ada_decode_frame_alloc(const uint8_t *frame, int64_t len, uint8_t **out, int64_t *out_len,
                              int64_t *frame_consumed);
int lz4ada_decode_stream_alloc(const uint8_t *input, int64_t len, uint8_t **out,
                               int64_t *out_len);
void lz4ada_buffer_free(uint8_t *p);

/* lz4ada_decode_frame_alloc, except that on failure *out / *out_len hold
 * what the reference would have output before raising: every block before
 * the failing one, each returned by its own Update call (lz4ada.adb:383-418,
 * 661-714; tool_unlz4ada/unlz4ada.adb:41 writes each at once).  The exact
 * path resumes at (or just before) the failing block with the stream state
 * replayed from the decoded lengths, so the error comes in about the time
 * the bulk path needs, not after a redo of the frame.  Free *out with
 * lz4ada_buffer_free() in both cases. */
int lz4ada_decode_frame_partial(const uint8_t *frame, int64_t len, uint8_t **out,
                                int64_t *out_len, int64_t *frame_consumed);

/* The linked-frame bulk path over a device-resident frame (BASELINE
 * configs[4]): every block at once against a synthetic history, resolved
 * on the GPU, into contiguous device output d_out
 * (out_cap bytes); descs are the HOST descriptors from lz4ada_frame_index.
 * Synchronous on `stream`.  Returns LZ4ADA_EXACT_PATH when the reference
 * would raise or diverge in a way the GPU does not reproduce (block error,
 * checksum mismatch, a quirk-D1 read it does not emulate, a reference
 * before the frame start) -- lz4ada_decode_frame() then gives
 * the reference's result.  The content checksum is the caller's. */
int lz4ada_decode_linked_device(const void *d_frame, uint64_t frame_len,
                                const lz4ada_block_desc *descs, int64_t nblocks, int64_t block_max,
                                void *d_out, int64_t out_cap, int64_t *out_len, void *stream);

/* Paths the last lz4ada_decode_* call on this thread took (bit mask):
 * independent blocks in bulk, linked blocks in bulk (synthetic history
 * resolved on the GPU), the reference-exact serial path. */
#define LZ4ADA_PATH_INDEPENDENT 1
#define LZ4ADA_PATH_LINKED 2
#define LZ4ADA_PATH_EXACT 4
#define LZ4ADA_PATH_MULTI 8 /* lz4ada_decode_frame_multi* took the call */
#define LZ4ADA_PATH_BATCH 16 /* the frame was committed from a multi-frame pass */
int lz4ada_last_path(void);

/* ------------------------------------------- many frames in one device pass */
/*
 * A caller with many small frames (concatenated .lz4 files, one frame per
 * flush or per page) gets one device pass per budgetful of frames instead
 * of one per frame: the frames' blocks are decoded by one launch, a device
 * scan (k_frames_plan) lays the output out back to back and judges every
 * frame, content checksums are hashed side by side on the GPU
 * (k_xxh32_spans), and one small copy of the per-frame records plus one
 * copy of the bytes bring the results back.  No
 * reference twin: the calls replace the caller's per-frame
 * Init_With_Header / Update loop (tool_unlz4ada/unlz4ada.adb:84-103).  A
 * frame the pass does not find good in every respect is decoded again on
 * its own by the path lz4ada_decode_frame takes, which gives the
 * reference's output, exception and message.
 */

/* Why a frame does not take the batch path (lz4ada_stream_entry.batchable). */
#define LZ4ADA_BATCH_OK 0
#define LZ4ADA_BATCH_LINKED 1      /* modern with B.Indep clear */
#define LZ4ADA_BATCH_BIG_BLOCK 2   /* a block slot over 4 MiB, or blocks the lone-block decoder takes */
#define LZ4ADA_BATCH_OVER_BUDGET 3 /* its slots alone exceed LZ4ADA_BATCH_BYTES */
#define LZ4ADA_BATCH_NOT_INDEXED 4 /* does not index, or is cut short */

typedef struct {
	int64_t offset, frame_len; /* where the frame lies in the input */
	lz4ada_frame_info info;    /* as lz4ada_frame_index gives it */
	int32_t batchable;         /* LZ4ADA_BATCH_* reason code, 0 = takes the batch path */
	int32_t pad;
} lz4ada_stream_entry;

/* Walk every frame of a concatenated stream (host only, no HIP call).
 * entries may be NULL to count.  Stops at the first frame that does not
 * index or is cut short: *nframes counts the frames before it and the
 * return value is that frame's status (message in
 * lz4ada_thread_last_error()). */
int lz4ada_stream_index(const uint8_t *input, int64_t len, lz4ada_stream_entry *entries,
                        int64_t cap, int64_t *nframes);

typedef struct {
	const uint8_t *frame; /* in: one frame (Single_Frame semantics) */
	int64_t len;
	int64_t out_off, out_len; /* out: its bytes inside *out */
	int64_t consumed;         /* out: bytes of the frame */
	int32_t status;           /* out: lz4ada_status of THIS frame */
	int32_t path;             /* out: LZ4ADA_PATH_* bits this frame took */
} lz4ada_frame_job;

/* Decode njobs independent frames.  Returns LZ4ADA_OK when the call itself
 * worked, whatever the per-job statuses; a failed job holds what the
 * reference had output before raising (as lz4ada_decode_frame_partial).
 * *out is library-allocated (lz4ada_buffer_free). */
int lz4ada_decode_frames(lz4ada_frame_job *jobs, int64_t njobs, uint8_t **out, int64_t *out_len);
/* Message of job i of the last lz4ada_decode_frames call on this thread
 * ("" for a job that succeeded or an index out of range). */
const char *lz4ada_frames_error(int64_t i);

/* lz4ada_decode_stream / _alloc take the same engine when the stream holds
 * at least two batchable frames (LZ4ADA_NO_BATCH=1: never); the frames are
 * committed in order and the first failing frame's exception is returned
 * after the frames before it, as the per-frame loop does. */

typedef struct {
	int64_t frames_batched, frames_single, passes, gpu_hashed, host_hashed;
} lz4ada_batch_stats;
/* Counters of the last lz4ada_decode_frames / _stream call on this thread:
 * frames committed from a pass, frames decoded on their own, passes, content
 * checksums hashed by k_xxh32_spans and by the host chain.  No HIP call. */
void lz4ada_last_batch_stats(lz4ada_batch_stats *out);
/* The decoded length up to which a pass hashes a frame's content checksum
 * on the GPU (longer frames: the host chain while their bytes are copied
 * out): the built-in default, or LZ4ADA_BATCH_HASH_MAX, read per call. */
int64_t lz4ada_batch_hash_max(void);
/* k_xxh32_spans alone (tools/frames_batch_xxh.py, tests): XXH32, seed 0, of
 * the nspans spans (off[i], len[i]) -- host arrays -- of the device buffer
 * d_buf into the host array hash[i]; four spans per wave.  Synchronous;
 * *kernel_ms (may be NULL) gets the kernel's time between device events. */
int lz4ada_xxh32_spans_device(const void *d_buf, const int64_t *off, const int64_t *len,
                              int64_t nspans, uint32_t *hash, float *kernel_ms);

/* ---------------------------------------------- linked frames in a pass */
/*
 * Linked blocks are the LZ4F default, so many small frames written by a
 * library are linked frames.  With LZ4ADA_FRAMES_LINKED in `flags`, a modern
 * frame with B.Indep clear shares the pass when it passes every other rule
 * and its slots sum to at most lz4ada_batch_linked_max() bytes; one wave
 * decodes its blocks in order (k_decode_idx_frames),
 * N frames side by side.  A frame over the cap keeps LZ4ADA_BATCH_LINKED.
 * info.independent stays 0.  A linked frame the pass does not find good in
 * every respect (a block error, a block checksum, quirk D1 in its round
 * state, a reference before the frame start, a short middle block) goes the
 * single way as every other such frame: the reference's bytes and exception
 * from the host calls, LZ4ADA_EXACT_PATH / LZ4ADA_DEVFRAME_BLOCK from the
 * device call.  A committed linked frame reports LZ4ADA_PATH_BATCH |
 * LZ4ADA_PATH_LINKED.  flags 0 is the call without _opt.  The calls without
 * _opt, lz4ada_decode_stream / _alloc and the CLIs built on them take
 * LZ4ADA_BATCH_LINKED=1 from the environment, read per call, as their flags.
 */
#define LZ4ADA_FRAMES_LINKED 1u /* flags: linked frames up to lz4ada_batch_linked_max() share the pass */
int lz4ada_decode_frames_opt(lz4ada_frame_job *jobs, int64_t njobs, uint32_t flags, uint8_t **out,
                             int64_t *out_len);
int lz4ada_stream_index_opt(const uint8_t *input, int64_t len, uint32_t flags,
                            lz4ada_stream_entry *entries, int64_t cap, int64_t *nframes);
/* The slot bytes (sum of the block slots, each rounded up to 256) up to which
 * a linked frame shares a pass: the built-in default, or
 * LZ4ADA_BATCH_LINKED_MAX, read per call. */
int64_t lz4ada_batch_linked_max(void);
/* Test-only, like lz4ada_index_table_debug: k_index + k_decode_idx_frames alone
 * over nframes block ranges first[0..nframes] (host array, nframes + 1 rising
 * entries) of d_descs; linked[i] != 0 marks the frames to walk, and the blocks
 * of the others see no launch.  d_status gets a code per block of a marked
 * frame: 0 with out_len, or non-zero from the block that ended the frame's
 * chain on.  Returns after the stream has drained. */
int lz4ada_decode_idx_frames_debug(const void *d_frame, uint64_t frame_len,
                                   const lz4ada_block_desc *d_descs, int64_t nblocks,
                                   const int64_t *first, const uint8_t *linked, int64_t nframes,
                                   void *d_out, lz4ada_block_status *d_status, void *stream);

/* ------------------------- many frames, device memory to device memory */
/*
 * The same pass for frames that already lie in device memory (read there by
 * another library, received over RCCL, produced by a kernel) and whose
 * plaintext is wanted there: the frames are indexed where they lie (one GPU
 * lane walks one frame's header and size words), the decoders read d_in
 * itself, and the compaction writes into d_out.  The
 * host sees per-frame records only -- verdicts, sizes, checksums -- with one
 * exception: a content checksum over more than lz4ada_batch_hash_max()
 * decoded bytes is hashed by the host chain (lz4ada_content_xxh32_d2h), so
 * those bytes visit the host to be hashed, and go nowhere else.
 *
 * jobs is a host array, in any order; the engine works in rising in_off.  A
 * job's range is the frame and whatever follows it (Single_Frame semantics),
 * so it may run on to the end of d_in.  API misuse, LZ4ADA_ASSERTION_ERROR
 * with nothing launched: a range outside [0, in_len), or two ranges that
 * share bytes unless the earlier one ends with d_in.  An accepted frame that
 * reaches into the next job's range is the same misuse, found after the
 * index kernel alone has run.
 *
 * A frame the pass does not find good in every respect gets status
 * LZ4ADA_EXACT_PATH, a reason, and out_len = consumed = 0; no exception text
 * is invented: lz4ada_decode_frame / _partial on the frame's host bytes give
 * the reference's result.  A skippable frame is LZ4ADA_OK with out_len 0.
 * Both calls return LZ4ADA_OK when the call itself worked, whatever the
 * per-job statuses.  lz4ada_last_batch_stats() counts the frames committed
 * (frames_batched), the passes and the checksums; lz4ada_last_path() is
 * LZ4ADA_PATH_BATCH | LZ4ADA_PATH_INDEPENDENT.  Host synchronisations on
 * `stream`: one for the index (per call) and one per pass.
 */
#define LZ4ADA_DEVFRAME_OK 0
/* 1..4 keep the LZ4ADA_BATCH_* meanings (LINKED, BIG_BLOCK, OVER_BUDGET, NOT_INDEXED) */
#define LZ4ADA_DEVFRAME_BLOCK 5     /* a block failed: status, slot overflow, block checksum */
#define LZ4ADA_DEVFRAME_SIZE 6      /* decoded length != declared content size */
#define LZ4ADA_DEVFRAME_CHECKSUM 7  /* content checksum mismatch */

typedef struct {
	int64_t in_off, in_len;   /* in: the frame, and whatever follows it, inside d_in */
	int64_t out_off, out_len; /* out: its bytes inside d_out (out_len 0 unless status is OK) */
	int64_t consumed;         /* out: bytes of the frame (0 unless OK) */
	int32_t status;           /* out: LZ4ADA_OK, or LZ4ADA_EXACT_PATH: not decoded here */
	int32_t reason;           /* out: LZ4ADA_DEVFRAME_* */
} lz4ada_device_frame_job;

/* Index njobs frames on the device and return an out_cap that always suffices
 * (sum of slot caps of the frames the pass takes).  Every job gets the index's
 * verdict (status, reason 0..4).  Synchronous on stream (a hipStream_t). */
int lz4ada_frames_device_bound(const void *d_in, int64_t in_len,
                               lz4ada_device_frame_job *jobs, int64_t njobs,
                               int64_t *bound, void *stream);
/* Decode.  No payload byte crosses to the host.  The frames' bytes lie in
 * d_out in rising in_off, back to back within a pass; bytes between reported
 * spans are unspecified (a failed frame's blocks), bytes at and beyond
 * *out_len are not written.  out_cap below the bound: LZ4ADA_TOO_LITTLE_MEMORY,
 * *out_len = the bound, d_out untouched.  Synchronous on stream. */
int lz4ada_decode_frames_device(const void *d_in, int64_t in_len,
                                lz4ada_device_frame_job *jobs, int64_t njobs,
                                void *d_out, int64_t out_cap, int64_t *out_len, void *stream);
/* The two calls with flags (LZ4ADA_FRAMES_LINKED, above): the walk then accepts
 * linked frames up to lz4ada_batch_linked_max(); lz4ada_last_path() gains
 * LZ4ADA_PATH_LINKED when a linked frame was committed. */
int lz4ada_frames_device_bound_opt(const void *d_in, int64_t in_len,
                                   lz4ada_device_frame_job *jobs, int64_t njobs, uint32_t flags,
                                   int64_t *bound, void *stream);
int lz4ada_decode_frames_device_opt(const void *d_in, int64_t in_len,
                                    lz4ada_device_frame_job *jobs, int64_t njobs, uint32_t flags,
                                    void *d_out, int64_t out_cap, int64_t *out_len, void *stream);

/* ------------------------------ exact decoded sizes, and a decode that fits */
/*
 * The bound above counts every block at its slot capacity: 255 times its
 * payload, or the frame's block maximum.  The exact sizes cost one parse and
 * no output traffic: pass 1 of the index decoder
 * records the output bytes of every 32 payload bytes, a kernel adds them up
 * per block (k_block_sizes; a block pass 1 declines is walked by the wave,
 * a stored one is its payload), another per frame (k_frame_sizes).  One more
 * host synchronisation on `stream` per call: the per-frame size records.
 *
 * lz4ada_frames_device_sizes: per job status and reason as
 * lz4ada_frames_device_bound_opt gives them, and also LZ4ADA_EXACT_PATH with
 * LZ4ADA_DEVFRAME_BLOCK (a block's sequence chain is malformed, a block
 * decodes to more than its slot capacity, a linked frame's middle block is
 * short) or LZ4ADA_DEVFRAME_SIZE (the sizes do not add up to the declared
 * content size).  out_len is the exact decoded length of an accepted frame
 * (0 for a skippable one); out_off and consumed are 0.  *total is their sum:
 * an out_cap that suffices for the decode with LZ4ADA_FRAMES_EXACT, and its
 * *out_len when every frame is committed.  A size is a statement about the
 * sequence chain alone: a frame whose offsets or checksums are bad has a size
 * here and fails in the decode.  flags: LZ4ADA_FRAMES_LINKED as elsewhere.
 *
 * LZ4ADA_FRAMES_EXACT in the flags of lz4ada_decode_frames_device_opt: the
 * same stage runs first; out_cap below *total is LZ4ADA_TOO_LITTLE_MEMORY with
 * *out_len = the total and d_out untouched; a frame the stage fails is
 * rejected with its reason and takes no slot; the passes are split and the
 * library's scratch is sized by the slots the sizes need (each block's size
 * rounded up to 256), not by the capacities.  Results are those of the call
 * without the flag.  (A frame whose capacities alone exceed LZ4ADA_BATCH_BYTES
 * keeps LZ4ADA_BATCH_OVER_BUDGET: the walk judges that before any size is
 * known.)
 */
#define LZ4ADA_FRAMES_EXACT 2u /* flags: lay the passes out by the exact sizes */
int lz4ada_frames_device_sizes(const void *d_in, int64_t in_len,
                               lz4ada_device_frame_job *jobs, int64_t njobs, uint32_t flags,
                               int64_t *total, void *stream);

/* Test-only, in the spirit of lz4ada_index_table_debug. */
/* The size rule on the host (block_decoded_size, the serial statement that
 * k_block_sizes is tested against): the decoded length of the block payload
 * at block[0 .. n), stored or compressed, or -1 when its sequence chain is
 * one Decompress_Full_Block (lz4ada.adb:716-788) raises on; offsets are not
 * judged.  Host only, no HIP call. */
int64_t lz4ada_block_size_host(const uint8_t *block, int64_t n, int stored);
/* The walk on the host: verdict as return value (LZ4ADA_DEVFRAME_* 0..4), info
 * and descs as lz4ada_frame_index lays them out (descs may be NULL; at most
 * desc_cap are written, info->nblocks counts them all).  info is complete
 * unless the verdict is NOT_INDEXED.  Host only, no HIP call. */
int lz4ada_frame_walk_host(const uint8_t *frame, int64_t len, lz4ada_frame_info *info,
                           lz4ada_block_desc *descs, int64_t desc_cap);
/* The same with flags (LZ4ADA_FRAMES_LINKED and its cap); flags 0 is the call above. */
int lz4ada_frame_walk_host_opt(const uint8_t *frame, int64_t len, uint32_t flags,
                               lz4ada_frame_info *info, lz4ada_block_desc *descs,
                               int64_t desc_cap);
/* k_frames_walk + scan + k_frames_fill alone: per job the verdict and nblocks
 * (0 for a frame that does not index), and the descriptors of all accepted
 * frames in pass order (rising in_off), copied to the host: in_off absolute in
 * d_in, out_off the slot layout (steps of slot capacity rounded up to 256),
 * out_cap the slot capacity. */
int lz4ada_frames_index_device_debug(const void *d_in, int64_t in_len,
                                     const lz4ada_device_frame_job *jobs, int64_t njobs,
                                     int32_t *verdict, int64_t *nblocks,
                                     lz4ada_block_desc *descs, int64_t desc_cap, void *stream);

/* ------------------------------- device-resident frames with a dictionary */
/*
 * Small frames are what LZ4F dictionaries exist for: a 2 KiB record that
 * compresses badly alone compresses well against a shared 64 KiB dictionary
 * (LZ4F_compressFrame_usingCDict).  The two calls below are
 * lz4ada_frames_device_bound_opt / lz4ada_decode_frames_device_opt with one
 * dictionary, in device memory, shared by every frame of the call (DESIGN.md
 * section 15).  Semantics are the LZ4 frame specification's
 * (LZ4F_decompress_usingDict), not the reference's: the reference knows no
 * dictionary and raises "Backreference location out of range" on such a
 * frame, so these calls have no reference twin and replay none of its quirks
 * (quirk D1 has no meaning where the reference cannot decode the frame at
 * all: a match it would concern reads plain history).
 *
 * The last min(dict_len, 65536) bytes of the dictionary precede the first
 * block of a linked modern frame and every block of an independent one;
 * legacy blocks read no dictionary.  flags (LZ4ADA_FRAMES_LINKED,
 * LZ4ADA_FRAMES_EXACT), job semantics, ordering, bounds, the
 * LZ4ADA_TOO_LITTLE_MEMORY rule, lz4ada_last_batch_stats(), lz4ada_last_path()
 * and the host synchronisations are those of the _opt calls (one more per call
 * with LZ4ADA_DICT_CHECK_ID); the bound and out_cap count decoded bytes only,
 * the room for the dictionary in front of the slots is the library's scratch
 * and is charged against LZ4ADA_BATCH_BYTES when the passes are split.  A
 * frame that never reads the dictionary decodes to the bytes the _opt call
 * gives.  dict == NULL or dict_len == 0 is the _opt call itself, launch by
 * launch.  API misuse, LZ4ADA_ASSERTION_ERROR before any launch: dict_len < 0,
 * d_dict == NULL with dict_len > 0, unknown bits in dict->flags.
 *
 * With LZ4ADA_DICT_CHECK_ID a modern frame whose header carries a dictionary
 * id (FLG bit 0) other than dict_id gets LZ4ADA_EXACT_PATH /
 * LZ4ADA_DEVFRAME_DICT from the index stage, in both calls, and takes no slot;
 * a frame without an id is accepted, as LZ4F allows.  Without the flag no id
 * is looked at.
 *
 * A frame the pass does not find good gets LZ4ADA_EXACT_PATH and a reason, as
 * in the _opt call.  The blocks of a dictionary call go through the index
 * decoder alone (its fallback decoders know no history), so a block its first
 * pass declines -- a block maximum over 256 KiB, or a literal-heavy payload --
 * fails its frame with LZ4ADA_DEVFRAME_BLOCK, as does a match that reaches
 * further back than the dictionary's first used byte.  One caution of the
 * shared block decoder remains: where 2 KiB of a block's payload decode to
 * more than 4,080 bytes, a match that starts before the block with an offset
 * of 65,529 or more fails the frame the same way (elsewhere such a match is
 * decoded).  The caller's way for such a frame is
 * lz4ada_decode_frame_dict_host on its host bytes.
 */
#define LZ4ADA_DEVFRAME_DICT 8 /* the frame names another dictionary id */
#define LZ4ADA_DICT_CHECK_ID 1u
typedef struct {
	const void *d_dict; /* device memory */
	int64_t dict_len;   /* any length >= 0; the last 65,536 bytes are used */
	uint32_t dict_id;   /* compared only with LZ4ADA_DICT_CHECK_ID */
	uint32_t flags;     /* LZ4ADA_DICT_* */
} lz4ada_device_dict;
int lz4ada_frames_device_bound_dict(const void *d_in, int64_t in_len,
                                    lz4ada_device_frame_job *jobs, int64_t njobs, uint32_t flags,
                                    const lz4ada_device_dict *dict, int64_t *bound, void *stream);
int lz4ada_decode_frames_device_dict(const void *d_in, int64_t in_len,
                                     lz4ada_device_frame_job *jobs, int64_t njobs, uint32_t flags,
                                     const lz4ada_device_dict *dict, void *d_out, int64_t out_cap,
                                     int64_t *out_len, void *stream);
/* One modern frame (linked or independent, stored blocks included) decoded
 * against a dictionary on the host: plain serial code, no HIP call, the LZ4
 * specification's semantics as above.  It verifies block checksums, the
 * content size and the content checksum, and compares no dictionary id.
 * LZ4ADA_DATA_CORRUPTION (a malformed or truncated frame, a match reaching
 * before the dictionary's first used byte, a wrong content size),
 * LZ4ADA_CHECKSUM_ERROR, LZ4ADA_TOO_LITTLE_MEMORY (out_cap is too small),
 * LZ4ADA_NOT_SUPPORTED (a legacy or skippable frame, unknown header bits); the
 * message, this library's own, is in lz4ada_thread_last_error().  dict may be
 * NULL with dict_len 0.  *out_len and *frame_consumed are 0 unless LZ4ADA_OK. */
int lz4ada_decode_frame_dict_host(const uint8_t *frame, int64_t len, const uint8_t *dict,
                                  int64_t dict_len, uint8_t *out, int64_t out_cap, int64_t *out_len,
                                  int64_t *frame_consumed);

/* --------------------- seek index and ranged decode of device-resident frames */
/*
 * The exact sizes above are one prefix sum away from a seek table.  A seek
 * index keeps, for a set of frames lying in device memory, every accepted
 * frame's block descriptors and the decoded offset at which each block starts
 * (DESIGN.md section 14): 48 bytes of device memory per block, which the index
 * owns -- it is not the per-thread scratch and survives
 * lz4ada_release_device_cache().  A ranged decode then takes many byte ranges
 * of the *decoded* frames in one call, decodes only the blocks those ranges
 * touch, and lays the requested bytes back to back in the caller's device
 * buffer.  There is no reference twin: like lz4ada_decode_frames_device it
 * replaces a loop the caller would otherwise write.
 *
 * lz4ada_seek_index_build: the index and sizes stages over jobs, as
 * lz4ada_frames_device_sizes runs them -- every job gets the same status,
 * reason and out_len = exact decoded size -- and then the table is kept.
 * flags must be 0: a linked frame is refused with LZ4ADA_BATCH_LINKED, since a
 * block of a linked frame needs the output before it (lz4ada_seek_index_build_opt
 * below takes them, with history checkpoints).  njobs == 0 builds an
 * empty index without a device call.  On failure *idx is NULL.  Synchronous
 * on stream; host synchronisations: the two of lz4ada_frames_device_sizes and
 * one that ends the build, after which the index never changes.  Any number of
 * threads may then run ranged calls on it at once, each in its own thread's
 * scratch.  lz4ada_seek_index_free(NULL) is a no-op;
 * lz4ada_seek_index_bytes is the device memory held (no HIP call).
 *
 * lz4ada_decode_ranges_device.  d_in / in_len must be the input the index was
 * built over: another in_len is LZ4ADA_ASSERTION_ERROR; the pointer may differ
 * (descriptors are relative to d_in).  If the bytes changed since the build,
 * blocks fail or decode to other bytes; nothing is read outside
 * [d_in, d_in + in_len) and nothing written outside the library's scratch and
 * the ranges' own bytes, since every bound comes from the index and in_len.
 *  - A range is clipped to its frame: want = max(0, min(off + len, size) - off).
 *    off at or past the end, len == 0, a skippable frame and an empty frame
 *    give LZ4ADA_OK with out_len == 0.
 *  - The ranges' bytes lie in d_out back to back in the order of the ranges
 *    array: out_off of range i is the sum of want over the ranges before it.
 *    Ranges may overlap, repeat and come in any order of job and offset.
 *    *out_len is the sum of all want.  out_cap below it is
 *    LZ4ADA_TOO_LITTLE_MEMORY with *out_len = that sum and d_out untouched, so
 *    out_cap = 0 is how a caller learns the clipped total.  Nothing at or
 *    beyond *out_len is ever written.
 *  - A range of a frame the index did not accept: LZ4ADA_EXACT_PATH, the
 *    frame's reason, out_len 0; it takes no room.
 *  - A range one of whose touched blocks fails -- a non-zero decode status (a
 *    match that reaches before the block start included), a decoded length
 *    unequal to its indexed size, a declared block checksum unequal to the
 *    computed one: LZ4ADA_EXACT_PATH / LZ4ADA_DEVFRAME_BLOCK with out_len 0.
 *    The range keeps its place: the want bytes at out_off are unspecified and
 *    nothing outside them is touched.  A failing block costs only the ranges
 *    that touch it.  A block is touched when it shares a byte with the clipped
 *    range; an empty block between two touched ones rides along.
 *  - A single range whose blocks' slots (their sizes rounded up to 256) exceed
 *    LZ4ADA_BATCH_BYTES: LZ4ADA_EXACT_PATH / LZ4ADA_BATCH_OVER_BUDGET, likewise
 *    in place.
 *  - What a delivered range asserts: the whole frame's header and size words
 *    indexed; every block's sequence chain adds up, and to the declared
 *    content size if there is one (the sizes stage); the touched blocks
 *    decoded and their block checksums hold.  It does NOT assert the content
 *    checksum, nor the offsets and block checksums of blocks it did not touch.
 *    So a frame that lz4ada_decode_frames_device rejects with
 *    LZ4ADA_DEVFRAME_CHECKSUM, or whose corrupt block lies outside the range,
 *    still serves the range.  That is the point of random access.
 *  - API misuse, LZ4ADA_ASSERTION_ERROR before any device call: NULL idx,
 *    ranges, out_len or d_in; a job outside [0, njobs); a negative off or len;
 *    off + len overflowing; nranges < 0; and flags != 0 in the build.
 *    nranges == 0 is a call that worked and launches nothing.
 *  - Synchronous on stream.  Host synchronisations: one for the selection
 *    records and one per pass; a call whose ranges are all empty makes none.
 *    lz4ada_last_batch_stats().passes counts the passes (the other counters
 *    stay 0); lz4ada_last_path() is LZ4ADA_PATH_BATCH | LZ4ADA_PATH_INDEPENDENT
 *    when a range was delivered through a pass.
 */
typedef struct lz4ada_seek_index lz4ada_seek_index;

int lz4ada_seek_index_build(const void *d_in, int64_t in_len,
                            lz4ada_device_frame_job *jobs, int64_t njobs, uint32_t flags,
                            lz4ada_seek_index **idx, void *stream);
void lz4ada_seek_index_free(lz4ada_seek_index *idx);
int64_t lz4ada_seek_index_bytes(const lz4ada_seek_index *idx);

/*
 * Linked frames in the seek index, through history checkpoints (DESIGN.md
 * section 16).  lz4ada_seek_index_build_opt with opt == NULL or opt->flags == 0
 * is lz4ada_seek_index_build(..., 0, ...) launch by launch.  With
 * LZ4ADA_SEEK_LINKED the index stage runs as the many-frame pass does with
 * LZ4ADA_FRAMES_LINKED: a linked modern frame of at most
 * lz4ada_batch_linked_max() slot bytes is taken (above it: LZ4ADA_BATCH_LINKED,
 * as before), and the build decodes every such frame once, in passes under
 * LZ4ADA_BATCH_BYTES into the calling thread's scratch (one more host
 * synchronisation per pass; lz4ada_last_batch_stats().passes counts them).  A
 * frame whose chain fails there -- a declined block, a bad block checksum,
 * quirk D1's round state -- gets LZ4ADA_EXACT_PATH / LZ4ADA_DEVFRAME_BLOCK and
 * out_len 0 in the job report and for every later range.  The content checksum
 * is not asserted.
 *
 * Checkpoints: per linked frame K = max(1, ceil(checkpoint_bytes / block_max))
 * blocks form a group (checkpoint_bytes == 0: 1 MiB), and for every group start
 * b = K, 2K, ... < nblocks the index keeps the 65,536 decoded bytes in front of
 * block b.  lz4ada_seek_index_bytes, exactly, with nb the blocks of the accepted
 * frames and n the jobs:
 *     32 * nb + 8 * (n + 1) + 16 * (nb + n)                  any index with n > 0
 *   + 65536 * C + 8 * (n + 1) + 8 * n                        LZ4ADA_SEEK_LINKED, n > 0
 * where C is the sum of (nblocks - 1) / K (integer division) over the linked
 * frames with blocks that the sizes stage accepted (a frame whose chain then
 * fails at the build keeps its share of the store).
 *
 * A range of a linked frame decodes its chain: the blocks from the start of
 * the group of its first touched block to its last touched block, every group
 * in a wave of its own from its checkpoint, so the cost of a range no longer
 * grows with its distance from the frame's start.  Everything
 * lz4ada_decode_ranges_device says above holds, with these additions:
 *  - the range fails with LZ4ADA_DEVFRAME_BLOCK when any block of its chain
 *    fails, touched or not;
 *  - a range whose chain's slots and gaps (65,792 bytes in front of every
 *    group start but block 0) exceed LZ4ADA_BATCH_BYTES is
 *    LZ4ADA_BATCH_OVER_BUDGET in place;
 *  - a delivered range asserts its chain's blocks (decoded, block checksums)
 *    and, at the build, the whole frame's; the bytes are the reference's,
 *    since the build refused quirk D1's round state;
 *  - if the input changed since the build, a group whose own blocks are
 *    unchanged still delivers what the build saw: its history is the
 *    checkpoint;
 *  - lz4ada_last_path() carries LZ4ADA_PATH_LINKED when a linked range was
 *    delivered.
 * Misuse, LZ4ADA_ASSERTION_ERROR before any device call with *idx = NULL:
 * unknown bits in opt->flags, opt->reserved != 0, opt->checkpoint_bytes < 0,
 * and everything lz4ada_seek_index_build calls misuse.
 */
#define LZ4ADA_SEEK_LINKED 1u /* opt->flags: take linked frames, with checkpoints */
typedef struct {
	uint32_t flags;           /* LZ4ADA_SEEK_* */
	uint32_t reserved;        /* must be 0 */
	int64_t checkpoint_bytes; /* decoded bytes between checkpoints; 0: the default */
} lz4ada_seek_options;
int lz4ada_seek_index_build_opt(const void *d_in, int64_t in_len,
                                lz4ada_device_frame_job *jobs, int64_t njobs,
                                const lz4ada_seek_options *opt,
                                lz4ada_seek_index **idx, void *stream);

/*
 * Dictionary frames in the seek index: the small
 * records a dictionary exists for are the ones a caller fetches by position.
 * lz4ada_seek_index_build_dict is lz4ada_seek_index_build_opt with one
 * dictionary, as lz4ada_decode_frames_device_dict takes it, shared by every
 * frame of the index.  dict == NULL or dict_len == 0 is
 * lz4ada_seek_index_build_opt itself, launch by launch, and the index runs every
 * ranged call as before.  lz4ada_decode_ranges_device keeps its signature and
 * takes no dictionary:
 *
 * The index owns its dictionary.  The build copies the last dict_used =
 * min(dict_len, 65536) bytes into device memory of its own, laid out as the gap
 * a pass puts in front of a block: G = round256(dict_used + 32) bytes, G -
 * dict_used zeros and then the bytes.  The caller may free or overwrite d_dict
 * once the build returns; a ranged call cannot be handed another dictionary.
 * lz4ada_seek_index_bytes, exactly, adds to the two lines above
 *   + G + 8 * n                                   a dictionary, n > 0
 * (8 per job: which of the frame's blocks read the dictionary); an index over
 * n == 0 jobs holds nothing and makes no device call.
 *
 * Semantics are those of lz4ada_decode_frames_device_dict, the LZ4 frame
 * specification's: the dictionary precedes every block of an independent modern
 * frame and block 0 of a linked one (LZ4ADA_SEEK_LINKED; the build decodes each
 * linked frame once against the dictionary, the gap charged to the pass, and
 * saves the checkpoints as before); legacy blocks read none and decode as in
 * any index.  No quirk-D1 round state, at the build or in the ranges.  A match
 * that reaches further back than dict_used bytes before such a block fails its
 * range with LZ4ADA_DEVFRAME_BLOCK: a short dictionary is never padded.
 * With LZ4ADA_DICT_CHECK_ID in dict->flags a frame naming another id gets
 * LZ4ADA_EXACT_PATH / LZ4ADA_DEVFRAME_DICT in the job report, and so does every
 * later range of it; it holds no block in the index.
 *
 * Ranges: everything lz4ada_decode_ranges_device says above holds, with these
 * additions:
 *  - the modern blocks of a dictionary index go through the index decoder
 *    alone, one wave per chain (an independent frame's block is a chain of
 *    one), since the fallback decoders know no history: a block whose first
 *    pass declines it -- a block maximum over 256 KiB, or a literal-heavy
 *    payload of 64 KiB or more -- fails its ranges with LZ4ADA_DEVFRAME_BLOCK.
 *    The shared block decoder's one caution stands as in section 15: where
 *    2 KiB of a block's payload decode to more than 4,080 bytes, a match that
 *    starts before the block with an offset of 65,529 or more fails the range
 *    the same way;
 *  - every marked block that reads the dictionary has G bytes in front of its
 *    slot, charged against LZ4ADA_BATCH_BYTES like a head's 65,792: a range
 *    whose slots and gaps alone exceed the budget is LZ4ADA_BATCH_OVER_BUDGET
 *    in place;
 *  - a delivered range asserts what it did before, decoded against the
 *    dictionary the index was built with.
 * Misuse, LZ4ADA_ASSERTION_ERROR before any device call with *idx = NULL: what
 * lz4ada_seek_index_build_opt rejects, dict_len < 0, d_dict == NULL with
 * dict_len > 0, unknown bits in dict->flags.
 */
int lz4ada_seek_index_build_dict(const void *d_in, int64_t in_len,
                                 lz4ada_device_frame_job *jobs, int64_t njobs,
                                 const lz4ada_seek_options *opt,
                                 const lz4ada_device_dict *dict,
                                 lz4ada_seek_index **idx, void *stream);

typedef struct {
	int64_t job;             /* in: which of the njobs frames the index was built over */
	int64_t off, len;         /* in: decoded bytes [off, off + len) of that frame */
	int64_t out_off, out_len; /* out: where its bytes lie in d_out, and how many */
	int32_t status;           /* out: LZ4ADA_OK, or LZ4ADA_EXACT_PATH: not delivered */
	int32_t reason;           /* out: LZ4ADA_DEVFRAME_* */
} lz4ada_frame_range;

int lz4ada_decode_ranges_device(const lz4ada_seek_index *idx, const void *d_in, int64_t in_len,
                                lz4ada_frame_range *ranges, int64_t nranges,
                                void *d_out, int64_t out_cap, int64_t *out_len, void *stream);

/* Test-only, as above. */
/* The block search on the host (range_blocks, lz4ada_range_blocks.h, the
 * statement k_ranges_select runs), for n ranges of one frame: start[0 ..
 * nblocks] is the frame's exclusive prefix sum of block sizes and its size.
 * first[i] / count[i]: the blocks the clipped range i touches (count 0: none);
 * want[i]: its clipped length.  LZ4ADA_ASSERTION_ERROR on a NULL or negative
 * argument.  Host only, no HIP call. */
int lz4ada_range_blocks_host(const uint64_t *start, int64_t nblocks, const int64_t *off,
                             const int64_t *len, int64_t n, int64_t *first, int64_t *count,
                             int64_t *want);
/* The chain rule on the host (lz4ada_range_chains.h, the statement the ranged
 * decode's kernels and its host sweep run), for one linked frame of nblocks
 * blocks in groups of `group` (0: independent blocks) and the touched
 * intervals [first[i], first[i] + count[i]) of n ranges (count 0: none):
 * marked[b] / head[b] (nblocks bytes each, 0 or 1) and the chains in rising
 * order as chain_first / chain_count (room for nblocks), *nchains of them.
 * LZ4ADA_ASSERTION_ERROR on a NULL or out-of-range argument.  Host only, no
 * HIP call. */
int lz4ada_range_chains_host(int64_t nblocks, int64_t group, const int64_t *first,
                             const int64_t *count, int64_t n, uint8_t *marked, uint8_t *head,
                             int64_t *chain_first, int64_t *chain_count, int64_t *nchains);
/* The gap count of an interval on the host (lz4ada_range_chains.h, what the
 * ranged decode charges and lays out): among the blocks [lo, hi) of a frame of
 * nblocks blocks in groups of `group`, *heads = those decoded from a checkpoint
 * (65,792 bytes in front of each) and *dict_gaps = those that read the
 * dictionary of a dictionary index, by the frame's kind (0: none of them -- a
 * legacy frame, or no dictionary; 1: a linked frame, block 0; 2: an independent
 * modern frame, every block).  LZ4ADA_ASSERTION_ERROR on a NULL or out-of-range
 * argument.  Host only, no HIP call. */
int lz4ada_range_gaps_host(int64_t nblocks, int64_t group, int32_t kind, int64_t lo, int64_t hi,
                           int64_t *heads, int64_t *dict_gaps);
/* Like lz4ada_decode_idx_frames_debug: k_index + k_decode_idx_chains alone, the
 * chain decoder of a ranged pass over a dictionary index.  descs: nblocks
 * descriptors (host array) laid out as such a pass lays them; chain i holds the
 * blocks [first[i], first[i] + count[i]) (rising, disjoint) and starts with
 * hist[i] bytes of history, which the caller has put in front of its first
 * block's slot in d_out; gapped[i] != 0 marks that block as having such a gap.
 * d_status (device, zeroed by the caller) gets a code per block of a chain: 0
 * with out_len, or non-zero from the block that ended the chain on; the blocks
 * of a chain whose first block is not gapped, or lies less than
 * round256(min(hist, 65536) + 32) bytes into d_out, get a non-zero code and
 * nothing of theirs is written.  Returns after the stream has drained. */
int lz4ada_decode_idx_chains_debug(const void *d_frame, uint64_t frame_len,
                                   const lz4ada_block_desc *descs, int64_t nblocks,
                                   const int64_t *first, const int64_t *count, const uint32_t *hist,
                                   const uint8_t *gapped, int64_t nchains, void *d_out,
                                   lz4ada_block_status *d_status, void *stream);
/* One job of an index: its reason (0: accepted), its block count, and, when
 * start is not NULL, its start[0 .. nblocks] copied to the host (start_cap
 * entries of room). */
int lz4ada_seek_index_debug(const lz4ada_seek_index *idx, int64_t job, int32_t *reason,
                            int64_t *nblocks, uint64_t *start, int64_t start_cap, void *stream);
/* k_ranges_select and the marks of one pass over all the ranges, nothing
 * decoded: per range its first touched block and their count (frame-relative;
 * 0, 0 for an empty range), and *marked: the blocks a pass would decode once
 * shared ones count once (in a linked frame the chains' blocks, section 16).  ranges gets out_off, out_len, status and reason as the index
 * alone gives them. */
int lz4ada_ranges_select_debug(const lz4ada_seek_index *idx, lz4ada_frame_range *ranges,
                               int64_t nranges, int64_t *first, int64_t *count, int64_t *marked,
                               void *stream);

/* ------------------------ records compressed into frames, device to device */
/*
 * The write side of the device calls above: every job's
 * record, in_len bytes at d_in + in_off, becomes one LZ4 frame (format 1.6.x,
 * version 01, independent blocks, no dictionary id) and the frames are laid
 * back to back into d_out in job order, the first at d_out: a job's out_off /
 * out_len say where its frame lies, *out_len is their sum, and nothing at or
 * beyond d_out + *out_len is written.  Jobs may overlap in d_in and come in any
 * order of in_off; in_len may be 0 (header, end mark and, if asked for, the
 * checksum).  opt == NULL is {0, 0}.  opt->block_id: the frame's block maximum,
 * 4..7 = 64 KiB, 256 KiB, 1 MiB, 4 MiB; 0 means 4.  One wave compresses one
 * block, so a 4 MiB block is one wave's serial work and 64 KiB is the default.
 * opt->flags: LZ4ADA_COMP_BLOCK_CHECKSUM (XXH32 of every block's payload as
 * written), LZ4ADA_COMP_CONTENT_CHECKSUM (XXH32 of the record after the end
 * mark), LZ4ADA_COMP_CONTENT_SIZE (the 8-byte content size in the header).  A
 * block is stored (size word bit 31) whenever its compressed form is not
 * shorter than the block; stored_blocks counts a job's.
 *
 * The bound, exact worst-case arithmetic (every block stored): per frame
 *   7 + (CONTENT_SIZE ? 8 : 0)
 *   + nblocks * (4 + (BLOCK_CHECKSUM ? 4 : 0)) + in_len
 *   + 4 + (CONTENT_CHECKSUM ? 4 : 0),      nblocks = ceil(in_len / block_len),
 * and lz4ada_compress_frames_bound is its sum over the jobs (host only, no HIP
 * call; -1 on the misuse below).  out_cap below the bound:
 * LZ4ADA_TOO_LITTLE_MEMORY with *out_len set to the bound and d_out untouched.
 * API misuse, LZ4ADA_ASSERTION_ERROR before any launch: a NULL jobs / d_in /
 * d_out / out_len where one is needed, a range outside [0, in_len), a block_id
 * outside {0, 4..7}, unknown flag bits.  No GPU: LZ4ADA_DEVICE_ERROR.
 *
 * The host synchronises `stream` once per call for the per-job results (once
 * per pass when the blocks' scratch slots exceed LZ4ADA_BATCH_BYTES and the
 * jobs are cut into passes).  No payload byte crosses to the host, except that
 * a content checksum over more than lz4ada_batch_hash_max() bytes is hashed by
 * the host chain (lz4ada_content_xxh32_d2h with no host destination), which
 * costs a synchronisation more.
 *
 * Every LZ4F decoder reads the frames: this library's calls without any flag,
 * liblz4.  The compressor is its own (no reference twin, as with dictionaries):
 * lz4ada_compress_block_host states the matching rule serially and the kernel
 * produces the same bytes, so lz4ada_compress_frame_host(record) is bytewise
 * what the device call writes for that job.
 */
#define LZ4ADA_COMP_BLOCK_CHECKSUM   1u
#define LZ4ADA_COMP_CONTENT_CHECKSUM 2u
#define LZ4ADA_COMP_CONTENT_SIZE     4u
typedef struct {
	uint32_t block_id; /* 4..7 = 64 KiB..4 MiB; 0 means 4 */
	uint32_t flags;    /* LZ4ADA_COMP_* */
} lz4ada_compress_options;
typedef struct {
	int64_t in_off, in_len;   /* in: the record inside d_in (in_len may be 0) */
	int64_t out_off, out_len; /* out: its frame inside d_out */
	int32_t status;           /* out */
	int32_t stored_blocks;    /* out: blocks written uncompressed */
} lz4ada_compress_job;
int64_t lz4ada_compress_frames_bound(const lz4ada_compress_job *jobs, int64_t njobs,
                                     const lz4ada_compress_options *opt);
int lz4ada_compress_frames_device(const void *d_in, int64_t in_len, lz4ada_compress_job *jobs,
                                  int64_t njobs, const lz4ada_compress_options *opt, void *d_out,
                                  int64_t out_cap, int64_t *out_len, void *stream);
/* The serial statement of the block compressor: src[0 .. n) as one LZ4 block
 * into dst[0 .. cap) -> its length, 0 when it does not fit into cap bytes
 * (nothing beyond dst + cap is written), -1 on a NULL pointer, a negative
 * length or n over 0x7E000000.  Host only, no HIP call. */
int64_t lz4ada_compress_block_host(const uint8_t *src, int64_t n, uint8_t *dst, int64_t cap);
/* One record as one frame, as the device call writes it -> the frame's length;
 * -LZ4ADA_TOO_LITTLE_MEMORY when cap is below the bound above (dst untouched),
 * -LZ4ADA_ASSERTION_ERROR on the misuse above.  Host only, no HIP call. */
int64_t lz4ada_compress_frame_host(const uint8_t *src, int64_t n, const lz4ada_compress_options *opt,
                                   uint8_t *dst, int64_t cap);

/* -------------- records compressed against a shared dictionary, on the device */
/*
 * The write side of lz4ada_decode_frames_device_dict:
 * lz4ada_compress_frames_device with one dictionary, in device memory, shared
 * by every frame of the call, as LZ4F_compressFrame_usingCDict shares one.
 * The last min(dict_len, 65536) bytes of the dictionary lie in front of every
 * block of every record (the blocks are independent, so each starts from the
 * dictionary afresh), and a block's matches may begin there.  The frames
 * decode through lz4ada_decode_frames_device_dict,
 * lz4ada_decode_frame_dict_host and liblz4's LZ4F_decompress_usingDict with
 * the same dictionary; a decoder without it rejects or garbles them.
 *
 * dict->flags: with LZ4ADA_COMP_DICT_WRITE_ID every header carries FLG bit 0
 * and dict_id, 4 bytes after the content size and before HC (which covers
 * them), and the bound grows by 4 per frame; without it dict_id is ignored and
 * the header is the plain call's.  lz4ada_compress_frames_bound_dict reads
 * dict->flags alone (host only, no HIP call; d_dict is not dereferenced; -1 on
 * misuse).  opt is the plain call's and rejects what it rejects there.
 * dict == NULL, or dict_len == 0 without LZ4ADA_COMP_DICT_WRITE_ID, is
 * lz4ada_compress_frames_device itself, launch by launch.  API misuse,
 * LZ4ADA_ASSERTION_ERROR before any launch: the plain call's, dict_len < 0,
 * d_dict == NULL with dict_len > 0, unknown bits in dict->flags.  The rest of
 * the contract is the plain call's: LZ4ADA_TOO_LITTLE_MEMORY below the bound
 * with *out_len set to it and d_out untouched, dense frames in job order,
 * nothing written at or beyond d_out + *out_len, one host synchronisation per
 * pass.  The dictionary's hash table (16 KiB, built once per call) lies in the
 * library's scratch.
 *
 * lz4ada_compress_block_dict_host and lz4ada_compress_frame_dict_host state
 * the rule serially, as their plain twins do: the device call's bytes for a
 * job are lz4ada_compress_frame_dict_host's for its record.  dict may be NULL
 * with dict_len 0, which gives the plain twins' bytes; dict_flags and dict_id
 * are dict->flags and dict->dict_id.  Host only, no HIP call.
 */
#define LZ4ADA_COMP_DICT_WRITE_ID 1u
typedef struct {
	const void *d_dict; /* device memory */
	int64_t dict_len;   /* any length >= 0; the last 65,536 bytes are used */
	uint32_t dict_id;   /* written into the header with LZ4ADA_COMP_DICT_WRITE_ID */
	uint32_t flags;     /* LZ4ADA_COMP_DICT_* */
} lz4ada_compress_dict;
int64_t lz4ada_compress_frames_bound_dict(const lz4ada_compress_job *jobs, int64_t njobs,
                                          const lz4ada_compress_options *opt,
                                          const lz4ada_compress_dict *dict);
int lz4ada_compress_frames_device_dict(const void *d_in, int64_t in_len, lz4ada_compress_job *jobs,
                                       int64_t njobs, const lz4ada_compress_options *opt,
                                       const lz4ada_compress_dict *dict, void *d_out,
                                       int64_t out_cap, int64_t *out_len, void *stream);
int64_t lz4ada_compress_block_dict_host(const uint8_t *src, int64_t n, const uint8_t *dict,
                                        int64_t dict_len, uint8_t *dst, int64_t cap);
int64_t lz4ada_compress_frame_dict_host(const uint8_t *src, int64_t n,
                                        const lz4ada_compress_options *opt, const uint8_t *dict,
                                        int64_t dict_len, uint32_t dict_id, uint32_t dict_flags,
                                        uint8_t *dst, int64_t cap);

/* ------------------- records compressed into frames of linked blocks, on the device */
/*
 * lz4ada_compress_frames_device_dict writing frames of linked blocks, the
 * LZ4F default: FLG bit 5 (B.Indep) is clear, and
 * block i >= 1 of a record is compressed with the 65,536 bytes of its own
 * record in front of it, so its matches may begin there -- a record that
 * repeats itself across a block boundary, or ends in a short block, no longer
 * pays for the boundary.  Block 0 is compressed against the dictionary's tail,
 * or against nothing, and its bytes are exactly the unlinked call's; from block
 * 1 on the dictionary has slid out of the 64 KiB window and is not read,
 * as in LZ4F_compressFrame_usingCDict.  A record of at most one block yields
 * the unlinked frame with B.Indep clear (and so another HC) and nothing else
 * different.  The history is read from d_in: a block's lies wholly inside its
 * own record, so jobs may overlap and come in any order as before.
 *
 * dict may be NULL (no dictionary); otherwise it is the dictionary call's in
 * every respect.  The contract is lz4ada_compress_frames_device_dict's word
 * for word: the same misuse is LZ4ADA_ASSERTION_ERROR before any launch,
 * out_cap below lz4ada_compress_frames_bound_dict(jobs, njobs, opt, dict) --
 * the bound of this call too -- is LZ4ADA_TOO_LITTLE_MEMORY with *out_len set
 * to the bound and d_out untouched, the frames lie dense in job order, nothing
 * at or beyond d_out + *out_len is written, and the host synchronises `stream`
 * once per pass.  opt->flags stays closed: linking is this entry, not a flag.
 * A pass without a block i >= 1 queues exactly the launches of the unlinked
 * call.
 *
 * The frames decode through the calls that take linked frames:
 * lz4ada_decode_frame_dict_host, lz4ada_decode_frames_device(_dict) with
 * LZ4ADA_FRAMES_LINKED, a seek index built with LZ4ADA_SEEK_LINKED, and liblz4.
 * A linked frame may carry offsets of 65,529 and more across a block boundary.
 * A decoder with the reference's quirk D1 -- the
 * reference itself, the oracle, lz4ada_decode_frame and the facade -- may read
 * such a frame differently from the specification, as it may liblz4's own
 * linked frames.
 *
 * lz4ada_compress_frame_linked_host states one record serially: the device
 * call's bytes for a job are its bytes for that record.  It is
 * lz4ada_compress_frame_dict_host with the history of block i >= 1 replaced;
 * dict may be NULL with dict_len 0.  Host only, no HIP call.
 */
int lz4ada_compress_frames_device_linked(const void *d_in, int64_t in_len, lz4ada_compress_job *jobs,
                                         int64_t njobs, const lz4ada_compress_options *opt,
                                         const lz4ada_compress_dict *dict, void *d_out,
                                         int64_t out_cap, int64_t *out_len, void *stream);
int64_t lz4ada_compress_frame_linked_host(const uint8_t *src, int64_t n,
                                          const lz4ada_compress_options *opt, const uint8_t *dict,
                                          int64_t dict_len, uint32_t dict_id, uint32_t dict_flags,
                                          uint8_t *dst, int64_t cap);

/* ------------- records compressed into frames, with the frames' seek index */
/*
 * lz4ada_compress_frames_device, _dict or _linked -- by dict and by
 * LZ4ADA_COMP_INDEX_LINKED in xopt->flags -- that also writes the seek index
 * of the frames it writes, so that a caller who wants
 * byte ranges of them (lz4ada_decode_ranges_device) needs no
 * lz4ada_seek_index_build* over what the compressor already knew: where every
 * block lies, what it decodes to, and, for a linked frame, the 65,536 record
 * bytes in front of every checkpointed block, which lay in d_in.
 *
 * Frames.  d_out, *out_len and jobs[] come out byte for byte as that existing
 * call gives them; the bound, LZ4ADA_TOO_LITTLE_MEMORY and every misuse of it
 * behave the same, and on those outcomes *idx is NULL and nothing is
 * allocated.  Misuse of this entry alone -- idx NULL, unknown bits in
 * xopt->flags, xopt->reserved != 0, xopt->checkpoint_bytes < 0 -- is
 * LZ4ADA_ASSERTION_ERROR before any device call.  xopt NULL is {0, 0, 0}.
 *
 * Index.  On success *idx is an index over the input (d_out, *out_len); job k
 * is the frame at jobs[k].out_off.  lz4ada_decode_ranges_device,
 * lz4ada_seek_index_bytes, _free, _debug and lz4ada_ranges_select_debug take
 * it as they take a built one.  It holds what
 *   lz4ada_seek_index_build_dict(d_out, *out_len, frames, njobs,
 *       {linked ? LZ4ADA_SEEK_LINKED : 0, 0, checkpoint_bytes},
 *       {dict->d_dict, dict->dict_len, dict->dict_id, 0}, ...)
 * would hold -- descriptors, block starts, tight slots, frame kinds, its own
 * copy of the dictionary (any dict_len > 0; the caller's may be freed after the
 * call), checkpoint groups and the checkpoint store -- and
 * lz4ada_seek_index_bytes is that build's figure, with two deliberate
 * differences:
 *  1. The verdicts are those of the build's index stage alone: frame_walk's
 *     rule over the written sizes, which for these frames can only say
 *     LZ4ADA_BATCH_BIG_BLOCK (the lone-block rule: a frame of at most 24 blocks
 *     with a payload of 512 KiB or more, so only with 1 MiB and 4 MiB blocks,
 *     and never under LZ4ADA_NO_LONE).  LZ4ADA_BATCH_OVER_BUDGET is not judged
 *     (the ranged call judges a range's own blocks against LZ4ADA_BATCH_BYTES).
 *     Nothing is decoded, so there is no LZ4ADA_DEVFRAME_BLOCK from a block the
 *     index decoder declines or, in a linked frame without a dictionary, from
 *     quirk D1's round state at build time; such a block fails its ranges at
 *     range time with LZ4ADA_EXACT_PATH / LZ4ADA_DEVFRAME_BLOCK, as in a
 *     dictionary index today (the ranged decode has the specification's
 *     semantics).
 *  2. lz4ada_batch_linked_max() is not applied: a linked frame of any length
 *     is taken, with its checkpoints.  The limit belongs to passes that put one
 *     wave on a whole frame; a range decodes chains of at most K blocks.
 * njobs == 0 gives an empty index and makes no device call.
 *
 * frames, when given (njobs entries), is filled as the build would report it:
 * in_off / in_len the frame's place in d_out, out_len the record's length (0
 * for a frame the index did not take), status (LZ4ADA_OK or LZ4ADA_EXACT_PATH)
 * and reason; out_off and consumed 0.
 *
 * Synchronous on `stream`.  Host synchronisations: the compress passes' own
 * (one per pass, one more for a content checksum over LZ4ADA_BATCH_HASH_MAX
 * bytes) and no other -- the index's kernels of a pass are queued in front of
 * that pass's synchronisation -- unless the lone-block rule turned a frame
 * down: then one more, after which the index's arrays lie in memory of exactly
 * the build's size.  The index's device memory is allocated before the first
 * pass, for every frame taken.
 */
#define LZ4ADA_COMP_INDEX_LINKED 1u /* frames of linked blocks (the _linked call's frames) */
typedef struct {
	uint32_t flags;           /* LZ4ADA_COMP_INDEX_* */
	uint32_t reserved;        /* must be 0 */
	int64_t checkpoint_bytes; /* as lz4ada_seek_options; 0: the default; < 0: misuse */
} lz4ada_compress_index_options;
int lz4ada_compress_frames_device_indexed(const void *d_in, int64_t in_len,
                                          lz4ada_compress_job *jobs, int64_t njobs,
                                          const lz4ada_compress_options *opt,
                                          const lz4ada_compress_dict *dict,
                                          const lz4ada_compress_index_options *xopt, void *d_out,
                                          int64_t out_cap, int64_t *out_len,
                                          lz4ada_device_frame_job *frames,
                                          lz4ada_seek_index **idx, void *stream);
/* Test-only.  The rule the indexed call's kernels run (lz4ada_compress_index.h)
 * over one frame that lz4ada_compress_frame_host, _dict_host or _linked_host
 * wrote from a record of record_len bytes under opt and dict_flags: the written
 * sizes are read from the frame's size words, nothing else of it but the block
 * checksums.  descs / sizes (cap entries each; fewer blocks are written when
 * the frame holds more): every block's descriptor as the walk emits it for a
 * pass -- in_off = frame_off + its place in the frame, out_off from out_base in
 * steps of the slot capacity rounded up to 256, out_cap the slot capacity -- and
 * its decoded size.  *verdict: LZ4ADA_BATCH_OK or _BIG_BLOCK; *group and
 * *checkpoints: K and the checkpoint count of a linked frame (`linked`) with a
 * checkpoint every checkpoint_bytes (0: the default), else 0.  A frame that is
 * not the record's is LZ4ADA_ASSERTION_ERROR.  Host only, no HIP call. */
int lz4ada_compress_index_host(const uint8_t *frame, int64_t frame_len, int64_t record_len,
                               const lz4ada_compress_options *opt, uint32_t dict_flags,
                               uint32_t linked, int64_t checkpoint_bytes, uint64_t frame_off,
                               uint64_t out_base, lz4ada_block_desc *descs, uint32_t *sizes,
                               int64_t cap, int64_t *nblocks, int32_t *verdict, int64_t *group,
                               int64_t *checkpoints);
/* Test-only.  The checkpoint store of an index, copied to the host: *nckpt
 * entries of 65,536 bytes (store may be NULL to ask for the count alone). */
int lz4ada_seek_index_store_debug(const lz4ada_seek_index *idx, void *store, int64_t store_cap,
                                  int64_t *nckpt, void *stream);

/* ------------------------------- the indexes of several calls, laid into one */
/*
 * A record store grows batch by batch, and every compress call (or build)
 * returns an index of its own, while a ranged call takes one index over one
 * input.  lz4ada_seek_index_concat makes that one index
 * without reading a frame byte or decoding anything: every piece an index holds
 * is relative to its frame or is an offset that one constant per part rebases.
 *
 * On success *idx is a new index over an input of in_len bytes in which the
 * input that part p was made over lies at [in_base[p], in_base[p] + its
 * in_len).  Job j of part p is job (jobs of parts 0 .. p-1) + j of the result.
 * The result holds what one index over the whole input would hold, array for
 * array -- when the parts come from compress calls over consecutive groups of
 * records, the index one call over all the records writes -- and is an
 * ordinary index: lz4ada_decode_ranges_device (which demands the new in_len),
 * lz4ada_seek_index_bytes, _free, _debug, _store_debug and
 * lz4ada_ranges_select_debug take it, and it may be a part of a later concat.
 * lz4ada_seek_index_bytes is the formulas above over the sums: nb, n and C
 * summed over the parts, the LZ4ADA_SEEK_LINKED line when any part has it, the
 * dictionary line once.
 *
 * Parts are not modified and not consumed; a part may serve ranged calls on
 * other threads meanwhile, and may be freed as soon as the call returns: the
 * result owns copies of everything, the dictionary image and the checkpoints
 * included.  A part's jobs need not lie in rising in_off (a built index): its
 * sorted positions are kept, shifted by the frames before it.  Linked and
 * unlinked parts may be mixed: if any part holds checkpoint arrays the result
 * does, and the frames of parts without them get K = 0 and no checkpoint, as
 * an LZ4ADA_SEEK_LINKED build gives independent frames.  A part with no job
 * contributes nothing; if all are such, or nparts == 0, the result is an empty
 * index over in_len and no device call is made.  The same part may be named
 * twice (two copies of its frames in the input).
 *
 * Dictionaries: either no part with jobs holds one or every one does, and then
 * all hold the same -- the same dict_used and the same image bytes.  A mix, or
 * another dict_used, is LZ4ADA_ASSERTION_ERROR before any device call.  Other
 * bytes are found by a comparison on the device whose flag the host reads at
 * the call's one synchronisation: LZ4ADA_ASSERTION_ERROR then too, after the
 * kernels ran, with *idx NULL and the parts as they were.
 *
 * Misuse, LZ4ADA_ASSERTION_ERROR before any device call with *idx NULL: a NULL
 * idx; NULL parts or in_base with nparts > 0; a NULL part; nparts < 0;
 * in_len < 0; a negative base; in_base[p] < in_base[p-1] + the in_len of part
 * p-1 (parts rise and stay apart; touching and gaps are fine); a part that
 * ends past in_len.  2^31 jobs or blocks in all, or more:
 * LZ4ADA_CONSTRAINT_ERROR, as the builds.
 *
 * Synchronous on stream.  One copy takes the part table up, a fixed number of
 * launches follows whatever nparts is, and the call makes exactly one host
 * synchronisation, at its end, after which the index never changes.
 * lz4ada_last_batch_stats() is all zero.
 */
int lz4ada_seek_index_concat(const lz4ada_seek_index *const *parts, const int64_t *in_base,
                             int64_t nparts, int64_t in_len, lz4ada_seek_index **idx,
                             void *stream);
/* Test-only.  The merge rule on the host (lz4ada_index_merge.h, what the concat
 * validates and sums by and its kernels look parts up with): parts given by
 * their jobs n[], blocks nb[], checkpoints nck[], input lengths part_len[] and
 * nominal slots slots[], at in_base[] of an input of in_len bytes.  prefix (5 *
 * (nparts + 1) entries) gets the exclusive prefixes of frames, blocks, blocks +
 * frames, checkpoints and nominal slots, one after the other.  part_of[q]: the
 * part that merged element elem[q] of prefix kind[q] (0 .. 4) belongs to.
 * LZ4ADA_ASSERTION_ERROR for what the concat calls misuse and for a query
 * outside its prefix's total, LZ4ADA_CONSTRAINT_ERROR from 2^31 jobs or blocks.
 * Host only, no HIP call. */
int lz4ada_index_merge_plan_host(const int64_t *n, const int64_t *nb, const int64_t *nck,
                                 const int64_t *part_len, const int64_t *slots,
                                 const int64_t *in_base, int64_t nparts, int64_t in_len,
                                 uint64_t *prefix, const int64_t *kind, const int64_t *elem,
                                 int64_t nq, int64_t *part_of);
/* Test-only.  An index's device arrays copied to the host.  *nframes, *nblocks,
 * *nckpt: its counts; *has_ckpt / *has_kind: whether it holds kgrp and ckfirst
 * / fkind.  Each array may be NULL (call once for the counts); the caller gives
 * room for nblocks descriptors, nframes + 1 entries of first and ckfirst,
 * nblocks + nframes of start and slotp, nframes of kgrp and fkind.  An index
 * without jobs holds no array. */
int lz4ada_seek_index_arrays_debug(const lz4ada_seek_index *idx, int64_t *nframes,
                                   int64_t *nblocks, int64_t *nckpt, int32_t *has_ckpt,
                                   int32_t *has_kind, lz4ada_block_desc *desc, uint64_t *first,
                                   uint64_t *start, uint64_t *slotp, uint64_t *kgrp,
                                   uint64_t *ckfirst, uint64_t *fkind, void *stream);

/* The bulk path keeps its large device scratch (output slots, linked-frame
 * decode copies) per thread between calls; this frees the calling thread's,
 * and empties the process-wide device / pinned memory pools and the stream
 * pool that the streaming contexts and the bulk paths draw from. */
void lz4ada_release_device_cache(void);

/* What those pools hold idle right now (the per-thread scratch is not
 * counted): bytes of device and of pinned host memory, and pooled sets of
 * a context's two streams and event.  Reads counters only: no HIP call. */
typedef struct {
	int64_t device_idle_bytes, pinned_idle_bytes, idle_streams;
} lz4ada_cache_stats;
void lz4ada_device_cache_stats(lz4ada_cache_stats *out);

/* Upper bound of the decoded size of a stream (sum of block maxima); -1 if
 * some frame does not index (then use the _alloc calls). */
int64_t lz4ada_decoded_bound(const uint8_t *input, int64_t len);

/* ------------------------------------------------- multi-GPU bulk decode */
/*
 * One frame over n_gpus devices from ONE process (no
 * reference twin -- it replaces the caller's whole Update loop
 * (lz4ada.ads:281-287, tool_unlz4ada/unlz4ada.adb:84-103) for a frame, like
 * lz4ada_decode_frame, and spreads it over GPUs).  An independent-block
 * modern frame is split into contiguous block ranges balanced by compressed
 * bytes (lz4ada_plan_shards); one host worker thread per device copies its
 * range in and decodes it; RCCL (ncclCommInitAll over the devices) carries
 * one all-reduce of the block verdict and the per-device output sizes, and
 * for the _gather variant the bytes to the first device.  The content
 * checksum is one XXH32 chain in frame order.  Linked, legacy and skippable
 * frames, and any frame the bulk path would not take (block error, checksum
 * mismatch, cross-block references, failed frame checks), are decoded by
 * lz4ada_decode_frame on the first device, which gives the reference's
 * output or exception.  devices: n_gpus HIP ordinals, or NULL for
 * 0 .. n_gpus-1.  Calls are serialised (the communicators are shared).
 */
int lz4ada_decode_frame_multi(const uint8_t *frame, int64_t len, int n_gpus, const int *devices,
                              uint8_t *out, int64_t out_cap, int64_t *out_len,
                              int64_t *frame_consumed);
/* The same with the output gathered into d_out on the first device
 * (out_cap bytes, device memory) instead of host memory. */
int lz4ada_decode_frame_multi_gather(const uint8_t *frame, int64_t len, int n_gpus,
                                     const int *devices, void *d_out, int64_t out_cap,
                                     int64_t *out_len, int64_t *frame_consumed);
/* The block split of the above (and of bo-lz4-ada_amd/shard.py): rank r
 * decodes blocks [bounds[r], bounds[r+1]) (bounds has n_gpus + 1 entries);
 * the blocks whose compressed-prefix midpoint falls in
 * [r, r+1) * total / n_gpus.  Host-only. */
int lz4ada_plan_shards(const lz4ada_block_desc *descs, int64_t nblocks, int n_gpus,
                       int64_t *bounds);
/* Device allocations the multi-GPU workers made so far for HIP ordinal
 * `device` (each worker keeps its buffers and pinned staging between calls:
 * a repeated call of the same size adds none); -1 if it has no worker yet. */
int64_t lz4ada_multi_device_allocs(int device);
/* The RCCL version the process actually bound (ncclGetVersion, e.g. 22606
 * for 2.26.6): in a process that loaded another librccl.so.1 first (a torch
 * job loads its bundled one), that library serves this one's calls too;
 * a plain C / Ada program gets /opt/rocm/lib's (the library's RUNPATH). */
int lz4ada_rccl_version(void);

/* ------------------------------------------------------------------ misc */

/* 0 when a HIP device is usable, else LZ4ADA_DEVICE_ERROR (message in
 * lz4ada_thread_last_error()). */
int lz4ada_device_check(void);
int lz4ada_abi_version(void);

/*
 * Deterministic synthetic LZ4 block generator for benches and tests
 * (SURVEY §8d): emits one valid compressed block whose decoded size is
 * exactly raw_len.  kind: 0 dense (~5 B/sequence), 1 mixed (~32 B/seq,
 * ratio ~2), 2 rle (zeros, offset 1), 3 literal-heavy, 4 chain (matches
 * only, offsets <= 16), 5 mixed with offsets <= 65528 (no match can meet
 * quirk D1 in a linked frame).  Writes the decoded
 * bytes to raw (raw_len bytes) and the block payload to comp; returns the
 * payload length, or -1 if comp_cap is too small.
 */
int64_t lz4ada_gen_block(int kind, uint64_t seed, uint8_t *raw, int64_t raw_len,
                         uint8_t *comp, int64_t comp_cap);
/* The same for one block of a linked frame: buf holds `hist` bytes of the
 * frame's earlier output, then room for raw_len decoded bytes (written at
 * buf + hist); offsets may reach back into the history (up to 65535). */
int64_t lz4ada_gen_block_linked(int kind, uint64_t seed, uint8_t *buf, int64_t hist,
                                int64_t raw_len, uint8_t *comp, int64_t comp_cap);

#ifdef __cplusplus
}
#endif
#endif
