// lz4ada_host_common.h -- what the host units of the MI355X LZ4Ada
// decompressor share: the reference's exceptions and 'Image texts, the
// process-wide device / pinned memory pools and stream pool, the frame
// header parser (lib/lz4ada.adb:155-375), the host XXH32 chain and the
// device-status -> exception map.  This header holds the types, the
// templates and the declarations; lz4ada_host_common.cpp holds the one
// instance of the shared state and every non-template body.  Units that
// include it: lz4ada_facade.cpp (the streaming Update facade and the
// XXHash32 C-ABI), lz4ada_bulk.cpp (the bulk frame paths and their C-ABI),
// lz4ada_bulk_linked.cpp (the linked-frame bulk path in stages; its round
// state is lz4ada_round_state.h's, its host decisions -- laying a batch,
// accepting blocks, plane modes -- lz4ada_linked_accept.h's, both plain C++ for
// tools/linked_accept_check.cpp), lz4ada_bulk_frames.cpp
// (many frames in one device pass), lz4ada_bulk_frames_device.cpp (the same
// pass from device memory to device memory), lz4ada_frames_pass.cpp (the
// device half of that pass, which both share), lz4ada_bulk_ranges.cpp (the
// seek index over device-resident frames and the ranged decode, which begins
// with the device engine's index and sizes stages).  lz4ada_multi.cpp
// (the multi-GPU entry) keeps a per-device cache of its own and includes
// only lz4ada_internal.h.
//
// The host only parses framing.  Every block byte is produced on the GPU;
// there is no CPU decoder: without a GPU, decoding calls fail with
// LZ4ADA_DEVICE_ERROR.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "lz4ada_hip.h"
#include "lz4ada_internal.h"
#include "lz4ada_linked_accept.h"
#include "lz4ada_pass_runs.h"

namespace lz4ada {

// ------------------------------------------------------------------ errors

struct Error {
	int code;
	std::string msg;
};

[[noreturn]] inline void raise(int code, std::string msg) { throw Error{ code, std::move(msg) }; }

// Ada 'Image: leading blank for non-negative numbers.
inline std::string img(int64_t v)
{
	return v >= 0 ? " " + std::to_string(v) : std::to_string(v);
}
inline std::string img_u(uint64_t v) { return " " + std::to_string(v); }
std::string hex32(uint32_t v);

inline uint32_t load32(const uint8_t* p)
{
	return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) |
	       (uint32_t(p[3]) << 24);
}

// ------------------------------------------------------------------ device

#define HIP_OK(expr)                                                                          \
	do {                                                                                  \
		hipError_t _e = (expr);                                                       \
		if (_e != hipSuccess)                                                         \
			raise(LZ4ADA_DEVICE_ERROR,                                            \
			      std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr); \
	} while (0)

void device_check_or_raise();

// Process-wide pools of the small device and pinned host allocations and
// of the facade's streams.  A streaming context per frame (tool_unlz4ada
// re-inits per frame, unlz4ada.adb:84-87) otherwise pays stream creation
// and a dozen hipMalloc / hipHostMalloc calls per frame -- ~3.5 ms, more
// than a 4 MiB frame of 64 KiB blocks takes to decode (tools/facade_c).
// Blocks up to POOL_MAX bytes are kept by power-of-two size class, at most
// keep_limit() idle bytes per kind over all devices (`kept`); a block is
// pooled only after a device synchronisation (the implicit one of the
// hipFree it replaces), so no queued work still uses it.
// lz4ada_release_device_cache() empties them; lz4ada_device_cache_stats()
// reports what they hold.
struct MemPool {
	static constexpr size_t POOL_MAX = size_t(256) << 20;
	// idle bytes kept per pool (device / pinned): 1 GiB, or LZ4ADA_POOL_KEEP_MB
	static size_t keep_limit();
	std::mutex mu;
	std::vector<std::tuple<int, size_t, void*>> free;  // (device, class bytes, block)
	size_t kept = 0;
	bool pinned;
	explicit MemPool(bool pin) : pinned(pin) {}
	static size_t size_class(size_t b);
	void raw_free(void* p);
	// A block and the device that was current when it was taken: put() syncs
	// and files it under THAT device (a buffer released after the
	// caller switched GPUs must not be pooled under the new one).  Pinned
	// blocks are pooled for any device but still sync the device they served.
	struct Block {
		void* p;
		size_t bytes;
		int dev;
	};
	Block get(size_t bytes);
	void put(void* p, size_t c, int dev);
	void release_all();
};
MemPool& dev_pool();
MemPool& pin_pool();

template <class T>
struct DevBuf {
	T* p = nullptr;
	size_t n = 0;      // elements
	size_t bytes = 0;  // the block's usable bytes
	int dev = 0;       // the device it was allocated on
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { release(); }
	void release()
	{
		if (p)
			dev_pool().put(p, bytes, dev);
		p = nullptr;
		n = bytes = 0;
	}
	void reserve(size_t count)
	{
		if (count <= n && p)
			return;
		release();
		const auto b = dev_pool().get(std::max<size_t>(count, 1) * sizeof(T) + 64);
		p = static_cast<T*>(b.p);
		bytes = b.bytes;
		dev = b.dev;
		n = count;
	}
};

// Per-block arrays (descriptors, statuses) between a host vector and device
// memory, sized from the vector itself -- never from a block count captured
// earlier (round 5: a status copy sized before a quirk-D1 stop shrank the
// batch overran its vector) -- and checked against the device buffer's
// capacity.
template <class T>
inline void vec_h2d(DevBuf<T>& d, const std::vector<T>& v, hipStream_t stream)
{
	if (v.size() > d.n)
		raise(LZ4ADA_DEVICE_ERROR, "host array larger than its device buffer");
	HIP_OK(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
}
template <class T>
inline void vec_d2h(std::vector<T>& v, const DevBuf<T>& d, hipStream_t stream)
{
	if (v.size() > d.n)
		raise(LZ4ADA_DEVICE_ERROR, "host array larger than its device buffer");
	HIP_OK(hipMemcpyAsync(v.data(), d.p, v.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
}

// Pinned host memory, grow-only (the facade's output staging).
struct PinBuf {
	uint8_t* p = nullptr;
	size_t n = 0, bytes = 0;
	int dev = 0;  // the device current when it was taken (synced on release)
	PinBuf() = default;
	PinBuf(const PinBuf&) = delete;
	PinBuf& operator=(const PinBuf&) = delete;
	~PinBuf() { release(); }
	void release()
	{
		pin_pool().put(p, bytes, dev);
		p = nullptr;
		n = bytes = 0;
	}
	void reserve(size_t count)
	{
		if (count <= n && p)
			return;
		release();
		const auto b = pin_pool().get(std::max<size_t>(count, 1));
		p = static_cast<uint8_t*>(b.p);
		bytes = b.bytes;
		dev = b.dev;
		n = count;
	}
	void swap(PinBuf& o)
	{
		std::swap(p, o.p);
		std::swap(n, o.n);
		std::swap(bytes, o.bytes);
		std::swap(dev, o.dev);
	}
};

// The facade's streams and event, reused across contexts.  take_streams:
// an idle set of `device` from the pool, else a new one (false: HIP could
// not create it; nothing is left half made).  give_streams: back to the
// pool once both streams are idle, destroyed otherwise.
// destroy_idle_streams: every pooled set, on its own device.
struct StreamSet {
	int device = -1;
	hipStream_t stream = nullptr, side = nullptr;
	hipEvent_t ev = nullptr;
};
bool take_streams(int device, StreamSet& s);
void give_streams(const StreamSet& s);
void destroy_idle_streams();

// One long-lived helper thread running one job at a time (the facade's
// content checksum of a large block while the caller feeds the next one);
// wait() joins the current job.
struct Worker {
	std::thread th;
	std::mutex mu;
	std::condition_variable cv, done_cv;
	std::function<void()> job;
	bool busy = false, stop = false;
	Worker() = default;
	Worker(const Worker&) = delete;
	Worker& operator=(const Worker&) = delete;
	~Worker();
	void submit(std::function<void()> f);
	void wait();
	void loop();
};

// ------------------------------------------------------------------ meta

enum Fmt { F_TBD, F_LEGACY, F_MODERN, F_BLOCK, F_SKIPPABLE };               // lz4ada.ads:355
enum Hps { NEED_MAGIC, NEED_MODERN, NEED_FLAGS, NEED_SKIP_LEN, HDR_DONE };  // lz4ada.ads:356

constexpr uint32_t MAGIC_MODERN = 0x184d2204u;  // lz4ada.ads:348-353
constexpr uint32_t MAGIC_LEGACY = 0x184c2102u;
constexpr uint32_t MAGIC_SKIP_LO = 0x184d2a50u, MAGIC_SKIP_HI = 0x184d2a5fu;

struct Meta {  // Decompressor_Meta, lz4ada.ads:359-370
	int is_format = F_TBD;
	int header_parsing = NEED_MAGIC;
	int memory_reservation = LZ4ADA_FOR_ALL;
	int content_checksum_length = 0;
	int block_checksum_length = 0;
	int status_eof = LZ4ADA_EOF_NO;
	int64_t input_buffer_filled = 0;
	bool is_compressed = false;
	bool has_content_size = false;
	uint64_t size_remaining = 4;
	// frame descriptor facts the reference does not keep (bulk path)
	uint8_t flg = 0, bd = 0;
};

inline bool concrete(int r) { return r >= LZ4ADA_SZ_64_KIB && r <= LZ4ADA_SZ_8_MIB; }

// The header parser (lz4ada.adb:65-77, 155-375): Get_Block_Size, the magic
// word's step (the facade also takes it at a legacy frame's next magic) and
// Process_Header_Bytes, which returns the bytes it consumed.
int64_t block_size_of(int r);
void header_magic(Meta& m, uint32_t magic);
int64_t header_bytes(Meta& m, uint8_t* hb, const uint8_t* in, int64_t len);
bool is_any_magic(uint32_t v);

// XXHash32.Update / Final (lz4ada.adb:942-1017) on host bytes the GPU
// decoded (content checksums: the facade's Hash_All_Data and the bulk
// path's pipeline).  The state layout is the one the GPU kernel
// k_xxh32_update advances, so the two can continue each other.
void host_xxh32_update(lz4ada_xxh32_state& h, const uint8_t* p, size_t n);
uint32_t host_xxh32_final(const lz4ada_xxh32_state& h);

// Device status of a decode kernel -> the reference's exception.
[[noreturn]] void raise_device_status(const SerialState& s);

// ---------------------------------------------- shared by the host units

// A few large blocks: one block at a time through the lone-block decoder
// (lz4ada_lone.hip, the whole GPU per block: ~0.4 ms per 4 MiB mixed block)
// beats the bulk decoder's one wave per block (~13 ms per 4 MiB block, at
// any count up to the chip's 2,048 resident waves) below ~30 blocks.
bool few_large_blocks(const std::vector<lz4ada_block_desc>& d);
// LZ4ADA_NO_LONE is set (read once per process): few_large_blocks is never true.
bool lone_blocks_disabled();
// decode_lone_blocks: every block of d (host descriptors, offsets into d_in
// and d_out) through the lone-block decoder, stored ones as a copy, while
// host threads hash the blocks' host bytes for their checksums
// (lz4ada.adb:698-707).  st gets code, out_len and cksum as the bulk
// decoder's statuses carry them; false when a block was declined (the
// caller then runs the bulk decoder, which produces the exact status).
bool decode_lone_blocks(const uint8_t* host_in, const uint8_t* d_in,
                        const std::vector<lz4ada_block_desc>& d, uint8_t* d_out,
                        lz4ada_block_status* d_st, std::vector<lz4ada_block_status>& st,
                        DevBuf<uint8_t>& scr, hipStream_t stream);
enum BulkResult { BULK_OK, BULK_EXACT, BULK_PRE_REF, BULK_FAIL_AT };
// Where a linked batch's resolved bytes go: dst(n) returns the device
// buffer for the batch's n bytes (nullptr: no room), done(p, n) runs once
// they are there.
struct LinkedSink {
	std::function<uint8_t*(int64_t)> dst;
	std::function<void(const uint8_t*, int64_t)> done;
};

// A linked batch that starts mid-frame (the facade's read-ahead): the
// history before its first block, as device bytes oldest first (the
// reference's Buffer keeps it in two places), and the round state there
// (quirk D1).
struct LinkedHist {
	const uint8_t* h0 = nullptr;
	int64_t n0 = 0;
	const uint8_t* h1 = nullptr;
	int64_t n1 = 0;
	RoundState round;
};
BulkResult bulk_linked(const uint8_t* d_frame, uint64_t frame_len, int64_t block_max,
                              const std::vector<lz4ada_block_desc>& descs, LinkedSink& sink,
                              uint64_t& total, std::vector<uint32_t>& lens, int64_t& fail,
                              hipStream_t stream, const LinkedHist* hist = nullptr);

// Where decoded bytes go: the caller's fixed buffer, or a malloc'd buffer
// that grows (lz4ada_decode_*_alloc).  `len` is what is committed so far.
struct Sink {
	uint8_t* p = nullptr;
	int64_t cap = 0;
	bool growable = false;
	int64_t len = 0;
	// Room for n more bytes after len.
	uint8_t* room(int64_t n)
	{
		if (len + n > cap) {
			if (!growable)
				raise(LZ4ADA_CONSTRAINT_ERROR, "output capacity exceeded");
			int64_t c = std::max<int64_t>(len + n, std::max<int64_t>(2 * cap, 1 << 16));
			void* q = realloc(p, size_t(c));
			if (!q)
				raise(LZ4ADA_CONSTRAINT_ERROR, "output allocation failed");
			p = static_cast<uint8_t*>(q);
			cap = c;
		}
		return p + len;
	}
	void commit(int64_t n) { len += n; }
};

// Where the exact path resumes a frame the bulk path decoded up to a failing
// block: the stream state Decode_Full_Block_With_Trailer would have there
// (lz4ada.adb:661-714) -- Output_Pos / Output_Pos_History replayed from the
// decoded lengths (:678-690, 785-787), the content size left (:826-839) and
// the content hash (:709-714) over the bytes already committed.
struct Resume {
	int64_t at = 0;          // frame offset of the resume block's size word
	RoundState round;        // the round state before it
	uint64_t committed = 0;  // bytes of the blocks before it
	lz4ada_xxh32_state hash{};
	const uint8_t* output = nullptr;  // those bytes, and each block's length
	const std::vector<uint32_t>* lens = nullptr;
	bool checksum_first = false;  // check the resume block's checksum before decoding it
};

// ------------------------------------------------ bulk-path device helpers

// A device allocation that may fail without raising (the bulk path then
// shrinks its batch or hands the frame to the exact path).
template <class T>
inline bool try_reserve(DevBuf<T>& b, size_t count)
{
	if (count <= b.n && b.p)
		return true;
	b.release();
	const size_t bytes = std::max<size_t>(count, 1) * sizeof(T) + 64;
	if (hipMalloc(reinterpret_cast<void**>(&b.p), bytes) != hipSuccess) {
		(void)hipGetLastError();
		b.p = nullptr;
		return false;
	}
	b.n = count;
	b.bytes = bytes;  // not a pool size class: freed, never pooled
	return true;
}

// Device scratch of the bulk path, kept per thread between calls: the
// large buffers (slots, decode copies, resolution words) cost a hipMalloc
// and a first-touch each time otherwise -- more than the decode itself on a
// 1 GiB linked frame.  lz4ada_release_device_cache() frees them.  The
// cache is never destroyed at thread exit (the HIP runtime may be gone).
// SC_BATCH / SC_BATCH_META: a many-frame pass's compacted output and its
// per-block / per-frame arrays (PassArrays below), which outlive the
// single-frame decodes of the frames the pass did not find good.
// SC_SIZES: what the sizes stage of a device call leaves for its passes
// (lz4ada_bulk_frames_device.cpp).
// SC_DICT: a dictionary call's small per-frame words.
// SC_SEEK: the walk records a seek index's linked build keeps beside the
// index's own for all its passes (lz4ada_bulk_ranges.cpp).
enum ScratchRole { SC_FRAME, SC_OUT, SC_COMPACT, SC_X, SC_Y, SC_H, SC_Z, SC_TAB, SC_P, SC_F, SC_LONE, SC_U,
	           SC_LINK, SC_M, SC_BATCH, SC_BATCH_META, SC_SIZES, SC_DICT, SC_SEEK, SC_N };
struct ScratchCache {
	DevBuf<uint8_t> b[SC_N];
	PinBuf pin;  // the linked path's small host transfers (pinned: no staging copy)
};
ScratchCache& scratch_cache();
// bytes of scratch `role`, or nullptr when the device has no room (the
// caller then shrinks its batch or takes the exact path; other roles may be
// in use, so they are kept)
uint8_t* scratch(int role, size_t bytes);

// a positive byte count from the environment, else dflt
int64_t env_bytes(const char* name, int64_t dflt);

// (slot_cap, a block's output slot capacity, and round256: lz4ada_linked_accept.h)

// Contiguous runs of blocks [lo, hi) whose slot bytes (plus `extra` per
// block) stay within `budget` (at least one block each).
std::vector<std::pair<uint32_t, uint32_t>> batches_of(const std::vector<lz4ada_block_desc>& descs,
                                                      int64_t bmax, uint64_t extra, uint64_t budget);

// a synchronous device-to-host copy on `stream`
void d2h(void* dst, const void* src, size_t n, hipStream_t stream);

// Reference-exact path for one frame: the unlz4ada loop
// (tool_unlz4ada/unlz4ada.adb:84-103) over the streaming engine, from the
// frame start or from `resume` (lz4ada_facade.cpp).
void exact_frame(const uint8_t* f, int64_t len, Sink& out, int64_t& consumed_total,
                 const Resume* resume = nullptr);

// The content hash of device-resident output through the D2H pipeline
// (lz4ada_facade.cpp); host_out gets the bytes on the way (may be null).
void content_xxh32_d2h(lz4ada_xxh32_state& h, const uint8_t* d_data, int64_t len, uint8_t* host_out,
                       hipStream_t stream);

// ------------------------------------------ frames, one at a time or many

// Walk one frame's block size words (lz4ada_bulk.cpp); descs may be null.
void index_frame(const uint8_t* f, int64_t len, lz4ada_frame_info& info,
                 std::vector<lz4ada_block_desc>* descs);
// One frame from host memory (Single_Frame semantics) through the bulk
// paths or the exact path: the reference's output or exception
// (lz4ada_bulk.cpp).
void decode_one_frame(const uint8_t* f, int64_t len, Sink& out, int64_t& consumed);
// A stream's next frame starts with fewer than 7 bytes left.
void partial_frame_check(int64_t left);
// Every frame of a concatenated stream into `out`, committed in order
// (lz4ada_bulk_frames.cpp): runs of batchable frames in one device pass
// each, every other frame by decode_one_frame.  *committed (may be null)
// follows out.len after each frame or run that succeeded; the first failing
// frame's exception propagates.
void decode_stream_frames(const uint8_t* input, int64_t len, Sink& out, int64_t* committed);

// What the many-frame engines share (lz4ada_frames_pass.cpp).  Read per call:
// a pass's slot byte budget (LZ4ADA_BATCH_BYTES), the decoded length up to
// which it hashes a content checksum on the GPU (LZ4ADA_BATCH_HASH_MAX), the
// slot bytes up to which a linked frame shares it (LZ4ADA_BATCH_LINKED_MAX,
// DESIGN.md §12), the flags of the entries that take none (LZ4ADA_BATCH_LINKED=1
// -> LZ4ADA_FRAMES_LINKED).  The thread's counters (lz4ada_last_batch_stats).
int64_t batch_budget();
int64_t batch_hash_max();
int64_t batch_linked_max();
uint32_t batch_env_flags();
lz4ada_batch_stats& batch_stats();
// A pass's device arrays in this thread's scratch.  SC_BATCH_META: descriptors
// | frame records | statuses | dst_off | loc | part.  SC_OUT: the slots.
// SC_TAB: the sequence index, only when a run is linked.  reserve() queues
// nothing; null, or what had no room: "block arrays", "slots", "sequence index".
struct PassArrays {
	uint32_t nb = 0, nf = 0;
	size_t desc_b = 0, rec_b = 0, st_b = 0;
	lz4ada_block_desc* d_desc = nullptr;
	FrameRec* d_rec = nullptr;
	lz4ada_block_status* d_st = nullptr;
	uint64_t *d_off = nullptr, *d_loc = nullptr, *d_part = nullptr;
	uint8_t *d_slots = nullptr, *d_tab = nullptr;
	std::vector<PassRun> runs;  // pass_runs(frames)
	uint32_t dict_used = 0;     // a dictionary pass: the history of a BLOCK_DICT block (runs with .dict)
	const char* reserve(const std::vector<PassFrame>& frames, uint64_t slots, uint64_t in_len);
};
// The device half of a pass, once a.d_desc and a.d_rec are queued on stream.
// decode_pass_blocks: the status memset, each run's decode launches and
// k_frames_plan (where the seek index's linked build goes its own way).
// decode_pass: that, k_compact into dst, k_xxh32_spans, the frame records into
// the pinned h_rec, the pass's one synchronisation, ++passes.  in_off must rise
// strictly over the whole pass (frame order, block order) and in_len cover every
// block: the index decoder's table keeps block b's records at ((in_off >> 8) + b)
// and is sized from in_len (index_table_bytes), or two blocks' records would
// overlap or leave the table.  A linked run indexes into d_tab + b0 * 64, as one
// launch_index over the pass.
void decode_pass_blocks(const PassArrays& a, const uint8_t* d_in, uint64_t in_len, hipStream_t stream);
void decode_pass(const PassArrays& a, const uint8_t* d_in, uint64_t in_len, uint8_t* dst, uint64_t hash_max,
                 FrameRec* h_rec, hipStream_t stream);
// A frame's record after the pass, against its declared content checksum: the
// LZ4ADA_DEVFRAME_* reason, or FV_HOST_HASH: good so far, the checksum (over
// hash_max bytes) is the host chain's.  *gpu_hashed: the record carries a hash.
enum FrameVerdict { FV_GOOD = LZ4ADA_DEVFRAME_OK, FV_BLOCK = LZ4ADA_DEVFRAME_BLOCK, FV_SIZE = LZ4ADA_DEVFRAME_SIZE,
	            FV_CHECKSUM = LZ4ADA_DEVFRAME_CHECKSUM, FV_HOST_HASH };
FrameVerdict frame_verdict(const FrameRec& r, uint32_t declared, bool* gpu_hashed);

// ------------------------------- frames indexed where they lie, on the device

// The jobs of a device call in rising in_off, indexed on the device
// (lz4ada_bulk_frames_device.cpp; the seek index of lz4ada_bulk_ranges.cpp is
// built from one).  The device arrays live in this thread's SC_FRAME scratch
// (a device pass stages nothing there).
struct FramesIndex {
	std::vector<uint32_t> order;     // sorted position -> job
	std::vector<FrameWalkRec> walk;  // by sorted position
	std::vector<FrameSpan> span;     // by sorted position
	FrameSpan* d_span = nullptr;
	FrameWalkRec* d_walk = nullptr;
	uint64_t *d_first = nullptr, *d_slot = nullptr;  // n + 1 entries each
	bool take_linked = false;                        // LZ4ADA_FRAMES_LINKED, and its cap
	uint64_t linked_max = 0;
	bool linked(size_t k) const { return (walk[k].flags & FRAME_LINKED) != 0; }
	bool taken(size_t k) const { return walk[k].verdict == LZ4ADA_BATCH_OK; }
	bool skippable(size_t k) const { return walk[k].format == LZ4ADA_FORMAT_SKIPPABLE; }
	// The sizes stage (size_jobs), when it ran: every frame's
	// exact and tight bytes, and on the device (this thread's SC_SIZES scratch)
	// the walk records with the tight slots, every frame's first block among
	// the block sizes, and the block sizes of the whole call.
	bool sized = false;
	std::vector<FrameSizeRec> size;  // by sorted position
	FrameWalkRec* d_tight = nullptr;
	uint64_t* d_size_first = nullptr;
	uint32_t* d_size = nullptr;
	uint64_t slots(size_t k) const { return sized ? size[k].tight : walk[k].slots; }
};
// The two stages and what each says about every job (bodies and comments in
// lz4ada_bulk_frames_device.cpp).  index_jobs: the argument checks, the sort
// and the walk, one host synchronisation; `entry` names the caller in a
// misuse's text.  size_jobs: the exact sizes, one more.  report_index /
// report_sizes: status, reason and (sizes) out_len of every job; they return
// the bound / the total.
void index_jobs(const char* entry, const void* d_in, int64_t in_len, const lz4ada_device_frame_job* jobs,
                int64_t njobs, uint32_t flags, hipStream_t stream, FramesIndex& ix);
void size_jobs(FramesIndex& ix, const uint8_t* d_in, uint64_t in_len, hipStream_t stream);
int64_t report_index(const FramesIndex& ix, lz4ada_device_frame_job* jobs);
int64_t report_sizes(const FramesIndex& ix, lz4ada_device_frame_job* jobs);
// A dictionary call's dictionary.  check_dict: its misuse
// (a negative length, a NULL pointer with bytes, unknown flag bits), raised
// before any launch; dict may be null.  check_dict_ids (LZ4ADA_DICT_CHECK_ID),
// after index_jobs: a taken modern frame naming another id is no longer
// taken(), LZ4ADA_DEVFRAME_DICT its verdict on the host and on the device; one
// host synchronisation.
void check_dict(const char* entry, const lz4ada_device_dict* dict);
void check_dict_ids(FramesIndex& ix, const uint8_t* d_in, uint32_t dict_id, hipStream_t stream);
// The dictionary as the passes see it: k_dict_fill copies the last `used` of
// its `len` bytes (a _dict call's dictionary, or a seek index's gap image).
struct DictCtx {
	const uint8_t* d_dict;
	uint64_t len;
	uint32_t used;  // min(the dictionary's length, DICT_MAX)
	uint64_t gap;   // dict_gap(used)
};
// A pass over the sorted jobs [lo, hi) up to its decode (bodies and comments in
// lz4ada_bulk_frames_device.cpp), for the device engine and for the seek
// index's linked build, which passes a view of its index in which only the
// linked frames are taken.  reserve_pass: the arrays (`slots`: slot bytes, gaps
// included).  fill_pass: descriptors and frame records.  lay_dict_pass: a
// dictionary's gaps (gapped_blocks of each job) and the runs cut for its
// decoders; h_kind: pinned room for hi - lo words no queued copy may still read.
uint64_t gapped_blocks(const FramesIndex& ix, size_t k);
void reserve_pass(PassArrays& a, const FramesIndex& ix, size_t lo, size_t hi, uint64_t slots, uint64_t in_len);
void fill_pass(const FramesIndex& ix, size_t lo, size_t hi, const uint8_t* d_in, const PassArrays& m,
               hipStream_t stream);
void lay_dict_pass(PassArrays& m, const FramesIndex& ix, size_t lo, size_t hi, uint64_t total, uint64_t in_len,
                   const DictCtx& dc, uint64_t* h_kind, hipStream_t stream);

// The seek index a compress call writes while it compresses (DESIGN.md §22;
// bodies and comments in lz4ada_bulk_ranges.cpp, the caller is
// lz4ada_bulk_compress.cpp).  comp_index_open: the index's two device blocks,
// sized for every frame taken, and the dictionary's image queued on s; n may be
// 0 (no device call).  A pass queues launch_compress_index with `out`, `base`
// and its settings and hands its records (hi - lo + 1) to comp_index_pass after
// its synchronisation.  comp_index_close: in_len, the frames' report (frames may
// be null) and the index, which the sink owns until then.
struct CompIndexSink {
	lz4ada_seek_index* x = nullptr;
	CompIndexOut out{};
	CompIndexRec base{};  // the totals after the passes so far
	bool linked = false, no_lone = false;
	uint64_t every = 0;  // decoded bytes between checkpoints
	uint32_t kind = 0;   // the CHAIN_KIND_* of a taken frame with blocks
	CompIndexSink() = default;
	CompIndexSink(const CompIndexSink&) = delete;
	CompIndexSink& operator=(const CompIndexSink&) = delete;
	~CompIndexSink();
};
// checkpoint_bytes of lz4ada_seek_options as decoded bytes between checkpoints (0: the default).
uint64_t seek_checkpoint_every(int64_t checkpoint_bytes);
void comp_index_open(CompIndexSink& k, const lz4ada_compress_job* jobs, size_t n, uint32_t block_id, bool linked,
                     int64_t checkpoint_bytes, const lz4ada_compress_dict* cdict, hipStream_t s);
void comp_index_pass(CompIndexSink& k, const lz4ada_compress_job* jobs, size_t lo, size_t hi, uint32_t block_id,
                     const CompIndexRec* rec);
lz4ada_seek_index* comp_index_close(CompIndexSink& k, const lz4ada_compress_job* jobs, int64_t out_len,
                                    lz4ada_device_frame_job* frames, hipStream_t s);

// A C-ABI call: the reference's exception as the status code, its text in
// *err (the context's) and in the thread's last error.
template <class F>
inline int guarded(std::string* err, F&& f)
{
	try {
		f();
		if (err)
			err->clear();
		return LZ4ADA_OK;
	} catch (const Error& e) {
		if (err)
			*err = e.msg;
		set_thread_error(e.msg);
		return e.code;
	} catch (const std::bad_alloc&) {
		if (err)
			*err = "out of host memory";
		set_thread_error("out of host memory");
		return LZ4ADA_CONSTRAINT_ERROR;
	}
}

}  // namespace lz4ada
