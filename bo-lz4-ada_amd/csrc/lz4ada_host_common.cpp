// lz4ada_host_common.cpp -- the one home of what lz4ada_host_common.h
// declares: the process-wide device / pinned memory pools and the stream
// pool (one instance each, whichever unit asks), the calling thread's last
// error and path bits, the frame header parser (lib/lz4ada.adb:155-375), the
// host XXH32 chain, the device-status -> exception map, the lone-block batch
// and the bulk paths' small helpers.
#include "lz4ada_frame_walk.h"
#include "lz4ada_host_common.h"

#include <future>

namespace lz4ada {

// ------------------------------------------------------------ thread state

// The calling thread's message for lz4ada_thread_last_error() and the
// LZ4ADA_PATH_* bits of its last lz4ada_decode_* call (lz4ada_last_path()).
static thread_local std::string g_thread_error;
static thread_local int g_last_path = 0;

void set_thread_error(const std::string& msg) { g_thread_error = msg; }
void set_last_path(int bits) { g_last_path = bits; }
void add_last_path(int bits) { g_last_path |= bits; }

// ------------------------------------------------------------------ errors

static std::string hex8(uint32_t v)
{
	char b[8];
	snprintf(b, sizeof b, "%02x", v & 0xffu);
	return b;
}
std::string hex32(uint32_t v)
{
	char b[16];
	snprintf(b, sizeof b, "%08x", v);
	return b;
}

void device_check_or_raise()
{
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0)
		raise(LZ4ADA_DEVICE_ERROR,
		      "no usable HIP device: the LZ4Ada MI355X decoder has no CPU fallback");
}

// ------------------------------------------------------------ memory pools

MemPool& dev_pool()
{
	static MemPool* p = new MemPool(false);  // never destroyed: process lifetime
	return *p;
}
MemPool& pin_pool()
{
	static MemPool* p = new MemPool(true);
	return *p;
}

size_t MemPool::keep_limit()
{
	static const size_t k = [] {
		const char* e = getenv("LZ4ADA_POOL_KEEP_MB");
		return e ? size_t(strtoull(e, nullptr, 10)) << 20 : size_t(1) << 30;
	}();
	return k;
}

size_t MemPool::size_class(size_t b)
{
	size_t c = 4096;
	while (c < b)
		c <<= 1;
	return c;
}

void MemPool::raw_free(void* p) { (void)(pinned ? hipHostFree(p) : hipFree(p)); }

MemPool::Block MemPool::get(size_t bytes)
{
	int dev = 0;
	(void)hipGetDevice(&dev);
	const int key = pinned ? 0 : dev;
	const size_t c = bytes <= POOL_MAX ? size_class(bytes) : bytes;
	if (c <= POOL_MAX) {
		std::lock_guard<std::mutex> l(mu);
		for (size_t i = 0; i < free.size(); ++i)
			if (std::get<0>(free[i]) == key && std::get<1>(free[i]) == c) {
				void* p = std::get<2>(free[i]);
				free[i] = free.back();
				free.pop_back();
				kept -= c;
				return { p, c, dev };
			}
	}
	void* p = nullptr;
	hipError_t e = pinned ? hipHostMalloc(&p, c, hipHostMallocDefault) : hipMalloc(&p, c);
	if (e != hipSuccess) {  // the pool's idle blocks first, then once more
		(void)hipGetLastError();
		release_all();
		e = pinned ? hipHostMalloc(&p, c, hipHostMallocDefault) : hipMalloc(&p, c);
	}
	HIP_OK(e);
	return { p, c, dev };
}

void MemPool::put(void* p, size_t c, int dev)
{
	if (!p)
		return;
	// the implicit synchronisation of the hipFree this replaces, on the
	// block's own device
	int cur = 0;
	(void)hipGetDevice(&cur);
	if (cur != dev)
		(void)hipSetDevice(dev);
	const bool synced = hipDeviceSynchronize() == hipSuccess;
	if (cur != dev)
		(void)hipSetDevice(cur);
	if (c > POOL_MAX || c != size_class(c) || !synced) {
		raw_free(p);
		return;
	}
	std::lock_guard<std::mutex> l(mu);
	if (kept + c > keep_limit()) {
		raw_free(p);
		return;
	}
	free.emplace_back(pinned ? 0 : dev, c, p);
	kept += c;
}

void MemPool::release_all()
{
	std::lock_guard<std::mutex> l(mu);
	int cur = 0;
	(void)hipGetDevice(&cur);
	for (auto& f : free) {
		if (!pinned)
			(void)hipSetDevice(std::get<0>(f));
		raw_free(std::get<2>(f));
	}
	if (!pinned)
		(void)hipSetDevice(cur);
	free.clear();
	kept = 0;
}

// ------------------------------------------------------------- stream pool

static std::mutex g_stream_mu;
static std::vector<StreamSet>& stream_pool()
{
	static std::vector<StreamSet>* v = new std::vector<StreamSet>;  // process lifetime
	return *v;
}

static void destroy_streams(const StreamSet& s)
{
	if (s.side)
		(void)hipStreamDestroy(s.side);
	if (s.ev)
		(void)hipEventDestroy(s.ev);
	if (s.stream)
		(void)hipStreamDestroy(s.stream);
}

bool take_streams(int device, StreamSet& s)
{
	{
		std::lock_guard<std::mutex> l(g_stream_mu);
		auto& pool = stream_pool();
		for (size_t i = 0; i < pool.size(); ++i)
			if (pool[i].device == device) {
				s = pool[i];
				pool[i] = pool.back();
				pool.pop_back();
				return true;
			}
	}
	StreamSet n;
	n.device = device;
	if (hipStreamCreateWithFlags(&n.stream, hipStreamNonBlocking) != hipSuccess ||
	    hipStreamCreateWithFlags(&n.side, hipStreamNonBlocking) != hipSuccess ||
	    hipEventCreateWithFlags(&n.ev, hipEventDisableTiming) != hipSuccess) {
		destroy_streams(n);
		return false;
	}
	s = n;
	return true;
}

void give_streams(const StreamSet& s)
{
	// idle streams go back to the pool for the next context
	const bool idle = hipStreamSynchronize(s.side) == hipSuccess && hipStreamSynchronize(s.stream) == hipSuccess;
	if (idle) {
		std::lock_guard<std::mutex> l(g_stream_mu);
		stream_pool().push_back(s);
	} else {
		destroy_streams(s);
	}
}

void destroy_idle_streams()
{
	std::vector<StreamSet> sets;
	{
		std::lock_guard<std::mutex> l(g_stream_mu);
		sets.swap(stream_pool());
	}
	int cur = 0;
	(void)hipGetDevice(&cur);
	for (auto& x : sets) {
		(void)hipSetDevice(x.device);
		destroy_streams(x);
	}
	(void)hipSetDevice(cur);
}

// ------------------------------------------------------------------ worker

Worker::~Worker()
{
	{
		std::lock_guard<std::mutex> l(mu);
		stop = true;
	}
	cv.notify_one();
	if (th.joinable())
		th.join();
}

void Worker::submit(std::function<void()> f)
{
	wait();
	if (!th.joinable())
		th = std::thread([this] { loop(); });
	{
		std::lock_guard<std::mutex> l(mu);
		job = std::move(f);
		busy = true;
	}
	cv.notify_one();
}

void Worker::wait()
{
	std::unique_lock<std::mutex> l(mu);
	done_cv.wait(l, [this] { return !busy; });
}

void Worker::loop()
{
	std::unique_lock<std::mutex> l(mu);
	for (;;) {
		cv.wait(l, [this] { return (busy && job) || stop; });
		if (!(busy && job))
			return;  // stop, nothing pending
		std::function<void()> f = std::move(job);
		job = nullptr;
		l.unlock();
		f();
		l.lock();
		busy = false;
		done_cv.notify_all();
	}
}

// ----------------------------------------------------------- header parser

static const char* const RES_IMAGE[] = { "SZ_64_KIB", "SZ_256_KIB", "SZ_1_MIB",    "SZ_4_MIB",
	                                 "SZ_8_MIB",  "USE_FIRST",  "SINGLE_FRAME" };

static uint64_t load64(const uint8_t* p) { return uint64_t(load32(p)) | (uint64_t(load32(p + 4)) << 32); }

// XXH32 of the 2..14-byte frame descriptor for the header checksum byte
// (lz4ada.adb:351-361).  Framing, not block data: it runs on the host.
static uint32_t descriptor_xxh32(const uint8_t* p, size_t n)
{
	auto rotl = [](uint32_t x, int r) { return (x << r) | (x >> (32 - r)); };
	uint32_t h = uint32_t(n) + P5;  // n < 16: no stripes
	size_t d = 0;
	for (; d + 4 <= n; d += 4)
		h = rotl(h + load32(p + d) * P3, 17) * P4;
	for (; d < n; ++d)
		h = rotl(h + uint32_t(p[d]) * P5, 11) * P1;
	h = (h ^ (h >> 15)) * P2;
	h = (h ^ (h >> 13)) * P3;
	return h ^ (h >> 16);
}

int64_t block_size_of(int r)  // Get_Block_Size, lz4ada.adb:65-77
{
	static const int64_t lut[] = { 64 << 10, 256 << 10, 1 << 20, 4 << 20, 8 << 20 };
	return lut[r];
}

static void check_reservation(int requested, int& effective)  // lz4ada.adb:241-260
{
	if (concrete(requested)) {
		if (effective > requested)
			raise(LZ4ADA_TOO_LITTLE_MEMORY,
			      std::string("LZ4 header requres reservation ") + RES_IMAGE[effective] +
			              ", but API call requested that only " + RES_IMAGE[requested] +
			              " be used. This frame cannot be processed under the given "
			              "constraints.");
		effective = requested;
	}
}

static void legacy_end_of_header(Meta& m)  // lz4ada.adb:225-239
{
	int eff = LZ4ADA_FOR_LEGACY;
	m.input_buffer_filled = 0;
	m.is_format = F_LEGACY;
	m.header_parsing = HDR_DONE;
	m.size_remaining = 0;
	m.status_eof = LZ4ADA_EOF_MAYBE;
	m.block_checksum_length = 0;
	m.content_checksum_length = 0;
	m.has_content_size = false;
	m.is_compressed = true;
	check_reservation(m.memory_reservation, eff);
	m.memory_reservation = eff;
}

void header_magic(Meta& m, uint32_t magic)  // lz4ada.adb:199-223
{
	if (magic == MAGIC_MODERN) {
		m.is_format = F_MODERN;
		m.header_parsing = NEED_FLAGS;
		m.size_remaining = 2;
	} else if (magic == MAGIC_LEGACY) {
		legacy_end_of_header(m);
	} else if (magic >= MAGIC_SKIP_LO && magic <= MAGIC_SKIP_HI) {
		m.is_format = F_SKIPPABLE;
		m.header_parsing = NEED_SKIP_LEN;
		m.size_remaining = 4;
		m.block_checksum_length = 0;
		m.content_checksum_length = 0;
	} else {
		raise(LZ4ADA_NOT_SUPPORTED, "Invalid or unsupported magic: 0x" + hex32(magic));
	}
}

static void header_flags(Meta& m, const uint8_t* hb)  // lz4ada.adb:262-328
{
	const uint8_t flg = hb[4], bd = hb[5];
	const unsigned version = (flg & 0xc0u) >> 6, bmax = (bd & 0x70u) >> 4;
	if (version != 1)
		raise(LZ4ADA_NOT_SUPPORTED, "Only LZ4 frame format version 01 supported. Detected 0x" +
		                                    hex8(version) + " instead.");
	if ((flg & 2u) || (bd & 0x8fu))
		raise(LZ4ADA_NOT_SUPPORTED,
		      "Found reserved bits /= 0. Data might be too new to be processed by this "
		      "implementation!");
	m.status_eof = LZ4ADA_EOF_NO;
	int required;
	switch (bmax) {
	case 4: required = LZ4ADA_SZ_64_KIB; break;
	case 5: required = LZ4ADA_SZ_256_KIB; break;
	case 6: required = LZ4ADA_SZ_1_MIB; break;
	case 7: required = LZ4ADA_SZ_4_MIB; break;
	default: raise(LZ4ADA_NOT_SUPPORTED, "Unknown maximum block size flag: 0x" + hex8(bmax));
	}
	m.flg = flg;
	m.bd = bd;
	m.block_checksum_length = (flg & 16u) ? 4 : 0;
	m.content_checksum_length = (flg & 4u) ? 4 : 0;
	m.has_content_size = (flg & 8u) != 0;
	m.header_parsing = NEED_MODERN;
	m.size_remaining = 1 + (m.has_content_size ? 8 : 0) + ((flg & 1u) ? 4 : 0);
	check_reservation(m.memory_reservation, required);
	if (m.memory_reservation != LZ4ADA_SINGLE_FRAME)
		m.memory_reservation = required;
}

static void header_modern_end(Meta& m, const uint8_t* hb)  // lz4ada.adb:330-361
{
	const uint8_t hc = hb[m.input_buffer_filled - 1];
	if (m.has_content_size)
		m.size_remaining = load64(hb + 6);
	const uint8_t computed =
	        uint8_t((descriptor_xxh32(hb + 4, size_t(m.input_buffer_filled - 1 - 4)) >> 8) & 0xffu);
	if (hc != computed)
		raise(LZ4ADA_CHECKSUM_ERROR, "Computed Header Checksum 0x" + hex8(computed) +
		                                     " does not match expected Header Checksum 0x" +
		                                     hex8(hc));
	m.header_parsing = HDR_DONE;
	m.input_buffer_filled = 0;
}

// Process_Header_Bytes (lz4ada.adb:155-191)
int64_t header_bytes(Meta& m, uint8_t* hb, const uint8_t* in, int64_t len)
{
	const int64_t copy = std::min<int64_t>(len, int64_t(m.size_remaining));
	if (!(copy > 0))
		raise(LZ4ADA_ASSERTION_ERROR, "lz4ada.adb:161");
	memcpy(hb + m.input_buffer_filled, in, size_t(copy));
	m.input_buffer_filled += copy;
	m.size_remaining -= uint64_t(copy);
	if (m.size_remaining == 0) {
		switch (m.header_parsing) {
		case NEED_MAGIC: header_magic(m, load32(hb)); break;
		case NEED_FLAGS: header_flags(m, hb); break;
		case NEED_MODERN: header_modern_end(m, hb); break;
		case NEED_SKIP_LEN:
			m.memory_reservation = LZ4ADA_SZ_64_KIB;  // quirk Q3
			m.header_parsing = HDR_DONE;
			m.size_remaining = load32(hb + 4);
			m.status_eof = m.size_remaining == 0 ? LZ4ADA_EOF_YES : LZ4ADA_EOF_NO;
			m.input_buffer_filled = 0;
			break;
		default:
			raise(LZ4ADA_CONSTRAINT_ERROR,
			      "Header_Complete case must not be reached while processing header bytes. "
			      "Library bug detected.");
		}
	}
	return copy;
}

bool is_any_magic(uint32_t v)
{
	return v == MAGIC_MODERN || v == MAGIC_LEGACY || (v >= MAGIC_SKIP_LO && v <= MAGIC_SKIP_HI);
}

// -------------------------------------------------------------- host XXH32

static inline uint32_t rotl32h(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static inline uint32_t xxh_round(uint32_t acc, uint32_t w) { return rotl32h(acc + w * P2, 13) * P1; }

void host_xxh32_update(lz4ada_xxh32_state& h, const uint8_t* p, size_t n)
{
	h.total_length += n;
	size_t bs = size_t(h.buffer_size);
	if (bs + n < 16) {
		if (n)
			memcpy(h.buffer + bs, p, n);
		h.buffer_size = int32_t(bs + n);
		return;
	}
	if (bs) {  // complete the buffered stripe (Update1, :965-991)
		const size_t k = 16 - bs;
		memcpy(h.buffer + bs, p, k);
		p += k;
		n -= k;
		for (int i = 0; i < 4; ++i)
			h.state[i] = xxh_round(h.state[i], load32(h.buffer + 4 * i));
	}
	uint32_t v0 = h.state[0], v1 = h.state[1], v2 = h.state[2], v3 = h.state[3];
	for (; n >= 16; p += 16, n -= 16) {  // stripes (Process, :951-958)
		v0 = xxh_round(v0, load32(p));
		v1 = xxh_round(v1, load32(p + 4));
		v2 = xxh_round(v2, load32(p + 8));
		v3 = xxh_round(v3, load32(p + 12));
	}
	h.state[0] = v0;
	h.state[1] = v1;
	h.state[2] = v2;
	h.state[3] = v3;
	if (n)
		memcpy(h.buffer, p, n);
	h.buffer_size = int32_t(n);
}

uint32_t host_xxh32_final(const lz4ada_xxh32_state& h)  // :993-1017
{
	uint32_t acc = h.total_length >= 16 ? rotl32h(h.state[0], 1) + rotl32h(h.state[1], 7) +
	                                          rotl32h(h.state[2], 12) + rotl32h(h.state[3], 18)
	                                    : h.state[2] + P5;
	acc += uint32_t(h.total_length);
	const uint8_t* p = h.buffer;
	size_t n = size_t(h.buffer_size);
	for (; n >= 4; p += 4, n -= 4)
		acc = rotl32h(acc + load32(p) * P3, 17) * P4;
	for (; n; ++p, --n)
		acc = rotl32h(acc + uint32_t(*p) * P5, 11) * P1;
	acc ^= acc >> 15;
	acc *= P2;
	acc ^= acc >> 13;
	acc *= P3;
	acc ^= acc >> 16;
	return acc;
}

// Device status of a decode kernel -> the reference's exception.
void raise_device_status(const SerialState& s)
{
	switch (s.code) {
	case DS_OFFSET0: raise(LZ4ADA_DATA_CORRUPTION, "Corrupted Block: Offset = 0 detected.");
	case DS_ML_AFTER_LIT:
		raise(LZ4ADA_DATA_CORRUPTION,
		      "Match_Length=" + img(s.aux) +
		              " suggests compressed data but this sequence already ends after the "
		              "literals. This might also happen with an untypical encoder?");
	case DS_LIT_OVERRUN:
		raise(LZ4ADA_DATA_CORRUPTION, "Corrupted Block: literal run exceeds the end of the block.");
	case DS_TRUNCATED:
		raise(LZ4ADA_DATA_CORRUPTION,
		      "Corrupted Block: sequence truncated at the end of the block.");
	case DS_OUT_OVERFLOW:
		raise(LZ4ADA_DATA_CORRUPTION,
		      "Corrupted Block: decompressed data exceeds the output buffer.");
	case DS_BACKREF:
		raise(LZ4ADA_DATA_CORRUPTION, "Backreference location out of range. Read from offset " +
		                                      img(s.detail) +
		                                      " not possible (earliest available index is 0).");
	case DS_CONTENT_SIZE:
		raise(LZ4ADA_DATA_CORRUPTION,
		      "Produced content size exceeds declared content size. The supplied data is "
		      "inconsistent.");
	default: raise(LZ4ADA_CONSTRAINT_ERROR, "unexpected device status " + std::to_string(s.code));
	}
}

// ------------------------------------------------ bulk-path device helpers

ScratchCache& scratch_cache()
{
	static thread_local ScratchCache* c = new ScratchCache;
	return *c;
}

uint8_t* scratch(int role, size_t bytes)
{
	DevBuf<uint8_t>& d = scratch_cache().b[role];
	return try_reserve(d, bytes) ? d.p : nullptr;
}

int64_t env_bytes(const char* name, int64_t dflt)
{
	const char* e = getenv(name);
	if (!e || !*e)
		return dflt;
	const long long v = atoll(e);
	return v > 0 ? int64_t(v) : dflt;
}

bool lone_blocks_disabled()
{
	static const bool off = getenv("LZ4ADA_NO_LONE") != nullptr;
	return off;
}

bool few_large_blocks(const std::vector<lz4ada_block_desc>& d)
{
	if (lone_blocks_disabled() || d.empty() || d.size() > size_t(WALK_LONE_BLOCKS))
		return false;
	uint32_t mx = 0;
	for (const auto& x : d)
		mx = std::max(mx, x.in_len);
	return mx >= WALK_LONE_MIN_IN && int64_t(mx) <= LONE_MAX_IN;
}

bool decode_lone_blocks(const uint8_t* host_in, const uint8_t* d_in,
                        const std::vector<lz4ada_block_desc>& d, uint8_t* d_out,
                        lz4ada_block_status* d_st, std::vector<lz4ada_block_status>& st,
                        DevBuf<uint8_t>& scr, hipStream_t stream)
{
	const size_t nb = d.size();
	int64_t sb = 0;
	for (const auto& x : d) {
		if (x.flags & LZ4ADA_BLOCK_STORED) {
			if (x.in_len > x.out_cap)
				return false;
		} else {
			if (x.in_len == 0)
				return false;
			sb = std::max(sb, lone_scratch_bytes(x.in_len, x.out_cap));
		}
	}
	if (sb && !try_reserve(scr, size_t(sb)))
		return false;
	HIP_OK(hipMemsetAsync(d_st, 0, nb * sizeof(lz4ada_block_status), stream));
	for (size_t i = 0; i < nb; ++i) {
		const auto& x = d[i];
		if (x.flags & LZ4ADA_BLOCK_STORED) {
			if (x.in_len)
				HIP_OK(hipMemcpyAsync(d_out + x.out_off, d_in + x.in_off, x.in_len,
				                      hipMemcpyDeviceToDevice, stream));
		} else {
			HIP_OK(launch_decode_lone(d_in + x.in_off, x.in_len, d_out + x.out_off, x.out_cap,
			                          d_st + i, scr.p, sb, stream));
		}
	}
	std::vector<std::future<uint32_t>> ck(nb);
	for (size_t i = 0; i < nb; ++i)
		if (d[i].flags & LZ4ADA_BLOCK_HAS_CKSUM) {
			const uint8_t* p = host_in + d[i].in_off;
			const size_t n = d[i].in_len;
			ck[i] = std::async(std::launch::async, [p, n] {
				lz4ada_xxh32_state h;
				lz4ada_xxh32_reset(&h, 0);
				host_xxh32_update(h, p, n);
				return host_xxh32_final(h);
			});
		}
	st.assign(nb, lz4ada_block_status{});
	HIP_OK(hipMemcpyAsync(st.data(), d_st, nb * sizeof(lz4ada_block_status), hipMemcpyDeviceToHost,
	                      stream));
	HIP_OK(hipStreamSynchronize(stream));
	bool ok = true;
	for (size_t i = 0; i < nb; ++i) {
		if (d[i].flags & LZ4ADA_BLOCK_STORED) {
			st[i].code = DS_OK;
			st[i].out_len = d[i].in_len;
		}
		if (ck[i].valid())
			st[i].cksum = ck[i].get();
		if (st[i].code != DS_OK)
			ok = false;
	}
	if (ok)  // the statuses also on the device, as the bulk decoder leaves them
		HIP_OK(hipMemcpy(d_st, st.data(), nb * sizeof(lz4ada_block_status), hipMemcpyHostToDevice));
	return ok;
}

std::vector<std::pair<uint32_t, uint32_t>> batches_of(const std::vector<lz4ada_block_desc>& descs,
                                                      int64_t bmax, uint64_t extra, uint64_t budget)
{
	std::vector<std::pair<uint32_t, uint32_t>> v;
	uint32_t lo = 0;
	uint64_t acc = 0;
	for (uint32_t i = 0; i < descs.size(); ++i) {
		const uint64_t need = round256(slot_cap(descs[i], bmax)) + extra;
		if (i > lo && acc + need > budget) {
			v.emplace_back(lo, i);
			lo = i;
			acc = 0;
		}
		acc += need;
	}
	if (lo < descs.size())
		v.emplace_back(lo, uint32_t(descs.size()));
	return v;
}

void d2h(void* dst, const void* src, size_t n, hipStream_t stream)
{
	HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
}

}  // namespace lz4ada

using namespace lz4ada;

extern "C" {

const char* lz4ada_thread_last_error(void) { return g_thread_error.c_str(); }

int lz4ada_last_path(void) { return g_last_path; }

void lz4ada_release_device_cache(void)
{
	for (auto& x : scratch_cache().b)
		x.release();
	scratch_cache().pin.release();
	dev_pool().release_all();
	pin_pool().release_all();
	destroy_idle_streams();
}

void lz4ada_device_cache_stats(lz4ada_cache_stats* out)
{
	{
		std::lock_guard<std::mutex> l(dev_pool().mu);
		out->device_idle_bytes = int64_t(dev_pool().kept);
	}
	{
		std::lock_guard<std::mutex> l(pin_pool().mu);
		out->pinned_idle_bytes = int64_t(pin_pool().kept);
	}
	std::lock_guard<std::mutex> l(g_stream_mu);
	out->idle_streams = int64_t(stream_pool().size());
}

}  // extern "C"
