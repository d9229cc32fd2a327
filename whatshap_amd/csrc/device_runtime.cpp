// device_runtime.cpp -- the process-wide device runtime of device_runtime.h: pools, upload streams, staging areas, arena cache, the call
// session, and the code that empties all of them.  Host code only: no kernel lives here, so an edit recompiles none.
#include "device_runtime.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>

#include "debug_build.h"
#include "genotype.h"
#include "host_parallel.h"

namespace whamd {

whamd_status_t open_device(int device, std::string& msg) {
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		(void)hipGetLastError();
		msg = "no HIP device visible: the whatshap_amd device path needs an MI355X (gfx950); there is no CPU fallback";
		return WHAMD_ERR_DEVICE;
	}
	if (device < 0 || device >= ndev) {
		msg = "device index " + std::to_string(device) + " out of range (" + std::to_string(ndev) + " visible)";
		return WHAMD_ERR_DEVICE;
	}
	HIP_TRY(hipSetDevice(device));
	return WHAMD_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------- device pool
struct DevPool {
	std::mutex mu;
	struct Block { void* ptr; size_t bytes; int device; };
	std::vector<Block> idle;
	size_t idle_bytes = 0;
};
DevPool g_pool;
constexpr size_t POOL_KEEP = (size_t)24 << 30;   // most bytes kept idle
size_t pool_class(size_t bytes) {
	bytes = std::max<size_t>(bytes, 256);
	size_t p = 256;
	while (p < bytes) p <<= 1;
	const size_t step = std::max<size_t>(p / 8, 256);
	return (bytes + step - 1) / step * step;
}

struct HostBlock { void* ptr; size_t bytes; };
struct MiscPool {
	std::mutex mu;
	std::vector<StreamSet> streams;
	std::vector<HostBlock> pinned;
	size_t pinned_bytes = 0;
};
MiscPool g_misc;

}  // namespace

hipError_t devpool_take(int device, size_t bytes, void** out, size_t* got) {
	const size_t want = pool_class(bytes);
	*got = want;
	{
		std::lock_guard<std::mutex> lock(g_pool.mu);
		for (size_t i = 0; i < g_pool.idle.size(); ++i) {
			if (g_pool.idle[i].device != device || g_pool.idle[i].bytes != want) continue;
			*out = g_pool.idle[i].ptr;
			g_pool.idle_bytes -= want;
			g_pool.idle[i] = g_pool.idle.back();
			g_pool.idle.pop_back();
			return hipSuccess;
		}
	}
	hipError_t e = hipMalloc(out, want);
	if (e != hipSuccess) {   // out of memory with idle blocks around: give them back and try once more
		(void)hipGetLastError();
		devpool_release();
		e = hipMalloc(out, want);
	}
	return e;
}
void devpool_give(int device, void* ptr, size_t bytes) {
	if (!ptr) return;
	{
		std::lock_guard<std::mutex> lock(g_pool.mu);
		if (g_pool.idle_bytes + bytes <= POOL_KEEP && bytes <= ((size_t)2 << 30)) {
			g_pool.idle.push_back(DevPool::Block{ptr, bytes, device});
			g_pool.idle_bytes += bytes;
			return;
		}
	}
	(void)hipFree(ptr);
}
void devpool_release() {
	std::vector<DevPool::Block> blocks;
	{
		std::lock_guard<std::mutex> lock(g_pool.mu);
		blocks.swap(g_pool.idle);
		g_pool.idle_bytes = 0;
	}
	int cur = 0;
	(void)hipGetDevice(&cur);
	for (const DevPool::Block& b : blocks) { (void)hipSetDevice(b.device); (void)hipFree(b.ptr); }
	(void)hipSetDevice(cur);
}

bool streamset_take(int device, StreamSet& out) {
	{
		std::lock_guard<std::mutex> lock(g_misc.mu);
		for (size_t i = 0; i < g_misc.streams.size(); ++i) {
			if (g_misc.streams[i].device != device) continue;
			out = g_misc.streams[i];
			g_misc.streams[i] = g_misc.streams.back();
			g_misc.streams.pop_back();
			return true;
		}
	}
	out = StreamSet();
	out.device = device;
	if (hipStreamCreateWithFlags(&out.stream, hipStreamNonBlocking) != hipSuccess) return false;
	for (int k = 0; k < 6; ++k)
		if ((k < 4 ? hipEventCreate(&out.ev[k]) : hipEventCreateWithFlags(&out.ev[k], hipEventDisableTiming)) != hipSuccess) return false;
	return true;
}
void streamset_give(const StreamSet& ss) {   // (the stream is idle: the caller synchronised it)
	if (!ss.stream) return;
	std::lock_guard<std::mutex> lock(g_misc.mu);
	if (g_misc.streams.size() < 256) { g_misc.streams.push_back(ss); return; }
	for (hipEvent_t e : ss.ev) if (e) (void)hipEventDestroy(e);
	(void)hipStreamDestroy(ss.stream);
}

// The streams the UPLOADS of all tables of a device go through: two, shared, used for nothing else.  A table's own stream carries its solve; an upload that went
// through it completed, under a running group solve, only when that solve's queue had drained: the staging areas came back late and 96 creates under a running solve
// took 137 - 190 ms instead of 81 - 93 ms alone (scripts/gpu_create_under_solve.py); on streams of their own: 72 - 101 ms.
namespace {
struct UploadStreams {
	std::mutex mu;
	std::vector<std::pair<int, hipStream_t>> streams;   // (device, stream); never destroyed: they live as long as the process
	std::atomic<uint32_t> next{0};
};
UploadStreams g_upload_streams;
constexpr uint32_t UPLOAD_STREAMS = 2;   // (creating one costs ~10 ms, paid by the first creates of a process; the link serialises the copies anyway)
}  // namespace
hipStream_t upload_stream_of(int device) {
	const uint32_t slot = g_upload_streams.next.fetch_add(1, std::memory_order_relaxed) % UPLOAD_STREAMS;
	std::lock_guard<std::mutex> lock(g_upload_streams.mu);
	uint32_t seen = 0;
	for (const auto& e : g_upload_streams.streams)
		if (e.first == device && seen++ == slot) return e.second;
	hipStream_t made = nullptr;
	while (seen <= slot) {
		int least = 0, greatest = 0;
		(void)hipDeviceGetStreamPriorityRange(&least, &greatest);
		hipStream_t st = nullptr;
		// (default priority.  Streams of the HIGHEST priority -- debug library, WHAMD_UPLOAD_STREAMS_HIGH=1 -- were the first version: the creates under a running solve
		//  gained the same, but the mere existence of such streams made three full-width tables solved at once on their own streams 3.2 x slower, 177 ms against 55:
		//  scripts/gpu_wide_tables_concurrent.py)
		const bool high = debug_env("WHAMD_UPLOAD_STREAMS_HIGH") != nullptr;
		if ((high ? hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		g_upload_streams.streams.emplace_back(device, st);
		made = st;
		++seen;
	}
	return made;
}
hipError_t pinned_take(size_t bytes, void** out, size_t* got) {
	const size_t want = pool_class(bytes);
	*got = want;
	{
		std::lock_guard<std::mutex> lock(g_misc.mu);
		for (size_t i = 0; i < g_misc.pinned.size(); ++i) {
			if (g_misc.pinned[i].bytes != want) continue;
			*out = g_misc.pinned[i].ptr;
			g_misc.pinned_bytes -= want;
			g_misc.pinned[i] = g_misc.pinned.back();
			g_misc.pinned.pop_back();
			return hipSuccess;
		}
	}
	return hipHostMalloc(out, want, hipHostMallocPortable);
}
void pinned_give(void* ptr, size_t bytes) {
	if (!ptr) return;
	{
		std::lock_guard<std::mutex> lock(g_misc.mu);
		if (g_misc.pinned_bytes + bytes <= ((size_t)1 << 30)) { g_misc.pinned.push_back(HostBlock{ptr, bytes}); g_misc.pinned_bytes += bytes; return; }
	}
	(void)hipHostFree(ptr);
}

// ---------------------------------------------------------------------------------------------- pinned staging of the create path
// hipMemcpyAsync from pageable memory goes through the runtime's own small staging buffers: ~5 GB/s measured for the ~100 MB of
// descriptors of a configs[2] table, 20 ms of a 58 ms create.  The create path copies its large arrays into ONE process-wide pinned
// area with a few host threads and sends them from there (the copies overlap the host work that follows).  One upload() at a
// time owns the area; it grows to what the largest table so far needed (at most STAGE_MAX; larger uploads go in rounds).
namespace {
struct UploadStage {
	std::mutex mu;
	struct Area { char* base = nullptr; size_t cap = 0; bool busy = false; hipEvent_t ev = nullptr; bool parked = false; };   // parked: the last session left copies in flight, `ev` says when they are done
	std::vector<Area> areas;   // a few pinned areas: tables created by several host threads at once (blocks.solve_blocks) do not wait for each other
	size_t want = 0;
	bool broken = false;   // hipHostMalloc failed once: pageable copies from then on
};
UploadStage g_stage;
constexpr size_t STAGE_MIN_COPY = (size_t)256 << 10, STAGE_GRAIN = (size_t)16 << 20, STAGE_AREAS = 32;   // (eight areas: the ninth and later of 64 concurrent creates fell back to pageable copies, 9.5 GB/s and synchronous)
}  // namespace
StageSession::StageSession(hipStream_t s) : stream(s), enabled(debug_env("WHAMD_NO_PINNED_STAGE") == nullptr) {
	std::lock_guard<std::mutex> lock(g_stage.mu);
	size_t best = g_stage.areas.size();
	for (size_t i = 0; i < g_stage.areas.size(); ++i)
		if (!g_stage.areas[i].busy && (best == g_stage.areas.size() || (g_stage.areas[best].parked && !g_stage.areas[i].parked) ||
		                               (g_stage.areas[best].parked == g_stage.areas[i].parked && g_stage.areas[i].cap > g_stage.areas[best].cap))) best = i;
	if (best == g_stage.areas.size() && g_stage.areas.size() < STAGE_AREAS) { g_stage.areas.emplace_back(); best = g_stage.areas.size() - 1; }
	hipEvent_t wait_for = nullptr;
	if (best != g_stage.areas.size()) {
		slot = (int)best;
		g_stage.areas[best].busy = true;
		base = g_stage.areas[best].base;
		cap = g_stage.areas[best].cap;
		if (g_stage.areas[best].parked) wait_for = g_stage.areas[best].ev;
		g_stage.areas[best].parked = false;
	}
	if (wait_for) (void)hipEventSynchronize(wait_for);   // (the previous table's copies out of this area: normally long done)
}
bool StageSession::park() {
	if (slot < 0 || !pending) return true;
	std::lock_guard<std::mutex> lock(g_stage.mu);
	UploadStage::Area& a = g_stage.areas[slot];
	if (!a.ev && hipEventCreateWithFlags(&a.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); a.ev = nullptr; return false; }
	if (hipEventRecord(a.ev, stream) != hipSuccess) { (void)hipGetLastError(); return false; }
	a.parked = true;
	pending = false;
	used = 0;
	return true;
}
StageSession::~StageSession() {
	if (pending) (void)hipStreamSynchronize(stream);
	std::lock_guard<std::mutex> lock(g_stage.mu);
	g_stage.want = std::max(g_stage.want, std::min(total, STAGE_MAX));
	if (slot >= 0) {
		g_stage.areas[slot].base = base;
		g_stage.areas[slot].cap = cap;
		g_stage.areas[slot].busy = false;
	}
}
bool StageSession::ensure(size_t bytes) {
	if (slot < 0) return false;
	size_t want = 0;
	{
		std::lock_guard<std::mutex> lock(g_stage.mu);
		want = g_stage.want;
	}
	const size_t need = (std::max(std::min(bytes, STAGE_MAX), want) + STAGE_GRAIN - 1) / STAGE_GRAIN * STAGE_GRAIN;
	if (cap >= need) return true;
	if (base) (void)hipHostFree(base);
	base = nullptr;
	cap = 0;
	void* ptr = nullptr;
	if (hipHostMalloc(&ptr, need, hipHostMallocPortable) != hipSuccess) {
		(void)hipGetLastError();
		g_stage.broken = true;
		return false;
	}
	base = (char*)ptr;
	cap = need;
	return true;
}
hipError_t StageSession::copy(void* dst, const void* src, size_t bytes) {
	if (!enabled || g_stage.broken || slot < 0 || bytes < STAGE_MIN_COPY || image) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
	total += (bytes + 255) & ~(size_t)255;
	size_t done = 0;
	while (done < bytes) {
		if (!pending && used == 0 && !ensure(bytes - done)) return hipMemcpyAsync((char*)dst + done, (const char*)src + done, bytes - done, hipMemcpyHostToDevice, stream);
		const size_t chunk = std::min(bytes - done, cap - used);
		if (chunk == 0) {   // area full: wait for what is in flight, start over
			hipError_t e = hipStreamSynchronize(stream);
			if (e != hipSuccess) return e;
			pending = false;
			used = 0;
			continue;
		}
		char* at = base + used;
		const char* from = (const char*)src + done;
		parallel_ranges(chunk, host_threads(chunk, (size_t)2 << 20), [&](uint64_t b0, uint64_t b1, uint32_t) { std::memcpy(at + b0, from + b0, b1 - b0); });
		hipError_t e = hipMemcpyAsync((char*)dst + done, at, chunk, hipMemcpyHostToDevice, stream);
		if (e != hipSuccess) return e;
		pending = true;
		used += (chunk + 255) & ~(size_t)255;
		done += chunk;
	}
	return hipSuccess;
}
bool StageSession::begin_image(size_t bytes) {
	if (!enabled || g_stage.broken || slot < 0 || pending || used != 0) return false;
	image = ensure(bytes);
	return image;
}
void StageSession::expect(size_t bytes) {
	std::lock_guard<std::mutex> lock(g_stage.mu);
	g_stage.want = std::max(g_stage.want, std::min(bytes, STAGE_MAX));
}

// ---------------------------------------------------------------------------------------------- arenas kept between tables
// hipFree + hipMalloc of a 13 GB backtrace arena per table stalls for up to a second every few tables (measured: create 26 ms,
// 26 ms, 26 ms, 997 ms; 24 tables of 100 000 columns created and released one after the other: 50 - 100 ms each).  The arenas of closed
// tables stay allocated (a few blocks per process, at most 60 % of the device); the next table takes the smallest one that is large enough
// and not wastefully large.  Counted as free memory when a table sizes its arena; given back when memory is tight.
namespace {
struct ArenaCache {
	std::mutex mu;
	struct Block { void* ptr; size_t bytes; int device; };
	std::vector<Block> blocks;
};
ArenaCache g_arena;
constexpr size_t ARENA_BLOCKS = 512;   // (32 until round 6: the 96 tables of one step kept 32 arenas and hipFree-d 64 -- 13 ms of their releases -- and the next step allocated them again; the bytes are bounded separately, arena_give)
void arena_free_block(const ArenaCache::Block& b) {
	int cur = 0;
	(void)hipGetDevice(&cur);
	(void)hipSetDevice(b.device);
	(void)hipFree(b.ptr);
	(void)hipSetDevice(cur);
}
}  // namespace
size_t arena_idle_bytes(int device) {
	std::lock_guard<std::mutex> lock(g_arena.mu);
	size_t sum = 0;
	for (const ArenaCache::Block& b : g_arena.blocks) if (b.device == device) sum += b.bytes;
	return sum;
}
void* arena_take(int device, size_t need, size_t& got, bool make_room) {
	std::vector<ArenaCache::Block> drop;
	void* out = nullptr;
	{
		std::lock_guard<std::mutex> lock(g_arena.mu);
		size_t best = g_arena.blocks.size();
		for (size_t i = 0; i < g_arena.blocks.size(); ++i) {
			const ArenaCache::Block& b = g_arena.blocks[i];
			if (b.device != device || b.bytes < need || b.bytes > 2 * need + ((size_t)1 << 30)) continue;
			if (best == g_arena.blocks.size() || b.bytes < g_arena.blocks[best].bytes) best = i;
		}
		if (best != g_arena.blocks.size()) {
			out = g_arena.blocks[best].ptr;
			got = g_arena.blocks[best].bytes;
			g_arena.blocks[best] = g_arena.blocks.back();
			g_arena.blocks.pop_back();
		} else if (make_room) {
			// nothing fits: the allocation that follows must not fail because of idle blocks -- free them when they are needed
			size_t free_b = 0, total_b = 0;
			if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)4 << 30)) drop.swap(g_arena.blocks);
		}
	}
	for (const ArenaCache::Block& b : drop) arena_free_block(b);
	return out;
}
void arena_give(int device, void* ptr, size_t bytes) {   // called with `device` current
	if (!ptr) return;
	{
		std::lock_guard<std::mutex> lock(g_arena.mu);
		size_t idle = 0, total_b = 0, free_b = 0;
		for (const ArenaCache::Block& b : g_arena.blocks) idle += b.bytes;
		const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && idle + bytes <= total_b / 5 * 3;   // (eight trio tables of 100 000 columns: 8 x 15 GB)
		if (room && g_arena.blocks.size() < ARENA_BLOCKS && bytes >= ((size_t)32 << 20) && debug_env("WHAMD_NO_ARENA_CACHE") == nullptr) {
			g_arena.blocks.push_back(ArenaCache::Block{ptr, bytes, device});
			return;
		}
	}
	(void)hipFree(ptr);
}

void arena_release() {
	std::vector<ArenaCache::Block> blocks;
	{
		std::lock_guard<std::mutex> lock(g_arena.mu);
		blocks.swap(g_arena.blocks);
	}
	for (const ArenaCache::Block& b : blocks) arena_free_block(b);
}

namespace {
void misc_pool_release() {
	std::vector<StreamSet> streams;
	std::vector<HostBlock> pinned;
	{
		std::lock_guard<std::mutex> lock(g_misc.mu);
		streams.swap(g_misc.streams);
		pinned.swap(g_misc.pinned);
		g_misc.pinned_bytes = 0;
	}
	int cur = 0;
	(void)hipGetDevice(&cur);
	for (const StreamSet& ss : streams) {
		(void)hipSetDevice(ss.device);
		for (hipEvent_t e : ss.ev) if (e) (void)hipEventDestroy(e);
		(void)hipStreamDestroy(ss.stream);
	}
	(void)hipSetDevice(cur);
	for (const HostBlock& b : pinned) (void)hipHostFree(b.ptr);
}

void stage_release() {
	std::lock_guard<std::mutex> lock(g_stage.mu);
	for (UploadStage::Area& a : g_stage.areas) {
		if (a.busy) continue;   // (an upload in flight on another thread keeps its area)
		if (a.parked && a.ev) (void)hipEventSynchronize(a.ev);   // (copies of a finished create may still be reading it)
		a.parked = false;
		if (a.base) (void)hipHostFree(a.base);
		a.base = nullptr;
		a.cap = 0;
	}
	g_stage.want = 0;
}
}  // namespace

void device_release_caches() {
	genotype_release_cache();
	devpool_release();
	arena_release();
	misc_pool_release();
	stage_release();
}

// ---------------------------------------------------------------------------------------------- one call on one device
whamd_status_t Session::open(int dev_index, int n_events, std::string& msg) {
	WHAMD_TRY(open_device(dev_index, msg));
	device = dev_index;
	HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
	ev.reserve(n_events);
	for (int k = 0; k < n_events; ++k) {
		hipEvent_t e = nullptr;
		HIP_TRY(hipEventCreate(&e));
		ev.push_back(e);
	}
	timed = n_events == 4;
	return WHAMD_OK;
}
namespace {
enum CallEvent { UPLOAD_BEGIN, UPLOAD_END, KERNELS_END, DOWNLOAD_END };   // what ev[0 .. 3] of a timed session mark
double ms_between(hipEvent_t a, hipEvent_t b) {
	float t = 0.0f;
	return hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0;
}
}  // namespace
whamd_status_t Session::work(const ImageLayout& layout, Image& image, std::string& msg) {
	image.total = layout.total;
	return device_block(layout.total, (void**)&image.base, msg);
}
whamd_status_t Session::results(const ImageLayout& layout, Image& image, std::string& msg) {
	image.total = layout.total;
	return pinned_block(layout.total, (void**)&image.stage, msg);
}
whamd_status_t Session::zero(const Image& image, size_t bytes, std::string& msg) {
	HIP_TRY(hipMemsetAsync(image.base, 0, bytes, stream));
	return WHAMD_OK;
}
whamd_status_t Session::upload(const Image& image, size_t bytes, std::string& msg) {
	if (timed) HIP_TRY(hipEventRecord(ev[UPLOAD_BEGIN], stream));
	HIP_TRY(hipMemcpyAsync(image.base, image.stage, bytes, hipMemcpyHostToDevice, stream));
	if (timed) HIP_TRY(hipEventRecord(ev[UPLOAD_END], stream));
	return WHAMD_OK;
}
whamd_status_t Session::kernels_done(std::string& msg) {
	if (timed) HIP_TRY(hipEventRecord(ev[KERNELS_END], stream));
	return WHAMD_OK;
}
whamd_status_t Session::fetch(void* dst, const void* src, size_t bytes, std::string& msg) {
	HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
	return WHAMD_OK;
}
whamd_status_t Session::finish(CallTimes& times, std::string& msg, bool downloaded) {
	if (timed && downloaded) HIP_TRY(hipEventRecord(ev[DOWNLOAD_END], stream));
	HIP_TRY(hipStreamSynchronize(stream));
	if (!timed) return WHAMD_OK;
	times.upload_ms = ms_between(ev[UPLOAD_BEGIN], ev[UPLOAD_END]);
	times.kernel_ms = ms_between(ev[UPLOAD_END], ev[KERNELS_END]);
	times.download_ms = downloaded ? ms_between(ev[KERNELS_END], ev[DOWNLOAD_END]) : 0.0;
	return WHAMD_OK;
}
void Session::close() {
	if (stream) (void)hipStreamSynchronize(stream);
	for (auto& b : dev) devpool_give(device, b.first, b.second);
	for (auto& b : pinned) pinned_give(b.first, b.second);
	for (void* p : fresh) (void)hipFree(p);
	for (hipEvent_t e : ev) (void)hipEventDestroy(e);
	for (hipStream_t s : streams) (void)hipStreamDestroy(s);
	if (stream) (void)hipStreamDestroy(stream);
	dev.clear(); pinned.clear(); fresh.clear(); ev.clear(); streams.clear();
	stream = nullptr;
}
whamd_status_t Session::device_block(size_t bytes, void** out, std::string& msg) {
	size_t got = 0;
	HIP_TRY(devpool_take(device, std::max<size_t>(bytes, 256), out, &got));
	dev.emplace_back(*out, got);
	return WHAMD_OK;
}
whamd_status_t Session::pinned_block(size_t bytes, void** out, std::string& msg) {
	size_t got = 0;
	HIP_TRY(pinned_take(std::max<size_t>(bytes, 256), out, &got));
	pinned.emplace_back(*out, got);
	return WHAMD_OK;
}
hipError_t Session::fresh_block(void** out, size_t bytes) {
	hipError_t e = hipMalloc(out, std::max<size_t>(bytes, 16));
	if (e != hipSuccess) {   // idle blocks of the pool may hold the memory: give them back, try once more
		(void)hipGetLastError();
		devpool_release();
		e = hipMalloc(out, std::max<size_t>(bytes, 16));
	}
	if (e == hipSuccess) fresh.push_back(*out);
	return e;
}
hipError_t Session::add_stream(hipStream_t* out) {
	const hipError_t e = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
	if (e == hipSuccess) streams.push_back(*out);
	return e;
}
hipError_t Session::sync_event(hipEvent_t* out) {
	const hipError_t e = hipEventCreateWithFlags(out, hipEventDisableTiming);
	if (e == hipSuccess) ev.push_back(*out);
	return e;
}

}  // namespace whamd
