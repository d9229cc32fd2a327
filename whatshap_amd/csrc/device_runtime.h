// device_runtime.h -- what every device layer shares on the host side (device_runtime.cpp; no kernels): the pools that keep device
// buffers, pinned blocks, streams with their events and backtrace arenas between calls (per process, every device), the upload streams
// and pinned staging areas of the create path, and the per-call Session.  whamd_release_caches() empties the pools through
// device_release_caches().
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"

// `msg` (std::string&) is in scope; the enclosing function returns whamd_status_t.
#define HIP_TRY(expr)                                                                                 \
	do {                                                                                              \
		hipError_t err_ = (expr);                                                                     \
		if (err_ != hipSuccess) {                                                                     \
			msg = std::string(#expr) + " failed: " + hipGetErrorString(err_);                         \
			return WHAMD_ERR_DEVICE;                                                                  \
		}                                                                                             \
	} while (0)

// A step that returns a whamd_status_t: a failure is returned from the enclosing function at once, so no step runs after it.
#define WHAMD_TRY(expr)                                                                               \
	do {                                                                                              \
		const whamd_status_t st_ = (expr);                                                            \
		if (st_ != WHAMD_OK) return st_;                                                              \
	} while (0)

namespace whamd {

// Makes `device` current; the two messages of a call without a usable device are written here and nowhere else.
whamd_status_t open_device(int device, std::string& msg);

// ---------------------------------------------------------------------------------------------- device pool
// A create / solve used to hipMalloc 20 - 30 arrays and hipFree them again, each a driver round trip behind one driver lock (tables
// created on several host threads at once waited for each other there).  Blocks are taken from and given back to a pool, rounded to
// size classes (eight per power of two: at most 12.5 % over) so that the tables of one run reuse each other's.
// *got = the block's real size (the class): give exactly that back.
hipError_t devpool_take(int device, size_t bytes, void** out, size_t* got);
// The caller has made sure nothing on the device still uses the block (stream synchronised).
void devpool_give(int device, void* ptr, size_t bytes);
void devpool_release();
// The pinned host blocks (the solves' download buffers, the calls' staging blocks): same size classes, at most 1 GiB kept idle.
hipError_t pinned_take(size_t bytes, void** out, size_t* got);
void pinned_give(void* ptr, size_t bytes);

// A table's stream and events come from a pool as well: creating and destroying them per table (a stream, five events, hipHostMalloc /
// hipHostFree of the path buffer) was as expensive as the whole create of a coverage-15 table (24 tables: create 103 ms on 8 threads,
// close 110 ms).  ev[0 .. 3] record times, ev[4] and ev[5] do not.
struct StreamSet { hipStream_t stream = nullptr; hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; int device = -1; };
bool streamset_take(int device, StreamSet& out);
void streamset_give(const StreamSet& ss);   // (the stream is idle: the caller synchronised it)

// One of the streams the UPLOADS of all tables of `device` go through (shared, used for nothing else); nullptr if none could be made.
hipStream_t upload_stream_of(int device);

// ---------------------------------------------------------------------------------------------- arenas kept between tables
// nullptr: nothing suitable.  `make_room`: the caller is about to hipMalloc `need` bytes -- blocks that do not fit are freed first.
void* arena_take(int device, size_t need, size_t& got, bool make_room = true);
void arena_give(int device, void* ptr, size_t bytes);   // called with `device` current
size_t arena_idle_bytes(int device);
void arena_release();   // every idle arena goes back to the driver (a call that finds the device more than half full does this first)

// Everything above and the idle staging areas, and the genotyper's column store (genotype.h): whamd_release_caches.
void device_release_caches();

// ---------------------------------------------------------------------------------------------- pinned staging of the create path
constexpr size_t STAGE_MAX = (size_t)1 << 30;
// One upload()'s hold on a pinned staging area (device_runtime.cpp, UploadStage) and the copies it sends from there on `stream`.
struct StageSession {
	hipStream_t stream;
	size_t used = 0, total = 0;
	bool pending = false;
	const bool enabled;
	int slot = -1;          // the area this session owns, -1: none (pageable copies)
	char* base = nullptr;
	size_t cap = 0;
	// One image of everything a table uploads (DeviceTable::upload): the area holds `bytes` and copy() leaves it alone (pieces that do not fit the image go
	// out as copies of their own, straight from the caller's memory).
	bool image = false;
	explicit StageSession(hipStream_t s);
	~StageSession();
	// The table's create returns without waiting for the copies (DeviceTable::upload): the area stays reserved -- for the NEXT session -- behind an event.
	bool park();
	bool ensure(size_t bytes);   // area empty (nothing pending): make it hold `bytes`, or everything the largest table so far staged
	hipError_t copy(void* dst, const void* src, size_t bytes);
	bool begin_image(size_t bytes);
	void expect(size_t bytes);   // before the first copy: one allocation
	void finish() {              // after the caller synchronised the stream
		pending = false;
		used = 0;
	}
};

// ---------------------------------------------------------------------------------------------- one call on one device
// What a call holds on the device and in pinned memory; given back on every way out.
// The steps of a batch call (one image up, kernels, results down), in this order; each sets `msg` and returns the status, and the call
// wraps each in WHAMD_TRY:
//   stage(layout, image)      the image's pinned and device block (call_image.h); the call fills image.host(piece).  Also an image the
//                             kernels write and that comes down whole (no upload)
//   work(layout, image)       an image the kernels make and use: its device block only
//   results(layout, image)    an image the fetched pieces come down into: its pinned block only
//   upload(image)             the image, or its first `bytes`, to the device
//   zero(image, bytes)        the front of a work image
//   ... launch(s, times, msg, kernel, grid, block, lds, args...), counted in times.launches ...
//   fetch_now(res, piece, src)  at most once, in the middle: a fetch the host waits for, because the value sizes what follows
//   kernels_done()
//   fetch(res, piece, src)    device to pinned host, one copy per piece; as many as the call needs (before kernels_done(): part of the
//                             kernel time).  fetch(dst, src, n) for a part of a piece
//   finish(times)             waits for the stream; upload / kernel / download ms of `times`
// A session opened with four events records one around each phase; one opened with none records nothing and finish() leaves `times` alone.
struct Session {
	int device = -1;
	hipStream_t stream = nullptr;
	std::vector<hipEvent_t> ev;              // [0, n_events) of open() record times (ms); sync_event() appends
	bool timed = false;                      // open() with four events: the steps record them
	std::vector<hipStream_t> streams;        // add_stream()
	std::vector<std::pair<void*, size_t>> dev, pinned;   // (pointer, size class) of the pools
	std::vector<void*> fresh;                // fresh_block()
	Session() = default;
	Session(const Session&) = delete;
	Session& operator=(const Session&) = delete;
	~Session() { close(); }
	// open_device(), a stream of the call's own and `n_events` events that record times.
	whamd_status_t open(int dev_index, int n_events, std::string& msg);
	// Waits for the stream, gives the blocks back, destroys events and streams.  (The destructor; a caller that times it calls it itself.)
	void close();
	whamd_status_t device_block(size_t bytes, void** out, std::string& msg);
	whamd_status_t pinned_block(size_t bytes, void** out, std::string& msg);
	whamd_status_t stage(const ImageLayout& layout, Image& image, std::string& msg) {
		WHAMD_TRY(results(layout, image, msg));
		return work(layout, image, msg);
	}
	// One device block of the layout's total: sets base and total, leaves stage null.  A layer that scatters lays its work image out as
	// rs_add_zeroed() (run_scatter.h), its own zeroed pieces, rs_add_rest(), the rest: the zeroed pieces come first, and the layout's total
	// after the last of them is the byte count for zero().
	whamd_status_t work(const ImageLayout& layout, Image& image, std::string& msg);
	whamd_status_t zero(const Image& image, size_t bytes, std::string& msg);   // the image's first `bytes`, on the stream
	// One pinned block of the layout's total: sets stage and total.
	whamd_status_t results(const ImageLayout& layout, Image& image, std::string& msg);
	whamd_status_t upload(const Image& image, size_t bytes, std::string& msg);
	whamd_status_t upload(const Image& image, std::string& msg) { return upload(image, image.total, msg); }
	whamd_status_t kernels_done(std::string& msg);
	whamd_status_t fetch(void* dst, const void* src, size_t bytes, std::string& msg);
	template <class T>
	whamd_status_t fetch(const Image& res, const Piece<T>& p, const T* src, std::string& msg) { return fetch(res.host(p), src, p.bytes(), msg); }
	// fetch() and then a wait for the stream: the one wait in the middle of a call.  The fetched value sizes what follows (kept pairs,
	// table rows), so the host needs it before it can take the blocks and launch the rest.
	template <class T>
	whamd_status_t fetch_now(const Image& res, const Piece<T>& p, const T* src, std::string& msg) {
		WHAMD_TRY(fetch(res, p, src, msg));
		HIP_TRY(hipStreamSynchronize(stream));
		return WHAMD_OK;
	}
	// downloaded = false: nothing was fetched after kernels_done() -- no event is recorded for it and download_ms is exactly 0.
	whamd_status_t finish(CallTimes& times, std::string& msg, bool downloaded = true);
	// Not from the pool: hipMalloc -- after devpool_release() once more if the first fails -- and hipFree when the session ends.
	hipError_t fresh_block(void** out, size_t bytes);
	hipError_t add_stream(hipStream_t* out);
	hipError_t sync_event(hipEvent_t* out);   // hipEventDisableTiming: orders streams, records no time
};

#if defined(__HIPCC__)
// One launch on the session's stream with `lds` bytes of dynamic LDS, checked and counted in times.launches.
template <class... P>
whamd_status_t launch(Session& s, CallTimes& times, std::string& msg, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, P... args) {
	hipLaunchKernelGGL(kernel, grid, block, lds, s.stream, args...);
	HIP_TRY(hipGetLastError());
	++times.launches;
	return WHAMD_OK;
}
#endif

}  // namespace whamd
