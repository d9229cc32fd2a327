// dp_device.hip -- gfx950 kernels and the device driver of the wMEC / PedMEC forward pass + backtrace.
//
// What is computed (bit-exact restatement of src/pedigreedptable.cpp:177-335):
//   D_c[x][i]  = cost_{c,i}(x) (+) min_j ( Pr_{c-1}[x & lowmask_b][j] + popcount(i^j) * recomb_c ),  lowest j on ties
//   Pr_c[y][i] = min { D_c[x][i] : pext(x, fwd_mask_c) == y },  argmin = the x with the smallest Gray-code rank
// The reference walks x in reflected-Gray-code order with strict '<' updates; here every cell is evaluated
// independently (closed-form cost, no Gray stepping) and ties are broken with the key (value, gray_rank(x)).
//
// Kernels (included below, one file per family):
//   kernels_column.h     one launch per column: column_step_fused (thread = one projection entry, ballot-packed argmin
//                        planes), column_step_keys + column_finalize (64-bit atomicMin keys; many ending reads, tiny
//                        columns, the last column)
//   kernels_resident.h   single-individual runs: ~23 columns per launch, the projection column lives in LDS
//   kernels_trio.h       trio runs (T = 4)
//   kernels_backtrace.h  follows the stored argmins from the last column to the first (src/pedigreedptable.cpp:137-173)
// This file: the launch tables and what of the host driver touches the device (DeviceTable: the phases of upload() that allocate, copy or launch; the
// preview; resumable submission, the group solve, wait; the debug library's launch ledger).  What a create decides on the host alone -- the arena's layout,
// windows, jobs, lanes, backtrace units, chunks, the schedule, the preview's plan -- is table_plan.h / table_plan.cpp, which no HIP header reaches; Impl
// holds its result (TablePlan) beside the caller's options (TableOptions), the table's device arrays (TableArrays) and the solve in flight.
// No MFMA (integer min-plus), no CUDA compatibility layer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "debug_build.h"
#ifdef WHAMD_DEBUG_BUILD
#include "../../include/whatshap_amd_debug.h"
#endif
#include "device_runtime.h"
#include "device_table.h"
#include "genotype.h"
#include "table_plan.h"

namespace whamd {

namespace {

// device code, in dependency order (each file documents its kernels)
#include "kernels_column.h"
#include "kernels_resident.h"
#include "kernels_trio.h"
#include "kernels_slots.h"
#include "kernels_pedslots.h"
#include "kernels_backtrace.h"

// ---------------------------------------------------------------------------------------------- launch tables
using FusedFn = void (*)(DevProblem, uint32_t, const uint32_t*, uint32_t*);
using KeysFn = void (*)(DevProblem, uint32_t, const uint32_t*, uint32_t);

template <int T, int NIND>
void pick(FusedFn& ff, KeysFn& kf) {
	ff = column_step_fused<T, NIND>;
	kf = column_step_keys<T, NIND>;
}

bool select_kernels(uint32_t T, uint32_t n_ind, FusedFn& ff, KeysFn& kf) {
	const uint32_t ni = n_ind ? n_ind : 1;  // an empty pedigree has no terms to add; NIND=1 with zero deltas is equivalent
	ff = nullptr;
	kf = nullptr;
#define WHAMD_CASE(TT, NN) if (T == TT && ni == NN) { pick<TT, NN>(ff, kf); return true; }
	WHAMD_CASE(1, 1) WHAMD_CASE(1, 2) WHAMD_CASE(1, 3) WHAMD_CASE(1, 4) WHAMD_CASE(1, 5) WHAMD_CASE(1, 6)
	WHAMD_CASE(4, 3) WHAMD_CASE(4, 4) WHAMD_CASE(4, 5) WHAMD_CASE(4, 6)
	WHAMD_CASE(16, 4) WHAMD_CASE(16, 5) WHAMD_CASE(16, 6)
#undef WHAMD_CASE
	return false;
}

// The kernels of the solve, one pointer type per signature.  Which instantiation a run takes is decided by the *_kernel functions of "launch tables of the
// solve", which stand BELOW opt_in_large_lds: the compiler emits the instantiations in the order they are first named, and that table names most of them first.
using SegmentFn = void (*)(DevProblem, ResSegment, const uint32_t*, uint32_t*, uint32_t*);
using PedSegmentFn = void (*)(DevProblem, ResSegment, const uint32_t*, uint32_t*);
using ResBatchFn = void (*)(DevProblem, const ResBatchEntry*);
using SlotRunFn = void (*)(DevProblem, SlotRun, const uint32_t*, uint32_t*, uint32_t*);
using SlotRunXFn = void (*)(DevProblem, SlotRun, const uint32_t*, uint32_t*, uint32_t*, uint32_t);
using PedSlotRunFn = void (*)(DevProblem, SlotRun, PedSlotExtra, const uint32_t*, uint32_t*);
using SlotBatchFn = void (*)(DevProblem, const SlotBatchEntry*);
using GroupFn = void (*)(SlotGroupArgs);

}  // namespace

// ================================================================================================ what a create shares between its phases

namespace {

// `bytes` from the device pool, entered in `allocations`: whoever owns that list gives them back (Impl::release, Impl::give_preview_block).
hipError_t pool_alloc(int device, std::vector<std::pair<void*, size_t>>& allocations, void** dptr, size_t bytes) {
	size_t got = 0;
	const hipError_t e = devpool_take(device, std::max<size_t>(bytes, 16), dptr, &got);
	if (e == hipSuccess) allocations.emplace_back(*dptr, got);
	return e;
}

// The upload half of a create.  ONE device block and ONE staging image per table: every uploaded array is a piece of the block at the offset it has in the
// pinned area, and the pieces leave as a few large copies.  (Per-array copies of ~1 MB ran at 25 GB/s -- 96 coverage-15 tables, 28 MB each, spent their
// creates waiting for the link --; pieces of 32 MB and more reach 56 GB/s: scripts/micro/r6_h2d_rate.py.)  Without an image or a block every array is an
// allocation and a copy of its own.
struct TableUploader {
	const int device;
	const hipStream_t stream;   // every copy of the create and its table kernels (all tables' images on ONE shared stream instead of sixteen at once was measured: 1 055 - 1 273 against 1 015 - 1 153 creates/s, noise)
	StageSession stage;
	std::vector<std::pair<void*, size_t>>& allocations;   // the table's: what alloc() takes, Impl::release() gives back
	char* d_slab = nullptr;
	size_t slab_cap = 0, slab_used = 0, slab_flushed = 0;
	bool unstaged_copies = false;   // a copy whose source is pageable memory of this call: the create must wait for it

	TableUploader(int dev, hipStream_t us, std::vector<std::pair<void*, size_t>>& table_allocations) : device(dev), stream(us), stage(us), allocations(table_allocations) {}

	hipError_t alloc(void** dptr, size_t bytes) { return pool_alloc(device, allocations, dptr, bytes); }
	// The staging image and the device block for `upload_bytes` (an upper bound of everything up() will be given); where either is not to be had, up() falls back.
	void open_block(size_t upload_bytes) {
		stage.expect(upload_bytes);
		if (upload_bytes <= STAGE_MAX && !debug_env("WHAMD_NO_UPLOAD_SLAB") && stage.begin_image(upload_bytes)) {
			void* ptr = nullptr;
			if (alloc(&ptr, upload_bytes) == hipSuccess) { d_slab = (char*)ptr; slab_cap = upload_bytes; }
			else { (void)hipGetLastError(); stage.image = false; }
		}
	}
	hipError_t flush() {
		if (!d_slab || slab_used == slab_flushed) return hipSuccess;
		// (WHAMD_SKIP_SLAB_COPY=1, debug library, RESULTS INVALID: the image is built but does not travel -- what the creates cost without the link)
		const hipError_t e = debug_env("WHAMD_SKIP_SLAB_COPY") ? hipSuccess : hipMemcpyAsync(d_slab + slab_flushed, stage.base + slab_flushed, slab_used - slab_flushed, hipMemcpyHostToDevice, stream);
		stage.pending = true;
		slab_flushed = slab_used;
		return e;
	}
	hipError_t up(void** dptr, const void* src, size_t bytes) {
		const size_t padded = (bytes + 255) & ~(size_t)255;
		if (d_slab && slab_used + padded <= slab_cap) {
			*dptr = d_slab + slab_used;
			char* at = stage.base + slab_used;
			const char* from = (const char*)src;
			if (bytes >= ((size_t)4 << 20)) parallel_ranges(bytes, host_threads(bytes, (size_t)2 << 20), [at, from](uint64_t b0, uint64_t b1, uint32_t) { std::memcpy(at + b0, from + b0, b1 - b0); });
			else if (bytes) std::memcpy(at, from, bytes);
			slab_used += padded;
			stage.total += padded;
			return slab_used - slab_flushed >= ((size_t)32 << 20) ? flush() : hipSuccess;
		}
		hipError_t e = alloc(dptr, bytes);
		if (e != hipSuccess) return e;
		if (bytes) e = stage.copy(*dptr, src, bytes);
		if (bytes && stage.image) unstaged_copies = true;   // (did not fit the image: copied straight from the caller's memory)
		return e;
	}
	// reserves `bytes` like up(), sends only the byte ranges of `pieces`
	hipError_t up_pieces(void** dptr, const void* src, size_t bytes, const std::vector<std::pair<size_t, size_t>>& pieces) {
		const size_t padded = (bytes + 255) & ~(size_t)255;
		const bool in_slab = d_slab && slab_used + padded <= slab_cap;
		if (in_slab) {
			hipError_t e = flush();   // what is staged so far leaves as it is; this array's pieces go out on their own
			if (e != hipSuccess) return e;
			*dptr = d_slab + slab_used;
			slab_used += padded;
			slab_flushed = slab_used;      // (nothing of this array is in the staging image)
		} else {
			hipError_t e = alloc(dptr, bytes);
			if (e != hipSuccess) return e;
		}
		const size_t image_at = slab_used - padded;   // (in_slab: where the array lies in the block AND in the staging image)
		for (const auto& pc : pieces) {
			if (pc.second <= pc.first) continue;
			const char* from = (const char*)src + pc.first;
			if (in_slab) {   // through the pinned image, like everything else: the copy's source outlives the create
				std::memcpy(stage.base + image_at + pc.first, from, pc.second - pc.first);
				from = stage.base + image_at + pc.first;
				stage.pending = true;
			} else {
				unstaged_copies = true;   // (straight from the caller's pageable memory: the create ends with a host wait)
			}
			hipError_t e = hipMemcpyAsync((char*)*dptr + pc.first, from, pc.second - pc.first, hipMemcpyHostToDevice, stream);
			if (e != hipSuccess) return e;
		}
		return hipSuccess;
	}
};

}  // namespace

// ================================================================================================ DeviceTable

#ifdef WHAMD_DEBUG_BUILD
// What a launch site knows of the choice it made, for the ledger: a whamd_debug_launch with every fact "not known" (-1), filled by name.
struct LaunchFacts : whamd_debug_launch {
	LaunchFacts() {
		std::memset(static_cast<whamd_debug_launch*>(this), 0, sizeof(whamd_debug_launch));
		lr = yflags = spec = stamps = tb = nf = ncols = threads = streamed = pack = tight = variant = T = n_ind = mode = wide = ped = sym = entries = -1;
	}
	static LaunchFacts of_run(const SlotRun& run, bool spec_v, bool stamps_v) {
		LaunchFacts f;
		f.lr = (int32_t)run.lr; f.yflags = (int32_t)run.yflags; f.ncols = (int32_t)run.ncols; f.threads = (int32_t)run.threads;
		f.spec = spec_v; f.stamps = stamps_v;
		return f;
	}
};
// WHAMD_NOTE(table, site, kernel, grid, block, lds, stream, forward, facts): the debug library enters the launch in the table's ledger; the product has no ledger.
#define WHAMD_NOTE(table, ...) (table).note(__VA_ARGS__)
#else
#define WHAMD_NOTE(table, ...) ((void)0)
#endif

// The table's device arrays, and the two host blocks that mirror device memory.  release() gives `allocations`, the arena and the pinned block back and
// default-constructs the rest with them.
struct TableArrays {
	std::vector<std::pair<void*, size_t>> allocations;   // (pointer, size class) of device_pool.h: everything below but the arena
	void* d_arena = nullptr;    // the backtrace arena: not in `allocations`, handed to the arena cache on release
	size_t arena_bytes = 0;
	DevProblem dp{};
	DevColumn* d_cols = nullptr;
	uint32_t* d_pr[2] = {nullptr, nullptr};
	size_t key_entries = 0;     // of dp.keys and of every lane's key scratch
	// one result block, laid out like h_pinned (take_result_block)
	uint32_t* d_path_index = nullptr;
	uint32_t* d_path_trans = nullptr;
	uint32_t* d_score = nullptr;
	uint32_t* d_job_scores = nullptr;
	uint32_t* d_bt_counters = nullptr;
	size_t h_pinned_bytes = 0;
	uint32_t* h_pinned = nullptr;  // [2 n + jobs + 3]: path index, path transmission, score of the final job, scores of the others, the chunked backtrace's three counters
	// schedule and backtrace
	BtUnit* d_units = nullptr;
	ResBatchEntry* d_entries = nullptr;
	SlotBatchEntry* d_slot_entries = nullptr;
	BtJob* d_btjobs = nullptr;
	// chunked speculative backtrace (kernels_backtrace.h)
	BtChunk* d_chunks = nullptr;
	uint32_t* d_unit_x = nullptr;   // [2][units]
	uint32_t* d_path2 = nullptr;    // [2][columns]: speculative walks of the two orientations
	uint32_t* d_trans2 = nullptr;   // [orientations][columns]: their transmission values
	uint8_t* d_sel = nullptr;
	uint32_t* d_guess = nullptr;
	BtGroupEntry h_bt_entry{};          // what a batched backtrace launch reads for this table (kernels_backtrace.h backtrace_chunks_group), and its device copy
	BtGroupEntry* d_bt_entry = nullptr;
	// windowed solve (Window)
	uint8_t* d_checkpoints = nullptr;   // [windows - 1] exchange columns
	uint32_t* d_bt_state = nullptr;     // (x, transmission) the walk of a window hands to the next older one
	BtJob* d_window_jobs = nullptr;
	SuperreadArgs super_args{};         // superreads_single: where its inputs and its result lie
};

struct DeviceTable::Impl {
	// ---- the device, the pooled stream and events (open / release_device), and what is known of the stream and the upload
	int device = 0;
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
	hipEvent_t ev_group = nullptr;      // group solve: "the forward pass of every table of the group is submitted up to here"
	hipEvent_t ev_upload = nullptr;     // "everything upload() put on `stream` -- the copies, the table kernels -- is done": a solve waits for it ON THE DEVICE (begin_solve)
	bool counted = false;               // this table is counted in tables_on_device
	static inline std::atomic<int> tables_on_device[64];   // tables of the process that hold device resources, per device (open / release_device)
	bool alone_on_device() const { return device >= 0 && device < 64 && tables_on_device[device].load() == 1; }
	bool own_stream_used = false;       // something has been submitted to `stream` since it was last synchronised (a member of a group solve never touches its own: its
	                                    // solve and tail are on the lead's stream, its uploads on an upload stream -- release() then has nothing to wait for there)
	bool upload_pending = false;        // the uploads went through a shared upload stream and no solve has been ordered behind `ev_upload` yet
	hipStream_t upload_stream = nullptr;
	// ---- the four kinds of state
	TableOptions opt;    // what the caller set: only the set_* functions write it, no release touches it
	TablePlan tp;        // the host description of the built table (table_plan.h)
	TableArrays dev;     // its device arrays
	FusedFn fused = nullptr;   // the templated per-column kernels of (T, individuals): choose_plan sets both with tp.wide in every create; null where the table is wide
	KeysFn keysfn = nullptr;

	// the phases of a create (DeviceTable::upload) that touch the device or the planner, in the order they run; the host-only phases between them are table_plan.h's
	whamd_status_t open(int dev, std::string& msg);
	whamd_status_t choose_plan(Problem& p, TableBuild& b, bool from_create, std::string& msg);
	void dump_plan(const Problem& p) const;
	whamd_status_t upload_column_arrays(const Problem& p, TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t upload_slot_arrays(TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t make_windows(const TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t take_result_block(uint32_t n, TableUploader& up, std::string& msg);
	whamd_status_t make_chunks(const Problem& p, TableUploader& up, std::string& msg);
	whamd_status_t take_arena(uint64_t bytes, std::string& msg);
	whamd_status_t take_solve_buffers(const Problem& p, TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t make_lanes(const TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t upload_entries(TableUploader& up, std::string& msg);
	whamd_status_t launch_table_kernels(const Problem& p, const TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t arm_debug_stamps(TableUploader& up, std::string& msg);
	whamd_status_t record_group_backtrace(uint32_t n, TableUploader& up, std::string& msg);
	// The solve being submitted or awaiting collection.  (own_stream_used and upload_pending above describe the stream and the upload, not a solve.)
	struct SolveInFlight {
		hipStream_t run_stream = nullptr;   // where the forward steps go: `stream`, or the stream of the group's lead.  Set where a solve opens (enqueue_some_unguarded,
		                                    // GroupSubmission::open_members); read by begin_solve, the launch_* functions, submit_super_step, submit_singles
		uint32_t group_tables = 1;          // tables that shared the forward launches.  Set where a solve opens; read by wait (whamd_solve_stats)
		bool enqueue_open = false;          // a solve has been opened and its tail is not submitted yet.  Set where a solve opens, cleared by rewind; read by
		                                    // enqueue_some_unguarded (resume or open) and group_eligible
		size_t next_super = 0;              // cursor of the resumable enqueue.  Set by begin_solve and rewind, advanced and read by enqueue_some_unguarded only
		uint64_t launches = 0;              // forward launches so far.  Set by begin_solve, enqueue_some_unguarded and GroupSubmission::submit_tails; read by wait
		hipStream_t tail_stream = nullptr;  // where the tail (backtrace, downloads) went, and its place in the order of all tails of the process.  Set by submit_tail;
		uint64_t tail_seq = 0;              // read by wait_last_of_each_stream
		bool tail_elsewhere = false;        // the tail went onto another table's stream.  Set by submit_tail; read by wait (waits for ev3, not for `stream`),
		                                    // wait_last_of_each_stream and release
		bool timing_pending = false;        // wait has collected a solve whose event timings nobody has read yet.  Set by wait, cleared by begin_solve (the events
		                                    // are the new solve's from there on) and read_timing
		static inline std::atomic<uint64_t> tails_submitted{0};   // numbers tail_seq
		// No solve is being submitted: the next enqueue begins with the preamble again, on the table's own stream.
		void rewind(hipStream_t own) { enqueue_open = false; next_super = 0; run_stream = own; }
	} inflight;
#ifdef WHAMD_DEBUG_BUILD
	// The launch ledger (whatshap_amd_debug.h): one line per distinct launch of the solve in flight, with a count.  begin_solve empties it.
	std::vector<whamd_debug_launch> ledger;
	void note(uint32_t site, const void* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t on, bool forward, const LaunchFacts& facts);
#endif
	// the solve, step by step
	struct GroupSubmission;
	void launch_column_step(const Problem& p, const Step& step, const Lane& lane, const uint32_t* prev, uint32_t* cur, uint64_t& launches);
	void launch_run(const ResBatchEntry& e, uint64_t& launches);
	void launch_slot_run(const DevProblem& dp, const SlotBatchEntry& e, uint64_t& launches);
	whamd_status_t begin_solve(const Problem& p, Solution& s, std::string& msg, bool behind_preview = false);
	whamd_status_t submit_super_step(const Problem& p, const SuperStep& ss, uint64_t& launches, std::string& msg);
	whamd_status_t submit_singles(const Problem& p, const SuperStep& ss, uint64_t& launches, std::string& msg);
	whamd_status_t submit_tail(const Problem& p, std::string& msg, hipStream_t tail_stream = nullptr, bool walked_by_group = false);
	whamd_status_t report_slot_stamps(std::string& msg) const;
	whamd_status_t report_slot_wave_stamps(std::string& msg) const;
	whamd_status_t report_resident_stamps(std::string& msg) const;

	// The preview (DESIGN.md 6.1 "preview"): the leading slot runs of a lone table's forward pass, launched on `stream` from INSIDE the create -- from arrays of
	// their own, uploaded first -- so that the device works while the host builds and uploads the whole table.  The finished schedule is then held against what
	// was launched (verify_preview); the first enqueue continues behind the preview where every step agrees, and starts at step 0 as ever where not.
	struct Preview {
		uint32_t why = PV_NOT_CREATE;       // PV_RAN, or why there was none
		uint32_t pieces = 0;                // plan pieces the preview covered
		uint32_t launched = 0;              // super-steps launched
		uint32_t agreed = 0;                // S: leading super-steps of the finished schedule that are launch for launch what was launched (verify_preview)
		bool launching = false;             // start_preview is submitting its launches
		bool tried = false;                 // start_preview has been called for this upload (choose_plan's head hook, or upload() itself)
		bool from_hook = false;             // ... from the planner's head hook: the launches went out before the plan's second half
		bool pending = false;               // launched, and no solve has been opened since
		bool continued = false;             // the solve in flight / collected last began behind the preview
		bool use_chunks = false;            // what the launches were chosen with
		uint64_t launches = 0;              // forward launches of the preview
		std::vector<SlotRun> runs;          // what every launched step was given by value
		DevProblem dp{};                    // ... and as its problem: the preview's own rows, control words and tables; the TABLE's arena, exchange columns and seeds
		uint32_t* d_pr[2] = {nullptr, nullptr};   // taken for the table before the launches (in the table's `allocations`); take_solve_buffers / make_chunks adopt them
		size_t exchange_bytes = 0;
		unsigned long long* spec_keys = nullptr;
		size_t spec_bytes = 0;
		std::vector<std::pair<void*, size_t>> allocations;   // the preview's own device block: given back by wait and release
	} preview;
	void give_preview_block() {   // (the caller knows the preview's launches are done)
		for (auto& a : preview.allocations) devpool_give(device, a.first, a.second);
		preview.allocations.clear();
	}
	whamd_status_t start_preview(const Problem& p, TableBuild& b, bool from_create, std::string& msg);
	void verify_preview();
	whamd_status_t arm_keys(std::string& msg);

	// the pooled stream and events (device_runtime.h), taken on the first create and given back by release_device
	void adopt(const StreamSet& ss) { stream = ss.stream; ev0 = ss.ev[0]; ev1 = ss.ev[1]; ev2 = ss.ev[2]; ev3 = ss.ev[3]; ev_group = ss.ev[4]; ev_upload = ss.ev[5]; }
	StreamSet stream_set() const {
		StreamSet ss;
		ss.stream = stream; ss.ev[0] = ev0; ss.ev[1] = ev1; ss.ev[2] = ev2; ss.ev[3] = ev3; ss.ev[4] = ev_group; ss.ev[5] = ev_upload; ss.device = device;
		return ss;
	}

	// Waits for whatever may still read the table's memory, gives the memory back, and leaves plan, device arrays and preview as a new table has them.
	void release() {
		if (inflight.tail_elsewhere && ev3) (void)hipEventSynchronize(ev3);   // (a solve whose tail ran on the group's lead stream: nothing of it may still be reading the buffers)
		inflight.tail_elsewhere = false;
		if (upload_pending && ev_upload) (void)hipEventSynchronize(ev_upload);   // (a table closed without a solve: its copies may still be on the upload stream)
		upload_pending = false;
		if (stream && own_stream_used && (!dev.allocations.empty() || dev.d_arena)) { (void)hipStreamSynchronize(stream); own_stream_used = false; }   // (hipFree used to wait for the table's last kernels)
		for (auto& a : dev.allocations) devpool_give(device, a.first, a.second);
		give_preview_block();   // (its launches were on `stream`: synchronised above)
		arena_give(device, dev.d_arena, dev.arena_bytes);
		pinned_give(dev.h_pinned, dev.h_pinned_bytes);
		tp = TablePlan();
		dev = TableArrays();
		preview = Preview();
	}
};

DeviceTable::DeviceTable() : impl_(new Impl()) {}

DeviceTable::~DeviceTable() {
	if (impl_) {
		release_device();
		delete impl_;
	}
}

void DeviceTable::release_device() {
	Impl& m = *impl_;
	(void)hipSetDevice(m.device);
	m.release();   // (synchronises the stream before anything is handed back)
	if (m.stream) {
		if (m.own_stream_used) (void)hipStreamSynchronize(m.stream);   // (13 ms for the 96 tables of a step when every table waited for a stream it had never used)
		m.own_stream_used = false;
		streamset_give(m.stream_set());
	}
	m.adopt(StreamSet());
	if (m.counted && m.device >= 0 && m.device < 64) Impl::tables_on_device[m.device].fetch_sub(1);
	m.counted = false;
	m.inflight.run_stream = nullptr;
	m.inflight.timing_pending = false;
}

int DeviceTable::device_count() {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

bool DeviceTable::device_pci_bus_id(int device, std::string& out) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return false;
	char text[64] = {0};
	if (hipDeviceGetPCIBusId(text, (int)sizeof text - 1, device) != hipSuccess) return false;
	out = text;
	for (char& ch : out) ch = (char)tolower((unsigned char)ch);   // (sysfs spells the id in lower case)
	return true;
}

bool DeviceTable::set_path(const std::string& path) {
	if (path != "auto" && path != "column" && path != "column_keys" && path != "resident" && path != "slots") return false;
	impl_->opt.path = path;
	return true;
}

void DeviceTable::set_l_pref(int l) { impl_->opt.l_pref = std::max(4, std::min(l, RES_LMAX)); }
void DeviceTable::set_lanes(int n) { impl_->opt.max_lanes = n < 1 ? 1 : (n > 64 ? 64 : n); }

void DeviceTable::set_fold(bool v) { impl_->opt.fold = v; }
void DeviceTable::set_slot_l(int l) { impl_->opt.slot_l = std::max(2, std::min(l, 12)); impl_->opt.slot_l_set = true; }
void DeviceTable::set_slot_lr(int lr) { impl_->opt.slot_lr = lr >= 3 ? 3 : (lr <= 1 ? 1 : 2); }

void DeviceTable::set_arena_limit(uint64_t bytes) { impl_->opt.arena_limit = bytes; }
void DeviceTable::set_shared_launches(bool v) { impl_->opt.shared_hint = v; }
void DeviceTable::set_side_by_side(bool v) { impl_->opt.side_by_side = v; }
void DeviceTable::set_preview(int mode) { impl_->opt.preview_mode = mode < 0 ? -1 : (mode ? 1 : 0); }
void DeviceTable::set_preview_pieces(uint32_t pieces) { impl_->opt.preview_pieces = pieces; }
void DeviceTable::set_thread_budget(bool v) { impl_->opt.thread_budget = v; }
void DeviceTable::set_symmetry(int level) { impl_->opt.symmetry = level < 0 ? 0 : (level > 2 ? 2 : level); }

// ================================================================================================ create: the phases of DeviceTable::upload
// The phases that decide something on the host alone are free functions of table_plan.h over the options, the build object and the plan; upload() calls them
// between the phases below, which are the ones that ask the device, allocate, copy or launch.  Each of these says in its parameters what it touches: `Problem`,
// the build object (TableBuild: what later phases read), the uploader (TableUploader).  Everything else it reads and writes is Impl's: `opt` (read only), the
// plan `tp`, the device arrays `dev`.  The order of the phases that take an uploader IS the layout of the table's device block and the order of its driver calls.

whamd_status_t DeviceTable::Impl::open(int dev, std::string& msg) {
	Impl& m = *this;
	m.device = dev;
	const whamd_status_t opened = open_device(dev, msg);
	if (opened != WHAMD_OK) return opened;
	if (!m.stream) {
		StreamSet ss;
		if (!streamset_take(dev, ss)) { msg = "could not create the table's stream and events"; return WHAMD_ERR_DEVICE; }
		m.adopt(ss);
	}
	m.release();
	if (!m.counted && dev >= 0 && dev < 64) { Impl::tables_on_device[dev].fetch_add(1); m.counted = true; }
	return WHAMD_OK;
}

// The kernels (templated or wide), the forward path (slot runs, LDS-resident runs, per column) and its plan.  Produces b.force_keys and b.free_b, decides where the superreads
// are made, and fills the problem's lazy term lists where the chosen path reads them.
whamd_status_t DeviceTable::Impl::choose_plan(Problem& p, TableBuild& b, bool from_create, std::string& msg) {
	Impl& m = *this;
	m.preview.tried = false;
	m.preview.from_hook = false;
	// pedigrees beyond the templated kernels (three trios, more than six individuals): the generic per-column kernel, key path only
	m.tp.wide = !select_kernels(p.T, p.n_ind, m.fused, m.keysfn);
	if (m.tp.wide && (p.T > (uint32_t)MAX_T_WIDE || p.n_ind > (uint32_t)MAX_IND_WIDE)) {
		msg = "no device kernel for T=" + std::to_string(p.T) + ", individuals=" + std::to_string(p.n_ind);
		return WHAMD_ERR_UNSUPPORTED;
	}
	// ... and a column with more allele-assignment terms than the templated kernels stage in LDS (genotypes not trusted, seven and more
	// individuals): the generic kernel reads them from global memory
	for (uint32_t c = 0; c < p.n_cols && !m.tp.wide; ++c) m.tp.wide = p.term_end(c, p.T - 1) - p.term_begin(c, 0) > (uint64_t)COL_MAXTERMS;
	b.laps.lap("plan: kernels chosen, term counts scanned");
	b.force_keys = m.opt.path == "column_keys" || m.tp.wide;
	const bool want_resident = (m.opt.path == "auto" || m.opt.path == "resident") && !m.tp.wide;
	size_t free_b = 0, total_b = 0;
	HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	if (free_b < total_b / 2) {   // a genotyping call of this process may be holding its column store (genotype.h): give it back first
		genotype_release_cache();
		HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	}
	if (free_b < total_b / 4) {   // tight: the arenas and buffers kept from closed tables go back as well
		arena_release();
		devpool_release();
		HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	}
	free_b += arena_idle_bytes(m.device);   // (taken by take_solve_buffers, or freed before this table's own arena is allocated)
	b.free_b = free_b;
	b.laps.lap("plan: free device memory asked");
	// A wide single-individual table (coverage >= 18: 128 and more workgroups per launch) that will share its launches with many others
	// takes EIGHT cells per thread and twelve local slots: half the wavefronts per table and longer runs -- 24 coverage-20 tables
	// 7.7 M columns/s instead of 6.4 M; alone the same table is slower that way (1.87 M against 2.26 M), and narrow tables gain nothing.
	int slot_lr = m.opt.slot_lr, slot_l = m.opt.slot_l;
	if (m.opt.shared_hint && p.T == 1 && p.max_k >= 18 && !m.opt.slot_l_set && m.opt.slot_lr == 2) { slot_lr = 3; slot_l = 12; }
	// Coverage 21 and 22 (512 / 1 024 workgroups of four cells per launch: the table fills the chip by itself, rounds of workgroups queue behind each
	// other) take the eight-cell layout ALONE as well: 14.0 against 17.9 us per launch at 21, 20.3 against 30.1 at 22 (scripts/gpu_wide_ab.py; the same
	// kernels with their operands streamed: 14.4 / 22.6).  At 23 the four-cell kernel with streamed operands wins (36.2 against 43.0 us): launch_slot_run.
	if (p.T == 1 && p.max_k >= 21 && p.max_k <= 22 && !m.opt.slot_l_set && m.opt.slot_lr == 2 && !debug_env("WHAMD_NO_WIDE_LAYOUT")) { slot_lr = 3; slot_l = 12; }
	m.tp.slot_lr_used = slot_lr;
	// A lone single-individual table: the planner finishes the steps of the table's preview first and calls back (slots.h SlotPlanHead); the preview's runs are
	// launched from there, and the planner's second half happens under them.  What start_preview reads of this function's results is set here, as it will be below.
	whamd_status_t head_status = WHAMD_OK;
	bool steps_adopted = false;
	auto adopt_steps = [&]() {   // the driver walks plan.steps / plan.component_first_step; slot runs are steps of kind 2
		m.tp.plan = ResidentPlan();
		m.tp.plan.steps = m.tp.splan.steps;
		m.tp.plan.component_first_step = m.tp.splan.component_first_step;
		m.tp.plan.col_to_res.assign(p.n_cols, -1);
		steps_adopted = true;
	};
	SlotPlanHead head;
	{
		const uint32_t n_pieces = slot_plan_pieces(p.n_cols);
		const uint32_t pieces = std::min(n_pieces - 1, preview_pieces_of(m.opt.preview_pieces, n_pieces));
		head.col_limit = slot_plan_piece_begin(p.n_cols, pieces);
		head.at_head = [&](uint32_t n_head) {
			if (n_head == 0) return;   // (the table does not begin with slot runs: upload() asks start_preview, which says why there is none)
			m.tp.use_slots = true;
			m.tp.table_bytes = 0;
			adopt_steps();
			b.laps.lap("plan: the planner up to the head's callback");
			m.preview.tried = true;
			m.preview.from_hook = true;
			head_status = m.start_preview(p, b, from_create, msg);
			if (m.preview.why != PV_RAN) m.preview.from_hook = false;
		};
	}
	// (only where a preview can still come about: what rules it out whatever the plan says -- plan_preview's first checks -- leaves the planner as it was)
	bool head_first = from_create && p.T == 1 && m.opt.preview_mode != 0 && slot_plan_pieces(p.n_cols) >= 2 && !m.opt.shared_hint && !m.opt.side_by_side && !debug_env("WHAMD_NO_PREVIEW") &&
	                  !debug_env("WHAMD_NO_HEAD_FIRST");
	if (head_first && m.opt.preview_mode < 0)
		head_first = !m.opt.thread_budget && slot_plan_pieces(p.n_cols) >= 8 && m.alone_on_device();
	m.tp.use_slots = (m.opt.path == "auto" || m.opt.path == "slots") && !m.tp.wide &&
	              plan_forward_slots(p, p.T > 1 ? (m.opt.slot_l_set ? -m.opt.slot_l : 0) : std::max(8, slot_l), m.opt.symmetry, m.tp.splan, slot_lr, false, head_first ? &head : nullptr);
	if (head_status != WHAMD_OK) return head_status;
	b.laps.lap("plan: the planner");
	// pedigree slot runs keep their cost-form tables in HBM (slots.h): at most a quarter of what is free, else the older paths
	if (m.tp.use_slots && m.tp.splan.ped && m.tp.splan.table_words * 4ull > free_b / 4) m.tp.use_slots = false;
	m.tp.table_bytes = m.tp.use_slots && m.tp.splan.ped ? m.tp.splan.table_words * 4ull : 0ull;
	if (p.lazy_terms) {
		// generic term lists where something will read them: the columns a pedigree slot plan leaves to the per-column kernels; every column on any other path
		std::vector<uint8_t> need(p.n_cols, 1);
		if (m.tp.use_slots && m.tp.splan.ped) for (uint32_t c = 0; c < p.n_cols; ++c) need[c] = m.tp.splan.col_to_row[c] < 0;
		const whamd_status_t st = fill_lazy_terms(p, need, msg);
		if (st != WHAMD_OK) return st;
	}
	if (m.tp.use_slots) {
		if (!steps_adopted) adopt_steps();
	} else {
		m.tp.splan = SlotPlan();
		plan_forward(p, want_resident, m.opt.l_pref, m.opt.fold, m.tp.plan, m.opt.symmetry);
	}
	// The superreads of a single-individual table with trusted genotypes are made on the device, behind the backtrace (the condition is finish_columns' first branch).
	m.tp.device_superreads = p.n_ind == 1 && p.T == 1 && p.P == 2 && !p.distrust && p.h2p.size() >= 2 && p.h2p[0] == 0 && p.h2p[1] == 1 && p.genotype.size() >= p.n_cols &&
	                      !debug_env("WHAMD_HOST_SUPERREADS");
	b.laps.lap("plan: steps adopted, lazy terms");
	return WHAMD_OK;
}

// WHAMD_DEBUG_PLAN (debug library): the chosen plan, one line per step.
void DeviceTable::Impl::dump_plan(const Problem& p) const {
	const Impl& m = *this;
	for (const Step& st : m.tp.plan.steps) {
		if (st.kind == 0) { fprintf(stderr, "[plan] column %u k=%u b=%u f=%u\n", st.index, p.k[st.index], p.b[st.index], p.f[st.index]); continue; }
		if (st.kind == 2) {
			const SlotRun& r = m.tp.splan.runs[st.index];
			fprintf(stderr, "[plan] slot run c0=%u ncols=%u g=%u L=%u half=%u ends=%u has_prev=%u in_identity=%u in_half=%u mirror_pos=%u in_occ=%x out_occ=%x mirror_out=%u\n",
			        r.c0, r.ncols, r.g, r.L, r.half, r.n_ends, r.has_prev, r.in_identity, r.in_half, r.in_mirror_pos, r.in_occ, r.out_occ, r.mirror_out);
			if (m.tp.splan.ped) fprintf(stderr, "[plan]   pedigree run: T=%u forms per value=%u table words=%u record words per workgroup=%u\n", 1u << m.tp.splan.pextra[st.index].tb,
			                         m.tp.splan.pextra[st.index].nf, m.tp.splan.pextra[st.index].s_off + r.ncols * 64u * pslot_ns(m.tp.splan.pextra[st.index].nf), m.tp.splan.pextra[st.index].rec_words);
			continue;
		}
		const ResSegment& sgm = m.tp.plan.segments[st.index];
		fprintf(stderr, "[plan] run c0=%u ncols=%u g=%u threads=%u max_l=%u stage_words=%u\n", sgm.c0, sgm.ncols, sgm.g, sgm.threads, sgm.max_l, sgm.stage_words);
		for (uint32_t i = 0; i < sgm.ncols; ++i) {
			const ResColumn& rc = m.tp.plan.columns[sgm.col_off + i];
			const ResBacktrace& rb = m.tp.plan.backtrace[sgm.col_off + i];
			fprintf(stderr, "[plan]   col %u mode=%u nfold=%u Lb=%u Lf=%u ebits=%u epos0=%u nthr=%u stage_off=%u nwords=%u | bt layout=%u n_g=%u n_l=%u\n",
			        sgm.c0 + i, rc.mode, rc.nfold, rc.Lb, rc.Lf, rc.ebits, rc.epos[0], rc.nthr, rc.stage_off, rc.nwords, rb.layout, rb.n_g, rb.n_l);
		}
	}
}

// The per-column arrays (descriptors, deltas, term offsets, terms -- whole, or only the columns outside slot runs), the superread inputs, segment lists and the
// descriptors of the LDS-resident runs.
whamd_status_t DeviceTable::Impl::upload_column_arrays(const Problem& p, TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	const uint32_t n = b.n;
	static_assert(sizeof(CostTerm) == sizeof(DevTerm), "Problem::terms / fterms are uploaded as they are");
	const RawVec<CostTerm>& terms = p.terms;
	const int32_t* delta_src = p.delta.data();
	size_t delta_count = (size_t)p.col_ptr[n] * p.n_ind;
	if (p.n_ind == 0) { b.delta_fallback.assign(std::max<size_t>(p.col_ptr[n], 1), 0); delta_src = b.delta_fallback.data(); delta_count = b.delta_fallback.size(); }
	// A single-individual table on slot runs: no kernel reads the per-column arrays (descriptor, deltas, term offsets, terms) of a column INSIDE a run -- the run
	// kernels and slot_tables work from the rows, the backtrace from its units -- so only the columns outside runs travel (the coverage ramp, the last column, what an
	// irregular layout leaves between runs): 96 of a column's 450 bytes, and concurrent creates are bound by bytes through the link.  The arrays keep
	// their size and indexing on the device; the pieces that are not sent are never read.
	const bool sparse_columns = m.tp.use_slots && !b.ped_slots && p.T == 1 && !m.tp.windowed && !debug_env("WHAMD_DENSE_COLUMN_UPLOAD");
	if (sparse_columns) {
		std::vector<std::pair<size_t, size_t>> pc_cols, pc_delta, pc_tptr, pc_terms;   // byte ranges of the columns [c, e) outside runs
		for (uint32_t c = 0; c < n;) {
			if (m.tp.splan.col_to_row[c] >= 0) { ++c; continue; }
			uint32_t e = c + 1;
			while (e < n && m.tp.splan.col_to_row[e] < 0) ++e;
			pc_cols.emplace_back((size_t)c * sizeof(DevColumn), (size_t)e * sizeof(DevColumn));
			pc_delta.emplace_back((size_t)p.col_ptr[c] * p.n_ind * sizeof(int32_t), (size_t)p.col_ptr[e] * p.n_ind * sizeof(int32_t));
			pc_tptr.emplace_back((size_t)c * (p.T + 1) * sizeof(uint32_t), (size_t)e * (p.T + 1) * sizeof(uint32_t));
			pc_terms.emplace_back((size_t)p.term_ptr[(size_t)c * p.T] * sizeof(DevTerm), (size_t)p.term_ptr[(size_t)e * p.T] * sizeof(DevTerm));
			c = e;
		}
		HIP_TRY(up.up_pieces((void**)&m.dev.d_cols, m.tp.cols.data(), m.tp.cols.size() * sizeof(DevColumn), pc_cols));
		// (the deltas travel whole when the device makes the superreads: superreads_single reads every column's)
		if (m.tp.device_superreads) HIP_TRY(up.up((void**)&m.dev.dp.delta, delta_src, delta_count * sizeof(int32_t)));
		else HIP_TRY(up.up_pieces((void**)&m.dev.dp.delta, delta_src, delta_count * sizeof(int32_t), pc_delta));
		HIP_TRY(up.up_pieces((void**)&m.dev.dp.term_ptr, b.term_ptr32.data(), b.term_ptr32.size() * sizeof(uint32_t), pc_tptr));
		HIP_TRY(up.up_pieces((void**)&m.dev.dp.terms, terms.data(), terms.size() * sizeof(DevTerm), pc_terms));
	} else {
		HIP_TRY(up.up((void**)&m.dev.d_cols, m.tp.cols.data(), m.tp.cols.size() * sizeof(DevColumn)));
		HIP_TRY(up.up((void**)&m.dev.dp.delta, delta_src, delta_count * sizeof(int32_t)));
		HIP_TRY(up.up((void**)&m.dev.dp.term_ptr, b.term_ptr32.data(), b.term_ptr32.size() * sizeof(uint32_t)));
		HIP_TRY(up.up((void**)&m.dev.dp.terms, terms.data(), terms.size() * sizeof(DevTerm)));
	}
	m.dev.dp.cols = m.dev.d_cols;
	if (m.tp.device_superreads) {
		m.dev.super_args = SuperreadArgs{};
		HIP_TRY(up.up((void**)&m.dev.super_args.col_ptr, p.col_ptr.data(), ((size_t)n + 1) * sizeof(uint64_t)));
		HIP_TRY(up.up((void**)&m.dev.super_args.genotype, p.genotype.data(), (size_t)n));
		m.dev.super_args.delta = m.dev.dp.delta;
		m.dev.super_args.n_cols = n;
		m.tp.super_words = (size_t)n + ((size_t)2 * n + 3) / 4;
	}
	b.d_fterms = nullptr;
	if (!p.fterms.empty()) HIP_TRY(up.up((void**)&b.d_fterms, p.fterms.data(), p.fterms.size() * sizeof(DevTerm)));   // factorised lines (pedslot_tables, PSLOT_FACT)
	HIP_TRY(up.up((void**)&m.dev.dp.segs, b.segs.data(), b.segs.size() * sizeof(uint32_t)));
	HIP_TRY(up.up((void**)&m.dev.dp.res_cols, m.tp.plan.columns.data(), m.tp.plan.columns.size() * sizeof(ResColumn)));
	HIP_TRY(up.up((void**)&m.dev.dp.res_bt, m.tp.plan.backtrace.data(), m.tp.plan.backtrace.size() * sizeof(ResBacktrace)));
	m.tp.plan.ped_columns.resize(m.tp.plan.ped_columns.empty() ? 0 : m.tp.plan.columns.size());
	HIP_TRY(up.up((void**)&m.dev.dp.ped_cols, m.tp.plan.ped_columns.data(), m.tp.plan.ped_columns.size() * sizeof(PedColumn)));
	HIP_TRY(up.up((void**)&m.dev.dp.ped_terms, m.tp.plan.ped_terms.data(), m.tp.plan.ped_terms.size() * sizeof(PedTerm)));
	b.laps.lap("column arrays: allocations + copies");
	return WHAMD_OK;
}

// What the slot-run kernels read: rows, backtrace blobs, control words, the runs themselves and the block their tables are built in (single individual:
// slot_tables; pedigree: pedslot_tables, with the pedigree rows and extras).  Produces b.d_runs / b.d_pextra for launch_table_kernels.
whamd_status_t DeviceTable::Impl::upload_slot_arrays(TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	build_slot_blobs(m.tp, b);
	b.laps.lap("slot backtrace blobs (host)");
	if (!m.tp.splan.rows.empty()) m.tp.splan.rows.resize(m.tp.splan.rows.size() + SLOT_ROW_PAD);   // the kernel's scalar-cache warm-up touches a fixed number of rows
	HIP_TRY(up.up((void**)&m.dev.dp.slot_rows, m.tp.splan.rows.data(), m.tp.splan.rows.size() * sizeof(SlotRow)));
	b.laps.lap("slot rows: allocation + copy");
	HIP_TRY(up.up((void**)&m.dev.dp.slot_blob, b.slot_blob.data(), b.slot_blob.size() * sizeof(uint32_t)));
	HIP_TRY(up.up((void**)&m.dev.dp.slot_ctrl, m.tp.splan.ctrl.data(), m.tp.splan.ctrl.size() * sizeof(uint32_t)));
	m.dev.dp.slot_tab = nullptr;
	b.d_runs = nullptr;
	if (m.tp.use_slots && !b.ped_slots) {
		const uint64_t slot_tab_words = lay_out_slot_tables(m.tp, b);
		if (slot_tab_words >= 0xFFFFFFFFull) { msg = "slot-run tables exceed 32-bit offsets"; return WHAMD_ERR_UNSUPPORTED; }
		HIP_TRY(up.up((void**)&b.d_runs, m.tp.splan.runs.data(), m.tp.splan.runs.size() * sizeof(SlotRun)));
		b.laps.lap("slot blobs, control words, runs: allocations + copies");
		HIP_TRY(up.alloc((void**)&m.dev.dp.slot_tab, slot_tab_words * 4));
		b.laps.lap("slot tables: allocation");
	}
	m.dev.dp.pslot_rows = nullptr;
	m.dev.dp.pslot_tab = nullptr;
	b.d_pextra = nullptr;
	if (b.ped_slots) {
		HIP_TRY(up.up((void**)&m.dev.dp.pslot_rows, m.tp.splan.prows.data(), m.tp.splan.prows.size() * sizeof(PedSlotRow)));
		HIP_TRY(up.up((void**)&b.d_runs, m.tp.splan.runs.data(), m.tp.splan.runs.size() * sizeof(SlotRun)));
		HIP_TRY(up.up((void**)&b.d_pextra, m.tp.splan.pextra.data(), m.tp.splan.pextra.size() * sizeof(PedSlotExtra)));
		HIP_TRY(up.alloc((void**)&m.dev.dp.pslot_tab, m.tp.table_bytes));
	}
	b.laps.lap("slot rows / blobs / control words: allocations + copies");
	return WHAMD_OK;
}

// A windowed table (see Window): the windows and their backtrace jobs (cut_windows), the kept boundary columns and the state one window's walk hands to the next.
whamd_status_t DeviceTable::Impl::make_windows(const TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.dev.dp.bt_state = nullptr;
	if (!m.tp.windowed) return WHAMD_OK;
	std::vector<BtJob> wjobs;
	const whamd_status_t cut = cut_windows(b, m.tp, wjobs, msg);
	if (cut != WHAMD_OK) return cut;
	HIP_TRY(up.up((void**)&m.dev.d_window_jobs, wjobs.data(), wjobs.size() * sizeof(BtJob)));
	HIP_TRY(up.alloc((void**)&m.dev.d_checkpoints, (m.tp.windows.size() - 1) * m.tp.checkpoint_bytes));
	HIP_TRY(up.alloc((void**)&m.dev.d_bt_state, 16));
	m.dev.dp.bt_state = m.dev.d_bt_state;
	if (b.laps.on) fprintf(stderr, "[whamd timing] windowed solve: %zu windows, arena %.2f GB\n", m.tp.windows.size(), (double)b.bt / 1e9);
	return WHAMD_OK;
}

// Everything a solve hands back lies in ONE device block, laid out like the pinned buffer it is downloaded into: [n] path index, [n] path transmission, the
// final job's score with the other jobs' behind it (d_job_scores[0] IS d_score: job 0 is the final one and has no entry of its own), four words of backtrace
// counters, the superreads.  Five copies per table -- 4.6 us each as blit kernels, one after the other on a group's stream: 2.6 ms behind a 96-table solve -- are one.
whamd_status_t DeviceTable::Impl::take_result_block(uint32_t n, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.tp.super_off = 2 * (size_t)n + 4 + m.tp.jobs.size();
	void* d_res = nullptr;
	HIP_TRY(up.alloc(&d_res, (m.tp.super_off + (m.tp.device_superreads ? m.tp.super_words : 0)) * sizeof(uint32_t) + 16));
	uint32_t* res = (uint32_t*)d_res;
	m.dev.d_path_index = res;
	m.dev.d_path_trans = res + n;
	m.dev.d_score = res + 2 * (size_t)n;
	m.dev.d_job_scores = res + 2 * (size_t)n;
	m.dev.d_bt_counters = res + 2 * (size_t)n + m.tp.jobs.size();
	if (m.tp.device_superreads) {
		m.dev.super_args.out = res + m.tp.super_off;
		m.dev.super_args.path_index = m.dev.d_path_index;
	}
	return WHAMD_OK;
}

// The chunks (cut_chunks), their device copy, the walk's buffers and m.dev.dp.spec_keys (the schedule's entries carry it and the stride).
whamd_status_t DeviceTable::Impl::make_chunks(const Problem& p, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	const uint32_t n = p.n_cols;
	m.dev.dp.spec_keys = nullptr;
	cut_chunks(p, m.tp, m.dev.dp.spec_stride);
	if (!m.tp.use_chunks) return WHAMD_OK;
	const uint32_t stride = m.dev.dp.spec_stride;
	HIP_TRY(up.up((void**)&m.dev.d_chunks, m.tp.chunks.data(), m.tp.chunks.size() * sizeof(BtChunk)));
	HIP_TRY(up.alloc((void**)&m.dev.d_unit_x, (size_t)m.tp.n_orient_max * m.tp.units.size() * 4));
	HIP_TRY(up.alloc((void**)&m.dev.d_path2, (size_t)m.tp.n_orient_max * n * 4));
	HIP_TRY(up.alloc((void**)&m.dev.d_trans2, (size_t)m.tp.n_orient_max * n * 4));
	HIP_TRY(up.alloc((void**)&m.dev.d_sel, m.tp.units.size() + 16));
	HIP_TRY(up.alloc((void**)&m.dev.d_guess, m.tp.chunks.size() * 4));
	if (m.preview.spec_keys && m.preview.spec_bytes >= ((size_t)m.tp.n_spec + 1) * stride * 8) m.dev.dp.spec_keys = m.preview.spec_keys;   // (armed, and being written by the preview's launches)
	else HIP_TRY(up.alloc((void**)&m.dev.dp.spec_keys, ((size_t)m.tp.n_spec + 1) * stride * 8));
	return WHAMD_OK;
}

// The backtrace arena of `bytes`: from the arena cache, else from the driver.
whamd_status_t DeviceTable::Impl::take_arena(uint64_t bytes, std::string& msg) {
	Impl& m = *this;
	size_t got = 0;
	void* d_bt = arena_take(m.device, bytes, got);
	if (!d_bt) {
		HIP_TRY(hipMalloc(&d_bt, std::max<size_t>(bytes, 16)));
		got = std::max<size_t>(bytes, 16);
	}
	m.dev.d_arena = d_bt;
	m.dev.arena_bytes = got;
	return WHAMD_OK;
}

// The units' device copy, the LDS sizes of the two backtrace kernels, the runs' table block, the backtrace arena (b.bt bytes), key scratch, the two exchange
// buffers of lane 0 and the pinned block a solve downloads into.
whamd_status_t DeviceTable::Impl::take_solve_buffers(const Problem& p, TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	HIP_TRY(up.up((void**)&m.dev.d_units, m.tp.units.data(), m.tp.units.size() * sizeof(BtUnit)));
	backtrace_lds_sizes(b, m.tp);
	void* d_rtab = nullptr;
	const bool ped_plan = !m.tp.plan.ped_columns.empty();
	HIP_TRY(up.alloc(&d_rtab, m.tp.plan.columns.size() * (ped_plan ? PED_TABLE : RES_TABLE) * sizeof(int32_t)));
	m.dev.dp.res_tables = ped_plan ? nullptr : (int32_t*)d_rtab;
	m.dev.dp.ped_tables = ped_plan ? (int32_t*)d_rtab : nullptr;
	b.laps.lap("jobs, backtrace units, schedule");
	b.laps.next_stage();
	{
		if (m.dev.d_arena && m.dev.arena_bytes < std::max<size_t>(b.bt, 16)) {   // the preview took an arena that turns out too small: its launches are given up
			HIP_TRY(hipStreamSynchronize(m.stream));
			arena_give(m.device, m.dev.d_arena, m.dev.arena_bytes);
			m.dev.d_arena = nullptr;
			m.dev.arena_bytes = 0;
		}
		if (!m.dev.d_arena) {   // (else: the arena the preview's launches are writing their records into)
			const whamd_status_t taken = m.take_arena(b.bt, msg);
			if (taken != WHAMD_OK) return taken;
		}
		m.dev.dp.bt = (uint8_t*)m.dev.d_arena;
	}
	b.laps.next_stage();
	m.dev.key_entries = (size_t)(1ull << b.max_keys_f) * p.T;
	HIP_TRY(up.alloc((void**)&m.dev.dp.keys, m.dev.key_entries * 8));
	HIP_TRY(up.alloc((void**)&m.dev.dp.last_keys, (size_t)MAX_T_WIDE * 8));
	if (m.preview.d_pr[0] && m.preview.exchange_bytes >= b.exchange_bytes) {   // (the exchange columns the preview's launches are handing each other)
		m.dev.d_pr[0] = m.preview.d_pr[0];
		m.dev.d_pr[1] = m.preview.d_pr[1];
	} else {
		HIP_TRY(up.alloc((void**)&m.dev.d_pr[0], b.exchange_bytes));
		HIP_TRY(up.alloc((void**)&m.dev.d_pr[1], b.exchange_bytes));
	}
	HIP_TRY(pinned_take((m.tp.super_off + (m.tp.device_superreads ? m.tp.super_words : 0)) * sizeof(uint32_t), (void**)&m.dev.h_pinned, &m.dev.h_pinned_bytes));
	return WHAMD_OK;
}

// Lanes (assign_lanes): lane 0 runs on the table's buffers; every other lane gets exchange buffers and key scratch of its own.
whamd_status_t DeviceTable::Impl::make_lanes(const TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	assign_lanes(m.opt, b, m.tp);
	m.tp.lanes[0].d_pr[0] = m.dev.d_pr[0];
	m.tp.lanes[0].d_pr[1] = m.dev.d_pr[1];
	m.tp.lanes[0].d_keys = m.dev.dp.keys;
	for (size_t l = 1; l < m.tp.lanes.size(); ++l) {
		HIP_TRY(up.alloc((void**)&m.tp.lanes[l].d_pr[0], b.exchange_bytes));
		HIP_TRY(up.alloc((void**)&m.tp.lanes[l].d_pr[1], b.exchange_bytes));
		HIP_TRY(up.alloc((void**)&m.tp.lanes[l].d_keys, m.dev.key_entries * 8));
	}
	return WHAMD_OK;
}

// The entries of the batched launches and the backtrace jobs: the last arrays of the image.
whamd_status_t DeviceTable::Impl::upload_entries(TableUploader& up, std::string& msg) {
	Impl& m = *this;
	HIP_TRY(up.up((void**)&m.dev.d_entries, m.tp.entries.data(), m.tp.entries.size() * sizeof(ResBatchEntry)));
	m.tp.slot_entries.resize(m.tp.slot_entries.size() + 2);   // (two unused entries behind the last: a group launch warms 512 bytes behind its own entry, slot_runx_stream_core)
	HIP_TRY(up.up((void**)&m.dev.d_slot_entries, m.tp.slot_entries.data(), m.tp.slot_entries.size() * sizeof(SlotBatchEntry)));
	m.tp.slot_entries.resize(m.tp.slot_entries.size() - 2);
	std::vector<BtJob> btjobs;
	for (const Job& job : m.tp.jobs) btjobs.push_back(BtJob{job.unit_off, job.unit_count, job.final ? 1u : 0u, 0u});
	HIP_TRY(up.up((void**)&m.dev.d_btjobs, btjobs.data(), btjobs.size() * sizeof(BtJob)));
	return WHAMD_OK;
}

// The rest of the image leaves; behind it the kernels that build the slot runs' tables, once per table (blockIdx.y = run); `ev_upload` marks the end of it all.
whamd_status_t DeviceTable::Impl::launch_table_kernels(const Problem& p, const TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	const hipStream_t us = up.stream;
	HIP_TRY(up.flush());   // (everything is staged; the table kernels below read it)
	if (b.ped_slots) {
		// the cost-form tables of every run (slots.h)
		uint32_t most = 0;
		for (size_t ri = 0; ri < m.tp.splan.runs.size(); ++ri)
			most = std::max<uint32_t>(most, (m.tp.splan.pextra[ri].fwn << m.tp.splan.runs[ri].g) + (m.tp.splan.pextra[ri].fwn << m.tp.splan.runs[ri].lw) + m.tp.splan.runs[ri].ncols * (64u * pslot_ns(m.tp.splan.pextra[ri].nf) + p.T * pslot_nk(m.tp.splan.pextra[ri].nf)));
		const uint32_t bx = std::max(1u, std::min(1024u, (most + 255u) / 256u));
		for (size_t r0 = 0; r0 < m.tp.splan.runs.size(); r0 += 32768) {   // (gridDim.y <= 65535)
			const uint32_t ny = (uint32_t)std::min<size_t>(32768, m.tp.splan.runs.size() - r0);
			hipLaunchKernelGGL(pedslot_tables, dim3(bx, ny), dim3(256), 0, us, m.dev.dp, b.d_runs + r0, b.d_pextra + r0, (uint32_t*)m.dev.dp.pslot_tab, b.d_fterms);
		}
		HIP_TRY(hipGetLastError());
	}
	if (m.tp.use_slots && !b.ped_slots && !m.tp.splan.runs.empty()) {
		uint32_t most = 0;
		for (const SlotRun& run : m.tp.splan.runs) most = std::max<uint32_t>(most, ((run.ncols + 8u) << (run.g - run.half)) + (run.ncols + 8u) * ((run.threads >> 6) + 64u));
		const uint32_t bx = std::max(1u, std::min(64u, (most + 255u) / 256u));
		for (size_t r0 = 0; r0 < m.tp.splan.runs.size(); r0 += 32768) {
			const uint32_t ny = (uint32_t)std::min<size_t>(32768, m.tp.splan.runs.size() - r0);
			hipLaunchKernelGGL(slot_tables, dim3(bx, ny), dim3(256), 0, us, m.dev.dp, b.d_runs + r0, (uint32_t*)m.dev.dp.slot_tab);
		}
		HIP_TRY(hipGetLastError());
	}
	// No host wait: the solve is ordered behind `ev_upload` on the device (begin_solve) and the staging area behind its own event (StageSession::park) -- a create
	// used to end with hipStreamSynchronize: 1.5 - 2 ms of copy tail and table kernel for configs[2], and under many concurrent creates every worker thread sat in
	// the queue of the others' copies (half of a create's wall time at 16 workers).  WHAMD_SYNC_UPLOAD=1 (debug library) restores the wait.
	HIP_TRY(hipEventRecord(m.ev_upload, us));
	m.upload_pending = true;
	if (debug_env("WHAMD_SYNC_UPLOAD") || up.unstaged_copies || !up.stage.image || !up.stage.park()) {
		HIP_TRY(hipStreamSynchronize(us));
		up.stage.finish();
	}
	return WHAMD_OK;
}

// The in-kernel cycle stamps and timing experiments of the debug library (m.dev.dp.dbg, dbg_wg_off, dbg_flags).
whamd_status_t DeviceTable::Impl::arm_debug_stamps(TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.dev.dp.dbg = nullptr;
	if (debug_env("WHAMD_DEBUG_STAMPS") && !m.tp.use_slots) {   // in-kernel cycle stamps of the LDS-resident runs (WHAMD_DEBUG_TIMING: host phases only)
		const size_t dbg_bytes = (m.tp.plan.segments.size() + 1) * 64 + 4 * 512 * 16 + 64;
		HIP_TRY(up.alloc((void**)&m.dev.dp.dbg, dbg_bytes));
		HIP_TRY(hipMemset(m.dev.dp.dbg, 0, dbg_bytes));
		m.dev.dp.dbg_wg_off = (uint32_t)((m.tp.plan.segments.size() + 1) * 8);
		m.dev.dp.dbg_flags = (uint32_t)atoi(debug_env("WHAMD_DEBUG_STAMPS"));
	}
	bool wave_stamps = false;
	if (debug_env("WHAMD_SLOT_STAMPS") && m.tp.use_slots) {   // in-kernel cycle stamps of workgroup 0 / wave 0 of every slot run
		wave_stamps = atoi(debug_env("WHAMD_SLOT_STAMPS")) >= 2;   // (= 2: every wave of three workgroups of every X run, behind the other stamps)
		const size_t dbg_bytes = (m.tp.splan.runs.size() + 1) * 48 * 8 + 4 * 512 * 16 + 128 +   // + the backtrace kernel's own stamps
		                         (wave_stamps ? (m.tp.splan.runs.size() + 1) * SLOT_WAVE_STAMP_WGS * SLOT_WAVE_STAMP_WORDS * 8 : 0);
		HIP_TRY(up.alloc((void**)&m.dev.dp.dbg, dbg_bytes));
		HIP_TRY(hipMemset(m.dev.dp.dbg, 0, dbg_bytes));
		m.dev.dp.dbg_wg_off = (uint32_t)((m.tp.splan.runs.size() + 1) * 48);
		for (size_t i = 0; i < m.tp.slot_entries.size(); ++i) m.tp.slot_entries[i].run.pad = (uint32_t)i;
	}
	if (const char* skip = debug_env("WHAMD_SLOT_SKIP")) m.dev.dp.dbg_flags = (uint32_t)atoi(skip);  // timing experiments (results invalid): 1 no exit
	                                                                                          // stores, 2 no records, 4 one column per run, 8 no ending reads, 16 no cost update
	if (wave_stamps) m.dev.dp.dbg_flags |= 256u;   // (the X runs keep per-wave stamps INSTEAD of wave 0's column stamps)
	return WHAMD_OK;
}

// Kernels with more than 64 KiB of dynamic LDS need the opt-in on every device they run on -- once per process and device (23 driver calls
// per table were a tenth of a coverage-15 create when many tables are built at once).
// (The array is a function of its own because the debug library's kernel registry reads it too: the registry's large_lds_opted_in IS this array.)
static const void* const* large_lds_kernels(size_t& count) {
#define K(...) reinterpret_cast<const void*>((__VA_ARGS__))
#define WHAMD_RUNX(XC, STAMPS) K(slot_runx<2, XC, STAMPS, false>), K(slot_runx<2, XC, STAMPS, true>)
#define WHAMD_PSLOT(TBV, NFV) K(pedslot_run<TBV, NFV, false, false>), K(pedslot_run<TBV, NFV, false, true>), K(pedslot_run<TBV, NFV, true, false>), K(pedslot_run<TBV, NFV, true, true>)
#define WHAMD_PSLOTX(TBV, NFV) K(pedslot_runx<TBV, NFV, 32, false>), K(pedslot_runx<TBV, NFV, 32, true>)
	// (The compiler emits the instantiations in the order they are first named, here: a reordered table is a reordered code object.  The debug
	// library's additions -- cycle stamps, pedigree X runs -- stand where it has always named them.)
	static const void* const kernels[] = {
		K(resident_segment<false, false>), K(resident_segment<false, true>),
#ifdef WHAMD_DEBUG_BUILD
		K(resident_segment<true, true>),
#endif
		K(resident_batch<false>), K(resident_batch<true>), K(backtrace_kernel), K(resident_segment_ped<false>),
#ifdef WHAMD_DEBUG_BUILD
		K(resident_segment_ped<true>),
#endif
		K(resident_segment_ped<false, true>),
		// every instantiation launch_slot_run / enqueue_group may pick: a 9..16-column run of 512 threads needs slotx_lds_bytes(512, 16) = 72 KB, above the
		// 64 KB a kernel gets without the attribute (XC = 0: streamed operands, 16 KB; XC = 8: 56 KB -- registered all the same, the limit is per function)
		WHAMD_RUNX(24, false), WHAMD_RUNX(32, false), WHAMD_RUNX(0, false), WHAMD_RUNX(8, false), WHAMD_RUNX(16, false),
		K(slot_groupx<2, false>), K(slot_groupx<3, false>),
#ifdef WHAMD_DEBUG_BUILD
		WHAMD_RUNX(24, true), WHAMD_RUNX(32, true),
		WHAMD_PSLOTX(2, 2), WHAMD_PSLOTX(2, 4), WHAMD_PSLOTX(4, 2), WHAMD_PSLOTX(4, 4), WHAMD_PSLOTX(2, 16), WHAMD_PSLOTX(2, PSLOT_FACT),
#endif
		WHAMD_PSLOT(2, 4), WHAMD_PSLOT(4, 2), WHAMD_PSLOT(4, 4),
		WHAMD_PSLOT(2, 16), K(pedslot_group<2, 16>),
		WHAMD_PSLOT(2, PSLOT_FACT), K(pedslot_group<2, PSLOT_FACT>),
		WHAMD_PSLOT(4, PSLOT_FACT4), K(pedslot_group<4, PSLOT_FACT4>),
		K(pedslot_group<2, 2>), K(pedslot_group<2, 4>), K(pedslot_group<4, 2>), K(pedslot_group<4, 4>),
	};
#undef K
#undef WHAMD_RUNX
#undef WHAMD_PSLOT
#undef WHAMD_PSLOTX
	count = sizeof(kernels) / sizeof(kernels[0]);
	return kernels;
}

static whamd_status_t opt_in_large_lds(int device, std::string& msg) {
	static std::mutex attr_mu;
	static unsigned long long attr_done = 0;   // bit = device
	std::lock_guard<std::mutex> lock(attr_mu);
	if (device < 64 && ((attr_done >> device) & 1ull)) return WHAMD_OK;
	size_t count = 0;
	const void* const* kernels = large_lds_kernels(count);
	for (size_t i = 0; i < count; ++i) HIP_TRY(hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)CU_LDS_BYTES));
	if (device < 64) attr_done |= 1ull << device;
	return WHAMD_OK;
}

// What a batched backtrace launch reads for this table (BtGroupEntry): a copy of the finished m.dev.dp and the walk's buffers, on the device behind `ev_upload`.
whamd_status_t DeviceTable::Impl::record_group_backtrace(uint32_t n, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.dev.d_bt_entry = nullptr;
	if (!m.tp.use_chunks) return WHAMD_OK;
	BtGroupEntry& e = m.dev.h_bt_entry;
	e = BtGroupEntry{};
	e.P = m.dev.dp;
	e.units = m.dev.d_units; e.chunks = m.dev.d_chunks;
	e.n_chunks = (uint32_t)m.tp.chunks.size(); e.n_units = (uint32_t)m.tp.units.size(); e.n_orient_max = m.tp.n_orient_max; e.n_cols = n;
	e.path2 = m.dev.d_path2; e.trans2 = m.dev.d_trans2; e.out_score = m.dev.d_score; e.unit_x2 = m.dev.d_unit_x; e.guess = m.dev.d_guess; e.sel = m.dev.d_sel; e.counters = m.dev.d_bt_counters;
	e.path_index = m.dev.d_path_index; e.path_trans = m.dev.d_path_trans;
	if (m.tp.device_superreads) e.super = m.dev.super_args;
	void* d_entry = nullptr;
	HIP_TRY(up.alloc(&d_entry, sizeof(BtGroupEntry)));
	HIP_TRY(hipMemcpyAsync(d_entry, &m.dev.h_bt_entry, sizeof(BtGroupEntry), hipMemcpyHostToDevice, up.stream));   // (the source is a member: it outlives the copy)
	HIP_TRY(hipEventRecord(m.ev_upload, up.stream));
	m.dev.d_bt_entry = (BtGroupEntry*)d_entry;
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- the preview
// A lone single-individual table's device sits idle through its whole create, and nothing of the create's second half -- column descriptors, the arena's layout,
// staging and sending ~100 MB, backtrace units, schedule -- is needed by the FIRST launches, which read the rows, control words and tables of their own
// columns only.  Right behind the plan this function therefore uploads exactly that for the runs plan_preview chose (a prefix of the arrays the table will
// upload whole: every offset a run carries is the same in both), takes the buffers the solve will write -- arena, exchange columns, seeds -- and launches those
// runs on the table's own stream, with an event behind the last.  Nothing plan_preview worked out is trusted: verify_preview holds the finished schedule against it.
whamd_status_t DeviceTable::Impl::start_preview(const Problem& p, TableBuild& b, bool from_create, std::string& msg) {
	Impl& m = *this;
	Preview& pv = m.preview;
	PreviewPlan pp;
	plan_preview(p, m.opt, b, m.tp, from_create, m.alone_on_device(), pp);
	pv.why = pp.why;
	if (pp.why != PV_RAN) return WHAMD_OK;
	const uint32_t n = b.n, S = pp.steps, pieces = pp.pieces, end_col = pp.end_col, n_spec = pp.n_spec, stride = pp.stride, max_f = pp.max_f;
	const uint64_t bt = pp.arena, tab_words = pp.tab_words;
	const size_t ctrl_words = pp.ctrl_words;
	const bool chunked = pp.chunked;
	const std::vector<uint64_t>& rec = pp.rec;
	const std::vector<uint32_t>& spec = pp.spec;
	const std::vector<SlotRun>& runs = m.tp.splan.runs;
	b.laps.lap("preview: steps, offsets, seeds (host)");
	// ---- the buffers the solve writes: the table's from here on
	{
		const whamd_status_t taken = m.take_arena(bt, msg);
		if (taken != WHAMD_OK) return taken;
	}
	pv.exchange_bytes = (size_t)(1ull << max_f) * p.T * 4;
	HIP_TRY(pool_alloc(m.device, m.dev.allocations, (void**)&pv.d_pr[0], pv.exchange_bytes));
	HIP_TRY(pool_alloc(m.device, m.dev.allocations, (void**)&pv.d_pr[1], pv.exchange_bytes));
	pv.spec_bytes = chunked ? ((size_t)n_spec + 1) * stride * 8 : 0;
	if (chunked) HIP_TRY(pool_alloc(m.device, m.dev.allocations, (void**)&pv.spec_keys, pv.spec_bytes));
	// ---- the preview's own arrays: a prefix of the table's rows, control words and runs; its tables
	DevProblem hdp{};
	hdp.n_cols = n; hdp.T = p.T; hdp.tbits = b.tbits; hdp.n_ind = p.n_ind;
	{
		const hipStream_t us = m.upload_stream;
		TableUploader up(m.device, us, pv.allocations);
		const size_t row_count = (size_t)end_col + SLOT_ROW_PAD;
		up.open_block(row_count * sizeof(SlotRow) + ctrl_words * 4 + (size_t)S * sizeof(SlotRun) + 4096);
		const SlotRun* d_runs = nullptr;
		HIP_TRY(up.up((void**)&hdp.slot_rows, m.tp.splan.rows.data(), row_count * sizeof(SlotRow)));
		HIP_TRY(up.up((void**)&hdp.slot_ctrl, m.tp.splan.ctrl.data(), ctrl_words * 4));
		HIP_TRY(up.up((void**)&d_runs, runs.data(), (size_t)S * sizeof(SlotRun)));
		HIP_TRY(up.alloc((void**)&hdp.slot_tab, tab_words * 4));
		HIP_TRY(up.flush());
		uint32_t most = 0;
		for (uint32_t k = 0; k < S; ++k) most = std::max<uint32_t>(most, ((runs[k].ncols + 8u) << (runs[k].g - runs[k].half)) + (runs[k].ncols + 8u) * ((runs[k].threads >> 6) + 64u));
		const uint32_t bx = std::max(1u, std::min(64u, (most + 255u) / 256u));
		for (uint32_t r0 = 0; r0 < S; r0 += 32768) hipLaunchKernelGGL(slot_tables, dim3(bx, std::min<uint32_t>(32768, S - r0)), dim3(256), 0, us, hdp, d_runs + r0, (uint32_t*)hdp.slot_tab);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(m.ev_upload, us));   // (the create records it again behind the table's own uploads; the wait below keeps this record)
		if (up.unstaged_copies || !up.stage.image || !up.stage.park()) {
			HIP_TRY(hipStreamSynchronize(us));
			up.stage.finish();
		}
	}
	b.laps.lap("preview: rows, control words, tables: allocations + copies");
	// ---- armed once, then the launches
	{
		const whamd_status_t opted = opt_in_large_lds(m.device, msg);   // (the first table of a process: an X run's LDS is above what a kernel gets without)
		if (opted != WHAMD_OK) return opted;
	}
	const hipStream_t rs = m.stream;
	m.inflight.run_stream = rs;
	m.own_stream_used = true;
	HIP_TRY(hipStreamWaitEvent(rs, m.ev_upload, 0));
	hdp.bt = (uint8_t*)m.dev.d_arena;
	hdp.spec_keys = pv.spec_keys;
	hdp.spec_stride = stride;
	if (chunked) HIP_TRY(hipMemsetAsync(pv.spec_keys, 0xFF, pv.spec_bytes, rs));
	m.inflight.timing_pending = false;   // (the events are the coming solve's from here on)
	HIP_TRY(hipEventRecord(m.ev0, rs));
	m.tp.use_chunks = chunked;   // (launch_slot_run: a run leaves a seed where the backtrace is chunked)
#ifdef WHAMD_DEBUG_BUILD
	m.ledger.clear();
#endif
	pv.runs.resize(S);
	uint64_t launches = 0;
	pv.launching = true;   // (the ledger marks these lines)
	if (b.laps.on)
		fprintf(stderr, "[whamd timing] preview: first launch %.2f ms after the create's upload began, at t = %.2f ms (%s)\n", b.laps.since_origin_ms(), timing_stamp_ms(),
		        pv.from_hook ? "from the planner's head hook" : "behind the plan");
	for (uint32_t k = 0; k < S; ++k) {
		SlotBatchEntry e{};
		e.run = runs[k];
		if (k == 0) e.run.has_prev = 0;   // (make_schedule: a job starts from cost 0)
		e.run.rec_lo = (uint32_t)rec[k];
		e.run.rec_hi = (uint32_t)(rec[k] >> 32);
		e.run.spec_id = spec[k];
		e.prev = pv.d_pr[k & 1u];
		e.cur = pv.d_pr[(k & 1u) ^ 1u];
		pv.runs[k] = e.run;
		m.launch_slot_run(hdp, e, launches);
	}
	pv.launching = false;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(m.ev3, rs));   // "the preview is done": a solve that starts over on another stream waits for it there (begin_solve); the solve's tail records ev3 anew
	pv.dp = hdp;
	pv.use_chunks = chunked;
	pv.why = PV_RAN;
	pv.pieces = pieces;
	pv.launched = S;
	pv.launches = launches;
	pv.pending = true;
	b.laps.lap("preview: launches submitted");
	return WHAMD_OK;
}

// The finished table against its preview: S = the leading super-steps of the schedule that are, launch for launch, what the preview launched -- the same run by
// value (every field: the preview's arrays are prefixes of the table's, so even the offsets into them agree), the same exchange columns, arena and seeds, and the
// same facts behind the choice of kernel, grid and LDS (launch_slot_run decides from the run, the problem's debug fields, use_chunks and side_by_side).
void DeviceTable::Impl::verify_preview() {
	Impl& m = *this;
	Preview& pv = m.preview;
	pv.agreed = 0;
	if (!pv.launched) return;
	const bool same_ground = m.tp.use_slots && !m.tp.windowed && m.tp.jobs.size() == 1 && m.tp.lanes.size() == 1 && m.dev.dp.bt == pv.dp.bt && m.dev.dp.spec_keys == pv.dp.spec_keys &&
	                         m.tp.use_chunks == pv.use_chunks && (!m.tp.use_chunks || m.dev.dp.spec_stride == pv.dp.spec_stride) && !m.dev.dp.dbg && !m.dev.dp.dbg_flags &&
	                         m.dev.d_pr[0] == pv.d_pr[0] && m.dev.d_pr[1] == pv.d_pr[1] && !m.opt.side_by_side;
	for (uint32_t k = 0; same_ground && k < pv.launched && k + 1 < m.tp.schedule.size(); ++k) {
		const SuperStep& ss = m.tp.schedule[k];
		if (ss.entry_count != 1 || !ss.singles.empty() || ss.ck_load >= 0 || ss.ck_save >= 0 || ss.bt_window >= 0) break;
		const SlotBatchEntry& e = m.tp.slot_entries[ss.entry_off];
		if (std::memcmp(&e.run, &pv.runs[k], sizeof(SlotRun)) != 0 || e.prev != pv.d_pr[k & 1u] || e.cur != pv.d_pr[(k & 1u) ^ 1u] || e.score_out) break;
		++pv.agreed;
	}
	if (const char* at = debug_env("WHAMD_PREVIEW_MISMATCH_AT")) pv.agreed = std::min<uint32_t>(pv.agreed, (uint32_t)std::max(0, atoi(at)));   // (debug library: "step `at` differs")
	if (getenv("WHAMD_DEBUG_TIMING"))
		fprintf(stderr, "[whamd timing] preview: %u plan pieces, %u steps launched, %u agree with the schedule\n", pv.pieces, pv.launched, pv.agreed);
}

// Everything whamd_dptable_create does after the planner, phase by phase (DESIGN.md 6.1 lists what crosses between them).
whamd_status_t DeviceTable::upload(Problem& p, int device, std::string& msg, bool from_create) {
	Impl& m = *impl_;
	whamd_status_t st = m.open(device, msg);
	if (st != WHAMD_OK || p.n_cols == 0) return st;
	TableBuild b;
	b.n = p.n_cols;
	b.tbits = 2 * p.n_triples;
	b.ni = std::max<uint32_t>(p.n_ind, 1);
	m.dev.dp.n_cols = b.n;
	m.dev.dp.T = p.T;
	m.dev.dp.tbits = b.tbits;
	m.dev.dp.n_ind = p.n_ind;
	// ---- everything this function sends or launches goes through one of the device's upload streams (upload_stream_of); begin_solve orders the solve behind
	// ev_upload.  WHAMD_UPLOAD_ON_TABLE_STREAM=1 (debug library): the table's own stream, as before.  (Chosen in front of the plan: a preview may start inside it.)
	m.upload_stream = debug_env("WHAMD_UPLOAD_ON_TABLE_STREAM") ? nullptr : upload_stream_of(device);
	if (!m.upload_stream) m.upload_stream = m.stream;
	if (m.upload_stream == m.stream) m.own_stream_used = true;
	// ---- host: path and plan, column descriptors, the layout of the backtrace arena
	if ((st = m.choose_plan(p, b, from_create, msg)) != WHAMD_OK) return st;
	b.ped_slots = m.tp.use_slots && m.tp.splan.ped;
	b.laps.next_stage();
	if (debug_env("WHAMD_DEBUG_PLAN")) m.dump_plan(p);
	// ---- a lone table: its first runs start on the device -- from inside the planner (choose_plan's head hook), or here --, and the rest of the create happens under them
	if (!m.preview.tried && (st = m.start_preview(p, b, from_create, msg)) != WHAMD_OK) return st;
	if ((st = describe_columns(p, b, m.tp, msg)) != WHAMD_OK) return st;
	if ((st = lay_out_arena(p, m.opt, b, m.tp, msg)) != WHAMD_OK) return st;
	TableUploader up(device, m.upload_stream, m.dev.allocations);
	b.laps.lap("staging area taken");
	up.open_block(upload_bound(p, b, m.tp));
	b.laps.lap("staging image sized, device block taken");
	// ---- the device block fills in this order; the image leaves in pieces of 32 MB
	if ((st = m.upload_column_arrays(p, b, up, msg)) != WHAMD_OK) return st;
	if ((st = m.upload_slot_arrays(b, up, msg)) != WHAMD_OK) return st;
	make_jobs(m.opt, m.tp);
	make_units(b, m.tp);
	if ((st = m.make_windows(b, up, msg)) != WHAMD_OK) return st;
	if ((st = m.take_result_block(b.n, up, msg)) != WHAMD_OK) return st;
	if ((st = m.make_chunks(p, up, msg)) != WHAMD_OK) return st;
	if ((st = m.take_solve_buffers(p, b, up, msg)) != WHAMD_OK) return st;
	if ((st = m.make_lanes(b, up, msg)) != WHAMD_OK) return st;
	if ((st = make_schedule(b, m.dev.dp, m.dev.d_job_scores, m.tp, msg)) != WHAMD_OK) return st;
	make_briefs(m.tp);
	if ((st = m.upload_entries(up, msg)) != WHAMD_OK) return st;
	// ---- the image's tail and the table kernels go out; what follows only completes what the solve's launches read
	if ((st = m.launch_table_kernels(p, b, up, msg)) != WHAMD_OK) return st;
	b.laps.summary((double)b.bt / 1e9);
	if ((st = m.arm_debug_stamps(up, msg)) != WHAMD_OK) return st;
	if ((st = opt_in_large_lds(device, msg)) != WHAMD_OK) return st;
	if ((st = m.record_group_backtrace(b.n, up, msg)) != WHAMD_OK) return st;
	m.verify_preview();
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- launch tables of the solve
// Which instantiation a run takes, one function per kernel signature; the launch_* functions and the group's flush compute grid, block and LDS, ask here
// and launch.  (They stand here, and in this order, because the instantiations are emitted in the order they are first named: see opt_in_large_lds.  The
// instantiations with cycle stamps and timing switches exist in the debug library only, debug_build.h: `stamps` is false in the product.)
namespace {

SegmentFn segment_kernel(bool stamps, bool sym) {
#ifdef WHAMD_DEBUG_BUILD
	if (stamps) return resident_segment<true, true>;
#endif
	return sym ? resident_segment<false, true> : resident_segment<false, false>;
}

PedSegmentFn ped_segment_kernel(bool stamps, bool spec) {
#ifdef WHAMD_DEBUG_BUILD
	if (stamps) return resident_segment_ped<true>;
#endif
	return spec ? resident_segment_ped<false, true> : resident_segment_ped<false>;
}

ResBatchFn resident_batch_kernel(bool sym) { return sym ? resident_batch<true> : resident_batch<false>; }

#ifdef WHAMD_DEBUG_BUILD
// X run of a pedigree (kernels_pedslots.h pedslot_runx; WHAMD_PED_XRUN=1): the costs of xc = 16 or 32 columns formed in the prologue, scalars through the scalar cache
PedSlotRunFn pedslot_runx_kernel(uint32_t tb, uint32_t nf, uint32_t xc, bool spec) {
#define WHAMD_ROW(TB, NF) { pedslot_runx<TB, NF, 16, true>, pedslot_runx<TB, NF, 16, false>, pedslot_runx<TB, NF, 32, true>, pedslot_runx<TB, NF, 32, false> }
	static const PedSlotRunFn table[6][4] = {WHAMD_ROW(2, PSLOT_FACT), WHAMD_ROW(2, 16), WHAMD_ROW(2, 2), WHAMD_ROW(2, 4), WHAMD_ROW(4, 2), WHAMD_ROW(4, 4)};
#undef WHAMD_ROW
	const int row = tb == 2 ? (nf == (uint32_t)PSLOT_FACT ? 0 : nf == 16 ? 1 : nf == 2 ? 2 : 3) : (nf == 2 ? 4 : 5);
	return table[row][(xc == 16 ? 0 : 2) + (spec ? 0 : 1)];
}
#endif

PedSlotRunFn pedslot_run_kernel(uint32_t tb, uint32_t nf, bool spec, bool packed) {
#define WHAMD_ROW(TB, NF) { pedslot_run<TB, NF, true, true>, pedslot_run<TB, NF, true, false>, pedslot_run<TB, NF, false, true>, pedslot_run<TB, NF, false, false> }
	static const PedSlotRunFn table[7][4] = {WHAMD_ROW(2, PSLOT_FACT), WHAMD_ROW(4, PSLOT_FACT4), WHAMD_ROW(2, 16), WHAMD_ROW(2, 2), WHAMD_ROW(2, 4), WHAMD_ROW(4, 2), WHAMD_ROW(4, 4)};
#undef WHAMD_ROW
	const int row = tb == 2 && nf == (uint32_t)PSLOT_FACT ? 0 : tb == 4 && nf == (uint32_t)PSLOT_FACT4 ? 1 : tb == 2 ? (nf == 16 ? 2 : nf == 2 ? 3 : 4) : (nf == 2 ? 5 : 6);
	return table[row][(spec ? 0 : 2) + (packed ? 0 : 1)];
}

// X run of a single individual, four cells per thread; xc: columns whose operands the prologue forms (0: streamed operands, which has no form with stamps)
SlotRunXFn slot_runx_kernel(uint32_t xc, bool stamps, bool spec) {
#define WHAMD_PAIR(XC, STAMPS) { slot_runx<2, XC, STAMPS, true>, slot_runx<2, XC, STAMPS, false> }
#ifdef WHAMD_DEBUG_BUILD
	static const SlotRunXFn stamped[2][2] = {WHAMD_PAIR(24, true), WHAMD_PAIR(32, true)};
	if (stamps && xc) return stamped[xc == 24 ? 0 : 1][spec ? 0 : 1];
#endif
	static const SlotRunXFn table[5][2] = {WHAMD_PAIR(0, false), WHAMD_PAIR(8, false), WHAMD_PAIR(16, false), WHAMD_PAIR(24, false), WHAMD_PAIR(32, false)};
#undef WHAMD_PAIR
	return table[xc / 8][spec ? 0 : 1];
}

// Slot run of a single individual: 2^lr cells per thread; Y form (slot_plan.cpp): one instruction per cell-column
SlotRunFn slot_run_kernel(uint32_t lr, bool yform, bool stamps, bool spec) {
#ifdef WHAMD_DEBUG_BUILD
#define WHAMD_ROW(LR, YF) { slot_run<LR, true, true, YF>, slot_run<LR, true, false, YF>, slot_run<LR, false, true, YF>, slot_run<LR, false, false, YF> }
#else
#define WHAMD_ROW(LR, YF) { nullptr, nullptr, slot_run<LR, false, true, YF>, slot_run<LR, false, false, YF> }
#endif
	static const SlotRunFn table[5][4] = {WHAMD_ROW(3, true), WHAMD_ROW(3, false), WHAMD_ROW(1, false), WHAMD_ROW(2, true), WHAMD_ROW(2, false)};
#undef WHAMD_ROW
	const int row = lr == 3 ? (yform ? 0 : 1) : lr == 1 ? 2 : (yform ? 3 : 4);
	return table[row][(stamps ? 0 : 2) + (spec ? 0 : 1)];
}

SlotBatchFn slot_batch_kernel(int lr) {
	if (lr == 1) return slot_batch<1>;
	if (lr == 3) return slot_batch<3>;
	return slot_batch<2>;
}

// tight: the variants held to 80 SGPRs (four workgroups per CU); dbg: the lead's timing switches (debug library)
GroupFn group_kernel(GroupVariant v, bool dbg, bool tight) {
	switch (v) {
		case GV_SINGLE4:
#ifdef WHAMD_DEBUG_BUILD
			if (dbg) return slot_group<2, true, false>;
#endif
			return tight ? slot_group<2, false, true> : slot_group<2, false, false>;
		case GV_PED_2_2: return pedslot_group<2, 2>;
		case GV_PED_2_4: return pedslot_group<2, 4>;
		case GV_PED_4_2: return pedslot_group<4, 2>;
		case GV_PED_4_4: return pedslot_group<4, 4>;
		case GV_PED_2_16: return pedslot_group<2, 16>;
		case GV_SINGLE8: return tight ? slot_group<3, false, true> : slot_group<3, false, false>;
		case GV_TRIO_FACT: return pedslot_group<2, PSLOT_FACT>;
		case GV_X4: return slot_groupx<2, false>;
		case GV_X8: return slot_groupx<3, false>;
		case GV_QUARTET_FACT: return pedslot_group<4, PSLOT_FACT4>;
		case GROUP_VARIANTS: break;
	}
	return nullptr;
}

}  // namespace

// ================================================================================================ solve: one table
// enqueue_some opens the solve (begin_solve), submits super-steps (submit_super_step) and, when none is left, the tail (submit_tail); wait collects.
// DESIGN.md 6.2 lists the steps and what crosses between them.
whamd_status_t DeviceTable::solve(const Problem& p, Solution& s, whamd_solve_stats& st, std::string& msg) {
	whamd_status_t status = enqueue(p, s, msg);
	if (status != WHAMD_OK) return status;
	return wait(p, s, st, msg);
}

whamd_status_t DeviceTable::enqueue(const Problem& p, Solution& s, std::string& msg) {
	bool done = false;
	whamd_status_t status = WHAMD_OK;
	while (status == WHAMD_OK && !done) status = enqueue_some(p, s, ~0ull, done, msg);
	return status;
}

// Launches one forward step on a lane's stream: reads `prev`, writes `cur`.
// One per-column step (column_step_fused, or column_step_keys + column_finalize) of a lane.
void DeviceTable::Impl::launch_column_step(const Problem& p, const Step& step, const Lane& lane, const uint32_t* prev, uint32_t* cur,
                                           uint64_t& launches) {
	Impl& m = *this;
	const hipStream_t rs = m.inflight.run_stream;
	DevProblem dp = m.dev.dp;
	dp.keys = lane.d_keys;
	const uint32_t c = step.index;
	const DevColumn& d = m.tp.cols[c];
#ifdef WHAMD_DEBUG_BUILD
	const auto column_facts = [&m](const Problem& pr, const DevColumn& col) { LaunchFacts f; f.T = (int32_t)pr.T; f.n_ind = (int32_t)m.dev.dp.n_ind; f.mode = (int32_t)col.mode; f.wide = m.tp.wide; return f; };
#endif
	if (d.mode == 0) {
		const uint32_t threads = 1u << d.f;
		const uint32_t block = std::min<uint32_t>(256, threads);
		hipLaunchKernelGGL(m.fused, dim3(threads / block), dim3(block), 0, rs, dp, c, prev, cur);
		WHAMD_NOTE(m, WHAMD_LAUNCH_COLUMN, (const void*)m.fused, dim3(threads / block), dim3(block), 0, rs, true, column_facts(p, d));
		launches += 1;
	} else {
		const uint64_t total = (1ull << (d.f + d.ebits - d.eloop)) * (m.tp.wide ? p.T : 1u);
		const uint32_t block = (uint32_t)std::min<uint64_t>(256, (total + 63) / 64 * 64);
		if (m.tp.wide) hipLaunchKernelGGL(column_step_wide, dim3((uint32_t)((total + block - 1) / block)), dim3(block), 0, rs, dp, c, prev, (uint32_t)total);
		else hipLaunchKernelGGL(m.keysfn, dim3((uint32_t)((total + block - 1) / block)), dim3(block), 0, rs, dp, c, prev, (uint32_t)total);
		WHAMD_NOTE(m, WHAMD_LAUNCH_COLUMN, m.tp.wide ? (const void*)column_step_wide : (const void*)m.keysfn, dim3((uint32_t)((total + block - 1) / block)), dim3(block), 0, rs, true, column_facts(p, d));
		const uint32_t entries = (1u << d.f) * p.T;
		const uint32_t fblock = std::min<uint32_t>(256, (entries + 63) / 64 * 64);
		hipLaunchKernelGGL(column_finalize, dim3((entries + fblock - 1) / fblock), dim3(fblock), 0, rs, dp, c, cur, entries);
		WHAMD_NOTE(m, WHAMD_LAUNCH_COLUMN, (const void*)column_finalize, dim3((entries + fblock - 1) / fblock), dim3(fblock), 0, rs, true, column_facts(p, d));
		launches += 2;
	}
}

// One run as a launch of its own (kernel arguments by value).
void DeviceTable::Impl::launch_run(const ResBatchEntry& e, uint64_t& launches) {
	Impl& m = *this;
	const ResSegment& sg = e.sg;
	const hipStream_t rs = m.inflight.run_stream;
	const bool stamps = DEBUG_BUILD && m.dev.dp.dbg != nullptr;
#ifdef WHAMD_DEBUG_BUILD
	const auto segment_facts = [&sg, stamps](bool spec, bool sym) {
		LaunchFacts f;
		f.ped = sg.kind == 1; f.stamps = stamps; f.ncols = (int32_t)sg.ncols; f.threads = (int32_t)sg.threads;
		if (sg.kind == 1) f.spec = spec; else f.sym = sym;
		return f;
	};
#endif
	const size_t lds = res_segment_lds_bytes(sg);
	if (sg.kind == 1) {
		const PedSegmentFn kernel = ped_segment_kernel(stamps, sg.in_mirror_bit && m.tp.use_chunks);
		hipLaunchKernelGGL(kernel, dim3(1u << sg.g), dim3(sg.threads), lds, rs, m.dev.dp, sg, e.prev, e.cur);
		WHAMD_NOTE(m, WHAMD_LAUNCH_RUN, (const void*)kernel, dim3(1u << sg.g), dim3(sg.threads), lds, rs, true, segment_facts(sg.in_mirror_bit && m.tp.use_chunks, false));
	} else {
		const SegmentFn kernel = segment_kernel(stamps, sg.half || sg.in_half || sg.mirror_out);
		hipLaunchKernelGGL(kernel, dim3(1u << (sg.g - sg.half)), dim3(sg.threads), lds, rs, m.dev.dp, sg, e.prev, e.cur, e.score_out);
		WHAMD_NOTE(m, WHAMD_LAUNCH_RUN, (const void*)kernel, dim3(1u << (sg.g - sg.half)), dim3(sg.threads), lds, rs, true, segment_facts(false, sg.half || sg.in_half || sg.mirror_out));
	}
	launches += 1;
}

// One slot run as a launch of its own (kernel arguments by value); `dp`: the table's problem, or the preview's with arrays of its own.
void DeviceTable::Impl::launch_slot_run(const DevProblem& dp, const SlotBatchEntry& e, uint64_t& launches) {
	Impl& m = *this;
	const SlotRun& run = e.run;
	const hipStream_t rs = m.inflight.run_stream;
	const bool spec = run.spec_id != 0 && m.tp.use_chunks && !debug_env("WHAMD_NO_SPEC_KERNEL");
	const bool stamps = DEBUG_BUILD && (dp.dbg != nullptr || dp.dbg_flags != 0);
	launches += 1;
	if (m.tp.splan.ped) {
		const PedSlotExtra& ex = m.tp.splan.pextra[e.pad];
		size_t lds = pedslot_lds_bytes(run.threads, run.ncols, ex);
		PedSlotRunFn kernel = pedslot_run_kernel(ex.tb, ex.nf, spec, (run.yflags & 16u) != 0);
#ifdef WHAMD_DEBUG_BUILD
		if ((run.yflags & 8u) && !m.opt.side_by_side) {   // X run (WHAMD_PED_XRUN=1)
			const uint32_t xc = run.ncols <= 16u ? 16u : 32u;
			lds = pedslotx_lds_bytes(run.threads, xc);
			kernel = pedslot_runx_kernel(ex.tb, ex.nf, xc, spec);
		}
#endif
		hipLaunchKernelGGL(kernel, dim3(1u << run.g), dim3(run.threads), lds, rs, dp, run, ex, e.prev, e.cur);
#ifdef WHAMD_DEBUG_BUILD
		LaunchFacts facts = LaunchFacts::of_run(run, spec, stamps);
		facts.ped = 1; facts.tb = (int32_t)ex.tb; facts.nf = (int32_t)ex.nf; facts.pack = (run.yflags & 16u) != 0;
		WHAMD_NOTE(m, WHAMD_LAUNCH_SLOT_RUN, (const void*)kernel, dim3(1u << run.g), dim3(run.threads), lds, rs, true, facts);
#endif
		return;
	}
	const dim3 grid(1u << (run.g - run.half)), block(run.threads);
	if ((run.yflags & 8u) && run.lr == 2u) {   // X run with four cells per thread: registers instead of LDS lines (LDS: the wave-slot exchange buffers + the threads' own operand lines)
		// (no LDS lines: room for other tables' workgroups on the CU -- or, from 1 024 workgroups on, for FOUR of this table's own instead of two:
		// a launch of 2 048 workgroups -- coverage 23 -- takes 36.2 instead of 56.2 us, scripts/gpu_wide_ab.py)
		const bool streamed = m.opt.side_by_side || debug_env("WHAMD_XSTREAM") || (grid.x >= 1024u && !debug_env("WHAMD_NO_WIDE_LAYOUT"));
		const size_t lds_x = streamed ? (size_t)2 * run.threads * 16 : slotx_lds_bytes(run.threads, (run.ncols + 7u) & ~7u);
		// narrow tables: the run's workgroups packed onto one XCD (slot_runx: eight times the grid, every eighth workgroup works)
		const uint32_t pack = (grid.x <= 32u && !m.opt.side_by_side && !debug_env("WHAMD_NO_XCD_PACK")) ? 1u : 0u;
		// the prologue forms the operands of XC columns (an irregular layout's runs are ~10 columns long); with stamps there are the two long forms only
		const uint32_t xc = streamed ? 0u : (run.ncols <= 8u && !stamps) ? 8u : (run.ncols <= 16u && !stamps) ? 16u : run.ncols <= 24u ? 24u : 32u;
		const SlotRunXFn kernel = slot_runx_kernel(xc, stamps, spec);
		hipLaunchKernelGGL(kernel, dim3(pack ? grid.x * 8u : grid.x), block, lds_x, rs, dp, run, e.prev, e.cur, e.score_out, pack);
#ifdef WHAMD_DEBUG_BUILD
		LaunchFacts facts = LaunchFacts::of_run(run, spec, stamps);
		facts.ped = 0; facts.streamed = streamed; facts.pack = (int32_t)pack;
		WHAMD_NOTE(m, WHAMD_LAUNCH_SLOT_RUN, (const void*)kernel, dim3(pack ? grid.x * 8u : grid.x), block, lds_x, rs, true, facts);
#endif
		return;
	}
	const size_t lds = slot_run_lds_bytes(run.threads, run.lr, run.ncols);   // wave-slot exchange + hot lines + per-wave A + lane sums
	const SlotRunFn kernel = slot_run_kernel(run.lr, (run.yflags & 1u) != 0, stamps, spec);
	hipLaunchKernelGGL(kernel, grid, block, lds, rs, dp, run, e.prev, e.cur, e.score_out);
#ifdef WHAMD_DEBUG_BUILD
	LaunchFacts facts = LaunchFacts::of_run(run, spec, stamps);
	facts.ped = 0;
	WHAMD_NOTE(m, WHAMD_LAUNCH_SLOT_RUN, (const void*)kernel, grid, block, lds, rs, true, facts);
#endif
}

// Resumable submission: the first call does the preamble, every call submits super-steps until at least `budget`
// launches went out, the call that runs out of super-steps appends the backtrace and the downloads.  Lets one host
// thread interleave the launch sequences of several tables (whamd_dptable_enqueue_many).
whamd_status_t DeviceTable::enqueue_some(const Problem& p, Solution& s, uint64_t budget, bool& done, std::string& msg) {
	const whamd_status_t status = enqueue_some_unguarded(p, s, budget, done, msg);
	if (status != WHAMD_OK) abort_enqueue();  // never leave a half-submitted schedule behind: the next enqueue starts over
	return status;
}

// Drops a partially submitted solve: waits for what is already on the stream and rewinds the resumable cursor, so that
// a later enqueue()/solve() of this table begins with the preamble again (key re-arm, events, path buffers).
void DeviceTable::abort_enqueue() {
	Impl& m = *impl_;
	if (m.stream) {
		(void)hipSetDevice(m.device);
		(void)hipStreamSynchronize(m.stream);
		(void)hipGetLastError();
	}
	m.inflight.rewind(m.stream);
}

// The key scratch of the per-column kernels and of the last column, all-ones, on the run stream.
whamd_status_t DeviceTable::Impl::arm_keys(std::string& msg) {
	Impl& m = *this;
	const hipStream_t rs = m.inflight.run_stream;
	for (const Lane& lane : m.tp.lanes) HIP_TRY(hipMemsetAsync(lane.d_keys, 0xFF, m.dev.key_entries * 8, rs));
	HIP_TRY(hipMemsetAsync(m.dev.dp.last_keys, 0xFF, (size_t)MAX_T_WIDE * 8, rs));
	return WHAMD_OK;
}

// The preamble of a solve on its run stream: path buffers, key re-arm, the start event, the lookup tables of the LDS-resident paths.
// behind_preview: the solve continues behind the table's preview (enqueue_some_unguarded decides) -- the cursor opens at the preview's last step; the seeds of
// the speculative backtrace and the start event were armed in front of the preview and stay; the key scratch, which no slot run reads, is armed here.
// In every other case a preview that is still pending is given up: the steps start over at 0, behind it in stream order or behind a host wait.
whamd_status_t DeviceTable::Impl::begin_solve(const Problem& p, Solution& s, std::string& msg, bool behind_preview) {
	Impl& m = *this;
	const hipStream_t rs = m.inflight.run_stream;
	const uint32_t n = p.n_cols;
	s.path_index.assign(n, 0);
	s.path_trans.assign(n, 0);
	s.superreads_done = false;
	if (m.preview.pending && !behind_preview && rs != m.stream) HIP_TRY(hipStreamWaitEvent(rs, m.ev3, 0));   // (its launches write what this solve's are about to write: ev3 stands behind the last)
	m.preview.pending = false;
	m.preview.continued = behind_preview;
	m.inflight.launches = behind_preview ? m.preview.launches : 0;
	m.inflight.next_super = behind_preview ? m.preview.agreed : 0;
#ifdef WHAMD_DEBUG_BUILD
	if (!behind_preview) m.ledger.clear();   // (the preview's launches are lines of this solve's ledger)
#endif
	if (n == 0) return WHAMD_OK;
	if (rs == m.stream) m.own_stream_used = true;
	if (m.ev_upload && (m.upload_pending || rs != m.stream)) HIP_TRY(hipStreamWaitEvent(rs, m.ev_upload, 0));   // (the uploads went through an upload stream; once a solve has been collected they are known to be there)
	{
		const whamd_status_t armed = m.arm_keys(msg);
		if (armed != WHAMD_OK) return armed;
	}
	if (behind_preview) {
		m.inflight.timing_pending = false;
		return WHAMD_OK;
	}
	if (m.tp.use_chunks) HIP_TRY(hipMemsetAsync(m.dev.dp.spec_keys, 0xFF, ((size_t)m.tp.n_spec + 1) * m.dev.dp.spec_stride * 8, rs));
	if (m.tp.windowed) HIP_TRY(hipMemsetAsync(m.dev.d_path_trans, 0, (size_t)n * 4, rs));
	m.inflight.timing_pending = false;   // (the events are this solve's from here on)
	HIP_TRY(hipEventRecord(m.ev0, rs));
	if (!m.tp.plan.ped_columns.empty()) {
		const uint32_t entries = (uint32_t)m.tp.plan.ped_columns.size() * PED_TABLE;
		hipLaunchKernelGGL(ped_tables, dim3((entries + 255) / 256), dim3(256), 0, rs, m.dev.dp.ped_cols, (uint32_t)m.tp.plan.ped_columns.size(), m.dev.dp.ped_tables);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TABLES, (const void*)ped_tables, dim3((entries + 255) / 256), dim3(256), 0, rs, false, LaunchFacts());
	} else if (!m.tp.use_slots && !m.tp.plan.columns.empty()) {
		const uint32_t entries = (uint32_t)m.tp.plan.columns.size() * RES_TABLE;
		hipLaunchKernelGGL(resident_tables, dim3((entries + 255) / 256), dim3(256), 0, rs, m.dev.dp.res_cols, (uint32_t)m.tp.plan.columns.size(), m.dev.dp.res_tables);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TABLES, (const void*)resident_tables, dim3((entries + 255) / 256), dim3(256), 0, rs, false, LaunchFacts());
	}
	return WHAMD_OK;
}

// One super-step of a table on its own: the kept column of a window boundary restored, the runs (one batched launch, or the single run as a launch of its
// own), the per-column steps, the column kept for a later window, the window's walk.
whamd_status_t DeviceTable::Impl::submit_super_step(const Problem& p, const SuperStep& ss, uint64_t& launches, std::string& msg) {
	Impl& m = *this;
	const hipStream_t rs = m.inflight.run_stream;
	const dim3 grid(ss.grid_x, ss.entry_count), block(ss.threads);
	if (ss.ck_load >= 0) HIP_TRY(hipMemcpyAsync(ss.io[0], m.dev.d_checkpoints + (size_t)ss.ck_load * m.tp.checkpoint_bytes, m.tp.checkpoint_bytes, hipMemcpyDeviceToDevice, rs));
	if (ss.entry_count == 1) {
		if (m.tp.use_slots) m.launch_slot_run(m.dev.dp, m.tp.slot_entries[ss.entry_off], launches);
		else m.launch_run(m.tp.entries[ss.entry_off], launches);
	} else if (ss.entry_count > 1) {
		if (m.tp.use_slots) { const SlotBatchFn kernel = slot_batch_kernel(m.tp.slot_lr_used); hipLaunchKernelGGL(kernel, grid, block, ss.lds, rs, m.dev.dp, m.dev.d_slot_entries + ss.entry_off); }
		else { const ResBatchFn kernel = resident_batch_kernel(ss.sym); hipLaunchKernelGGL(kernel, grid, block, ss.lds, rs, m.dev.dp, m.dev.d_entries + ss.entry_off); }
#ifdef WHAMD_DEBUG_BUILD
		LaunchFacts facts;
		facts.entries = (int32_t)ss.entry_count;
		if (m.tp.use_slots) facts.lr = m.tp.slot_lr_used; else facts.sym = ss.sym;
		WHAMD_NOTE(m, WHAMD_LAUNCH_BATCH, m.tp.use_slots ? (const void*)slot_batch_kernel(m.tp.slot_lr_used) : (const void*)resident_batch_kernel(ss.sym), grid, block, ss.lds, rs, true, facts);
#endif
		launches += 1;
	}
	const whamd_status_t st = m.submit_singles(p, ss, launches, msg);
	if (st != WHAMD_OK) return st;
	if (ss.ck_save >= 0) HIP_TRY(hipMemcpyAsync(m.dev.d_checkpoints + (size_t)ss.ck_save * m.tp.checkpoint_bytes, ss.io[1], m.tp.checkpoint_bytes, hipMemcpyDeviceToDevice, rs));
	if (ss.bt_window >= 0)
	{
		hipLaunchKernelGGL(backtrace_kernel, dim3(1), dim3(1024), m.tp.bt_lds, rs, m.dev.dp, m.dev.d_units, m.dev.d_window_jobs + ss.bt_window,
		                   m.dev.d_path_index, m.dev.d_path_trans, m.dev.d_score);
		WHAMD_NOTE(m, WHAMD_LAUNCH_WINDOW_WALK, (const void*)backtrace_kernel, dim3(1), dim3(1024), m.tp.bt_lds, rs, false, LaunchFacts());
	}
	return WHAMD_OK;
}

// The per-column steps of one super-step (each a launch of its own on the run stream).
whamd_status_t DeviceTable::Impl::submit_singles(const Problem& p, const SuperStep& ss, uint64_t& launches, std::string& msg) {
	Impl& m = *this;
	const hipStream_t rs = m.inflight.run_stream;
	for (const Single& sg : ss.singles) {
		const Lane& lane = m.tp.lanes[sg.lane];
		if (sg.zero_prev) HIP_TRY(hipMemsetAsync(lane.d_pr[sg.flip], 0, 4 * (size_t)p.T, rs));
		m.launch_column_step(p, m.tp.plan.steps[sg.step], lane, lane.d_pr[sg.flip], lane.d_pr[sg.flip ^ 1], launches);
		if (sg.score_job >= 0)
			HIP_TRY(hipMemcpyAsync(m.dev.d_job_scores + sg.score_job, lane.d_pr[sg.flip ^ 1], 4, hipMemcpyDeviceToDevice, rs));
	}
	return WHAMD_OK;
}

// Everything after the forward pass, on `tail_stream` (default: the table's OWN stream): backtrace, downloads, events.  walked_by_group: a batched launch
// has walked this table and made its superreads with the rest of its group; ev1 was recorded in front of it.
whamd_status_t DeviceTable::Impl::submit_tail(const Problem& p, std::string& msg, hipStream_t tail_stream, bool walked_by_group) {
	Impl& m = *this;
	const hipStream_t ts = tail_stream ? tail_stream : m.stream;
	m.inflight.tail_elsewhere = ts != m.stream;
	if (ts == m.stream) m.own_stream_used = true;
	m.inflight.tail_stream = ts;
	m.inflight.tail_seq = ++Impl::SolveInFlight::tails_submitted;
	const uint32_t n = p.n_cols;
	HIP_TRY(hipGetLastError());
	if (!walked_by_group) HIP_TRY(hipEventRecord(m.ev1, ts));
	if (walked_by_group) {
	} else if (m.tp.use_chunks) {
		hipLaunchKernelGGL(backtrace_chunks, dim3(m.tp.n_orient_max * (uint32_t)m.tp.chunks.size()), dim3(256), m.tp.chunk_lds, ts, m.dev.dp, m.dev.d_units, m.dev.d_chunks,
		                   (uint32_t)m.tp.chunks.size(), (uint32_t)m.tp.units.size(), 0u, m.tp.n_orient_max, m.dev.d_path2, m.dev.d_trans2, m.dev.d_score, m.dev.d_unit_x, m.dev.d_guess, m.dev.d_sel, m.dev.d_bt_counters);
		hipLaunchKernelGGL(backtrace_chunks, dim3(1), dim3(256), m.tp.chunk_lds, ts, m.dev.dp, m.dev.d_units, m.dev.d_chunks,
		                   (uint32_t)m.tp.chunks.size(), (uint32_t)m.tp.units.size(), 1u, m.tp.n_orient_max, m.dev.d_path2, m.dev.d_trans2, m.dev.d_score, m.dev.d_unit_x, m.dev.d_guess, m.dev.d_sel, m.dev.d_bt_counters);
		hipLaunchKernelGGL(backtrace_gather, dim3((uint32_t)m.tp.units.size()), dim3(64), 0, ts, m.dev.d_units, (uint32_t)m.tp.units.size(), n, m.dev.d_path2, m.dev.d_trans2, m.dev.d_sel,
		                   m.dev.d_path_index, m.dev.d_path_trans);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_chunks, dim3(m.tp.n_orient_max * (uint32_t)m.tp.chunks.size()), dim3(256), m.tp.chunk_lds, ts, false, LaunchFacts());
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_chunks, dim3(1), dim3(256), m.tp.chunk_lds, ts, false, LaunchFacts());
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_gather, dim3((uint32_t)m.tp.units.size()), dim3(64), 0, ts, false, LaunchFacts());
	} else if (!m.tp.windowed) {   // (windowed: every window was walked right after its steps)
		hipLaunchKernelGGL(backtrace_kernel, dim3((uint32_t)m.tp.jobs.size()), dim3(1024), m.tp.bt_lds, ts, m.dev.dp, m.dev.d_units, m.dev.d_btjobs,
		                   m.dev.d_path_index, m.dev.d_path_trans, m.dev.d_score);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_kernel, dim3((uint32_t)m.tp.jobs.size()), dim3(1024), m.tp.bt_lds, ts, false, LaunchFacts());
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(m.ev2, ts));
	if (m.tp.device_superreads && !walked_by_group) {
		hipLaunchKernelGGL(superreads_single, dim3((n + 255u) / 256u), dim3(256), 0, ts, m.dev.super_args);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)superreads_single, dim3((n + 255u) / 256u), dim3(256), 0, ts, false, LaunchFacts());
		HIP_TRY(hipGetLastError());
	}
	// ONE download per table (the device block has the pinned buffer's layout, upload()); pinned: a copy into pageable memory would block this call until the stream drains
	HIP_TRY(hipMemcpyAsync(m.dev.h_pinned, m.dev.d_path_index, (m.tp.super_off + (m.tp.device_superreads ? m.tp.super_words : 0)) * sizeof(uint32_t), hipMemcpyDeviceToHost, ts));
	HIP_TRY(hipEventRecord(m.ev3, ts));
	return WHAMD_OK;
}

whamd_status_t DeviceTable::enqueue_some_unguarded(const Problem& p, Solution& s, uint64_t budget, bool& done, std::string& msg) {
	Impl& m = *impl_;
	const uint32_t n = p.n_cols;
	done = false;
	if (n) HIP_TRY(hipSetDevice(m.device));
	if (!m.inflight.enqueue_open) {
		m.inflight.enqueue_open = true;
		m.inflight.run_stream = m.stream;
		m.inflight.group_tables = 1;
		// behind the preview: the table alone on its own stream, every launched step agreed with the finished schedule, and its launches chosen as this solve's are
		const bool behind_preview = n && m.preview.pending && m.preview.agreed > 0 && m.preview.agreed == m.preview.launched && !m.opt.side_by_side;
		const whamd_status_t st = m.begin_solve(p, s, msg, behind_preview);
		if (st != WHAMD_OK) return st;
		if (n == 0) {  // src/pedigreedptable.cpp:88-92
			s.optimal_score = 0;
			m.inflight.enqueue_open = false;
			done = true;
			return WHAMD_OK;
		}
	}
	uint64_t launches = 0;
	while (m.inflight.next_super < m.tp.schedule.size() && launches < budget) {
		const whamd_status_t st = m.submit_super_step(p, m.tp.schedule[m.inflight.next_super++], launches, msg);
		if (st != WHAMD_OK) return st;
	}
	m.inflight.launches += launches;
	if (m.inflight.next_super < m.tp.schedule.size()) return WHAMD_OK;
	const whamd_status_t st = m.submit_tail(p, msg);
	if (st != WHAMD_OK) return st;
	m.inflight.enqueue_open = false;
	done = true;
	return WHAMD_OK;
}

// ================================================================================================ solve: a group
// Several independent tables as ONE sequence of launches (whamd_dptable_enqueue_many): super-step k of the group = step k of every
// member that still has one; the runs of all members go out as one slot_group / pedslot_group launch per kernel variant
// (blockIdx.y = member), on the stream of the group's first table; per-column steps follow as launches of their own.  When the
// forward pass is submitted every member's own stream waits for it (one event) and runs that table's backtrace and downloads --
// those overlap across the members -- so whamd_dptable_wait works per table as before.
bool DeviceTable::group_eligible(const Problem& p) const {
	const Impl& m = *impl_;
	if (p.n_cols == 0 || !m.tp.use_slots || m.tp.windowed || m.inflight.enqueue_open || m.dev.dp.dbg || (m.dev.dp.dbg_flags && m.tp.splan.ped)) return false;
	if (!m.tp.splan.ped && m.tp.slot_lr_used != 2 && m.tp.slot_lr_used != 3) return false;   // (group kernels: four or eight cells per thread)
	return debug_env("WHAMD_NO_GROUP") == nullptr;
}

int DeviceTable::device_index() const { return impl_->device; }
uint32_t DeviceTable::widest_launch() const { return impl_->tp.max_grid_x; }

// One group solve in the making: what the steps of enqueue_group share.  A launch takes SLOT_GROUP_MAX runs (BT_GROUP_MAX tables for the
// walk): a larger group flushes a variant's batch in the middle of a super-step and cuts the batched backtrace, and every member counts the launches it has a run in.
// (Cutting a group into parts on streams of their own was measured and gave nothing: profiles/r04/experiments_not_kept.md, ROUND4.md row 1b)
struct DeviceTable::Impl::GroupSubmission {
	struct Batch { SlotGroupArgs args; uint32_t grid_x = 0, threads = 0; size_t lds = 0; };   // the runs collected for the next launch of one variant
	DeviceTable* const* tables;
	const Problem* const* problems;
	Solution* const* solutions;
	const size_t n;                          // members
	Impl& lead;                              // the first member: the forward pass of all of them goes onto its stream
	std::string& msg;
	bool tight = false;                      // more than three workgroups per CU: the variants held to 80 SGPRs (four workgroups per CU)
	size_t max_steps = 0;                    // super-steps of the longest member
	std::vector<Batch> batches;              // [variant]
	std::vector<uint8_t> counted;            // [member][variant]: the member has a run in the variant's open batch
	std::vector<uint64_t> table_launches;    // [member]: forward launches it had a run in, and its own per-column steps (whamd_solve_stats::forward_launches)
	std::vector<uint8_t> walked;             // [member]: a batched backtrace launch walked it
#ifdef WHAMD_DEBUG_BUILD
	const bool touch_fat = debug_env("WHAMD_GROUP_TOUCH_ENTRIES") != nullptr;
	volatile uint64_t fat_sink = 0;
#endif

	GroupSubmission(DeviceTable* const* t, const Problem* const* p, Solution* const* s, size_t n_tables, std::string& m)
		: tables(t), problems(p), solutions(s), n(n_tables), lead(*t[0]->impl_), msg(m), batches(GROUP_VARIANTS), counted(n_tables * GROUP_VARIANTS, 0),
		  table_launches(n_tables, 0), walked(n_tables, 0) {}
	Impl& member(size_t i) const { return *tables[i]->impl_; }

	// Drops what has been submitted: every member can be solved again from the start.
	whamd_status_t abort(whamd_status_t st) {
		(void)hipStreamSynchronize(lead.stream);
		(void)hipGetLastError();
		for (size_t i = 0; i < n; ++i) {
			(void)hipStreamSynchronize(member(i).stream);
			member(i).inflight.rewind(member(i).stream);
		}
		return st;
	}
	whamd_status_t fail(const char* what) { msg = what; return abort(WHAMD_ERR_DEVICE); }

	// Every member's solve opens on the lead's stream.
	whamd_status_t open_members() {
		uint64_t width = 0;
		for (size_t i = 0; i < n; ++i) width += member(i).tp.max_grid_x;
		tight = width > 768 && !debug_env("WHAMD_GROUP_LOOSE");
		for (size_t i = 0; i < n; ++i) {
			Impl& m = member(i);
			m.inflight.enqueue_open = true;
			m.inflight.run_stream = lead.stream;
			m.inflight.group_tables = (uint32_t)n;
			const whamd_status_t st = m.begin_solve(*problems[i], *solutions[i], msg);
			if (st != WHAMD_OK) return abort(st);
			max_steps = std::max(max_steps, m.tp.schedule.size());
		}
		return WHAMD_OK;
	}

	// The runs of super-step k of every member that has one, each into the batch of its variant.
	void add_super_step(size_t k) {
		std::fill(counted.begin(), counted.end(), 0);
		for (size_t i = 0; i < n; ++i) {
			Impl& m = member(i);
			if (k >= m.tp.step_brief.size()) continue;
			const StepBrief& sb = m.tp.step_brief[k];   // (a few bytes per table and super-step: StepBrief)
#ifdef WHAMD_DEBUG_BUILD
			if (touch_fat) {   // (A/B of the round-5 change: read what the loop used to read -- the super-step and its 320-byte entries)
				const SuperStep& ss = m.tp.schedule[k];
				for (uint32_t q = 0; q < ss.entry_count; ++q) { const SlotBatchEntry& he = m.tp.slot_entries[ss.entry_off + q]; fat_sink += he.run.yflags + he.run.g + he.run.threads + he.ex.nf + (uint32_t)ss.lds; }
			}
#endif
			for (uint32_t q = 0; q < sb.entry_count; ++q) {
				const EntryBrief& eb = m.tp.entry_brief[sb.entry_off + q];
				const bool xrun = eb.variant.x != eb.variant.plain && !m.dev.dp.dbg_flags;   // (the X kernel: operands streamed from the tables, 16 KB of LDS)
				const GroupVariant v = xrun ? eb.variant.x : eb.variant.plain;
				Batch& b = batches[v];
				if (b.args.n == (uint32_t)SLOT_GROUP_MAX) flush(v);
				b.args.entry[b.args.n++] = m.dev.d_slot_entries + sb.entry_off + q;
				b.grid_x = std::max<uint32_t>(b.grid_x, eb.grid_x);
				b.threads = std::max<uint32_t>(b.threads, eb.threads);
				b.lds = std::max<size_t>(b.lds, xrun ? eb.lds_x : sb.lds);
				counted[i * GROUP_VARIANTS + v] = 1;
			}
		}
	}

	// The open batch of one variant goes out as one launch; every member with a run in it counts it.
	void flush(GroupVariant v) {
		Batch& b = batches[v];
		if (!b.args.n) return;
		// a table's workgroups on ONE XCD (slot_group_who): the table is the fast grid dimension, padded to a multiple of eight -- where that spreads the tables
		// evenly over the eight XCDs (a multiple of eight of them, or so many that the remainder does not matter)
		const bool by_table = (b.args.n % 8u == 0u || b.args.n >= 40u) && !debug_env("WHAMD_GROUP_BY_WORKGROUP");
		b.args.pad = by_table ? 1u : 0u;
		const dim3 grid = by_table ? dim3((b.args.n + 7u) & ~7u, b.grid_x) : dim3(b.grid_x, b.args.n), block(b.threads);
		const GroupFn kernel = group_kernel(v, DEBUG_BUILD && lead.dev.dp.dbg_flags != 0, tight);
		hipLaunchKernelGGL(kernel, grid, block, b.lds, lead.stream, b.args);
#ifdef WHAMD_DEBUG_BUILD
		const uint32_t members = b.args.n;
		const size_t lds = b.lds;
#endif
		b.args.n = 0;
		b.grid_x = b.threads = 0;
		b.lds = 0;
#ifdef WHAMD_DEBUG_BUILD
		LaunchFacts facts;
		facts.variant = (int32_t)v; facts.tight = tight; facts.stamps = lead.dev.dp.dbg_flags != 0; facts.entries = (int32_t)members;
#endif
		for (size_t j = 0; j < n; ++j)
			if (counted[j * GROUP_VARIANTS + v]) {
				table_launches[j] += 1;
				counted[j * GROUP_VARIANTS + v] = 0;
				WHAMD_NOTE(member(j), WHAMD_LAUNCH_GROUP, (const void*)kernel, grid, block, lds, lead.stream, true, facts);
			}
	}

	// The per-column steps of super-step k, member by member.
	whamd_status_t submit_singles(size_t k) {
		for (size_t i = 0; i < n; ++i) {
			Impl& m = member(i);
			if (k >= m.tp.step_brief.size() || !m.tp.step_brief[k].has_singles) continue;
			const whamd_status_t st = m.submit_singles(*problems[i], m.tp.schedule[k], table_launches[i], msg);
			if (st != WHAMD_OK) return abort(st);
		}
		return WHAMD_OK;
	}

	// "The forward pass of every member is submitted up to here."
	whamd_status_t mark_forward_end() {
		if (hipGetLastError() != hipSuccess) return fail("group launch failed");
		if (hipEventRecord(lead.ev_group, lead.stream) != hipSuccess) return fail("hipEventRecord failed");
		return WHAMD_OK;
	}

	// The chunked backtrace of the members that have one as ONE launch per mode + one gather (blockIdx.y = member), on the lead's stream.
	whamd_status_t walk_back() {
		if (debug_env("WHAMD_TAIL_OWN_STREAM") || debug_env("WHAMD_NO_GROUP_BACKTRACE")) return WHAMD_OK;
		std::vector<size_t> batch;
		for (size_t i = 0; i < n; ++i) {
			const Impl& m = member(i);
			if (!m.tp.use_chunks || m.tp.windowed || !m.dev.d_bt_entry) continue;
			batch.push_back(i);
			if (batch.size() == (size_t)BT_GROUP_MAX && !walk_batch(batch)) return fail("group backtrace launch failed");
		}
		if (!walk_batch(batch)) return fail("group backtrace launch failed");
		return WHAMD_OK;
	}

	// (a batch of one is left to the member's own tail)
	bool walk_batch(std::vector<size_t>& batch) {
		if (batch.size() < 2) { batch.clear(); return true; }
		BtGroupArgs args{};
		uint32_t gx = 1, gu = 1;
		size_t lds = 0;
		for (size_t i : batch) {
			Impl& m = member(i);
			args.entry[args.n++] = m.dev.d_bt_entry;
			gx = std::max(gx, m.tp.n_orient_max * (uint32_t)m.tp.chunks.size());
			gu = std::max(gu, (uint32_t)m.tp.units.size());
			lds = std::max(lds, m.tp.chunk_lds);
			if (hipEventRecord(m.ev1, lead.stream) != hipSuccess) return false;
		}
		hipLaunchKernelGGL(backtrace_chunks_group, dim3(gx, args.n), dim3(256), lds, lead.stream, args, 0u);
		hipLaunchKernelGGL(backtrace_chunks_group, dim3(1, args.n), dim3(256), lds, lead.stream, args, 1u);
		hipLaunchKernelGGL(backtrace_gather_group, dim3(gu, args.n), dim3(64), 0, lead.stream, args);
		uint32_t gs = 0;   // (the superreads of the members the device makes them for, behind the gather)
		for (size_t i : batch) if (member(i).tp.device_superreads) gs = std::max(gs, (problems[i]->n_cols + 255u) / 256u);
		if (gs) hipLaunchKernelGGL(superreads_group, dim3(gs, args.n), dim3(256), 0, lead.stream, args);
		if (hipGetLastError() != hipSuccess) return false;
#ifdef WHAMD_DEBUG_BUILD
		for (size_t i : batch) {   // (every member the launches walk; superreads_group in those it makes superreads for)
			Impl& m = member(i);
			LaunchFacts facts;
			facts.entries = (int32_t)args.n;
			m.note(WHAMD_LAUNCH_GROUP_WALK, (const void*)backtrace_chunks_group, dim3(gx, args.n), dim3(256), lds, lead.stream, false, facts);
			m.note(WHAMD_LAUNCH_GROUP_WALK, (const void*)backtrace_chunks_group, dim3(1, args.n), dim3(256), lds, lead.stream, false, facts);
			m.note(WHAMD_LAUNCH_GROUP_WALK, (const void*)backtrace_gather_group, dim3(gu, args.n), dim3(64), 0, lead.stream, false, facts);
			if (gs && m.tp.device_superreads) m.note(WHAMD_LAUNCH_GROUP_WALK, (const void*)superreads_group, dim3(gs, args.n), dim3(256), 0, lead.stream, false, facts);
		}
#endif
		for (size_t i : batch) walked[i] = 1;
		batch.clear();
		return true;
	}

	// The tail (backtrace, downloads) of every member goes onto the LEAD's stream, behind the group's last launch in the same hardware queue.  On the members'
	// own streams -- each waiting for the lead's event -- a 96-table step was bimodal: 67 ms or 95 ms, the device's forward pass 39 ms either way
	// (hardware queues that hold only a barrier are rescheduled late; more queues, GPU_MAX_HW_QUEUES=16, made every step 180 ms).  WHAMD_TAIL_OWN_STREAM=1
	// (debug library) restores the old placement.
	// ... except a member that walks back through the SEQUENTIAL kernel (several jobs, or too few units for chunks): milliseconds of one workgroup per table --
	// those run side by side on the members' own streams, behind the group's event, instead of one after the other on the lead's.
	whamd_status_t submit_tails() {
		for (size_t i = 0; i < n; ++i) {
			Impl& m = member(i);
			m.inflight.launches = table_launches[i];
			const bool own = debug_env("WHAMD_TAIL_OWN_STREAM") != nullptr || (!walked[i] && !m.tp.use_chunks && !m.tp.windowed && m.stream != lead.stream);
			if (own) m.own_stream_used = true;
			if (own && m.stream != lead.stream && hipStreamWaitEvent(m.stream, lead.ev_group, 0) != hipSuccess) return fail("hipStreamWaitEvent failed");
			const whamd_status_t st = m.submit_tail(*problems[i], msg, own ? nullptr : lead.stream, walked[i] != 0);
			if (st != WHAMD_OK) return abort(st);
			m.inflight.rewind(m.stream);
		}
		return WHAMD_OK;
	}
};

whamd_status_t DeviceTable::enqueue_group(DeviceTable* const* tables, const Problem* const* problems, Solution* const* solutions, size_t n_tables, std::string& msg) {
	if (n_tables == 0) return WHAMD_OK;
	HIP_TRY(hipSetDevice(tables[0]->impl_->device));
	Impl::GroupSubmission g(tables, problems, solutions, n_tables, msg);
	whamd_status_t st = g.open_members();
	if (st != WHAMD_OK) return st;
	const auto t_submit0 = std::chrono::steady_clock::now();
	for (size_t k = 0; k < g.max_steps; ++k) {
		g.add_super_step(k);
		for (int v = 0; v < GROUP_VARIANTS; ++v) g.flush((GroupVariant)v);   // (ascending: the order of the launches inside a super-step)
		if ((st = g.submit_singles(k)) != WHAMD_OK) return st;
	}
	if (getenv("WHAMD_DEBUG_TIMING"))
		fprintf(stderr, "[whamd timing] group of %zu tables in 1 part(s): %zu super-steps submitted in %.2f ms (host)\n", n_tables, g.max_steps,
		        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_submit0).count());
	if ((st = g.mark_forward_end()) != WHAMD_OK) return st;
	if ((st = g.walk_back()) != WHAMD_OK) return st;
	return g.submit_tails();
}

// Tables in flight whose tails share a stream (a group: every member's tail is on the lead's stream, in order) finish in that order: ONE wait for the last of each
// stream, on the calling thread, and every table's own wait() returns at once.  (32 threads inside hipEventSynchronize at the same time woke up over 6 - 13 ms
// after the device had recorded the last event -- the events of one table 1.8 ms apart; one waiter wakes once.)
void DeviceTable::wait_last_of_each_stream(DeviceTable* const* tables, size_t n_tables) {
	std::vector<std::pair<hipStream_t, const Impl*>> last;
	for (size_t i = 0; i < n_tables; ++i) {
		const Impl& m = *tables[i]->impl_;
		if (!m.inflight.tail_elsewhere || !m.ev3) continue;
		bool found = false;
		for (auto& e : last) {
			if (e.first != m.inflight.tail_stream || e.second->device != m.device) continue;
			found = true;
			if (m.inflight.tail_seq > e.second->inflight.tail_seq) e.second = &m;
		}
		if (!found) last.emplace_back(m.inflight.tail_stream, &m);
	}
	for (const auto& e : last) {
		if (hipSetDevice(e.second->device) != hipSuccess || hipEventSynchronize(e.second->ev3) != hipSuccess) (void)hipGetLastError();   // (the table's own wait() reports it)
	}
}

// The event timings of the last collected solve (forward, backtrace, first to last event), filled into `st` once; a no-op when they have been
// read already or when a new solve has been submitted since (the events then belong to that one).
void DeviceTable::read_timing(whamd_solve_stats& st) {
	Impl& m = *impl_;
	if (!m.inflight.timing_pending) return;
	m.inflight.timing_pending = false;
	if (hipSetDevice(m.device) != hipSuccess) return;
	float f01 = 0, f12 = 0, f03 = 0;
	if (hipEventElapsedTime(&f01, m.ev0, m.ev1) != hipSuccess || hipEventElapsedTime(&f12, m.ev1, m.ev2) != hipSuccess || hipEventElapsedTime(&f03, m.ev0, m.ev3) != hipSuccess) {
		(void)hipGetLastError();
		return;
	}
	st.forward_ms = f01;
	st.backtrace_ms = f12;
	st.total_ms = f03;
}

// The in-kernel cycle stamps of the slot runs (WHAMD_SLOT_STAMPS, debug library): full-length runs, wave 0 of workgroup 0.
whamd_status_t DeviceTable::Impl::report_slot_stamps(std::string& msg) const {
	const Impl& m = *this;
	if (m.dev.dp.dbg_flags & 256u) return m.report_slot_wave_stamps(msg);
	std::vector<unsigned long long> d(m.tp.splan.runs.size() * 48);
	HIP_TRY(hipMemcpy(d.data(), m.dev.dp.dbg, d.size() * 8, hipMemcpyDeviceToHost));
	double a[6] = {0, 0, 0, 0, 0, 0};
	double percol[32] = {0};
	size_t cnt = 0;
	for (size_t i = 0; i < m.tp.splan.runs.size(); ++i) {
		if (m.tp.splan.runs[i].ncols != 22 || d[48 * i + 5] == 0) continue;   // full-length runs only
		for (int k = 0; k < 6; ++k) a[k] += (double)d[48 * i + k];
		for (int k = 0; k < 22; ++k) percol[k] += (double)d[48 * i + 8 + k];
		++cnt;
	}
	if (cnt) fprintf(stderr, "[whamd slot stamps] %zu runs, wave 0 of workgroup 0, shader cycles: prologue issue %.0f, loads landed %.0f, column loop %.0f (%.1f per column, %.1f columns), exit %.0f\n",
	                 cnt, a[0] / cnt, a[1] / cnt, a[2] / cnt, a[2] / std::max(a[4], 1.0), a[4] / cnt, a[3] / cnt);
	if (cnt) {
		fprintf(stderr, "[whamd slot stamps] cycles after the loop start at which column c had its cost added:");
		for (int k = 0; k < 22; ++k) fprintf(stderr, " %.0f", percol[k] / cnt);
		fprintf(stderr, "\n");
	}
	return WHAMD_OK;
}

// The per-wave stamps of the X runs (WHAMD_SLOT_STAMPS=2, debug library): full-length runs of eight waves, workgroups 0, 3 and 6 (three XCDs).  Every stamp
// as cycles after the EARLIEST wave start of its workgroup, averaged per wave; its spread over the eight waves; which wave is last; and the entering
// cells' own latency by the order in which the waves issued their request (a queue in front of a late request shows as latency growing with the rank).
whamd_status_t DeviceTable::Impl::report_slot_wave_stamps(std::string& msg) const {
	const Impl& m = *this;
	constexpr int NW = 8, NS = 9;
	static const char* const names[NS] = {"wave start", "entering cells requested", "last prologue request", "entering cells landed", "all landed, loop starts",
	                                      "scalar tables landed too", "first wave-slot ending reached", "first wave-slot ending left", "loop end"};
	static const int word[NS] = {0, 1, 2, 3, 7, 8, 4, 5, 6};   // (the order of slot_runx_exit's words -> the order of the events; 8: the high half of word 7)
	auto stamp = [](const unsigned long long* wave_words, int k) { return k == 8 ? wave_words[7] >> 32 : (k == 7 ? wave_words[7] & 0xFFFFFFFFull : wave_words[k]); };
	const size_t nruns = m.tp.splan.runs.size(), per_run = (size_t)SLOT_WAVE_STAMP_WGS * SLOT_WAVE_STAMP_WORDS;
	std::vector<unsigned long long> d(nruns * per_run);
	HIP_TRY(hipMemcpy(d.data(), m.dev.dp.dbg + m.dev.dp.dbg_wg_off + SLOT_WAVE_STAMP_OFF, d.size() * 8, hipMemcpyDeviceToHost));
	for (uint32_t sel = 0; sel < SLOT_WAVE_STAMP_WGS; ++sel) {
		double mean[NS][NW] = {}, spread[NS] = {}, spread_max[NS] = {}, lat_rank[NW] = {}, req_rank[NW] = {}, land_rank[NW] = {};
		size_t last[2][NW] = {}, cnt = 0;
		for (size_t i = 0; i < nruns; ++i) {
			const unsigned long long* r = d.data() + i * per_run + sel * SLOT_WAVE_STAMP_WORDS;
			bool full = m.tp.splan.runs[i].ncols == 22;
			for (int v = 0; v < NW; ++v) full = full && r[v * 8 + 6] != 0 && r[v * 8 + 4] != 0;   // (a run of eight waves with a wave-slot ending)
			if (!full) continue;
			unsigned long long s0 = r[0];
			for (int v = 1; v < NW; ++v) s0 = std::min(s0, r[v * 8]);
			double at[NS][NW];
			for (int k = 0; k < NS; ++k) {
				double lo = 1e300, hi = 0;
				int hi_at = 0;
				for (int v = 0; v < NW; ++v) {
					at[k][v] = (double)(r[v * 8] - s0) + (k ? (double)stamp(r + v * 8, word[k]) : 0.0);
					mean[k][v] += at[k][v];
					lo = std::min(lo, at[k][v]);
					if (at[k][v] > hi) { hi = at[k][v]; hi_at = v; }
				}
				spread[k] += hi - lo;
				spread_max[k] = std::max(spread_max[k], hi - lo);
				if (k == 3) last[0][hi_at]++;
				if (k == 6) last[1][hi_at]++;
			}
			int order[NW];
			for (int v = 0; v < NW; ++v) order[v] = v;
			std::sort(order, order + NW, [&](int a, int b) { return at[1][a] < at[1][b]; });
			for (int q = 0; q < NW; ++q) { req_rank[q] += at[1][order[q]]; land_rank[q] += at[3][order[q]]; lat_rank[q] += at[3][order[q]] - at[1][order[q]]; }
			++cnt;
		}
		if (!cnt) continue;
		fprintf(stderr, "[whamd slot wave stamps] workgroup %u: %zu runs of 22 columns, shader cycles after the workgroup's earliest wave start; waves 0 .. 7 | mean spread, largest spread\n", 3 * sel, cnt);
		for (int k = 0; k < NS; ++k) {
			fprintf(stderr, "[whamd slot wave stamps]   %-31s", names[k]);
			for (int v = 0; v < NW; ++v) fprintf(stderr, " %6.0f", mean[k][v] / cnt);
			fprintf(stderr, " | %6.0f %6.0f\n", spread[k] / cnt, spread_max[k]);
		}
		for (int h = 0; h < 2; ++h) {
			fprintf(stderr, "[whamd slot wave stamps]   runs in which wave v is the last %-14s", h ? "at the ending:" : "to have cells:");
			for (int v = 0; v < NW; ++v) fprintf(stderr, " %6zu", last[h][v]);
			fprintf(stderr, "\n");
		}
		fprintf(stderr, "[whamd slot wave stamps]   by the order of the waves' requests -- requested:     ");
		for (int q = 0; q < NW; ++q) fprintf(stderr, " %6.0f", req_rank[q] / cnt);
		fprintf(stderr, "\n[whamd slot wave stamps]                                           landed:        ");
		for (int q = 0; q < NW; ++q) fprintf(stderr, " %6.0f", land_rank[q] / cnt);
		fprintf(stderr, "\n[whamd slot wave stamps]                                           latency:       ");
		for (int q = 0; q < NW; ++q) fprintf(stderr, " %6.0f", lat_rank[q] / cnt);
		fprintf(stderr, "\n");
	}
	return WHAMD_OK;
}

// The in-kernel cycle stamps of the LDS-resident runs (WHAMD_DEBUG_STAMPS, debug library), with the backtrace's and four runs' workgroup by workgroup.
whamd_status_t DeviceTable::Impl::report_resident_stamps(std::string& msg) const {
	const Impl& m = *this;
	std::vector<unsigned long long> d(m.tp.plan.segments.size() * 8);
	HIP_TRY(hipMemcpy(d.data(), m.dev.dp.dbg, d.size() * 8, hipMemcpyDeviceToHost));
	unsigned long long a = 0, b = 0, c2 = 0, cols = 0, p1 = 0, p2 = 0, p3 = 0, ns = 0;
	for (size_t i = 0; i < m.tp.plan.segments.size(); ++i) { a += d[8 * i]; b += d[8 * i + 1]; c2 += d[8 * i + 2]; cols += d[8 * i + 3]; p1 += d[8 * i + 4]; p2 += d[8 * i + 5]; p3 += d[8 * i + 6]; ns += d[8 * i + 7]; }
	if (!m.tp.plan.ped_columns.empty() || (m.dev.dp.dbg_flags & 4u))
		fprintf(stderr, "[whamd timing] run prologue (wave 0 of workgroup 0), cycles after the first instruction: kernel arguments usable %.0f, first loaded data %.0f, everything staged %.0f\n",
		        (double)p2 / std::max<unsigned long long>(ns, 1), (double)p3 / std::max<unsigned long long>(ns, 1), (double)p1 / std::max<unsigned long long>(ns, 1));
	else
	fprintf(stderr, "[whamd timing] per barrier step (wave 0 of workgroup 0, %.1f steps per run): hot words %.0f, evaluate %.0f, barrier %.0f cycles\n",
	        (double)ns / m.tp.plan.segments.size(), (double)p1 / std::max<unsigned long long>(ns, 1), (double)p2 / std::max<unsigned long long>(ns, 1), (double)p3 / std::max<unsigned long long>(ns, 1));
	{
		unsigned long long b3[6] = {0, 0, 0, 0, 0, 0};
		HIP_TRY(hipMemcpy(b3, m.dev.dp.dbg + m.dev.dp.dbg_wg_off + 4 * 512 * 2, sizeof b3, hipMemcpyDeviceToHost));
		if (b3[2]) fprintf(stderr, "[whamd timing] backtrace per run: record load + prefetch %.0f cycles, walk + hand-over %.0f cycles (%llu runs); of the latter: local exit index %.0f, chain %.0f, logical indices + stores %.0f\n",
		                   (double)b3[0] / b3[2], (double)b3[1] / b3[2], b3[2], (double)b3[3] / b3[2], (double)b3[4] / b3[2], (double)b3[5] / b3[2]);
	}
	if (m.tp.plan.segments.size() > 104) {
		std::vector<unsigned long long> wg(4 * 512 * 2);
		HIP_TRY(hipMemcpy(wg.data(), m.dev.dp.dbg + m.dev.dp.dbg_wg_off, wg.size() * 8, hipMemcpyDeviceToHost));
		unsigned long long prev_end = 0;
		for (int sgi = 0; sgi < 4; ++sgi) {
			const uint32_t G = 1u << m.tp.plan.segments[100 + sgi].g;
			unsigned long long s0 = ~0ull, s1 = 0, e0 = ~0ull, e1 = 0;
			for (uint32_t ww = 0; ww < G; ++ww) {
				const unsigned long long a2 = wg[((size_t)sgi * 512 + ww) * 2], b2 = wg[((size_t)sgi * 512 + ww) * 2 + 1];
				s0 = std::min(s0, a2); s1 = std::max(s1, a2); e0 = std::min(e0, b2); e1 = std::max(e1, b2);
			}
			fprintf(stderr, "[whamd timing] run %d (%u workgroups): first start +%.2f us after previous run's last end; starts spread %.2f us; first end %.2f us, last end %.2f us after first start\n",
			        100 + sgi, G, prev_end ? (double)(s0 - prev_end) / 100.0 : 0.0, (double)(s1 - s0) / 100.0, (double)(e0 - s0) / 100.0, (double)(e1 - s0) / 100.0);
			prev_end = e1;
		}
	}
	float f01 = 0;
	(void)hipEventElapsedTime(&f01, m.ev0, m.ev1);
	fprintf(stderr, "[whamd timing] segments %zu cols %llu | cycles/segment: prologue %.0f columns %.0f (%.0f per column) store %.0f | fwd %.3f ms, %.2f us per segment\n",
	        m.tp.plan.segments.size(), cols, (double)a / m.tp.plan.segments.size(), (double)b / m.tp.plan.segments.size(),
	        (double)b / std::max<unsigned long long>(cols, 1), (double)c2 / m.tp.plan.segments.size(), f01, f01 * 1e3 / m.tp.plan.segments.size());
	return WHAMD_OK;
}

// Synchronise, copy out, fill the stats.
whamd_status_t DeviceTable::wait(const Problem& p, Solution& s, whamd_solve_stats& st, std::string& msg) {
	Impl& m = *impl_;
	if (p.n_cols == 0) return WHAMD_OK;
	HIP_TRY(hipSetDevice(m.device));
	const uint64_t launches = m.inflight.launches;
	if (m.inflight.tail_elsewhere) HIP_TRY(hipEventSynchronize(m.ev3));   // (the last thing submit_tail recorded, on the stream the tail went to)
	else { HIP_TRY(hipStreamSynchronize(m.stream)); m.own_stream_used = false; }
	m.upload_pending = false;   // (the solve ran behind ev_upload: the uploads are there)
	m.give_preview_block();     // (the preview ran in front of this solve, or was waited for when the solve began on another stream)
	const uint32_t n = p.n_cols;
	std::memcpy(s.path_index.data(), m.dev.h_pinned, (size_t)n * 4);
	std::memcpy(s.path_trans.data(), m.dev.h_pinned + n, (size_t)n * 4);
	s.optimal_score = m.dev.h_pinned[2 * (size_t)n];
	if (m.tp.device_superreads) {
		const uint32_t* q = m.dev.h_pinned + m.tp.super_off;
		const uint8_t* h = (const uint8_t*)(q + n);
		if (std::memchr(h, SUPERREAD_CONFLICT, (size_t)2 * n) == nullptr) {   // (a conflict: the host's loop runs and reports it, finish_solution)
			s.quality.resize(n);
			s.allele0.resize(n);
			s.allele1.resize(n);
			std::memcpy(s.quality.data(), q, (size_t)n * 4);
			std::memcpy(s.allele0.data(), h, n);
			std::memcpy(s.allele1.data(), h + n, n);
			s.superreads_done = true;
		}
	}
	for (size_t j = 1; j < m.tp.jobs.size(); ++j) s.optimal_score += m.dev.h_pinned[2 * (size_t)n + j];  // connected components solved as their own jobs
	// (the event timings are read when somebody asks -- read_timing(), from whamd_dptable_get_stats: three runtime calls per table, from every
	//  waiting thread at once, are a measurable part of collecting a 96-table step and most callers never look at them)
	st.forward_ms = st.backtrace_ms = st.total_ms = 0;
	m.inflight.timing_pending = true;
	st.forward_launches = launches;
	st.group_tables = m.inflight.group_tables;
	st.bt_chunks = st.bt_missed = st.bt_rewalked = 0;
	if (m.tp.use_chunks) {
		const uint32_t* c = m.dev.h_pinned + 2 * (size_t)n + m.tp.jobs.size();   // (downloaded with the path)
		st.bt_chunks = (uint32_t)m.tp.chunks.size();
		st.bt_missed = c[0];
		st.bt_rewalked = c[1];
		if (debug_env("WHAMD_BT_STATS")) fprintf(stderr, "[whamd backtrace] %zu chunks, %u guesses missed (%u of them only in the transmission value), %u units walked again (of %zu)\n", m.tp.chunks.size(), c[0], c[2], c[1], m.tp.units.size());
	}
	whamd_status_t reported = m.dev.dp.dbg && m.tp.use_slots ? m.report_slot_stamps(msg) : WHAMD_OK;   // (the debug library's in-kernel cycle stamps)
	if (reported == WHAMD_OK && m.dev.dp.dbg && !m.tp.plan.segments.empty()) reported = m.report_resident_stamps(msg);
	return reported;
}

// ================================================================================================ the launch ledger (debug library)
#ifdef WHAMD_DEBUG_BUILD
namespace {

// The registry of the launch ledger: EVERY kernel a solve can launch, under the spelling of its instantiation.  A table of its own -- the *_kernel functions
// do not feed it, so that a test can hold what they return against it -- and at the END of the file, behind every launch, so that it is nowhere the first to
// name a kernel (the code object keeps its order: opt_in_large_lds).  A new instantiation is added HERE as well, and tests/test_gpu_kernel_choice.py must reach
// it.  debug_only: cycle stamps, timing switches, pedigree X runs.
template <int T, int NIND>
const void* column_pair(bool keys) {
	FusedFn ff;
	KeysFn kf;
	pick<T, NIND>(ff, kf);
	return keys ? reinterpret_cast<const void*>(kf) : reinterpret_cast<const void*>(ff);
}

const std::vector<whamd_debug_kernel>& solve_kernels() {
#define K(...) {reinterpret_cast<const void*>((__VA_ARGS__)), #__VA_ARGS__, 0, 0}
#define D(...) {reinterpret_cast<const void*>((__VA_ARGS__)), #__VA_ARGS__, 0, 1}
// (the per-column kernels are named by pick<T, NIND> alone, first in the code object: spelled here they would be named before pick is instantiated and move)
#define WHAMD_COLUMN(T, NIND) {column_pair<T, NIND>(false), "column_step_fused<" #T ", " #NIND ">", 0, 0}, {column_pair<T, NIND>(true), "column_step_keys<" #T ", " #NIND ">", 0, 0}
#define WHAMD_PSLOT(TB, NF) K(pedslot_run<TB, NF, true, true>), K(pedslot_run<TB, NF, true, false>), K(pedslot_run<TB, NF, false, true>), K(pedslot_run<TB, NF, false, false>)
#define WHAMD_PSLOTX(TB, NF) D(pedslot_runx<TB, NF, 16, true>), D(pedslot_runx<TB, NF, 16, false>), D(pedslot_runx<TB, NF, 32, true>), D(pedslot_runx<TB, NF, 32, false>)
#define WHAMD_RUNX(XC) K(slot_runx<2, XC, false, true>), K(slot_runx<2, XC, false, false>)
#define WHAMD_RUN(LR, YF) K(slot_run<LR, false, true, YF>), K(slot_run<LR, false, false, YF>), D(slot_run<LR, true, true, YF>), D(slot_run<LR, true, false, YF>)
	static const std::vector<whamd_debug_kernel> table = [] {
		std::vector<whamd_debug_kernel> t = {
			WHAMD_COLUMN(1, 1), WHAMD_COLUMN(1, 2), WHAMD_COLUMN(1, 3), WHAMD_COLUMN(1, 4), WHAMD_COLUMN(1, 5), WHAMD_COLUMN(1, 6),
			WHAMD_COLUMN(4, 3), WHAMD_COLUMN(4, 4), WHAMD_COLUMN(4, 5), WHAMD_COLUMN(4, 6),
			WHAMD_COLUMN(16, 4), WHAMD_COLUMN(16, 5), WHAMD_COLUMN(16, 6),
			K(column_step_wide), K(column_finalize),
			K(ped_tables), K(resident_tables),
			K(resident_segment<false, false>), K(resident_segment<false, true>), D(resident_segment<true, true>),
			K(resident_segment_ped<false>), K(resident_segment_ped<false, true>), D(resident_segment_ped<true>),
			K(resident_batch<false>), K(resident_batch<true>),
			WHAMD_RUN(1, false), WHAMD_RUN(2, false), WHAMD_RUN(2, true), WHAMD_RUN(3, false), WHAMD_RUN(3, true),
			WHAMD_RUNX(0), WHAMD_RUNX(8), WHAMD_RUNX(16), WHAMD_RUNX(24), WHAMD_RUNX(32),
			D(slot_runx<2, 24, true, true>), D(slot_runx<2, 24, true, false>), D(slot_runx<2, 32, true, true>), D(slot_runx<2, 32, true, false>),
			K(slot_batch<1>), K(slot_batch<2>), K(slot_batch<3>),
			WHAMD_PSLOT(2, 2), WHAMD_PSLOT(2, 4), WHAMD_PSLOT(4, 2), WHAMD_PSLOT(4, 4), WHAMD_PSLOT(2, 16), WHAMD_PSLOT(2, PSLOT_FACT), WHAMD_PSLOT(4, PSLOT_FACT4),
			WHAMD_PSLOTX(2, 2), WHAMD_PSLOTX(2, 4), WHAMD_PSLOTX(4, 2), WHAMD_PSLOTX(4, 4), WHAMD_PSLOTX(2, 16), WHAMD_PSLOTX(2, PSLOT_FACT),
			K(slot_group<2, false, false>), K(slot_group<2, false, true>), K(slot_group<3, false, false>), K(slot_group<3, false, true>), D(slot_group<2, true, false>),
			K(slot_groupx<2, false>), K(slot_groupx<3, false>),
			K(pedslot_group<2, 2>), K(pedslot_group<2, 4>), K(pedslot_group<4, 2>), K(pedslot_group<4, 4>), K(pedslot_group<2, 16>),
			K(pedslot_group<2, PSLOT_FACT>), K(pedslot_group<4, PSLOT_FACT4>),
			K(backtrace_kernel), K(backtrace_chunks), K(backtrace_gather), K(superreads_single),
			K(backtrace_chunks_group), K(backtrace_gather_group), K(superreads_group),
		};
		size_t count = 0;
		const void* const* opted = large_lds_kernels(count);   // (the very array opt_in_large_lds walks)
		for (whamd_debug_kernel& k : t) k.large_lds_opted_in = std::find(opted, opted + count, k.kernel) != opted + count;
		return t;
	}();
#undef K
#undef D
#undef WHAMD_COLUMN
#undef WHAMD_PSLOT
#undef WHAMD_PSLOTX
#undef WHAMD_RUNX
#undef WHAMD_RUN
	return table;
}

}  // namespace

size_t DeviceTable::debug_solve_kernels(whamd_debug_kernel* out, size_t capacity) {
	const std::vector<whamd_debug_kernel>& t = solve_kernels();
	for (size_t i = 0; out && i < t.size() && i < capacity; ++i) out[i] = t[i];
	return t.size();
}

// The ledger of the last solve, every kernel resolved to its registry name (nullptr: not registered).
size_t DeviceTable::debug_launches(whamd_debug_launch* out, size_t capacity) const {
	const std::vector<whamd_debug_launch>& ledger = impl_->ledger;
	for (size_t i = 0; out && i < ledger.size() && i < capacity; ++i) {
		out[i] = ledger[i];
		for (const whamd_debug_kernel& k : solve_kernels())
			if (k.kernel == ledger[i].kernel) { out[i].name = k.name; break; }
	}
	return ledger.size();
}

static const char* const* preview_why_lines() {   // [PreviewWhy]
	static const char* const why[13] = {
		"", "no preview: switched off", "no preview: not inside whamd_dptable_create", "no preview: not a single-individual table on slot runs", "no preview: a debug switch changes the launches",
		"no preview: the table shares its launches", "no preview: the create is held to a thread budget", "no preview: more than one connected component", "no preview: too few plan pieces",
		"no preview: not alone", "no preview: the table does not begin with slot runs", "no preview: too close to the table's end", "no preview: the backtrace arena does not fit one window"};
	return why;
}

// plan_preview against the phases it runs ahead of, without a device (whamd_debug_preview_plan): the plan as choose_plan makes it for a single individual, the
// preview forced with `pieces`, then table_plan.h's describe_columns, lay_out_arena, the units and cut_chunks in upload()'s order -- free HBM is taken as 1 TiB.
whamd_status_t DeviceTable::debug_preview_plan(Problem& p, uint32_t pieces, whamd_debug_preview_plan_result* out, uint64_t* rec_predicted, uint64_t* rec_laid_out,
                                               uint32_t* spec_predicted, uint32_t* spec_laid_out, size_t capacity, std::string& msg) {
	TableOptions opt;
	TablePlan tp;
	uint32_t spec_stride = 64;
	TableBuild b;
	b.n = p.n_cols;
	b.tbits = 2 * p.n_triples;
	b.ni = std::max<uint32_t>(p.n_ind, 1);
	b.free_b = (size_t)1 << 40;
	if (p.T != 1 || p.n_cols == 0) { msg = "a single-individual table expected"; return WHAMD_ERR_UNSUPPORTED; }
	tp.use_slots = plan_forward_slots(p, std::max(8, opt.slot_l), opt.symmetry, tp.splan, opt.slot_lr);
	if (!tp.use_slots) { msg = "the table is not planned on slot runs"; return WHAMD_ERR_UNSUPPORTED; }
	tp.plan = ResidentPlan();
	tp.plan.steps = tp.splan.steps;
	tp.plan.component_first_step = tp.splan.component_first_step;
	tp.plan.col_to_res.assign(p.n_cols, -1);
	opt.preview_mode = 1;
	opt.preview_pieces = pieces;
	PreviewPlan pp;
	plan_preview(p, opt, b, tp, true, true, pp);   // (forced: `alone` is not asked)
	whamd_status_t st = describe_columns(p, b, tp, msg);
	if (st == WHAMD_OK) st = lay_out_arena(p, opt, b, tp, msg);
	if (st != WHAMD_OK) return st;
	build_slot_blobs(tp, b);
	lay_out_slot_tables(tp, b, false);
	make_jobs(opt, tp);
	make_units(b, tp);
	cut_chunks(p, tp, spec_stride);
	static const char* const* why = preview_why_lines();
	*out = whamd_debug_preview_plan_result{};
	out->n_pieces = slot_plan_pieces(p.n_cols);
	out->pieces = pp.pieces;
	out->steps = pp.steps;
	out->n_steps = (uint32_t)tp.plan.steps.size();
	out->why_not = why[pp.why < PV_WHYS ? pp.why : 0];
	out->chunked_predicted = pp.chunked; out->chunked = tp.use_chunks;
	out->n_seeds_predicted = pp.n_spec; out->n_seeds = tp.n_spec;
	out->stride_predicted = pp.stride; out->stride = tp.use_chunks ? spec_stride : 64u;
	out->arena_predicted = pp.arena; out->arena_laid_out = b.bt;
	out->windowed = tp.windowed;
	out->exchange_predicted = (uint64_t)(1ull << pp.max_f) * p.T * 4; out->exchange_laid_out = b.exchange_bytes;
	for (uint32_t k = 0; k < pp.steps && k < capacity; ++k) {
		const SlotRun& run = tp.splan.runs[tp.plan.steps[k].index];
		if (rec_predicted) rec_predicted[k] = pp.rec[k];
		if (rec_laid_out) rec_laid_out[k] = ((uint64_t)run.rec_hi << 32) | run.rec_lo;
		if (spec_predicted) spec_predicted[k] = pp.spec[k];
		if (spec_laid_out) spec_laid_out[k] = run.spec_id;
	}
	return WHAMD_OK;
}

// What became of the table's preview (whamd_debug_dptable_preview).
void DeviceTable::debug_preview(whamd_debug_preview* out) const {
	static const char* const* why = preview_why_lines();
	const Impl::Preview& pv = impl_->preview;
	out->ran = pv.why == PV_RAN;
	out->continued = pv.continued;
	out->pieces = pv.pieces;
	out->launched_steps = pv.launched;
	out->agreed_steps = pv.agreed;
	out->from_hook = pv.why == PV_RAN && pv.from_hook ? 1u : 0u;
	out->why_not = why[pv.why < PV_WHYS ? pv.why : 0];
}

// One launch into the ledger: a line that agrees in everything but the count takes it, else it opens a new line.
void DeviceTable::Impl::note(uint32_t site, const void* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t on, bool forward, const LaunchFacts& facts) {
	whamd_debug_launch rec = facts;
	rec.kernel = kernel;
	rec.site = site;
	rec.grid_x = grid.x; rec.grid_y = grid.y; rec.block = block.x;
	rec.lds = (uint32_t)lds;
	rec.own_stream = on == stream ? 1u : 0u;
	rec.forward = forward ? 1u : 0u;
	rec.preview = preview.launching ? 1 : 0;
	rec.reserved = 0;
	rec.count = 0;
	rec.name = nullptr;
	for (whamd_debug_launch& have : ledger)
		if (std::memcmp(&have, &rec, offsetof(whamd_debug_launch, count)) == 0) { have.count += 1; return; }
	rec.count = 1;
	ledger.push_back(rec);
}
#endif


}  // namespace whamd
