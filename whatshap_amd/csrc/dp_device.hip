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
// This file: launch tables and the host driver (DeviceTable: upload, jobs / lanes, resumable submission, wait).
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

// The kernel variants of a group launch (DESIGN.md 6.2 has the table).  The values are the order of the launches inside a super-step.
enum GroupVariant : uint8_t { GV_SINGLE4 = 0, GV_PED_2_2, GV_PED_2_4, GV_PED_4_2, GV_PED_4_4, GV_PED_2_16, GV_SINGLE8, GV_TRIO_FACT, GV_X4, GV_X8, GV_QUARTET_FACT, GROUP_VARIANTS };
struct GroupVariantPair { GroupVariant plain, x; };   // x: the X kernel's variant where the run is eligible (else = plain)

GroupVariantPair group_variants_of(const SlotBatchEntry& he, bool ped) {
	if (ped) {
		const GroupVariant v = he.ex.nf == (uint32_t)PSLOT_FACT4 ? GV_QUARTET_FACT : he.ex.nf == (uint32_t)PSLOT_FACT ? GV_TRIO_FACT : he.ex.nf == 16 ? GV_PED_2_16
		                       : he.ex.tb == 4 ? (he.ex.nf == 4 ? GV_PED_4_4 : GV_PED_4_2) : (he.ex.nf == 4 ? GV_PED_2_4 : GV_PED_2_2);
		return {v, v};
	}
	const GroupVariant v = he.run.lr == 3 ? GV_SINGLE8 : GV_SINGLE4;
	return {v, (he.run.yflags & 8u) ? (he.run.lr == 3 ? GV_X8 : GV_X4) : v};
}

}  // namespace

// ================================================================================================ what a create shares between its phases

namespace {

// The laps of a create under WHAMD_DEBUG_TIMING: lap() prints the time since the previous lap; every lap also counts towards one of the four stages of
// the closing summary line (plan | descriptors + copies | backtrace arena | rest).  Without the switch nothing is measured.
struct CreateLaps {
	using Clock = std::chrono::steady_clock;
	const bool on = getenv("WHAMD_DEBUG_TIMING") != nullptr;
	const Clock::time_point origin = Clock::now();   // (the create's upload begins)
	Clock::time_point last = origin;
	double since_origin_ms() const { return std::chrono::duration<double, std::milli>(Clock::now() - origin).count(); }
	double stage_ms[4] = {0.0, 0.0, 0.0, 0.0};
	int stage = 0;
	double take() {
		const auto now = Clock::now();
		const double ms = std::chrono::duration<double, std::milli>(now - last).count();
		last = now;
		stage_ms[stage] += ms;
		return ms;
	}
	void lap(const char* what) {
		if (on) fprintf(stderr, "[whamd timing]   upload: %s %.2f ms\n", what, take());
	}
	void next_stage() {
		if (!on) return;
		take();
		if (stage < 3) ++stage;
	}
	void summary(double arena_gb) {
		if (!on) return;
		take();
		fprintf(stderr, "[whamd timing] upload: plan %.1f ms, descriptors + copies %.1f ms, backtrace arena (%.2f GB) %.1f ms, rest %.1f ms\n", stage_ms[0], stage_ms[1], arena_gb, stage_ms[2],
		        stage_ms[3]);
	}
};

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

	hipError_t alloc(void** dptr, size_t bytes) {
		size_t got = 0;
		hipError_t e = devpool_take(device, std::max<size_t>(bytes, 16), dptr, &got);
		if (e == hipSuccess) allocations.emplace_back(*dptr, got);
		return e;
	}
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

// What one create passes from phase to phase (DeviceTable::upload); everything that outlives the create is in Impl.
struct TableBuild {
	CreateLaps laps;
	// sizes
	uint32_t n = 0;              // columns
	uint32_t tbits = 0;          // transmission bits of an argmin
	uint32_t ni = 1;             // individuals, at least one
	size_t free_b = 0;           // free HBM when the create began, idle arenas included
	uint64_t arena_cap = 0;      // what the backtrace arena may take
	uint64_t bt = 0;             // bytes of the arena (the largest window's)
	uint32_t max_f = 0, max_keys_f = 0;   // log2 of the widest exchange column / of the widest column on the key path
	size_t exchange_bytes = 0;   // one exchange column at max_f: a d_pr buffer of a lane, a kept window boundary
	// flags
	bool force_keys = false;     // every per-column step takes the key path
	bool ped_slots = false;      // pedigree slot runs
	// host arrays whose copies may still be reading them when their phase returns, or that a later phase reads
	std::vector<uint32_t> segs;               // deposit segments of the columns outside slot runs (the column backtrace units inline them)
	RawVec<uint32_t> term_ptr32;
	std::vector<uint32_t> window_first_col;   // first column of every window after the first
	RawVec<uint32_t> slot_blob;
	std::vector<uint32_t> slot_blob_off, slot_blob_words;   // per slot run: its piece of the blob (the slot backtrace units)
	std::vector<int32_t> delta_fallback;
	// device arrays only the table kernels read
	const SlotRun* d_runs = nullptr;
	const PedSlotExtra* d_pextra = nullptr;
	const DevTerm* d_fterms = nullptr;
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

struct DeviceTable::Impl {
	int device = 0;
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
	hipEvent_t ev_group = nullptr;      // group solve: "the forward pass of every table of the group is submitted up to here"
	hipEvent_t ev_upload = nullptr;     // "everything upload() put on `stream` -- the copies, the table kernels -- is done": a solve waits for it ON THE DEVICE (begin_solve)
	std::vector<std::pair<void*, size_t>> allocations;   // (pointer, size class) of device_pool.h
	void* d_arena = nullptr;    // the backtrace arena: not in `allocations`, handed to the arena cache on release
	size_t arena_bytes = 0;
	DevColumn* d_cols = nullptr;
	uint32_t* d_pr[2] = {nullptr, nullptr};
	uint32_t* d_path_index = nullptr;
	uint32_t* d_path_trans = nullptr;
	uint32_t* d_score = nullptr;
	BtUnit* d_units = nullptr;
	std::vector<BtUnit> units;
	size_t bt_lds = 0;
	RawVec<DevColumn> cols;
	ResidentPlan plan;
	DevProblem dp{};
	FusedFn fused = nullptr;
	KeysFn keysfn = nullptr;
	bool wide = false;   // column_step_wide instead of the templated per-column kernels
	size_t key_entries = 0;
	std::string path = "auto";
	int l_pref = 11;
	bool fold = true;
	int symmetry = 1;  // single individual: compute only half of a run, the rest is its mirror image (plan_forward)
	uint64_t bt_bytes = 0;
	uint32_t max_grid_x = 1;    // widest launch of the schedule, in workgroups
	size_t h_pinned_bytes = 0;
	uint32_t* h_pinned = nullptr;  // [2 n + jobs + 3]: path index, path transmission, score of the final job, scores of the others, the chunked backtrace's three counters
	// A job is a sequence of forward steps with its own backtrace.  Job 0 ("final") is the last connected component (it
	// ends with the table's last column, whose optimum comes from the key scratch); every other job is one earlier
	// connected component: it starts from cost 0, its last column projects onto a single entry -- that value is added on
	// the host -- and its backtrace starts at entry 0.  Jobs are independent: they are spread over lanes (private
	// exchange buffers and key scratch) and the lanes advance in lockstep, one *super-step* at a time: the runs of a
	// super-step go out as ONE batched launch (resident_batch), per-column steps as launches of their own; one backtrace
	// launch at the end walks all jobs, one workgroup each.
	struct Job {
		std::vector<uint32_t> steps;  // indices into plan.steps, execution order
		uint32_t unit_off = 0, unit_count = 0;
		bool final = false;
	};
	struct Lane {
		uint32_t* d_pr[2] = {nullptr, nullptr};
		unsigned long long* d_keys = nullptr;  // atomic-min scratch of the per-column kernels
		std::vector<uint32_t> jobs;
	};
	struct Single {        // a per-column step inside a super-step
		uint32_t lane, step, flip;
		bool zero_prev;    // first step of its job: the entry it may read must hold cost 0
		int32_t score_job; // >= 0: last step of that (non-final) job: copy its single exit value aside
	};
	struct SuperStep {
		uint32_t entry_off = 0, entry_count = 0, grid_x = 0, threads = 0;
		size_t lds = 0;
		bool sym = false;  // some run of the batch takes part in the complement symmetry
		std::vector<Single> singles;
		// windowed solve: restore the kept column of boundary ck_load into this step's input before it runs; keep this
		// step's output as boundary ck_save; walk window bt_window after it
		int32_t ck_load = -1, ck_save = -1, bt_window = -1;
		uint32_t* io[2] = {nullptr, nullptr};   // input / output exchange buffer of the step (single lane)
	};
	std::vector<Job> jobs;
	std::vector<Lane> lanes;
	std::vector<SuperStep> schedule;
	// What a GROUP submission (enqueue_group) needs of a super-step and of its entries, a few bytes each: with 96 tables per launch the submitting thread read a
	// 320-byte SlotBatchEntry and a SuperStep per table and super-step out of cold memory -- 31 ms of host time for 2 276 super-steps, 13 ms with these
	// (scripts/gpu_group_submit_ab.py).  Built at create time (where the entries are made, on the create's own threads).
	struct StepBrief { uint32_t entry_off, lds; uint16_t entry_count; uint8_t has_singles, pad; };
	struct EntryBrief { uint16_t grid_x, threads; uint32_t lds_x; GroupVariantPair variant; uint8_t pad[2]; };
	std::vector<StepBrief> step_brief;
	std::vector<EntryBrief> entry_brief;
	std::vector<ResBatchEntry> entries;
	ResBatchEntry* d_entries = nullptr;
	// chunked speculative backtrace (kernels_backtrace.h) of a table made of slot runs
	bool use_chunks = false;
	std::vector<BtChunk> chunks;
	BtChunk* d_chunks = nullptr;
	uint32_t* d_unit_x = nullptr;   // [2][units]
	uint32_t* d_path2 = nullptr;    // [2][columns]: speculative walks of the two orientations
	uint32_t* d_trans2 = nullptr;   // [orientations][columns]: their transmission values
	uint32_t n_orient_max = 1;      // most orientations any chunk has (2 for a single individual, 8 for a trio)
	uint8_t* d_sel = nullptr;
	uint32_t* d_guess = nullptr;
	uint32_t* d_bt_counters = nullptr;
	uint32_t n_spec = 0;
	size_t chunk_lds = 0;
	// slot runs (slots.h): the default forward path of a single individual
	SlotPlan splan;
	bool use_slots = false;
	int slot_l = 11;            // preferred number of local slots (lr + 6 .. lr + 9; pedigree runs: 6 - log2 T .. + 3, only when set explicitly)
	bool slot_l_set = false;
	int slot_lr = 2;            // reg slots: 4 cells per thread -> 8 waves per workgroup at 11 local slots (two waves per SIMD)
	int slot_lr_used = 2;       // ... of the plan in use (the shared-launches layout takes 3)
	std::vector<SlotBatchEntry> slot_entries;   // (pedigree runs: `pad` holds the run's index into splan.pextra)
	SlotBatchEntry* d_slot_entries = nullptr;
	uint64_t table_bytes = 0;   // pedigree slot runs: cost-form tables
	BtJob* d_btjobs = nullptr;
	uint32_t* d_job_scores = nullptr;
	bool shared_hint = false;   // option shared_launches: the table will be solved together with many others (enqueue_many)
	bool side_by_side = false;  // this solve's launches run beside other tables' on their own streams: X runs take the streamed variant (16 KB of LDS instead of ~90:
	                            // three tables on three streams, 3.1 M columns/s with the LDS lines -- one workgroup per CU, the streams take turns -- 5 M without)
	int max_lanes = 32;
	// Windowed solve (backtrace arena larger than what HBM can hold): the steps are cut into WINDOWS whose records fit the
	// arena one at a time.  Pass 1 runs the whole forward pass (records of all windows but the last are written and
	// dropped) and keeps the exchange column at every window boundary; then, newest window first, the window's steps
	// are run again from the kept column -- this time its records survive until its units have been walked.  Twice the
	// forward work, any table length.  Offsets into the arena are window-relative.
	struct Window {
		uint32_t step_lo = 0, step_hi = 0;   // positions in the job's step list
		uint32_t unit_off = 0, unit_count = 0;
	};
	uint64_t arena_limit = 0;   // option arena_limit_bytes (0: what hipMemGetInfo leaves)
	bool windowed = false;
	std::vector<Window> windows;
	uint8_t* d_checkpoints = nullptr;   // [windows - 1] exchange columns
	size_t checkpoint_bytes = 0;
	uint32_t* d_bt_state = nullptr;     // (x, transmission) the walk of a window hands to the next older one
	BtJob* d_window_jobs = nullptr;

	// the phases of a create (DeviceTable::upload), in the order they run
	whamd_status_t open(int dev, std::string& msg);
	whamd_status_t choose_plan(Problem& p, TableBuild& b, bool from_create, std::string& msg);
	void dump_plan(const Problem& p) const;
	whamd_status_t describe_columns(const Problem& p, TableBuild& b, std::string& msg);
	whamd_status_t lay_out_arena(const Problem& p, TableBuild& b, std::string& msg);
	size_t upload_bound(const Problem& p, const TableBuild& b) const;
	whamd_status_t upload_column_arrays(const Problem& p, TableBuild& b, TableUploader& up, std::string& msg);
	void build_slot_blobs(TableBuild& b) const;
	uint64_t lay_out_slot_tables(const TableBuild& b, bool report = true);
	whamd_status_t upload_slot_arrays(TableBuild& b, TableUploader& up, std::string& msg);
	void make_jobs();
	void make_units(const TableBuild& b);
	whamd_status_t make_windows(const TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t take_result_block(uint32_t n, TableUploader& up, std::string& msg);
	void cut_chunks(const Problem& p);
	whamd_status_t make_chunks(const Problem& p, TableUploader& up, std::string& msg);
	whamd_status_t take_solve_buffers(const Problem& p, TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t make_lanes(const TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t make_schedule(const TableBuild& b, std::string& msg);
	void make_briefs();
	whamd_status_t upload_entries(TableUploader& up, std::string& msg);
	whamd_status_t launch_table_kernels(const Problem& p, const TableBuild& b, TableUploader& up, std::string& msg);
	whamd_status_t arm_debug_stamps(TableUploader& up, std::string& msg);
	whamd_status_t record_group_backtrace(uint32_t n, TableUploader& up, std::string& msg);
	// The solve being submitted or awaiting collection.  (own_stream_used and upload_pending below describe the stream and the upload, not a solve.)
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
	whamd_status_t report_resident_stamps(std::string& msg) const;
	BtGroupEntry h_bt_entry{};          // what a batched backtrace launch reads for this table (kernels_backtrace.h backtrace_chunks_group), and its device copy
	BtGroupEntry* d_bt_entry = nullptr;
	// get_super_reads on the device (kernels_backtrace.h superreads_single): a table with one individual and trusted genotypes
	bool device_superreads = false;
	SuperreadArgs super_args{};
	size_t super_words = 0, super_off = 0;   // size of the result (u32 words) and where it lies in h_pinned
	bool own_stream_used = false;       // something has been submitted to `stream` since it was last synchronised (a member of a group solve never touches its own: its
	                                    // solve and tail are on the lead's stream, its uploads on an upload stream -- release() then has nothing to wait for there)
	bool upload_pending = false;        // the uploads went through a shared upload stream and no solve has been ordered behind `ev_upload` yet
	hipStream_t upload_stream = nullptr;

	// The preview (DESIGN.md 6.1 "preview"): the leading slot runs of a lone table's forward pass, launched on `stream` from INSIDE the create -- from arrays of
	// their own, uploaded first -- so that the device works while the host builds and uploads the whole table.  The finished schedule is then held against what
	// was launched (verify_preview); the first enqueue continues behind the preview where every step agrees, and starts at step 0 as ever where not.
	enum PreviewWhy : uint32_t { PV_RAN = 0, PV_OFF, PV_NOT_CREATE, PV_NOT_SLOTS, PV_DEBUG_SWITCH, PV_SHARED, PV_THREAD_BUDGET, PV_COMPONENTS, PV_FEW_PIECES, PV_NOT_ALONE, PV_NO_LEADING_RUNS,
	                           PV_ROW_PAD, PV_ARENA, PV_WHYS };
	struct Preview {
		int mode = -1;                      // option preview: -1 auto, 0 never, 1 wherever the table's form allows it
		uint32_t pieces_wanted = 0;         // option preview_pieces (0: the library's rule)
		bool thread_budget = false;         // the create is held to a thread budget (option host_threads)
		bool counted = false;               // this table is counted in tables_on_device
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
	static inline std::atomic<int> tables_on_device[64];   // tables of the process that hold device resources, per device (open / release_device)
	void give_preview_block() {   // (the caller knows the preview's launches are done)
		for (auto& a : preview.allocations) devpool_give(device, a.first, a.second);
		preview.allocations.clear();
	}
	struct PreviewPlan {   // plan_preview's answer
		uint32_t why = PV_NOT_CREATE, pieces = 0, steps = 0, end_col = 0, n_spec = 0, stride = 64, max_f = 0;
		bool chunked = false;
		uint64_t arena = 0, tab_words = 0;   // bytes of the arena (all steps), words of the preview's table block
		size_t ctrl_words = 0;
		std::vector<uint64_t> rec;           // [steps] record offsets
		std::vector<uint32_t> spec;          // [steps] seed ids
	};
	void plan_preview(const Problem& p, const TableBuild& b, bool from_create, PreviewPlan& out);
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

	void release_lanes() {
		max_grid_x = 1;
		lanes.clear();
		jobs.clear();
		schedule.clear();
		entries.clear();
		slot_entries.clear();
		windows.clear();
	}

	void release() {
		if (inflight.tail_elsewhere && ev3) (void)hipEventSynchronize(ev3);   // (a solve whose tail ran on the group's lead stream: nothing of it may still be reading the buffers)
		inflight.tail_elsewhere = false;
		if (upload_pending && ev_upload) (void)hipEventSynchronize(ev_upload);   // (a table closed without a solve: its copies may still be on the upload stream)
		upload_pending = false;
		release_lanes();
		windowed = false;
		if (stream && own_stream_used && (!allocations.empty() || d_arena)) { (void)hipStreamSynchronize(stream); own_stream_used = false; }   // (hipFree used to wait for the table's last kernels)
		for (auto& a : allocations) devpool_give(device, a.first, a.second);
		allocations.clear();
		give_preview_block();   // (its launches were on `stream`: synchronised above)
		if (preview.why != PV_NOT_CREATE) {   // (a table that never got as far as start_preview has nothing to reset; the options and the count outlive a release)
			Preview fresh;
			fresh.mode = preview.mode; fresh.pieces_wanted = preview.pieces_wanted; fresh.thread_budget = preview.thread_budget; fresh.counted = preview.counted;
			preview = std::move(fresh);
		}
		arena_give(device, d_arena, arena_bytes);
		d_arena = nullptr;
		arena_bytes = 0;
		pinned_give(h_pinned, h_pinned_bytes);
		h_pinned = nullptr;
		d_cols = nullptr;
		d_units = nullptr;
		d_pr[0] = d_pr[1] = nullptr;
		d_path_index = d_path_trans = d_score = nullptr;
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
	if (m.preview.counted && m.device >= 0 && m.device < 64) Impl::tables_on_device[m.device].fetch_sub(1);
	m.preview.counted = false;
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

// Runs of set bits of `mask` as deposit segments (compact position | mask position << 8 | length << 16).
static void append_segments(uint32_t mask, std::vector<uint32_t>& out, uint16_t& count) {
	uint32_t src = 0;
	count = 0;
	for (uint32_t bit = 0; bit < 32;) {
		if (!((mask >> bit) & 1u)) { ++bit; continue; }
		uint32_t len = 0;
		while (bit + len < 32 && ((mask >> (bit + len)) & 1u)) ++len;
		out.push_back(src | (bit << 8) | (len << 16));
		++count;
		src += len;
		bit += len;
	}
}

bool DeviceTable::set_path(const std::string& path) {
	if (path != "auto" && path != "column" && path != "column_keys" && path != "resident" && path != "slots") return false;
	impl_->path = path;
	return true;
}

void DeviceTable::set_l_pref(int l) { impl_->l_pref = std::max(4, std::min(l, RES_LMAX)); }
void DeviceTable::set_lanes(int n) { impl_->max_lanes = n < 1 ? 1 : (n > 64 ? 64 : n); }

void DeviceTable::set_fold(bool v) { impl_->fold = v; }
void DeviceTable::set_slot_l(int l) { impl_->slot_l = std::max(2, std::min(l, 12)); impl_->slot_l_set = true; }
void DeviceTable::set_slot_lr(int lr) { impl_->slot_lr = lr >= 3 ? 3 : (lr <= 1 ? 1 : 2); }

void DeviceTable::set_arena_limit(uint64_t bytes) { impl_->arena_limit = bytes; }
void DeviceTable::set_shared_launches(bool v) { impl_->shared_hint = v; }
void DeviceTable::set_side_by_side(bool v) { impl_->side_by_side = v; }
void DeviceTable::set_preview(int mode) { impl_->preview.mode = mode < 0 ? -1 : (mode ? 1 : 0); }
void DeviceTable::set_preview_pieces(uint32_t pieces) { impl_->preview.pieces_wanted = pieces; }
void DeviceTable::set_thread_budget(bool v) { impl_->preview.thread_budget = v; }
void DeviceTable::set_symmetry(int level) { impl_->symmetry = level < 0 ? 0 : (level > 2 ? 2 : level); }

// ================================================================================================ create: the phases of DeviceTable::upload
// Each phase says in its parameters what it touches: `Problem`, the build object (TableBuild: what later phases read), the uploader (TableUploader: the phase
// allocates, copies or launches).  Everything else it reads and writes is the table's own state in Impl.  The order of the phases that take an uploader IS the
// layout of the table's device block and the order of its driver calls.

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
	if (!m.preview.counted && dev >= 0 && dev < 64) { Impl::tables_on_device[dev].fetch_add(1); m.preview.counted = true; }
	return WHAMD_OK;
}

// The plan pieces a preview covers: what the option asks for, else a sixth of the table's (plan_preview; choose_plan's head hook asks the planner for the same).
static uint32_t preview_pieces_of(uint32_t wanted, uint32_t n_pieces) { return wanted ? wanted : std::max(1u, n_pieces / 6); }

// The kernels (templated or wide), the forward path (slot runs, LDS-resident runs, per column) and its plan.  Produces b.force_keys and b.free_b, decides where the superreads
// are made, and fills the problem's lazy term lists where the chosen path reads them.
whamd_status_t DeviceTable::Impl::choose_plan(Problem& p, TableBuild& b, bool from_create, std::string& msg) {
	Impl& m = *this;
	m.preview.tried = false;
	m.preview.from_hook = false;
	// pedigrees beyond the templated kernels (three trios, more than six individuals): the generic per-column kernel, key path only
	m.wide = !select_kernels(p.T, p.n_ind, m.fused, m.keysfn);
	if (m.wide && (p.T > (uint32_t)MAX_T_WIDE || p.n_ind > (uint32_t)MAX_IND_WIDE)) {
		msg = "no device kernel for T=" + std::to_string(p.T) + ", individuals=" + std::to_string(p.n_ind);
		return WHAMD_ERR_UNSUPPORTED;
	}
	// ... and a column with more allele-assignment terms than the templated kernels stage in LDS (genotypes not trusted, seven and more
	// individuals): the generic kernel reads them from global memory
	for (uint32_t c = 0; c < p.n_cols && !m.wide; ++c) m.wide = p.term_end(c, p.T - 1) - p.term_begin(c, 0) > (uint64_t)COL_MAXTERMS;
	b.laps.lap("plan: kernels chosen, term counts scanned");
	b.force_keys = m.path == "column_keys" || m.wide;
	const bool want_resident = (m.path == "auto" || m.path == "resident") && !m.wide;
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
	int slot_lr = m.slot_lr, slot_l = m.slot_l;
	if (m.shared_hint && p.T == 1 && p.max_k >= 18 && !m.slot_l_set && m.slot_lr == 2) { slot_lr = 3; slot_l = 12; }
	// Coverage 21 and 22 (512 / 1 024 workgroups of four cells per launch: the table fills the chip by itself, rounds of workgroups queue behind each
	// other) take the eight-cell layout ALONE as well: 14.0 against 17.9 us per launch at 21, 20.3 against 30.1 at 22 (scripts/gpu_wide_ab.py; the same
	// kernels with their operands streamed: 14.4 / 22.6).  At 23 the four-cell kernel with streamed operands wins (36.2 against 43.0 us): launch_slot_run.
	if (p.T == 1 && p.max_k >= 21 && p.max_k <= 22 && !m.slot_l_set && m.slot_lr == 2 && !debug_env("WHAMD_NO_WIDE_LAYOUT")) { slot_lr = 3; slot_l = 12; }
	m.slot_lr_used = slot_lr;
	// A lone single-individual table: the planner finishes the steps of the table's preview first and calls back (slots.h SlotPlanHead); the preview's runs are
	// launched from there, and the planner's second half happens under them.  What start_preview reads of this function's results is set here, as it will be below.
	whamd_status_t head_status = WHAMD_OK;
	bool steps_adopted = false;
	auto adopt_steps = [&]() {   // the driver walks plan.steps / plan.component_first_step; slot runs are steps of kind 2
		m.plan = ResidentPlan();
		m.plan.steps = m.splan.steps;
		m.plan.component_first_step = m.splan.component_first_step;
		m.plan.col_to_res.assign(p.n_cols, -1);
		steps_adopted = true;
	};
	SlotPlanHead head;
	{
		const uint32_t n_pieces = slot_plan_pieces(p.n_cols);
		const uint32_t pieces = std::min(n_pieces - 1, preview_pieces_of(m.preview.pieces_wanted, n_pieces));
		head.col_limit = slot_plan_piece_begin(p.n_cols, pieces);
		head.at_head = [&](uint32_t n_head) {
			if (n_head == 0) return;   // (the table does not begin with slot runs: upload() asks start_preview, which says why there is none)
			m.use_slots = true;
			m.table_bytes = 0;
			adopt_steps();
			b.laps.lap("plan: the planner up to the head's callback");
			m.preview.tried = true;
			m.preview.from_hook = true;
			head_status = m.start_preview(p, b, from_create, msg);
			if (m.preview.why != PV_RAN) m.preview.from_hook = false;
		};
	}
	// (only where a preview can still come about: what rules it out whatever the plan says -- plan_preview's first checks -- leaves the planner as it was)
	bool head_first = from_create && p.T == 1 && m.preview.mode != 0 && slot_plan_pieces(p.n_cols) >= 2 && !m.shared_hint && !m.side_by_side && !debug_env("WHAMD_NO_PREVIEW") &&
	                  !debug_env("WHAMD_NO_HEAD_FIRST");
	if (head_first && m.preview.mode < 0)
		head_first = !m.preview.thread_budget && slot_plan_pieces(p.n_cols) >= 8 && m.device >= 0 && m.device < 64 && Impl::tables_on_device[m.device].load() == 1;
	m.use_slots = (m.path == "auto" || m.path == "slots") && !m.wide &&
	              plan_forward_slots(p, p.T > 1 ? (m.slot_l_set ? -m.slot_l : 0) : std::max(8, slot_l), m.symmetry, m.splan, slot_lr, false, head_first ? &head : nullptr);
	if (head_status != WHAMD_OK) return head_status;
	b.laps.lap("plan: the planner");
	// pedigree slot runs keep their cost-form tables in HBM (slots.h): at most a quarter of what is free, else the older paths
	if (m.use_slots && m.splan.ped && m.splan.table_words * 4ull > free_b / 4) m.use_slots = false;
	m.table_bytes = m.use_slots && m.splan.ped ? m.splan.table_words * 4ull : 0ull;
	if (p.lazy_terms) {
		// generic term lists where something will read them: the columns a pedigree slot plan leaves to the per-column kernels; every column on any other path
		std::vector<uint8_t> need(p.n_cols, 1);
		if (m.use_slots && m.splan.ped) for (uint32_t c = 0; c < p.n_cols; ++c) need[c] = m.splan.col_to_row[c] < 0;
		const whamd_status_t st = fill_lazy_terms(p, need, msg);
		if (st != WHAMD_OK) return st;
	}
	if (m.use_slots) {
		if (!steps_adopted) adopt_steps();
	} else {
		m.splan = SlotPlan();
		plan_forward(p, want_resident, m.l_pref, m.fold, m.plan, m.symmetry);
	}
	// The superreads of a single-individual table with trusted genotypes are made on the device, behind the backtrace (the condition is finish_columns' first branch).
	m.device_superreads = p.n_ind == 1 && p.T == 1 && p.P == 2 && !p.distrust && p.h2p.size() >= 2 && p.h2p[0] == 0 && p.h2p[1] == 1 && p.genotype.size() >= p.n_cols &&
	                      !debug_env("WHAMD_HOST_SUPERREADS");
	b.laps.lap("plan: steps adopted, lazy terms");
	return WHAMD_OK;
}

// WHAMD_DEBUG_PLAN (debug library): the chosen plan, one line per step.
void DeviceTable::Impl::dump_plan(const Problem& p) const {
	const Impl& m = *this;
	for (const Step& st : m.plan.steps) {
		if (st.kind == 0) { fprintf(stderr, "[plan] column %u k=%u b=%u f=%u\n", st.index, p.k[st.index], p.b[st.index], p.f[st.index]); continue; }
		if (st.kind == 2) {
			const SlotRun& r = m.splan.runs[st.index];
			fprintf(stderr, "[plan] slot run c0=%u ncols=%u g=%u L=%u half=%u ends=%u has_prev=%u in_identity=%u in_half=%u mirror_pos=%u in_occ=%x out_occ=%x mirror_out=%u\n",
			        r.c0, r.ncols, r.g, r.L, r.half, r.n_ends, r.has_prev, r.in_identity, r.in_half, r.in_mirror_pos, r.in_occ, r.out_occ, r.mirror_out);
			if (m.splan.ped) fprintf(stderr, "[plan]   pedigree run: T=%u forms per value=%u table words=%u record words per workgroup=%u\n", 1u << m.splan.pextra[st.index].tb,
			                         m.splan.pextra[st.index].nf, m.splan.pextra[st.index].s_off + r.ncols * 64u * pslot_ns(m.splan.pextra[st.index].nf), m.splan.pextra[st.index].rec_words);
			continue;
		}
		const ResSegment& sgm = m.plan.segments[st.index];
		fprintf(stderr, "[plan] run c0=%u ncols=%u g=%u threads=%u max_l=%u stage_words=%u\n", sgm.c0, sgm.ncols, sgm.g, sgm.threads, sgm.max_l, sgm.stage_words);
		for (uint32_t i = 0; i < sgm.ncols; ++i) {
			const ResColumn& rc = m.plan.columns[sgm.col_off + i];
			const ResBacktrace& rb = m.plan.backtrace[sgm.col_off + i];
			fprintf(stderr, "[plan]   col %u mode=%u nfold=%u Lb=%u Lf=%u ebits=%u epos0=%u nthr=%u stage_off=%u nwords=%u | bt layout=%u n_g=%u n_l=%u\n",
			        sgm.c0 + i, rc.mode, rc.nfold, rc.Lb, rc.Lf, rc.ebits, rc.epos[0], rc.nthr, rc.stage_off, rc.nwords, rb.layout, rb.n_g, rb.n_l);
		}
	}
}

// What a column's descriptor holds by itself, and its 32-bit term offsets (b.term_ptr32): a few host threads.  Fails if the problem exceeds 32-bit offsets.  Host only.
whamd_status_t DeviceTable::Impl::describe_columns(const Problem& p, TableBuild& b, std::string& msg) {
	Impl& m = *this;
	const uint32_t n = b.n, ni = b.ni, tbits = b.tbits;
	if (p.terms.size() >= 0xFFFFFFFFull || (uint64_t)p.col_ptr[n] * ni >= 0xFFFFFFFFull) {
		msg = "problem too large for 32-bit device offsets";
		return WHAMD_ERR_UNSUPPORTED;
	}
	m.cols.resize(n);
	b.term_ptr32.resize((size_t)n * (p.T + 1));
	RawVec<uint32_t>& term_ptr32 = b.term_ptr32;
	parallel_ranges(n, host_threads(n, 16384), [&m, &p, &term_ptr32, n, ni, tbits](uint64_t c0, uint64_t c1, uint32_t) {
		for (uint32_t c = (uint32_t)c0; c < (uint32_t)c1; ++c) {
			DevColumn d{};
			d.k = p.k[c];
			d.b = p.b[c];
			d.f = p.f[c];
			d.recomb = p.recomb[c];
			d.delta_off = (uint32_t)(p.col_ptr[c] * ni);
			d.term_off = (uint32_t)((size_t)c * (p.T + 1));
			for (uint32_t t = 0; t <= p.T; ++t) term_ptr32[(size_t)c * (p.T + 1) + t] = (uint32_t)p.term_ptr[(size_t)c * p.T + t];
			d.ebits = d.k - d.f;
			d.is_last = (c + 1 == n);
			d.eloop = std::min<uint32_t>(d.ebits, QMAX);
			d.nplanes = d.ebits + tbits;
			m.cols[c] = d;
		}
	});
	return WHAMD_OK;
}

// The path a per-column step takes (0 fused, 1 keys) and the bytes of its backtrace record, from the column's sizes alone (lay_out_arena; the preview's arena bound).
static uint32_t column_step_mode(bool force_keys, bool is_last, uint32_t f, uint32_t ebits) { return (!force_keys && !is_last && f >= 6 && ebits <= (uint32_t)QMAX) ? 0u : 1u; }
static uint64_t column_record_bytes(uint32_t mode, uint32_t T, uint32_t f, uint32_t nplanes) {
	return mode == 0 ? (uint64_t)nplanes * T * (1ull << (f - 6)) * 8ull : (uint64_t)T * (1ull << f) * 4ull;
}
// What the backtrace arena may take: free HBM minus the descriptors (~1 KiB per column), exchange buffers, tables and slack; at most the option arena_limit_bytes.
static uint64_t arena_capacity(uint64_t free_b, uint32_t n, uint64_t table_bytes, uint64_t arena_limit) {
	const uint64_t reserve = (3ull << 30) + (uint64_t)n * 1024ull + table_bytes;
	uint64_t cap = free_b > reserve ? free_b - reserve : 0;
	if (arena_limit) cap = std::min<uint64_t>(cap, arena_limit);
	return cap;
}
// Where the next record starts behind one of `bytes` at `bt` (records are 16-byte aligned).
static uint64_t arena_behind(uint64_t bt, uint64_t bytes) { return (bt + bytes + 15ull) & ~15ull; }
// The record of one single-individual slot run: only launched workgroups write.
static uint64_t slot_run_record_bytes(const SlotRun& run) { return (uint64_t)run.n_ends * run.threads * (1ull << (run.g - run.half)); }

// The offsets that run through the table, in column order: segment lists (b.segs), the place of every backtrace unit's record in the arena (DevColumn::bt_off, the
// runs' rec / bt words), the windows where the arena is smaller than the records (b.window_first_col).  Produces b.arena_cap, b.bt, b.max_f, b.max_keys_f,
// b.exchange_bytes; fails if a unit or the whole does not fit.  Host only.
whamd_status_t DeviceTable::Impl::lay_out_arena(const Problem& p, TableBuild& b, std::string& msg) {
	Impl& m = *this;
	const uint32_t n = b.n;
	const bool ped_slots = b.ped_slots;
	std::vector<uint32_t>& segs = b.segs;
	uint64_t bt = 0, seg_bt = 0;
	size_t seg_cursor = 0, slot_cursor = 0;
	uint32_t max_f = 0, max_keys_f = 0;
	auto slot_record_bytes = [&m, ped_slots](size_t ri) -> uint64_t {   // record of one slot run: only launched workgroups write
		const SlotRun& run = m.splan.runs[ri];
		if (ped_slots) return (uint64_t)m.splan.pextra[ri].rec_words * 4ull << run.g;
		return slot_run_record_bytes(run);
	};
	const uint64_t arena_cap = arena_capacity(b.free_b, n, m.table_bytes, m.arena_limit);
	b.arena_cap = arena_cap;
	std::vector<uint32_t>& window_first_col = b.window_first_col;
	uint64_t bt_max = 0;
	auto open_unit = [&bt, &bt_max, &window_first_col, arena_cap](uint32_t c, uint64_t bytes) -> bool {   // a backtrace unit of `bytes` starts at column c
		if (bytes + 16 > arena_cap) return false;
		if (bt + bytes + 16 > arena_cap) {
			bt_max = std::max(bt_max, bt);
			bt = 0;
			window_first_col.push_back(c);
		}
		return true;
	};
	auto unit_too_large = [&msg, &b](uint32_t c) {
		msg = "the backtrace record of the unit at column " + std::to_string(c) + " alone does not fit in the arena (" + std::to_string(b.arena_cap >> 20) +
		      " MiB of " + std::to_string(b.free_b >> 20) + " MiB free HBM)";
		return WHAMD_ERR_UNSUPPORTED;
	};
	for (uint32_t c = 0; c < n; ++c) {
		DevColumn& d = m.cols[c];
		const bool in_slot_run = m.use_slots && m.splan.col_to_row[c] >= 0;   // (the run kernels read none of the per-column arrays)
		d.seg_off = (uint32_t)segs.size();
		const uint32_t kmask = d.k >= 32 ? 0xFFFFFFFFu : ((1u << d.k) - 1u);
		if (!in_slot_run) {
			append_segments(p.fwd_mask[c], segs, d.nseg_fwd);
			append_segments(kmask & ~p.fwd_mask[c], segs, d.nseg_end);
		}
		d.bt_off = bt;
		if (m.use_slots && m.splan.col_to_row[c] >= 0) {
			d.mode = 3;
			d.res_idx = (uint32_t)m.splan.col_to_row[c];
			if (slot_cursor < m.splan.runs.size() && m.splan.runs[slot_cursor].c0 == c) {  // first column of a slot run
				SlotRun& run = m.splan.runs[slot_cursor];
				if (!open_unit(c, slot_record_bytes(slot_cursor))) return unit_too_large(c);
				run.rec_lo = (uint32_t)bt;
				run.rec_hi = (uint32_t)(bt >> 32);
				seg_bt = bt;
				bt += slot_record_bytes(slot_cursor);
				max_f = std::max(max_f, run.L + run.g);   // entry / exit indices in physical order need 2^(L + g) entries
				++slot_cursor;
			}
			d.bt_off = seg_bt;
		} else if (m.plan.col_to_res[c] >= 0) {
			d.mode = 2;
			d.res_idx = (uint32_t)m.plan.col_to_res[c];
			if (seg_cursor < m.plan.segments.size() && m.plan.segments[seg_cursor].c0 == c) {  // first column of a run
				ResSegment& sgm = m.plan.segments[seg_cursor];
				if (!open_unit(c, (uint64_t)sgm.stage_words * (1ull << sgm.g) * 8ull)) return unit_too_large(c);
				sgm.bt_lo = (uint32_t)bt;
				sgm.bt_hi = (uint32_t)(bt >> 32);
				seg_bt = bt;
				bt += (uint64_t)sgm.stage_words * (1ull << sgm.g) * 8ull;
				++seg_cursor;
			}
			d.bt_off = seg_bt;
		} else {
			d.mode = column_step_mode(b.force_keys, d.is_last, d.f, d.ebits);
			const uint64_t bytes = column_record_bytes(d.mode, p.T, d.f, d.nplanes);
			if (!open_unit(c, bytes)) return unit_too_large(c);
			d.bt_off = bt;
			bt += bytes;
			if (d.mode != 0) max_keys_f = std::max(max_keys_f, d.f);
		}
		bt = (bt + 15ull) & ~15ull;
		max_f = std::max(max_f, d.f);
	}
	b.laps.lap("column descriptors (host)");
	bt = std::max(bt_max, bt);
	b.bt = bt;
	b.max_f = max_f;
	b.max_keys_f = max_keys_f;
	b.exchange_bytes = (size_t)(1ull << max_f) * p.T * 4;
	m.bt_bytes = bt;
	m.windowed = !window_first_col.empty();
	m.checkpoint_bytes = b.exchange_bytes;
	const uint64_t need = bt + (2ull + window_first_col.size()) * b.exchange_bytes + (1ull << max_keys_f) * p.T * 8ull;
	if (need + (1ull << 30) > b.free_b) {
		msg = "backtrace arena of " + std::to_string(need >> 20) + " MiB does not fit in free HBM (" + std::to_string(b.free_b >> 20) + " MiB)";
		return WHAMD_ERR_UNSUPPORTED;
	}
	return WHAMD_OK;
}

// An upper bound of what the phases below hand to TableUploader::up (the size of the table's device block and staging image).
size_t DeviceTable::Impl::upload_bound(const Problem& p, const TableBuild& b) const {
	const Impl& m = *this;
	const size_t delta_count = p.n_ind == 0 ? std::max<size_t>(p.col_ptr[b.n], 1) : (size_t)p.col_ptr[b.n] * p.n_ind;
	const size_t super_upload = m.device_superreads ? ((size_t)b.n + 1) * 8 + b.n + 1024 : 0;
	return m.cols.size() * sizeof(DevColumn) + delta_count * sizeof(int32_t) + b.term_ptr32.size() * 4 + (p.terms.size() + p.fterms.size()) * sizeof(DevTerm) + b.segs.size() * 4 +
	       m.plan.columns.size() * (sizeof(ResColumn) + sizeof(ResBacktrace) + sizeof(PedColumn)) + m.plan.ped_terms.size() * sizeof(PedTerm) +
	       (m.splan.rows.size() + SLOT_ROW_PAD) * sizeof(SlotRow) + m.splan.prows.size() * sizeof(PedSlotRow) + m.splan.bt_cols.size() * (sizeof(SlotBtCol) + 8) +
	       m.splan.runs.size() * (sizeof(SlotRun) + sizeof(PedSlotExtra) + sizeof(BtUnit) + sizeof(SlotBatchEntry) + 64) + m.plan.segments.size() * (sizeof(ResBatchEntry) + sizeof(BtUnit)) + super_upload + ((size_t)8 << 20);
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
	const bool sparse_columns = m.use_slots && !b.ped_slots && p.T == 1 && !m.windowed && !debug_env("WHAMD_DENSE_COLUMN_UPLOAD");
	if (sparse_columns) {
		std::vector<std::pair<size_t, size_t>> pc_cols, pc_delta, pc_tptr, pc_terms;   // byte ranges of the columns [c, e) outside runs
		for (uint32_t c = 0; c < n;) {
			if (m.splan.col_to_row[c] >= 0) { ++c; continue; }
			uint32_t e = c + 1;
			while (e < n && m.splan.col_to_row[e] < 0) ++e;
			pc_cols.emplace_back((size_t)c * sizeof(DevColumn), (size_t)e * sizeof(DevColumn));
			pc_delta.emplace_back((size_t)p.col_ptr[c] * p.n_ind * sizeof(int32_t), (size_t)p.col_ptr[e] * p.n_ind * sizeof(int32_t));
			pc_tptr.emplace_back((size_t)c * (p.T + 1) * sizeof(uint32_t), (size_t)e * (p.T + 1) * sizeof(uint32_t));
			pc_terms.emplace_back((size_t)p.term_ptr[(size_t)c * p.T] * sizeof(DevTerm), (size_t)p.term_ptr[(size_t)e * p.T] * sizeof(DevTerm));
			c = e;
		}
		HIP_TRY(up.up_pieces((void**)&m.d_cols, m.cols.data(), m.cols.size() * sizeof(DevColumn), pc_cols));
		// (the deltas travel whole when the device makes the superreads: superreads_single reads every column's)
		if (m.device_superreads) HIP_TRY(up.up((void**)&m.dp.delta, delta_src, delta_count * sizeof(int32_t)));
		else HIP_TRY(up.up_pieces((void**)&m.dp.delta, delta_src, delta_count * sizeof(int32_t), pc_delta));
		HIP_TRY(up.up_pieces((void**)&m.dp.term_ptr, b.term_ptr32.data(), b.term_ptr32.size() * sizeof(uint32_t), pc_tptr));
		HIP_TRY(up.up_pieces((void**)&m.dp.terms, terms.data(), terms.size() * sizeof(DevTerm), pc_terms));
	} else {
		HIP_TRY(up.up((void**)&m.d_cols, m.cols.data(), m.cols.size() * sizeof(DevColumn)));
		HIP_TRY(up.up((void**)&m.dp.delta, delta_src, delta_count * sizeof(int32_t)));
		HIP_TRY(up.up((void**)&m.dp.term_ptr, b.term_ptr32.data(), b.term_ptr32.size() * sizeof(uint32_t)));
		HIP_TRY(up.up((void**)&m.dp.terms, terms.data(), terms.size() * sizeof(DevTerm)));
	}
	m.dp.cols = m.d_cols;
	if (m.device_superreads) {
		m.super_args = SuperreadArgs{};
		HIP_TRY(up.up((void**)&m.super_args.col_ptr, p.col_ptr.data(), ((size_t)n + 1) * sizeof(uint64_t)));
		HIP_TRY(up.up((void**)&m.super_args.genotype, p.genotype.data(), (size_t)n));
		m.super_args.delta = m.dp.delta;
		m.super_args.n_cols = n;
		m.super_words = (size_t)n + ((size_t)2 * n + 3) / 4;
	}
	b.d_fterms = nullptr;
	if (!p.fterms.empty()) HIP_TRY(up.up((void**)&b.d_fterms, p.fterms.data(), p.fterms.size() * sizeof(DevTerm)));   // factorised lines (pedslot_tables, PSLOT_FACT)
	HIP_TRY(up.up((void**)&m.dp.segs, b.segs.data(), b.segs.size() * sizeof(uint32_t)));
	HIP_TRY(up.up((void**)&m.dp.res_cols, m.plan.columns.data(), m.plan.columns.size() * sizeof(ResColumn)));
	HIP_TRY(up.up((void**)&m.dp.res_bt, m.plan.backtrace.data(), m.plan.backtrace.size() * sizeof(ResBacktrace)));
	m.plan.ped_columns.resize(m.plan.ped_columns.empty() ? 0 : m.plan.columns.size());
	HIP_TRY(up.up((void**)&m.dp.ped_cols, m.plan.ped_columns.data(), m.plan.ped_columns.size() * sizeof(PedColumn)));
	HIP_TRY(up.up((void**)&m.dp.ped_terms, m.plan.ped_terms.data(), m.plan.ped_terms.size() * sizeof(PedTerm)));
	b.laps.lap("column arrays: allocations + copies");
	return WHAMD_OK;
}

// Slot runs: the backtrace blob ([ncols] SlotBtCol + ending slots per run) and where every run's piece lies in it (b.slot_blob_off / _words).  Host only.
void DeviceTable::Impl::build_slot_blobs(TableBuild& b) const {
	const Impl& m = *this;
	b.slot_blob_off.assign(m.splan.runs.size(), 0);
	b.slot_blob_words.assign(m.splan.runs.size(), 0);
	// offsets first (one pass over the runs), then every run copies its own piece (8 MB for configs[2]: 0.9 ms when it was one growing vector)
	size_t words = 0;
	for (size_t ri = 0; ri < m.splan.runs.size(); ++ri) {
		const SlotRun& run = m.splan.runs[ri];
		b.slot_blob_off[ri] = (uint32_t)words;
		b.slot_blob_words[ri] = (uint32_t)((size_t)run.ncols * (sizeof(SlotBtCol) / 4) + (run.n_ends + 3) / 4 + 1);
		words += b.slot_blob_words[ri];
	}
	b.slot_blob.resize(words);
	uint32_t* blob = b.slot_blob.data();
	const uint32_t* blob_off = b.slot_blob_off.data();
	parallel_ranges(m.splan.runs.size(), host_threads(m.splan.runs.size(), 512), [&m, blob, blob_off](uint64_t r0, uint64_t r1, uint32_t) {
		for (size_t ri = r0; ri < r1; ++ri) {
			const SlotRun& run = m.splan.runs[ri];
			uint32_t* dst = blob + blob_off[ri];
			const size_t col_words = (size_t)run.ncols * (sizeof(SlotBtCol) / 4);
			std::memcpy(dst, m.splan.bt_cols.data() + run.row_off, col_words * 4);
			const size_t end_words = (run.n_ends + 3) / 4 + 1;
			std::memset(dst + col_words, 0, end_words * 4);
			if (run.n_ends) std::memcpy(dst + col_words, m.splan.end_slots.data() + m.splan.end_off[ri], run.n_ends);
		}
	});
}

// Single-individual slot runs: where the prologue's tables of every run (SlotRun::tab_g / tab_w / tab_sl, an X run's tab_kr / tab_par) lie in the table block that
// slot_tables fills; marks the X runs.  Returns the block's size in words.  Host only, and the same on every call (the preview lays the tables out before the create does).
uint64_t DeviceTable::Impl::lay_out_slot_tables(const TableBuild& b, bool report) {
	Impl& m = *this;
	uint64_t slot_tab_words = 0;
	for (SlotRun& run : m.splan.runs) {
		auto pad4 = [](uint64_t v) { return (v + 3ull) & ~3ull; };
		// X runs (kernels_slots.h, slot_runx_body): a Y-form run with four cells per thread whose columns and ending reads fit the kernel's registers; the
		// rows of its tables are padded with zero columns to a pair of trips
		const bool xrun = (run.yflags & 1u) && (run.lr == 2u || (run.lr == 3u && !debug_env("WHAMD_NO_XRUN8"))) && run.ncols <= (uint32_t)SLOT_XCOLS &&
		                  run.n_ends <= (uint32_t)SLOT_XENDS && !debug_env("WHAMD_NO_XRUN");
		const uint64_t ncp = xrun ? ((run.ncols + 7u) & ~7u) : run.ncols;
		run.tab_g = (uint32_t)slot_tab_words;
		slot_tab_words += pad4(ncp << (run.g - run.half));
		run.tab_w = (uint32_t)slot_tab_words;
		slot_tab_words += pad4(ncp * (run.threads >> 6));
		run.tab_sl = (uint32_t)slot_tab_words;
		slot_tab_words += ncp * 64u;
		if (xrun) {
			run.yflags |= 8u;
			slot_tab_words = (slot_tab_words + 15u) & ~(uint64_t)15;   // (a trip's sixteen Kr words are ONE 64-byte line of the scalar cache)
			run.tab_kr = (uint32_t)slot_tab_words;
			slot_tab_words += pad4((((uint64_t)run.ncols + SLOT_XPAD) << run.lr) + run.ncols + SLOT_XPAD);   // Kr words, then one control word per column
			run.tab_par = (uint32_t)slot_tab_words;
			slot_tab_words += pad4((uint64_t)run.threads + (1ull << (run.g - run.half)));
		}
	}
	slot_tab_words += (uint64_t)SLOT_XCOLS * 64u;   // (an X run requests the lane parts of SLOT_XCOLS columns whatever its length)
	if (b.laps.on && report) {
		size_t nx = 0, not_y = 0, not_lr = 0, long_run = 0, many_ends = 0;
		for (const SlotRun& run : m.splan.runs) {
			nx += (run.yflags & 8u) != 0;
			not_y += !(run.yflags & 1u); not_lr += run.lr != 2u && run.lr != 3u; long_run += run.ncols > (uint32_t)SLOT_XCOLS; many_ends += run.n_ends > (uint32_t)SLOT_XENDS;
		}
		fprintf(stderr, "[whamd timing]   X runs: %zu of %zu (not Y form %zu, cells per thread %zu, more than %d columns %zu, more than %d ending reads %zu)\n", nx, m.splan.runs.size(), not_y,
		        not_lr, SLOT_XCOLS, long_run, SLOT_XENDS, many_ends);
	}
	return slot_tab_words;
}

// What the slot-run kernels read: rows, backtrace blobs, control words, the runs themselves and the block their tables are built in (single individual:
// slot_tables; pedigree: pedslot_tables, with the pedigree rows and extras).  Produces b.d_runs / b.d_pextra for launch_table_kernels.
whamd_status_t DeviceTable::Impl::upload_slot_arrays(TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	build_slot_blobs(b);
	b.laps.lap("slot backtrace blobs (host)");
	if (!m.splan.rows.empty()) m.splan.rows.resize(m.splan.rows.size() + SLOT_ROW_PAD);   // the kernel's scalar-cache warm-up touches a fixed number of rows
	HIP_TRY(up.up((void**)&m.dp.slot_rows, m.splan.rows.data(), m.splan.rows.size() * sizeof(SlotRow)));
	b.laps.lap("slot rows: allocation + copy");
	HIP_TRY(up.up((void**)&m.dp.slot_blob, b.slot_blob.data(), b.slot_blob.size() * sizeof(uint32_t)));
	HIP_TRY(up.up((void**)&m.dp.slot_ctrl, m.splan.ctrl.data(), m.splan.ctrl.size() * sizeof(uint32_t)));
	m.dp.slot_tab = nullptr;
	b.d_runs = nullptr;
	if (m.use_slots && !b.ped_slots) {
		const uint64_t slot_tab_words = lay_out_slot_tables(b);
		if (slot_tab_words >= 0xFFFFFFFFull) { msg = "slot-run tables exceed 32-bit offsets"; return WHAMD_ERR_UNSUPPORTED; }
		HIP_TRY(up.up((void**)&b.d_runs, m.splan.runs.data(), m.splan.runs.size() * sizeof(SlotRun)));
		b.laps.lap("slot blobs, control words, runs: allocations + copies");
		HIP_TRY(up.alloc((void**)&m.dp.slot_tab, slot_tab_words * 4));
		b.laps.lap("slot tables: allocation");
	}
	m.dp.pslot_rows = nullptr;
	m.dp.pslot_tab = nullptr;
	b.d_pextra = nullptr;
	if (b.ped_slots) {
		HIP_TRY(up.up((void**)&m.dp.pslot_rows, m.splan.prows.data(), m.splan.prows.size() * sizeof(PedSlotRow)));
		HIP_TRY(up.up((void**)&b.d_runs, m.splan.runs.data(), m.splan.runs.size() * sizeof(SlotRun)));
		HIP_TRY(up.up((void**)&b.d_pextra, m.splan.pextra.data(), m.splan.pextra.size() * sizeof(PedSlotExtra)));
		HIP_TRY(up.alloc((void**)&m.dp.pslot_tab, m.table_bytes));
	}
	b.laps.lap("slot rows / blobs / control words: allocations + copies");
	return WHAMD_OK;
}

// Jobs (see Impl::Job): connected components made of runs only get their own job.  Host only.
void DeviceTable::Impl::make_jobs() {
	Impl& m = *this;
	m.release_lanes();
	Impl::Job final_job;
	final_job.final = true;
	std::vector<Impl::Job> component_jobs;
	const std::vector<uint32_t>& first = m.plan.component_first_step;
	// Components as jobs of their own run side by side on lanes -- and walk back one after the other through the SEQUENTIAL backtrace (the chunked one takes a
	// single job): 16 ms for an irregular coverage-20 table of 200 000 columns whose forward pass is 57 ms, nearly all of it one giant component (a Poisson layout
	// leaves a gap every few ten thousand columns).  A table whose largest component holds four fifths of its steps or more stays ONE job: the lanes would gain
	// less than the walk loses ((1 - s) x forward against s x 16 ms).  WHAMD_SPLIT_COMPONENTS=1 (debug library): always split, as before.
	size_t largest = 0;
	for (size_t k = 0; k < first.size(); ++k) largest = std::max<size_t>(largest, (k + 1 < first.size() ? first[k + 1] : m.plan.steps.size()) - first[k]);
	const bool worth_splitting = largest * 5 < m.plan.steps.size() * 4 || debug_env("WHAMD_SPLIT_COMPONENTS");
	const bool split = m.max_lanes > 1 && first.size() > 1 && worth_splitting && !debug_env("WHAMD_DEBUG_STAMPS") && !m.windowed;
	if (!split) {
		for (uint32_t si = 0; si < m.plan.steps.size(); ++si) final_job.steps.push_back(si);
	} else {
		for (size_t k = 0; k < first.size(); ++k) {
			const uint32_t s0 = first[k], s1 = k + 1 < first.size() ? first[k + 1] : (uint32_t)m.plan.steps.size();
			Impl::Job* job = &final_job;
			if (k + 1 < first.size()) { component_jobs.emplace_back(); job = &component_jobs.back(); }
			for (uint32_t si = s0; si < s1; ++si) job->steps.push_back(si);
		}
	}
	m.jobs.push_back(std::move(final_job));
	for (Impl::Job& j : component_jobs) m.jobs.push_back(std::move(j));
}

// The backtrace units: every job's steps in reverse order, each with everything the walk needs of it.  Reads b.segs, b.slot_blob_off / _words.  Host only.
void DeviceTable::Impl::make_units(const TableBuild& b) {
	Impl& m = *this;
	m.units.clear();
	for (Impl::Job& job : m.jobs) {
		job.unit_off = (uint32_t)m.units.size();
		for (size_t sj = job.steps.size(); sj-- > 0;) {
			const Step& st = m.plan.steps[job.steps[sj]];
			BtUnit u{};
			u.kind = st.kind;
			if (st.kind == 0) {
				// column step: everything the backtrace needs, so that its chain holds no descriptor load
				const DevColumn& d = m.cols[st.index];
				u.c0 = st.index;
				u.ncols = 1;
				u.g = d.f; u.Lf_last = d.mode; u.stage_words = d.nplanes; u.n_wext = d.ebits;
				u.bt_lo = (uint32_t)d.bt_off; u.bt_hi = (uint32_t)(d.bt_off >> 32);
				u.n_lext = d.nseg_fwd; u.pad0 = d.nseg_end;
				const uint32_t nseg = (uint32_t)d.nseg_fwd + d.nseg_end;
				if (nseg <= (uint32_t)(RES_IOSEG + RES_BT_LRUNS)) {
					uint32_t* dst = u.wext;  // wext[6] and lext[10] are contiguous: 16 run slots
					for (uint32_t i = 0; i < nseg; ++i) dst[i] = b.segs[d.seg_off + i];
					u.pad1[0] = 1;  // runs are inline
				}
			} else if (st.kind == 2) {
				const SlotRun& run = m.splan.runs[st.index];
				SlotBtUnit su{};
				su.kind = b.ped_slots ? 3 : 2; su.c0 = run.c0; su.ncols = run.ncols; su.blob_off = b.slot_blob_off[st.index];
				su.g = run.g; su.L = run.L; su.n_ends = run.n_ends; su.threads = run.threads;
				su.bt_lo = run.rec_lo; su.bt_hi = run.rec_hi; su.half = run.half; su.blob_words = b.slot_blob_words[st.index];
				su.f_exit = m.splan.f_exit[st.index];
				for (uint32_t j = 0; j < su.f_exit && j < 32; ++j) su.exit_pos[j] = (uint8_t)slot_pos(run.out_pos, m.splan.exit_slot[st.index][j]);
				su.lr = run.lr;
				if (b.ped_slots) { su.n_ends = m.splan.pextra[st.index].rec_words; su.lr = m.splan.pextra[st.index].tb; }   // kind 3: words of one workgroup's record, log2 T
				for (uint32_t j = 0; j < su.f_exit && j < 32; ++j) su.exit_slot[j] = m.splan.exit_slot[st.index][j];
				static_assert(sizeof(SlotBtUnit) == sizeof(BtUnit), "unit headers share one array");
				std::memcpy(&u, &su, sizeof u);
			} else {
				const ResSegment& sgm = m.plan.segments[st.index];
				u.c0 = sgm.c0; u.ncols = sgm.ncols; u.col_off = sgm.col_off; u.g = sgm.g; u.Lf_last = sgm.Lf_last;
				u.stage_words = sgm.stage_words; u.n_wext = sgm.n_wext; u.bt_lo = sgm.bt_lo; u.bt_hi = sgm.bt_hi;
				u.n_lext = sgm.n_lext;
				u.pad0 = (uint32_t)sgm.bt_active | ((uint32_t)sgm.bt_simple << 16) | (sgm.half << 20);
				std::copy(sgm.wext, sgm.wext + RES_IOSEG, u.wext);
				std::copy(sgm.lext, sgm.lext + RES_BT_LRUNS, u.lext);
			}
			m.units.push_back(u);
		}
		job.unit_count = (uint32_t)m.units.size() - job.unit_off;
	}
}

// Windows (see Impl::Window): the single job's steps cut where the arena offsets start over (b.window_first_col); their backtrace jobs, the kept boundary columns
// and the state one window's walk hands to the next.
whamd_status_t DeviceTable::Impl::make_windows(const TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.dp.bt_state = nullptr;
	if (!m.windowed) return WHAMD_OK;
	const std::vector<uint32_t>& window_first_col = b.window_first_col;
	const std::vector<uint32_t>& steps = m.jobs[0].steps;
	const uint32_t n_steps = (uint32_t)steps.size();
	auto first_col = [&m, &steps](uint32_t pos) {
		const Step& st = m.plan.steps[steps[pos]];
		return st.kind == 0 ? st.index : (st.kind == 2 ? m.splan.runs[st.index].c0 : m.plan.segments[st.index].c0);
	};
	Impl::Window w;
	size_t next = 0;
	for (uint32_t pos = 0; pos < n_steps; ++pos) {
		if (next < window_first_col.size() && first_col(pos) == window_first_col[next]) {
			w.step_hi = pos;
			m.windows.push_back(w);
			w = Impl::Window();
			w.step_lo = pos;
			++next;
		}
	}
	w.step_hi = n_steps;
	m.windows.push_back(w);
	if (next != window_first_col.size()) { msg = "internal error: a window does not start at a step"; return WHAMD_ERR_DEVICE; }
	std::vector<BtJob> wjobs;
	for (size_t wi = 0; wi < m.windows.size(); ++wi) {   // units are the steps in reverse order
		Impl::Window& win = m.windows[wi];
		win.unit_off = n_steps - win.step_hi;
		win.unit_count = win.step_hi - win.step_lo;
		wjobs.push_back(BtJob{win.unit_off, win.unit_count, wi + 1 == m.windows.size() ? 1u : 2u, 0u});
	}
	HIP_TRY(up.up((void**)&m.d_window_jobs, wjobs.data(), wjobs.size() * sizeof(BtJob)));
	HIP_TRY(up.alloc((void**)&m.d_checkpoints, (m.windows.size() - 1) * m.checkpoint_bytes));
	HIP_TRY(up.alloc((void**)&m.d_bt_state, 16));
	m.dp.bt_state = m.d_bt_state;
	if (b.laps.on) fprintf(stderr, "[whamd timing] windowed solve: %zu windows, arena %.2f GB\n", m.windows.size(), (double)b.bt / 1e9);
	return WHAMD_OK;
}

// Everything a solve hands back lies in ONE device block, laid out like the pinned buffer it is downloaded into: [n] path index, [n] path transmission, the
// final job's score with the other jobs' behind it (d_job_scores[0] IS d_score: job 0 is the final one and has no entry of its own), four words of backtrace
// counters, the superreads.  Five copies per table -- 4.6 us each as blit kernels, one after the other on a group's stream: 2.6 ms behind a 96-table solve -- are one.
whamd_status_t DeviceTable::Impl::take_result_block(uint32_t n, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.super_off = 2 * (size_t)n + 4 + m.jobs.size();
	void* d_res = nullptr;
	HIP_TRY(up.alloc(&d_res, (m.super_off + (m.device_superreads ? m.super_words : 0)) * sizeof(uint32_t) + 16));
	uint32_t* res = (uint32_t*)d_res;
	m.d_path_index = res;
	m.d_path_trans = res + n;
	m.d_score = res + 2 * (size_t)n;
	m.d_job_scores = res + 2 * (size_t)n;
	m.d_bt_counters = res + 2 * (size_t)n + m.jobs.size();
	if (m.device_superreads) {
		m.super_args.out = res + m.super_off;
		m.super_args.path_index = m.d_path_index;
	}
	return WHAMD_OK;
}

namespace {

// Orientation generators of the speculative backtrace (BtChunk): per individual the transmission bits its relabelling flips -- a founder those of the
// trios it is a parent of, a child both of its own trio (exact where genotypes are heterozygous); individuals that are
// both, or pedigrees with more than BT_GENERATORS individuals, get no generator (still exact, more walked twice).  Pure in the problem.
struct OrientationGenerators {
	std::vector<int> of_individual;   // -1: none
	std::vector<uint32_t> tflip;
	explicit OrientationGenerators(const Problem& p) : of_individual(std::max<uint32_t>(p.n_ind, 1), -1) {
		if (p.n_ind < 2 || p.n_ind > BT_GENERATORS) return;
		for (uint32_t s = 0; s < p.n_ind; ++s) {
			uint32_t as_parent = 0, as_child = 0;
			for (uint32_t t3 = 0; t3 < p.n_triples; ++t3) {
				if (p.triples[t3][0] == s) as_parent |= 1u << (2 * t3);
				if (p.triples[t3][1] == s) as_parent |= 1u << (2 * t3 + 1);
				if (p.triples[t3][2] == s) as_child |= 3u << (2 * t3);
			}
			if (as_parent && as_child) continue;
			if (!as_parent && !as_child) continue;   // unrelated individual of a multi-sample table
			of_individual[s] = (int)tflip.size();
			tflip.push_back(as_parent | as_child);
		}
	}
	// the orientations of a chunk that starts from the projection column of column c_last: bit j = j-th forwarded read
	void orient(const Problem& p, uint32_t c_last, BtChunk& ch) const {
		ch.n_orient = 1;
		for (uint32_t q = 0; q < BT_GENERATORS; ++q) ch.flip[q] = 0;
		if (p.n_triples == 0 && p.n_ind <= 1) {
			const uint32_t fb = p.f[c_last];
			ch.flip[0] = fb >= BT_STATE_TSHIFT ? BT_STATE_XMASK : ((1u << fb) - 1u);
			ch.n_orient = 2;
			return;
		}
		if (tflip.empty()) return;
		const ColumnEntry* col = p.col_begin(c_last);
		uint32_t bit = 0;
		for (uint32_t j = 0; j < p.k[c_last]; ++j) {
			if (!((p.fwd_mask[c_last] >> j) & 1u)) continue;
			const int gq = of_individual[col[j].sample];
			if (gq >= 0) ch.flip[gq] |= 1u << bit;
			++bit;
		}
		for (size_t q = 0; q < tflip.size(); ++q) ch.flip[q] |= tflip[q] << BT_STATE_TSHIFT;
		ch.n_orient = 1u << tflip.size();
	}
};

}  // namespace

namespace {
// The chunk rule of the speculative backtrace over a job's units, newest first (unit u is the job's step size - 1 - u): a run that finds BT_CHUNK_RUNS runs in the
// chunk in front of it starts a new chunk and leaves that chunk's seed.  starts(u, id) is called for every such unit, id = 1, 2, ...; returns how many there are.
// (make_chunks walks the units with it, the preview the plan's steps: one rule.)
template <class IsRun, class Starts>
uint32_t cut_chunk_starts(size_t n_units, IsRun is_run, Starts starts) {
	uint32_t n_spec = 0, runs_in_chunk = 0;
	for (size_t u = 0; u < n_units; ++u) {
		const bool run = is_run(u);
		if (run && runs_in_chunk >= (uint32_t)BT_CHUNK_RUNS && u > 0) {
			starts(u, ++n_spec);
			runs_in_chunk = 0;
		}
		runs_in_chunk += run;
	}
	return n_spec;
}
// Whether a table walks back in chunks at all: runs (slot runs, or the LDS-resident trio runs), one job, not windowed, more than two chunks' worth of units.
bool backtrace_is_chunked(bool on_runs, size_t n_jobs, bool windowed, size_t n_units) {
	return on_runs && n_jobs == 1 && !windowed && !getenv("WHAMD_BT_SEQUENTIAL") && n_units > 2u * BT_CHUNK_RUNS;
}
// The seeds' stride: the most waves any run that leaves a seed has (at least 64 words).
uint32_t seed_stride_of(uint32_t stride, const SlotRun& run) { return std::max(stride, (run.threads >> 6) << (run.g - run.half)); }
}  // namespace

// Chunks of the speculative backtrace (single job only); the run that leaves a chunk's seed gets its spec id.  Host only.
// Produces m.use_chunks, m.chunks, m.n_spec, m.n_orient_max and m.dp.spec_stride.
void DeviceTable::Impl::cut_chunks(const Problem& p) {
	Impl& m = *this;
	m.use_chunks = false;
	m.chunks.clear();
	m.n_spec = 0;
	for (SlotRun& run : m.splan.runs) run.spec_id = 0;
	const bool trio_runs = !m.use_slots && !m.plan.ped_columns.empty();   // LDS-resident trio runs (kernels_trio.h)
	if (trio_runs) for (ResSegment& sgm : m.plan.segments) sgm.in_mirror_bit = 0;   // (trio runs have no mirror: the field carries the spec id)
	if (!backtrace_is_chunked(m.use_slots || trio_runs, m.jobs.size(), m.windowed, m.units.size())) return;
	m.use_chunks = true;
	const OrientationGenerators generators(p);
	BtChunk first{};
	first.n_orient = 1;   // the newest chunk starts from the table's optimum
	m.chunks.push_back(first);
	m.n_spec = cut_chunk_starts(m.units.size(),
		[&m, trio_runs](size_t u) { return m.units[u].kind == 2 || m.units[u].kind == 3 || (trio_runs && m.units[u].kind == 1); },
		[&m, &p, &generators, trio_runs](size_t u, uint32_t id) {
			m.chunks.back().unit_count = (uint32_t)u - m.chunks.back().unit_off;
			BtChunk cur{};
			cur.unit_off = (uint32_t)u;
			cur.spec_id = id;
			generators.orient(p, m.units[u].c0 + m.units[u].ncols - 1, cur);   // (the last column of unit u's step)
			m.chunks.push_back(cur);
			// the run of unit u leaves the seed: units are the job's steps in reverse order
			const Step& st = m.plan.steps[m.jobs[0].steps[m.jobs[0].steps.size() - 1 - u]];
			if (trio_runs) m.plan.segments[st.index].in_mirror_bit = id;
			else m.splan.runs[st.index].spec_id = id;
		});
	m.chunks.back().unit_count = (uint32_t)m.units.size() - m.chunks.back().unit_off;
	m.n_orient_max = 1;
	for (const BtChunk& ch : m.chunks) m.n_orient_max = std::max(m.n_orient_max, ch.n_orient);
	uint32_t stride = 64;
	for (const SlotRun& run : m.splan.runs) if (run.spec_id) stride = seed_stride_of(stride, run);
	if (trio_runs) for (const ResSegment& sgm : m.plan.segments) if (sgm.in_mirror_bit) stride = std::max(stride, (sgm.threads >> 6) << sgm.g);
	m.dp.spec_stride = stride;
}

// The chunks (cut_chunks), their device copy, the walk's buffers and m.dp.spec_keys (the schedule's entries carry it and the stride).
whamd_status_t DeviceTable::Impl::make_chunks(const Problem& p, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	const uint32_t n = p.n_cols;
	m.dp.spec_keys = nullptr;
	m.cut_chunks(p);
	if (!m.use_chunks) return WHAMD_OK;
	const uint32_t stride = m.dp.spec_stride;
	HIP_TRY(up.up((void**)&m.d_chunks, m.chunks.data(), m.chunks.size() * sizeof(BtChunk)));
	HIP_TRY(up.alloc((void**)&m.d_unit_x, (size_t)m.n_orient_max * m.units.size() * 4));
	HIP_TRY(up.alloc((void**)&m.d_path2, (size_t)m.n_orient_max * n * 4));
	HIP_TRY(up.alloc((void**)&m.d_trans2, (size_t)m.n_orient_max * n * 4));
	HIP_TRY(up.alloc((void**)&m.d_sel, m.units.size() + 16));
	HIP_TRY(up.alloc((void**)&m.d_guess, m.chunks.size() * 4));
	if (m.preview.spec_keys && m.preview.spec_bytes >= ((size_t)m.n_spec + 1) * stride * 8) m.dp.spec_keys = m.preview.spec_keys;   // (armed, and being written by the preview's launches)
	else HIP_TRY(up.alloc((void**)&m.dp.spec_keys, ((size_t)m.n_spec + 1) * stride * 8));
	return WHAMD_OK;
}

// The units' device copy, the LDS sizes of the two backtrace kernels, the runs' table block, the backtrace arena (b.bt bytes: from the arena cache, else from the
// driver), key scratch, the two exchange buffers of lane 0 and the pinned block a solve downloads into.
whamd_status_t DeviceTable::Impl::take_solve_buffers(const Problem& p, TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	HIP_TRY(up.up((void**)&m.d_units, m.units.data(), m.units.size() * sizeof(BtUnit)));
	{
		uint32_t max_stage = 0;
		for (const ResSegment& sgm : m.plan.segments) max_stage = std::max(max_stage, sgm.stage_words);
		for (size_t ri = 0; ri < m.splan.runs.size(); ++ri)
			max_stage = std::max(max_stage, b.ped_slots ? m.splan.pextra[ri].rec_words / 2u : (m.splan.runs[ri].n_ends * m.splan.runs[ri].threads + 7) / 8);
		m.bt_lds = (size_t)2 * RES_MAXCOLS * 128 + 512 + 16 + (size_t)BT_CELLS * 4 + (size_t)RES_MAXCOLS * 4 + (size_t)max_stage * 8 + 16;
		m.chunk_lds = (size_t)(32 + 4 + BT_CELLS + BT_CHUNK_BLOB) * 4 + (size_t)max_stage * 8 + 16;
	}
	void* d_rtab = nullptr;
	const bool ped_plan = !m.plan.ped_columns.empty();
	HIP_TRY(up.alloc(&d_rtab, m.plan.columns.size() * (ped_plan ? PED_TABLE : RES_TABLE) * sizeof(int32_t)));
	m.dp.res_tables = ped_plan ? nullptr : (int32_t*)d_rtab;
	m.dp.ped_tables = ped_plan ? (int32_t*)d_rtab : nullptr;
	b.laps.lap("jobs, backtrace units, schedule");
	b.laps.next_stage();
	{
		if (m.d_arena && m.arena_bytes < std::max<size_t>(b.bt, 16)) {   // the preview took an arena that turns out too small: its launches are given up
			HIP_TRY(hipStreamSynchronize(m.stream));
			arena_give(m.device, m.d_arena, m.arena_bytes);
			m.d_arena = nullptr;
			m.arena_bytes = 0;
		}
		if (!m.d_arena) {   // (else: the arena the preview's launches are writing their records into)
			size_t got = 0;
			void* d_bt = arena_take(m.device, b.bt, got);
			if (!d_bt) {
				HIP_TRY(hipMalloc(&d_bt, std::max<size_t>(b.bt, 16)));
				got = std::max<size_t>(b.bt, 16);
			}
			m.d_arena = d_bt;
			m.arena_bytes = got;
		}
		m.dp.bt = (uint8_t*)m.d_arena;
	}
	b.laps.next_stage();
	m.key_entries = (size_t)(1ull << b.max_keys_f) * p.T;
	HIP_TRY(up.alloc((void**)&m.dp.keys, m.key_entries * 8));
	HIP_TRY(up.alloc((void**)&m.dp.last_keys, (size_t)MAX_T_WIDE * 8));
	if (m.preview.d_pr[0] && m.preview.exchange_bytes >= b.exchange_bytes) {   // (the exchange columns the preview's launches are handing each other)
		m.d_pr[0] = m.preview.d_pr[0];
		m.d_pr[1] = m.preview.d_pr[1];
	} else {
		HIP_TRY(up.alloc((void**)&m.d_pr[0], b.exchange_bytes));
		HIP_TRY(up.alloc((void**)&m.d_pr[1], b.exchange_bytes));
	}
	HIP_TRY(pinned_take((m.super_off + (m.device_superreads ? m.super_words : 0)) * sizeof(uint32_t), (void**)&m.h_pinned, &m.h_pinned_bytes));
	return WHAMD_OK;
}

// Lanes: longest job first to the least loaded lane; lane 0 always runs the final job.  Every lane but the first gets exchange buffers and key scratch of its own.
whamd_status_t DeviceTable::Impl::make_lanes(const TableBuild& b, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	// at most 1 GiB of private exchange buffers (coverage 23: 64 MiB per lane)
	const size_t lane_bytes = 2 * b.exchange_bytes;
	const size_t by_memory = std::max<size_t>(1, ((size_t)1 << 30) / std::max<size_t>(lane_bytes, 1));
	const size_t n_lanes = std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)m.max_lanes, by_memory), m.jobs.size()));
	m.lanes.assign(n_lanes, Impl::Lane());
	std::vector<uint64_t> load(n_lanes, 0);
	std::vector<uint32_t> order;
	for (uint32_t j = 1; j < m.jobs.size(); ++j) order.push_back(j);
	std::stable_sort(order.begin(), order.end(), [&m](uint32_t x, uint32_t y) { return m.jobs[x].steps.size() > m.jobs[y].steps.size(); });
	m.lanes[0].jobs.push_back(0);
	load[0] = m.jobs[0].steps.size() + 1;
	for (uint32_t j : order) {
		const size_t l = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
		m.lanes[l].jobs.push_back(j);
		load[l] += m.jobs[j].steps.size() + 1;
	}
	m.lanes[0].d_pr[0] = m.d_pr[0];
	m.lanes[0].d_pr[1] = m.d_pr[1];
	m.lanes[0].d_keys = m.dp.keys;
	for (size_t l = 1; l < n_lanes; ++l) {
		HIP_TRY(up.alloc((void**)&m.lanes[l].d_pr[0], b.exchange_bytes));
		HIP_TRY(up.alloc((void**)&m.lanes[l].d_pr[1], b.exchange_bytes));
		HIP_TRY(up.alloc((void**)&m.lanes[l].d_keys, m.key_entries * 8));
	}
	return WHAMD_OK;
}

// The schedule: the lanes advance in lockstep; super-step t holds step t of every lane that still has one.  Makes the entries of the batched launches
// (m.entries / m.slot_entries: they carry the device pointers of everything above) and, windowed, the replay of every older window.  Host only.
whamd_status_t DeviceTable::Impl::make_schedule(const TableBuild& b, std::string& msg) {
	Impl& m = *this;
	const bool ped_slots = b.ped_slots;
	struct Cursor { size_t job_i = 0, step_i = 0; uint32_t flip = 0; };
	std::vector<Cursor> cur(m.lanes.size());
	for (;;) {
		Impl::SuperStep ss;
		ss.entry_off = (uint32_t)(m.use_slots ? m.slot_entries.size() : m.entries.size());
		for (size_t li = 0; li < m.lanes.size(); ++li) {
			Impl::Lane& lane = m.lanes[li];
			Cursor& c = cur[li];
			if (c.job_i == lane.jobs.size()) continue;
			const uint32_t job_id = lane.jobs[c.job_i];
			const Impl::Job& job = m.jobs[job_id];
			const uint32_t si = job.steps[c.step_i];
			const bool first = c.step_i == 0, last = c.step_i + 1 == job.steps.size();
			const Step& step = m.plan.steps[si];
			ss.io[0] = lane.d_pr[c.flip]; ss.io[1] = lane.d_pr[c.flip ^ 1];
			if (step.kind == 2) {
				SlotBatchEntry e{};
				e.run = m.splan.runs[step.index];
				if (first) e.run.has_prev = 0;  // a job starts from cost 0
				e.prev = lane.d_pr[c.flip];
				e.cur = lane.d_pr[c.flip ^ 1];
				e.score_out = (last && !job.final) ? m.d_job_scores + job_id : nullptr;
				if (m.splan.ped) {
					const PedSlotExtra& pex = m.splan.pextra[step.index];
					ss.lds = std::max<size_t>(ss.lds, pedslot_lds_bytes(e.run.threads, e.run.ncols, pex));
				} else
				ss.lds = std::max<size_t>(ss.lds, slot_run_lds_bytes(e.run.threads, e.run.lr, e.run.ncols));
				e.pad = step.index;
				// the owning table's arrays: a group launch (slot_group / pedslot_group) serves runs of several tables
				if (ped_slots) e.ex = m.splan.pextra[step.index];
				e.tab = ped_slots ? m.dp.pslot_tab : m.dp.slot_tab;
				e.rows = ped_slots ? (const void*)m.dp.pslot_rows : (const void*)m.dp.slot_rows;
				e.ctrl = m.dp.slot_ctrl;
				e.bt = m.dp.bt;
				e.spec_keys = m.dp.spec_keys;
				e.spec_stride = m.dp.spec_stride;
				if (const char* skip = debug_env("WHAMD_SLOT_SKIP")) e.pad2 = (uint32_t)atoi(skip);   // (timing experiments in a group launch)
				if (debug_env("WHAMD_NO_WARM")) e.pad2 |= 0x10000u;
				ss.grid_x = std::max(ss.grid_x, 1u << (e.run.g - e.run.half));
				ss.threads = std::max(ss.threads, e.run.threads);
				m.slot_entries.push_back(e);
				++ss.entry_count;
			} else if (step.kind == 1) {
				ResBatchEntry e{};
				e.sg = m.plan.segments[step.index];
				e.sg.pad = step.index;
				if (first) e.sg.has_prev = 0;  // a job starts from cost 0
				e.prev = lane.d_pr[c.flip];
				e.cur = lane.d_pr[c.flip ^ 1];
				e.score_out = (last && !job.final) ? m.d_job_scores + job_id : nullptr;
				const size_t lds = e.sg.kind == 1
					? ((((size_t)e.sg.ncols * (PED_LDSWORDS + PED_TABLE) + (size_t)e.sg.n_terms * 2 + 3) & ~(size_t)3) * 4 + 2 * ((size_t)16 << e.sg.max_l) + (size_t)e.sg.stage_words * 8)
					: ((size_t)e.sg.ncols * (64 + RES_TABLE) * 4 + 2 * ((size_t)4 << e.sg.max_l) + (size_t)e.sg.stage_words * 8);
				ss.lds = std::max(ss.lds, lds);
				ss.grid_x = std::max(ss.grid_x, 1u << (e.sg.g - e.sg.half));
				ss.threads = std::max(ss.threads, e.sg.threads);
				ss.sym = ss.sym || e.sg.half || e.sg.in_half || e.sg.mirror_out;
				m.entries.push_back(e);
				++ss.entry_count;
			} else {
				ss.singles.push_back(Impl::Single{(uint32_t)li, si, c.flip, first, (last && !job.final) ? (int32_t)job_id : -1});
			}
			c.flip ^= 1;
			if (last) { ++c.job_i; c.step_i = 0; } else ++c.step_i;
		}
		if (!ss.entry_count && ss.singles.empty()) break;
		m.max_grid_x = std::max(m.max_grid_x, ss.grid_x * std::max(1u, ss.entry_count));
		m.schedule.push_back(std::move(ss));
	}
	if (m.windowed) {
		// one lane, one job: super-step i is step i.  Pass 1 = the schedule as it is, plus the kept columns and the
		// walk of the newest window; then every older window again, newest first.
		if (m.schedule.size() != m.jobs[0].steps.size()) { msg = "internal error: windowed schedule"; return WHAMD_ERR_DEVICE; }
		const size_t nw = m.windows.size();
		for (size_t wi = 0; wi + 1 < nw; ++wi) m.schedule[m.windows[wi].step_hi - 1].ck_save = (int32_t)wi;
		m.schedule.back().bt_window = (int32_t)(nw - 1);
		for (size_t wi = nw - 1; wi-- > 0;) {
			const Impl::Window& win = m.windows[wi];
			for (uint32_t pos = win.step_lo; pos < win.step_hi; ++pos) {
				Impl::SuperStep again = m.schedule[pos];
				again.ck_save = -1;
				again.ck_load = (pos == win.step_lo && wi > 0) ? (int32_t)(wi - 1) : -1;
				again.bt_window = pos + 1 == win.step_hi ? (int32_t)wi : -1;
				m.schedule.push_back(std::move(again));
			}
		}
	}
	return WHAMD_OK;
}

// What a group submission reads of the schedule (see StepBrief / EntryBrief).  Host only.
void DeviceTable::Impl::make_briefs() {
	Impl& m = *this;
	m.step_brief.clear();
	m.entry_brief.clear();
	if (!m.use_slots) return;
	m.step_brief.reserve(m.schedule.size());
	m.entry_brief.reserve(m.slot_entries.size());
	for (const Impl::SuperStep& ss : m.schedule) {
		m.step_brief.push_back(Impl::StepBrief{(uint32_t)m.entry_brief.size(), (uint32_t)ss.lds, (uint16_t)ss.entry_count, (uint8_t)(ss.singles.empty() ? 0 : 1), 0});
		for (uint32_t q = 0; q < ss.entry_count; ++q) {
			const SlotBatchEntry& he = m.slot_entries[ss.entry_off + q];
			Impl::EntryBrief eb{};
			eb.grid_x = (uint16_t)(1u << (he.run.g - he.run.half));
			eb.threads = (uint16_t)he.run.threads;
			eb.lds_x = (uint32_t)((size_t)2 * he.run.threads * (4u << he.run.lr));
			eb.variant = group_variants_of(he, m.splan.ped);
			m.entry_brief.push_back(eb);
		}
	}
}

// The entries of the batched launches and the backtrace jobs: the last arrays of the image.
whamd_status_t DeviceTable::Impl::upload_entries(TableUploader& up, std::string& msg) {
	Impl& m = *this;
	HIP_TRY(up.up((void**)&m.d_entries, m.entries.data(), m.entries.size() * sizeof(ResBatchEntry)));
	m.slot_entries.resize(m.slot_entries.size() + 2);   // (two unused entries behind the last: a group launch warms 512 bytes behind its own entry, slot_runx_core)
	HIP_TRY(up.up((void**)&m.d_slot_entries, m.slot_entries.data(), m.slot_entries.size() * sizeof(SlotBatchEntry)));
	m.slot_entries.resize(m.slot_entries.size() - 2);
	std::vector<BtJob> btjobs;
	for (const Impl::Job& job : m.jobs) btjobs.push_back(BtJob{job.unit_off, job.unit_count, job.final ? 1u : 0u, 0u});
	HIP_TRY(up.up((void**)&m.d_btjobs, btjobs.data(), btjobs.size() * sizeof(BtJob)));
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
		for (size_t ri = 0; ri < m.splan.runs.size(); ++ri)
			most = std::max<uint32_t>(most, (m.splan.pextra[ri].fwn << m.splan.runs[ri].g) + (m.splan.pextra[ri].fwn << m.splan.runs[ri].lw) + m.splan.runs[ri].ncols * (64u * pslot_ns(m.splan.pextra[ri].nf) + p.T * pslot_nk(m.splan.pextra[ri].nf)));
		const uint32_t bx = std::max(1u, std::min(1024u, (most + 255u) / 256u));
		for (size_t r0 = 0; r0 < m.splan.runs.size(); r0 += 32768) {   // (gridDim.y <= 65535)
			const uint32_t ny = (uint32_t)std::min<size_t>(32768, m.splan.runs.size() - r0);
			hipLaunchKernelGGL(pedslot_tables, dim3(bx, ny), dim3(256), 0, us, m.dp, b.d_runs + r0, b.d_pextra + r0, (uint32_t*)m.dp.pslot_tab, b.d_fterms);
		}
		HIP_TRY(hipGetLastError());
	}
	if (m.use_slots && !b.ped_slots && !m.splan.runs.empty()) {
		uint32_t most = 0;
		for (const SlotRun& run : m.splan.runs) most = std::max<uint32_t>(most, ((run.ncols + 8u) << (run.g - run.half)) + (run.ncols + 8u) * ((run.threads >> 6) + 64u));
		const uint32_t bx = std::max(1u, std::min(64u, (most + 255u) / 256u));
		for (size_t r0 = 0; r0 < m.splan.runs.size(); r0 += 32768) {
			const uint32_t ny = (uint32_t)std::min<size_t>(32768, m.splan.runs.size() - r0);
			hipLaunchKernelGGL(slot_tables, dim3(bx, ny), dim3(256), 0, us, m.dp, b.d_runs + r0, (uint32_t*)m.dp.slot_tab);
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

// The in-kernel cycle stamps and timing experiments of the debug library (m.dp.dbg, dbg_wg_off, dbg_flags).
whamd_status_t DeviceTable::Impl::arm_debug_stamps(TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.dp.dbg = nullptr;
	if (debug_env("WHAMD_DEBUG_STAMPS") && !m.use_slots) {   // in-kernel cycle stamps of the LDS-resident runs (WHAMD_DEBUG_TIMING: host phases only)
		const size_t dbg_bytes = (m.plan.segments.size() + 1) * 64 + 4 * 512 * 16 + 64;
		HIP_TRY(up.alloc((void**)&m.dp.dbg, dbg_bytes));
		HIP_TRY(hipMemset(m.dp.dbg, 0, dbg_bytes));
		m.dp.dbg_wg_off = (uint32_t)((m.plan.segments.size() + 1) * 8);
		m.dp.dbg_flags = (uint32_t)atoi(debug_env("WHAMD_DEBUG_STAMPS"));
	}
	if (debug_env("WHAMD_SLOT_STAMPS") && m.use_slots) {   // in-kernel cycle stamps of workgroup 0 / wave 0 of every slot run
		const size_t dbg_bytes = (m.splan.runs.size() + 1) * 48 * 8 + 4 * 512 * 16 + 128;   // + the backtrace kernel's own stamps
		HIP_TRY(up.alloc((void**)&m.dp.dbg, dbg_bytes));
		HIP_TRY(hipMemset(m.dp.dbg, 0, dbg_bytes));
		m.dp.dbg_wg_off = (uint32_t)((m.splan.runs.size() + 1) * 48);
		for (size_t i = 0; i < m.slot_entries.size(); ++i) m.slot_entries[i].run.pad = (uint32_t)i;
	}
	if (const char* skip = debug_env("WHAMD_SLOT_SKIP")) m.dp.dbg_flags = (uint32_t)atoi(skip);  // timing experiments (results invalid): 1 no exit
	                                                                                          // stores, 2 no records, 4 one column per run, 8 no ending reads, 16 no cost update
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
	for (size_t i = 0; i < count; ++i) HIP_TRY(hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
	if (device < 64) attr_done |= 1ull << device;
	return WHAMD_OK;
}

// What a batched backtrace launch reads for this table (BtGroupEntry): a copy of the finished m.dp and the walk's buffers, on the device behind `ev_upload`.
whamd_status_t DeviceTable::Impl::record_group_backtrace(uint32_t n, TableUploader& up, std::string& msg) {
	Impl& m = *this;
	m.d_bt_entry = nullptr;
	if (!m.use_chunks) return WHAMD_OK;
	BtGroupEntry& e = m.h_bt_entry;
	e = BtGroupEntry{};
	e.P = m.dp;
	e.units = m.d_units; e.chunks = m.d_chunks;
	e.n_chunks = (uint32_t)m.chunks.size(); e.n_units = (uint32_t)m.units.size(); e.n_orient_max = m.n_orient_max; e.n_cols = n;
	e.path2 = m.d_path2; e.trans2 = m.d_trans2; e.out_score = m.d_score; e.unit_x2 = m.d_unit_x; e.guess = m.d_guess; e.sel = m.d_sel; e.counters = m.d_bt_counters;
	e.path_index = m.d_path_index; e.path_trans = m.d_path_trans;
	if (m.device_superreads) e.super = m.super_args;
	void* d_entry = nullptr;
	HIP_TRY(up.alloc(&d_entry, sizeof(BtGroupEntry)));
	HIP_TRY(hipMemcpyAsync(d_entry, &m.h_bt_entry, sizeof(BtGroupEntry), hipMemcpyHostToDevice, up.stream));   // (the source is a member: it outlives the copy)
	HIP_TRY(hipEventRecord(m.ev_upload, up.stream));
	m.d_bt_entry = (BtGroupEntry*)d_entry;
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- the preview
// Which steps a preview would launch and what each is given by value, worked out ahead of the phases that normally produce it.  Host only (the debug library's
// whamd_debug_preview_plan holds it against lay_out_arena and cut_chunks without a device).  out.why says whether there is one: the table's form, the options,
// and -- under `auto` -- that the table is alone.  The record offsets are the sum lay_out_arena will make, from its own helpers; the seeds' ids come from the
// chunk rule make_chunks walks (cut_chunk_starts), here over the plan's steps.
void DeviceTable::Impl::plan_preview(const Problem& p, const TableBuild& b, bool from_create, PreviewPlan& out) {
	Impl& m = *this;
	const Preview& pv = m.preview;
	const uint32_t n = b.n, n_pieces = slot_plan_pieces(n);
	out = PreviewPlan();
	auto none = [&out](uint32_t why) { out.why = why; };
	if (pv.mode == 0 || debug_env("WHAMD_NO_PREVIEW")) return none(PV_OFF);
	if (!from_create) return none(PV_NOT_CREATE);
	if (!m.use_slots || m.splan.ped || p.T != 1) return none(PV_NOT_SLOTS);
	if (debug_env("WHAMD_DEBUG_STAMPS") || debug_env("WHAMD_SLOT_STAMPS") || debug_env("WHAMD_SLOT_SKIP")) return none(PV_DEBUG_SWITCH);
	if (m.shared_hint || m.side_by_side) return none(PV_SHARED);
	if (m.plan.component_first_step.size() != 1) return none(PV_COMPONENTS);
	if (n_pieces < 2) return none(PV_FEW_PIECES);
	if (pv.mode < 0) {   // auto: only where a speculative forward pass competes with nothing
		if (pv.thread_budget) return none(PV_THREAD_BUDGET);
		if (n_pieces < 8) return none(PV_FEW_PIECES);
		if (m.device < 0 || m.device >= 64 || Impl::tables_on_device[m.device].load() != 1) return none(PV_NOT_ALONE);
	}
	out.pieces = std::min(n_pieces - 1, preview_pieces_of(pv.pieces_wanted, n_pieces));
	const uint32_t col_limit = slot_plan_piece_begin(n, out.pieces);
	// ---- the leading steps that are slot runs inside the pieces (a piece edge is a run boundary)
	const std::vector<Step>& steps = m.plan.steps;
	const std::vector<SlotRun>& runs = m.splan.runs;
	uint32_t S = 0;
	while (S < steps.size() && steps[S].kind == 2 && steps[S].index == S && runs[S].c0 + runs[S].ncols <= col_limit) ++S;
	if (S == 0 || S >= steps.size()) return none(PV_NO_LEADING_RUNS);
	out.end_col = runs[S - 1].c0 + runs[S - 1].ncols;
	if ((size_t)out.end_col + SLOT_ROW_PAD > m.splan.rows.size()) return none(PV_ROW_PAD);   // (a run's scalar-cache warm-up touches a fixed number of rows behind its own)
	// ---- what the runs carry by value: table offsets, record offsets, the ids of the seeds they leave
	const uint64_t tab_words_all = m.lay_out_slot_tables(b, false);
	out.tab_words = (S < runs.size() ? runs[S].tab_g : tab_words_all) + (uint64_t)SLOT_XCOLS * 64u;   // (lay_out_slot_tables: the slack an X run may request)
	out.ctrl_words = (size_t)runs[S - 1].ctrl_off + SLOT_CTRL_WORDS;
	if (tab_words_all >= 0xFFFFFFFFull || out.ctrl_words > m.splan.ctrl.size()) return none(PV_NO_LEADING_RUNS);
	out.rec.assign(S, 0);
	uint64_t bt = 0;
	{
		// the records of ALL steps, in order, as lay_out_arena places them when they fit one window (arena_capacity, arena_behind, the record sizes: its own)
		const uint64_t cap = arena_capacity(b.free_b, n, m.table_bytes, m.arena_limit);
		for (size_t k = 0; k < steps.size(); ++k) {
			uint64_t bytes = 0;
			if (steps[k].kind == 2) bytes = slot_run_record_bytes(runs[steps[k].index]);
			else {
				const uint32_t c = steps[k].index, f = p.f[c], ebits = p.k[c] - f;
				bytes = column_record_bytes(column_step_mode(b.force_keys, c + 1 == n, f, ebits), p.T, f, ebits + b.tbits);
			}
			if (bt + bytes + 16 > cap) return none(PV_ARENA);   // (windowed, or too large altogether)
			if (k < S) out.rec[k] = bt;
			bt = arena_behind(bt, bytes);
		}
		if (bt + (1ull << 31) > b.free_b) return none(PV_ARENA);
	}
	out.arena = bt;
	out.spec.assign(S, 0);
	out.stride = 64;
	out.chunked = backtrace_is_chunked(true, 1, false, steps.size());   // (one job of slot runs, not windowed: checked above)
	if (out.chunked)
		out.n_spec = cut_chunk_starts(steps.size(), [&steps](size_t u) { return steps[steps.size() - 1 - u].kind == 2; },
			[&](size_t u, uint32_t id) {
				const size_t k = steps.size() - 1 - u;
				out.stride = seed_stride_of(out.stride, runs[steps[k].index]);
				if (k < S) out.spec[k] = id;
			});
	out.max_f = p.max_k;   // (a bound of the widest exchange column: no column forwards more reads than it has, a run's entries are 2^(L + g))
	for (const SlotRun& run : runs) out.max_f = std::max(out.max_f, run.L + run.g);
	out.steps = S;
	out.why = PV_RAN;
}

// A lone single-individual table's device sits idle through its whole create, and nothing of the create's second half -- column descriptors, the arena's layout,
// staging and sending ~100 MB, backtrace units, schedule -- is needed by the FIRST launches, which read the rows, control words and tables of their own
// columns only.  Right behind the plan this function therefore uploads exactly that for the runs plan_preview chose (a prefix of the arrays the table will
// upload whole: every offset a run carries is the same in both), takes the buffers the solve will write -- arena, exchange columns, seeds -- and launches those
// runs on the table's own stream, with an event behind the last.  Nothing plan_preview worked out is trusted: verify_preview holds the finished schedule against it.
whamd_status_t DeviceTable::Impl::start_preview(const Problem& p, TableBuild& b, bool from_create, std::string& msg) {
	Impl& m = *this;
	Preview& pv = m.preview;
	PreviewPlan pp;
	m.plan_preview(p, b, from_create, pp);
	pv.why = pp.why;
	if (pp.why != PV_RAN) return WHAMD_OK;
	const uint32_t n = b.n, S = pp.steps, pieces = pp.pieces, end_col = pp.end_col, n_spec = pp.n_spec, stride = pp.stride, max_f = pp.max_f;
	const uint64_t bt = pp.arena, tab_words = pp.tab_words;
	const size_t ctrl_words = pp.ctrl_words;
	const bool chunked = pp.chunked;
	const std::vector<uint64_t>& rec = pp.rec;
	const std::vector<uint32_t>& spec = pp.spec;
	const std::vector<SlotRun>& runs = m.splan.runs;
	b.laps.lap("preview: steps, offsets, seeds (host)");
	// ---- the buffers the solve writes: the table's from here on
	auto take = [&m](void** out, size_t bytes) {
		size_t got = 0;
		const hipError_t e = devpool_take(m.device, std::max<size_t>(bytes, 16), out, &got);
		if (e == hipSuccess) m.allocations.emplace_back(*out, got);
		return e;
	};
	{
		size_t got = 0;
		void* d_bt = arena_take(m.device, bt, got);
		if (!d_bt) {
			HIP_TRY(hipMalloc(&d_bt, std::max<size_t>(bt, 16)));
			got = std::max<size_t>(bt, 16);
		}
		m.d_arena = d_bt;
		m.arena_bytes = got;
	}
	pv.exchange_bytes = (size_t)(1ull << max_f) * p.T * 4;
	HIP_TRY(take((void**)&pv.d_pr[0], pv.exchange_bytes));
	HIP_TRY(take((void**)&pv.d_pr[1], pv.exchange_bytes));
	pv.spec_bytes = chunked ? ((size_t)n_spec + 1) * stride * 8 : 0;
	if (chunked) HIP_TRY(take((void**)&pv.spec_keys, pv.spec_bytes));
	// ---- the preview's own arrays: a prefix of the table's rows, control words and runs; its tables
	DevProblem hdp{};
	hdp.n_cols = n; hdp.T = p.T; hdp.tbits = b.tbits; hdp.n_ind = p.n_ind;
	{
		const hipStream_t us = m.upload_stream;
		TableUploader up(m.device, us, pv.allocations);
		const size_t row_count = (size_t)end_col + SLOT_ROW_PAD;
		up.open_block(row_count * sizeof(SlotRow) + ctrl_words * 4 + (size_t)S * sizeof(SlotRun) + 4096);
		const SlotRun* d_runs = nullptr;
		HIP_TRY(up.up((void**)&hdp.slot_rows, m.splan.rows.data(), row_count * sizeof(SlotRow)));
		HIP_TRY(up.up((void**)&hdp.slot_ctrl, m.splan.ctrl.data(), ctrl_words * 4));
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
	hdp.bt = (uint8_t*)m.d_arena;
	hdp.spec_keys = pv.spec_keys;
	hdp.spec_stride = stride;
	if (chunked) HIP_TRY(hipMemsetAsync(pv.spec_keys, 0xFF, pv.spec_bytes, rs));
	m.inflight.timing_pending = false;   // (the events are the coming solve's from here on)
	HIP_TRY(hipEventRecord(m.ev0, rs));
	m.use_chunks = chunked;   // (launch_slot_run: a run leaves a seed where the backtrace is chunked)
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
	const bool same_ground = m.use_slots && !m.windowed && m.jobs.size() == 1 && m.lanes.size() == 1 && m.dp.bt == pv.dp.bt && m.dp.spec_keys == pv.dp.spec_keys &&
	                         m.use_chunks == pv.use_chunks && (!m.use_chunks || m.dp.spec_stride == pv.dp.spec_stride) && !m.dp.dbg && !m.dp.dbg_flags &&
	                         m.d_pr[0] == pv.d_pr[0] && m.d_pr[1] == pv.d_pr[1] && !m.side_by_side;
	for (uint32_t k = 0; same_ground && k < pv.launched && k + 1 < m.schedule.size(); ++k) {
		const Impl::SuperStep& ss = m.schedule[k];
		if (ss.entry_count != 1 || !ss.singles.empty() || ss.ck_load >= 0 || ss.ck_save >= 0 || ss.bt_window >= 0) break;
		const SlotBatchEntry& e = m.slot_entries[ss.entry_off];
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
	m.dp.n_cols = b.n;
	m.dp.T = p.T;
	m.dp.tbits = b.tbits;
	m.dp.n_ind = p.n_ind;
	// ---- everything this function sends or launches goes through one of the device's upload streams (upload_stream_of); begin_solve orders the solve behind
	// ev_upload.  WHAMD_UPLOAD_ON_TABLE_STREAM=1 (debug library): the table's own stream, as before.  (Chosen in front of the plan: a preview may start inside it.)
	m.upload_stream = debug_env("WHAMD_UPLOAD_ON_TABLE_STREAM") ? nullptr : upload_stream_of(device);
	if (!m.upload_stream) m.upload_stream = m.stream;
	if (m.upload_stream == m.stream) m.own_stream_used = true;
	// ---- host: path and plan, column descriptors, the layout of the backtrace arena
	if ((st = m.choose_plan(p, b, from_create, msg)) != WHAMD_OK) return st;
	b.ped_slots = m.use_slots && m.splan.ped;
	b.laps.next_stage();
	if (debug_env("WHAMD_DEBUG_PLAN")) m.dump_plan(p);
	// ---- a lone table: its first runs start on the device -- from inside the planner (choose_plan's head hook), or here --, and the rest of the create happens under them
	if (!m.preview.tried && (st = m.start_preview(p, b, from_create, msg)) != WHAMD_OK) return st;
	if ((st = m.describe_columns(p, b, msg)) != WHAMD_OK) return st;
	if ((st = m.lay_out_arena(p, b, msg)) != WHAMD_OK) return st;
	TableUploader up(device, m.upload_stream, m.allocations);
	b.laps.lap("staging area taken");
	up.open_block(m.upload_bound(p, b));
	b.laps.lap("staging image sized, device block taken");
	// ---- the device block fills in this order; the image leaves in pieces of 32 MB
	if ((st = m.upload_column_arrays(p, b, up, msg)) != WHAMD_OK) return st;
	if ((st = m.upload_slot_arrays(b, up, msg)) != WHAMD_OK) return st;
	m.make_jobs();
	m.make_units(b);
	if ((st = m.make_windows(b, up, msg)) != WHAMD_OK) return st;
	if ((st = m.take_result_block(b.n, up, msg)) != WHAMD_OK) return st;
	if ((st = m.make_chunks(p, up, msg)) != WHAMD_OK) return st;
	if ((st = m.take_solve_buffers(p, b, up, msg)) != WHAMD_OK) return st;
	if ((st = m.make_lanes(b, up, msg)) != WHAMD_OK) return st;
	if ((st = m.make_schedule(b, msg)) != WHAMD_OK) return st;
	m.make_briefs();
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
	DevProblem dp = m.dp;
	dp.keys = lane.d_keys;
	const uint32_t c = step.index;
	const DevColumn& d = m.cols[c];
#ifdef WHAMD_DEBUG_BUILD
	const auto column_facts = [&m](const Problem& pr, const DevColumn& col) { LaunchFacts f; f.T = (int32_t)pr.T; f.n_ind = (int32_t)m.dp.n_ind; f.mode = (int32_t)col.mode; f.wide = m.wide; return f; };
#endif
	if (d.mode == 0) {
		const uint32_t threads = 1u << d.f;
		const uint32_t block = std::min<uint32_t>(256, threads);
		hipLaunchKernelGGL(m.fused, dim3(threads / block), dim3(block), 0, rs, dp, c, prev, cur);
		WHAMD_NOTE(m, WHAMD_LAUNCH_COLUMN, (const void*)m.fused, dim3(threads / block), dim3(block), 0, rs, true, column_facts(p, d));
		launches += 1;
	} else {
		const uint64_t total = (1ull << (d.f + d.ebits - d.eloop)) * (m.wide ? p.T : 1u);
		const uint32_t block = (uint32_t)std::min<uint64_t>(256, (total + 63) / 64 * 64);
		if (m.wide) hipLaunchKernelGGL(column_step_wide, dim3((uint32_t)((total + block - 1) / block)), dim3(block), 0, rs, dp, c, prev, (uint32_t)total);
		else hipLaunchKernelGGL(m.keysfn, dim3((uint32_t)((total + block - 1) / block)), dim3(block), 0, rs, dp, c, prev, (uint32_t)total);
		WHAMD_NOTE(m, WHAMD_LAUNCH_COLUMN, m.wide ? (const void*)column_step_wide : (const void*)m.keysfn, dim3((uint32_t)((total + block - 1) / block)), dim3(block), 0, rs, true, column_facts(p, d));
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
	const bool stamps = DEBUG_BUILD && m.dp.dbg != nullptr;
#ifdef WHAMD_DEBUG_BUILD
	const auto segment_facts = [&sg, stamps](bool spec, bool sym) {
		LaunchFacts f;
		f.ped = sg.kind == 1; f.stamps = stamps; f.ncols = (int32_t)sg.ncols; f.threads = (int32_t)sg.threads;
		if (sg.kind == 1) f.spec = spec; else f.sym = sym;
		return f;
	};
#endif
	if (sg.kind == 1) {
		const size_t words = ((size_t)sg.ncols * (PED_LDSWORDS + PED_TABLE) + (size_t)sg.n_terms * 2 + 3) & ~(size_t)3;
		const size_t lds_ped = words * 4 + 2 * ((size_t)16 << sg.max_l) + (size_t)sg.stage_words * 8;
		const PedSegmentFn kernel = ped_segment_kernel(stamps, sg.in_mirror_bit && m.use_chunks);
		hipLaunchKernelGGL(kernel, dim3(1u << sg.g), dim3(sg.threads), lds_ped, rs, m.dp, sg, e.prev, e.cur);
		WHAMD_NOTE(m, WHAMD_LAUNCH_RUN, (const void*)kernel, dim3(1u << sg.g), dim3(sg.threads), lds_ped, rs, true, segment_facts(sg.in_mirror_bit && m.use_chunks, false));
	} else {
		const size_t lds = (size_t)sg.ncols * (64 + RES_TABLE) * 4 + 2 * ((size_t)4 << sg.max_l) + (size_t)sg.stage_words * 8;
		const SegmentFn kernel = segment_kernel(stamps, sg.half || sg.in_half || sg.mirror_out);
		hipLaunchKernelGGL(kernel, dim3(1u << (sg.g - sg.half)), dim3(sg.threads), lds, rs, m.dp, sg, e.prev, e.cur, e.score_out);
		WHAMD_NOTE(m, WHAMD_LAUNCH_RUN, (const void*)kernel, dim3(1u << (sg.g - sg.half)), dim3(sg.threads), lds, rs, true, segment_facts(false, sg.half || sg.in_half || sg.mirror_out));
	}
	launches += 1;
}

// One slot run as a launch of its own (kernel arguments by value); `dp`: the table's problem, or the preview's with arrays of its own.
void DeviceTable::Impl::launch_slot_run(const DevProblem& dp, const SlotBatchEntry& e, uint64_t& launches) {
	Impl& m = *this;
	const SlotRun& run = e.run;
	const hipStream_t rs = m.inflight.run_stream;
	const bool spec = run.spec_id != 0 && m.use_chunks && !debug_env("WHAMD_NO_SPEC_KERNEL");
	const bool stamps = DEBUG_BUILD && (dp.dbg != nullptr || dp.dbg_flags != 0);
	launches += 1;
	if (m.splan.ped) {
		const PedSlotExtra& ex = m.splan.pextra[e.pad];
		size_t lds = pedslot_lds_bytes(run.threads, run.ncols, ex);
		PedSlotRunFn kernel = pedslot_run_kernel(ex.tb, ex.nf, spec, (run.yflags & 16u) != 0);
#ifdef WHAMD_DEBUG_BUILD
		if ((run.yflags & 8u) && !m.side_by_side) {   // X run (WHAMD_PED_XRUN=1)
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
		const bool streamed = m.side_by_side || debug_env("WHAMD_XSTREAM") || (grid.x >= 1024u && !debug_env("WHAMD_NO_WIDE_LAYOUT"));
		const size_t lds_x = streamed ? (size_t)2 * run.threads * 16 : slotx_lds_bytes(run.threads, (run.ncols + 7u) & ~7u);
		// narrow tables: the run's workgroups packed onto one XCD (slot_runx: eight times the grid, every eighth workgroup works)
		const uint32_t pack = (grid.x <= 32u && !m.side_by_side && !debug_env("WHAMD_NO_XCD_PACK")) ? 1u : 0u;
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
	for (const Impl::Lane& lane : m.lanes) HIP_TRY(hipMemsetAsync(lane.d_keys, 0xFF, m.key_entries * 8, rs));
	HIP_TRY(hipMemsetAsync(m.dp.last_keys, 0xFF, (size_t)MAX_T_WIDE * 8, rs));
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
	if (m.use_chunks) HIP_TRY(hipMemsetAsync(m.dp.spec_keys, 0xFF, ((size_t)m.n_spec + 1) * m.dp.spec_stride * 8, rs));
	if (m.windowed) HIP_TRY(hipMemsetAsync(m.d_path_trans, 0, (size_t)n * 4, rs));
	m.inflight.timing_pending = false;   // (the events are this solve's from here on)
	HIP_TRY(hipEventRecord(m.ev0, rs));
	if (!m.plan.ped_columns.empty()) {
		const uint32_t entries = (uint32_t)m.plan.ped_columns.size() * PED_TABLE;
		hipLaunchKernelGGL(ped_tables, dim3((entries + 255) / 256), dim3(256), 0, rs, m.dp.ped_cols, (uint32_t)m.plan.ped_columns.size(), m.dp.ped_tables);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TABLES, (const void*)ped_tables, dim3((entries + 255) / 256), dim3(256), 0, rs, false, LaunchFacts());
	} else if (!m.use_slots && !m.plan.columns.empty()) {
		const uint32_t entries = (uint32_t)m.plan.columns.size() * RES_TABLE;
		hipLaunchKernelGGL(resident_tables, dim3((entries + 255) / 256), dim3(256), 0, rs, m.dp.res_cols, (uint32_t)m.plan.columns.size(), m.dp.res_tables);
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
	if (ss.ck_load >= 0) HIP_TRY(hipMemcpyAsync(ss.io[0], m.d_checkpoints + (size_t)ss.ck_load * m.checkpoint_bytes, m.checkpoint_bytes, hipMemcpyDeviceToDevice, rs));
	if (ss.entry_count == 1) {
		if (m.use_slots) m.launch_slot_run(m.dp, m.slot_entries[ss.entry_off], launches);
		else m.launch_run(m.entries[ss.entry_off], launches);
	} else if (ss.entry_count > 1) {
		if (m.use_slots) { const SlotBatchFn kernel = slot_batch_kernel(m.slot_lr_used); hipLaunchKernelGGL(kernel, grid, block, ss.lds, rs, m.dp, m.d_slot_entries + ss.entry_off); }
		else { const ResBatchFn kernel = resident_batch_kernel(ss.sym); hipLaunchKernelGGL(kernel, grid, block, ss.lds, rs, m.dp, m.d_entries + ss.entry_off); }
#ifdef WHAMD_DEBUG_BUILD
		LaunchFacts facts;
		facts.entries = (int32_t)ss.entry_count;
		if (m.use_slots) facts.lr = m.slot_lr_used; else facts.sym = ss.sym;
		WHAMD_NOTE(m, WHAMD_LAUNCH_BATCH, m.use_slots ? (const void*)slot_batch_kernel(m.slot_lr_used) : (const void*)resident_batch_kernel(ss.sym), grid, block, ss.lds, rs, true, facts);
#endif
		launches += 1;
	}
	const whamd_status_t st = m.submit_singles(p, ss, launches, msg);
	if (st != WHAMD_OK) return st;
	if (ss.ck_save >= 0) HIP_TRY(hipMemcpyAsync(m.d_checkpoints + (size_t)ss.ck_save * m.checkpoint_bytes, ss.io[1], m.checkpoint_bytes, hipMemcpyDeviceToDevice, rs));
	if (ss.bt_window >= 0)
	{
		hipLaunchKernelGGL(backtrace_kernel, dim3(1), dim3(1024), m.bt_lds, rs, m.dp, m.d_units, m.d_window_jobs + ss.bt_window,
		                   m.d_path_index, m.d_path_trans, m.d_score);
		WHAMD_NOTE(m, WHAMD_LAUNCH_WINDOW_WALK, (const void*)backtrace_kernel, dim3(1), dim3(1024), m.bt_lds, rs, false, LaunchFacts());
	}
	return WHAMD_OK;
}

// The per-column steps of one super-step (each a launch of its own on the run stream).
whamd_status_t DeviceTable::Impl::submit_singles(const Problem& p, const SuperStep& ss, uint64_t& launches, std::string& msg) {
	Impl& m = *this;
	const hipStream_t rs = m.inflight.run_stream;
	for (const Impl::Single& sg : ss.singles) {
		const Impl::Lane& lane = m.lanes[sg.lane];
		if (sg.zero_prev) HIP_TRY(hipMemsetAsync(lane.d_pr[sg.flip], 0, 4 * (size_t)p.T, rs));
		m.launch_column_step(p, m.plan.steps[sg.step], lane, lane.d_pr[sg.flip], lane.d_pr[sg.flip ^ 1], launches);
		if (sg.score_job >= 0)
			HIP_TRY(hipMemcpyAsync(m.d_job_scores + sg.score_job, lane.d_pr[sg.flip ^ 1], 4, hipMemcpyDeviceToDevice, rs));
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
	} else if (m.use_chunks) {
		hipLaunchKernelGGL(backtrace_chunks, dim3(m.n_orient_max * (uint32_t)m.chunks.size()), dim3(256), m.chunk_lds, ts, m.dp, m.d_units, m.d_chunks,
		                   (uint32_t)m.chunks.size(), (uint32_t)m.units.size(), 0u, m.n_orient_max, m.d_path2, m.d_trans2, m.d_score, m.d_unit_x, m.d_guess, m.d_sel, m.d_bt_counters);
		hipLaunchKernelGGL(backtrace_chunks, dim3(1), dim3(256), m.chunk_lds, ts, m.dp, m.d_units, m.d_chunks,
		                   (uint32_t)m.chunks.size(), (uint32_t)m.units.size(), 1u, m.n_orient_max, m.d_path2, m.d_trans2, m.d_score, m.d_unit_x, m.d_guess, m.d_sel, m.d_bt_counters);
		hipLaunchKernelGGL(backtrace_gather, dim3((uint32_t)m.units.size()), dim3(64), 0, ts, m.d_units, (uint32_t)m.units.size(), n, m.d_path2, m.d_trans2, m.d_sel,
		                   m.d_path_index, m.d_path_trans);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_chunks, dim3(m.n_orient_max * (uint32_t)m.chunks.size()), dim3(256), m.chunk_lds, ts, false, LaunchFacts());
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_chunks, dim3(1), dim3(256), m.chunk_lds, ts, false, LaunchFacts());
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_gather, dim3((uint32_t)m.units.size()), dim3(64), 0, ts, false, LaunchFacts());
	} else if (!m.windowed) {   // (windowed: every window was walked right after its steps)
		hipLaunchKernelGGL(backtrace_kernel, dim3((uint32_t)m.jobs.size()), dim3(1024), m.bt_lds, ts, m.dp, m.d_units, m.d_btjobs,
		                   m.d_path_index, m.d_path_trans, m.d_score);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)backtrace_kernel, dim3((uint32_t)m.jobs.size()), dim3(1024), m.bt_lds, ts, false, LaunchFacts());
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(m.ev2, ts));
	if (m.device_superreads && !walked_by_group) {
		hipLaunchKernelGGL(superreads_single, dim3((n + 255u) / 256u), dim3(256), 0, ts, m.super_args);
		WHAMD_NOTE(m, WHAMD_LAUNCH_TAIL, (const void*)superreads_single, dim3((n + 255u) / 256u), dim3(256), 0, ts, false, LaunchFacts());
		HIP_TRY(hipGetLastError());
	}
	// ONE download per table (the device block has the pinned buffer's layout, upload()); pinned: a copy into pageable memory would block this call until the stream drains
	HIP_TRY(hipMemcpyAsync(m.h_pinned, m.d_path_index, (m.super_off + (m.device_superreads ? m.super_words : 0)) * sizeof(uint32_t), hipMemcpyDeviceToHost, ts));
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
		const bool behind_preview = n && m.preview.pending && m.preview.agreed > 0 && m.preview.agreed == m.preview.launched && !m.side_by_side;
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
	while (m.inflight.next_super < m.schedule.size() && launches < budget) {
		const whamd_status_t st = m.submit_super_step(p, m.schedule[m.inflight.next_super++], launches, msg);
		if (st != WHAMD_OK) return st;
	}
	m.inflight.launches += launches;
	if (m.inflight.next_super < m.schedule.size()) return WHAMD_OK;
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
	if (p.n_cols == 0 || !m.use_slots || m.windowed || m.inflight.enqueue_open || m.dp.dbg || (m.dp.dbg_flags && m.splan.ped)) return false;
	if (!m.splan.ped && m.slot_lr_used != 2 && m.slot_lr_used != 3) return false;   // (group kernels: four or eight cells per thread)
	return debug_env("WHAMD_NO_GROUP") == nullptr;
}

int DeviceTable::device_index() const { return impl_->device; }
uint32_t DeviceTable::widest_launch() const { return impl_->max_grid_x; }

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
		for (size_t i = 0; i < n; ++i) width += member(i).max_grid_x;
		tight = width > 768 && !debug_env("WHAMD_GROUP_LOOSE");
		for (size_t i = 0; i < n; ++i) {
			Impl& m = member(i);
			m.inflight.enqueue_open = true;
			m.inflight.run_stream = lead.stream;
			m.inflight.group_tables = (uint32_t)n;
			const whamd_status_t st = m.begin_solve(*problems[i], *solutions[i], msg);
			if (st != WHAMD_OK) return abort(st);
			max_steps = std::max(max_steps, m.schedule.size());
		}
		return WHAMD_OK;
	}

	// The runs of super-step k of every member that has one, each into the batch of its variant.
	void add_super_step(size_t k) {
		std::fill(counted.begin(), counted.end(), 0);
		for (size_t i = 0; i < n; ++i) {
			Impl& m = member(i);
			if (k >= m.step_brief.size()) continue;
			const Impl::StepBrief& sb = m.step_brief[k];   // (a few bytes per table and super-step: Impl::StepBrief)
#ifdef WHAMD_DEBUG_BUILD
			if (touch_fat) {   // (A/B of the round-5 change: read what the loop used to read -- the super-step and its 320-byte entries)
				const Impl::SuperStep& ss = m.schedule[k];
				for (uint32_t q = 0; q < ss.entry_count; ++q) { const SlotBatchEntry& he = m.slot_entries[ss.entry_off + q]; fat_sink += he.run.yflags + he.run.g + he.run.threads + he.ex.nf + (uint32_t)ss.lds; }
			}
#endif
			for (uint32_t q = 0; q < sb.entry_count; ++q) {
				const Impl::EntryBrief& eb = m.entry_brief[sb.entry_off + q];
				const bool xrun = eb.variant.x != eb.variant.plain && !m.dp.dbg_flags;   // (the X kernel: operands streamed from the tables, 16 KB of LDS)
				const GroupVariant v = xrun ? eb.variant.x : eb.variant.plain;
				Batch& b = batches[v];
				if (b.args.n == (uint32_t)SLOT_GROUP_MAX) flush(v);
				b.args.entry[b.args.n++] = m.d_slot_entries + sb.entry_off + q;
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
		const GroupFn kernel = group_kernel(v, DEBUG_BUILD && lead.dp.dbg_flags != 0, tight);
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
		facts.variant = (int32_t)v; facts.tight = tight; facts.stamps = lead.dp.dbg_flags != 0; facts.entries = (int32_t)members;
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
			if (k >= m.step_brief.size() || !m.step_brief[k].has_singles) continue;
			const whamd_status_t st = m.submit_singles(*problems[i], m.schedule[k], table_launches[i], msg);
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
			if (!m.use_chunks || m.windowed || !m.d_bt_entry) continue;
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
			args.entry[args.n++] = m.d_bt_entry;
			gx = std::max(gx, m.n_orient_max * (uint32_t)m.chunks.size());
			gu = std::max(gu, (uint32_t)m.units.size());
			lds = std::max(lds, m.chunk_lds);
			if (hipEventRecord(m.ev1, lead.stream) != hipSuccess) return false;
		}
		hipLaunchKernelGGL(backtrace_chunks_group, dim3(gx, args.n), dim3(256), lds, lead.stream, args, 0u);
		hipLaunchKernelGGL(backtrace_chunks_group, dim3(1, args.n), dim3(256), lds, lead.stream, args, 1u);
		hipLaunchKernelGGL(backtrace_gather_group, dim3(gu, args.n), dim3(64), 0, lead.stream, args);
		uint32_t gs = 0;   // (the superreads of the members the device makes them for, behind the gather)
		for (size_t i : batch) if (member(i).device_superreads) gs = std::max(gs, (problems[i]->n_cols + 255u) / 256u);
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
			if (gs && m.device_superreads) m.note(WHAMD_LAUNCH_GROUP_WALK, (const void*)superreads_group, dim3(gs, args.n), dim3(256), 0, lead.stream, false, facts);
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
			const bool own = debug_env("WHAMD_TAIL_OWN_STREAM") != nullptr || (!walked[i] && !m.use_chunks && !m.windowed && m.stream != lead.stream);
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
	std::vector<unsigned long long> d(m.splan.runs.size() * 48);
	HIP_TRY(hipMemcpy(d.data(), m.dp.dbg, d.size() * 8, hipMemcpyDeviceToHost));
	double a[6] = {0, 0, 0, 0, 0, 0};
	double percol[32] = {0};
	size_t cnt = 0;
	for (size_t i = 0; i < m.splan.runs.size(); ++i) {
		if (m.splan.runs[i].ncols != 22 || d[48 * i + 5] == 0) continue;   // full-length runs only
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

// The in-kernel cycle stamps of the LDS-resident runs (WHAMD_DEBUG_STAMPS, debug library), with the backtrace's and four runs' workgroup by workgroup.
whamd_status_t DeviceTable::Impl::report_resident_stamps(std::string& msg) const {
	const Impl& m = *this;
	std::vector<unsigned long long> d(m.plan.segments.size() * 8);
	HIP_TRY(hipMemcpy(d.data(), m.dp.dbg, d.size() * 8, hipMemcpyDeviceToHost));
	unsigned long long a = 0, b = 0, c2 = 0, cols = 0, p1 = 0, p2 = 0, p3 = 0, ns = 0;
	for (size_t i = 0; i < m.plan.segments.size(); ++i) { a += d[8 * i]; b += d[8 * i + 1]; c2 += d[8 * i + 2]; cols += d[8 * i + 3]; p1 += d[8 * i + 4]; p2 += d[8 * i + 5]; p3 += d[8 * i + 6]; ns += d[8 * i + 7]; }
	if (!m.plan.ped_columns.empty() || (m.dp.dbg_flags & 4u))
		fprintf(stderr, "[whamd timing] run prologue (wave 0 of workgroup 0), cycles after the first instruction: kernel arguments usable %.0f, first loaded data %.0f, everything staged %.0f\n",
		        (double)p2 / std::max<unsigned long long>(ns, 1), (double)p3 / std::max<unsigned long long>(ns, 1), (double)p1 / std::max<unsigned long long>(ns, 1));
	else
	fprintf(stderr, "[whamd timing] per barrier step (wave 0 of workgroup 0, %.1f steps per run): hot words %.0f, evaluate %.0f, barrier %.0f cycles\n",
	        (double)ns / m.plan.segments.size(), (double)p1 / std::max<unsigned long long>(ns, 1), (double)p2 / std::max<unsigned long long>(ns, 1), (double)p3 / std::max<unsigned long long>(ns, 1));
	{
		unsigned long long b3[6] = {0, 0, 0, 0, 0, 0};
		HIP_TRY(hipMemcpy(b3, m.dp.dbg + m.dp.dbg_wg_off + 4 * 512 * 2, sizeof b3, hipMemcpyDeviceToHost));
		if (b3[2]) fprintf(stderr, "[whamd timing] backtrace per run: record load + prefetch %.0f cycles, walk + hand-over %.0f cycles (%llu runs); of the latter: local exit index %.0f, chain %.0f, logical indices + stores %.0f\n",
		                   (double)b3[0] / b3[2], (double)b3[1] / b3[2], b3[2], (double)b3[3] / b3[2], (double)b3[4] / b3[2], (double)b3[5] / b3[2]);
	}
	if (m.plan.segments.size() > 104) {
		std::vector<unsigned long long> wg(4 * 512 * 2);
		HIP_TRY(hipMemcpy(wg.data(), m.dp.dbg + m.dp.dbg_wg_off, wg.size() * 8, hipMemcpyDeviceToHost));
		unsigned long long prev_end = 0;
		for (int sgi = 0; sgi < 4; ++sgi) {
			const uint32_t G = 1u << m.plan.segments[100 + sgi].g;
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
	        m.plan.segments.size(), cols, (double)a / m.plan.segments.size(), (double)b / m.plan.segments.size(),
	        (double)b / std::max<unsigned long long>(cols, 1), (double)c2 / m.plan.segments.size(), f01, f01 * 1e3 / m.plan.segments.size());
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
	std::memcpy(s.path_index.data(), m.h_pinned, (size_t)n * 4);
	std::memcpy(s.path_trans.data(), m.h_pinned + n, (size_t)n * 4);
	s.optimal_score = m.h_pinned[2 * (size_t)n];
	if (m.device_superreads) {
		const uint32_t* q = m.h_pinned + m.super_off;
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
	for (size_t j = 1; j < m.jobs.size(); ++j) s.optimal_score += m.h_pinned[2 * (size_t)n + j];  // connected components solved as their own jobs
	// (the event timings are read when somebody asks -- read_timing(), from whamd_dptable_get_stats: three runtime calls per table, from every
	//  waiting thread at once, are a measurable part of collecting a 96-table step and most callers never look at them)
	st.forward_ms = st.backtrace_ms = st.total_ms = 0;
	m.inflight.timing_pending = true;
	st.forward_launches = launches;
	st.group_tables = m.inflight.group_tables;
	st.bt_chunks = st.bt_missed = st.bt_rewalked = 0;
	if (m.use_chunks) {
		const uint32_t* c = m.h_pinned + 2 * (size_t)n + m.jobs.size();   // (downloaded with the path)
		st.bt_chunks = (uint32_t)m.chunks.size();
		st.bt_missed = c[0];
		st.bt_rewalked = c[1];
		if (debug_env("WHAMD_BT_STATS")) fprintf(stderr, "[whamd backtrace] %zu chunks, %u guesses missed (%u of them only in the transmission value), %u units walked again (of %zu)\n", m.chunks.size(), c[0], c[2], c[1], m.units.size());
	}
	whamd_status_t reported = m.dp.dbg && m.use_slots ? m.report_slot_stamps(msg) : WHAMD_OK;   // (the debug library's in-kernel cycle stamps)
	if (reported == WHAMD_OK && m.dp.dbg && !m.plan.segments.empty()) reported = m.report_resident_stamps(msg);
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
// preview forced with `pieces`, then describe_columns, lay_out_arena, the units and cut_chunks exactly as upload() runs them -- free HBM is taken as 1 TiB.
whamd_status_t DeviceTable::debug_preview_plan(Problem& p, uint32_t pieces, whamd_debug_preview_plan_result* out, uint64_t* rec_predicted, uint64_t* rec_laid_out,
                                               uint32_t* spec_predicted, uint32_t* spec_laid_out, size_t capacity, std::string& msg) {
	Impl m;
	TableBuild b;
	b.n = p.n_cols;
	b.tbits = 2 * p.n_triples;
	b.ni = std::max<uint32_t>(p.n_ind, 1);
	b.free_b = (size_t)1 << 40;
	if (p.T != 1 || p.n_cols == 0) { msg = "a single-individual table expected"; return WHAMD_ERR_UNSUPPORTED; }
	m.wide = !select_kernels(p.T, p.n_ind, m.fused, m.keysfn);
	m.use_slots = plan_forward_slots(p, std::max(8, m.slot_l), m.symmetry, m.splan, m.slot_lr);
	if (!m.use_slots) { msg = "the table is not planned on slot runs"; return WHAMD_ERR_UNSUPPORTED; }
	m.plan = ResidentPlan();
	m.plan.steps = m.splan.steps;
	m.plan.component_first_step = m.splan.component_first_step;
	m.plan.col_to_res.assign(p.n_cols, -1);
	m.preview.mode = 1;
	m.preview.pieces_wanted = pieces;
	Impl::PreviewPlan pp;
	m.plan_preview(p, b, true, pp);
	whamd_status_t st = m.describe_columns(p, b, msg);
	if (st == WHAMD_OK) st = m.lay_out_arena(p, b, msg);
	if (st != WHAMD_OK) return st;
	m.build_slot_blobs(b);
	m.lay_out_slot_tables(b, false);
	m.make_jobs();
	m.make_units(b);
	m.cut_chunks(p);
	static const char* const* why = preview_why_lines();
	*out = whamd_debug_preview_plan_result{};
	out->n_pieces = slot_plan_pieces(p.n_cols);
	out->pieces = pp.pieces;
	out->steps = pp.steps;
	out->n_steps = (uint32_t)m.plan.steps.size();
	out->why_not = why[pp.why < Impl::PV_WHYS ? pp.why : 0];
	out->chunked_predicted = pp.chunked; out->chunked = m.use_chunks;
	out->n_seeds_predicted = pp.n_spec; out->n_seeds = m.n_spec;
	out->stride_predicted = pp.stride; out->stride = m.use_chunks ? m.dp.spec_stride : 64u;
	out->arena_predicted = pp.arena; out->arena_laid_out = b.bt;
	out->windowed = m.windowed;
	out->exchange_predicted = (uint64_t)(1ull << pp.max_f) * p.T * 4; out->exchange_laid_out = b.exchange_bytes;
	for (uint32_t k = 0; k < pp.steps && k < capacity; ++k) {
		const SlotRun& run = m.splan.runs[m.plan.steps[k].index];
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
	out->ran = pv.why == Impl::PV_RAN;
	out->continued = pv.continued;
	out->pieces = pv.pieces;
	out->launched_steps = pv.launched;
	out->agreed_steps = pv.agreed;
	out->from_hook = pv.why == Impl::PV_RAN && pv.from_hook ? 1u : 0u;
	out->why_not = why[pv.why < Impl::PV_WHYS ? pv.why : 0];
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
