// table_plan.h -- the host side of a phasing table's create (DeviceTable::upload in dp_device.hip), free of HIP calls: table_plan.cpp is compiled as host
// code, and tests/test_table_plan_host.py runs it as a stand-alone program.  From the Problem and the forward plan alone it decides
//   where every backtrace record lies in the arena and where the windows are cut,
//   which jobs, lanes, backtrace units, chunks and seeds there are,
//   what the schedule's super-steps contain, and what a preview may launch ahead of all that.
// The driver keeps what allocates, copies or launches, and calls these functions in the order of its phases.  Device pointers occur here only as values
// that are stored into entries and lanes; nothing here dereferences one.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "debug_build.h"
#include "device_types.h"
#include "host_parallel.h"
#include "problem.h"

namespace whamd {

// What the caller set (DeviceTable::set_*): read by the next upload(), untouched by a release.
struct TableOptions {
	std::string path = "auto";
	int l_pref = 11;
	bool fold = true;
	int symmetry = 1;           // single individual: compute only half of a run, the rest is its mirror image (plan_forward)
	int slot_l = 11;            // preferred number of local slots (lr + 6 .. lr + 9; pedigree runs: 6 - log2 T .. + 3, only when set explicitly)
	bool slot_l_set = false;
	int slot_lr = 2;            // reg slots: 4 cells per thread -> 8 waves per workgroup at 11 local slots (two waves per SIMD)
	bool shared_hint = false;   // option shared_launches: the table will be solved together with many others (enqueue_many)
	bool side_by_side = false;  // this solve's launches run beside other tables' on their own streams: X runs take the streamed variant (16 KB of LDS instead of ~90:
	                            // three tables on three streams, 3.1 M columns/s with the LDS lines -- one workgroup per CU, the streams take turns -- 5 M without)
	int max_lanes = 32;
	uint64_t arena_limit = 0;   // option arena_limit_bytes (0: what hipMemGetInfo leaves)
	int preview_mode = -1;      // option preview: -1 auto, 0 never, 1 wherever the table's form allows it
	uint32_t preview_pieces = 0;   // option preview_pieces (0: the library's rule)
	bool thread_budget = false; // the create is held to a thread budget (option host_threads)
};

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
// Windowed solve (backtrace arena larger than what HBM can hold): the steps are cut into WINDOWS whose records fit the
// arena one at a time.  Pass 1 runs the whole forward pass (records of all windows but the last are written and
// dropped) and keeps the exchange column at every window boundary; then, newest window first, the window's steps
// are run again from the kept column -- this time its records survive until its units have been walked.  Twice the
// forward work, any table length.  Offsets into the arena are window-relative.
struct Window {
	uint32_t step_lo = 0, step_hi = 0;   // positions in the job's step list
	uint32_t unit_off = 0, unit_count = 0;
};

// The kernel variants of a group launch (DESIGN.md 6.2 has the table).  The values are the order of the launches inside a super-step.
enum GroupVariant : uint8_t { GV_SINGLE4 = 0, GV_PED_2_2, GV_PED_2_4, GV_PED_4_2, GV_PED_4_4, GV_PED_2_16, GV_SINGLE8, GV_TRIO_FACT, GV_X4, GV_X8, GV_QUARTET_FACT, GROUP_VARIANTS };
struct GroupVariantPair { GroupVariant plain, x; };   // x: the X kernel's variant where the run is eligible (else = plain)
GroupVariantPair group_variants_of(const SlotBatchEntry& he, bool ped);

// What a GROUP submission (enqueue_group) needs of a super-step and of its entries, a few bytes each: with 96 tables per launch the submitting thread read a
// 320-byte SlotBatchEntry and a SuperStep per table and super-step out of cold memory -- 31 ms of host time for 2 276 super-steps, 13 ms with these
// (scripts/gpu_group_submit_ab.py).  Built at create time (where the entries are made, on the create's own threads).
struct StepBrief { uint32_t entry_off, lds; uint16_t entry_count; uint8_t has_singles, pad; };
struct EntryBrief { uint16_t grid_x, threads; uint32_t lds_x; GroupVariantPair variant; uint8_t pad[2]; };

// The host description of a built table: what the functions below produce and the solve reads.  Default-constructed by every release.
struct TablePlan {
	// plan and path
	RawVec<DevColumn> cols;
	ResidentPlan plan;
	SlotPlan splan;             // slot runs (slots.h): the default forward path of a single individual
	bool use_slots = false;
	int slot_lr_used = 2;       // reg slots of the plan in use (the shared-launches layout takes 3)
	uint64_t table_bytes = 0;   // pedigree slot runs: cost-form tables
	bool wide = false;          // column_step_wide instead of the templated per-column kernels
	bool device_superreads = false;   // get_super_reads on the device (kernels_backtrace.h superreads_single): a table with one individual and trusted genotypes
	// arena and windows
	uint64_t bt_bytes = 0;
	bool windowed = false;
	std::vector<Window> windows;
	size_t checkpoint_bytes = 0;
	// jobs, units and chunks (the chunked speculative backtrace, kernels_backtrace.h, of a table made of runs)
	std::vector<Job> jobs;
	std::vector<Lane> lanes;
	std::vector<BtUnit> units;
	std::vector<BtChunk> chunks;
	bool use_chunks = false;
	uint32_t n_spec = 0;
	uint32_t n_orient_max = 1;  // most orientations any chunk has (2 for a single individual, 8 for a trio)
	// schedule
	std::vector<SuperStep> schedule;
	std::vector<ResBatchEntry> entries;
	std::vector<SlotBatchEntry> slot_entries;   // (pedigree runs: `pad` holds the run's index into splan.pextra)
	std::vector<StepBrief> step_brief;
	std::vector<EntryBrief> entry_brief;
	uint32_t max_grid_x = 1;    // widest launch of the schedule, in workgroups
	size_t bt_lds = 0, chunk_lds = 0;   // LDS of backtrace_kernel / backtrace_chunks
	// superreads
	size_t super_words = 0, super_off = 0;   // size of the result (u32 words) and where it lies in the pinned block
};

// ---------------------------------------------------------------------------------------------- layout arithmetic
// Runs of set bits of `mask` as deposit segments (compact position | mask position << 8 | length << 16).
void append_segments(uint32_t mask, std::vector<uint32_t>& out, uint16_t& count);
// The path a per-column step takes (0 fused, 1 keys) and the bytes of its backtrace record, from the column's sizes alone (lay_out_arena; the preview's arena bound).
uint32_t column_step_mode(bool force_keys, bool is_last, uint32_t f, uint32_t ebits);
uint64_t column_record_bytes(uint32_t mode, uint32_t T, uint32_t f, uint32_t nplanes);
// What the backtrace arena may take: free HBM minus the descriptors (~1 KiB per column), exchange buffers, tables and slack; at most the option arena_limit_bytes.
uint64_t arena_capacity(uint64_t free_b, uint32_t n, uint64_t table_bytes, uint64_t arena_limit);
// Where the next record starts behind one of `bytes` at `bt` (records are 16-byte aligned).
uint64_t arena_behind(uint64_t bt, uint64_t bytes);
// The record of one single-individual slot run: only launched workgroups write.
uint64_t slot_run_record_bytes(const SlotRun& run);
// The plan pieces a preview covers: what the option asks for, else a sixth of the table's (plan_preview; choose_plan's head hook asks the planner for the same).
uint32_t preview_pieces_of(uint32_t wanted, uint32_t n_pieces);

// ---------------------------------------------------------------------------------------------- the phases, in the order upload() runs them
// (the comments of the definitions say what each reads and produces)
whamd_status_t describe_columns(const Problem& p, TableBuild& b, TablePlan& m, std::string& msg);
whamd_status_t lay_out_arena(const Problem& p, const TableOptions& o, TableBuild& b, TablePlan& m, std::string& msg);
size_t upload_bound(const Problem& p, const TableBuild& b, const TablePlan& m);
void build_slot_blobs(const TablePlan& m, TableBuild& b);
uint64_t lay_out_slot_tables(TablePlan& m, const TableBuild& b, bool report = true);
void make_jobs(const TableOptions& o, TablePlan& m);
void make_units(const TableBuild& b, TablePlan& m);
whamd_status_t cut_windows(const TableBuild& b, TablePlan& m, std::vector<BtJob>& wjobs, std::string& msg);

// The chunk rule of the speculative backtrace over a job's units, newest first (unit u is the job's step size - 1 - u): a run that finds BT_CHUNK_RUNS runs in the
// chunk in front of it starts a new chunk and leaves that chunk's seed.  starts(u, id) is called for every such unit, id = 1, 2, ...; returns how many there are.
// (cut_chunks walks the units with it, the preview the plan's steps: one rule.)
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
bool backtrace_is_chunked(bool on_runs, size_t n_jobs, bool windowed, size_t n_units);
// The seeds' stride: the most waves any run that leaves a seed has (at least 64 words).
uint32_t seed_stride_of(uint32_t stride, const SlotRun& run);
void cut_chunks(const Problem& p, TablePlan& m, uint32_t& spec_stride);
void backtrace_lds_sizes(const TableBuild& b, TablePlan& m);
void assign_lanes(const TableOptions& o, const TableBuild& b, TablePlan& m);
whamd_status_t make_schedule(const TableBuild& b, const DevProblem& dp, uint32_t* d_job_scores, TablePlan& m, std::string& msg);
void make_briefs(TablePlan& m);

// ---------------------------------------------------------------------------------------------- the preview's plan
// PV_RAN, or why a table has no preview.
enum PreviewWhy : uint32_t { PV_RAN = 0, PV_OFF, PV_NOT_CREATE, PV_NOT_SLOTS, PV_DEBUG_SWITCH, PV_SHARED, PV_THREAD_BUDGET, PV_COMPONENTS, PV_FEW_PIECES, PV_NOT_ALONE, PV_NO_LEADING_RUNS,
                           PV_ROW_PAD, PV_ARENA, PV_WHYS };
struct PreviewPlan {   // plan_preview's answer
	uint32_t why = PV_NOT_CREATE, pieces = 0, steps = 0, end_col = 0, n_spec = 0, stride = 64, max_f = 0;
	bool chunked = false;
	uint64_t arena = 0, tab_words = 0;   // bytes of the arena (all steps), words of the preview's table block
	size_t ctrl_words = 0;
	std::vector<uint64_t> rec;           // [steps] record offsets
	std::vector<uint32_t> spec;          // [steps] seed ids
};
// alone: this table is the only one of the process that holds resources of its device (asked under `auto` only).
void plan_preview(const Problem& p, const TableOptions& o, const TableBuild& b, TablePlan& m, bool from_create, bool alone, PreviewPlan& out);

}  // namespace whamd
