// device_table.h -- host-visible interface of the device driver (dp_device.hip).
#pragma once
#include <string>

#ifdef WHAMD_DEBUG_BUILD
#include "../../include/whatshap_amd_debug.h"
#endif
#include "device_types.h"
#include "problem.h"

namespace whamd {

class DeviceTable {
public:
	DeviceTable();
	~DeviceTable();
	DeviceTable(const DeviceTable&) = delete;
	DeviceTable& operator=(const DeviceTable&) = delete;

	static int device_count();
	static bool device_pci_bus_id(int device, std::string& out);   // "0000:c5:00.0"; false if there is no such device
	// Builds the per-column descriptors for `p` and uploads everything the kernels read.
	// (`p` is not const: a table with lazy generic terms -- Problem::lazy_terms -- gets the term lists of the columns its plan leaves outside runs here)
	// from_create: the call is whamd_dptable_create's own upload -- the only one that may start a preview (set_preview).
	whamd_status_t upload(Problem& p, int device, std::string& msg, bool from_create = false);
	// Forward pass + backtrace on the device; fills s.path_*, s.optimal_score and the timing fields of st.
	whamd_status_t solve(const Problem& p, Solution& s, whamd_solve_stats& st, std::string& msg);
	// The two halves of solve(): enqueue() only submits the launches to the table's stream (several tables can be in
	// flight at once on one device), wait() blocks until the path has arrived and reads the event timings.
	whamd_status_t enqueue(const Problem& p, Solution& s, std::string& msg);
	// Resumable enqueue(): at most `budget` forward launches per call; `done` once backtrace and downloads are submitted.
	whamd_status_t enqueue_some(const Problem& p, Solution& s, uint64_t budget, bool& done, std::string& msg);
	whamd_status_t wait(const Problem& p, Solution& s, whamd_solve_stats& st, std::string& msg);
	// forward_ms / backtrace_ms / total_ms of the solve wait() collected last: read from the events on demand (wait() leaves them 0).
	void read_timing(whamd_solve_stats& st);
	// Several tables of ONE device as one sequence of launches (see dp_device.hip, "group solve"): every table must be group_eligible().
	// Afterwards each table is in flight exactly as after enqueue(): collect with wait().
	static whamd_status_t enqueue_group(DeviceTable* const* tables, const Problem* const* problems, Solution* const* solutions, size_t n_tables, std::string& msg);
	// Before the wait() of several tables in flight: one host wait per stream that carries tails of a group (dp_device.hip).
	static void wait_last_of_each_stream(DeviceTable* const* tables, size_t n_tables);
	bool group_eligible(const Problem& p) const;
	int device_index() const;
	uint32_t widest_launch() const;   // workgroups of the widest launch of the schedule
	// Drops a partially submitted solve (enqueue_some that has not reported `done`): drains the stream, rewinds the cursor.
	void abort_enqueue();
	// Frees the device buffers, the stream and the events; the next upload() recreates them.
	void release_device();
	// Solver variant ("auto", "column", "column_keys", "resident", "slots"); takes effect at the next upload().
	// auto: slot runs (slots.h) for a single individual, LDS-resident runs for a trio, per-column kernels otherwise.
	bool set_path(const std::string& path);
	// Preferred log2 slice size of the resident path (tuning knob); takes effect at the next upload().
	void set_l_pref(int l);
	// Preferred number of local slots of a slot run (9 .. 12: 1 .. 8 waves per workgroup); next upload().
	void set_slot_l(int l);
	// Reg slots of a slot run: 2 (4 cells per thread, default) or 3 (8 cells per thread); next upload().
	void set_slot_lr(int lr);
	// Fold columns in which no read ends into the next resident column (default on); next upload().
	void set_fold(bool v);
	// Exploit D[~x] == D[x] in single-individual runs: 0 off, 1 full-chip runs (default), 2 every run; next upload().
	void set_symmetry(int level);
	// Lanes over which the connected components of a single-individual table are spread (default 32, 1 = off); the
	// lanes advance in lockstep, their runs go out as batched launches; next upload().
	void set_lanes(int n);
	// Upper bound of the backtrace arena in bytes (0 = whatever free HBM allows).  A table whose records need more is
	// solved in windows (the forward pass of every window but the newest runs twice); next upload().
	void set_arena_limit(uint64_t bytes);
	// The table will be solved together with many others (whamd_dptable_enqueue_many): a wide single-individual table then plans eight cells
	// per thread and twelve local slots (half the wavefronts per table); next upload().
	void set_shared_launches(bool v);
	// The preview: a lone single-individual table's leading slot runs are launched from inside the create and the first enqueue continues behind them
	// (dp_device.hip start_preview).  mode -1 auto (the default: only a table that is alone on its device, of eight plan pieces and more, created
	// without a thread budget), 0 never, 1 wherever the table's form allows it; pieces: plan pieces it covers (0: a sixth of them); next upload().
	void set_preview(int mode);
	void set_preview_pieces(uint32_t pieces);
	void set_thread_budget(bool v);   // the create is held to a thread budget (option host_threads): a caller that runs many tables at once
	// the table's launches will run BESIDE other tables' on the same device (own streams, whamd_dptable_enqueue_many): kernels that leave room on a CU
	void set_side_by_side(bool v);

#ifdef WHAMD_DEBUG_BUILD
	// The launch ledger of the debug library (include/whatshap_amd_debug.h): the registry of the solve's kernels, and the launches of the solve wait() collected last.
	static size_t debug_solve_kernels(whamd_debug_kernel* out, size_t capacity);
	size_t debug_launches(whamd_debug_launch* out, size_t capacity) const;
	void debug_preview(whamd_debug_preview* out) const;
	static whamd_status_t debug_preview_plan(Problem& p, uint32_t pieces, whamd_debug_preview_plan_result* out, uint64_t* rec_predicted, uint64_t* rec_laid_out,
	                                         uint32_t* spec_predicted, uint32_t* spec_laid_out, size_t capacity, std::string& msg);
#endif

private:
	whamd_status_t enqueue_some_unguarded(const Problem& p, Solution& s, uint64_t budget, bool& done, std::string& msg);
	struct Impl;
	Impl* impl_;
};

}  // namespace whamd
