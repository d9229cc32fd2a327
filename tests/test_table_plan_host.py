"""The host side of a phasing table's create (whatshap_amd/csrc/table_plan.h), on the host alone: a stand-alone C++ program built with the address and
undefined-behaviour sanitizers builds small problems, plans them as DeviceTable::choose_plan does and runs the host phases of DeviceTable::upload in its order
-- arena layout and windows, jobs, backtrace units, chunks, lanes, schedule, briefs, the preview's plan -- and holds their results against the invariants the
driver and the kernels rely on.  Nothing is loaded into Python, no device is needed, and the compile line has no HIP include path: table_plan.cpp is host code.

Tables: a single individual at coverage 8, as long as the plan needs for a chunked backtrace (about 600 columns); the same under an arena limit of a third
of its records (three windows and more) and of one byte less than its largest record (refused); five components on one lane and on four; a trio at coverage 6
on pedigree slot runs, on LDS-resident runs and per column.  The preview's prediction needs two plan pieces and more (16 384 columns), so it is held against
the layout on a table of the first kind with nine pieces, for 1 and 8 pieces; the short table must be refused a preview for having too few.

Time, measured with g++ 11: the whole test takes 20 s of wall time and 54 s of CPU time, nearly all of it the compiler at -O1 with both sanitizers -- which is
why the five units (this program and four sources) are compiled as separate objects side by side; the program itself runs in about a second."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whatshap_amd", "csrc")
SOURCES = ["table_plan.cpp", "problem.cpp", "slot_plan.cpp", "resident_plan.cpp"]

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <map>
#include <set>

#include "table_plan.h"

using namespace whamd;

#define CHECK(cond)                                                                      \
	do {                                                                                 \
		if (!(cond)) {                                                                   \
			std::printf("%s, line %d: %s does not hold\n", g_case, __LINE__, #cond);     \
			return false;                                                                \
		}                                                                                \
	} while (0)

static const char* g_case = "";

// ---- problems: reads of `coverage` variants starting at every variant (one read ends and one starts per column); `components` > 1: no read crosses the
// equally spaced boundaries; trio: reads round-robin over father, mother, child
struct Input {
	std::vector<uint64_t> read_ptr{0};
	std::vector<int32_t> position, sample;
	std::vector<uint8_t> allele;
	std::vector<uint32_t> quality, recomb, positions, ids, triples;
	std::vector<uint8_t> genotype;
};

static bool make_problem(uint32_t n, uint32_t coverage, uint32_t components, bool trio, Problem& p) {
	Input in;
	uint32_t state = 12345u + n + coverage;
	auto rnd = [&state]() { state = state * 1664525u + 1013904223u; return state >> 8; };
	std::vector<uint8_t> hap(n);
	for (uint32_t c = 0; c < n; ++c) hap[c] = rnd() & 1u;
	const uint32_t comp_len = (n + components - 1) / components;
	uint32_t r = 0;
	for (uint32_t s = 0; s + 1 < n; ++s) {
		const uint32_t comp_end = std::min(n, (s / comp_len + 1) * comp_len);
		const uint32_t e = std::min(s + coverage, comp_end);
		if (e - s < 2) continue;
		const uint32_t h = rnd() & 1u;
		for (uint32_t c = s; c < e; ++c) {
			in.position.push_back((int32_t)(1000 * (c + 1)));
			in.allele.push_back((uint8_t)(hap[c] ^ h ^ (rnd() % 50 == 0 ? 1u : 0u)));
			in.quality.push_back(5 + rnd() % 36);
		}
		in.read_ptr.push_back(in.position.size());
		in.sample.push_back(trio ? (int32_t)(r % 3) : 0);
		++r;
	}
	const uint32_t n_ind = trio ? 3 : 1;
	for (uint32_t i = 0; i < n_ind; ++i) in.ids.push_back(i);
	if (trio) in.triples = {0, 1, 2};
	in.genotype.assign((size_t)n_ind * n, 1);
	in.recomb.assign(n, trio ? 20u : 1u);
	if (trio) in.recomb[0] = 0;
	for (uint32_t c = 0; c < n; ++c) in.positions.push_back(1000 * (c + 1));
	whamd_readset_view rs{};
	rs.n_reads = r; rs.read_ptr = in.read_ptr.data(); rs.var_position = in.position.data(); rs.var_allele = in.allele.data(); rs.var_quality = in.quality.data();
	rs.read_sample_id = in.sample.data();
	whamd_pedigree_view ped{};
	ped.n_individuals = n_ind; ped.individual_id = in.ids.data(); ped.n_triples = trio ? 1 : 0; ped.triple_ids = in.triples.data(); ped.n_variants = n;
	ped.genotype = in.genotype.data();
	std::string msg;
	const whamd_status_t st = build_problem(&rs, in.recomb.data(), in.recomb.size(), &ped, false, in.positions.data(), in.positions.size(), p, msg);
	if (st != WHAMD_OK) std::printf("build_problem: %s\n", msg.c_str());
	return st == WHAMD_OK && p.n_cols == n;
}

// ---- a table, planned as choose_plan plans it and built by the host phases in upload()'s order
struct Table {
	TableOptions opt;
	TableBuild b;
	TablePlan tp;
	DevProblem dp{};
	std::vector<BtJob> wjobs;
	std::vector<uint32_t> scores;                  // stands for d_job_scores
	std::vector<std::vector<uint32_t>> buffers;    // [lane][0, 1: exchange buffers; 2: key scratch], never dereferenced
	whamd_status_t status = WHAMD_OK;              // of lay_out_arena
	std::string msg;
};

static bool plan_table(Problem& p, Table& t) {
	t.b.n = p.n_cols;
	t.b.tbits = 2 * p.n_triples;
	t.b.ni = std::max<uint32_t>(p.n_ind, 1);
	t.b.free_b = (size_t)1 << 40;
	t.b.force_keys = t.opt.path == "column_keys";
	TablePlan& tp = t.tp;
	tp.use_slots = (t.opt.path == "auto" || t.opt.path == "slots") &&
	               plan_forward_slots(p, p.T > 1 ? (t.opt.slot_l_set ? -t.opt.slot_l : 0) : std::max(8, t.opt.slot_l), t.opt.symmetry, tp.splan, t.opt.slot_lr);
	if (tp.use_slots && tp.splan.ped && tp.splan.table_words * 4ull > t.b.free_b / 4) tp.use_slots = false;
	tp.table_bytes = tp.use_slots && tp.splan.ped ? tp.splan.table_words * 4ull : 0ull;
	if (tp.use_slots) {
		tp.plan = ResidentPlan();
		tp.plan.steps = tp.splan.steps;
		tp.plan.component_first_step = tp.splan.component_first_step;
		tp.plan.col_to_res.assign(p.n_cols, -1);
	} else {
		tp.splan = SlotPlan();
		plan_forward(p, t.opt.path == "auto" || t.opt.path == "resident", t.opt.l_pref, t.opt.fold, tp.plan, t.opt.symmetry);
	}
	t.b.ped_slots = tp.use_slots && tp.splan.ped;
	return true;
}

static bool build_table(const Problem& p, Table& t) {
	TablePlan& tp = t.tp;
	TableBuild& b = t.b;
	CHECK(describe_columns(p, b, tp, t.msg) == WHAMD_OK);
	t.status = lay_out_arena(p, t.opt, b, tp, t.msg);
	if (t.status != WHAMD_OK) return true;
	CHECK(upload_bound(p, b, tp) > tp.cols.size() * sizeof(DevColumn));
	build_slot_blobs(tp, b);
	if (tp.use_slots && !b.ped_slots) CHECK(lay_out_slot_tables(tp, b) < 0xFFFFFFFFull);
	make_jobs(t.opt, tp);
	make_units(b, tp);
	if (tp.windowed) CHECK(cut_windows(b, tp, t.wjobs, t.msg) == WHAMD_OK);
	t.dp.spec_stride = 0;
	cut_chunks(p, tp, t.dp.spec_stride);
	backtrace_lds_sizes(b, tp);
	assign_lanes(t.opt, b, tp);
	t.scores.assign(tp.jobs.size(), 0);
	t.buffers.assign(tp.lanes.size() * 3, std::vector<uint32_t>(4));
	for (size_t l = 0; l < tp.lanes.size(); ++l) {
		tp.lanes[l].d_pr[0] = t.buffers[3 * l].data();
		tp.lanes[l].d_pr[1] = t.buffers[3 * l + 1].data();
		tp.lanes[l].d_keys = (unsigned long long*)t.buffers[3 * l + 2].data();
	}
	CHECK(make_schedule(b, t.dp, t.scores.data(), tp, t.msg) == WHAMD_OK);
	make_briefs(tp);
	return true;
}

// ---- what a step is, from the plan alone
struct StepFacts { uint32_t c0, ncols; uint64_t rec, bytes; uint32_t unit_kind; };

static StepFacts facts_of(const Problem& p, const Table& t, uint32_t si) {
	const TablePlan& tp = t.tp;
	const Step& st = tp.plan.steps[si];
	StepFacts f{};
	if (st.kind == 0) {
		const DevColumn& d = tp.cols[st.index];
		f = StepFacts{st.index, 1, d.bt_off, column_record_bytes(d.mode, p.T, d.f, d.nplanes), 0};
	} else if (st.kind == 2) {
		const SlotRun& run = tp.splan.runs[st.index];
		const uint64_t bytes = t.b.ped_slots ? ((uint64_t)tp.splan.pextra[st.index].rec_words * 4ull << run.g) : slot_run_record_bytes(run);
		f = StepFacts{run.c0, run.ncols, ((uint64_t)run.rec_hi << 32) | run.rec_lo, bytes, t.b.ped_slots ? 3u : 2u};
	} else {
		const ResSegment& sg = tp.plan.segments[st.index];
		f = StepFacts{sg.c0, sg.ncols, ((uint64_t)sg.bt_hi << 32) | sg.bt_lo, (uint64_t)sg.stage_words * (1ull << sg.g) * 8ull, 1};
	}
	return f;
}

static bool check_records(const Problem& p, const Table& t) {
	const TablePlan& tp = t.tp;
	const size_t n_steps = tp.plan.steps.size();
	std::set<uint32_t> first_cols;
	uint64_t end = 0, largest = 0;
	size_t window = 0;
	uint32_t next_col = 0;
	for (uint32_t si = 0; si < n_steps; ++si) {
		const StepFacts f = facts_of(p, t, si);
		CHECK(f.c0 == next_col);                      // the steps cover the columns in order
		next_col = f.c0 + f.ncols;
		first_cols.insert(f.c0);
		CHECK(f.rec % 16 == 0);
		if (window < t.b.window_first_col.size() && t.b.window_first_col[window] == f.c0) {   // a new window: offsets start over
			largest = std::max(largest, end);
			end = 0;
			++window;
			CHECK(f.rec == 0);
		}
		CHECK(f.rec >= end);                          // no overlap inside a window
		end = arena_behind(f.rec, f.bytes);
		CHECK(f.rec + f.bytes + 16 <= t.b.arena_cap); // every window within the capacity
	}
	CHECK(next_col == p.n_cols);
	CHECK(window == t.b.window_first_col.size());
	CHECK(t.b.bt == std::max(largest, end) && tp.bt_bytes == t.b.bt);
	CHECK(tp.windowed == !t.b.window_first_col.empty());
	for (uint32_t c : t.b.window_first_col) CHECK(first_cols.count(c) == 1);
	CHECK(t.b.exchange_bytes == ((size_t)1 << t.b.max_f) * p.T * 4 && tp.checkpoint_bytes == t.b.exchange_bytes);
	if (!tp.windowed) { CHECK(tp.windows.empty()); return true; }
	// the windows partition the single job's steps
	CHECK(tp.jobs.size() == 1 && tp.windows.size() == t.b.window_first_col.size() + 1 && t.wjobs.size() == tp.windows.size());
	uint32_t pos = 0;
	for (size_t wi = 0; wi < tp.windows.size(); ++wi) {
		const Window& w = tp.windows[wi];
		CHECK(w.step_lo == pos && w.step_hi > w.step_lo);
		pos = w.step_hi;
		if (wi > 0) CHECK(facts_of(p, t, tp.jobs[0].steps[w.step_lo]).c0 == t.b.window_first_col[wi - 1]);
		CHECK(w.unit_off == n_steps - w.step_hi && w.unit_count == w.step_hi - w.step_lo);
		CHECK(t.wjobs[wi].unit_off == w.unit_off && t.wjobs[wi].unit_count == w.unit_count && t.wjobs[wi].with_last_column == (wi + 1 == tp.windows.size() ? 1u : 2u));
	}
	CHECK(pos == n_steps);
	return true;
}

static bool check_jobs_and_units(const Problem& p, const Table& t) {
	const TablePlan& tp = t.tp;
	const size_t n_steps = tp.plan.steps.size();
	std::vector<uint32_t> seen(n_steps, 0);
	CHECK(!tp.jobs.empty() && tp.jobs[0].final && tp.jobs[0].steps.back() == n_steps - 1);
	size_t units = 0;
	for (size_t j = 0; j < tp.jobs.size(); ++j) {
		const Job& job = tp.jobs[j];
		CHECK(job.final == (j == 0) && !job.steps.empty());
		CHECK(job.unit_off == units && job.unit_count == job.steps.size());
		units += job.unit_count;
		for (size_t k = 0; k < job.steps.size(); ++k) {
			CHECK(job.steps[k] < n_steps && (k == 0 || job.steps[k] == job.steps[k - 1] + 1));
			++seen[job.steps[k]];
			const StepFacts f = facts_of(p, t, job.steps[k]);
			const BtUnit& u = tp.units[job.unit_off + job.steps.size() - 1 - k];   // the units are the job's steps in reverse
			SlotBtUnit su;
			std::memcpy(&su, &u, sizeof su);
			CHECK(u.kind == f.unit_kind && u.c0 == f.c0 && u.ncols == f.ncols);
			if (f.unit_kind >= 2) CHECK((((uint64_t)su.bt_hi << 32) | su.bt_lo) == f.rec);
			else CHECK((((uint64_t)u.bt_hi << 32) | u.bt_lo) == f.rec);
		}
	}
	CHECK(units == tp.units.size() && units == n_steps);
	for (uint32_t s : seen) CHECK(s == 1);
	if (tp.jobs.size() > 1) {   // split: one job per component, the final job holds the last one
		const std::vector<uint32_t>& first = tp.plan.component_first_step;
		CHECK(tp.jobs.size() == first.size() && tp.jobs[0].steps.front() == first.back());
		for (size_t k = 0; k + 1 < first.size(); ++k) CHECK(tp.jobs[k + 1].steps.front() == first[k] && tp.jobs[k + 1].steps.back() + 1 == first[k + 1]);
	}
	return true;
}

static bool check_chunks(const Table& t) {
	const TablePlan& tp = t.tp;
	const bool trio_runs = !tp.use_slots && !tp.plan.ped_columns.empty();
	std::map<uint32_t, uint32_t> seed_of_step;   // step -> id, from the runs
	for (uint32_t si = 0; si < tp.plan.steps.size(); ++si) {
		const Step& st = tp.plan.steps[si];
		const uint32_t id = st.kind == 2 ? tp.splan.runs[st.index].spec_id : (st.kind == 1 && trio_runs ? tp.plan.segments[st.index].in_mirror_bit : 0u);
		if (id) seed_of_step[si] = id;
	}
	if (tp.windowed || tp.jobs.size() > 1) CHECK(!tp.use_chunks);
	if (!tp.use_chunks) { CHECK(tp.chunks.empty() && tp.n_spec == 0 && seed_of_step.empty()); return true; }
	CHECK(tp.units.size() > 2u * BT_CHUNK_RUNS && tp.n_spec + 1 == tp.chunks.size());
	uint32_t off = 0, orient = 1;
	std::map<uint32_t, uint32_t> expected;
	for (size_t i = 0; i < tp.chunks.size(); ++i) {
		const BtChunk& ch = tp.chunks[i];
		CHECK(ch.unit_off == off && ch.unit_count > 0 && ch.spec_id == i && ch.n_orient >= 1 && ch.n_orient <= BT_ORIENT);
		off += ch.unit_count;
		orient = std::max(orient, ch.n_orient);
		if (i > 0) expected[(uint32_t)(tp.jobs[0].steps[tp.jobs[0].steps.size() - 1 - ch.unit_off])] = (uint32_t)i;   // the run of the chunk's first unit leaves its seed
	}
	CHECK(off == tp.units.size() && orient == tp.n_orient_max);
	CHECK(seed_of_step == expected);
	CHECK(t.dp.spec_stride >= 64);
	for (const auto& s : seed_of_step) {
		const Step& st = tp.plan.steps[s.first];
		if (st.kind == 2) CHECK(t.dp.spec_stride >= seed_stride_of(0, tp.splan.runs[st.index]));
		else CHECK(t.dp.spec_stride >= ((tp.plan.segments[st.index].threads >> 6) << tp.plan.segments[st.index].g));
	}
	return true;
}

static bool check_schedule(const Table& t) {
	const TablePlan& tp = t.tp;
	const size_t n_lanes = tp.lanes.size();
	CHECK(n_lanes >= 1 && n_lanes <= (size_t)t.opt.max_lanes && n_lanes <= tp.jobs.size());
	CHECK(!tp.lanes[0].jobs.empty() && tp.lanes[0].jobs[0] == 0);
	std::vector<uint32_t> lane_of(tp.jobs.size(), ~0u);
	std::vector<std::vector<std::pair<uint32_t, uint32_t>>> todo(n_lanes);   // per lane: (job, position in the job) in execution order
	for (size_t l = 0; l < n_lanes; ++l)
		for (uint32_t j : tp.lanes[l].jobs) {
			CHECK(j < tp.jobs.size() && lane_of[j] == ~0u);
			lane_of[j] = (uint32_t)l;
			for (uint32_t k = 0; k < tp.jobs[j].steps.size(); ++k) todo[l].emplace_back(j, k);
		}
	for (uint32_t l : lane_of) CHECK(l != ~0u);
	size_t first_pass = 0;
	for (const auto& q : todo) first_pass = std::max(first_pass, q.size());
	CHECK(tp.schedule.size() >= first_pass);
	size_t n_entries = 0;
	uint32_t widest = 1;
	for (size_t s = 0; s < first_pass; ++s) {
		const SuperStep& ss = tp.schedule[s];
		CHECK(ss.entry_off == n_entries);
		uint32_t e_i = 0;
		size_t single_i = 0;
		for (size_t l = 0; l < n_lanes; ++l) {
			if (s >= todo[l].size()) continue;
			const uint32_t j = todo[l][s].first, k = todo[l][s].second, flip = (uint32_t)(s & 1u);
			const Job& job = tp.jobs[j];
			const Step& st = tp.plan.steps[job.steps[k]];
			const bool first = k == 0, last = k + 1 == job.steps.size();
			const uint32_t* prev = tp.lanes[l].d_pr[flip];
			uint32_t* cur = tp.lanes[l].d_pr[flip ^ 1];
			const uint32_t* score = last && !job.final ? t.scores.data() + j : nullptr;
			if (st.kind == 2) {
				CHECK(tp.use_slots && e_i < ss.entry_count);
				const SlotBatchEntry& e = tp.slot_entries[ss.entry_off + e_i++];
				CHECK(e.pad == st.index && e.run.c0 == tp.splan.runs[st.index].c0 && e.run.spec_id == tp.splan.runs[st.index].spec_id);
				CHECK(e.prev == prev && e.cur == cur && e.score_out == score);
				if (first) CHECK(e.run.has_prev == 0);
				CHECK(e.spec_stride == t.dp.spec_stride && ss.grid_x >= (1u << (e.run.g - e.run.half)) && ss.threads >= e.run.threads);
			} else if (st.kind == 1) {
				CHECK(!tp.use_slots && e_i < ss.entry_count);
				const ResBatchEntry& e = tp.entries[ss.entry_off + e_i++];
				CHECK(e.sg.pad == st.index && e.sg.c0 == tp.plan.segments[st.index].c0);
				CHECK(e.prev == prev && e.cur == cur && e.score_out == score);
				if (first) CHECK(e.sg.has_prev == 0);
			} else {
				CHECK(single_i < ss.singles.size());
				const Single& sg = ss.singles[single_i++];
				CHECK(sg.lane == l && sg.step == job.steps[k] && sg.flip == flip && sg.zero_prev == first && sg.score_job == (last && !job.final ? (int32_t)j : -1));
			}
		}
		CHECK(e_i == ss.entry_count && single_i == ss.singles.size());
		n_entries += ss.entry_count;
		widest = std::max(widest, ss.grid_x * std::max(1u, ss.entry_count));
	}
	CHECK(n_entries == (tp.use_slots ? tp.slot_entries.size() : tp.entries.size()) && widest == tp.max_grid_x);
	if (!tp.windowed) {
		CHECK(tp.schedule.size() == first_pass);
		for (const SuperStep& ss : tp.schedule) CHECK(ss.ck_load == -1 && ss.ck_save == -1 && ss.bt_window == -1);
	} else {
		// pass 1 keeps the column at every boundary and walks the newest window; then the older windows again, newest first
		const size_t nw = tp.windows.size();
		std::vector<int32_t> save(first_pass, -1);
		for (size_t wi = 0; wi + 1 < nw; ++wi) save[tp.windows[wi].step_hi - 1] = (int32_t)wi;
		for (size_t s = 0; s < first_pass; ++s)
			CHECK(tp.schedule[s].ck_load == -1 && tp.schedule[s].ck_save == save[s] && tp.schedule[s].bt_window == (s + 1 == first_pass ? (int32_t)(nw - 1) : -1));
		size_t at = first_pass;
		for (size_t wi = nw - 1; wi-- > 0;) {
			const Window& w = tp.windows[wi];
			for (uint32_t pos = w.step_lo; pos < w.step_hi; ++pos, ++at) {
				CHECK(at < tp.schedule.size());
				const SuperStep& again = tp.schedule[at];
				const SuperStep& was = tp.schedule[pos];
				CHECK(again.entry_off == was.entry_off && again.entry_count == was.entry_count && again.singles.size() == was.singles.size() && again.io[0] == was.io[0] && again.io[1] == was.io[1]);
				CHECK(again.ck_save == -1 && again.ck_load == (pos == w.step_lo && wi > 0 ? (int32_t)(wi - 1) : -1) && again.bt_window == (pos + 1 == w.step_hi ? (int32_t)wi : -1));
			}
		}
		CHECK(at == tp.schedule.size());
	}
	// the briefs of a group submission
	if (!tp.use_slots) { CHECK(tp.step_brief.empty() && tp.entry_brief.empty()); return true; }
	CHECK(tp.step_brief.size() == tp.schedule.size());
	size_t eb_i = 0;
	for (size_t s = 0; s < tp.schedule.size(); ++s) {
		const SuperStep& ss = tp.schedule[s];
		const StepBrief& sb = tp.step_brief[s];
		CHECK(sb.entry_off == eb_i && sb.lds == ss.lds && sb.entry_count == ss.entry_count && sb.has_singles == (ss.singles.empty() ? 0 : 1));
		for (uint32_t q = 0; q < ss.entry_count; ++q, ++eb_i) {
			const SlotBatchEntry& e = tp.slot_entries[ss.entry_off + q];
			const EntryBrief& eb = tp.entry_brief[eb_i];
			const GroupVariantPair v = group_variants_of(e, tp.splan.ped);
			CHECK(eb.grid_x == (1u << (e.run.g - e.run.half)) && eb.threads == e.run.threads && eb.variant.plain == v.plain && eb.variant.x == v.x);
		}
	}
	CHECK(eb_i == tp.entry_brief.size());
	return true;
}

static bool check_all(const Problem& p, const Table& t) {
	return check_records(p, t) && check_jobs_and_units(p, t) && check_chunks(t) && check_schedule(t);
}

static bool single_tables() {
	// the shortest table whose plan has more steps than two chunks' worth
	g_case = "single individual, coverage 8";
	uint32_t n = 600;
	for (;; n += 100) {
		Problem p;
		Table t;
		CHECK(make_problem(n, 8, 1, false, p) && plan_table(p, t));
		if (t.tp.plan.steps.size() > 2u * BT_CHUNK_RUNS + 4) break;
		CHECK(n < 4000);
	}
	Problem p;
	CHECK(make_problem(n, 8, 1, false, p));
	uint64_t sum = 0, largest = 0;
	{
		Table t;
		CHECK(plan_table(p, t) && build_table(p, t) && t.status == WHAMD_OK);
		CHECK(t.tp.use_slots && !t.tp.splan.ped && t.tp.plan.component_first_step.size() == 1);
		CHECK(t.tp.use_chunks && t.tp.chunks.size() >= 3 && !t.tp.windowed && t.tp.jobs.size() == 1 && t.tp.lanes.size() == 1);
		CHECK(check_all(p, t));
		for (uint32_t si = 0; si < t.tp.plan.steps.size(); ++si) { const StepFacts f = facts_of(p, t, si); sum += f.bytes; largest = std::max(largest, f.bytes); }
		PreviewPlan pp;   // one plan piece: no preview, whatever the options
		t.opt.preview_mode = 1;
		plan_preview(p, t.opt, t.b, t.tp, true, true, pp);
		CHECK(pp.why == PV_FEW_PIECES);
	}
	{
		g_case = "single individual, arena of a third of the records";
		Table t;
		t.opt.arena_limit = sum / 3;
		CHECK(plan_table(p, t) && build_table(p, t) && t.status == WHAMD_OK);
		CHECK(t.tp.windowed && t.tp.windows.size() >= 3 && !t.tp.use_chunks && t.b.arena_cap == sum / 3);
		CHECK(check_all(p, t));
	}
	{
		g_case = "single individual, arena one byte below the largest record";
		Table t;
		t.opt.arena_limit = largest - 1;
		CHECK(plan_table(p, t) && build_table(p, t));
		CHECK(t.status == WHAMD_ERR_UNSUPPORTED && !t.msg.empty());
	}
	return true;
}

static bool component_tables() {
	Problem p;
	g_case = "five components";
	CHECK(make_problem(400, 8, 5, false, p));
	for (int lanes : {1, 4}) {
		g_case = lanes == 1 ? "five components, one lane" : "five components, four lanes";
		Table t;
		t.opt.max_lanes = lanes;
		CHECK(plan_table(p, t) && build_table(p, t) && t.status == WHAMD_OK);
		const std::vector<uint32_t>& first = t.tp.plan.component_first_step;
		CHECK(first.size() == 5);
		for (size_t k = 0; k < first.size(); ++k) CHECK(((k + 1 < first.size() ? first[k + 1] : t.tp.plan.steps.size()) - first[k]) * 5 < t.tp.plan.steps.size() * 4);
		CHECK(t.tp.jobs.size() == (lanes == 1 ? 1u : 5u) && t.tp.lanes.size() == (size_t)lanes);
		CHECK(check_all(p, t));
	}
	return true;
}

static bool trio_tables() {
	Problem p;
	g_case = "trio";
	CHECK(make_problem(200, 6, 1, true, p) && p.T == 4 && p.n_ind == 3);
	for (const char* path : {"auto", "resident", "column"}) {
		g_case = path[0] == 'a' ? "trio, pedigree slot runs" : path[0] == 'r' ? "trio, LDS-resident runs" : "trio, per column";
		Table t;
		t.opt.path = path;
		CHECK(plan_table(p, t) && build_table(p, t) && t.status == WHAMD_OK);
		size_t kinds[3] = {0, 0, 0};
		for (const Step& st : t.tp.plan.steps) ++kinds[st.kind];
		if (path[0] == 'a') CHECK(t.b.ped_slots && kinds[2] > 0 && kinds[1] == 0 && !t.tp.slot_entries.empty());
		if (path[0] == 'r') CHECK(!t.tp.use_slots && kinds[1] > 0 && kinds[2] == 0 && !t.tp.entries.empty());
		if (path[0] == 'c') CHECK(kinds[0] == t.tp.plan.steps.size() && t.tp.entries.empty() && t.tp.slot_entries.empty());
		CHECK(check_all(p, t));
	}
	return true;
}

// plan_preview against what lay_out_arena and cut_chunks then produce (what tests/test_preview_plan.py holds through the debug library)
static bool preview_table() {
	Problem p;
	g_case = "preview, nine plan pieces";
	CHECK(make_problem(9 * PLAN_PIECE, 8, 1, false, p) && slot_plan_pieces(p.n_cols) == 9);
	for (uint32_t pieces : {1u, 8u}) {
		Table t;
		t.opt.preview_pieces = pieces;
		CHECK(plan_table(p, t) && t.tp.use_slots);
		PreviewPlan off, pp;
		plan_preview(p, t.opt, t.b, t.tp, true, false, off);   // auto: a table that is not alone has none
		CHECK(off.why == PV_NOT_ALONE);
		plan_preview(p, t.opt, t.b, t.tp, false, true, off);
		CHECK(off.why == PV_NOT_CREATE);
		t.opt.preview_mode = 1;
		plan_preview(p, t.opt, t.b, t.tp, true, false, pp);
		CHECK(pp.why == PV_RAN && pp.pieces == pieces && pp.steps > 0 && pp.steps < t.tp.plan.steps.size());
		CHECK(pp.rec.size() == pp.steps && pp.spec.size() == pp.steps);
		CHECK(build_table(p, t) && t.status == WHAMD_OK && !t.tp.windowed);
		for (uint32_t k = 0; k < pp.steps; ++k) {
			const SlotRun& run = t.tp.splan.runs[t.tp.plan.steps[k].index];
			CHECK(t.tp.plan.steps[k].kind == 2 && pp.rec[k] == (((uint64_t)run.rec_hi << 32) | run.rec_lo) && pp.spec[k] == run.spec_id);
		}
		CHECK(pp.chunked == t.tp.use_chunks && pp.chunked && pp.n_spec == t.tp.n_spec && pp.stride == t.dp.spec_stride && pp.arena == t.b.bt);
		CHECK(((uint64_t)1 << pp.max_f) * p.T * 4 >= t.b.exchange_bytes);
		if (pieces == 1) CHECK(check_all(p, t));
	}
	return true;
}

int main() {
	if (!single_tables() || !component_tables() || !trio_tables() || !preview_table()) return 1;
	std::printf("ok\n");
	return 0;
}
"""


def _compiler():
    for name in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def test_table_plan_program_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    main = tmp_path / "table_plan_check.cpp"
    exe = tmp_path / "table_plan_check"
    main.write_text(PROGRAM)
    # (g++ links the sanitizers' runtimes as shared libraries unless told otherwise; linked in, they start first whatever else the process loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    flags = ["-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-I" + CSRC]
    units = [(str(main), str(tmp_path / "main.o"))] + [(os.path.join(CSRC, s), str(tmp_path / (s + ".o"))) for s in SOURCES]

    def compile_one(unit):
        return subprocess.run([cxx] + flags + ["-c", unit[0], "-o", unit[1]], capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=min(len(units), 6)) as pool:   # (the objects side by side: together they take over a minute one after the other)
        for done in pool.map(compile_one, units):
            assert done.returncode == 0, done.stderr
    subprocess.run([cxx] + flags + static + [u[1] for u in units] + ["-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
