"""The plan checks behind whamd_plan_summarize (check_slot_plan, check_genotype_slot_plan: slot_plan.cpp; check_resident_plan: resident_plan.cpp) and the
LDS size of a resident run (resident.h), on the host alone: a stand-alone C++ program built with the address and undefined-behaviour sanitizers plans small
tables and holds the checks against them.  Nothing is loaded into Python and no device is needed.

Tables (the generator of test_table_plan_host.py): a single individual at coverage 13, 300 columns in three components, planned as slot runs and as
LDS-resident runs; a trio at coverage 8, 200 columns, planned as pedigree slot runs and as resident runs; the single individual's plan in genotype mode.

1. Every check accepts the planner's own plan, and the summary it fills agrees with the plan (steps, runs, columns in runs, the largest run, the largest
   LDS request restated from the size functions).
2. Every check can fail: one field of a fresh copy of the plan is changed at a time, every index staying in range, and the check must return false --
   a run one column longer, two columns' rows swapped, a backtrace column's count of earlier ending reads, a slot used twice, an ending read's slot, a
   component boundary dropped, a resident column's record offset, a run's record size, a column's entering width, a resident run that holds the table's
   last column, and (genotype mode) the count of reads started earlier in the run.
   One hole is known and printed, not asserted: check_resident_plan skips its component test when the list is EMPTY (a trio's plan has none), so a
   single-component table whose only boundary is dropped passes; with several components a dropped boundary is caught.
3. res_segment_lds_bytes equals the arithmetic written out for a hand-computed segment of each kind (a trio run with an odd, an even and a padded term
   count), and the planner's budget test on running totals (ped_run_lds_bound, res_run_lds_bytes against RUN_LDS_BUDGET) decides as the expressions
   that stood in plan_forward at 153 576, 153 584, 153 592 and 153 600 unpadded bytes, for either parity of the term count.
4. Every resident run of the two tables asks for at most CU_LDS_BYTES.

Time: about 20 s, nearly all of it the compiler with both sanitizers (the units are compiled side by side)."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_table_plan_host import CSRC, PROGRAM as TABLE_PROGRAM, _compiler

SOURCES = ["problem.cpp", "slot_plan.cpp", "resident_plan.cpp"]

# the problem generator of test_table_plan_host.py: `struct Input` and make_problem(n, coverage, components, trio, p)
_GEN_BEGIN = TABLE_PROGRAM.index("// ---- problems:")
_GEN_END = TABLE_PROGRAM.index("// ---- a table,")
GENERATOR = TABLE_PROGRAM[_GEN_BEGIN:_GEN_END]

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>

#include "resident.h"
#include "slots.h"

using namespace whamd;

#define CHECK(cond)                                                                      \
	do {                                                                                 \
		if (!(cond)) {                                                                   \
			std::printf("%s, line %d: %s does not hold\n", g_case, __LINE__, #cond);     \
			return false;                                                                \
		}                                                                                \
	} while (0)

static const char* g_case = "";

""" + GENERATOR + r"""
// ---- 1 + 2 + 4: slot plans (single individual, pedigree)
static bool must_fail_slots(const Problem& p, const SlotPlan& sp, const char* what, const std::function<void(SlotPlan&)>& corrupt) {
	g_case = what;
	SlotPlan bad = sp;
	corrupt(bad);
	whamd_plan_summary s;
	CHECK(!check_slot_plan(p, bad, s) && s.invariants_ok == 0);
	return true;
}

static bool slot_checks(const Problem& p, const SlotPlan& sp, bool ped) {
	whamd_plan_summary s;
	CHECK(check_slot_plan(p, sp, s) && s.invariants_ok == 1 && sp.ped == ped);
	uint64_t in_runs = 0, longest = 0, lds = 0;
	for (size_t ri = 0; ri < sp.runs.size(); ++ri) {
		const SlotRun& run = sp.runs[ri];
		in_runs += run.ncols;
		longest = std::max<uint64_t>(longest, run.ncols);
		lds = std::max<uint64_t>(lds, ped ? pedslot_lds_bytes(run.threads, run.ncols, sp.pextra[ri]) : slot_run_lds_bytes(run.threads, run.lr, run.ncols));
	}
	CHECK(s.n_columns == p.n_cols && s.max_coverage == p.max_k && s.n_steps == sp.steps.size() && s.n_runs == sp.runs.size());
	CHECK(s.n_resident_columns == in_runs && in_runs == sp.n_run_columns && s.max_run_columns == longest && s.max_lds_bytes == lds && lds <= CU_LDS_BYTES);
	CHECK(s.n_components == sp.component_first_step.size() && (ped || s.n_components == 3));
	// a run followed by another run, with reads ending in it; a column of it (not its first) with two reads and more
	size_t si = 0;
	while (si + 1 < sp.steps.size() && !(sp.steps[si].kind == 2 && sp.steps[si + 1].kind == 2 && sp.runs[sp.steps[si].index].n_ends > 0)) ++si;
	CHECK(si + 1 < sp.steps.size());
	const uint32_t ri = sp.steps[si].index;
	const SlotRun run = sp.runs[ri];
	const uint32_t row = run.row_off + 1;
	CHECK(run.ncols >= 2 && sp.bt_cols[row].k >= 2 && sp.col_to_row[run.c0] >= 0 && sp.col_to_row[run.c0] != sp.col_to_row[run.c0 + 1]);
	CHECK(must_fail_slots(p, sp, "slot run one column longer", [&](SlotPlan& b) { b.runs[ri].ncols += 1; }));
	CHECK(must_fail_slots(p, sp, "two entries of col_to_row swapped", [&](SlotPlan& b) { std::swap(b.col_to_row[run.c0], b.col_to_row[run.c0 + 1]); }));
	CHECK(must_fail_slots(p, sp, "SlotBtCol::kf one more", [&](SlotPlan& b) { b.bt_cols[row].kf += 1; }));
	if (sp.bt_cols[row].kf > 0) CHECK(must_fail_slots(p, sp, "SlotBtCol::kf one less", [&](SlotPlan& b) { b.bt_cols[row].kf -= 1; }));
	CHECK(must_fail_slots(p, sp, "a slot used twice in SlotBtCol::slot", [&](SlotPlan& b) { b.bt_cols[row].slot[1] = b.bt_cols[row].slot[0]; }));
	CHECK(must_fail_slots(p, sp, "a byte of end_slots changed", [&](SlotPlan& b) { b.end_slots[b.end_off[ri]] ^= 1u; }));
	if (!ped) CHECK(must_fail_slots(p, sp, "a component boundary dropped", [&](SlotPlan& b) { b.component_first_step.erase(b.component_first_step.begin() + 1); }));
	return true;
}

// ---- 1 + 2 + 4: resident plans (single individual, trio)
static bool must_fail_resident(const Problem& p, const ResidentPlan& plan, const char* what, const std::function<void(ResidentPlan&)>& corrupt) {
	g_case = what;
	ResidentPlan bad = plan;
	corrupt(bad);
	whamd_plan_summary s;
	CHECK(!check_resident_plan(p, bad, s) && s.invariants_ok == 0);
	return true;
}

static bool resident_checks(Problem& p, const ResidentPlan& plan, bool trio) {
	whamd_plan_summary s;
	CHECK(check_resident_plan(p, plan, s) && s.invariants_ok == 1);
	uint64_t in_runs = 0, longest = 0, lds = 0;
	for (const ResSegment& sg : plan.segments) {
		CHECK(sg.kind == (trio ? 1u : 0u));
		in_runs += sg.ncols;
		longest = std::max<uint64_t>(longest, sg.ncols);
		lds = std::max<uint64_t>(lds, res_segment_lds_bytes(sg));
		CHECK(res_segment_lds_bytes(sg) <= CU_LDS_BYTES);   // (4)
	}
	CHECK(!plan.segments.empty() && s.n_columns == p.n_cols && s.max_coverage == p.max_k && s.n_steps == plan.steps.size() && s.n_runs == plan.segments.size());
	CHECK(s.n_resident_columns == in_runs && in_runs == plan.n_resident_columns && s.max_run_columns == longest && s.max_lds_bytes == lds);
	CHECK(s.n_components == plan.component_first_step.size() && s.n_components == (trio ? 0u : 3u));
	// a run followed by another run
	size_t si = 0;
	while (si + 1 < plan.steps.size() && !(plan.steps[si].kind == 1 && plan.steps[si + 1].kind == 1)) ++si;
	CHECK(si + 1 < plan.steps.size());
	const uint32_t gi = plan.steps[si].index;
	const ResSegment sg = plan.segments[gi];
	const uint32_t col = sg.col_off + 1;
	CHECK(must_fail_resident(p, plan, "resident run one column longer", [&](ResidentPlan& b) { b.segments[gi].ncols += 1; }));
	CHECK(must_fail_resident(p, plan, "two entries of col_to_res swapped", [&](ResidentPlan& b) { std::swap(b.col_to_res[sg.c0], b.col_to_res[sg.c0 + 1]); }));
	CHECK(must_fail_resident(p, plan, "ResColumn::stage_off one more", [&](ResidentPlan& b) { b.columns[col].stage_off += 1; }));
	CHECK(must_fail_resident(p, plan, "ResSegment::stage_words one more", [&](ResidentPlan& b) { b.segments[gi].stage_words += 1; }));
	if (sg.stage_words > 0) CHECK(must_fail_resident(p, plan, "ResSegment::stage_words one less", [&](ResidentPlan& b) { b.segments[gi].stage_words -= 1; }));
	CHECK(must_fail_resident(p, plan, "ResColumn::Lb one more", [&](ResidentPlan& b) { b.columns[col].Lb += 1; }));
	if (plan.columns[col].Lb > 0) CHECK(must_fail_resident(p, plan, "ResColumn::Lb one less", [&](ResidentPlan& b) { b.columns[col].Lb -= 1; }));
	if (!trio) {
		CHECK(must_fail_resident(p, plan, "a component boundary dropped", [&](ResidentPlan& b) { b.component_first_step.erase(b.component_first_step.begin() + 1); }));
		ResidentPlan none = plan;   // the known hole: an EMPTY list switches the component test off
		none.component_first_step.clear();
		whamd_plan_summary s2;
		std::printf("finding: check_resident_plan %s a plan whose component list was emptied\n", check_resident_plan(p, none, s2) ? "accepts" : "refuses");
	}
	{   // the table ends where the run ends: the run holds the last column (every array keeps its size, so every index stays in range)
		g_case = "a resident run that contains the last column";
		ResidentPlan bad = plan;
		bad.steps.resize(si + 1);
		while (!bad.component_first_step.empty() && bad.component_first_step.back() > si) bad.component_first_step.pop_back();
		const uint32_t n = p.n_cols;
		p.n_cols = sg.c0 + sg.ncols;
		whamd_plan_summary s3;
		const bool accepted = check_resident_plan(p, bad, s3);
		p.n_cols = n;
		CHECK(!accepted && s3.invariants_ok == 0);
	}
	return true;
}

// ---- 1 + 2: the genotyper's run plan
static bool genotype_checks(const Problem& p) {
	g_case = "genotype mode";
	SlotPlan sp;
	CHECK(plan_forward_slots(p, 0, 0, sp, 0, /*genotype_mode=*/true));
	whamd_plan_summary s;
	CHECK(check_genotype_slot_plan(p, sp, s) && s.invariants_ok == 1);
	uint64_t in_runs = 0;
	for (const SlotRun& run : sp.runs) in_runs += run.ncols;
	CHECK(s.n_columns == p.n_cols && s.n_steps == sp.steps.size() && s.n_runs == sp.runs.size() && s.n_resident_columns == in_runs && in_runs > 0);
	size_t ri = 0;
	while (ri < sp.runs.size() && sp.runs[ri].ncols < 2) ++ri;
	CHECK(ri < sp.runs.size());
	g_case = "PedSlotRow::pad[1] one more";
	SlotPlan bad = sp;
	bad.prows[sp.runs[ri].c0 + 1].pad[1] += 1;
	CHECK(!check_genotype_slot_plan(p, bad, s) && s.invariants_ok == 0);
	return true;
}

// ---- 3: the size functions against the arithmetic, and the planner's budget test against the expressions it replaces
static bool lds_sizes() {
	g_case = "LDS of a resident run";
	ResSegment one{};   // 5 columns of (64 + 256) words, two slices of 2^9 u32, 37 u64 of record
	one.kind = 0; one.ncols = 5; one.max_l = 9; one.stage_words = 37;
	CHECK(res_segment_lds_bytes(one) == 6400 + 4096 + 296);
	ResSegment trio{};  // 3 columns of (80 + 384) words and 7 terms of 2 words = 1406 words, padded to 1408; two slices of 2^6 x 16 bytes; 11 u64 of record
	trio.kind = 1; trio.ncols = 3; trio.n_terms = 7; trio.max_l = 6; trio.stage_words = 11;
	CHECK(res_segment_lds_bytes(trio) == 5632 + 2048 + 88);
	trio.n_terms = 6;   // 1404 words: no padding
	CHECK(res_segment_lds_bytes(trio) == 5616 + 2048 + 88);
	trio.n_terms = 5;   // 1402 words, padded to 1404
	CHECK(res_segment_lds_bytes(trio) == 5616 + 2048 + 88);
	CHECK(ped_slice_word<uint32_t>(3, 7) == 1408 && res_slice_word<uint32_t>(5) == 1600);
	g_case = "the planner's LDS budget";
	CHECK(RUN_LDS_BUDGET == 153600 && CU_LDS_BYTES == 163840);
	const uint64_t raws[5] = {153576, 153584, 153592, 153600, 153608};
	for (uint64_t raw : raws) {
		for (uint64_t n_terms : {20u, 21u}) {   // trio: 40 columns and two slices of 2^10 entries are 107 008 bytes, terms and record make up the rest
			const uint64_t ncols = 40, run_max_l = 10, run_stage = (raw - 107008) / 8 - n_terms;
			const uint64_t lds_bytes = ncols * (PED_LDSWORDS + PED_TABLE) * 4 + n_terms * 8 + 2 * (16ull << run_max_l) + run_stage * 8 + 16;   // (as it stood in plan_forward)
			CHECK(lds_bytes == raw + 16);
			const bool ends_run = lds_bytes > 150 * 1024;
			CHECK(ends_run == (ped_run_lds_bound(ncols, n_terms, (uint32_t)run_max_l, run_stage) > RUN_LDS_BUDGET) && ends_run == (raw >= 153592));
			const uint64_t launched = ped_run_lds_bytes(ncols, n_terms, (uint32_t)run_max_l, run_stage);
			CHECK(launched == raw + (n_terms & 1u) * 8);
			if (!ends_run) CHECK(launched <= RUN_LDS_BUDGET - 8 && launched <= CU_LDS_BYTES);
		}
		{   // single individual: 40 columns and two slices of 2^13 entries are 116 736 bytes
			const uint64_t ncols = 40, run_max_l = 13, run_stage = (raw - 116736) / 8;
			const uint64_t lds_bytes = ncols * (64 + RES_TABLE) * 4 + 2 * (4ull << run_max_l) + run_stage * 8;   // (as it stood in plan_forward)
			CHECK(lds_bytes == raw);
			const bool ends_run = lds_bytes > 150 * 1024;
			CHECK(ends_run == (res_run_lds_bytes(ncols, (uint32_t)run_max_l, run_stage) > RUN_LDS_BUDGET) && ends_run == (raw > 153600));
		}
	}
	return true;
}

int main() {
	Problem single, trio;
	g_case = "single individual, coverage 13";
	if (!make_problem(300, 13, 3, false, single)) return 1;
	g_case = "trio, coverage 8";
	if (!make_problem(200, 8, 1, true, trio) || trio.T != 4 || trio.n_ind != 3) return 1;
	SlotPlan sp, psp;
	ResidentPlan rp, prp;
	if (!plan_forward_slots(single, 11, 1, sp) || !plan_forward_slots(trio, 11, 1, psp)) { std::printf("not eligible for slot runs\n"); return 1; }
	plan_forward(single, true, 11, true, rp);
	plan_forward(trio, true, 11, true, prp);
	g_case = "single individual, slot runs";
	if (!slot_checks(single, sp, false)) return 1;
	g_case = "trio, pedigree slot runs";
	if (!slot_checks(trio, psp, true)) return 1;
	g_case = "single individual, resident runs";
	if (!resident_checks(single, rp, false)) return 1;
	g_case = "trio, resident runs";
	if (!resident_checks(trio, prp, true)) return 1;
	if (!genotype_checks(single) || !lds_sizes()) return 1;
	std::printf("ok\n");
	return 0;
}
"""


def test_plan_checks_program_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    main = tmp_path / "plan_checks.cpp"
    exe = tmp_path / "plan_checks"
    main.write_text(PROGRAM)
    # (g++ links the sanitizers' runtimes as shared libraries unless told otherwise; linked in, they start first whatever else the process loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    flags = ["-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-I" + CSRC]
    units = [(str(main), str(tmp_path / "main.o"))] + [(os.path.join(CSRC, s), str(tmp_path / (s + ".o"))) for s in SOURCES]

    def compile_one(unit):
        return subprocess.run([cxx] + flags + ["-c", unit[0], "-o", unit[1]], capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=len(units)) as pool:
        for done in pool.map(compile_one, units):
            assert done.returncode == 0, done.stderr
    subprocess.run([cxx] + flags + static + [u[1] for u in units] + ["-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok"
