"""GPU (-m gpu): every way out of an X run (kernels_slots.h slot_exit_cells and its parts, slot_runx_lds_core, slot_runx_stream_core, slot_runx_exit / slot_runx_exit_early), each against the oracle in full
-- cost, index path, partitioning, superreads -- with the debug library's launch ledger asserting that the intended kernel ran
(tests/test_gpu_kernel_choice.py: solve_and_check / solve_many_and_check and the rule the ledger is held to).

`slot_runx<2, XC > 0, ...>` forms the exit index of every thread in its PROLOGUE and carries it through the column loop in one register, with the store
form in one scalar; behind the loop only the store is left.  A wrong bit of that index, a thread that writes where it must not, a store form that takes
the 16-byte path for a general layout, or a seed of the speculative walk with the wrong index is a wrong result in one of the cases below.  The kernels
that share their launches (`slot_groupx`) run both parts back to back behind the loop, as before.

The problems are the small ones of tests/test_gpu_xrun_prologue.py (same keys: the oracle's solutions are computed once per session and shared).
"""
import numpy as np
import pytest

from test_gpu_kernel_choice import LAST_LEDGER, components, solve_and_check, solve_many_and_check
from whatshap_amd import _native
from whatshap_amd.synthetic import clip_to_columns, irregular_block, synthetic_block

pytestmark = pytest.mark.gpu


def x_records():
    """The ledger lines of the table solved last that are X runs of four cells per thread launched on their own."""
    return [r for r in LAST_LEDGER if r["site"] == "slot_run" and not r["ped"] and (r["yflags"] & 8) and r["lr"] == 2]


def flagship_like(coverage):
    return synthetic_block(96, coverage, seed=40 + coverage)


def two_components():
    return clip_to_columns(components(2, 60, 13, seed=11), 60 + 47)


def coverage_of(p, column):
    """Reads whose span covers `column` (physical coverage, from the problem's own arrays)."""
    ptr = p.read_ptr.astype(np.int64)
    first, last = p.var_position[ptr[:-1]], p.var_position[ptr[1:] - 1]
    x = p.positions[column]
    return int(((first <= x) & (last >= x)).sum())


@pytest.mark.parametrize("coverage,workgroups", [(12, 1), (13, 2), (17, 32), (18, 64)])
def test_halved_runs_and_the_mirror_store(coverage, workgroups):
    """1, 2, 32 and 64 workgroups, packed onto one XCD (up to 32) and not.  The runs are halved (only half of the mirror pairs is computed); the last run
    of the table stores every group of four twice, the second time at the complement index in reverse order (`mirror_out`), for the per-column step
    behind it -- the 16-byte store and its mirror from the carried index."""
    p = flagship_like(coverage)
    summary = _native.plan_summary(p)
    assert summary["n_halved_runs"] > 0 and summary["max_workgroups"] == workgroups, summary
    names, _ = solve_and_check(p, ("xrun prologue", coverage))
    recs = x_records()
    assert recs and all(not r["streamed"] for r in recs), recs
    widest = [r for r in recs if (r["grid_x"] // 8 if r["pack"] else r["grid_x"]) == workgroups]   # (the table's first runs are narrower: few reads yet)
    assert widest and all(bool(r["pack"]) == (workgroups <= 32) for r in widest), recs
    assert any(n.startswith("slot_runx<2, 24,") for n in names), names
    assert any(r["site"] == "column" and r["forward"] for r in LAST_LEDGER), LAST_LEDGER   # (the per-column step that reads the mirrored exit)


def test_an_exit_that_converts_to_d_form_and_one_that_does_not():
    """Two connected components in one table, one lane.  A run in front of another Y-form run leaves its cells as they are (yflags bit 2 set); the run in front
    of a component's per-column step converts Y back to D (bit 2 clear).  The clipped component's last run is a short one: another XC."""
    p = two_components()
    summary = _native.plan_summary(p)
    assert summary["n_components"] == 2 and summary["n_steps"] > summary["n_runs"] and summary["n_halved_runs"] > 0, summary
    names, _ = solve_and_check(p, ("xrun prologue components", 13), lanes=1)
    recs = x_records()
    assert recs and any(r["yflags"] & 4 for r in recs) and any(not (r["yflags"] & 4) for r in recs), recs
    assert any(r["site"] == "column" and r["forward"] for r in LAST_LEDGER), LAST_LEDGER
    assert len({r["name"] for r in recs}) >= 2, recs


def test_threads_that_do_not_write():
    """A free local slot at the exit: the threads with a set bit there hold no representative and store nothing -- their carried index is all ones.

    Which run: the last run of the clipped second component above, columns 97 .. 105 (nine columns: the `<2, 16, ...>` kernel).  It enters with 13 reads in
    its 13 slots (11 local, 2 grid); four of them end inside it and no read starts, so the per-column step behind it (column 106) has 9 reads.  The planner
    marks a slot occupied at the exit only where a read lives on behind the run's last column (slot_plan.cpp: `out_occ` from `exit_read[s] >= 0`), so four
    slots are free.  Neither the plan summary nor the ledger names them; the debug library's plan dump (WHAMD_DEBUG_PLAN) prints `out_occ=1f8d` with
    `L=11` for this run: lane slots 4, 5, 6 and reg slot 1 are free -- seven threads of eight store nothing, and the others store two of their four cells,
    cell by cell (the general store path, with the mirror image).  What the test can see for itself is asserted: the run, and the two coverages."""
    p = two_components()
    assert coverage_of(p, 96) == 13 and coverage_of(p, 105) == 13 and coverage_of(p, 106) == 9, [coverage_of(p, c) for c in (96, 105, 106)]
    names, _ = solve_and_check(p, ("xrun prologue components", 13), lanes=1)
    short = [r for r in x_records() if r["ncols"] == 9]
    assert len(short) == 1 and short[0]["name"] == "slot_runx<2, 16, false, false>" and not (short[0]["yflags"] & 4), x_records()


def test_short_runs_and_the_general_store_path():
    """An irregular layout: runs that end when the first grid read does, exits whose reg slots' reads are not the two lowest bits of the exit index or are
    free (cell by cell), free wave slots (the plan dump: `out_occ=f8ff` with `L=11` behind columns 37 .. 50 -- only wave 0 stores)."""
    p = irregular_block(120, 16, seed=7)
    assert _native.plan_summary(p)["n_halved_runs"] > 0
    names, _ = solve_and_check(p, ("xrun prologue irregular", 120, 16, 7))
    assert {"slot_runx<2, 8, false, false>", "slot_runx<2, 16, false, false>"} <= names, sorted(names)


XC32_COVERAGE = 8


def test_a_run_of_up_to_32_columns():
    """XC = 32.  The input was found on the host: `plan_summary` of `irregular_block(n, coverage, seed)` for n = 26, 27, ... (a run longer than 24 columns
    needs 26: the table's last column is a per-column step), coverage 8 .. 16, seed 1 .. 8, first hit with 24 < max_run_columns <= 32 -- n = 26, where
    coverage 8 .. 11 and seed 1 give one run of 25 columns, all of them through the X kernel of four cells per thread (ledger); the lowest coverage is used."""
    p = irregular_block(26, XC32_COVERAGE, seed=1)
    summary = _native.plan_summary(p)
    assert summary["max_run_columns"] == 25 and summary["n_runs"] == 1, summary
    names, _ = solve_and_check(p, ("xrun exit 32", 26, XC32_COVERAGE, 1))
    assert "slot_runx<2, 32, false, false>" in names, sorted(names)
    assert [r["ncols"] for r in x_records()] == [25], x_records()


def test_the_seed_of_the_speculative_walk():
    """SPEC: a table long enough for the chunked backtrace -- the runs that end a chunk leave the seed of the speculative walk, whose index is the carried
    exit index + the cell's number.  (A wrong seed is still exact -- the walk from it is verified -- so the result alone cannot show it; a wrong INDEX
    of the seed's cell store would.  No debug switch is set: the solve is the product's.)"""
    p = synthetic_block(900, 12, seed=61, step=1)
    names, stats = solve_and_check(p, ("xrun prologue spec", 900))
    assert stats["bt_chunks"] > 0, stats
    spec = [r for r in x_records() if r["spec"]]
    assert spec and all(r["name"].endswith("true>") and not r["name"].startswith("slot_runx<2, 0,") for r in spec), x_records()


def test_the_same_problems_sharing_their_launches():
    """`slot_groupx<2>` / `<3>`: both parts of the exit back to back behind the loop, device code as it was."""
    members = [(("xrun prologue", c), flagship_like(c), {"shared_launches": 1}) for c in (12, 13, 17, 18)]
    names, stats = solve_many_and_check(members)
    assert all(s["group_tables"] > 1 for s in stats), stats
    assert all("slot_groupx<2, false>" in n for n in names[:3]), names
    assert "slot_groupx<3, false>" in names[3], names
