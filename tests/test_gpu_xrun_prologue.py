"""GPU (-m gpu): every way into and out of an X run's prologue (kernels_slots.h slot_runx_arguments / slot_runx_lds_core / slot_runx_stream_core / slot_enter_cells), each against the
oracle in full -- cost, index path, partitioning, superreads -- with the debug library's launch ledger asserting that the intended kernel ran
(tests/test_gpu_kernel_choice.py: solve_and_check / solve_many_and_check and the rule the ledger is held to).

The kernel arguments of `slot_runx<2, XC > 0, ...>` are fetched by hand in one group: a word the group forgets, or takes from the wrong offset, is a wrong
result in exactly one of the cases below -- `pack` (narrow runs on one XCD), the halved runs' mirrored entry and the flip of its cells, a run without a
previous column, the D-form entry, the general entry layout with its own load of `in_pos`, the exit's words (`out_pos`, `cur`, `score_out`), the record
pointer (`P.bt`), the rows of a third ending read (`P.slot_rows`), the speculative seed (`P.spec_keys`).
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


@pytest.mark.parametrize("coverage,workgroups", [(12, 1), (13, 2), (17, 32)])
def test_narrow_runs_packed_onto_one_xcd(coverage, workgroups):
    """`pack` non-zero: eight times the grid, every eighth workgroup works (the others leave behind the one wait); halved runs, the mirrored entry."""
    p = flagship_like(coverage)
    summary = _native.plan_summary(p)
    assert summary["n_halved_runs"] > 0 and summary["max_workgroups"] == workgroups, summary   # (the flip of the entering cells is exercised)
    names, _ = solve_and_check(p, ("xrun prologue", coverage))
    recs = x_records()
    assert recs and all(r["pack"] == 1 and not r["streamed"] for r in recs), recs
    assert max(r["grid_x"] for r in recs) == 8 * workgroups, recs
    assert any(n.startswith("slot_runx<2, 24,") for n in names), names


def test_wide_runs_one_workgroup_per_cu():
    """No `pack`: coverage 18, 64 workgroups."""
    p = flagship_like(18)
    summary = _native.plan_summary(p)
    assert summary["n_halved_runs"] > 0 and summary["max_workgroups"] == 64, summary
    names, _ = solve_and_check(p, ("xrun prologue", 18))
    recs = x_records()
    wide = [r for r in recs if r["grid_x"] == 64]   # (the table's first runs are narrower: few reads yet)
    assert wide and all(r["pack"] == 0 and not r["streamed"] for r in wide) and max(r["grid_x"] for r in recs) == 64, recs
    assert any(r["name"].startswith("slot_runx<2, 24,") for r in wide), wide


def test_a_run_without_a_previous_column_and_the_d_form_entry():
    """Two connected components in one table: the second one's first run has no `prev`, and the run behind a component's per-column step enters in D form
    (yflags bit 1 clear) through the general layout -- the one load through the kernel-argument pointer that is not in the group, `in_pos`.  The second
    component is clipped so that its last run is a short one."""
    p = clip_to_columns(components(2, 60, 13, seed=11), 60 + 47)
    summary = _native.plan_summary(p)
    assert summary["n_components"] == 2 and summary["n_steps"] > summary["n_runs"] and summary["n_halved_runs"] > 0, summary
    names, stats = solve_and_check(p, ("xrun prologue components", 13), lanes=1)   # (one lane: the components one behind the other, every run a launch of its own)
    recs = x_records()
    assert recs and any(not (r["yflags"] & 2) for r in recs) and any(r["yflags"] & 2 for r in recs), recs   # (D-form and Y-form entries)
    assert any(r["site"] == "column" and r["forward"] for r in LAST_LEDGER), LAST_LEDGER                     # (a per-column step among the runs)
    assert len({r["name"] for r in recs}) >= 2, recs                                                        # (the clipped component's short run: another XC)


def test_short_runs_of_an_irregular_layout():
    """`slot_runx<2, 8, ...>` and `<2, 16, ...>`: runs that end when the first grid read does; third and later ending reads come from the rows."""
    p = irregular_block(120, 16, seed=7)
    assert _native.plan_summary(p)["n_halved_runs"] > 0
    names, _ = solve_and_check(p, ("xrun prologue irregular", 120, 16, 7))
    assert {"slot_runx<2, 8, false, false>", "slot_runx<2, 16, false, false>"} <= names, sorted(names)


def test_a_run_that_ends_a_backtrace_chunk():
    """SPEC: a table long enough for the chunked backtrace -- the runs that end a chunk leave the seed of the speculative walk."""
    p = synthetic_block(900, 12, seed=61, step=1)
    names, stats = solve_and_check(p, ("xrun prologue spec", 900))
    assert stats["bt_chunks"] > 0, stats
    spec = [r for r in x_records() if r["spec"]]
    assert spec and all(r["name"].endswith("true>") and not r["name"].startswith("slot_runx<2, 0,") for r in spec), x_records()


def test_the_same_problems_sharing_their_launches():
    """`slot_groupx<2>` (streamed operands, slot_runx_stream_core<2>: the flip as four selects, the entry read from memory)."""
    members = [(("xrun prologue", c), flagship_like(c), {"shared_launches": 1}) for c in (12, 13, 17, 18)]
    names, stats = solve_many_and_check(members)
    assert all(s["group_tables"] > 1 for s in stats), stats
    assert all("slot_groupx<2, false>" in n for n in names[:3]), names
    assert "slot_groupx<3, false>" in names[3], names   # (a wide table that shares its launches holds eight cells per thread: slot_runx_stream_core<3>)


def ending_reads_per_column(p):
    """How many reads end in each column, from the problem's arrays (the last entry of a read is its last column; positions are 1000 * (column + 1))."""
    last = np.asarray(p.var_position)[np.asarray(p.read_ptr[1:], dtype=np.int64) - 1] // 1000 - 1
    return np.bincount(last, minlength=p.n_variants)


def test_third_and_later_ending_reads_sharing_their_launches():
    """The walk over a column's ending reads is one text for four and for eight cells per thread (slotx_later_endings, slot_runx_stream_core<2 | 3>): the
    third and later ones come from the row, and their decode differs between the two by the width of the qmask alone -- wrong only in a column where three
    or more reads end.  Irregular tables (seeds chosen on the host so that each has such columns), two narrow and two wide, sharing their launches."""
    shapes = [(120, 16, 7), (120, 16, 5), (150, 18, 7), (200, 18, 9)]   # (columns, coverage, seed)
    members = [(("xrun irregular shared",) + s, irregular_block(s[0], s[1], seed=s[2]), {"shared_launches": 1}) for s in shapes]
    for key, p, _ in members:
        ends = ending_reads_per_column(p)
        assert (ends[:-1] >= 3).any(), (key, ends.max())   # (a column before the table's last: the last one ends every read that is left)
    names, stats = solve_many_and_check(members)
    assert all(s["group_tables"] > 1 for s in stats), stats
    assert all("slot_groupx<2, false>" in n for n in names[:2]), names
    assert all("slot_groupx<3, false>" in n for n in names[2:]), names
