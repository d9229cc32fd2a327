"""GPU (-m gpu): the preview of a lone single-individual table (options `preview` / `preview_pieces`) -- whamd_dptable_create launches the
table's leading slot runs itself and the first solve continues behind them.  Whatever becomes of the preview, the solve must be the solve without one:

* the full result tuple (cost, index path, transmission vector, partitioning, superreads) equals the same table with preview = 0 and the oracle;
* forward_launches and the launch ledger (as a multiset) are those of the solve without a preview;
* S, the steps the finished schedule agrees on, equals the steps the preview launched, and the solve says that it continued;
* every way out of the preview -- a reported mismatch, an option set after the create, a group with a second table, another live table under
  `auto`, a second solve, no solve at all, release_device before the solve -- gives the identical result.

Tables: 4 x 8 192 columns (four plan pieces, the smallest with more than one piece to preview) at coverage 8 - 10, forced with preview = 1 and
preview_pieces = 1 and 2; one table of nine pieces at coverage 12 under `auto` with nothing forced."""
import gc
import os

import pytest

import oracle
from helpers import first_difference, table_solution
from whatshap_amd import _native
from whatshap_amd.synthetic import synthetic_block

pytestmark = pytest.mark.gpu

PIECE = 8192


class debug_library:
    """Every table made inside goes through libwhatshap_amd_debug.so: the preview's record and the ledger exist there."""

    def __enter__(self):
        self.saved = _native._lib
        _native.use_debug_library()

    def __exit__(self, *exc):
        _native._lib = self.saved


def tie_heavy(p):
    p.var_quality[:] = 1   # every weight the same: ties at every minimum
    return p


def with_homozygous_columns(p, columns):
    for c in columns:
        p.genotype.reshape(-1)[c] = 0 if c % 2 else 2   # a run that holds such a column leaves Y form
    return p


CASES = {
    "regular_cov8": lambda: synthetic_block(n_variants=4 * PIECE, coverage=8, seed=41),
    "regular_cov10": lambda: synthetic_block(n_variants=4 * PIECE, coverage=10, seed=42),
    "tie_heavy_cov9": lambda: tie_heavy(synthetic_block(n_variants=4 * PIECE, coverage=9, seed=43)),
    "homozygous_in_prefix_cov8": lambda: with_homozygous_columns(synthetic_block(n_variants=4 * PIECE, coverage=8, seed=44), (700, 701, 3000, 9000)),
}
_cache = {}


def case(name):
    """(problem, the oracle's solution, the solution / forward launches / ledger of the table solved with preview = 0): made once, shared, never changed."""
    if name not in _cache:
        p = CASES[name]()
        want = table_solution(oracle.OracleTable(p))
        with debug_library():
            t = _native.NativeTable(p, solve=False, options={"preview": "0"})
            assert not _native.debug_preview(t)["ran"] and _native.debug_preview(t)["why_not"] == "no preview: switched off"
            t.solve()
            plain = table_solution(t)
            launches, ledger = t.stats()["forward_launches"], ledger_multiset(t)
            t.close()
        assert plain == want, first_difference(want, plain)
        _cache[name] = (p, want, launches, ledger)
    return _cache[name]


def ledger_multiset(table):
    """The ledger's lines with their counts, the preview mark set apart: a launch made by the create and the same launch made by the solve are one line."""
    lines = {}
    for rec in _native.debug_launches(table):
        key = tuple(sorted((k, str(v)) for k, v in rec.items() if k not in ("count", "preview")))
        lines[key] = lines.get(key, 0) + rec["count"]
    return sorted(lines.items())


def marked_launches(table):
    return sum(rec["count"] for rec in _native.debug_launches(table) if rec["preview"])


def check_same(table, name, continued):
    p, want, launches, ledger = case(name)
    got = table_solution(table)
    assert got == want, first_difference(want, got)
    assert table.stats()["forward_launches"] == launches
    assert ledger_multiset(table) == ledger
    assert _native.debug_preview(table)["continued"] == continued


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_a_forced_preview_is_continued_and_changes_nothing(name, pieces):
    p = case(name)[0]
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": str(pieces)})
        pv = _native.debug_preview(t)
        print("PREVIEW", name, pieces, pv)
        assert pv["ran"] and pv["why_not"] == "" and pv["pieces"] == pieces, pv
        assert pv["launched_steps"] > 0 and pv["agreed_steps"] == pv["launched_steps"], pv
        t.solve()
        check_same(t, name, continued=True)
        assert marked_launches(t) == pv["launched_steps"]   # (one launch per step: the ledger says which launches the create made)
        t.close()


def test_a_table_that_is_not_in_y_form_is_previewed_and_continued():
    """The Y form is decided for the whole table by the one plan the preview and the create share.  The decision cannot be made to fail on real input -- the sum
    it tests is at most twice the bound that keeps a table on slot runs at all, far below 2^32 -- so the debug library's switch turns the Y form off: the
    preview launches the plain-form kernels the schedule holds, every step agrees, and the solve continues."""
    p = synthetic_block(n_variants=4 * PIECE, coverage=8, seed=51)
    want = table_solution(oracle.OracleTable(p))
    os.environ["WHAMD_NO_YFORM"] = "1"
    try:
        with debug_library():
            plain = _native.NativeTable(p, solve=False, options={"preview": "0"})
            plain.solve()
            t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "2"})
            pv = _native.debug_preview(t)
            assert pv["ran"] and pv["launched_steps"] > 100 and pv["agreed_steps"] == pv["launched_steps"], pv
            t.solve()
            got = table_solution(t)
            assert got == want and got == table_solution(plain), first_difference(want, got)
            assert _native.debug_preview(t)["continued"] and t.stats()["forward_launches"] == plain.stats()["forward_launches"]
            assert ledger_multiset(t) == ledger_multiset(plain)
            assert all(rec["yflags"] in (None, 0) for rec in _native.debug_launches(t) if rec["site"] == "slot_run")
            t.close()
            plain.close()
    finally:
        del os.environ["WHAMD_NO_YFORM"]


@pytest.mark.parametrize("at", [0, 100])
def test_a_reported_mismatch_starts_the_solve_over(at):
    """S = 0 and S in the middle of the preview: the exchange columns have moved on past step S, so either way the solve begins at step 0."""
    name = "regular_cov8"
    p = case(name)[0]
    os.environ["WHAMD_PREVIEW_MISMATCH_AT"] = str(at)
    try:
        with debug_library():
            t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "2"})
    finally:
        del os.environ["WHAMD_PREVIEW_MISMATCH_AT"]
    with debug_library():
        pv = _native.debug_preview(t)
        assert pv["ran"] and pv["agreed_steps"] == at and pv["launched_steps"] > 100, pv
        t.solve()
        check_same(t, name, continued=False)
        assert marked_launches(t) == 0   # (the ledger is that of the solve that started over)
        t.close()


def test_an_option_set_after_the_create_starts_the_solve_over():
    name = "regular_cov10"
    p = case(name)[0]
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "1"})
        assert _native.debug_preview(t)["ran"]
        t.set_option("symmetry", "1")   # (the default: the plan is the same, the table is uploaded again)
        t.solve()
        check_same(t, name, continued=False)
        t.close()


@pytest.mark.parametrize("previewed_leads", [False, True])
def test_a_group_with_a_second_table_starts_the_solve_over(previewed_leads):
    """(the group's forward pass goes onto the stream of its first table: another table's, or the previewed table's own)"""
    name = "regular_cov8"
    p = case(name)[0]
    q = synthetic_block(n_variants=3000, coverage=8, seed=46)
    want_q = table_solution(oracle.OracleTable(q))
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "2"})
        assert _native.debug_preview(t)["ran"]
        u = _native.NativeTable(q, solve=False)
        group = [t, u] if previewed_leads else [u, t]
        _native.enqueue_many(group)
        _native.wait_many(group)
        assert t.stats()["group_tables"] == 2
        got = table_solution(t)
        assert got == case(name)[1], first_difference(case(name)[1], got)
        assert not _native.debug_preview(t)["continued"]
        assert table_solution(u) == want_q
        t.close()
        u.close()


def test_auto_with_another_live_table_does_not_preview():
    with debug_library():
        other = _native.NativeTable(synthetic_block(n_variants=400, coverage=8, seed=47), solve=False)
        t = _native.NativeTable(synthetic_block(n_variants=9 * PIECE, coverage=8, seed=48), solve=False)
        pv = _native.debug_preview(t)
        assert not pv["ran"] and pv["why_not"] == "no preview: not alone", pv
        t.close()
        other.close()


def test_a_second_solve_of_the_same_table_starts_at_step_0():
    name = "tie_heavy_cov9"
    p = case(name)[0]
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "2"})
        t.solve()
        check_same(t, name, continued=True)
        t.solve()
        check_same(t, name, continued=False)
        t.close()


def test_create_then_destroy_with_no_solve():
    p = case("regular_cov10")[0]
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "2"})
        assert _native.debug_preview(t)["ran"]
        t.close()
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "2"})   # (the buffers came back from the pools)
        t.solve()
        check_same(t, "regular_cov10", continued=True)
        t.close()


def test_create_then_release_device_then_solve():
    name = "regular_cov8"
    p = case(name)[0]
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": "1"})
        assert _native.debug_preview(t)["ran"]
        t.release_device()
        t.solve()
        check_same(t, name, continued=False)
        t.close()


def test_auto_previews_a_lone_table_of_nine_pieces_and_continues():
    gc.collect()   # (tables of earlier tests that nobody closed would count as live)
    p = synthetic_block(n_variants=9 * PIECE, coverage=12, seed=49)
    want = table_solution(oracle.OracleTable(p))
    with debug_library():
        t = _native.NativeTable(p, solve=False)
        pv = _native.debug_preview(t)
        print("PREVIEW auto", pv)
        assert pv["ran"] and pv["pieces"] == 1 and pv["launched_steps"] > 0 and pv["agreed_steps"] == pv["launched_steps"], pv
        t.solve()
        got = table_solution(t)
        assert got == want, first_difference(want, got)
        assert _native.debug_preview(t)["continued"]
        launches = t.stats()["forward_launches"]
        t.close()
        t = _native.NativeTable(p, solve=False, options={"preview": "0"})
        t.solve()
        assert table_solution(t) == want and t.stats()["forward_launches"] == launches
        t.close()
