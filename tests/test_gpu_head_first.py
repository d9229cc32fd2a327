"""GPU (-m gpu): the preview started from the planner's head hook (DESIGN.md 6.1 "The preview"; csrc/slots.h SlotPlanHead).  whamd_dptable_create launches the
table's leading slot runs from INSIDE plan_forward_slots, as soon as the steps of the head are finished, and the planner's second half -- the rows, exit slots
and layouts of every later step -- happens under them.  Nothing about the solve may change:

* the full result tuple (cost, index path, transmission vector, partitioning, superreads) equals the oracle's and the same table's with preview = 0;
* the preview ran, from the hook; S, the steps the finished schedule agrees on (all 192 bytes of every run), equals the steps launched; the solve continued;
* forward_launches and the launch ledger (as a multiset) are those of the solve without a preview.

Tables: 4 x 8 192 columns at coverage 8 - 10 with preview = 1 and preview_pieces = 1 and 2 -- one of them with a homozygous column in the run just behind either
head, so that the head's last run reads the flag of a run the planner finishes later --; one table of nine pieces at coverage 12 under `auto`."""
import gc

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
    p.var_quality[:] = 1
    return p


def with_homozygous_columns(p, columns):
    for c in columns:
        p.genotype.reshape(-1)[c] = 0 if c % 2 else 2   # a run that holds such a column leaves Y form
    return p


CASES = {
    "regular_cov8": lambda: synthetic_block(n_variants=4 * PIECE, coverage=8, seed=141),
    "tie_heavy_cov10": lambda: tie_heavy(synthetic_block(n_variants=4 * PIECE, coverage=10, seed=142)),
    "homozygous_behind_the_head_cov9": lambda: with_homozygous_columns(synthetic_block(n_variants=4 * PIECE, coverage=9, seed=143), (PIECE + 2, 2 * PIECE + 2)),
}
_cache = {}


def ledger_multiset(table):
    """The ledger's lines with their counts, the preview mark set apart: a launch made by the create and the same launch made by the solve are one line."""
    lines = {}
    for rec in _native.debug_launches(table):
        key = tuple(sorted((k, str(v)) for k, v in rec.items() if k not in ("count", "preview")))
        lines[key] = lines.get(key, 0) + rec["count"]
    return sorted(lines.items())


def solved_without_preview(p):
    """(the oracle's solution, forward launches and ledger of the table solved with preview = 0, which must give the oracle's solution)"""
    want = table_solution(oracle.OracleTable(p))
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "0"})
        pv = _native.debug_preview(t)
        assert not pv["ran"] and not pv["from_hook"] and pv["why_not"] == "no preview: switched off", pv
        t.solve()
        plain = table_solution(t)
        launches, ledger = t.stats()["forward_launches"], ledger_multiset(t)
        t.close()
    assert plain == want, first_difference(want, plain)
    return want, launches, ledger


def case(name):
    """Made once, shared, never changed."""
    if name not in _cache:
        p = CASES[name]()
        _cache[name] = (p,) + solved_without_preview(p)
    return _cache[name]


def check_previewed_from_the_hook(t, pv, want, launches, ledger):
    assert pv["ran"] and pv["why_not"] == "" and pv["from_hook"], pv
    assert pv["launched_steps"] > 0 and pv["agreed_steps"] == pv["launched_steps"], pv
    t.solve()
    got = table_solution(t)
    assert got == want, first_difference(want, got)
    assert t.stats()["forward_launches"] == launches
    assert ledger_multiset(t) == ledger
    after = _native.debug_preview(t)
    assert after["continued"] and after["from_hook"], after
    assert sum(rec["count"] for rec in _native.debug_launches(t) if rec["preview"]) == pv["launched_steps"]   # (one launch per step, made by the create)


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_a_preview_from_the_hook_is_continued_and_changes_nothing(name, pieces):
    p, want, launches, ledger = case(name)
    with debug_library():
        t = _native.NativeTable(p, solve=False, options={"preview": "1", "preview_pieces": str(pieces)})
        pv = _native.debug_preview(t)
        print("PREVIEW", name, pieces, pv)
        assert pv["pieces"] == pieces, pv
        check_previewed_from_the_hook(t, pv, want, launches, ledger)
        t.close()


def test_the_run_behind_the_head_is_not_in_y_form():
    """(what the homozygous case is there for, held on the plan itself: at both head sizes the first run behind the head has left Y form)"""
    p = case("homozygous_behind_the_head_cov9")[0]
    for pieces in (1, 2):
        last, behind = _native.debug_head_first_plan(p, pieces)["edge_yflags"]
        assert last is not None and behind is not None and last & 1 and not last & 4 and not behind & 1, (pieces, last, behind)


def test_auto_previews_a_lone_table_of_nine_pieces_from_the_hook():
    gc.collect()   # (tables of earlier tests that nobody closed would count as live)
    p = synthetic_block(n_variants=9 * PIECE, coverage=12, seed=149)
    want, launches, ledger = solved_without_preview(p)
    with debug_library():
        t = _native.NativeTable(p, solve=False)
        pv = _native.debug_preview(t)
        print("PREVIEW auto", pv)
        assert pv["pieces"] == 1, pv
        check_previewed_from_the_hook(t, pv, want, launches, ledger)
        t.close()
