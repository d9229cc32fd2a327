"""CPU: what a table's preview works out AHEAD of the create -- the record offsets and seed ids its leading runs are launched with, the
arena's size, the seeds' count and stride, the exchange columns' size -- against what the create's own phases (lay_out_arena, cut_chunks) give the same
table.  Through whamd_debug_preview_plan, a host entry point of the debug library: no device.  A rule restated wrongly in plan_preview would make every
preview wasted work (verify_preview would find no step that agrees) and only a GPU run would show it; this file shows it here.

Tables: single individuals of 4 and 9 plan pieces (coverage 8 and 12), regular, irregular_block and tie-heavy; P = 1, 2 and n_pieces - 1.  (An irregular
layout at coverage 8 has gaps -- several components, no preview: that table only has to say so; two irregular tables of one component are compared in full.)"""
import numpy as np
import pytest

from whatshap_amd import _native
from whatshap_amd.synthetic import irregular_block, synthetic_block

PIECE = 8192


def tie_heavy(p):
    p.var_quality[:] = 1
    return p


TABLES = {
    "regular_4_pieces_cov8": lambda: synthetic_block(n_variants=4 * PIECE, coverage=8, seed=61),
    "regular_9_pieces_cov12": lambda: synthetic_block(n_variants=9 * PIECE, coverage=12, seed=62),
    "irregular_4_pieces_cov8": lambda: irregular_block(n_variants=4 * PIECE, coverage=8, seed=63),
    "irregular_9_pieces_cov12": lambda: irregular_block(n_variants=9 * PIECE, coverage=12, seed=50),   # (one component: previewed)
    "irregular_4_pieces_cov12": lambda: irregular_block(n_variants=4 * PIECE, coverage=12, seed=73),   # (the same)
    "tie_heavy_4_pieces_cov8": lambda: tie_heavy(synthetic_block(n_variants=4 * PIECE, coverage=8, seed=65)),
    "tie_heavy_9_pieces_cov12": lambda: tie_heavy(synthetic_block(n_variants=9 * PIECE, coverage=12, seed=66)),
}
_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = TABLES[name]()
    return _problems[name]


@pytest.mark.parametrize("name", list(TABLES))
def test_what_the_preview_predicts_is_what_the_create_lays_out(name):
    p = problem(name)
    n_pieces = int(name.split("_pieces")[0].rsplit("_", 1)[1])
    previewed = 0
    for pieces in (1, 2, n_pieces - 1):
        r = _native.debug_preview_plan(p, pieces)
        assert r["n_pieces"] == n_pieces and not r["windowed"], r
        if r["steps"] == 0:   # an irregular layout may have several components, or begin with a per-column step: no preview, and it says why
            assert r["why_not"].startswith("no preview: "), r
            assert r["why_not"] in ("no preview: more than one connected component", "no preview: the table does not begin with slot runs"), r
            continue
        previewed += 1
        assert r["why_not"] == "" and r["pieces"] == pieces and 0 < r["steps"] < r["n_steps"], r
        assert np.array_equal(r["rec_predicted"], r["rec_laid_out"]), (pieces, np.flatnonzero(r["rec_predicted"] != r["rec_laid_out"])[:5])
        assert np.array_equal(r["spec_predicted"], r["spec_laid_out"]), (pieces, np.flatnonzero(r["spec_predicted"] != r["spec_laid_out"])[:5])
        assert (np.diff(r["rec_predicted"].astype(np.int64)) >= 0).all() and r["rec_predicted"][-1] > 0   # (records follow each other in step order)
        assert r["chunked_predicted"] == r["chunked"] == 1
        assert r["n_seeds_predicted"] == r["n_seeds"] > 0 and r["stride_predicted"] == r["stride"], r
        assert r["arena_predicted"] >= r["arena_laid_out"] > 0 and r["arena_predicted"] == r["arena_laid_out"], r   # (at least the laid-out size; in fact the same sum)
        assert r["exchange_predicted"] >= r["exchange_laid_out"] > 0, r
        # the seeds inside the preview: one every sixteen runs, counted from the table's END -- ids fall as the steps advance
        ids = r["spec_predicted"][r["spec_predicted"] > 0]
        assert ids.size >= r["steps"] // 16 - 1 and (np.diff(ids.astype(np.int64)) == -1).all(), ids[:8]
    if name != "irregular_4_pieces_cov8":   # (coverage 8 leaves gaps in an irregular layout: several components, no preview)
        assert previewed == 3


def test_more_pieces_only_extend_the_preview():
    p = problem("regular_9_pieces_cov12")
    one, eight = _native.debug_preview_plan(p, 1), _native.debug_preview_plan(p, 8)
    assert one["steps"] < eight["steps"]
    n = one["steps"]
    assert np.array_equal(one["rec_predicted"], eight["rec_predicted"][:n]) and np.array_equal(one["spec_predicted"], eight["spec_predicted"][:n])
    assert _native.debug_preview_plan(p, 0)["pieces"] == 1   # the library's rule: a sixth of nine pieces
    assert _native.debug_preview_plan(p, 100)["pieces"] == 8   # never the whole table
