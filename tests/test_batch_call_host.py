"""The protocol every batch layer shares (csrc/batch_call.h), through the debug library's host entry points: the empty call, a bad problem
index, "problem k: " in front of a preparation's message, the stats the driver stamps, and the texts of check_offsets.  Every layer
takes its smallest valid problem: one read with one entry (reordering: one read with two, there is no breakpoint inside one position).
progeny keeps a driver of its own (its problems live in the result) and follows the same protocol, so it is a case here too."""

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

from whatshap_amd import _native
from whatshap_amd import genotype as gt
from whatshap_amd import haplotag as ht
from whatshap_amd import haplotagphase as tp
from whatshap_amd import polythread as pt
from whatshap_amd import progeny as pg
from whatshap_amd import reorder as ro
from whatshap_amd.polyphase import AlleleMatrix

U64 = np.uint64


def with_attr(problem, name, value):
    """`problem` with one array replaced behind the checks of its constructor: the native validation is what is under test."""
    setattr(problem, name, np.ascontiguousarray(value, dtype=getattr(problem, name).dtype))
    return problem


def matrix(n_reads=1, n_pos=1):
    return AlleleMatrix.from_csr([n_pos * r for r in range(n_reads + 1)], list(range(n_pos)) * n_reads, [r % 2 for r in range(n_reads) for _ in range(n_pos)])


def tagphase_problem(n_reads=1):
    return tp.TagphaseProblem([0], list(range(n_reads + 1)), [0] * n_reads, [0] * n_reads, [7] * n_reads, [10] * n_reads, [0] * n_reads)


def prior_problem(n_reads=1):
    return gt.PriorProblem(list(range(n_reads + 1)), [5] * n_reads, [1] * n_reads, [30] * n_reads)


def haplotag_problem(n_reads=1):
    return ht.HaplotagProblem(2, [100], [100], [[0, 1]], list(range(n_reads + 1)), [100] * n_reads, [1] * n_reads, [9] * n_reads, [0] * n_reads,
                              list(range(n_reads)))


def thread_problem(n_reads=1):
    return pt.ThreadingProblem(matrix(n_reads), [[r] for r in range(n_reads)], 2)


def reorder_problem(n_reads=1):
    return ro.ReorderProblem(matrix(n_reads, 2), [[0, 1], [0, 1]], [[0, 1], [1, 0]], [[r] for r in range(n_reads)], [1], [[0, 1]], [list(range(n_reads))])


def progeny_problem(n_reads=1):
    table = pg.ProgenyGenotypeLikelihoods.from_array(np.full((1, 1, 3), 1.0 / 3.0, dtype=np.float32))   # one sample at ploidy 2
    return pg.ProgenyProblem(table, [0], [1], [0], 4)


class Layer(SimpleNamespace):
    """name: the C prefix; make(n_reads): a valid problem; batch: the Python call; view(problem); entry / debug_entry / extra: the native
    call; counts: the accessors that take a problem index; getters: (name, number of output pointers) of those that take one;
    fault(problem): the problem with one fault of its own view, and its text; fields: what a result compares by."""


REORDER_EXTRA = (math.log(0.93), math.log(0.07))
LAYERS = [
    Layer(name="whamd_tagphase", make=tagphase_problem, batch=tp.tagphase_batch, view=lambda p: p.view(False), View=_native.TagphaseView,
          entry="whamd_tagphase", debug_entry="whamd_debug_tagphase_host", extra=(), stats=_native.TagphaseStats,
          counts=("whamd_tagphase_count", "whamd_tagphase_row_count"), getters=(("whamd_tagphase_get", 9), ("whamd_tagphase_get_table", 5)),
          fault=lambda p: (with_attr(p, "read_ptr", [1, 1]), "read_ptr does not start at 0"),
          fields=("voted", "first", "n_phasesets", "best_ps", "best_id", "score", "total", "kept", "zero_total")),
    Layer(name="whamd_prior_genotypes", make=prior_problem, batch=gt.prior_genotypes_batch, view=lambda p: p.view(), View=_native.PriorGenotypesView,
          entry="whamd_prior_genotypes", debug_entry="whamd_debug_prior_genotypes_host", extra=(), stats=_native.PriorGenotypesStats,
          counts=("whamd_prior_genotypes_count",), getters=(("whamd_prior_genotypes_get", 4),),
          fault=lambda p: (with_attr(p, "read_ptr", [1, 1]), "read_ptr does not start at 0"), fields=("gl", "genotype", "reg", "reg_genotype")),
    Layer(name="whamd_haplotag", make=haplotag_problem, batch=ht.haplotag_batch, view=lambda p: p.view(), View=_native.HaplotagView,
          entry="whamd_haplotag", debug_entry="whamd_debug_haplotag_host", extra=(), stats=_native.HaplotagStats,
          counts=("whamd_haplotag_count", "whamd_haplotag_bx_count"), getters=(("whamd_haplotag_get", 3), ("whamd_haplotag_get_bx", 4)),
          fault=lambda p: (with_attr(p, "read_ptr", [1, 1]), "read_ptr does not start at 0"),
          fields=("haplotype", "quality", "phaseset", "bx", "bx_start", "bx_haplotype", "bx_phaseset")),
    Layer(name="whamd_poly_thread", make=thread_problem, batch=pt.threading_inputs_batch, view=lambda p: p.view(), View=_native.PolyThreadView,
          entry="whamd_poly_thread_inputs", debug_entry="whamd_debug_poly_thread_inputs_host", extra=(), stats=_native.PolyThreadStats,
          counts=("whamd_poly_thread_position_count", "whamd_poly_thread_row_count", "whamd_poly_thread_cov_count"),
          getters=(("whamd_poly_thread_get_rows", 5), ("whamd_poly_thread_get_cov", 4)),
          fault=lambda p: (with_attr(p, "cluster_ptr", [1, 1]), "cluster_ptr does not start at 0"),
          fields=("pc_ptr", "pc_cluster", "pc_depth", "pc_first", "pc_consensus", "cov_ptr", "cov_cluster", "cov_readded", "cov_rank")),
    Layer(name="whamd_poly_reorder", make=reorder_problem, batch=ro.link_likelihoods_batch, view=lambda p: p.view(), View=_native.PolyReorderView,
          entry="whamd_poly_reorder", debug_entry="whamd_debug_poly_reorder_host", extra=REORDER_EXTRA, stats=_native.PolyReorderStats,
          counts=("whamd_poly_reorder_breakpoint_count", "whamd_poly_reorder_llh_count", "whamd_poly_reorder_window_count"),
          getters=(("whamd_poly_reorder_get_llh", 3), ("whamd_poly_reorder_get_windows", 3), ("whamd_poly_reorder_get_phasing", 4)),
          fault=lambda p: (with_attr(p, "cluster_ptr", [1, 1]), "cluster_ptr must start at 0 and not decrease"),
          fields=("llh_ptr", "llh_flat", "best", "assignments", "threads", "haplotypes", "confidence")),
]
PROGENY = Layer(name="whamd_progeny_score", make=progeny_problem, batch=pg.score_variants_batch, view=lambda p: p.view(), View=_native.ProgenyView,
                entry="whamd_progeny_score", debug_entry="whamd_debug_progeny_score_host", extra=(), stats=_native.ProgenyScoreStats,
                counts=("whamd_progeny_score_count",), getters=(("whamd_progeny_score_get", 4),),
                fault=lambda p: (setattr(p, "scoring_window", 2) or p,
                                 "scoring_window 2 below 4: the reference's stride list is undefined there (it raises IndexError)"))
RUN_BATCH = pytest.mark.parametrize("layer", LAYERS, ids=lambda l: l.name)
ALL = pytest.mark.parametrize("layer", LAYERS + [PROGENY], ids=lambda l: l.name)


def last_error(L):
    return L.whamd_last_error().decode()


def host_call(layer, problems):
    """The debug library's host entry point on the problems' views: (library, handle); the caller destroys."""
    L = _native.debug_lib()
    views = (layer.View * max(len(problems), 1))(*[layer.view(p) for p in problems])
    h = C.c_void_p()
    assert getattr(L, layer.debug_entry)(views, len(problems), *layer.extra, C.byref(h)) == _native.WHAMD_OK, last_error(L)
    return L, h


@ALL
def test_an_empty_call_gives_an_empty_result_and_a_null_out_is_refused(layer):
    L, h = host_call(layer, [])
    try:
        assert h.value and getattr(L, layer.name + "_problem_count")(h) == 0
    finally:
        getattr(L, layer.name + "_destroy")(h)
    assert layer.batch([], host=True) == []
    assert getattr(L, layer.debug_entry)(None, 0, *layer.extra, None) == _native.WHAMD_ERR_INVALID
    assert last_error(L) == "null argument"


@ALL
def test_a_bad_problem_index_and_a_null_result(layer):
    L, h = host_call(layer, [layer.make()])
    stats = layer.stats()
    try:
        assert getattr(L, layer.name + "_problem_count")(h) == 1
        calls = [(name, (None,) * n_out) for name, n_out in layer.getters] + [(layer.name + "_get_stats", (C.byref(stats),))]
        for name, outs in calls:
            assert getattr(L, name)(h, 1, *outs) == _native.WHAMD_ERR_INVALID and last_error(L) == "problem index out of range", name
            assert getattr(L, name)(None, 0, *outs) == _native.WHAMD_ERR_INVALID and last_error(L) == "null argument", name
        assert getattr(L, layer.name + "_get_stats")(h, 0, None) == _native.WHAMD_ERR_INVALID and last_error(L) == "null argument"
        for name in layer.counts:
            assert getattr(L, name)(h, 1) == 0 and getattr(L, name)(None, 0) == 0, name
        assert getattr(L, layer.name + "_problem_count")(None) == 0
    finally:
        getattr(L, layer.name + "_destroy")(h)


@ALL
def test_a_message_names_its_problem_only_in_a_call_of_several(layer):
    bad, text = layer.fault(layer.make())
    with pytest.raises(ValueError) as alone:
        layer.batch([bad], host=True)
    assert str(alone.value) == text
    with pytest.raises(ValueError) as second:
        layer.batch([layer.make(), bad], host=True)
    assert str(second.value) == "problem 1: " + text
    L = _native.debug_lib()   # and *out is null after the failure
    views = (layer.View * 2)(layer.view(layer.make()), layer.view(bad))
    h = C.c_void_p(1)
    assert getattr(L, layer.debug_entry)(views, 2, *layer.extra, C.byref(h)) == _native.WHAMD_ERR_INVALID and h.value is None


@ALL
def test_the_stats_of_a_host_call_are_those_of_the_whole_call(layer):
    stats = []
    layer.batch([layer.make(), layer.make(2), layer.make()], host=True, stats=stats)
    assert len(stats) == 3
    for s in stats:
        assert (s["launches"], s["upload_ms"], s["kernel_ms"], s["download_ms"]) == (0, 0.0, 0.0, 0.0)
        assert 0.0 <= s["host_ms"] <= s["total_ms"]
        assert (s["host_ms"], s["total_ms"]) == (stats[0]["host_ms"], stats[0]["total_ms"])
        assert s.get("map_ms", s["host_ms"]) == s["host_ms"] and 0.0 <= s.get("fill_ms", 0.0) <= s["total_ms"]


# ---------------------------------------------------------------------------------------------- check_offsets, through the layers that use it
def fake_inputs(pc_ptr):
    return SimpleNamespace(ploidy=2, pc_ptr=np.ascontiguousarray(pc_ptr, dtype=U64), pc_cluster=np.zeros(2, dtype=np.uint32), pc_consensus=np.zeros((2, 2), dtype=np.int8))


OFFSETS = {
    "tagphase": lambda ptr: tp.tagphase_batch([with_attr(tagphase_problem(2), "read_ptr", ptr)], host=True),
    "prior_genotypes": lambda ptr: gt.prior_genotypes_batch([with_attr(prior_problem(2), "read_ptr", ptr)], host=True),
    "haplotag": lambda ptr: ht.haplotag_batch([with_attr(haplotag_problem(2), "read_ptr", ptr)], host=True),
    "polythread": lambda ptr: pt.threading_inputs_batch([with_attr(thread_problem(2), "cluster_ptr", ptr)], host=True),
    "haplotypes": lambda ptr: pt.haplotypes_from_inputs([[0, 0], [0, 0]], fake_inputs(ptr), host=True),
}


@pytest.mark.parametrize("user,array,item", [("tagphase", "read_ptr", "read"), ("prior_genotypes", "read_ptr", "read"), ("haplotag", "read_ptr", "read"),
                                             ("polythread", "cluster_ptr", "cluster"), ("haplotypes", "pc_ptr", "position")])
def test_the_texts_of_check_offsets(user, array, item):
    """The strings are those of the sources before batch_call.h, where every layer spelled the check out."""
    expected = {"read_ptr": ("read_ptr does not start at 0", "read_ptr decreases at read 1"),
                "cluster_ptr": ("cluster_ptr does not start at 0", "cluster_ptr decreases at cluster 1"),
                "pc_ptr": ("pc_ptr does not start at 0", "pc_ptr decreases at position 1")}[array]
    assert expected == (array + " does not start at 0", array + " decreases at " + item + " 1")
    OFFSETS[user]([0, 1, 2])   # the valid array passes
    for ptr, text in (([1, 1, 2], expected[0]), ([0, 2, 1], expected[1])):
        with pytest.raises(ValueError) as e:
            OFFSETS[user](ptr)
        assert str(e.value) == text


# ---------------------------------------------------------------------------------------------- on the device
def compared(layer, result):
    return [np.asarray(getattr(result, f)) for f in layer.fields]


@pytest.mark.gpu
@RUN_BATCH
def test_a_call_of_two_problems_on_the_device_equals_the_host_twin(layer):
    problems = [layer.make(), layer.make(2)]
    stats = []
    got = layer.batch(problems, stats=stats)
    want = layer.batch(problems, host=True)
    assert stats[0]["launches"] > 0 and stats[1]["launches"] == stats[0]["launches"]
    for g, w in zip(got, want):
        for f, a, b in zip(layer.fields, compared(layer, g), compared(layer, w)):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (layer.name, f)
