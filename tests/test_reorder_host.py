"""CPU: polyphase reordering (whatshap_amd.reorder) on one host thread of the debug library against what the reference's run_reordering
recorded for every case of tests/reorder_cases.py: every link log likelihood bit for bit, windows, chosen permutations, assignments, final
threads and haplotypes equal, confidences within the bound of reorder_cases.check_against_recording; the reference-signature functions;
every validation error; the host preparation and the host twin as a stand-alone program under AddressSanitizer and UBSan."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import reorder_cases as rc
from whatshap_amd import reorder as ro

GOLDEN = rc.load_golden()
CASES = {c["name"]: c for c in GOLDEN["cases"]}
CSRC = os.path.join(rc.ROOT, "whatshap_amd", "csrc")


@pytest.fixture(scope="module")
def host_results():
    """All recorded cases as one batch through the host twin, fed the recorded cluster order."""
    stats = []
    res = ro.link_likelihoods_batch([rc.problem(c, rc.recorded_clusters(c)) for c in CASES.values()], host=True, stats=stats)
    assert all(s["launches"] == 0 for s in stats)
    return dict(zip(CASES, res)), dict(zip(CASES, stats))


def test_every_case_is_recorded_and_generates_the_recorded_input():
    generated = {c["name"]: c for c in rc.all_cases()}
    assert sorted(generated) == sorted(CASES)
    for name, c in generated.items():
        for key, value in c.items():
            assert CASES[name][key] == value, (name, key)
        assert float.fromhex(CASES[name]["log_match"]) == math.log(1 - c["error_rate"]) and float.fromhex(CASES[name]["log_err"]) == math.log(c["error_rate"])
    # the mechanisms the cases are there for
    assert GOLDEN["tied_breakpoints"] >= 2
    assert {c["ploidy"] for c in CASES.values()} == {2, 3, 4, 6, 8}
    sizes = {(c["ploidy"], len(b[1])) for c in CASES.values() for b in c["breakpoints"]}
    assert {(p, k) for p in (2, 3, 4, 6) for k in range(2, p + 1)} <= sizes and (8, 7) in sizes
    windows = [(len(e["left"]), len(e["right"])) for c in CASES.values() for e in c["expected"]]
    assert (32, 32) in windows and (0, 0) in windows and any(l and not r for l, r in windows)
    assert any(l < 32 and r == 32 for l, r in windows) and any(l == 32 and r < 32 for l, r in windows)   # cut by the block's start / end
    assert any(-1 in row for row in CASES["alleles_0_to_3_and_minus_one"]["haplotypes"])
    assert {a for row in CASES["alleles_0_to_3_and_minus_one"]["reads"] for _, a in row} == {0, 1, 2, 3}
    assert any(row[x][0] == row[x + 1][0] for row in CASES["duplicate_positions"]["reads"] for x in range(len(row) - 1))
    assert not CASES["zero_breakpoints"]["breakpoints"]
    assert any(b not in c["ref_find_breakpoints"] for c in CASES.values() for b in c["breakpoints"])   # subsets find_breakpoints does not yield


def test_the_quirk_and_the_tile_cases_are_what_they_claim(host_results):
    _, stats = host_results
    q = CASES["empty_right_quirk"]
    assert q["expected"][0]["right"] == [] and q["expected"][0]["left"][-1] == 14 and q["reads"][0][0] == [14, q["haplotypes"][0][14]]
    # reads 0 and 1 start on the last window position, span the breakpoint and are dropped; the library visits exactly the others
    spanning = [r for r, row in enumerate(q["reads"]) if row[0][0] < 15 <= row[-1][0] and any(r in q["clustering"][c] for c in q["expected"][0]["clusters"])]
    assert 0 in spanning and 1 in spanning
    assert stats["empty_right_quirk"]["n_reads_visited"] == len([r for r in spanning if q["reads"][r][0][0] < 14])
    assert stats["lds_tile"]["n_reads_visited"] > rc.read_tile()
    assert stats["span_edges"]["n_reads_visited"] > 0 and all(float.fromhex(v) == 0.0 for v in CASES["span_edges"]["expected"][0]["llh"])
    assert stats["seven_of_eight"]["n_permutations"] == 5040


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_reference(name, host_results):
    rc.check_against_recording(CASES[name], host_results[0][name])


def _breakpoints(case):
    return [ro.PhaseBreakpoint(pos, affected, 0.0) for pos, affected in case["breakpoints"]]


@pytest.mark.parametrize("name", list(CASES))
def test_reference_signatures(name):
    case = CASES[name]
    am = rc.allele_matrix(case)
    bps = _breakpoints(case)
    # the array-level call with the order this interpreter gives the reference's set expression: what the wrappers must pass on
    array_level = ro.link_likelihoods_batch([rc.problem(case)], error_rate=case["error_rate"], host=True)[0]
    lllh = ro.compute_link_likelihoods(case["threads"], case["haplotypes"], bps, case["clustering"], am, case["error_rate"], host=True)
    assert len(lllh) == len(bps)
    for b, d in enumerate(lllh):
        assert list(d) == list(itertools.permutations(case["breakpoints"][b][1]))   # the reference's ILP reads the key order
        assert np.array(list(d.values())).view(np.uint64).tolist() == np.ascontiguousarray(array_level.llh[b]).view(np.uint64).tolist()
        assert ro.get_heterozygous_pos_for_haps(case["haplotypes"], case["breakpoints"][b][1], case["breakpoints"][b][0], 32) == \
            (case["expected"][b]["left"], case["expected"][b]["right"])
    same_order = rc.cluster_order(case) == rc.recorded_clusters(case)
    if same_order:
        assert [[v.hex() for v in d.values()] for d in lllh] == [e["llh"] for e in case["expected"]]
        assert ro.get_optimal_assignments(bps, lllh, case["ploidy"], None) == case["assignments"]
    assert [[b.position, b.haplotypes] for b in ro.find_breakpoints(case["threads"])] == case["ref_find_breakpoints"]
    assert ro.get_heterozygous_pos_for_haps(case["haplotypes"], [0, 1], 5) == ([], [])
    # run_reordering mutates its arguments in place, as the reference does
    threads = [list(t) for t in case["threads"]]
    haplotypes = [list(h) for h in case["haplotypes"]]
    rows = [id(h) for h in haplotypes]
    ro.run_reordering(am, case["clustering"], threads, haplotypes, bps, None, case["error_rate"], host=True)
    assert [id(h) for h in haplotypes] == rows
    assert threads == array_level.threads.tolist() and haplotypes == array_level.haplotypes.tolist()
    assert [b.confidence for b in bps] == array_level.confidence.tolist()
    if same_order:
        assert threads == case["final_threads"] and haplotypes == case["final_haplotypes"]


def test_most_recorded_cluster_orders_are_this_interpreters():
    """The recording and this interpreter iterate the small sets of cluster ids alike (where a test machine's Python does not, the
    wrappers are still held to the array-level call above)."""
    same = sum(rc.cluster_order(c) == rc.recorded_clusters(c) for c in CASES.values())
    assert same >= len(CASES) // 2, same


def test_prephasing_is_not_implemented():
    case = CASES["span_edges"]
    with pytest.raises(NotImplementedError, match="compute_link_likelihoods"):
        ro.run_reordering(rc.allele_matrix(case), case["clustering"], case["threads"], case["haplotypes"], _breakpoints(case), rc.allele_matrix(case), host=True)
    with pytest.raises(NotImplementedError):
        ro.get_optimal_assignments(_breakpoints(case), [], 2, [[[0.0]]])


def test_validation_errors():
    """WHAMD_ERR_INVALID with a message, from the debug and from the product library alike (nothing is launched: the device is never opened)."""
    case = CASES["duplicate_haplotypes"]   # ploidy 3, 40 positions, breakpoints 8 [0, 1], 12 [0, 1, 2], 24 [0, 1, 2]
    clusters = rc.recorded_clusters(case)
    n_reads, n_clusters = len(case["reads"]), len(case["clustering"])

    def make(positions=(8, 12, 24), affected=([0, 1], [0, 1, 2], [0, 1, 2]), bp_clusters=clusters, clustering=case["clustering"], haplotypes=case["haplotypes"],
             threads=case["threads"]):
        return ro.ReorderProblem(rc.allele_matrix(case), threads, haplotypes, clustering, list(positions), [list(a) for a in affected], bp_clusters)

    assert len(ro.link_likelihoods_batch([make()], host=True)[0].llh) == 3
    wide = [h for h in case["haplotypes"]] * 3   # ploidy 9 for an affected list of 9
    wide_threads = [t * 3 for t in case["threads"]]
    bad = [
        (dict(affected=([1, 0], [0, 1, 2], [0, 1, 2])), "not sorted"),
        (dict(affected=([0, 0], [0, 1, 2], [0, 1, 2])), "not sorted"),
        (dict(affected=([0], [0, 1, 2], [0, 1, 2])), "outside 2 .. 8"),
        (dict(affected=(list(range(9)), [0, 1, 2], [0, 1, 2]), haplotypes=wide, threads=wide_threads), "outside 2 .. 8"),
        (dict(affected=([0, 3], [0, 1, 2], [0, 1, 2])), "at ploidy 3"),
        (dict(haplotypes=[case["haplotypes"][0]] * 17, threads=[[0] * 17 for _ in case["threads"]]), "ploidy 17"),
        (dict(bp_clusters=[[n_clusters]] + clusters[1:]), "cluster id"),
        (dict(clustering=[[n_reads]] + case["clustering"][1:]), "read id"),
        (dict(positions=(12, 8, 24)), "does not ascend"),
        (dict(positions=(8, 8, 24)), "does not ascend"),
        (dict(positions=(0, 12, 24)), r"outside \[1, 40\)"),
        (dict(positions=(8, 12, 40)), r"outside \[1, 40\)"),
        (dict(haplotypes=[h + [0] for h in case["haplotypes"]], threads=case["threads"] + [case["threads"][-1]]), "number of positions"),
    ]
    for change, match in bad:
        for host in (True, False):
            with pytest.raises(ValueError, match=match):
                ro.link_likelihoods_batch([make(**change)], host=host)
    with pytest.raises(ValueError, match="problem 1"):
        ro.link_likelihoods_batch([make(), make(positions=(12, 8, 24))], host=True)


# ---------------------------------------------------------------------------------------------- the stand-alone program
PROGRAM = r"""
// The host preparation, the host twin and the tail of polyphase reordering through the debug C ABI, on cases read from a text file;
// prints every llh as a hexadecimal float.  What the library takes from elsewhere is stubbed: nothing here opens a device.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "polyreorder.h"
#include "../../include/whatshap_amd_debug.h"

namespace whamd {
static std::string g_error;
void set_last_error(const std::string& msg) { g_error = msg; }
whamd_status_t poly_score_device(const std::vector<PolyMatrix>&, uint32_t, float, int, std::vector<PolyResult>&, CallTimes&, std::string&) { return WHAMD_ERR_DEVICE; }
whamd_status_t reorder_score_device(const std::vector<ReorderProblem>&, double, double, int, std::vector<ReorderScores>&, CallTimes&, std::string&) {
	return WHAMD_ERR_DEVICE;
}
}  // namespace whamd

template <class T>
static std::vector<T> numbers(FILE* f) {
	unsigned long long n;
	if (fscanf(f, "%llu", &n) != 1) exit(2);
	std::vector<T> v(n);
	for (auto& x : v) {
		long long y;
		if (fscanf(f, "%lld", &y) != 1) exit(2);
		x = (T)y;
	}
	return v;
}

int main(int argc, char** argv) {
	FILE* f = fopen(argv[1], "r");
	int n_cases;
	if (!f || fscanf(f, "%d", &n_cases) != 1) return 2;
	for (int c = 0; c < n_cases; c++) {
		unsigned ploidy;
		char lm[64], le[64];
		if (fscanf(f, "%u %63s %63s", &ploidy, lm, le) != 3) return 2;
		auto read_ptr = numbers<uint64_t>(f);
		auto position = numbers<int64_t>(f);
		auto allele = numbers<int8_t>(f);
		auto haplotypes = numbers<int8_t>(f);
		auto threads = numbers<int32_t>(f);
		auto cluster_ptr = numbers<uint64_t>(f);
		auto cluster_reads = numbers<uint32_t>(f);
		auto bp_position = numbers<uint64_t>(f);
		auto affected_ptr = numbers<uint64_t>(f);
		auto affected = numbers<uint32_t>(f);
		auto bp_cluster_ptr = numbers<uint64_t>(f);
		auto bp_clusters = numbers<uint32_t>(f);
		whamd_poly_reorder_view v{};
		v.matrix = whamd_poly_matrix_view{read_ptr.size() - 1, read_ptr.data(), position.data(), allele.data()};
		v.ploidy = ploidy;
		v.n_pos = haplotypes.size() / ploidy;
		v.haplotypes = haplotypes.data();
		v.threads = threads.data();
		v.n_clusters = cluster_ptr.size() - 1;
		v.cluster_ptr = cluster_ptr.data();
		v.cluster_reads = cluster_reads.data();
		v.n_breakpoints = bp_position.size();
		v.bp_position = bp_position.data();
		v.bp_affected_ptr = affected_ptr.data();
		v.bp_affected = affected.data();
		v.bp_cluster_ptr = bp_cluster_ptr.data();
		v.bp_clusters = bp_clusters.data();
		whamd_poly_reorder_result* r = nullptr;
		if (whamd_debug_poly_reorder_host(&v, 1, strtod(lm, nullptr), strtod(le, nullptr), &r) != WHAMD_OK) {
			fprintf(stderr, "%s\n", whamd::g_error.c_str());
			return 1;
		}
		std::vector<double> llh(whamd_poly_reorder_llh_count(r, 0));
		std::vector<uint32_t> best(whamd_poly_reorder_breakpoint_count(r, 0)), assignments((best.size() + 1) * ploidy);
		std::vector<int32_t> out_threads(threads.size());
		std::vector<int8_t> out_haps(haplotypes.size());
		std::vector<double> confidence(best.size());
		if (whamd_poly_reorder_get_llh(r, 0, nullptr, llh.data(), best.data()) != WHAMD_OK) return 1;
		if (whamd_poly_reorder_get_phasing(r, 0, assignments.data(), out_threads.data(), out_haps.data(), confidence.data()) != WHAMD_OK) return 1;
		printf("case %zu", llh.size());
		for (double x : llh) printf(" %a", x);
		printf("\nbest");
		for (uint32_t x : best) printf(" %u", x);
		printf("\n");
		whamd_poly_reorder_destroy(r);
	}
	// an invalid problem takes the error path
	whamd_poly_reorder_view bad{};
	bad.ploidy = 17;
	whamd_poly_reorder_result* r = nullptr;
	if (whamd_debug_poly_reorder_host(&bad, 1, -0.1, -2.0, &r) != WHAMD_ERR_INVALID || r) return 1;
	fclose(f);
	printf("ok\n");
	return 0;
}
"""


def _compiler():
    for name in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def _numbers(values):
    flat = [int(x) for x in values]
    return " ".join([str(len(flat))] + [str(x) for x in flat])


def test_host_program_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    names = sorted((n for n in CASES if CASES[n]["breakpoints"]), key=lambda n: sum(len(r) for r in CASES[n]["reads"]))[:4] + ["empty_right_quirk", "duplicate_haplotypes"]
    lines = [str(len(names))]
    for name in names:
        case = CASES[name]
        p = rc.problem(case, rc.recorded_clusters(case))
        am = p.allele_matrix
        lines.append(f"{case['ploidy']} {case['log_match']} {case['log_err']}")
        for arr in (am.read_ptr, am.position, am.allele, p.haplotypes.reshape(-1), p.threads.reshape(-1), p.cluster_ptr, p.cluster_reads, p.bp_position,
                    p.bp_affected_ptr, p.bp_affected, p.bp_cluster_ptr, p.bp_clusters):
            lines.append(_numbers(arr))
    data = tmp_path / "cases.txt"
    data.write_text("\n".join(lines) + "\n")
    src = tmp_path / "reorder_check.cpp"
    exe = tmp_path / "reorder_check"
    src.write_text(PROGRAM)
    # (g++ links the sanitizers' runtimes as shared libraries unless told otherwise; linked in, they start first whatever else the process loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-g1", "-O0", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DWHAMD_DEBUG_BUILD"] + static +
                   ["-I" + CSRC, str(src), os.path.join(CSRC, "polyreorder.cpp"), os.path.join(CSRC, "polyscore.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.strip().split("\n")
    assert out[-1] == "ok" and len(out) == 2 * len(names) + 1
    for k, name in enumerate(names):
        head, count, *values = out[2 * k].split()
        want = [v for e in CASES[name]["expected"] for v in e["llh"]]
        assert head == "case" and int(count) == len(want)
        assert [float.fromhex(v).hex() for v in values] == want, name
        assert [int(x) for x in out[2 * k + 1].split()[1:]] == [e["chosen"] for e in CASES[name]["expected"]], name
