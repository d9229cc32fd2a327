"""CPU: comparing polyploid phasings (whatshap_amd.compare) on one host thread of the debug library against what the reference's
compare.py and SwitchFlipCalculator recorded for every case of tests/compare_cases.py.  Identical to the reference: the total, the
minimum Hamming distance, the switch errors, diff_genotypes and the matching positions, the one-position and one-match results, the
early returns.  Equal to compare_cases.dense_oracle: switches and flips (the split the layer defines: fewest flips among the paths of
minimum total, then lowest rank), flips at most the reference's.  The returned paths are valid; the errors of the ABI; compare_block at
ploidy 2 against the recording; the host twin as a stand-alone program under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import compare_cases as cc
from whatshap_amd import _native
from whatshap_amd import compare as cmp

GOLDEN = cc.load_golden()
CASES = {c["name"]: c for c in GOLDEN["cases"]}
CSRC = os.path.join(cc.ROOT, "whatshap_amd", "csrc")


@pytest.fixture(scope="module")
def host_results():
    """All recorded cases as one batch through the host twin: per case its cost pairs, then the switch-error job; every job with its path."""
    jobs, first = [], {}
    for name, case in CASES.items():
        first[name] = len(jobs)
        jobs += cc.jobs_of(case)
    stats = []
    res = cmp.switch_flips_batch(jobs, host=True, stats=stats)
    assert stats[0]["launches"] == 0 and stats[0]["n_jobs"] == len(jobs) and stats[0]["kernel_ms"] == 0
    return {name: res[at:at + len(CASES[name]["costs"]) + 1] for name, at in first.items()}


def test_every_case_is_recorded_and_generates_the_recorded_input():
    generated = {c["name"]: c for c in cc.all_cases()}
    assert sorted(generated) == sorted(CASES) and 40 <= len(CASES) <= 60
    for name, c in generated.items():
        for key, value in c.items():
            assert CASES[name][key] == value, (name, key)
    # the mechanisms the cases are there for
    shapes = {(c["ploidy"], len(c["phasing0"][0])) for c in CASES.values()}
    assert {p for p, _ in shapes} == {2, 3, 4, 5, 6}
    assert all({(p, n) for n in (1, 2, 3, 64, 65)} <= shapes for p in (2, 3, 4, 5, 6)) and all(any(q == p and n >= 89 for q, n in shapes) for p in (2, 3, 4, 5))
    assert max(n for p, n in shapes if p == 6) == 70 and max(n for _, n in shapes) < 100
    assert GOLDEN["splits_that_differ"] >= 1   # the reference's split is not the canonical one somewhere: the rule matters
    assert all(c["costs"] == [[1, 1], [2, 1], [1, 3], [0.5, 0.25]] for c in CASES.values())
    assert {a for c in CASES.values() for hap in c["phasing0"] for a in hap} == set("0123")
    n_match = {name: (len(c["ref"]["matching_pos"]), len(c["phasing0"][0])) for name, c in CASES.items()}
    assert n_match["no_match_p3"][0] == n_match["no_match_p5"][0] == 0 and n_match["one_match_p3"][0] == n_match["one_match_p4"][0] == n_match["one_match_p6"][0] == 1
    assert n_match["all_match_p4"] == (48, 48) and n_match["all_match_p5"] == (37, 37)
    for name in ("permuted_p3", "permuted_p4", "permuted_p5", "permuted_p6"):   # cost 0 on a path that does not sit on rank 0
        assert CASES[name]["ref"]["runs"][0]["raw"] == [0, 0] and CASES[name]["ref"]["runs"][0]["config"][0] != list(range(CASES[name]["ploidy"]))
    assert len(set(CASES["duplicates_p6"]["phasing0"])) == 1


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_reference_and_the_canonical_split(name, host_results):
    cc.check_against_recording(CASES[name], host_results[name])


def test_cost_zero_paths_stay_on_the_planted_permutation(host_results):
    for name in ("permuted_p3", "permuted_p4", "permuted_p5", "permuted_p6"):
        res = host_results[name][0]
        assert (res.total, res.switches, res.flips, res.min_hamming_sum) == (0.0, 0, 0, 0)
        assert len({tuple(p) for p in res.perms.tolist()}) == 1 and int(res.ranks[0]) != 0
        assert res.perms.tolist() == CASES[name]["ref"]["runs"][0]["config"]   # (the only path of cost 0: the reference's too)


def test_duplicate_haplotypes_take_rank_zero_everywhere(host_results):
    """Every permutation ties at every step: the lowest rank wins, first to last."""
    for name in ("duplicates_p3", "duplicates_p4", "duplicates_p6", "all_equal_p4", "all_equal_p6"):
        for res in host_results[name][:-1]:
            assert res.ranks.tolist() == [0] * len(res.ranks) and res.switches == 0


@pytest.mark.parametrize("name", list(CASES))
def test_compare_block_and_the_reference_signatures(name):
    case = CASES[name]
    ref, k = case["ref"], case["ploidy"]
    s0, s1 = case["phasing0"], case["phasing1"]
    p0, p1 = cc.arrays(case)
    block = cmp.compare_block(s0, s1, host=True)
    assert isinstance(block, cmp.PhasingErrors)
    assert (block.switches, block.hamming, block.diff_genotypes) == (ref["block"]["switches"], ref["block"]["hamming"], ref["block"]["diff_genotypes"])
    assert type(block.hamming) is type(ref["block"]["hamming"])
    assert cmp.compute_matching_genotype_pos(s0, s1) == ref["matching_pos"]
    if k == 2:   # the diploid branch: the reference's own result, field for field
        assert [block.switch_flips.switches, block.switch_flips.flips] == ref["block"]["switch_flips"]
        return
    n_pos = len(s0[0])
    want = ref["runs"][0]["raw"] if n_pos == 1 else list(cc.dense_oracle(p0, p1)[1:])
    assert [block.switch_flips.switches, block.switch_flips.flips] == [want[0] / k, want[1] / k]
    assert sum(want) == round(sum(ref["block"]["switch_flips"]) * k) or n_pos == 1   # costs (1, 1): the reference's total
    assert cmp.compute_switch_errors_poly(s0, s1, host=True) == cmp.compute_switch_errors_poly(s0, s1, ref["matching_pos"], host=True) == ref["switch_errors"]
    sf = cmp.compute_switch_flips_poly(s0, s1, switch_cost=2, flip_cost=1, host=True)
    result, switches_in_column, flips_in_column, config = cmp.compute_switch_flips_poly_bt([list(map(int, h)) for h in s0], [list(map(int, h)) for h in s1],
                                                                                           switch_cost=2, flip_cost=1, host=True)
    assert repr(sf) == repr(result) and len(switches_in_column) == len(flips_in_column) == len(config) == n_pos
    assert sum(switches_in_column) / k == result.switches and sum(len(f) for f in flips_in_column) / k == result.flips
    for x in range(n_pos):
        assert flips_in_column[x] == [i for i in range(k) if s0[config[x][i]][x] != s1[i][x]]


def test_early_returns_and_the_result_classes():
    assert cmp.compute_switch_flips_poly_bt(["", "", ""], ["", "", ""], host=True)[1:] == (None, None, None)
    assert repr(cmp.compute_switch_flips_poly_bt(["", "", ""], ["", "", ""], host=True)[0]) == "SwitchFlips(switches=0, flips=0)"
    assert cmp.compute_switch_flips_poly_bt([], [], host=True)[1:] == (None, None, None)
    assert repr(cmp.compute_switch_flips_poly(["", "", ""], ["", "", ""], host=True)) == "SwitchFlips(switches=0, flips=0)"
    empty = cmp.compare_block(["", "", ""], ["", "", ""], host=True)
    assert repr(empty) == "PhasingErrors(switches=0.0, hamming=0.0, switch_flips=0.0/0.0, diff_genotypes=0)"
    total = cmp.PhasingErrors()
    total += cmp.PhasingErrors(1.5, 2.0, cmp.SwitchFlips(0.5, 0.25), 3)
    total += cmp.PhasingErrors(1, 1, cmp.SwitchFlips(1, 1), 1)
    assert repr(total) == "PhasingErrors(switches=2.5, hamming=3.0, switch_flips=1.5/1.25, diff_genotypes=4)"   # (format() takes SwitchFlips.__str__)
    assert str(total.switch_flips) == "1.5/1.25"
    with pytest.raises(TypeError):
        total += cmp.SwitchFlips()
    # the one-position result through the reference's signature: ploidy - 1 raw switches
    assert repr(cmp.compute_switch_flips_poly(["0", "1", "1", "0"], ["1", "0", "1", "0"], host=True)) == "SwitchFlips(switches=0.75, flips=0.0)"
    assert repr(cmp.compute_switch_flips_poly(["0", "1", "1", "0", "1"], ["1", "0", "1", "0", "1"], host=True)) == "SwitchFlips(switches=0.8, flips=0.0)"


def test_empty_jobs_return_zeros():
    none = cc.arrays(CASES["no_match_p3"])
    jobs = [cmp.CompareJob(["", "", ""], ["", "", ""], want_path=True), cmp.CompareJob(none[0].astype(np.uint8), none[1].astype(np.uint8), 1, 5, matched_only=True, want_path=True)]
    stats = []
    for res in cmp.switch_flips_batch(jobs, host=True, stats=stats):
        assert (res.total, res.switches, res.flips, res.n_matched, res.n_visited, res.min_hamming_sum) == (0.0, 0, 0, 0, 0, 0) and len(res.positions) == 0
    assert stats[0]["n_visited"] == 0 and stats[0]["n_positions"] == 12 and stats[0]["launches"] == 0
    assert cmp.switch_flips_batch([], host=True) == []


def _header_constant(name):
    import re

    text = open(os.path.join(cc.ROOT, "include", "whatshap_amd.h")).read()
    return eval(re.search(r"#define " + name + r" \(\(uint64_t\)(.+)\)", text).group(1))


def test_abi_errors():
    """WHAMD_ERR_INVALID / WHAMD_ERR_UNSUPPORTED with a message, from the debug and from the product library alike (nothing is launched:
    the device is never opened)."""
    good = ["0110", "1010", "1100"]
    assert cmp.switch_flips_batch([cmp.CompareJob(good, good)], host=True)[0].total == 0.0
    limit = _header_constant("WHAMD_POLY_COMPARE_MAX_PATH_BYTES")
    assert limit == 1 << 30
    n_over = limit // (720 * 2) + 1   # one more position than a ploidy-6 path table may have
    big = np.zeros((n_over, 6), dtype=np.uint8)
    for host in (True, False):
        for cost in (dict(switch_cost=-1.0), dict(flip_cost=-0.5), dict(switch_cost=float("nan")), dict(flip_cost=float("inf")), dict(switch_cost=float("inf"))):
            with pytest.raises(ValueError, match="finite and not negative"):
                cmp.switch_flips_batch([cmp.CompareJob(good, good, **cost)], host=host)
        with pytest.raises(ValueError, match="ploidy 1 below 2"):
            cmp.switch_flips_batch([cmp.CompareJob(["01"], ["01"])], host=host)
        with pytest.raises(ValueError, match="ploidy 0 below 2"):
            cmp.switch_flips_batch([cmp.CompareJob([], [])], host=host)
        with pytest.raises(ValueError, match="job 1: ploidy 1 below 2"):
            cmp.switch_flips_batch([cmp.CompareJob(good, good), cmp.CompareJob(["01"], ["01"])], host=host)
        with pytest.raises(_native.SolverError, match="ploidy 7 above 6") as err:
            cmp.switch_flips_batch([cmp.CompareJob(["01"] * 7, ["01"] * 7)], host=host)
        assert err.value.status == _native.WHAMD_ERR_UNSUPPORTED
        with pytest.raises(_native.SolverError, match="WHAMD_POLY_COMPARE_MAX_PATH_BYTES") as err:
            cmp.switch_flips_batch([cmp.CompareJob(big, big, want_path=True)], host=host)
        assert err.value.status == _native.WHAMD_ERR_UNSUPPORTED
        # null arrays with positions
        L = _native.debug_lib() if host else _native.lib()
        view = _native.PolyCompareView(3, 0, 4, None, None, 1.0, 1.0, 0, 0)
        import ctypes as C

        h = C.c_void_p()
        st = L.whamd_debug_poly_compare_host(C.byref(view), 1, C.byref(h)) if host else L.whamd_poly_compare(C.byref(view), 1, 0, C.byref(h))
        assert st == _native.WHAMD_ERR_INVALID and not h and b"null argument" in L.whamd_last_error()
    with pytest.raises(ValueError, match="differ in shape"):
        cmp.CompareJob(good, good[:2])
    with pytest.raises(ValueError, match="outside 0-9"):
        cmp.CompareJob(["0a"], ["00"])
    with pytest.raises(ValueError, match="below 2"):
        cmp.compare_block(["01"], ["01"], host=True)


def test_the_product_library_has_no_debug_entry_point():
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"whamd_poly_compare", "whamd_poly_compare_job_count", "whamd_poly_compare_path_count", "whamd_poly_compare_get", "whamd_poly_compare_get_path",
            "whamd_poly_compare_get_stats", "whamd_poly_compare_destroy"} <= names
    assert not any(n.startswith("whamd_debug") for n in names)


# ---------------------------------------------------------------------------------------------- the stand-alone program
PROGRAM = r"""
// The validation, the host twin and the path expansion of comparing polyploid phasings through the debug C ABI, on jobs read from a text
// file; prints every job's result.  What the library takes from elsewhere is stubbed: nothing here opens a device.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "polycompare.h"
#include "../../include/whatshap_amd_debug.h"

namespace whamd {
static std::string g_error;
void set_last_error(const std::string& msg) { g_error = msg; }
whamd_status_t compare_device(const std::vector<CompareJob>&, int, std::vector<CompareResult>&, CallTimes&, std::string&) { return WHAMD_ERR_DEVICE; }
}  // namespace whamd

int main(int argc, char** argv) {
	FILE* f = fopen(argv[1], "r");
	int n_jobs;
	if (!f || fscanf(f, "%d", &n_jobs) != 1) return 2;
	std::vector<std::vector<uint8_t>> store;
	std::vector<whamd_poly_compare_view> views;
	for (int j = 0; j < n_jobs; j++) {
		unsigned ploidy, matched;
		unsigned long long n_pos;
		char sc[64], fc[64];
		if (fscanf(f, "%u %llu %u %63s %63s", &ploidy, &n_pos, &matched, sc, fc) != 5) return 2;
		for (int side = 0; side < 2; side++) {
			store.emplace_back(n_pos * ploidy);   // exactly the job's bytes: a read past them is caught
			for (auto& a : store.back()) {
				unsigned v;
				if (fscanf(f, "%u", &v) != 1) return 2;
				a = (uint8_t)v;
			}
		}
		whamd_poly_compare_view v{};
		v.ploidy = ploidy;
		v.matched_only = matched;
		v.n_pos = n_pos;
		v.switch_cost = strtod(sc, nullptr);
		v.flip_cost = strtod(fc, nullptr);
		v.want_path = 1;
		views.push_back(v);
	}
	for (int j = 0; j < n_jobs; j++) {
		views[j].phasing0 = store[2 * j].data();
		views[j].phasing1 = store[2 * j + 1].data();
	}
	whamd_poly_compare_result* r = nullptr;
	if (whamd_debug_poly_compare_host(views.data(), views.size(), &r) != WHAMD_OK) {
		fprintf(stderr, "%s\n", whamd::g_error.c_str());
		return 1;
	}
	std::vector<whamd_poly_compare_job_result> res(n_jobs);
	if (whamd_poly_compare_get(r, res.data()) != WHAMD_OK) return 1;
	for (int j = 0; j < n_jobs; j++) {
		const uint64_t m = whamd_poly_compare_path_count(r, j);
		std::vector<uint64_t> position(m);
		std::vector<uint16_t> rank(m);
		std::vector<uint8_t> perm(m * views[j].ploidy), flipped(m * views[j].ploidy);
		std::vector<uint32_t> switches(m);
		if (whamd_poly_compare_get_path(r, j, position.data(), rank.data(), perm.data(), flipped.data(), switches.data()) != WHAMD_OK) return 1;
		printf("job %a %u %u %llu %llu", res[j].total, res[j].switches, res[j].flips, (unsigned long long)res[j].min_hamming_sum, (unsigned long long)m);
		for (uint16_t x : rank) printf(" %u", (unsigned)x);
		printf("\n");
	}
	whamd_poly_compare_destroy(r);
	// an invalid job takes the error path
	whamd_poly_compare_view bad{};
	bad.ploidy = 1;
	r = nullptr;
	if (whamd_debug_poly_compare_host(&bad, 1, &r) != WHAMD_ERR_INVALID || r) return 1;
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


def test_host_program_under_sanitizers(tmp_path, host_results):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    names = ["planted_p3_n1", "planted_p4_n65", "one_match_p6", "no_match_p5", "alleles_0_to_3_p4", "planted_p6_n3", "duplicates_p6"]
    lines, want = [], []
    for name in names:
        case = CASES[name]
        p0, p1 = cc.arrays(case)
        for (sc, fc, matched), res in zip([(sc, fc, 0) for sc, fc in case["costs"]] + [(1, cc.switch_error_cost(case), 1)], host_results[name]):
            lines.append(f"{case['ploidy']} {len(p0)} {matched} {float(sc).hex()} {float(fc).hex()}")
            lines.append(" ".join(str(a) for a in p0.reshape(-1).tolist()))
            lines.append(" ".join(str(a) for a in p1.reshape(-1).tolist()))
            want.append([float(res.total).hex(), res.switches, res.flips, res.min_hamming_sum, len(res.ranks)] + res.ranks.tolist())
    data = tmp_path / "jobs.txt"
    data.write_text("\n".join([str(len(want))] + lines) + "\n")
    src = tmp_path / "compare_check.cpp"
    exe = tmp_path / "compare_check"
    src.write_text(PROGRAM)
    # (g++ links the sanitizers' runtimes as shared libraries unless told otherwise; linked in, they start first whatever else the process loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-g1", "-O0", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DWHAMD_DEBUG_BUILD"] + static +
                   ["-I" + CSRC, str(src), os.path.join(CSRC, "polycompare.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.strip().split("\n")
    assert out[-1] == "ok" and len(out) == len(want) + 1
    for line, w in zip(out, want):
        head, total, *numbers = line.split()
        assert head == "job" and [float.fromhex(total).hex()] + [int(x) for x in numbers] == w
