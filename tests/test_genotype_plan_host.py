"""The host arithmetic of the genotyper's device paths (whatshap_amd/csrc/genotype_plan.h), on the host alone: a stand-alone C++ program built
with the address and undefined-behaviour sanitizers cuts runs into windows, wires the rescaling of the runs, chooses the per-column window and sizes column grids.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whatshap_amd", "csrc")

PROGRAM = r"""
#include <cstdio>

#include "genotype_plan.h"

using namespace whamd;

#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond)) {                                                     \
			std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
			return 1;                                                      \
		}                                                                  \
	} while (0)

typedef std::vector<unsigned long long> Words;

static bool window_is(const GsWindow& w, size_t r0, size_t r1, unsigned long long words) { return w.r0 == r0 && w.r1 == r1 && w.words == words; }

int main() {
	{   // no budget: one window, the runs one behind the other
		const GenoWindowCut cut = geno_cut_windows(Words{4, 4, 4, 4}, ~0ull);
		CHECK(!cut.run_too_large);
		CHECK(cut.windows.size() == 1 && window_is(cut.windows[0], 0, 4, 16));
		CHECK((cut.store_off == Words{0, 4, 8, 12}));
		CHECK(cut.window_words == 16);
	}
	for (unsigned long long budget : {8ull, 9ull}) {   // 9: a run is never split, the ninth word stays unused
		const GenoWindowCut cut = geno_cut_windows(Words{4, 4, 4, 4}, budget);
		CHECK(!cut.run_too_large);
		CHECK(cut.windows.size() == 2 && window_is(cut.windows[0], 0, 2, 8) && window_is(cut.windows[1], 2, 4, 8));
		CHECK((cut.store_off == Words{0, 4, 0, 4}));
		CHECK(cut.window_words == 8);
	}
	CHECK(geno_cut_windows(Words{4, 10, 4}, 8).run_too_large);   // a single run exceeds the budget
	{   // a run of exactly the budget
		const GenoWindowCut cut = geno_cut_windows(Words{8}, 8);
		CHECK(!cut.run_too_large);
		CHECK(cut.windows.size() == 1 && window_is(cut.windows[0], 0, 1, 8));
		CHECK((cut.store_off == Words{0}) && cut.window_words == 8);
	}
	{   // windows of unequal size: window_words is the largest
		const GenoWindowCut cut = geno_cut_windows(Words{3, 3, 5, 2, 6}, 7);
		CHECK(cut.windows.size() == 3 && window_is(cut.windows[0], 0, 2, 6) && window_is(cut.windows[1], 2, 4, 7) && window_is(cut.windows[2], 4, 5, 6));
		CHECK((cut.store_off == Words{0, 3, 0, 5, 0}) && cut.window_words == 7);
	}

	// rescaling: runs in groups of GS_RESCALE; a forward run that is the first of its group and a backward run that is the last of its group
	// read exactly the per-workgroup sums their neighbour leaves, and the neighbour is told to leave them
	CHECK(GS_RESCALE >= 1 && GS_MIN_TOTAL > 1e-200 && GS_MIN_TOTAL < 1e-100);
	for (size_t n_runs : {1u, 2u, 4u, 5u, 9u}) {
		std::vector<GsRun> runs(n_runs);
		uint32_t next = 0;
		for (size_t ri = 0; ri < n_runs; ++ri) {
			runs[ri] = GsRun();
			runs[ri].g = (uint32_t)(ri % 3);   // 1, 2, 4 workgroups
			runs[ri].threads = 64u << (ri % 4);
			runs[ri].part_out_f = next; next += 1u << runs[ri].g;
			runs[ri].part_out_b = next; next += 1u << runs[ri].g;
		}
		geno_wire_rescaling(runs);
		for (size_t ri = 0; ri < n_runs; ++ri) {
			const GsRun& r = runs[ri];
			const bool first_of_group = ri > 0 && ri % GS_RESCALE == 0, last_of_group = ri + 1 < n_runs && (ri + 1) % GS_RESCALE == 0;
			CHECK((r.n_part_in_f != 0) == first_of_group);
			CHECK((r.n_part_in_b != 0) == last_of_group);
			if (first_of_group) CHECK(r.part_in_f == runs[ri - 1].part_out_f && r.n_part_in_f == 1u << runs[ri - 1].g && runs[ri - 1].emit_f == 1);
			if (last_of_group) CHECK(r.part_in_b == runs[ri + 1].part_out_b && r.n_part_in_b == 1u << runs[ri + 1].g && runs[ri + 1].emit_b == 1);
			// nobody emits what nobody reads
			CHECK(r.emit_f == (ri + 1 < n_runs && runs[ri + 1].n_part_in_f != 0 ? 1u : 0u));
			CHECK(r.emit_b == (ri > 0 && runs[ri - 1].n_part_in_b != 0 ? 1u : 0u));
			// the two chains rescale at the same boundaries: their product never carries more than one group
			if (ri > 0) CHECK((r.n_part_in_f != 0) == (runs[ri - 1].n_part_in_b != 0));
		}
	}
	CHECK(run_lds_bytes(256, 24, 16, 8, 16) <= GS_MAX_LDS && run_lds_bytes(256, 25, 16, 8, 16) > GS_MAX_LDS);   // a quartet's runs of four waves: 24 columns

	// per-column path: columns kept per window (per_column = 1000 bytes)
	CHECK(geno_column_window(10, 0, 1000.0, 1e9) == 10);   // everything fits: one window
	CHECK(geno_column_window(10, 0, 1000.0, 0.0) == 4);    // nothing free: ceil(sqrt(10))
	CHECK(geno_column_window(10, 0, 1000.0, 50000.0) == 10);   // 2 * 1000 * 10 <= 0.4 * 50000: the bound itself still fits
	CHECK(geno_column_window(10, 0, 1000.0, 49999.0) == 4);
	CHECK(geno_column_window(10, 3, 1000.0, 1e9) == 3);    // a hint is taken as given ...
	CHECK(geno_column_window(10, 100, 1000.0, 1e9) == 10); // ... up to the table
	CHECK(geno_column_window(1, 0, 1000.0, 0.0) == 1);
	CHECK(geno_column_window(1, 0, 1000.0, 1e9) == 1);

	// grid of a column kernel: 2^(k - min(k - proj, GENO_LOOP_BITS)) entries x T threads in blocks of GENO_BLOCK
	CHECK(blocks_for(0, 0, 1) == 1);
	CHECK(GENO_LOOP_BITS == 2 && GENO_BLOCK == 256);
	CHECK(blocks_for(12, 2, 1) == 4);       // k - proj = 10 > GENO_LOOP_BITS: 2^10 entries of 4 looped cells
	CHECK(blocks_for(12, 2, 4) == 16);
	CHECK(blocks_for(12, 11, 1) == 8);      // k - proj = 1: 2^11 entries
	CHECK(blocks_for(25, 0, 16) == (1u << 19));
	CHECK(blocks_for(3, 3, 16) == 1);       // 128 threads: one block

	// LDS of a run kernel: 2 exchange columns, A, priors, rho (padded to even), 16 doubles of scratch, the column descriptors
	CHECK(run_lds_bytes(64, 1, 1, 4, 4) == (128 + 4 + 4 + 2 + 16) * 8 + 32);
	CHECK(run_lds_bytes(512, 3, 4, 8, 16) == (1024 + 8 * 3 * 4 * 8 + 3 * 4 * 16 + 4 + 16) * 8 + 3 * 32);
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


def test_plan_arithmetic_program_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "genotype_plan_check.cpp"
    exe = tmp_path / "genotype_plan_check"
    src.write_text(PROGRAM)
    # (g++ links the sanitizers' runtimes as shared libraries unless told otherwise; linked in, they start first whatever else the process loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                   ["-pthread", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
