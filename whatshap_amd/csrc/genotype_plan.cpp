// genotype_plan.cpp -- host planning of the genotyper's device paths (genotype_plan.h): no HIP calls.
#include "genotype_plan.h"

#include <cstring>

#include "genotype.h"

namespace whamd {

bool geno_plan_runs(const Problem& p, const GenotypeModel& m, int l_pref, GenoRunPlan& pl) {
	const uint32_t n = p.n_cols, T = p.T, ni = p.n_ind;
	if (n < 2 || ni == 0 || ni > 4 || !(p.P == 2 || p.P == 4) || !(T == 1 || T == 4 || T == 16) || (T == 1) != (p.P == 2)) return false;
	SlotPlan plan;
	if (!plan_forward_slots(p, l_pref > 0 ? -l_pref : 0, 0, plan, 0, /*genotype_mode=*/true)) return false;
	for (const Step& s : plan.steps) if (s.kind != 2) return false;   // a column no run can take
	const uint32_t E = 2u * p.P, A = m.A;
	const size_t n_runs = plan.runs.size();
	pl = GenoRunPlan();
	pl.cols.resize(n);
	pl.rows.resize(n);
	pl.runs.resize(n_runs);
	pl.ccols.resize(n);
	for (size_t ri = 0; ri < n_runs; ++ri) {
		const SlotRun& sr = plan.runs[ri];
		GsRun& r = pl.runs[ri];
		r.c0 = sr.c0; r.ncols = sr.ncols; r.g = sr.g; r.L = sr.L; r.lw = sr.lw; r.threads = sr.threads;
		r.has_prev = sr.c0 > 0 ? 1u : 0u;
		r.has_next = sr.c0 + sr.ncols < n ? 1u : 0u;
		r.in_occ = sr.in_occ; r.in_identity = sr.in_identity; r.out_occ = sr.out_occ;
		std::memcpy(r.in_pos, sr.in_pos, sizeof r.in_pos);
		std::memcpy(r.out_pos, sr.out_pos, sizeof r.out_pos);
		const unsigned long long per_unit = (unsigned long long)sr.ncols * T * E;
		r.tab_off = pl.tab_words;
		r.v_off = (uint32_t)(per_unit << sr.g);
		r.s_off = r.v_off + (uint32_t)(per_unit << sr.lw);
		pl.tab_words += (unsigned long long)r.s_off + (unsigned long long)sr.ncols * 64u * E;
		pl.max_f = std::max(pl.max_f, sr.L + sr.g);
		const uint32_t nw = 1u << sr.g;   // per-workgroup partial sums of what the run hands on, one set per direction
		r.part_out_f = pl.n_partials; pl.n_partials += nw;
		r.part_out_b = pl.n_partials; pl.n_partials += nw;
		const uint32_t blocks = (uint32_t)((((size_t)sr.threads << sr.g) + 256u * GS_COMBINE_LANES - 1u) / (256u * GS_COMBINE_LANES));
		pl.max_blocks = std::max(pl.max_blocks, blocks);
		pl.max_lds = std::max(pl.max_lds, run_lds_bytes(sr.threads, sr.ncols, T, E, A));
		for (uint32_t ci = 0; ci < sr.ncols; ++ci) {
			const uint32_t c = sr.c0 + ci;
			const PedSlotRow& pr = plan.prows[c];
			const SlotBtCol& bc = plan.bt_cols[c];
			GsCol& cd = pl.cols[c];
			GsRow& rw = pl.rows[c];
			std::memset(&cd, 0, sizeof cd);
			std::memset(&rw, 0, sizeof rw);
			const ColumnEntry* col = p.col_begin(c);
			for (uint32_t j = 0; j < p.k[c]; ++j) {
				const uint32_t s = bc.slot[j];
				cd.active |= 1u << s;
				rw.pe[s] = m.error_prob[p.col_ptr[c] + j];
				rw.ind[s] = col[j].sample;
				rw.allele[s] = col[j].allele;
			}
			cd.first_of_table = c == 0;
			cd.last_of_table = c + 1 == n;
			if (pr.n_end > (uint32_t)GS_MAXLOCAL || pr.pad[0] > (uint32_t)GS_MAXLOCAL) return false;
			cd.n_end = (uint8_t)pr.n_end;
			for (uint32_t e = 0; e < pr.n_end; ++e) cd.end_slot[e] = plan.end_slots[plan.end_off[ri] + bc.kf + e];
			cd.n_start = (uint8_t)pr.pad[0];
			for (uint32_t e = 0; e < pr.pad[0]; ++e) cd.start_slot[e] = plan.start_slots[plan.start_off[ri] + pr.pad[1] + e];
			GsCombineCol& cc = pl.ccols[c];
			cc.tab_off = r.tab_off; cc.v_off = r.v_off; cc.s_off = r.s_off;   // (store_off: geno_plan_windows)
			cc.ci = ci; cc.ncols = sr.ncols; cc.g = sr.g; cc.L = sr.L; cc.threads = sr.threads; cc.n_blocks = blocks;
		}
	}
	geno_wire_rescaling(pl.runs);
	return true;
}

// The column stores are what grows with the table (a trio at coverage 15: 2 MiB per column and chain).  When both do not fit, the runs are cut
// into WINDOWS (the reference keeps sqrt(n) columns and recomputes, src/genotypedptable.cpp:116-157,159-195,324): pass 1 runs the whole forward
// chain keeping only the exchange column at every window boundary (and the columns of the newest window); then, newest window first, the
// forward columns of a window are recomputed from its kept exchange column, the backward chain runs through the window, and the window's
// likelihoods are formed.  Two sets of window stores: the recomputation of window w - 1 runs beside the backward chain and the combine of
// window w.  One more forward pass, any table length.
bool geno_plan_windows(GenoRunPlan& pl, uint32_t T, uint32_t A, size_t free_bytes, unsigned long long cap_words) {
	const size_t n = pl.cols.size(), n_runs = pl.runs.size();
	const double fixed = (double)pl.tab_words * 8 + (double)GS_COMBINE_BATCH * pl.max_blocks * T * A * 8 + 4.0 * ((double)(1ull << pl.max_f) * T * 8) +
	                     (double)n * (sizeof(GsCol) + sizeof(GsRow) + sizeof(GsCombineCol) + 8.0 * T * A + 8);
	if (pl.max_lds > GS_MAX_LDS) return false;
	std::vector<unsigned long long> run_words(n_runs);
	unsigned long long store_words = 0;
	for (size_t ri = 0; ri < n_runs; ++ri) {
		run_words[ri] = (unsigned long long)pl.runs[ri].ncols * ((unsigned long long)pl.runs[ri].threads << pl.runs[ri].g);
		store_words += run_words[ri];
	}
	const double room = 0.8 * (double)free_bytes - fixed - (double)(2ull << 30);
	unsigned long long budget_words = ~0ull;   // per store
	if (2.0 * (double)store_words * 8 > room) budget_words = room > 0 ? (unsigned long long)(room / 4.0 / 8.0) : 0ull;
	budget_words = std::min(budget_words, cap_words);
	GenoWindowCut cut = geno_cut_windows(run_words, budget_words);
	if (cut.run_too_large) return false;   // the per-column path
	pl.windows = std::move(cut.windows);
	pl.window_words = cut.window_words;
	pl.n_sets = pl.windows.size() > 1 ? 2 : 1;
	for (GsWindow& wdw : pl.windows) {
		wdw.c0 = pl.runs[wdw.r0].c0;
		wdw.c1 = pl.runs[wdw.r1 - 1].c0 + pl.runs[wdw.r1 - 1].ncols;
	}
	for (size_t ri = 0; ri < n_runs; ++ri) {
		GsRun& r = pl.runs[ri];
		r.store_off = cut.store_off[ri];   // (relative to the window's stores)
		for (uint32_t ci = 0; ci < r.ncols; ++ci) pl.ccols[r.c0 + ci].store_off = r.store_off;
	}
	return true;
}

whamd_status_t geno_slot_table(const Problem& p, GenoSlotTable& out, std::string& msg) {
	const uint32_t ni = p.n_ind, T = p.T;
	out = GenoSlotTable();
	// founders are the individuals whose two haplotypes ARE partitions (h2p does not depend on the transmission value)
	std::vector<uint8_t> is_child(ni, 0);
	for (uint32_t t3 = 0; t3 < p.n_triples; ++t3) is_child[p.triples[t3][2]] = 1;
	uint32_t child_slots = 0;
	for (uint32_t s = 0; s < ni; ++s) {
		if (!is_child[s]) {
			out.slot_of[2 * s] = (uint8_t)p.h2p[(size_t)s * 2];
			out.slot_of[2 * s + 1] = (uint8_t)p.h2p[(size_t)s * 2 + 1];
		} else {
			if (p.P != 4 || child_slots + 2 > 4) { msg = "unsupported pedigree shape for device genotyping"; return WHAMD_ERR_UNSUPPORTED; }
			for (uint32_t h = 0; h < 2; ++h) {
				out.slot_of[2 * s + h] = (uint8_t)(p.P + child_slots + h);
				for (uint32_t i = 0; i < T; ++i) out.child_part[i][child_slots + h] = (uint8_t)p.h2p[((size_t)i * ni + s) * 2 + h];
			}
			child_slots += 2;
		}
	}
	out.n_child_slots = child_slots;
	return WHAMD_OK;
}

}  // namespace whamd
