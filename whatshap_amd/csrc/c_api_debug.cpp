// c_api_debug.cpp -- the entry points of libwhatshap_amd_debug.so only (include/whatshap_amd_debug.h): test infrastructure.  (The host
// instantiation of the heuristic, whamd_debug_pedmec_heuristic_create_host, stands beside the product's create in c_api.cpp.)
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/whatshap_amd_debug.h"
#include "c_api.h"
#include "genotype.h"
#include "genotype_plan.h"
#include "slots.h"

using namespace whamd;

extern "C" {

whamd_status_t whamd_debug_emulate_slot_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                            const whamd_pedigree_view* pedigree, int distrust_genotypes, const uint32_t* positions,
                                            size_t n_positions, int slot_l, int symmetry, uint32_t* index_out, uint32_t* score_out,
                                            uint64_t* n_run_columns_out) {
	return guarded([&]() -> whamd_status_t {
	const int lr = slot_l >= 200 ? 1 : slot_l >= 100 ? 3 : 2;   // slot_l + 100: 8 cells per thread, + 200: 2 cells per thread
	if (slot_l >= 100) slot_l -= slot_l >= 200 ? 200 : 100;
	Problem p;
	if (whamd_status_t st = ProblemInputs{readset, recombcost, n_recombcost, pedigree, distrust_genotypes, positions, n_positions}.build(p)) return st;
	SlotPlan sp;
	if (p.T != 1 || !plan_forward_slots(p, slot_l, symmetry, sp, lr)) return fail(WHAMD_ERR_UNSUPPORTED, "slot runs apply to a single individual only");
	std::vector<uint32_t> path;
	uint32_t score = 0;
	std::string msg;
	if (!emulate_slot_plan(p, sp, path, score, msg)) return fail(WHAMD_ERR_INVALID, "slot plan inconsistent: " + msg);
	if (index_out && !path.empty()) std::memcpy(index_out, path.data(), path.size() * sizeof(uint32_t));
	if (score_out) *score_out = score;
	if (n_run_columns_out) *n_run_columns_out = sp.n_run_columns;
	return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_emulate_pedslot_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                               const whamd_pedigree_view* pedigree, int distrust_genotypes, const uint32_t* positions,
                                               size_t n_positions, int slot_l, uint32_t* index_out, uint32_t* transmission_out,
                                               uint32_t* score_out, uint64_t* n_run_columns_out) {
	return guarded([&]() -> whamd_status_t {
	Problem p;
	if (whamd_status_t st = ProblemInputs{readset, recombcost, n_recombcost, pedigree, distrust_genotypes, positions, n_positions}.build(p)) return st;
	SlotPlan sp;
	if (p.T == 1 || !plan_forward_slots(p, slot_l > 0 ? -slot_l : 0, 0, sp) || !sp.ped)
		return fail(WHAMD_ERR_UNSUPPORTED, "pedigree slot runs apply to tables with one or two trios whose columns need at most 4 cost forms per transmission value");
	std::vector<uint32_t> path, trans;
	uint32_t score = 0;
	std::string msg;
	if (!emulate_pedslot_plan(p, sp, path, trans, score, msg)) return fail(WHAMD_ERR_INVALID, "pedigree slot plan inconsistent: " + msg);
	if (index_out && !path.empty()) std::memcpy(index_out, path.data(), path.size() * sizeof(uint32_t));
	if (transmission_out && !trans.empty()) std::memcpy(transmission_out, trans.data(), trans.size() * sizeof(uint32_t));
	if (score_out) *score_out = score;
	if (n_run_columns_out) *n_run_columns_out = sp.n_run_columns;
	return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_lazy_terms_check(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                            const whamd_pedigree_view* pedigree, int distrust_genotypes, const uint32_t* positions, size_t n_positions,
                                            const uint8_t* need_in, int rounds, int* lazy_out, uint64_t* differences_out, uint64_t* built_before_out,
                                            uint64_t* built_after_out) {
	return guarded([&]() -> whamd_status_t {
	const ProblemInputs in{readset, recombcost, n_recombcost, pedigree, distrust_genotypes, positions, n_positions};
	Problem eager, lazy;
	if (whamd_status_t st = in.build(eager)) return st;
	if (whamd_status_t st = in.build(lazy, false, /*lazy_fact_terms=*/true)) return st;
	if (lazy_out) *lazy_out = lazy.lazy_terms ? 1 : 0;
	const uint32_t n = eager.n_cols;
	uint64_t before = 0, after = 0, diff = 0;
	for (uint32_t c = 0; c < n; ++c) before += lazy.term_end(c, lazy.T - 1) > lazy.term_begin(c, 0);
	std::vector<uint8_t> need(n, 1);
	if (need_in) for (uint32_t c = 0; c < n; ++c) need[c] = need_in[c] != 0;
	rounds = std::max(1, rounds);
	std::string msg;
	for (int r = 0; r < rounds; ++r) {
		std::vector<uint8_t> part(n, 0);
		for (uint32_t c = 0; c < n; ++c) part[c] = need[c] && (int)(c % (uint32_t)rounds) == r;
		const whamd_status_t st = fill_lazy_terms(lazy, part, msg);
		if (st != WHAMD_OK) return fail(st, msg);
	}
	for (uint32_t c = 0; c < n; ++c) {
		after += lazy.term_end(c, lazy.T - 1) > lazy.term_begin(c, 0);
		if (!need[c]) continue;
		bool same = true;
		for (uint32_t t = 0; t < eager.T && same; ++t) {
			const uint64_t a0 = eager.term_begin(c, t), a1 = eager.term_end(c, t), b0 = lazy.term_begin(c, t), b1 = lazy.term_end(c, t);
			same = a1 - a0 == b1 - b0;
			for (uint64_t i = 0; same && i < a1 - a0; ++i)
				same = eager.terms[a0 + i].c == lazy.terms[b0 + i].c && eager.terms[a0 + i].plus == lazy.terms[b0 + i].plus && eager.terms[a0 + i].minus == lazy.terms[b0 + i].minus;
		}
		diff += !same;
	}
	// what does not depend on the route: the factorised line itself and the problem's shape
	if (eager.fterm_kind != lazy.fterm_kind || eager.fterms.size() != lazy.fterms.size()) diff += n;
	else for (size_t i = 0; i < eager.fterms.size(); ++i) if (eager.fterms[i].c != lazy.fterms[i].c || eager.fterms[i].plus != lazy.fterms[i].plus || eager.fterms[i].minus != lazy.fterms[i].minus) { ++diff; break; }
	if (lazy.value_bound < eager.value_bound) diff += n;   // (the lazy bound may only be LARGER: it is what rules 32-bit wrap-around out)
	if (differences_out) *differences_out = diff;
	if (built_before_out) *built_before_out = before;
	if (built_after_out) *built_after_out = after;
	return WHAMD_OK;
	});
}

size_t whamd_debug_solve_kernels(whamd_debug_kernel* out, size_t capacity) { return DeviceTable::debug_solve_kernels(out, capacity); }

whamd_status_t whamd_debug_dptable_launches(const whamd_dptable* table, whamd_debug_launch* out, size_t capacity, size_t* n_out) {
	if (!table || !n_out) return fail(WHAMD_ERR_INVALID, "null argument");
	if (!table->solved) return fail(WHAMD_ERR_INVALID, "the table has not been solved: its ledger is read after whamd_dptable_wait");
	*n_out = table->device.debug_launches(out, capacity);
	return WHAMD_OK;
}

whamd_status_t whamd_debug_dptable_preview(const whamd_dptable* table, whamd_debug_preview* out) {
	if (!table || !out) return fail(WHAMD_ERR_INVALID, "null argument");
	table->device.debug_preview(out);
	return WHAMD_OK;
}

whamd_status_t whamd_debug_preview_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                        const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                        const uint32_t* positions, size_t n_positions, uint32_t pieces, whamd_debug_preview_plan_result* out,
                                        uint64_t* rec_predicted, uint64_t* rec_laid_out, uint32_t* spec_predicted, uint32_t* spec_laid_out, size_t capacity) {
	return guarded([&]() -> whamd_status_t {
	if (!out) return fail(WHAMD_ERR_INVALID, "out is NULL");
	Problem p;
	if (whamd_status_t st = ProblemInputs{readset, recombcost, n_recombcost, pedigree, distrust_genotypes, positions, n_positions}.build(p)) return st;
	std::string msg;
	const whamd_status_t st = DeviceTable::debug_preview_plan(p, pieces, out, rec_predicted, rec_laid_out, spec_predicted, spec_laid_out, capacity, msg);
	return st == WHAMD_OK ? WHAMD_OK : fail(st, msg);
	});
}

whamd_status_t whamd_debug_head_first_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                           const whamd_pedigree_view* pedigree, int distrust_genotypes,
                                           const uint32_t* positions, size_t n_positions, uint32_t head_pieces, whamd_debug_head_plan_result* out) {
	return guarded([&]() -> whamd_status_t {
	if (!out) return fail(WHAMD_ERR_INVALID, "out is NULL");
	Problem p;
	if (whamd_status_t st = ProblemInputs{readset, recombcost, n_recombcost, pedigree, distrust_genotypes, positions, n_positions}.build(p)) return st;
	if (p.T != 1) return fail(WHAMD_ERR_UNSUPPORTED, "the head hook applies to a single individual only");
	*out = whamd_debug_head_plan_result{};
	SlotPlan sp;
	SlotPlanHead head;
	const uint32_t n_pieces = slot_plan_pieces(p.n_cols);
	head.col_limit = slot_plan_piece_begin(p.n_cols, std::min(head_pieces, n_pieces));
	uint32_t calls = 0, head_steps = 0;
	uint64_t in_hook = 0;
	head.at_head = [&](uint32_t n_head) {
		++calls;
		head_steps = n_head;
		in_hook = slot_plan_runs_digest(sp, n_head);   // the part of the plan that belongs to the runs [0, n_head)
	};
	if (!plan_forward_slots(p, 11, 1, sp, 2, false, head_pieces ? &head : nullptr)) return fail(WHAMD_ERR_UNSUPPORTED, "the table is not eligible for slot runs");
	out->n_pieces = n_pieces;
	out->head_steps = head_steps;
	out->n_steps = (uint32_t)sp.steps.size();
	out->hook_calls = calls;
	out->head_digest_in_hook = in_hook;
	out->head_digest = slot_plan_runs_digest(sp, head_steps);
	out->n_runs = (uint32_t)sp.runs.size();
	out->n_components = (uint32_t)sp.component_first_step.size();
	out->digest = slot_plan_digest(sp);
	out->edge_yflags[0] = out->edge_yflags[1] = 0xFFFFFFFFu;
	if (head_steps) {
		out->edge_yflags[0] = sp.runs[head_steps - 1].yflags;
		if (head_steps < sp.steps.size() && sp.steps[head_steps].kind == 2) out->edge_yflags[1] = sp.runs[sp.steps[head_steps].index].yflags;
	}
	return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_genotype_run_plan(const whamd_readset_view* readset, const uint32_t* recombcost, size_t n_recombcost,
                                             const whamd_pedigree_view* pedigree, const uint32_t* positions, size_t n_positions,
                                             whamd_debug_genotype_run* out, size_t capacity, size_t* n_out, double* min_total_out) {
	return guarded([&]() -> whamd_status_t {
	if (!n_out) return fail(WHAMD_ERR_INVALID, "n_out is NULL");
	Problem p;
	if (whamd_status_t st = ProblemInputs{readset, recombcost, n_recombcost, pedigree, 0, positions, n_positions}.build(p, /*columns_only=*/true)) return st;
	GenotypeModel model;
	std::string msg;
	const whamd_status_t st = build_genotype_model(p, model, msg);
	if (st != WHAMD_OK) return fail(st, msg);
	GenoRunPlan pl;
	if (!geno_plan_runs(p, model, 0, pl)) return fail(WHAMD_ERR_UNSUPPORTED, "the table is not eligible for the genotyper's run path");
	*n_out = pl.runs.size();
	if (min_total_out) *min_total_out = GS_MIN_TOTAL;
	for (size_t ri = 0; out && ri < pl.runs.size() && ri < capacity; ++ri) {
		const GsRun& r = pl.runs[ri];
		whamd_debug_genotype_run o{};
		o.c0 = r.c0; o.ncols = r.ncols;
		o.rescale_f = r.n_part_in_f ? 1u : 0u; o.rescale_b = r.n_part_in_b ? 1u : 0u;
		o.emit_f = r.emit_f; o.emit_b = r.emit_b;
		o.n_part_out = 1u << r.g;
		o.part_out_f = r.part_out_f; o.part_out_b = r.part_out_b;
		o.part_in_f = r.part_in_f; o.n_part_in_f = r.n_part_in_f;
		o.part_in_b = r.part_in_b; o.n_part_in_b = r.n_part_in_b;
		out[ri] = o;
	}
	return WHAMD_OK;
	});
}

}  // extern "C"
