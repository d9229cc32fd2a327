// c_api.h -- what c_api.cpp and c_api_debug.cpp share: the table handle and the preamble of every entry point that flattens a table.
#pragma once
#include <string>

#include "api_guard.h"
#include "device_table.h"
#include "problem.h"

struct whamd_dptable {
	whamd::Problem problem;
	whamd::Solution solution;
	whamd::DeviceTable device;
	whamd_solve_stats stats{};
	int device_index = 0;
	bool uploaded = false;
	bool solved = false;
	bool in_flight = false;
};

namespace whamd {

// The seven arguments such an entry point is handed (whatshap_amd.h), in their order.  build(): build_problem on them; a failure is reported the
// way entry points report (fail(): the status, the message for whamd_last_error).
struct ProblemInputs {
	const whamd_readset_view* readset;
	const uint32_t* recombcost;
	size_t n_recombcost;
	const whamd_pedigree_view* pedigree;
	int distrust_genotypes;
	const uint32_t* positions;
	size_t n_positions;
	whamd_status_t build(Problem& p, bool columns_only = false, bool lazy_fact_terms = false) const {
		std::string msg;
		const whamd_status_t st = build_problem(readset, recombcost, n_recombcost, pedigree, distrust_genotypes != 0, positions, n_positions, p, msg,
		                                        columns_only, lazy_fact_terms);
		return st == WHAMD_OK ? WHAMD_OK : fail(st, msg);
	}
};

}  // namespace whamd
