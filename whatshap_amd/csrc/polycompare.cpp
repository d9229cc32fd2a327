// polycompare.cpp -- the host side of comparing polyploid phasings (polycompare.h): validation, the matching positions, the expansion
// of a job's path into permutations, flipped haplotypes and switches per position, the C ABI of whatshap_amd.h's comparing section; and,
// in the debug library only, the one-thread host twin of the kernel (whamd_debug_poly_compare_host).
#include "polycompare.h"

#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

whamd_status_t whamd::compare_prepare(const whamd_poly_compare_view& v, CompareJob& job, std::string& msg) {
	if (v.ploidy < 2) {
		msg = "ploidy " + std::to_string(v.ploidy) + " below 2";
		return WHAMD_ERR_INVALID;
	}
	if (!(v.switch_cost >= 0.0) || !(v.flip_cost >= 0.0) || std::isinf(v.switch_cost) || std::isinf(v.flip_cost)) {
		msg = "switch_cost and flip_cost must be finite and not negative";
		return WHAMD_ERR_INVALID;
	}
	if (v.n_pos && (!v.phasing0 || !v.phasing1)) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (v.ploidy > PC_MAX_PLOIDY) {
		msg = "ploidy " + std::to_string(v.ploidy) + " above " + std::to_string(PC_MAX_PLOIDY) + ": " + std::to_string(PC_MAX_PLOIDY + 1) +
		      "! permutation states per position are not supported";
		return WHAMD_ERR_UNSUPPORTED;
	}
	if (v.n_pos > PC_MAX_POSITIONS) {
		msg = "more than 2^28 positions in one job";
		return WHAMD_ERR_UNSUPPORTED;
	}
	job.k = v.ploidy;
	job.n_states = pr_factorial(v.ploidy);
	job.n_pos = v.n_pos;
	job.p0 = v.phasing0;
	job.p1 = v.phasing1;
	job.switch_cost = v.switch_cost;
	job.flip_cost = v.flip_cost;
	job.matched_only = v.matched_only != 0;
	job.want_path = v.want_path != 0;
	job.n_matched = 0;
	for (uint64_t x = 0; x < v.n_pos; x++) job.n_matched += pc_matched(pc_column(v.phasing0 + x * job.k, job.k), pc_column(v.phasing1 + x * job.k, job.k), job.k);
	job.n_visited = job.matched_only ? job.n_matched : job.n_pos;
	return WHAMD_OK;
}

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
void whamd::compare_host(const CompareJob& job, CompareResult& out) {
	out = CompareResult{};
	if (!job.n_visited) return;
	const uint32_t k = job.k, n = job.n_states;
	std::vector<uint32_t> perm(n);
	for (uint32_t r = 0; r < n; r++) perm[r] = pr_unrank(r, k);
	std::vector<double> score[2] = {std::vector<double>(n), std::vector<double>(n)};
	std::vector<uint32_t> flips[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)}, sw[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
	std::vector<uint64_t> ham(n, 0);
	std::vector<uint16_t> pred;
	if (job.want_path) pred.assign(job.n_visited * n, 0);
	uint32_t cur = 0;
	uint64_t v = 0;
	for (uint64_t x = 0; x < job.n_pos; x++) {
		const uint64_t c0 = pc_column(job.p0 + x * k, k), c1 = pc_column(job.p1 + x * k, k);
		if (job.matched_only && !pc_matched(c0, c1, k)) continue;
		for (uint32_t r = 0; r < n; r++) {
			const uint32_t f = pc_flips(perm[r], c0, c1, k);
			ham[r] += f;
			PcBest best = pc_best_none();
			if (v)
				for (uint32_t q = 0; q < n; q++) pc_consider(best, score[cur][q], flips[cur][q], q, job.switch_cost, pc_switches(perm[r], perm[q]));
			score[cur ^ 1][r] = pc_state_score(v == 0, best.value, job.flip_cost, f);
			flips[cur ^ 1][r] = (v ? flips[cur][best.q] : 0u) + f;
			sw[cur ^ 1][r] = v ? sw[cur][best.q] + pc_switches(perm[r], perm[best.q]) : 0u;
			if (job.want_path && v) pred[v * n + r] = (uint16_t)best.q;
		}
		cur ^= 1;
		++v;
	}
	uint32_t end = 0;
	uint64_t min_ham = ham[0];
	for (uint32_t r = 1; r < n; r++) {
		if (pc_end_better(score[cur][r], flips[cur][r], score[cur][end], flips[cur][end])) end = r;
		if (ham[r] < min_ham) min_ham = ham[r];
	}
	out.out = PcOut{score[cur][end], min_ham, pc_end_switches(job.n_visited, perm[end], sw[cur][end]), flips[cur][end]};
	if (job.want_path) {
		out.path.resize(job.n_visited);
		uint32_t r = end;
		for (uint64_t y = job.n_visited; y-- > 0;) {
			out.path[y] = (uint16_t)r;
			if (y) r = pred[y * n + r];
		}
	}
}
#endif

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_poly_compare_result {
	struct Job {
		whamd_poly_compare_job_result res{};
		uint32_t k = 0;
		std::vector<uint16_t> rank;                     // want_path: per visited position
		std::vector<uint64_t> position;
		std::vector<uint8_t> perm, flipped;             // [visited][k]
		std::vector<uint32_t> switches;
	};
	std::vector<Job> jobs;
	whamd_poly_compare_stats stats{};
};

namespace {

// The path's ranks to what the reference's three lists hold, front to back.
void expand_path(const CompareJob& job, const std::vector<uint16_t>& path, whamd_poly_compare_result::Job& o) {
	const uint32_t k = job.k;
	const uint64_t n = path.size();
	o.rank = path;
	o.position.resize(n);
	o.perm.resize(n * k);
	o.flipped.resize(n * k);
	o.switches.resize(n);
	uint64_t v = 0;
	uint32_t before = 0;
	for (uint64_t x = 0; x < job.n_pos && v < n; x++) {
		const uint64_t c0 = pc_column(job.p0 + x * k, k), c1 = pc_column(job.p1 + x * k, k);
		if (job.matched_only && !pc_matched(c0, c1, k)) continue;
		const uint32_t perm = pr_unrank(path[v], k), mask = pc_flipped_mask(perm, c0, c1, k);
		o.position[v] = x;
		for (uint32_t i = 0; i < k; i++) {
			o.perm[v * k + i] = (uint8_t)((perm >> (4 * i)) & 15u);
			o.flipped[v * k + i] = (uint8_t)((mask >> i) & 1u);
		}
		o.switches[v] = v ? pc_switches(perm, before) : pc_end_switches(n, perm, 0);
		before = perm;
		++v;
	}
}

whamd_status_t compare(const whamd_poly_compare_view* views, uint64_t n, int device, bool host, whamd_poly_compare_result** out) {
	if (!out || (n && !views)) return fail(WHAMD_ERR_INVALID, "null argument");
	*out = nullptr;
	BatchClock clock;
	clock.t0 = now_ms();
	std::vector<CompareJob> jobs(n);
	std::vector<CompareResult> results(n);
	std::string msg;
	uint64_t path_bytes = 0, n_positions = 0, n_visited = 0;
	for (uint64_t x = 0; x < n; x++) {
		const whamd_status_t st = compare_prepare(views[x], jobs[x], msg);
		if (st != WHAMD_OK) return fail(st, n > 1 ? "job " + std::to_string(x) + ": " + msg : msg);
		n_positions += jobs[x].n_pos;
		n_visited += jobs[x].n_visited;
		if (jobs[x].want_path) path_bytes += jobs[x].n_visited * jobs[x].n_states * sizeof(uint16_t);
	}
	if (path_bytes > WHAMD_POLY_COMPARE_MAX_PATH_BYTES)
		return fail(WHAMD_ERR_UNSUPPORTED, "the want_path tables of this call take " + std::to_string(path_bytes) + " bytes, above WHAMD_POLY_COMPARE_MAX_PATH_BYTES (" +
		                                       std::to_string(WHAMD_POLY_COMPARE_MAX_PATH_BYTES) + ")");
	clock.t1 = now_ms();
	CallTimes times;
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		for (uint64_t x = 0; x < n; x++) compare_host(jobs[x], results[x]);
#endif
	} else {
		const whamd_status_t st = compare_device(jobs, device, results, times, msg);
		if (st != WHAMD_OK) return fail(st, msg);
	}
	std::unique_ptr<whamd_poly_compare_result> r(new whamd_poly_compare_result());
	r->jobs.resize(n);
	for (uint64_t x = 0; x < n; x++) {
		whamd_poly_compare_result::Job& o = r->jobs[x];
		const PcOut& po = results[x].out;
		o.k = jobs[x].k;
		o.res = whamd_poly_compare_job_result{po.total, jobs[x].n_matched, jobs[x].n_visited, po.min_hamming_sum, po.switches, po.flips};
		if (jobs[x].want_path) expand_path(jobs[x], results[x].path, o);
	}
	whamd_poly_compare_stats& s = r->stats;
	s.n_jobs = n;
	s.n_positions = n_positions;
	s.n_visited = n_visited;
	s.path_bytes = path_bytes;
	clock.t3 = now_ms();
	stamp_times(s, times, clock);
	*out = r.release();
	return WHAMD_OK;
}

}  // namespace

extern "C" {

whamd_status_t whamd_poly_compare(const whamd_poly_compare_view* jobs, uint64_t n_jobs, int device, whamd_poly_compare_result** out) {
	return guarded([&]() -> whamd_status_t { return compare(jobs, n_jobs, device, false, out); });
}

uint64_t whamd_poly_compare_job_count(const whamd_poly_compare_result* r) { return r ? r->jobs.size() : 0; }

uint64_t whamd_poly_compare_path_count(const whamd_poly_compare_result* r, uint64_t j) { return r && j < r->jobs.size() ? r->jobs[j].rank.size() : 0; }

whamd_status_t whamd_poly_compare_get(const whamd_poly_compare_result* r, whamd_poly_compare_job_result* results_out) {
	if (!r || (!results_out && !r->jobs.empty())) return fail(WHAMD_ERR_INVALID, "null argument");
	for (size_t x = 0; x < r->jobs.size(); x++) results_out[x] = r->jobs[x].res;
	return WHAMD_OK;
}

whamd_status_t whamd_poly_compare_get_path(const whamd_poly_compare_result* r, uint64_t j, uint64_t* position_out, uint16_t* rank_out, uint8_t* perm_out,
                                           uint8_t* flipped_out, uint32_t* switches_out) {
	if (!r || j >= r->jobs.size()) return fail(WHAMD_ERR_INVALID, r ? "job index out of range" : "null argument");
	const auto& o = r->jobs[j];
	copy_out(position_out, o.position);
	copy_out(rank_out, o.rank);
	copy_out(perm_out, o.perm);
	copy_out(flipped_out, o.flipped);
	copy_out(switches_out, o.switches);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_compare_get_stats(const whamd_poly_compare_result* r, whamd_poly_compare_stats* stats_out) {
	if (!r || !stats_out) return fail(WHAMD_ERR_INVALID, "null argument");
	*stats_out = r->stats;
	return WHAMD_OK;
}

void whamd_poly_compare_destroy(whamd_poly_compare_result* r) { delete r; }

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_poly_compare_host(const whamd_poly_compare_view* jobs, uint64_t n_jobs, whamd_poly_compare_result** out) {
	return guarded([&]() -> whamd_status_t { return compare(jobs, n_jobs, 0, true, out); });
}
#endif

}  // extern "C"
