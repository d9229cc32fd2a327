// polythreader_device.hip -- the polyphase threading DP on gfx950 (polythreader.h).  The sections of all problems of a call are the jobs.
//   upload     per position its list (global ids), its log terms (doubles, made on the host), its ploidy; the tuple table; the sections.
//   count      one workgroup per position: the coverage cost of every tuple (ph_cost), the column's smallest, how many tuples stay
//              within 30 of it.  With WHAMD_POLY_THREADER_WANT_COSTS the costs are also written out.
//   scan       exclusive, two launches (run_scatter.hip): where every column's backtrace records begin, and how many there are (the one
//              wait of the call: the store is allocated exactly).
//   columns    one workgroup per section walks its dependent columns.  The column before stays in LDS (score, slot order, and its
//              tuples as counters over the new column's local ids); a column is: costs again, the survivors compacted in enumeration
//              order (their rank), then one thread per surviving tuple over all predecessors -- ph_offer, the same walk as the host twin,
//              in the same order -- and ph_permute against the winner.  One uint32 per entry goes to the store.
//   backtrace  one thread per section, from the section's end (lowest score, then lowest rank) back through the store: the path in
//              global ids, the coverage cost of every path tuple, the count of decisions the rank made.
// 5 launches per call whatever the problems (PH_LAUNCHES).  No multiplication anywhere: nothing can be contracted.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_runtime.h"
#include "polythreader.h"

#pragma clang fp contract(off)

namespace whamd {
namespace {

constexpr uint32_t B = RS_BLOCK;
constexpr uint32_t PH_GRID_CAP = 1u << 20;

struct PhArgs {
	// the image
	const uint32_t* tuples;
	PhTupleIndex index;
	const uint8_t* pos_n;          // [n_keys] clusters of the position's list
	const uint8_t* pos_ploidy;
	const uint32_t* pos_cov;       // [n_keys] first entry of its list in ids
	const uint64_t* pos_tab;       // [n_keys] first of its terms in tab
	const uint64_t* pos_costs;     // [n_keys] first of its tuples in all_costs (UINT64_MAX: not wanted); nullptr: no problem wants them
	const uint32_t* ids;
	const double* tab;
	const PhSection* sections;
	// made on the device
	uint32_t* counts;              // [n_keys] surviving tuples
	uint32_t* local;
	uint32_t* tile_sums;
	uint32_t* n_entries;           // [1]
	uint32_t* store;               // [n_store] backtrace records
	PhSectionEnd* ends;            // [n_sections]
	uint32_t* paths;
	float* path_cost;              // [n_keys]
	float* all_costs;
	uint64_t n_costs;
	uint32_t n_keys, n_sections, n_store;
};

// The smallest of one value per thread (a < b on floats, as the reference compares).  part: LDS [B / 64].
__device__ inline float block_smallest(float v, float* part) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const float other = __shfl_xor(v, o);
		v = other < v ? other : v;
	}
	if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
	__syncthreads();
	float m = part[0];
#pragma unroll
	for (int w = 1; w < (int)B / 64; w++) m = part[w] < m ? part[w] : m;
	__syncthreads();
	return m;
}

// The terms of position v into LDS, the costs of all its tuples into cost[], the column's prune limit.  Every thread of the workgroup.
__device__ inline float column_costs(const PhArgs& a, uint32_t v, uint32_t P, uint32_t n, const uint32_t* tt, uint32_t nt, double* tab, float* cost, float* part) {
	const double* src = a.tab + a.pos_tab[v];
	for (uint32_t i = threadIdx.x; i < n * P + (1u << n); i += B) tab[i] = src[i];
	__syncthreads();
	float smallest = __builtin_inff();
	for (uint32_t t = threadIdx.x; t < nt; t += B) {
		const float c = ph_cost(tab, P, n, ph_counts(tt[t], P));
		cost[t] = c;
		smallest = c < smallest ? c : smallest;
	}
	return 30.0f + block_smallest(smallest, part);   // (the sync inside: cost[] is complete)
}

__global__ void __launch_bounds__(B) polythreader_count_kernel(PhArgs a) {
	__shared__ double tab[PH_MAX_TABLE];
	__shared__ float cost[PH_MAX_TUPLES];
	__shared__ float part[B / 64];
	__shared__ uint32_t wave_total[B / 64];
	for (uint32_t v = blockIdx.x; v < a.n_keys; v += gridDim.x) {
		const uint32_t P = a.pos_ploidy[v], n = a.pos_n[v], nt = a.index.count[P][n];
		const uint32_t* tt = a.tuples + a.index.begin[P][n];
		const float limit = column_costs(a, v, P, n, tt, nt, tab, cost, part);
		uint32_t mine = 0;
		const uint64_t out = a.pos_costs ? a.pos_costs[v] : UINT64_MAX;
		for (uint32_t t = threadIdx.x; t < nt; t += B) {
			mine += cost[t] > limit ? 0u : 1u;
			if (out != UINT64_MAX && out + t < a.n_costs) a.all_costs[out + t] = cost[t];
		}
		uint32_t total;
		block_exclusive(mine, wave_total, total);
		if (threadIdx.x == 0) a.counts[v] = total;
	}
}

__global__ void __launch_bounds__(B) polythreader_columns_kernel(PhArgs a) {
	__shared__ double tab[PH_MAX_TABLE];
	__shared__ float cost[PH_MAX_TUPLES];
	__shared__ float score[2][PH_MAX_TUPLES];
	__shared__ uint32_t perm[2][PH_MAX_TUPLES];
	__shared__ uint32_t before_counts[PH_MAX_TUPLES];   // the column before over the new column's local ids
	__shared__ uint16_t survivor[PH_MAX_TUPLES];
	__shared__ float part[B / 64];
	__shared__ uint32_t wave_total[B / 64];
	__shared__ uint32_t old_ids[PH_MAX_CLUSTERS], new_ids[PH_MAX_CLUSTERS], old_to_new[PH_MAX_CLUSTERS];
	for (uint32_t job = blockIdx.x; job < a.n_sections; job += gridDim.x) {
		const PhSection sec = a.sections[job];
		const uint32_t P = sec.ploidy;
		uint32_t n_before = 0, n_old = 0, cur = 0;
		for (uint32_t col = 0; col < sec.n; col++, cur ^= 1u) {
			const uint32_t v = sec.first + col, n = a.pos_n[v], nt = a.index.count[P][n];
			const uint32_t* tt = a.tuples + a.index.begin[P][n];
			if (threadIdx.x < n) new_ids[threadIdx.x] = a.ids[a.pos_cov[v] + threadIdx.x];
			const float limit = column_costs(a, v, P, n, tt, nt, tab, cost, part);
			if (threadIdx.x < n_old) {
				uint32_t d = PH_ABSENT;
				for (uint32_t k = 0; k < n; k++) d = new_ids[k] == old_ids[threadIdx.x] ? k : d;
				old_to_new[threadIdx.x] = d;
			}
			__syncthreads();
			const float* score_before = score[cur ^ 1u];
			const uint32_t* perm_before = perm[cur ^ 1u];
			for (uint32_t r = threadIdx.x; r < n_before; r += B) before_counts[r] = ph_counts_in_new(perm_before[r], P, old_to_new);
			// the survivors in enumeration order: every thread a contiguous piece
			const uint32_t per = (nt + B - 1) / B, lo = min(threadIdx.x * per, nt), hi = min(lo + per, nt);
			uint32_t mine = 0;
			for (uint32_t t = lo; t < hi; t++) mine += cost[t] > limit ? 0u : 1u;
			uint32_t n_cur;
			uint32_t at = block_exclusive(mine, wave_total, n_cur);
			for (uint32_t t = lo; t < hi; t++)
				if (!(cost[t] > limit)) survivor[at++] = (uint16_t)t;
			__syncthreads();
			const uint32_t store_at = run_begin(a.local, a.tile_sums, v);
			for (uint32_t r = threadIdx.x; r < n_cur; r += B) {
				const uint32_t t = survivor[r], tuple = tt[t];
				uint32_t record = tuple;
				float s = 0.0f;
				if (col) {
					const uint32_t mine_counts = ph_counts(tuple, P);
					PhBest best{};
					for (uint32_t q = 0; q < n_before; q++) {
						const uint32_t k = P - ph_common(before_counts[q], mine_counts);
						ph_offer(best, q == 0, score_before[q], k, sec.cost[k], q);
					}
					s = best.s;
					record = ph_permute(tuple, perm_before[best.rank], P, old_to_new) | best.rank << PH_PERM_BITS | best.by_rank << PH_TIE_BIT;
				}
				score[cur][r] = s + cost[t];
				perm[cur][r] = record & ((1u << PH_PERM_BITS) - 1u);
				if ((uint64_t)store_at + r < a.n_store) a.store[store_at + r] = record;
			}
			__syncthreads();
			if (threadIdx.x < n) old_ids[threadIdx.x] = new_ids[threadIdx.x];
			n_old = n;
			n_before = n_cur;
			__syncthreads();
		}
		// the end of the section: the lowest score, then the lowest rank; more than one entry of that score is one ambiguity
		if (threadIdx.x == 0) {
			const float* last = score[cur ^ 1u];
			uint32_t r = 0, equal = 0;
			for (uint32_t k = 1; k < n_before; k++) r = last[k] < last[r] ? k : r;
			for (uint32_t k = 0; k < n_before; k++) equal += last[k] == last[r] ? 1u : 0u;
			a.ends[job] = PhSectionEnd{r, __float_as_uint(last[r]), equal > 1 ? 1u : 0u, 0};
		}
		__syncthreads();
	}
}

__global__ void __launch_bounds__(B) polythreader_backtrace_kernel(PhArgs a) {
	const uint32_t job = blockIdx.x * B + threadIdx.x;
	if (job >= a.n_sections) return;
	const PhSection sec = a.sections[job];
	const uint32_t P = sec.ploidy;
	uint32_t r = a.ends[job].rank, ambiguous = a.ends[job].ambiguous;
	for (uint32_t col = sec.n; col-- > 0;) {
		const uint32_t v = sec.first + col, n = a.pos_n[v];
		const uint64_t at = (uint64_t)run_begin(a.local, a.tile_sums, v) + r;
		const uint32_t record = at < a.n_store && r < a.counts[v] ? a.store[at] : 0u;
		const uint32_t* ids = a.ids + a.pos_cov[v];
		uint32_t* path = a.paths + sec.path_at + (uint64_t)col * P;
		for (uint32_t i = 0; i < P; i++) {
			const uint32_t c = (record >> (3 * i)) & 7u;
			path[i] = ids[c < n ? c : 0];
		}
		a.path_cost[v] = ph_cost(a.tab + a.pos_tab[v], P, n, ph_counts(record & ((1u << PH_PERM_BITS) - 1u), P));
		ambiguous += record >> PH_TIE_BIT & 1u;
		r = record >> PH_PERM_BITS & ((1u << PH_RANK_BITS) - 1u);
	}
	a.ends[job].ambiguous = ambiguous;
}

}  // namespace

whamd_status_t polythreader_device(const std::vector<ThreaderProblem>& ps, int device, std::vector<ThreaderPaths>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(ps.size(), ThreaderPaths{});
	PhTupleIndex index;
	const std::vector<uint32_t>& table = ph_tuple_table(index);
	std::vector<uint64_t> pos_base(ps.size() + 1, 0), cov_base(ps.size() + 1, 0), tab_base(ps.size() + 1, 0), sec_base(ps.size() + 1, 0), path_base(ps.size() + 1, 0),
		costs_base(ps.size() + 1, 0);
	uint64_t n_tuples = 0;
	bool want_costs = false;
	for (size_t x = 0; x < ps.size(); x++) {
		pos_base[x + 1] = pos_base[x] + ps[x].n_pos;
		cov_base[x + 1] = cov_base[x] + ps[x].cov_cluster.size();
		tab_base[x + 1] = tab_base[x] + ps[x].tab.size();
		sec_base[x + 1] = sec_base[x] + ps[x].sections.size();
		path_base[x + 1] = path_base[x] + ps[x].n_pos * ps[x].ploidy;
		costs_base[x + 1] = costs_base[x] + (ps[x].want_costs ? ps[x].n_tuples : 0);
		n_tuples += ps[x].n_tuples;
		want_costs |= ps[x].want_costs;
	}
	const uint64_t n_keys = pos_base[ps.size()], n_cov = cov_base[ps.size()], n_tab = tab_base[ps.size()], n_sections = sec_base[ps.size()],
	               n_path = path_base[ps.size()], n_costs = costs_base[ps.size()];
	if (!n_sections) return WHAMD_OK;   // no position anywhere: no device work at all
	if (n_keys >= 0xfffff000ull || n_cov >= 0xfffff000ull || n_tuples >= 0xfffff000ull) {
		msg = "the backtrace store does not fit: 2^32 - 4096 or more positions, list entries or tuples in one call (" + std::to_string(n_tuples) + " tuples)";
		return WHAMD_ERR_UNSUPPORTED;
	}
	ImageLayout in;
	const auto p_tab = in.add<double>(n_tab);
	const auto p_pos_tab = in.add<uint64_t>(n_keys);
	const auto p_pos_costs = in.add<uint64_t>(want_costs ? n_keys : 0);
	const auto p_sections = in.add<PhSection>(n_sections);
	const auto p_tuples = in.add<uint32_t>(table.size());
	const auto p_pos_cov = in.add<uint32_t>(n_keys);
	const auto p_ids = in.add<uint32_t>(n_cov);
	const auto p_pos_n = in.add<uint8_t>(n_keys);
	const auto p_pos_ploidy = in.add<uint8_t>(n_keys);
	ImageLayout work;
	const auto w_counts = work.add<uint32_t>(n_keys);
	const auto w_local = work.add<uint32_t>(n_keys);
	const auto w_tiles = work.add<uint32_t>(rs_tiles(n_keys));
	const auto w_n_entries = work.add<uint32_t>(1);
	ImageLayout results;
	const auto r_ends = results.add<PhSectionEnd>(n_sections);
	const auto r_paths = results.add<uint32_t>(n_path);
	const auto r_path_cost = results.add<float>(n_keys);
	const auto r_all_costs = results.add<float>(n_costs);
	ImageLayout fetched;
	const auto f_n_entries = fetched.add<uint32_t>(1);
	const auto f_counts = fetched.add<uint32_t>(n_keys);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, wk, res, got;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.work(work, wk, msg));
	WHAMD_TRY(s.stage(results, res, msg));   // written by the kernels, fetched whole
	WHAMD_TRY(s.results(fetched, got, msg));
	// the image
	std::memcpy(im.host(p_tuples), table.data(), table.size() * sizeof(uint32_t));
	for (size_t x = 0; x < ps.size(); x++) {
		const ThreaderProblem& p = ps[x];
		if (!p.tab.empty()) std::memcpy(im.host(p_tab) + tab_base[x], p.tab.data(), p.tab.size() * sizeof(double));
		if (!p.cov_cluster.empty()) std::memcpy(im.host(p_ids) + cov_base[x], p.cov_cluster.data(), p.cov_cluster.size() * sizeof(uint32_t));
		uint64_t tuples_before = 0;
		for (uint64_t y = 0; y < p.n_pos; y++) {
			const uint64_t v = pos_base[x] + y;
			const uint32_t n = (uint32_t)(p.cov_ptr[y + 1] - p.cov_ptr[y]);
			im.host(p_pos_tab)[v] = tab_base[x] + p.tab_ptr[y];
			im.host(p_pos_cov)[v] = (uint32_t)(cov_base[x] + p.cov_ptr[y]);
			im.host(p_pos_n)[v] = (uint8_t)n;
			im.host(p_pos_ploidy)[v] = (uint8_t)p.ploidy;
			if (want_costs) im.host(p_pos_costs)[v] = p.want_costs ? costs_base[x] + tuples_before : UINT64_MAX;
			tuples_before += index.count[p.ploidy][n];
		}
		for (size_t k = 0; k < p.sections.size(); k++) {
			PhSection& sec = im.host(p_sections)[sec_base[x] + k];
			sec = PhSection{};
			sec.first = (uint32_t)(pos_base[x] + p.sections[k].first);
			sec.n = (uint32_t)p.sections[k].second;
			sec.ploidy = p.ploidy;
			sec.path_at = path_base[x] + p.sections[k].first * p.ploidy;
			std::memcpy(sec.cost, p.cost, sizeof sec.cost);
		}
	}
	WHAMD_TRY(s.upload(im, msg));
	PhArgs a{};
	a.tuples = im.dev(p_tuples);
	a.index = index;
	a.pos_n = im.dev(p_pos_n);
	a.pos_ploidy = im.dev(p_pos_ploidy);
	a.pos_cov = im.dev(p_pos_cov);
	a.pos_tab = im.dev(p_pos_tab);
	a.pos_costs = want_costs ? im.dev(p_pos_costs) : nullptr;
	a.ids = im.dev(p_ids);
	a.tab = im.dev(p_tab);
	a.sections = im.dev(p_sections);
	a.counts = wk.dev_out(w_counts);
	a.local = wk.dev_out(w_local);
	a.tile_sums = wk.dev_out(w_tiles);
	a.n_entries = wk.dev_out(w_n_entries);
	a.ends = res.dev_out(r_ends);
	a.paths = res.dev_out(r_paths);
	a.path_cost = res.dev_out(r_path_cost);
	a.all_costs = res.dev_out(r_all_costs);
	a.n_costs = n_costs;
	a.n_keys = (uint32_t)n_keys;
	a.n_sections = (uint32_t)n_sections;
	WHAMD_TRY(rs_launch(s, times, msg, polythreader_count_kernel, dim3(grid_for(n_keys, 1, PH_GRID_CAP)), a));
	WHAMD_TRY(rs_scan(s, times, msg, a.counts, a.local, a.tile_sums, a.n_keys, nullptr, a.n_entries));
	WHAMD_TRY(s.fetch_now(got, f_n_entries, a.n_entries, msg));   // the number of backtrace records
	const uint64_t n_store = *got.host(f_n_entries);
	if (!n_store || n_store > n_tuples) {
		msg = "internal error: the surviving tuples and the tuples disagree";
		return WHAMD_ERR_DEVICE;
	}
	void* store = nullptr;
	{
		std::string why;
		if (s.device_block(n_store * sizeof(uint32_t), &store, why) != WHAMD_OK) {
			msg = "the backtrace store does not fit the device: " + std::to_string(n_store) + " records of 4 bytes (" + why + ")";
			return WHAMD_ERR_UNSUPPORTED;
		}
	}
	a.store = (uint32_t*)store;
	a.n_store = (uint32_t)n_store;
	WHAMD_TRY(rs_launch(s, times, msg, polythreader_columns_kernel, dim3(grid_for(n_sections, 1, PH_GRID_CAP)), a));
	WHAMD_TRY(rs_launch(s, times, msg, polythreader_backtrace_kernel, dim3(grid_for(n_sections, B)), a));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(got, f_counts, a.counts, msg));
	WHAMD_TRY(s.fetch(res.stage, res.base, res.total, msg));
	WHAMD_TRY(s.finish(times, msg));
	// back to the problems
	for (size_t x = 0; x < ps.size(); x++) {
		const ThreaderProblem& p = ps[x];
		ThreaderPaths& o = out[x];
		o.paths.assign(res.host(r_paths) + path_base[x], res.host(r_paths) + path_base[x + 1]);
		o.path_cost.assign(res.host(r_path_cost) + pos_base[x], res.host(r_path_cost) + pos_base[x + 1]);
		if (p.want_costs) o.all_costs.assign(res.host(r_all_costs) + costs_base[x], res.host(r_all_costs) + costs_base[x + 1]);
		for (uint64_t y = 0; y < p.n_pos; y++) o.n_entries += got.host(f_counts)[pos_base[x] + y];
		for (size_t k = 0; k < p.sections.size(); k++) {
			const PhSectionEnd& e = res.host(r_ends)[sec_base[x] + k];
			float score;
			std::memcpy(&score, &e.score_bits, sizeof score);
			o.score.push_back(score);
			o.ambiguous.push_back(e.ambiguous);
		}
	}
	return WHAMD_OK;
}

}  // namespace whamd
