// polythread.cpp -- the host side of the polyphase threading inputs (polythread.h): validation, the matrix rows (polyscore.cpp), every
// read's (cluster, rank) from the clustering CSR, the sequential gap filling of select_clusters, result assembly, the C ABI of
// whatshap_amd.h's threading section; and, in the debug library only, the one-thread host twins.
#include "polythread.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <memory>

#include "../../include/whatshap_amd_debug.h"
#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

namespace {

constexpr uint64_t NONE = std::numeric_limits<uint64_t>::max();

bool ploidy_ok(uint32_t ploidy, std::string& msg) {
	if (ploidy >= 1 && ploidy <= PT_MAX_PLOIDY) return true;
	msg = "ploidy " + std::to_string(ploidy) + " outside 1 .. " + std::to_string(PT_MAX_PLOIDY);
	return false;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- validation, reads to (cluster, rank)
whamd_status_t whamd::polythread_prepare(const whamd_poly_thread_view& v, ThreadProblem& p, std::string& msg) {
	if (!ploidy_ok(v.ploidy, msg)) return WHAMD_ERR_INVALID;
	if (v.n_alleles < 1 || v.n_alleles > PT_MAX_ALLELES) {
		msg = "n_alleles " + std::to_string(v.n_alleles) + " outside 1 .. " + std::to_string(PT_MAX_ALLELES);
		return WHAMD_ERR_INVALID;
	}
	if (v.flags & ~WHAMD_POLY_THREAD_DEPTHS_ONLY) {
		msg = "unknown flag bits";
		return WHAMD_ERR_INVALID;
	}
	const whamd_status_t st = poly_build_matrix(v.matrix, p.m, msg);
	if (st != WHAMD_OK) return st;
	if (p.m.max_allele > v.n_alleles) {
		msg = "allele " + std::to_string(p.m.max_allele - 1) + " outside 0 .. " + std::to_string(v.n_alleles - 1) + " (out of range)";
		return WHAMD_ERR_INVALID;
	}
	p.view = &v;
	p.ploidy = v.ploidy;
	p.n_alleles = v.n_alleles;
	p.depths_only = (v.flags & WHAMD_POLY_THREAD_DEPTHS_ONLY) != 0;
	const uint64_t n_reads = p.m.n_reads, n_clusters = v.n_clusters;
	if (n_clusters >= 0xffffffffull) {
		msg = "2^32 - 1 or more clusters";
		return WHAMD_ERR_UNSUPPORTED;
	}
	if (n_clusters && !v.cluster_ptr) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	if (!check_offsets(v.cluster_ptr, n_clusters, "cluster_ptr", "cluster", msg)) return WHAMD_ERR_INVALID;
	for (uint64_t c = 0; c < n_clusters; c++)
		if (v.cluster_ptr[c + 1] - v.cluster_ptr[c] >= PT_MAX_RANK) {
			msg = "cluster " + std::to_string(c) + " has 2^28 or more reads";
			return WHAMD_ERR_UNSUPPORTED;
		}
	if (n_clusters && v.cluster_ptr[n_clusters] && !v.cluster_reads) {
		msg = "null argument";
		return WHAMD_ERR_INVALID;
	}
	p.reads.assign(n_reads, PtRead{PT_NONE, 0, 0});
	std::vector<uint8_t> covered(p.m.n_positions, 0);
	for (uint64_t c = 0; c < n_clusters; c++)
		for (uint64_t k = v.cluster_ptr[c]; k < v.cluster_ptr[c + 1]; k++) {
			const uint32_t r = v.cluster_reads[k];
			if (r >= n_reads) {
				msg = "cluster " + std::to_string(c) + ": read id " + std::to_string(r) + " out of range (" + std::to_string(n_reads) + " reads)";
				return WHAMD_ERR_INVALID;
			}
			if (p.reads[r].cluster != PT_NONE) {
				msg = "read " + std::to_string(r) + " is in two clusters (" + std::to_string(p.reads[r].cluster) + " and " + std::to_string(c) +
				      "): every read can only be present in one cluster, once";
				return WHAMD_ERR_INVALID;
			}
			p.reads[r] = PtRead{(uint32_t)c, (uint32_t)(k - v.cluster_ptr[c]), 0};
			p.n_counted += p.m.row_ptr[r + 1] - p.m.row_ptr[r];
			for (uint64_t x = p.m.row_ptr[r]; x < p.m.row_ptr[r + 1]; x++) covered[p.m.row_pos[x]] = 1;
		}
	if (!p.depths_only)
		for (uint64_t x = 0; x < covered.size(); x++)
			if (!covered[x]) {
				msg = "position " + std::to_string(x) + " has no counted entry: no read of a cluster covers it";
				return WHAMD_ERR_INVALID;
			}
	return WHAMD_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------- gap filling (select_clusters, second loop)
// cov: [n_pos * stride] the lists, n_cov[p] entries each -- on entry the original selection in its order, on return extended (not sorted).
// ids are below n_ids.  Sequential over the positions; O(1) per candidate: nxt[cid] is the next position of cid's original selection
// behind the last one passed.  A candidate at p came down an unbroken chain from an original selection at some q < p and is not in the
// original selection of q + 1 .. p, so nxt[cid] is exactly its next original selection behind p.
void pt_fill_gaps(uint64_t n_pos, uint32_t stride, uint64_t max_gap, uint64_t n_ids, std::vector<uint32_t>& cov, std::vector<uint32_t>& n_cov) {
	if (n_pos < 3) return;
	std::vector<uint64_t> next_of(cov.size(), NONE), last(n_ids, NONE), nxt(n_ids, NONE);
	for (uint64_t p = n_pos; p-- > 0;)
		for (uint32_t s = 0; s < n_cov[p]; s++) {
			const uint32_t cid = cov[p * stride + s];
			next_of[p * stride + s] = last[cid];
			last[cid] = p;
		}
	std::vector<uint32_t> n_orig(n_cov);
	const auto pass = [&](uint64_t p) {
		for (uint32_t s = 0; s < n_orig[p]; s++) nxt[cov[p * stride + s]] = next_of[p * stride + s];
	};
	pass(0);
	for (uint64_t p = 1; p + 1 < n_pos; p++) {
		uint32_t* mine = cov.data() + p * stride;
		const uint32_t* before = cov.data() + (p - 1) * stride;
		for (uint32_t s = 0; s < n_cov[p - 1]; s++) {
			if (n_cov[p] >= stride) break;
			const uint32_t cid = before[s];
			if (std::find(mine, mine + n_cov[p], cid) != mine + n_cov[p]) continue;
			if (nxt[cid] != NONE && nxt[cid] - p <= max_gap) mine[n_cov[p]++] = cid;
		}
		pass(p);
	}
}

struct CovLists {
	std::vector<uint64_t> ptr;
	std::vector<uint32_t> cluster, rank;
	std::vector<uint8_t> readded;
};

// The extended lists, every position sorted ascending.
void pt_sorted_lists(uint64_t n_pos, uint32_t stride, const std::vector<uint32_t>& cov, const std::vector<uint32_t>& n_cov, const std::vector<uint32_t>& n_orig,
                     CovLists& out) {
	out.ptr.assign(n_pos + 1, 0);
	for (uint64_t p = 0; p < n_pos; p++) out.ptr[p + 1] = out.ptr[p] + n_cov[p];
	out.cluster.resize(out.ptr[n_pos]);
	out.rank.resize(out.ptr[n_pos]);
	out.readded.resize(out.ptr[n_pos]);
	std::vector<std::pair<uint32_t, uint32_t>> one;
	for (uint64_t p = 0; p < n_pos; p++) {
		one.clear();
		for (uint32_t s = 0; s < n_cov[p]; s++) one.emplace_back(cov[p * stride + s], s);
		std::sort(one.begin(), one.end());
		for (uint32_t s = 0; s < n_cov[p]; s++) {
			out.cluster[out.ptr[p] + s] = one[s].first;
			out.rank[out.ptr[p] + s] = one[s].second;
			out.readded[out.ptr[p] + s] = one[s].second >= n_orig[p] ? 1 : 0;
		}
	}
}

// ---------------------------------------------------------------------------------------------- host twin (debug library)
#ifdef WHAMD_DEBUG_BUILD
template <int NA>
void rows_of_runs(const ThreadProblem& p, const std::vector<uint64_t>& begin, std::vector<PtPlaced>& placed, ThreadRows& out) {
	const uint64_t n_pos = p.m.n_positions;
	for (uint64_t x = 0; x < n_pos; x++) {
		PtPlaced* run = placed.data() + begin[x];
		const uint64_t n = begin[x + 1] - begin[x];
		std::sort(run, run + n, [](const PtPlaced& a, const PtPlaced& b) { return a.cluster < b.cluster; });
		uint32_t rows = 0;
		for (uint64_t k = 0; k < n;) {
			uint32_t cnt[NA], first[NA], total = 0;
			for (int a = 0; a < NA; a++) {
				cnt[a] = 0;
				first[a] = PT_NONE;
			}
			const uint32_t c = run[k].cluster;
			for (; k < n && run[k].cluster == c; k++) {
				const uint32_t a = run[k].rank_allele & 15u, rank = run[k].rank_allele >> 4;
				++cnt[a];
				++total;
				first[a] = std::min(first[a], rank);
			}
			out.cluster.push_back(c);
			out.total.push_back(total);
			out.depth.insert(out.depth.end(), cnt, cnt + NA);
			out.first.insert(out.first.end(), first, first + NA);
			int8_t cons[PT_MAX_PLOIDY];
			pt_consensus<NA>(cnt, first, p.ploidy, cons);
			out.cons.insert(out.cons.end(), cons, cons + p.ploidy);
			++rows;
		}
		out.npc[x] = rows;
		if (n) ++(n <= PT_CLASS_A_MAX ? out.class_a : n <= PT_CLASS_B_MAX ? out.class_b : out.class_c);
	}
}

void select_host(const std::vector<uint32_t>& begin, const std::vector<uint32_t>& count, const std::vector<uint32_t>& total, uint32_t ploidy,
                 std::vector<uint32_t>& n_sel, std::vector<uint32_t>& sel) {
	const uint64_t n_pos = count.size();
	n_sel.assign(n_pos, 0);
	sel.assign(n_pos * (ploidy + 2), 0);
	for (uint64_t x = 0; x < n_pos; x++) n_sel[x] = pt_select(total.data() + begin[x], count[x], ploidy, sel.data() + x * (ploidy + 2));
}

void polythread_host(const ThreadProblem& p, ThreadRows& out) {
	const uint64_t n_pos = p.m.n_positions;
	std::vector<uint64_t> begin(n_pos + 1, 0);
	for (uint64_t r = 0; r < p.m.n_reads; r++)
		if (p.reads[r].cluster != PT_NONE)
			for (uint64_t x = p.m.row_ptr[r]; x < p.m.row_ptr[r + 1]; x++) ++begin[p.m.row_pos[x] + 1];
	for (uint64_t x = 0; x < n_pos; x++) begin[x + 1] += begin[x];
	std::vector<uint64_t> cursor(begin.begin(), begin.end() - 1);
	std::vector<PtPlaced> placed(begin[n_pos]);
	for (uint64_t r = 0; r < p.m.n_reads; r++)
		if (p.reads[r].cluster != PT_NONE)
			for (uint64_t x = p.m.row_ptr[r]; x < p.m.row_ptr[r + 1]; x++)
				placed[cursor[p.m.row_pos[x]]++] = PtPlaced{p.reads[r].cluster, p.reads[r].rank << 4 | p.m.row_allele[x]};
	out.npc.assign(n_pos, 0);
	out.na = p.n_alleles <= 4 ? 4 : 16;
	if (out.na == 4) rows_of_runs<4>(p, begin, placed, out);
	else rows_of_runs<16>(p, begin, placed, out);
	std::vector<uint32_t> row_begin(n_pos, 0);
	for (uint64_t x = 1; x < n_pos; x++) row_begin[x] = row_begin[x - 1] + out.npc[x - 1];
	select_host(row_begin, out.npc, out.total, p.ploidy, out.n_sel, out.sel);
}
#endif

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_poly_thread_result {
	struct Problem {
		uint32_t ploidy = 0, n_alleles = 0;
		std::vector<uint64_t> pc_ptr;
		std::vector<uint32_t> cluster, depth, first;
		std::vector<int8_t> cons;
		CovLists cov;
		whamd_poly_thread_stats stats{};
	};
	std::vector<Problem> problems;
};

namespace {

void assemble(const ThreadProblem& p, const ThreadRows& rows, whamd_poly_thread_result::Problem& out) {
	const uint64_t n_pos = p.m.n_positions, n_rows = rows.cluster.size();
	const uint32_t na = p.n_alleles, P = p.ploidy, stride = P + 2;
	out.ploidy = P;
	out.n_alleles = na;
	whamd_poly_thread_stats& s = out.stats;
	s.n_reads = p.m.n_reads;
	s.n_positions = n_pos;
	s.n_entries = p.m.row_pos.size();
	s.n_counted = p.n_counted;
	s.n_rows = n_rows;
	s.positions_class_a = rows.class_a;
	s.positions_class_b = rows.class_b;
	s.positions_class_c = rows.class_c;
	out.pc_ptr.assign(n_pos + 1, 0);
	for (uint64_t x = 0; x < n_pos && x < rows.npc.size(); x++) out.pc_ptr[x + 1] = out.pc_ptr[x] + rows.npc[x];
	out.cluster = rows.cluster;
	out.cons = rows.cons;
	out.depth.resize(n_rows * na);
	out.first.resize(n_rows * na);
	for (uint64_t r = 0; r < n_rows; r++)
		for (uint32_t a = 0; a < na; a++) {
			out.depth[r * na + a] = rows.depth[r * rows.na + a];
			out.first[r * na + a] = rows.first[r * rows.na + a];
		}
	out.cov.ptr.assign(n_pos + 1, 0);
	if (p.depths_only || !n_pos) return;
	// the lists as cluster ids, filled, sorted
	std::vector<uint32_t> cov(n_pos * stride, 0), n_cov(rows.n_sel);
	for (uint64_t x = 0; x < n_pos; x++)
		for (uint32_t k = 0; k < n_cov[x]; k++) cov[x * stride + k] = rows.cluster[out.pc_ptr[x] + rows.sel[x * stride + k]];
	const std::vector<uint32_t> n_orig(n_cov);
	pt_fill_gaps(n_pos, stride, p.view->max_cluster_gap, p.view->n_clusters, cov, n_cov);
	pt_sorted_lists(n_pos, stride, cov, n_cov, n_orig, out.cov);
	// the side effect: an appended cluster's depth row is emptied
	for (uint64_t x = 0; x < n_pos; x++) {
		s.n_selected += n_orig[x];
		for (uint64_t k = out.cov.ptr[x]; k < out.cov.ptr[x + 1]; k++) {
			if (!out.cov.readded[k]) continue;
			++s.n_readded;
			const uint32_t* b = out.cluster.data() + out.pc_ptr[x];
			const uint32_t* e = out.cluster.data() + out.pc_ptr[x + 1];
			const uint32_t* at = std::lower_bound(b, e, out.cov.cluster[k]);
			if (at == e || *at != out.cov.cluster[k]) continue;
			std::fill_n(out.depth.begin() + (uint64_t)(at - out.cluster.data()) * na, na, 0u);
			++s.n_emptied;
		}
	}
}

whamd_status_t thread_inputs(const whamd_poly_thread_view* views, uint64_t n, int device, bool host, whamd_poly_thread_result** out) {
	BatchClock clock;
	const whamd_status_t st = run_batch<ThreadProblem, ThreadRows>(
		views, n, host, out, polythread_prepare,
		[](auto& problems, auto& rows) {
			for (size_t x = 0; x < problems.size(); x++) polythread_host(problems[x], rows[x]);
		},
		[&](auto& problems, auto& rows, CallTimes& times, std::string& msg) { return polythread_device(problems, device, rows, times, msg); },
		[](const ThreadProblem& p, ThreadRows& rows, whamd_poly_thread_result::Problem& o) {
			if (rows.npc.empty()) {   // (nothing of the call touched the device: no rows anywhere)
				rows.npc.assign(p.m.n_positions, 0);
				rows.n_sel.assign(p.m.n_positions, 0);
				rows.na = 4;
			}
			assemble(p, rows, o);
		},
		&clock);
	if (st != WHAMD_OK) return st;
	for (auto& p : (*out)->problems) p.stats.fill_ms = clock.t3 - clock.t2;
	return WHAMD_OK;
}

whamd_status_t select_clusters(uint64_t n_pos, const uint64_t* pc_ptr, const uint32_t* pc_cluster, const uint32_t* pc_total, uint32_t ploidy, uint32_t max_gap,
                               int device, bool host, uint64_t* cov_ptr_out, uint32_t* cluster_out, uint8_t* readded_out, uint32_t* rank_out, uint32_t* launches_out) {
	std::string msg;
	if (launches_out) *launches_out = 0;
	if (!ploidy_ok(ploidy, msg)) return fail(WHAMD_ERR_INVALID, msg);
	if (!pc_ptr || !cov_ptr_out) return fail(WHAMD_ERR_INVALID, "null argument");
	if (n_pos >= 0xfffff000ull) return fail(WHAMD_ERR_UNSUPPORTED, "2^32 - 4096 or more positions");
	if (pc_ptr[0] != 0) return fail(WHAMD_ERR_INVALID, not_from_zero("pc_ptr"));
	for (uint64_t x = 0; x < n_pos; x++)   // (strict: not check_offsets)
		if (pc_ptr[x] >= pc_ptr[x + 1]) return fail(WHAMD_ERR_INVALID, "position " + std::to_string(x) + " lists no cluster");
	const uint64_t n_rows = pc_ptr[n_pos];
	if (n_rows >= 0xfffff000ull) return fail(WHAMD_ERR_UNSUPPORTED, "2^32 - 4096 or more rows");
	if (n_rows && (!pc_cluster || !pc_total || !cluster_out || !readded_out || !rank_out)) return fail(WHAMD_ERR_INVALID, "null argument");
	std::vector<uint32_t> ids(pc_cluster, pc_cluster + n_rows), one;
	std::sort(ids.begin(), ids.end());
	ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
	std::vector<uint32_t> begin(n_pos), count(n_pos), total(pc_total, pc_total + n_rows);
	for (uint64_t x = 0; x < n_pos; x++) {
		begin[x] = (uint32_t)pc_ptr[x];
		count[x] = (uint32_t)(pc_ptr[x + 1] - pc_ptr[x]);
		one.assign(pc_cluster + pc_ptr[x], pc_cluster + pc_ptr[x + 1]);
		std::sort(one.begin(), one.end());
		if (std::adjacent_find(one.begin(), one.end()) != one.end()) return fail(WHAMD_ERR_INVALID, "position " + std::to_string(x) + " lists a cluster twice");
		uint64_t all = 0;
		for (uint64_t k = pc_ptr[x]; k < pc_ptr[x + 1]; k++) all += pc_total[k];
		if (all > 0xffffffffull) return fail(WHAMD_ERR_INVALID, "position " + std::to_string(x) + ": the depths sum beyond uint32");
		if (!all && count[x] > 1) return fail(WHAMD_ERR_INVALID, "position " + std::to_string(x) + ": several clusters of total depth 0 (division by zero)");
	}
	std::vector<uint32_t> n_sel, sel;
	CallTimes times;
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		select_host(begin, count, total, ploidy, n_sel, sel);
#endif
	} else {
		const whamd_status_t st = polythread_select_device(begin, count, total, ploidy, device, n_sel, sel, times, msg);
		if (st != WHAMD_OK) return fail(st, msg);
	}
	if (launches_out) *launches_out = times.launches;
	const uint32_t stride = ploidy + 2;
	std::vector<uint32_t> cov(n_pos * stride, 0), n_cov(n_sel);
	for (uint64_t x = 0; x < n_pos; x++)
		for (uint32_t k = 0; k < n_cov[x]; k++)
			cov[x * stride + k] = (uint32_t)(std::lower_bound(ids.begin(), ids.end(), pc_cluster[pc_ptr[x] + sel[x * stride + k]]) - ids.begin());
	const std::vector<uint32_t> n_orig(n_cov);
	pt_fill_gaps(n_pos, stride, max_gap, ids.size(), cov, n_cov);
	CovLists lists;
	pt_sorted_lists(n_pos, stride, cov, n_cov, n_orig, lists);   // (dense ids ascend with the caller's)
	std::memcpy(cov_ptr_out, lists.ptr.data(), (n_pos + 1) * sizeof(uint64_t));
	for (uint64_t k = 0; k < lists.cluster.size(); k++) {
		cluster_out[k] = ids[lists.cluster[k]];
		readded_out[k] = lists.readded[k];
		rank_out[k] = lists.rank[k];
	}
	return WHAMD_OK;
}

whamd_status_t haplotypes(const uint32_t* paths, uint64_t n_pos, uint32_t ploidy, const uint64_t* pc_ptr, const uint32_t* pc_cluster, const int8_t* pc_cons, int device,
                          bool host, int8_t* out, uint32_t* launches_out) {
	std::string msg;
	if (launches_out) *launches_out = 0;
	if (!ploidy_ok(ploidy, msg)) return fail(WHAMD_ERR_INVALID, msg);
	if (!n_pos) return WHAMD_OK;
	if (!paths || !pc_ptr || !out) return fail(WHAMD_ERR_INVALID, "null argument");
	if (n_pos >= 0xfffff000ull) return fail(WHAMD_ERR_UNSUPPORTED, "2^32 - 4096 or more positions");
	if (!check_offsets(pc_ptr, n_pos, "pc_ptr", "position", msg)) return fail(WHAMD_ERR_INVALID, msg);
	if (pc_ptr[n_pos] >= 0xfffff000ull / ploidy) return fail(WHAMD_ERR_UNSUPPORTED, "too many rows for uint32 offsets");
	if (pc_ptr[n_pos] && (!pc_cluster || !pc_cons)) return fail(WHAMD_ERR_INVALID, "null argument");
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		for (uint64_t x = 0; x < n_pos; x++)
			pt_haplotype_position(paths + x * ploidy, ploidy, pc_cluster + pc_ptr[x], pc_cons + pc_ptr[x] * ploidy, (uint32_t)(pc_ptr[x + 1] - pc_ptr[x]), out + x, n_pos);
#endif
		return WHAMD_OK;
	}
	std::vector<int8_t> got;
	CallTimes times;
	const whamd_status_t st = polythread_haplotypes_device(paths, n_pos, ploidy, pc_ptr, pc_cluster, pc_cons, device, got, times, msg);
	if (st != WHAMD_OK) return fail(st, msg);
	if (launches_out) *launches_out = times.launches;
	std::memcpy(out, got.data(), got.size());
	return WHAMD_OK;
}

}  // namespace

extern "C" {

whamd_status_t whamd_poly_thread_inputs(const whamd_poly_thread_view* problems, uint64_t n_problems, int device, whamd_poly_thread_result** out) {
	return guarded([&]() -> whamd_status_t { return thread_inputs(problems, n_problems, device, false, out); });
}

uint64_t whamd_poly_thread_problem_count(const whamd_poly_thread_result* r) { return r ? r->problems.size() : 0; }

uint64_t whamd_poly_thread_position_count(const whamd_poly_thread_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->pc_ptr.size() - 1 : 0;
}

uint64_t whamd_poly_thread_row_count(const whamd_poly_thread_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->cluster.size() : 0;
}

uint64_t whamd_poly_thread_cov_count(const whamd_poly_thread_result* r, uint64_t m) {
	const auto* p = problem_of(r, m);
	return p ? p->cov.cluster.size() : 0;
}

whamd_status_t whamd_poly_thread_get_rows(const whamd_poly_thread_result* r, uint64_t m, uint64_t* pc_ptr_out, uint32_t* cluster_out, uint32_t* depth_out,
                                          uint32_t* first_out, int8_t* consensus_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(pc_ptr_out, p->pc_ptr);
	copy_out(cluster_out, p->cluster);
	copy_out(depth_out, p->depth);
	copy_out(first_out, p->first);
	copy_out(consensus_out, p->cons);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_thread_get_cov(const whamd_poly_thread_result* r, uint64_t m, uint64_t* cov_ptr_out, uint32_t* cluster_out, uint8_t* readded_out,
                                         uint32_t* rank_out) {
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	copy_out(cov_ptr_out, p->cov.ptr);
	copy_out(cluster_out, p->cov.cluster);
	copy_out(readded_out, p->cov.readded);
	copy_out(rank_out, p->cov.rank);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_thread_get_stats(const whamd_poly_thread_result* r, uint64_t m, whamd_poly_thread_stats* stats_out) {
	return get_stats_of(r, m, stats_out);
}

void whamd_poly_thread_destroy(whamd_poly_thread_result* r) { delete r; }

whamd_status_t whamd_poly_select_clusters(uint64_t n_pos, const uint64_t* pc_ptr, const uint32_t* pc_cluster, const uint32_t* pc_total, uint32_t ploidy,
                                          uint32_t max_cluster_gap, int device, uint64_t* cov_ptr_out, uint32_t* cluster_out, uint8_t* readded_out,
                                          uint32_t* rank_out, uint32_t* launches_out) {
	return guarded([&]() -> whamd_status_t {
		return select_clusters(n_pos, pc_ptr, pc_cluster, pc_total, ploidy, max_cluster_gap, device, false, cov_ptr_out, cluster_out, readded_out, rank_out, launches_out);
	});
}

whamd_status_t whamd_poly_haplotypes(const uint32_t* paths, uint64_t n_pos, uint32_t ploidy, const uint64_t* pc_ptr, const uint32_t* pc_cluster,
                                     const int8_t* pc_consensus, int device, int8_t* haplotypes_out, uint32_t* launches_out) {
	return guarded([&]() -> whamd_status_t { return haplotypes(paths, n_pos, ploidy, pc_ptr, pc_cluster, pc_consensus, device, false, haplotypes_out, launches_out); });
}

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_poly_thread_inputs_host(const whamd_poly_thread_view* problems, uint64_t n_problems, whamd_poly_thread_result** out) {
	return guarded([&]() -> whamd_status_t { return thread_inputs(problems, n_problems, 0, true, out); });
}

whamd_status_t whamd_debug_poly_select_clusters_host(uint64_t n_pos, const uint64_t* pc_ptr, const uint32_t* pc_cluster, const uint32_t* pc_total, uint32_t ploidy,
                                                     uint32_t max_cluster_gap, uint64_t* cov_ptr_out, uint32_t* cluster_out, uint8_t* readded_out, uint32_t* rank_out) {
	return guarded([&]() -> whamd_status_t {
		return select_clusters(n_pos, pc_ptr, pc_cluster, pc_total, ploidy, max_cluster_gap, 0, true, cov_ptr_out, cluster_out, readded_out, rank_out, nullptr);
	});
}

whamd_status_t whamd_debug_poly_haplotypes_host(const uint32_t* paths, uint64_t n_pos, uint32_t ploidy, const uint64_t* pc_ptr, const uint32_t* pc_cluster,
                                                const int8_t* pc_consensus, int8_t* haplotypes_out) {
	return guarded([&]() -> whamd_status_t { return haplotypes(paths, n_pos, ploidy, pc_ptr, pc_cluster, pc_consensus, 0, true, haplotypes_out, nullptr); });
}
#endif

}  // extern "C"
