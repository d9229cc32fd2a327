// polythread.h -- what lies on both sides of the threader in `whatshap polyphase` (whatshap/polyphase/threading.py): get_allele_depths
// (:274-317), select_clusters (:228-271) and compute_haplotypes (:112-131), restated from their behaviour.  Per (position, cluster) with
// at least one read of the cluster at the position: the depth of every allele, the consensus list of `ploidy` picks, and per position the
// clusters the threader may use.
//
// The matrix rows arrive read-major, the depths are per position: the transposition runs on the device (polythread_device.hip) as count,
// scan, place (run_scatter.h), then one team per position reduces its run cluster by cluster in ascending cluster id.  What is kept per
// (position, cluster, allele) is a count and the smallest rank, in the cluster's list, of a read with that allele: both are independent
// of the order inside a run, and the rank restates the reference's dict insertion order.  The functions below (consensus, selection, one
// position of compute_haplotypes) are shared by the kernels and by the host twin of the debug library.  The sequential gap filling of
// select_clusters runs on the host after the download (polythread.cpp, pt_fill_gaps).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "host_parallel.h"
#include "polyscore.h"
#include "run_scatter.h"

#if defined(__HIPCC__)
#define WHAMD_HD __host__ __device__
#else
#define WHAMD_HD
#endif

namespace whamd {

constexpr uint32_t PT_MAX_PLOIDY = WHAMD_POLY_THREAD_MAX_PLOIDY;
constexpr uint32_t PT_MAX_ALLELES = WHAMD_POLY_THREAD_MAX_ALLELES;
constexpr uint32_t PT_SEGMENT = RS_SEGMENT;       // lanes per position in class a
constexpr uint32_t PT_CLASS_A_MAX = 64;           // class a: 0 .. 64 placed entries
constexpr uint32_t PT_CLASS_B_MAX = 4096;         // class b: 65 .. 4096 (one wave); class c beyond (one workgroup, any length)
constexpr uint32_t PT_LAUNCHES = WHAMD_POLY_THREAD_LAUNCHES;   // count, scan (2), place, clusters a / b / c, scan (2), rows a / b / c, select
constexpr uint32_t PT_NONE = RS_NONE;
constexpr uint32_t PT_MAX_RANK = 1u << 28;        // reads per cluster (the rank shares a word with the allele)

struct PtRead {
	uint32_t cluster;   // PT_NONE: the read is in no cluster
	uint32_t rank;      // its place in the cluster's list
	uint32_t pos_base;  // first position of the read's problem in the call
};
struct PtPlaced {
	uint32_t cluster;
	uint32_t rank_allele;   // rank << 4 | allele
};

// The consensus list of one (position, cluster): `ploidy` picks, each the allele with the largest depth / (1 + times picked), a double
// division as in Python; equal quotients go to the allele a read of the cluster's list showed first (the reference walks a dict in
// insertion order and replaces its maximum on `>` only).  Alleles of depth 0 are not in that dict.
template <int NA>
WHAMD_HD inline void pt_consensus(const uint32_t (&cnt)[NA], const uint32_t (&first)[NA], uint32_t ploidy, int8_t* out) {
	uint32_t picked[NA];
#pragma unroll
	for (int a = 0; a < NA; a++) picked[a] = 0;
	for (uint32_t i = 0; i < ploidy; i++) {
		double best_q = 0.0;
		uint32_t best_first = PT_NONE;
		int best = 0;
#pragma unroll
		for (int a = 0; a < NA; a++) {
			const double q = cnt[a] ? (double)cnt[a] / (double)(1u + picked[a]) : 0.0;
			if (q > best_q || (q == best_q && cnt[a] && first[a] < best_first)) {
				best_q = q;
				best_first = first[a];
				best = a;
			}
		}
		out[i] = (int8_t)best;
#pragma unroll
		for (int a = 0; a < NA; a++) picked[a] += a == best ? 1u : 0u;
	}
}

// The selection of one position among its n clusters of total depth total[k]: descending depth, equal depths in listed order; the first
// always, then up to min(n, ploidy + 2) in all while depth / sum of all < 1.0 / (8.0 * ploidy) is false (doubles; both operands below
// 2^32, so exact before the division).  Writes the chosen k in that order, returns how many.
WHAMD_HD inline uint32_t pt_select(const uint32_t* total, uint32_t n, uint32_t ploidy, uint32_t* chosen) {
	if (!n) return 0;
	uint64_t all = 0;
	for (uint32_t k = 0; k < n; k++) all += total[k];
	const uint32_t cut = n < ploidy + 2 ? n : ploidy + 2;
	const double threshold = 1.0 / (8.0 * (double)ploidy);
	uint32_t prev_t = 0, prev_k = 0, m = 0;
	for (uint32_t s = 0; s < cut; s++) {
		uint32_t bt = 0, bk = PT_NONE;
		for (uint32_t k = 0; k < n; k++) {
			const uint32_t t = total[k];
			const bool after = s == 0 || t < prev_t || (t == prev_t && k > prev_k);
			if (after && (bk == PT_NONE || t > bt)) {
				bt = t;
				bk = k;
			}
		}
		if (bk == PT_NONE) break;
		if (s && (double)bt / (double)all < threshold) break;
		chosen[m++] = bk;
		prev_t = bt;
		prev_k = bk;
	}
	return m;
}

// compute_haplotypes at one position: slot i takes pick number (earlier slots of the same cluster) of that cluster's consensus list, -1
// where the cluster has no list at the position.  cluster / cons: the position's rows.
WHAMD_HD inline void pt_haplotype_position(const uint32_t* path, uint32_t ploidy, const uint32_t* cluster, const int8_t* cons, uint32_t n_rows, int8_t* out,
                                           uint64_t out_stride) {
	for (uint32_t i = 0; i < ploidy; i++) {
		const uint32_t cid = path[i];
		uint32_t k = 0;
		for (uint32_t j = 0; j < i; j++) k += path[j] == cid ? 1u : 0u;
		int8_t allele = -1;
		for (uint32_t row = 0; row < n_rows; row++)
			if (cluster[row] == cid) {
				allele = cons[(uint64_t)row * ploidy + k];
				break;
			}
		out[(uint64_t)i * out_stride] = allele;
	}
}

// One validated problem.
struct ThreadProblem {
	const whamd_poly_thread_view* view = nullptr;
	PolyMatrix m;                           // rows by local position (poly_build_matrix)
	uint32_t ploidy = 0, n_alleles = 0;
	uint64_t n_counted = 0;                 // row entries of reads that are in a cluster
	std::vector<PtRead> reads;              // per read: cluster, rank (pos_base 0)
	bool depths_only = false;
};

// Per problem, what the device (or the host twin) leaves before the gap filling.
struct ThreadRows {
	std::vector<uint32_t> npc;              // [n_pos] rows per position
	std::vector<uint32_t> cluster, total;   // per row
	uint32_t na = 4;                        // alleles per row here: 4 or 16 (the instantiation that made them)
	std::vector<uint32_t> depth, first;     // per row [na]
	std::vector<int8_t> cons;               // per row [ploidy]
	std::vector<uint32_t> n_sel, sel;       // per position: how many chosen, [n_pos * (ploidy + 2)] the chosen rows of the position, in order
	uint32_t class_a = 0, class_b = 0, class_c = 0;
};

whamd_status_t polythread_prepare(const whamd_poly_thread_view& v, ThreadProblem& p, std::string& msg);

// All problems of a call: one upload, PT_LAUNCHES launches whatever the problems.  No counted entry in the whole call: nothing touches
// the device (launches = 0).
whamd_status_t polythread_device(const std::vector<ThreadProblem>& ps, int device, std::vector<ThreadRows>& out, CallTimes& times, std::string& msg);

// The selection alone over a (position, cluster, depth) CSR: one launch.  begin / count: per position its rows in total[]; sel as in ThreadRows with
// a stride of ploidy + 2.
whamd_status_t polythread_select_device(const std::vector<uint32_t>& begin, const std::vector<uint32_t>& count, const std::vector<uint32_t>& total, uint32_t ploidy,
                                        int device, std::vector<uint32_t>& n_sel, std::vector<uint32_t>& sel, CallTimes& times, std::string& msg);

// compute_haplotypes over arrays: one launch.  out: [ploidy][n_pos].
whamd_status_t polythread_haplotypes_device(const uint32_t* paths, uint64_t n_pos, uint32_t ploidy, const uint64_t* pc_ptr, const uint32_t* pc_cluster,
                                            const int8_t* pc_cons, int device, std::vector<int8_t>& out, CallTimes& times, std::string& msg);

}  // namespace whamd
