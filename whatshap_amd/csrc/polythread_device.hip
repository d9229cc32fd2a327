// polythread_device.hip -- allele depths, consensus lists and the cluster selection of polyphase threading on gfx950 (polythread.h).
// The matrix rows arrive read-major, the depths are per position: count, scan and place are the shared ones of run_scatter.h with the
// key "position of the call" (the problem's first position plus the local one):
//   upload    per read {cluster, rank in the cluster's list, first position of its problem} and its first row entry, the row entries
//             (local position, allele), per position the ploidy of its problem.
//   count     one thread per row entry: its read (read_of_entry, run_teams.h); a read in no cluster is not counted (RS_NONE).
//   scan      exclusive, two launches; also appends the positions of more than 64 / 4096 entries to the class b / c list.
//   place     a counted entry goes to its position's run as {cluster, rank << 4 | allele}.  The order inside a run is whatever the
//             atomics give; nothing below depends on it.
//   clusters  one team per position -- class a eight lanes over all positions, class b one wave, class c one workgroup (any length),
//             both walking their list with a fixed grid -- counts the distinct clusters of the run: walk_ids of run_teams.h (scopes
//             and walk are shared with haplotagging and haplotagphase) with an empty body.
//   scan      of those counts: where every position's rows begin, and how many there are (the one wait of the call, to size the rows).
//   rows      the same teams, the same walk; its body is a second pass for the depth of every allele and the smallest rank of a read
//             with it (RowAcc; sums and minima: no order), and the team's first lane writes the row and its consensus list (pt_consensus).
//   select    one thread per position: pt_select over the totals of its rows.
// 13 launches per call whatever the problems (PT_LAUNCHES).  The rows keep NA = 4 or 16 alleles, by the largest n_alleles of the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_runtime.h"
#include "polythread.h"
#include "run_teams.h"

namespace whamd {
namespace {

constexpr int NW = RT_WAVES;

struct PtArgs {
	// the image
	const PtRead* reads;          // [n_reads]
	const uint32_t* read_ptr;     // [n_reads + 1]
	const uint32_t* row_pos;      // [n_entries] local to the read's problem
	const uint8_t* row_allele;
	const uint32_t* pos_ploidy;   // [n_keys]
	// made on the device
	RunIndex run;                 // keys: the positions of the call; counted: the entries of reads that are in a cluster
	PtPlaced* placed;             // [n_placed]
	uint32_t* npc;                // [n_keys] rows (distinct clusters) per position
	uint32_t* npc_local;
	uint32_t* npc_tile_sums;
	uint32_t* n_rows;             // [1]
	uint32_t* pc_cluster;         // [n_pc]
	uint32_t* pc_total;
	uint32_t* pc_depth;           // [n_pc][NA]
	uint32_t* pc_first;
	int8_t* pc_cons;              // [n_pc][max_ploidy]
	uint32_t* n_sel;              // [n_keys]
	uint32_t* sel;                // [n_keys][max_ploidy + 2]
	uint32_t n_reads, n_entries, n_pc, max_ploidy;
};

// ---------------------------------------------------------------------------------------------- count, place
// Row entry i of the call: the position it is counted at (PT_NONE: its read is in no cluster) and what is placed for it.
__device__ inline uint32_t counted_position(const PtArgs& a, uint32_t i, PtPlaced& what) {
	what = PtPlaced{0, 0};
	if (i >= a.n_entries) return PT_NONE;
	const PtRead rd = a.reads[read_of_entry(a.read_ptr, a.n_reads, a.n_entries, i)];
	if (rd.cluster == PT_NONE) return PT_NONE;
	const uint32_t v = rd.pos_base + a.row_pos[i];
	if (v >= a.run.n_keys) return PT_NONE;
	what = PtPlaced{rd.cluster, rd.rank << 4 | (uint32_t)(a.row_allele[i] & 15u)};
	return v;
}

__global__ void __launch_bounds__(RS_BLOCK) polythread_count_kernel(PtArgs a) {
	const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
	PtPlaced what;
	scatter_count(a.run, counted_position(a, i, what), threadIdx.x & 63u);
}

__global__ void __launch_bounds__(RS_BLOCK) polythread_place_kernel(PtArgs a) {
	const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
	PtPlaced what;
	const uint32_t at = scatter_place(a.run, counted_position(a, i, what), threadIdx.x & 63u);
	if (at != RS_NONE) a.placed[at] = what;
}

// ---------------------------------------------------------------------------------------------- a run, cluster by cluster
// One cluster of a run: per allele the depth and the smallest rank of a read with it.
template <int NA>
struct RowAcc {
	uint32_t cnt[NA], first[NA];
	template <int W>
	__device__ void across() {
#pragma unroll
		for (int x = 0; x < NA; x++) {
			cnt[x] = team_sum<W>(cnt[x]);
			first[x] = team_min<W>(first[x]);
		}
	}
	__device__ void merge(const RowAcc& o) {
#pragma unroll
		for (int x = 0; x < NA; x++) {
			cnt[x] += o.cnt[x];
			first[x] = min(first[x], o.first[x]);
		}
	}
};

// The clusters of run[0, n) in ascending order (walk_ids), for the owners with `need`.  Returns how many there are.  ROWS: per cluster a
// second pass for its depths; the owner's `leader` lane writes one row per cluster from row0 on, at most max_rows and none at or beyond
// a.n_pc.
template <int NA, bool ROWS, class Scope>
__device__ inline uint32_t per_cluster(const PtArgs& a, const PtPlaced* run, uint32_t n, uint32_t l, bool need, const Scope& scope, uint32_t row0, uint32_t max_rows,
                                       uint32_t ploidy, bool leader) {
	const auto cluster_of = [&](uint32_t i) { return run[i].cluster; };
	if constexpr (!ROWS) return walk_ids(scope, n, l, need, cluster_of, [](uint32_t, bool, uint32_t) {});
	else return walk_ids(scope, n, l, need, cluster_of, [&](uint32_t next, bool active, uint32_t ordinal) {
		RowAcc<NA> acc;
#pragma unroll
		for (int x = 0; x < NA; x++) {
			acc.cnt[x] = 0;
			acc.first[x] = PT_NONE;
		}
		team_pass<Scope>(n, l, active, [&](uint32_t i) {
			const PtPlaced e = run[i];
			const uint32_t allele = e.rank_allele & 15u, rank = e.rank_allele >> 4;
#pragma unroll
			for (int x = 0; x < NA; x++) {
				const bool hit = e.cluster == next && allele == (uint32_t)x;
				acc.cnt[x] += hit ? 1u : 0u;
				acc.first[x] = hit ? min(acc.first[x], rank) : acc.first[x];
			}
		});
		scope.combine(acc);
		const uint64_t row = (uint64_t)row0 + ordinal;
		if (active && leader && ordinal < max_rows && row < a.n_pc) {
			uint32_t total = 0;
#pragma unroll
			for (int x = 0; x < NA; x++) {
				total += acc.cnt[x];
				a.pc_depth[row * NA + x] = acc.cnt[x];
				a.pc_first[row * NA + x] = acc.first[x];
			}
			a.pc_cluster[row] = next;
			a.pc_total[row] = total;
			pt_consensus<NA>(acc.cnt, acc.first, ploidy, a.pc_cons + row * a.max_ploidy);
		}
	});
}

__device__ inline uint32_t row_begin(const PtArgs& a, uint32_t v) { return run_begin(a.npc_local, a.npc_tile_sums, v); }

// One owner, one position: count its clusters (ROWS false) or write its rows.
template <int NA, bool ROWS, class Scope>
__device__ inline void position_by(const PtArgs& a, uint32_t v, bool have, uint32_t l, const Scope& scope, bool leader) {
	const uint32_t n = have ? a.run.counts[v] : 0;
	const PtPlaced* run = a.placed + (have ? run_begin(a.run.local, a.run.tile_sums, v) : 0);
	const uint32_t row0 = ROWS && have ? row_begin(a, v) : 0, max_rows = ROWS && have ? a.npc[v] : 0, ploidy = have ? a.pos_ploidy[v] : 1;
	const uint32_t n_rows = per_cluster<NA, ROWS>(a, run, n, l, have, scope, row0, max_rows, ploidy, leader);
	if (!ROWS && have && leader) a.npc[v] = n_rows;
}

// Class a: eight lanes per position, over all positions; those of more entries are left to the lists.
template <int NA, bool ROWS>
__global__ void __launch_bounds__(RS_BLOCK) polythread_a_kernel(PtArgs a) {
	const SegmentKey k = segment_key(a.run);
	position_by<NA, ROWS>(a, k.v, k.have, k.l, TeamScope<(int)PT_SEGMENT>{}, k.l == 0);
}

// Class b: one wave per listed position.
template <int NA, bool ROWS>
__global__ void __launch_bounds__(RS_BLOCK) polythread_b_kernel(PtArgs a) {
	const uint32_t lane = threadIdx.x & 63u, n_list = a.run.list_n[0];
	for (uint32_t k = blockIdx.x * NW + (threadIdx.x >> 6); k < n_list; k += gridDim.x * NW)
		position_by<NA, ROWS>(a, a.run.list_b[k], true, lane, TeamScope<64>{}, lane == 0);
}

// Class c: one workgroup per listed position, a run of any length.
template <int NA, bool ROWS>
__global__ void __launch_bounds__(RS_BLOCK) polythread_c_kernel(PtArgs a) {
	__shared__ uint32_t word[NW];
	__shared__ RowAcc<NA> part[NW];
	const uint32_t n_list = a.run.list_n[1];
	const BlockScope<RowAcc<NA>> scope{word, part, threadIdx.x & 63u, threadIdx.x >> 6};
	for (uint32_t k = blockIdx.x; k < n_list; k += gridDim.x) position_by<NA, ROWS>(a, a.run.list_c[k], true, threadIdx.x, scope, threadIdx.x == 0);
}

// ---------------------------------------------------------------------------------------------- selection, haplotypes
struct PtSelectArgs {
	const uint32_t* total;        // per row
	const uint32_t* begin;        // [n_keys] first row of the position; nullptr: run_begin(begin_local, begin_tile_sums)
	const uint32_t* begin_local;
	const uint32_t* begin_tile_sums;
	const uint32_t* count;        // [n_keys] rows of the position
	const uint32_t* pos_ploidy;   // [n_keys]; nullptr: `ploidy` for all
	uint32_t* n_sel;              // [n_keys]
	uint32_t* sel;                // [n_keys][stride]
	uint32_t n_keys, n_total, ploidy, stride;
};

__global__ void __launch_bounds__(RS_BLOCK) polythread_select_kernel(PtSelectArgs a) {
	const uint64_t v = (uint64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
	if (v >= a.n_keys) return;
	const uint32_t begin = a.begin ? a.begin[v] : run_begin(a.begin_local, a.begin_tile_sums, (uint32_t)v);
	uint32_t n = a.count[v];
	if (begin > a.n_total || n > a.n_total - begin) n = 0;   // (never: the rows were sized by the same counts)
	const uint32_t ploidy = a.pos_ploidy ? a.pos_ploidy[v] : a.ploidy;
	a.n_sel[v] = ploidy + 2 <= a.stride ? pt_select(a.total + begin, n, ploidy, a.sel + v * a.stride) : 0;
}

struct PtHaplotypeArgs {
	const uint32_t* paths;        // [n_pos][ploidy]
	const uint32_t* row_begin;    // [n_pos + 1]
	const uint32_t* cluster;      // per row
	const int8_t* cons;           // [rows][ploidy]
	int8_t* out;                  // [ploidy][n_pos]
	uint32_t n_pos, ploidy;
};

__global__ void __launch_bounds__(RS_BLOCK) polythread_haplotypes_kernel(PtHaplotypeArgs a) {
	const uint64_t x = (uint64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
	if (x >= a.n_pos) return;
	const uint32_t b = a.row_begin[x], e = a.row_begin[x + 1];
	pt_haplotype_position(a.paths + x * a.ploidy, a.ploidy, a.cluster + b, a.cons + (uint64_t)b * a.ploidy, e - b, a.out + x, a.n_pos);
}

template <int NA>
whamd_status_t launch_clusters_and_rows(Session& s, CallTimes& times, std::string& msg, const PtArgs& a, bool rows, dim3 per_segment) {
	if (rows) {
		WHAMD_TRY(rs_launch(s, times, msg, polythread_a_kernel<NA, true>, per_segment, a));
		WHAMD_TRY(rs_launch(s, times, msg, polythread_b_kernel<NA, true>, dim3(RS_LIST_GRID), a));
		return rs_launch(s, times, msg, polythread_c_kernel<NA, true>, dim3(RS_LIST_GRID), a);
	}
	WHAMD_TRY(rs_launch(s, times, msg, polythread_a_kernel<NA, false>, per_segment, a));
	WHAMD_TRY(rs_launch(s, times, msg, polythread_b_kernel<NA, false>, dim3(RS_LIST_GRID), a));
	return rs_launch(s, times, msg, polythread_c_kernel<NA, false>, dim3(RS_LIST_GRID), a);
}

}  // namespace

whamd_status_t polythread_device(const std::vector<ThreadProblem>& ps, int device, std::vector<ThreadRows>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(ps.size(), ThreadRows{});
	std::vector<uint64_t> pos_base(ps.size() + 1, 0), read_base(ps.size() + 1, 0), ent_base(ps.size() + 1, 0);
	uint64_t n_placed = 0;
	uint32_t max_ploidy = 1, max_alleles = 1;
	for (size_t x = 0; x < ps.size(); x++) {
		pos_base[x + 1] = pos_base[x] + ps[x].m.n_positions;
		read_base[x + 1] = read_base[x] + ps[x].m.n_reads;
		ent_base[x + 1] = ent_base[x] + ps[x].m.row_pos.size();
		n_placed += ps[x].n_counted;
		max_ploidy = std::max(max_ploidy, ps[x].ploidy);
		max_alleles = std::max(max_alleles, ps[x].n_alleles);
	}
	const uint64_t n_keys = pos_base[ps.size()], n_reads = read_base[ps.size()], n_entries = ent_base[ps.size()];
	if (!n_placed) return WHAMD_OK;   // nothing is counted: no device work at all
	if (n_keys >= 0xfffff000ull || n_entries >= 0xfffff000ull || n_keys * (max_ploidy + 2) >= 0xfffff000ull) {   // (indices are uint32 with room to round grids up)
		msg = "2^32 - 4096 or more positions, row entries or list slots in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	const uint32_t na = max_alleles <= 4 ? 4 : 16, sel_stride = max_ploidy + 2;
	ImageLayout in;
	const auto p_reads = in.add<PtRead>(n_reads);
	const auto p_rptr = in.add<uint32_t>(n_reads + 1);
	const auto p_rpos = in.add<uint32_t>(n_entries);
	const auto p_ploidy = in.add<uint32_t>(n_keys);
	const auto p_rallele = in.add<uint8_t>(n_entries);
	// what the kernels make: the zeroed words first
	ImageLayout work;
	RunPieces w_run;
	rs_add_zeroed(work, n_keys, w_run);
	const auto w_n_rows = work.add<uint32_t>(1);
	const auto w_npc = work.add<uint32_t>(n_keys);
	const size_t zeroed = work.total;
	rs_add_rest(work, n_keys, w_run);
	const auto w_npc_local = work.add<uint32_t>(n_keys);
	const auto w_npc_tiles = work.add<uint32_t>(rs_tiles(n_keys));
	const auto w_placed = work.add<PtPlaced>(n_placed);
	const auto w_n_sel = work.add<uint32_t>(n_keys);
	const auto w_sel = work.add<uint32_t>(n_keys * sel_stride);
	ImageLayout results;   // what comes back, beside the rows
	const auto r_counts = results.add<uint32_t>(n_keys);
	const auto r_npc = results.add<uint32_t>(n_keys);
	const auto r_n_sel = results.add<uint32_t>(n_keys);
	const auto r_sel = results.add<uint32_t>(n_keys * sel_stride);
	const auto r_n_rows = results.add<uint32_t>(1);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, wk, res, rw;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.work(work, wk, msg));
	WHAMD_TRY(s.results(results, res, msg));
	// the image
	for (size_t x = 0; x < ps.size(); x++) {
		const ThreadProblem& p = ps[x];
		PtRead* reads = im.host(p_reads) + read_base[x];
		uint32_t* rptr = im.host(p_rptr) + read_base[x];
		for (uint64_t r = 0; r < p.m.n_reads; r++) {
			reads[r] = PtRead{p.reads[r].cluster, p.reads[r].rank, (uint32_t)pos_base[x]};
			rptr[r] = (uint32_t)(ent_base[x] + p.m.row_ptr[r]);
		}
		std::fill_n(im.host(p_ploidy) + pos_base[x], p.m.n_positions, p.ploidy);
		const uint64_t n = p.m.row_pos.size();
		if (n) {
			std::memcpy(im.host(p_rpos) + ent_base[x], p.m.row_pos.data(), n * sizeof(uint32_t));
			std::memcpy(im.host(p_rallele) + ent_base[x], p.m.row_allele.data(), n);
		}
	}
	im.host(p_rptr)[n_reads] = (uint32_t)n_entries;
	WHAMD_TRY(s.upload(im, msg));
	WHAMD_TRY(s.zero(wk, zeroed, msg));
	PtArgs a{};
	a.reads = im.dev(p_reads);
	a.read_ptr = im.dev(p_rptr);
	a.row_pos = im.dev(p_rpos);
	a.row_allele = im.dev(p_rallele);
	a.pos_ploidy = im.dev(p_ploidy);
	a.run = rs_bind(wk, w_run, n_keys, n_placed, PT_CLASS_A_MAX, PT_CLASS_B_MAX);
	a.placed = wk.dev_out(w_placed);
	a.npc = wk.dev_out(w_npc);
	a.npc_local = wk.dev_out(w_npc_local);
	a.npc_tile_sums = wk.dev_out(w_npc_tiles);
	a.n_rows = wk.dev_out(w_n_rows);
	a.n_sel = wk.dev_out(w_n_sel);
	a.sel = wk.dev_out(w_sel);
	a.n_reads = (uint32_t)n_reads;
	a.n_entries = (uint32_t)n_entries;
	a.n_pc = 0;
	a.max_ploidy = max_ploidy;
	const RunIndex& run = a.run;
	const dim3 per_entry(grid_for(n_entries, RS_BLOCK)), per_segment(grid_for(n_keys, RS_BLOCK / PT_SEGMENT)), per_key(grid_for(n_keys, RS_BLOCK));
	WHAMD_TRY(rs_launch(s, times, msg, polythread_count_kernel, per_entry, a));
	WHAMD_TRY(rs_scan(s, times, msg, run.counts, run.local, run.tile_sums, run.n_keys, &run, nullptr));
	WHAMD_TRY(rs_launch(s, times, msg, polythread_place_kernel, per_entry, a));
	WHAMD_TRY(launch_clusters_and_rows<4>(s, times, msg, a, false, per_segment));
	WHAMD_TRY(rs_scan(s, times, msg, a.npc, a.npc_local, a.npc_tile_sums, run.n_keys, nullptr, a.n_rows));
	WHAMD_TRY(s.fetch_now(res, r_n_rows, a.n_rows, msg));   // the number of rows
	const uint64_t n_pc = *res.host(r_n_rows);
	if (!n_pc || n_pc > n_placed) {
		msg = "internal error: the rows and the counted entries disagree";
		return WHAMD_ERR_DEVICE;
	}
	a.n_pc = (uint32_t)n_pc;
	ImageLayout rows;
	const auto r_cluster = rows.add<uint32_t>(n_pc);
	const auto r_total = rows.add<uint32_t>(n_pc);
	const auto r_depth = rows.add<uint32_t>(n_pc * na);
	const auto r_first = rows.add<uint32_t>(n_pc * na);
	const auto r_cons = rows.add<int8_t>(n_pc * max_ploidy);
	WHAMD_TRY(s.stage(rows, rw, msg));   // the second result image: sized by the wait, written by the kernels, fetched whole
	a.pc_cluster = rw.dev_out(r_cluster);
	a.pc_total = rw.dev_out(r_total);
	a.pc_depth = rw.dev_out(r_depth);
	a.pc_first = rw.dev_out(r_first);
	a.pc_cons = rw.dev_out(r_cons);
	HIP_TRY(hipMemsetAsync(a.pc_cons, 0, n_pc * max_ploidy, s.stream));
	if (na == 4) WHAMD_TRY(launch_clusters_and_rows<4>(s, times, msg, a, true, per_segment));
	else WHAMD_TRY(launch_clusters_and_rows<16>(s, times, msg, a, true, per_segment));
	PtSelectArgs sa{};
	sa.total = a.pc_total;
	sa.begin = nullptr;
	sa.begin_local = a.npc_local;
	sa.begin_tile_sums = a.npc_tile_sums;
	sa.count = a.npc;
	sa.pos_ploidy = a.pos_ploidy;
	sa.n_sel = a.n_sel;
	sa.sel = a.sel;
	sa.n_keys = (uint32_t)n_keys;
	sa.n_total = (uint32_t)n_pc;
	sa.ploidy = 0;
	sa.stride = sel_stride;
	WHAMD_TRY(rs_launch(s, times, msg, polythread_select_kernel, per_key, sa));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, r_counts, run.counts, msg));
	WHAMD_TRY(s.fetch(res, r_npc, a.npc, msg));
	WHAMD_TRY(s.fetch(res, r_n_sel, a.n_sel, msg));
	WHAMD_TRY(s.fetch(res, r_sel, a.sel, msg));
	WHAMD_TRY(s.fetch(rw.stage, rw.base, rw.total, msg));
	WHAMD_TRY(s.finish(times, msg));
	const uint32_t *res_counts = res.host(r_counts), *res_npc = res.host(r_npc), *res_n_sel = res.host(r_n_sel), *res_sel = res.host(r_sel);
	// back to the problems
	uint64_t row_at = 0;
	for (size_t x = 0; x < ps.size(); x++) {
		const ThreadProblem& p = ps[x];
		ThreadRows& o = out[x];
		const uint64_t n_pos = p.m.n_positions, stride = p.ploidy + 2;
		o.na = na;
		o.npc.assign(res_npc + pos_base[x], res_npc + pos_base[x + 1]);
		uint64_t mine = 0;
		for (uint32_t c : o.npc) mine += c;
		if (row_at + mine > n_pc) {
			msg = "internal error: the rows and their counts per position disagree";
			return WHAMD_ERR_DEVICE;
		}
		o.cluster.assign(rw.host(r_cluster) + row_at, rw.host(r_cluster) + row_at + mine);
		o.total.assign(rw.host(r_total) + row_at, rw.host(r_total) + row_at + mine);
		o.depth.assign(rw.host(r_depth) + row_at * na, rw.host(r_depth) + (row_at + mine) * na);
		o.first.assign(rw.host(r_first) + row_at * na, rw.host(r_first) + (row_at + mine) * na);
		o.cons.resize(mine * p.ploidy);
		for (uint64_t r = 0; r < mine; r++) std::memcpy(o.cons.data() + r * p.ploidy, rw.host(r_cons) + (row_at + r) * max_ploidy, p.ploidy);
		o.n_sel.assign(n_pos, 0);
		o.sel.assign(n_pos * stride, 0);
		for (uint64_t y = 0; y < n_pos; y++) {
			const uint64_t v = pos_base[x] + y;
			const uint32_t c = res_counts[v], m = res_n_sel[v];
			if (c) ++(c <= PT_CLASS_A_MAX ? o.class_a : c <= PT_CLASS_B_MAX ? o.class_b : o.class_c);
			if (m > stride || m > o.npc[y]) {
				msg = "internal error: a position's selection is longer than its rows";
				return WHAMD_ERR_DEVICE;
			}
			o.n_sel[y] = m;
			for (uint32_t k = 0; k < m; k++) {
				o.sel[y * stride + k] = res_sel[v * sel_stride + k];
				if (o.sel[y * stride + k] >= o.npc[y]) {
					msg = "internal error: a selected row outside its position";
					return WHAMD_ERR_DEVICE;
				}
			}
		}
		row_at += mine;
	}
	return WHAMD_OK;
}

whamd_status_t polythread_select_device(const std::vector<uint32_t>& begin, const std::vector<uint32_t>& count, const std::vector<uint32_t>& total, uint32_t ploidy,
                                        int device, std::vector<uint32_t>& n_sel, std::vector<uint32_t>& sel, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	const uint64_t n_keys = count.size(), stride = ploidy + 2;
	n_sel.assign(n_keys, 0);
	sel.assign(n_keys * stride, 0);
	if (!n_keys) return WHAMD_OK;
	if (n_keys * stride >= 0xfffff000ull) {
		msg = "2^32 - 4096 or more list slots in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	ImageLayout in;
	const auto p_begin = in.add<uint32_t>(n_keys);
	const auto p_count = in.add<uint32_t>(n_keys);
	const auto p_total = in.add<uint32_t>(total.size());
	ImageLayout work;
	const auto w_n_sel = work.add<uint32_t>(n_keys);
	const auto w_sel = work.add<uint32_t>(n_keys * stride);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, wk;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.stage(work, wk, msg));   // (written by the kernel, fetched whole)
	std::memcpy(im.host(p_begin), begin.data(), n_keys * sizeof(uint32_t));
	std::memcpy(im.host(p_count), count.data(), n_keys * sizeof(uint32_t));
	if (!total.empty()) std::memcpy(im.host(p_total), total.data(), total.size() * sizeof(uint32_t));
	WHAMD_TRY(s.upload(im, msg));
	PtSelectArgs sa{};
	sa.total = im.dev(p_total);
	sa.begin = im.dev(p_begin);
	sa.count = im.dev(p_count);
	sa.pos_ploidy = nullptr;
	sa.n_sel = wk.dev_out(w_n_sel);
	sa.sel = wk.dev_out(w_sel);
	sa.n_keys = (uint32_t)n_keys;
	sa.n_total = (uint32_t)total.size();
	sa.ploidy = ploidy;
	sa.stride = (uint32_t)stride;
	WHAMD_TRY(rs_launch(s, times, msg, polythread_select_kernel, dim3(grid_for(n_keys, RS_BLOCK)), sa));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(wk.stage, wk.base, wk.total, msg));
	WHAMD_TRY(s.finish(times, msg));
	std::memcpy(n_sel.data(), wk.host(w_n_sel), n_keys * sizeof(uint32_t));
	std::memcpy(sel.data(), wk.host(w_sel), n_keys * stride * sizeof(uint32_t));
	for (uint64_t v = 0; v < n_keys; v++) {
		bool ok = n_sel[v] <= stride && n_sel[v] <= count[v];
		for (uint32_t k = 0; ok && k < n_sel[v]; k++) ok = sel[v * stride + k] < count[v];
		if (!ok) {
			msg = "internal error: a position's selection does not fit its rows";
			return WHAMD_ERR_DEVICE;
		}
	}
	return WHAMD_OK;
}

whamd_status_t polythread_haplotypes_device(const uint32_t* paths, uint64_t n_pos, uint32_t ploidy, const uint64_t* pc_ptr, const uint32_t* pc_cluster,
                                            const int8_t* pc_cons, int device, std::vector<int8_t>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(n_pos * ploidy, -1);
	if (!n_pos) return WHAMD_OK;
	const uint64_t n_rows = pc_ptr[n_pos];
	ImageLayout in;
	const auto p_paths = in.add<uint32_t>(n_pos * ploidy);
	const auto p_begin = in.add<uint32_t>(n_pos + 1);
	const auto p_cluster = in.add<uint32_t>(n_rows);
	const auto p_cons = in.add<int8_t>(n_rows * ploidy);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im;
	int8_t *dev_out = nullptr, *res = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.device_block(n_pos * ploidy, (void**)&dev_out, msg));
	WHAMD_TRY(s.pinned_block(n_pos * ploidy, (void**)&res, msg));
	std::memcpy(im.host(p_paths), paths, n_pos * ploidy * sizeof(uint32_t));
	for (uint64_t x = 0; x <= n_pos; x++) im.host(p_begin)[x] = (uint32_t)pc_ptr[x];
	if (n_rows) {
		std::memcpy(im.host(p_cluster), pc_cluster, n_rows * sizeof(uint32_t));
		std::memcpy(im.host(p_cons), pc_cons, n_rows * ploidy);
	}
	WHAMD_TRY(s.upload(im, msg));
	PtHaplotypeArgs ha{im.dev(p_paths), im.dev(p_begin), im.dev(p_cluster), im.dev(p_cons), dev_out, (uint32_t)n_pos, ploidy};
	WHAMD_TRY(rs_launch(s, times, msg, polythread_haplotypes_kernel, dim3(grid_for(n_pos, RS_BLOCK)), ha));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, dev_out, n_pos * ploidy, msg));
	WHAMD_TRY(s.finish(times, msg));
	std::memcpy(out.data(), res, n_pos * ploidy);
	return WHAMD_OK;
}

}  // namespace whamd
