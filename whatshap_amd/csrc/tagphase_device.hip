// tagphase_device.hip -- the votes and the consensus of haplotagphase on gfx950 (tagphase.h).  The reads arrive read-major, the sums are
// per variant: a scatter.  It is done as a store pass and a per-destination sum, nothing is summed through global atomics; count, scan
// and place are the shared ones of run_scatter.h, with this layer's key and payload:
//   upload    per variant {flags | problem << 8}, per problem the gap threshold, per read {phase set << 1 | haplotype, first variant of its
//             problem} and its first entry, the three entry arrays as the caller holds them (variant, id, quality).
//   count     one thread per entry: its read (read_of_entry, run_teams.h), does it vote, and an integer atomic on the variant's counter
//             -- one per run of neighbouring lanes that hit the same variant.
//   scan      exclusive, two launches: tiles of 2048 counters (the tile's own prefix, the tile's total), then the totals by one workgroup.
//             The first also appends every variant of more than 64 / 4096 entries to the class b / c list.
//   place     one thread per entry again: a voting entry goes to run begin + atomic cursor of its variant as {phase set << 1 | (haplotype
//             ^ id), quality, entry index}.  The order inside a run is whatever the atomics give; nothing below depends on it.
//   reduce    one team per variant -- class a (0 .. 64 entries) eight lanes, over all variants; class b (.. 4096) one wave and class c one
//             workgroup, both walking their list with a fixed grid.  A team keeps up to R = 4 phase sets in registers (sums of both
//             haplotypes, smallest entry index); with more it walks them in the order of the ids, one phase set per trip (slot naming,
//             scopes and walk: run_teams.h; this file has the payload, Slots and PsAcc, and the walk's body).  Either way (sum0,
//             sum1, phase set, first) go to tp_consider and the choice to tp_result (tagphase.h, shared with the host twin), which applies
//             the consensus filters; one lane writes the variant's 32 bytes.
//   rows      want_table only: the phase-set counts are scanned like the entry counts, the call waits once to size the table, then the
//             pass-per-phase-set route writes every variant's rows (eight lanes for class a, one wave for the listed variants).
// 7 launches per call, 11 with a table, whatever the problems, reads and variants (TP_LAUNCHES, TP_LAUNCHES_TABLE).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_runtime.h"
#include "run_teams.h"
#include "tagphase.h"

namespace whamd {
namespace {

constexpr int R = (int)TP_REG_PHASESETS;
constexpr int NW = RT_WAVES;

struct TpArgs {
	// the image
	const uint32_t* vinfo;        // [n_var]
	const double* gap;            // [problems of the call]
	const TpRead* reads;          // [n_reads]
	const uint32_t* read_ptr;     // [n_reads + 1]
	const uint32_t* entry_var;    // [n_entries] local to the read's problem
	const uint8_t* entry_id;
	const int32_t* entry_quality;
	// made on the device
	RunIndex run;                 // keys: the n_var variants; counted: the voting entries
	TpPlaced* placed;             // [n_placed]
	TpOut* out;                   // [n_var]
	uint32_t* nps;                // [n_var] phase sets per variant; nullptr: no table
	uint32_t* nps_local;
	uint32_t* nps_tile_sums;
	uint32_t* n_rows;             // [1]
	TpRow* rows;
	uint32_t n_reads, n_entries;
};

// ---------------------------------------------------------------------------------------------- count, place
// Entry i of the call: the variant it votes at (TP_NONE: it does not vote) and the key it votes for.
__device__ inline uint32_t voting_variant(const TpArgs& a, uint32_t i, uint32_t& key) {
	key = 0;
	if (i >= a.n_entries) return TP_NONE;
	const TpRead rd = a.reads[read_of_entry(a.read_ptr, a.n_reads, a.n_entries, i)];
	if (rd.code == TP_NOT_COUNTED) return TP_NONE;
	const uint32_t v = rd.var_base + a.entry_var[i];
	if (v >= a.run.n_keys || (a.vinfo[v] & TP_HOMOZYGOUS)) return TP_NONE;
	key = rd.code ^ (uint32_t)(a.entry_id[i] & 1u);
	return v;
}

// The scatter's key is the variant; what is placed carries the vote's key.
__global__ void __launch_bounds__(RS_BLOCK) tagphase_count_kernel(TpArgs a) {
	const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
	uint32_t key;
	scatter_count(a.run, voting_variant(a, i, key), threadIdx.x & 63u);
}

__global__ void __launch_bounds__(RS_BLOCK) tagphase_place_kernel(TpArgs a) {
	const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
	uint32_t key;
	const uint32_t at = scatter_place(a.run, voting_variant(a, i, key), threadIdx.x & 63u);
	if (at != RS_NONE) a.placed[at] = TpPlaced{key, a.entry_quality[i], i};
}

// ---------------------------------------------------------------------------------------------- reduce and decide
// The register route's phase sets (SlotNames, run_teams.h) with their sums and smallest entry index.
struct Slots : SlotNames<R> {
	int64_t s[R][2];
	uint32_t first[R];
};

// One phase set on the pass-per-phase-set route: the sums of both haplotypes and the smallest entry index.
struct PsAcc {
	int64_t s[2];
	uint32_t first;
	template <int W>
	__device__ void across() {
		s[0] = team_sum<W>(s[0]);
		s[1] = team_sum<W>(s[1]);
		first = team_min<W>(first);
	}
	__device__ void merge(const PsAcc& o) {
		s[0] += o.s[0];
		s[1] += o.s[1];
		first = min(first, o.first);
	}
};

// Placed entry i of the run, or nothing (ps = TP_NONE) beyond it.
__device__ inline void load_placed(const TpPlaced* run, uint32_t i, uint32_t n, bool on, uint32_t& ps, uint32_t& hap, int64_t& q, uint32_t& index) {
	ps = TP_NONE;
	hap = 0;
	q = 0;
	index = TP_NONE;
	if (on && i < n) {
		const TpPlaced e = run[i];
		ps = e.key >> 1;
		hap = e.key & 1u;
		q = (int64_t)e.quality;
		index = e.index;
	}
}

// The register route over run[0, n) by the W lanes of a team (lane l of the team, the team's lanes `teammask`, its first lane `lane0`).
// Every lane of the wave calls this together; n is the team's.
template <int W>
__device__ inline void scan_run(const TpPlaced* run, uint32_t n, uint32_t l, uint64_t teammask, uint32_t lane0, Slots& S) {
	S.clear();
#pragma unroll
	for (int s = 0; s < R; s++) {
		S.first[s] = TP_NONE;
		S.s[s][0] = S.s[s][1] = 0;
	}
	for (uint32_t base = 0; __any(base < n && !S.overflow); base += W) {   // (a team that has overflowed takes the other route: its sums are not used)
		uint32_t ps, hap, index;
		int64_t q;
		load_placed(run, base + l, n, !S.overflow, ps, hap, q, index);
		const int slot = S.claim(ps != TP_NONE, ps, teammask, lane0 + l, [](int, uint32_t) {});
#pragma unroll
		for (int s = 0; s < R; s++) {
			const bool here = slot == s;
			S.s[s][0] += (here && hap == 0) ? q : 0;
			S.s[s][1] += (here && hap == 1) ? q : 0;
			S.first[s] = here ? min(S.first[s], index) : S.first[s];
		}
	}
#pragma unroll
	for (int s = 0; s < R; s++)
		if (__any(S.n > (uint32_t)s)) {
			S.s[s][0] = team_sum<W>(S.s[s][0]);
			S.s[s][1] = team_sum<W>(S.s[s][1]);
			S.first[s] = team_min<W>(S.first[s]);
		}
}

// The pass-per-phase-set route for the owners with `need`: walk_ids over the run's phase sets; per phase set a second pass for its sums
// and first entry, which go to tp_consider.  rows: where the owner's `leader` lane writes one row per phase set, at most max_rows
// (nullptr: none).
template <class Scope>
__device__ inline void pass_per_phase_set(const TpPlaced* run, uint32_t n, uint32_t l, bool need, const Scope& scope, TpBest& best, TpRow* rows, uint32_t max_rows, bool leader) {
	walk_ids(
	    scope, n, l, need, [&](uint32_t i) { return run[i].key >> 1; },
	    [&](uint32_t next, bool active, uint32_t ordinal) {
		    PsAcc acc{{0, 0}, TP_NONE};
		    team_pass<Scope>(n, l, active, [&](uint32_t i) {
			    uint32_t ps, hap, index;
			    int64_t q;
			    load_placed(run, i, n, true, ps, hap, q, index);
			    const bool here = ps == next;   // (selects, not a branch: the entry stays one load)
			    acc.first = here ? min(acc.first, index) : acc.first;
			    acc.s[0] += (here && hap == 0) ? q : 0;
			    acc.s[1] += (here && hap == 1) ? q : 0;
		    });
		    scope.combine(acc);
		    if (active) {
			    tp_consider(best, acc.s[0], acc.s[1], next, acc.first);
			    if (rows && leader && ordinal < max_rows) rows[ordinal] = TpRow{acc.s[0], acc.s[1], next, acc.first, {0, 0}};
		    }
	    });
}

__device__ inline void write_result(const TpArgs& a, uint32_t v, const TpBest& best) {
	const uint32_t info = a.vinfo[v];
	a.out[v] = tp_result(best, info, a.gap[info >> 8]);
	if (a.nps) a.nps[v] = best.n_ps;
}

// A team of W lanes reduces the run of variant v (have: the team has one) and its first lane writes the result.
template <int W>
__device__ inline void reduce_by_team(const TpArgs& a, uint32_t v, bool have, uint32_t l, uint32_t lane) {
	const uint32_t lane0 = lane - l;
	const uint64_t teammask = (W == 64 ? ~0ull : ((1ull << W) - 1)) << lane0;
	const uint32_t n = have ? a.run.counts[v] : 0;
	const TpPlaced* run = a.placed + (have ? run_begin(a.run.local, a.run.tile_sums, v) : 0);
	Slots S;
	scan_run<W>(run, n, l, teammask, lane0, S);
	TpBest best = tp_start();
	if (!S.overflow) {
#pragma unroll
		for (int s = 0; s < R; s++)
			if ((uint32_t)s < S.n) tp_consider(best, S.s[s][0], S.s[s][1], S.ps[s], S.first[s]);
	}
	if (__any(S.overflow)) pass_per_phase_set(run, n, l, S.overflow, TeamScope<W>{}, best, nullptr, 0, false);
	if (have && l == 0) write_result(a, v, best);
}

// Class a: eight lanes per variant, over all variants; those of more entries are left to the lists.
__global__ void __launch_bounds__(RS_BLOCK) tagphase_reduce_a_kernel(TpArgs a) {
	const SegmentKey k = segment_key(a.run);
	reduce_by_team<(int)TP_SEGMENT>(a, k.v, k.have, k.l, threadIdx.x & 63u);
}

// Class b: one wave per listed variant.
__global__ void __launch_bounds__(RS_BLOCK) tagphase_reduce_b_kernel(TpArgs a) {
	const uint32_t lane = threadIdx.x & 63u, n_list = a.run.list_n[0];
	for (uint32_t k = blockIdx.x * NW + (threadIdx.x >> 6); k < n_list; k += gridDim.x * NW) reduce_by_team<64>(a, a.run.list_b[k], true, lane, lane);
}

// Class c: one workgroup per listed variant; every wave takes a contiguous quarter of the run, the quarters meet in LDS.
__global__ void __launch_bounds__(RS_BLOCK) tagphase_reduce_c_kernel(TpArgs a) {
	__shared__ int64_t w_sums[NW][R][2];
	__shared__ uint32_t w_ps[NW][R], w_first[NW][R], w_n[NW], w_overflow[NW];
	__shared__ PsAcc r_part[NW];
	__shared__ uint32_t r_word[NW];
	__shared__ uint32_t go_slow;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, n_list = a.run.list_n[1];
	for (uint32_t k = blockIdx.x; k < n_list; k += gridDim.x) {
		const uint32_t v = a.run.list_c[k], n = a.run.counts[v];
		const TpPlaced* run = a.placed + run_begin(a.run.local, a.run.tile_sums, v);
		const uint32_t per = ((n + NW - 1) / NW + 63u) & ~63u;
		const uint64_t b64 = (uint64_t)w * per;
		const uint32_t begin = (uint32_t)min(b64, (uint64_t)n), end = (uint32_t)min(b64 + per, (uint64_t)n);
		Slots S;
		scan_run<64>(run + begin, end - begin, lane, ~0ull, 0, S);
		if (lane == 0) {
			w_n[w] = S.n;
			w_overflow[w] = S.overflow;
#pragma unroll
			for (int s = 0; s < R; s++) {
				w_ps[w][s] = S.ps[s];
				w_first[w][s] = S.first[s];
				w_sums[w][s][0] = S.s[s][0];
				w_sums[w][s][1] = S.s[s][1];
			}
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			// merge the waves' slots by phase set; more than R distinct ones: the slower route
			uint32_t m_ps[R], m_first[R], m_n = 0;
			int64_t m_sums[R][2];
			bool slow = false;
			for (int ww = 0; ww < NW && !slow; ww++) {
				if (w_overflow[ww]) slow = true;
				for (uint32_t s = 0; s < w_n[ww] && !slow; s++) {
					uint32_t at = m_n;
					for (uint32_t y = 0; y < m_n; y++)
						if (m_ps[y] == w_ps[ww][s]) at = y;
					if (at == m_n) {
						if (m_n == (uint32_t)R) {
							slow = true;
							break;
						}
						m_ps[at] = w_ps[ww][s];
						m_first[at] = TP_NONE;
						m_sums[at][0] = m_sums[at][1] = 0;
						m_n++;
					}
					m_first[at] = min(m_first[at], w_first[ww][s]);
					m_sums[at][0] += w_sums[ww][s][0];
					m_sums[at][1] += w_sums[ww][s][1];
				}
			}
			go_slow = slow;
			if (!slow) {
				TpBest best = tp_start();
				for (uint32_t y = 0; y < m_n; y++) tp_consider(best, m_sums[y][0], m_sums[y][1], m_ps[y], m_first[y]);
				write_result(a, v, best);
			}
		}
		__syncthreads();
		if (go_slow) {
			TpBest best = tp_start();
			pass_per_phase_set(run, n, threadIdx.x, true, BlockScope<PsAcc>{r_word, r_part, lane, w}, best, nullptr, 0, false);
			if (threadIdx.x == 0) write_result(a, v, best);
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------------------------------------- table rows
__device__ inline uint32_t row_begin(const TpArgs& a, uint32_t v) { return run_begin(a.nps_local, a.nps_tile_sums, v); }

__global__ void __launch_bounds__(RS_BLOCK) tagphase_rows_a_kernel(TpArgs a) {
	const SegmentKey k = segment_key(a.run);
	const uint32_t v = k.v, l = k.l;
	const bool have = k.have && a.run.counts[v] > 0;
	TpBest best = tp_start();
	pass_per_phase_set(a.placed + (have ? run_begin(a.run.local, a.run.tile_sums, v) : 0), have ? a.run.counts[v] : 0, l, have, TeamScope<(int)TP_SEGMENT>{}, best,
	                   a.rows + (have ? row_begin(a, v) : 0), have ? a.nps[v] : 0, l == 0);
}

__global__ void __launch_bounds__(RS_BLOCK) tagphase_rows_list_kernel(TpArgs a) {
	const uint32_t lane = threadIdx.x & 63u, n_b = a.run.list_n[0], n_list = n_b + a.run.list_n[1];
	for (uint32_t k = blockIdx.x * NW + (threadIdx.x >> 6); k < n_list; k += gridDim.x * NW) {
		const uint32_t v = k < n_b ? a.run.list_b[k] : a.run.list_c[k - n_b];
		TpBest best = tp_start();
		pass_per_phase_set(a.placed + run_begin(a.run.local, a.run.tile_sums, v), a.run.counts[v], lane, true, TeamScope<64>{}, best, a.rows + row_begin(a, v), a.nps[v], lane == 0);
	}
}

}  // namespace

whamd_status_t tagphase_device(const std::vector<TagphaseProblem>& ps, int device, std::vector<TagphaseScores>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(ps.size(), TagphaseScores{});
	// the problems with a voting entry are the call's: their variants, reads and entries one after the other
	std::vector<uint64_t> var_base(ps.size() + 1, 0), read_base(ps.size() + 1, 0), ent_base(ps.size() + 1, 0), slot(ps.size() + 1, 0);
	uint64_t n_placed = 0;
	bool want_table = false;
	for (size_t x = 0; x < ps.size(); x++) {
		const bool in = ps[x].n_voting > 0;
		var_base[x + 1] = var_base[x] + (in ? ps[x].n_variants : 0);
		read_base[x + 1] = read_base[x] + (in ? ps[x].n_reads : 0);
		ent_base[x + 1] = ent_base[x] + (in ? ps[x].n_entries : 0);
		slot[x + 1] = slot[x] + (in ? 1 : 0);
		n_placed += ps[x].n_voting;
		want_table = want_table || (in && ps[x].want_table);
	}
	const uint64_t n_var = var_base[ps.size()], n_reads = read_base[ps.size()], n_entries = ent_base[ps.size()], n_in = slot[ps.size()];
	if (!n_placed) return WHAMD_OK;   // nothing votes: no device work at all
	if (n_var >= 0xfffff000ull || n_entries >= 0xfffff000ull || n_in >= (1ull << 24)) {   // (indices are uint32 with room to round grids up)
		msg = "2^32 - 4096 or more variants or entries, or 2^24 or more problems, in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	ImageLayout in;
	const auto p_vinfo = in.add<uint32_t>(n_var);
	const auto p_gap = in.add<double>(n_in);
	const auto p_reads = in.add<TpRead>(n_reads);
	const auto p_rptr = in.add<uint32_t>(n_reads + 1);
	const auto p_evar = in.add<uint32_t>(n_entries);
	const auto p_eq = in.add<int32_t>(n_entries);
	const auto p_eid = in.add<uint8_t>(n_entries);
	// what the kernels make: the zeroed words first
	ImageLayout work;
	RunPieces w_run;
	rs_add_zeroed(work, n_var, w_run);
	const auto w_n_rows = work.add<uint32_t>(1);
	const size_t zeroed = work.total;
	rs_add_rest(work, n_var, w_run);
	const auto w_nps = work.add<uint32_t>(want_table ? n_var : 0);
	const auto w_nps_local = work.add<uint32_t>(want_table ? n_var : 0);
	const auto w_nps_tiles = work.add<uint32_t>(want_table ? rs_tiles(n_var) : 0);
	const auto w_placed = work.add<TpPlaced>(n_placed);
	const auto w_out = work.add<TpOut>(n_var);
	ImageLayout results;   // what comes back
	const auto r_out = results.add<TpOut>(n_var);
	const auto r_counts = results.add<uint32_t>(n_var);
	const auto r_n_rows = results.add<uint32_t>(1);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, wk, res, rows;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.work(work, wk, msg));
	WHAMD_TRY(s.results(results, res, msg));
	// the image: per variant and per read a few words; the entry arrays are copied as they are
	for (size_t x = 0; x < ps.size(); x++) {
		const TagphaseProblem& p = ps[x];
		if (!p.n_voting) continue;
		const whamd_tagphase_view& v = *p.view;
		const uint32_t bits = (v.only_indels ? (uint32_t)TP_ONLY_INDELS : 0u) | ((uint32_t)slot[x] << 8);
		im.host(p_gap)[slot[x]] = v.gap_threshold;
		uint32_t* vinfo = im.host(p_vinfo) + var_base[x];
		for (uint64_t y = 0; y < p.n_variants; y++) vinfo[y] = v.variant_flags[y] | bits;
		TpRead* reads = im.host(p_reads) + read_base[x];
		uint32_t* rptr = im.host(p_rptr) + read_base[x];
		for (uint64_t r = 0; r < p.n_reads; r++) {
			reads[r] = TpRead{p.read_code[r], (uint32_t)var_base[x]};
			rptr[r] = (uint32_t)(ent_base[x] + v.read_ptr[r]);
		}
		const uint64_t chunk = (uint64_t)1 << 20, n_chunks = (p.n_entries + chunk - 1) / chunk;
		parallel_ranges(n_chunks, host_threads(p.n_entries, 1 << 20), [&](uint64_t b, uint64_t e, uint32_t) {
			const uint64_t from = b * chunk, n = std::min(e * chunk, p.n_entries) - from;
			std::memcpy(im.host(p_evar) + ent_base[x] + from, v.entry_variant + from, n * sizeof(uint32_t));
			std::memcpy(im.host(p_eq) + ent_base[x] + from, v.entry_quality + from, n * sizeof(int32_t));
			std::memcpy(im.host(p_eid) + ent_base[x] + from, v.entry_id + from, n);
		});
	}
	im.host(p_rptr)[n_reads] = (uint32_t)n_entries;
	WHAMD_TRY(s.upload(im, msg));
	WHAMD_TRY(s.zero(wk, zeroed, msg));
	TpArgs a{};
	a.vinfo = im.dev(p_vinfo);
	a.gap = im.dev(p_gap);
	a.reads = im.dev(p_reads);
	a.read_ptr = im.dev(p_rptr);
	a.entry_var = im.dev(p_evar);
	a.entry_id = im.dev(p_eid);
	a.entry_quality = im.dev(p_eq);
	a.run = rs_bind(wk, w_run, n_var, n_placed, TP_CLASS_A_MAX, TP_CLASS_B_MAX);
	a.n_rows = wk.dev_out(w_n_rows);
	a.nps = want_table ? wk.dev_out(w_nps) : nullptr;
	a.nps_local = want_table ? wk.dev_out(w_nps_local) : nullptr;
	a.nps_tile_sums = want_table ? wk.dev_out(w_nps_tiles) : nullptr;
	a.placed = wk.dev_out(w_placed);
	a.out = wk.dev_out(w_out);
	a.rows = nullptr;
	a.n_reads = (uint32_t)n_reads;
	a.n_entries = (uint32_t)n_entries;
	const RunIndex& run = a.run;
	const dim3 per_entry(grid_for(n_entries, RS_BLOCK)), per_segment(grid_for(n_var, RS_BLOCK / TP_SEGMENT));
	const auto launch = [&](void (*kernel)(TpArgs), dim3 grid) { return rs_launch(s, times, msg, kernel, grid, a); };
	WHAMD_TRY(launch(tagphase_count_kernel, per_entry));
	WHAMD_TRY(rs_scan(s, times, msg, run.counts, run.local, run.tile_sums, run.n_keys, &run, nullptr));
	WHAMD_TRY(launch(tagphase_place_kernel, per_entry));
	WHAMD_TRY(launch(tagphase_reduce_a_kernel, per_segment));
	WHAMD_TRY(launch(tagphase_reduce_b_kernel, dim3(RS_LIST_GRID)));
	WHAMD_TRY(launch(tagphase_reduce_c_kernel, dim3(RS_LIST_GRID)));
	Piece<TpRow> r_rows;
	uint64_t n_rows = 0;
	if (want_table) {
		WHAMD_TRY(rs_scan(s, times, msg, a.nps, a.nps_local, a.nps_tile_sums, run.n_keys, nullptr, a.n_rows));
		WHAMD_TRY(s.fetch_now(res, r_n_rows, a.n_rows, msg));   // the table's size
		n_rows = *res.host(r_n_rows);
		if (n_rows > n_placed) {
			msg = "internal error: more table rows than voting entries";
			return WHAMD_ERR_DEVICE;
		}
		ImageLayout table;   // the second result image: sized by the wait
		r_rows = table.add<TpRow>(n_rows);
		WHAMD_TRY(s.stage(table, rows, msg));
		a.rows = rows.dev_out(r_rows);
		WHAMD_TRY(launch(tagphase_rows_a_kernel, per_segment));
		WHAMD_TRY(launch(tagphase_rows_list_kernel, dim3(RS_LIST_GRID)));
	}
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, r_out, a.out, msg));
	WHAMD_TRY(s.fetch(res, r_counts, run.counts, msg));
	if (n_rows) WHAMD_TRY(s.fetch(rows, r_rows, a.rows, msg));
	WHAMD_TRY(s.finish(times, msg));
	// back to the problems: entry indices become local to each
	const TpOut* res_out = res.host(r_out);
	const uint32_t* res_counts = res.host(r_counts);
	const TpRow* res_rows = rows.host(r_rows);   // (null without a table)
	uint64_t row_at = 0;
	for (size_t x = 0; x < ps.size(); x++) {
		const TagphaseProblem& p = ps[x];
		if (!p.n_voting) continue;
		TagphaseScores& sc = out[x];
		sc.out.assign(res_out + var_base[x], res_out + var_base[x + 1]);
		sc.count.assign(res_counts + var_base[x], res_counts + var_base[x + 1]);
		const uint32_t eb = (uint32_t)ent_base[x];
		for (TpOut& o : sc.out)
			if (o.flags & TP_VOTED) o.first -= eb;
		if (!want_table) continue;
		sc.row_ptr.assign(p.n_variants + 1, 0);
		for (uint64_t y = 0; y < p.n_variants; y++) sc.row_ptr[y + 1] = sc.row_ptr[y] + sc.out[y].n_ps;
		const uint64_t mine = sc.row_ptr[p.n_variants];
		if (row_at + mine > n_rows) {
			msg = "internal error: the table's rows and the phase-set counts disagree";
			return WHAMD_ERR_DEVICE;
		}
		if (p.want_table) {
			sc.rows.assign(res_rows + row_at, res_rows + row_at + mine);
			for (TpRow& row : sc.rows) row.first -= eb;
		} else {
			sc.row_ptr.clear();
		}
		row_at += mine;
	}
	return WHAMD_OK;
}

}  // namespace whamd
