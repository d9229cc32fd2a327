// priorgt_device.hip -- the prior genotype likelihoods on gfx950 (priorgt.h).  The reads arrive read-major, the distributions are per
// position: a scatter, done with the count / scan / place that haplotagphase uses too (run_scatter.h; the key is the column, what is
// placed the entry's index) -- but a column's chain rounds after every entry, so the order inside a run is part of the result and the
// runs are put into entry order before they are walked:
//   upload    per column the problem's place in the call, per problem (constant, gt_prob, want_regularized), the 30 factor triples, per
//             entry its column in the call (PG_NONE: not counted) and its factor code.
//   count     one thread per entry: an integer atomic on the column's counter -- one per run of neighbouring lanes with the same column.
//   scan      exclusive, two launches: tiles of 2048 counters (the tile's own prefix, the tile's total), then the totals by one
//             workgroup.  The first also appends every column of more than 64 / 1024 entries to the class b / c list.
//   place     one thread per entry again: a counted entry's INDEX goes to run begin + atomic cursor of its column.  The order inside a
//             run is whatever the atomics give.
//   order     every run is sorted by entry index -- entry order is read order, and a read has at most one entry per column.  The indices
//             of a run are distinct, so an entry's place is the number of smaller ones: a rank, computed by comparing, written once, no
//             exchange and no dependence on where the atomics put it.  The factor code of the entry goes to that place of a second
//             array.  Class a (0 .. 64 entries) eight lanes per column straight from memory, over all columns; class b (.. 1024) one
//             wave with the run in LDS; class c one workgroup that streams the run through LDS in tiles of 4096 while every thread
//             ranks eight of its entries -- any length.  b and c walk their list with a fixed grid.
//   chain     one lane per column walks its ordered codes through pg_chain and pg_tail (priorgt.h, shared with the host twin) with the
//             factor table in LDS and writes the column's record.  The chain is sequential by definition: it is not split.
// 8 launches per call whatever the problems, reads and positions (PG_LAUNCHES).  No fast-math anywhere; f64 division is the compiler's
// IEEE sequence, subnormals included.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_runtime.h"
#include "priorgt.h"

namespace whamd {
namespace {

constexpr int NW = (int)RS_BLOCK / 64;

struct PgParams {
	double constant, gt_prob;
	uint32_t want_reg, pad;
};

struct PgArgs {
	// the image
	const uint32_t* col_slot;     // [n_col] the problem's place in the call
	const PgParams* params;       // [problems of the call]
	const double* table;          // [PG_CODES][3]
	const uint32_t* entry_col;    // [n_entries] column in the call, PG_NONE
	const uint8_t* entry_code;    // [n_entries]
	// made on the device
	RunIndex run;                 // keys: the n_col columns
	uint32_t* placed;             // [n_placed] entry indices, runs in arrival order
	uint8_t* ordered;             // [n_placed] factor codes, runs in entry order
	PgOut* out;                   // [n_col]
	uint32_t n_entries;
};

// ---------------------------------------------------------------------------------------------- count, place
__device__ inline uint32_t column_of(const PgArgs& a, uint32_t i) {
	if (i >= a.n_entries) return PG_NONE;
	const uint32_t c = a.entry_col[i];
	return c < a.run.n_keys ? c : PG_NONE;
}

__global__ void __launch_bounds__(RS_BLOCK) priorgt_count_kernel(PgArgs a) {
	const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
	scatter_count(a.run, column_of(a, i), threadIdx.x & 63u);
}

__global__ void __launch_bounds__(RS_BLOCK) priorgt_place_kernel(PgArgs a) {
	const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
	const uint32_t at = scatter_place(a.run, column_of(a, i), threadIdx.x & 63u);
	if (at != RS_NONE) a.placed[at] = i;
}

// ---------------------------------------------------------------------------------------------- order
// Entry `index`, the rank-th smallest of its run, hands its factor code to that place of the ordered run.
__device__ inline void put_ordered(const PgArgs& a, uint32_t begin, uint32_t n, uint32_t rank, uint32_t index) {
	const uint32_t at = begin + rank;
	if (rank < n && at < a.run.n_placed && index < a.n_entries) a.ordered[at] = a.entry_code[index];
}

// Class a: eight lanes per column, over all columns; those of more entries are left to the lists.  Lane l ranks entries l, l + 8, ...
// against the whole run, read straight from memory (the eight lanes read the same word).
__global__ void __launch_bounds__(RS_BLOCK) priorgt_order_a_kernel(PgArgs a) {
	const uint32_t l = threadIdx.x & (RS_SEGMENT - 1);
	const uint64_t c64 = (uint64_t)blockIdx.x * (RS_BLOCK / RS_SEGMENT) + threadIdx.x / RS_SEGMENT;
	if (c64 >= a.run.n_keys) return;
	const uint32_t c = (uint32_t)c64, n = a.run.counts[c];
	if (n > PG_CLASS_A_MAX) return;
	const uint32_t begin = run_begin(a.run.local, a.run.tile_sums, c);
	if (begin + n > a.run.n_placed) return;
	const uint32_t* run = a.placed + begin;
	for (uint32_t e = l; e < n; e += RS_SEGMENT) {
		const uint32_t mine = run[e];
		uint32_t rank = 0;
		for (uint32_t j = 0; j < n; j++) rank += run[j] < mine ? 1u : 0u;
		put_ordered(a, begin, n, rank, mine);
	}
}

// Class b: one wave per listed column, the run in the wave's part of LDS.
__global__ void __launch_bounds__(RS_BLOCK) priorgt_order_b_kernel(PgArgs a) {
	__shared__ uint32_t keys[NW][PG_CLASS_B_MAX];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, n_list = a.run.list_n[0];
	for (uint32_t first = blockIdx.x * NW; first < n_list; first += gridDim.x * NW) {   // (the same trips for the four waves: the barriers are met by all)
		const uint32_t k = first + w;
		uint32_t n = 0, begin = 0;
		if (k < n_list) {
			const uint32_t c = a.run.list_b[k];
			n = min(a.run.counts[c], PG_CLASS_B_MAX);
			begin = run_begin(a.run.local, a.run.tile_sums, c);
			if ((uint64_t)begin + n > a.run.n_placed) n = 0;
		}
		const uint32_t* run = a.placed + begin;
		__syncthreads();
		for (uint32_t e = lane; e < n; e += 64) keys[w][e] = run[e];
		__syncthreads();
		for (uint32_t e = lane; e < n; e += 64) {
			const uint32_t mine = keys[w][e];
			uint32_t rank = 0;
			for (uint32_t j = 0; j < n; j++) rank += keys[w][j] < mine ? 1u : 0u;
			put_ordered(a, begin, n, rank, mine);
		}
	}
}

// Class c: one workgroup per listed column, any length.  Per pass every thread takes PG_OWN entries of the run and the whole run goes
// through LDS in tiles of PG_TILE; a pass ranks RS_BLOCK * PG_OWN entries.
__global__ void __launch_bounds__(RS_BLOCK) priorgt_order_c_kernel(PgArgs a) {
	__shared__ __align__(16) uint32_t keys[PG_TILE];
	const uint4* keys4 = reinterpret_cast<const uint4*>(keys);
	const uint32_t n_list = a.run.list_n[1];
	for (uint32_t k = blockIdx.x; k < n_list; k += gridDim.x) {   // (one column per workgroup: every thread takes the same branches, the barriers are met by all)
		const uint32_t c = a.run.list_c[k], n = a.run.counts[c];
		const uint32_t begin = run_begin(a.run.local, a.run.tile_sums, c);
		if ((uint64_t)begin + n > a.run.n_placed) continue;
		const uint32_t* run = a.placed + begin;
		for (uint64_t pass = 0; pass < n; pass += RS_BLOCK * PG_OWN) {
			uint32_t mine[PG_OWN], rank[PG_OWN];
#pragma unroll
			for (uint32_t o = 0; o < PG_OWN; o++) {
				const uint64_t e = pass + (uint64_t)o * RS_BLOCK + threadIdx.x;
				mine[o] = e < n ? run[e] : 0u;   // (beyond the run: ranked along, never written)
				rank[o] = 0;
			}
			for (uint32_t tile = 0; tile < n; tile += PG_TILE) {
				const uint32_t len = min(PG_TILE, n - tile), padded = (len + 3u) & ~3u;   // (PG_TILE is a multiple of four: padded <= PG_TILE)
				__syncthreads();
				for (uint32_t j = threadIdx.x; j < padded; j += RS_BLOCK) keys[j] = j < len ? run[tile + j] : PG_NONE;   // (the padding is below nobody)
				__syncthreads();
				for (uint32_t j = 0; j < padded / 4; j++) {
					const uint4 other = keys4[j];   // (one 16-byte LDS read, the same for every lane, per four entries)
#pragma unroll
					for (uint32_t o = 0; o < PG_OWN; o++)
						rank[o] += (other.x < mine[o] ? 1u : 0u) + (other.y < mine[o] ? 1u : 0u) + (other.z < mine[o] ? 1u : 0u) + (other.w < mine[o] ? 1u : 0u);
				}
			}
#pragma unroll
			for (uint32_t o = 0; o < PG_OWN; o++) {
				const uint64_t e = pass + (uint64_t)o * RS_BLOCK + threadIdx.x;
				if (e < n) put_ordered(a, begin, n, rank[o], mine[o]);
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------- chain
__global__ void __launch_bounds__(RS_BLOCK) priorgt_chain_kernel(PgArgs a) {
	__shared__ double table[3 * PG_CODES];
	for (uint32_t k = threadIdx.x; k < 3 * PG_CODES; k += RS_BLOCK) table[k] = a.table[k];
	__syncthreads();
	const uint64_t c64 = (uint64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
	if (c64 >= a.run.n_keys) return;
	const uint32_t c = (uint32_t)c64;
	uint32_t n = a.run.counts[c];
	const uint32_t begin = run_begin(a.run.local, a.run.tile_sums, c);
	if ((uint64_t)begin + n > a.run.n_placed) n = 0;
	double d[3];
	pg_chain(a.ordered + begin, n, table, d);
	const PgParams p = a.params[a.col_slot[c]];
	a.out[c] = pg_tail(d, p.constant, p.gt_prob, p.want_reg != 0);
}

}  // namespace

whamd_status_t priorgt_device(const std::vector<PriorProblem>& ps, int device, std::vector<PriorScores>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(ps.size(), PriorScores{});
	// the problems with a counted entry are the call's: their columns and entries one after the other
	std::vector<uint64_t> col_base(ps.size() + 1, 0), ent_base(ps.size() + 1, 0), slot(ps.size() + 1, 0);
	uint64_t n_placed = 0;
	for (size_t x = 0; x < ps.size(); x++) {
		const bool in = ps[x].n_counted > 0;
		col_base[x + 1] = col_base[x] + (in ? ps[x].n_positions : 0);
		ent_base[x + 1] = ent_base[x] + (in ? ps[x].n_entries : 0);
		slot[x + 1] = slot[x] + (in ? 1 : 0);
		n_placed += ps[x].n_counted;
	}
	const uint64_t n_col = col_base[ps.size()], n_entries = ent_base[ps.size()], n_in = slot[ps.size()];
	if (!n_placed) return WHAMD_OK;   // nothing counts: no device work at all
	if (n_col >= 0xfffff000ull || n_entries >= 0xfffff000ull) {   // (indices are uint32 with room to round grids up)
		msg = "2^32 - 4096 or more positions or entries in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	ImageLayout in;
	const auto p_slot = in.add<uint32_t>(n_col);
	const auto p_params = in.add<PgParams>(n_in);
	const auto p_table = in.add<double>(3 * PG_CODES);
	const auto p_ecol = in.add<uint32_t>(n_entries);
	const auto p_ecode = in.add<uint8_t>(n_entries);
	// what the kernels make: the zeroed words first
	ImageLayout work;
	RunPieces w_run;
	rs_add_zeroed(work, n_col, w_run);
	const auto w_ordered = work.add<uint8_t>(n_placed);   // (zeroed too: a code is always one of the table's)
	const size_t zeroed = work.total;
	rs_add_rest(work, n_col, w_run);
	const auto w_placed = work.add<uint32_t>(n_placed);
	const auto w_out = work.add<PgOut>(n_col);
	ImageLayout results;   // what comes back
	const auto r_out = results.add<PgOut>(n_col);
	const auto r_counts = results.add<uint32_t>(n_col);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, wk, res;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.work(work, wk, msg));
	WHAMD_TRY(s.results(results, res, msg));
	// the image: a word per column, and per entry the column moved to its place in the call and the code as prepared
	pg_factor_table(im.host(p_table));
	for (size_t x = 0; x < ps.size(); x++) {
		const PriorProblem& p = ps[x];
		if (!p.n_counted) continue;
		const whamd_prior_genotypes_view& v = *p.view;
		im.host(p_params)[slot[x]] = PgParams{v.constant, v.gt_prob, p.want_reg ? 1u : 0u, 0u};
		uint32_t* col_slot = im.host(p_slot) + col_base[x];
		for (uint64_t c = 0; c < p.n_positions; c++) col_slot[c] = (uint32_t)slot[x];
		const uint32_t cb = (uint32_t)col_base[x];
		uint32_t* ecol = im.host(p_ecol) + ent_base[x];
		uint8_t* ecode = im.host(p_ecode) + ent_base[x];
		parallel_ranges(p.n_entries, host_threads(p.n_entries, 1 << 20), [&](uint64_t b, uint64_t e, uint32_t) {
			for (uint64_t i = b; i < e; i++) ecol[i] = p.column[i] == PG_NONE ? PG_NONE : p.column[i] + cb;
			std::memcpy(ecode + b, p.code.data() + b, e - b);
		});
	}
	WHAMD_TRY(s.upload(im, msg));
	WHAMD_TRY(s.zero(wk, zeroed, msg));
	PgArgs a{};
	a.col_slot = im.dev(p_slot);
	a.params = im.dev(p_params);
	a.table = im.dev(p_table);
	a.entry_col = im.dev(p_ecol);
	a.entry_code = im.dev(p_ecode);
	a.run = rs_bind(wk, w_run, n_col, n_placed, PG_CLASS_A_MAX, PG_CLASS_B_MAX);
	a.placed = wk.dev_out(w_placed);
	a.ordered = wk.dev_out(w_ordered);
	a.out = wk.dev_out(w_out);
	a.n_entries = (uint32_t)n_entries;
	const RunIndex& run = a.run;
	const dim3 per_entry(grid_for(n_entries, RS_BLOCK)), per_segment(grid_for(n_col, RS_BLOCK / RS_SEGMENT)), per_column(grid_for(n_col, RS_BLOCK));
	const auto launch = [&](void (*kernel)(PgArgs), dim3 grid) { return rs_launch(s, times, msg, kernel, grid, a); };
	WHAMD_TRY(launch(priorgt_count_kernel, per_entry));
	WHAMD_TRY(rs_scan(s, times, msg, run.counts, run.local, run.tile_sums, run.n_keys, &run, nullptr));
	WHAMD_TRY(launch(priorgt_place_kernel, per_entry));
	WHAMD_TRY(launch(priorgt_order_a_kernel, per_segment));
	WHAMD_TRY(launch(priorgt_order_b_kernel, dim3(RS_LIST_GRID)));
	WHAMD_TRY(launch(priorgt_order_c_kernel, dim3(RS_LIST_GRID)));
	WHAMD_TRY(launch(priorgt_chain_kernel, per_column));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, r_out, a.out, msg));
	WHAMD_TRY(s.fetch(res, r_counts, run.counts, msg));
	WHAMD_TRY(s.finish(times, msg));
	const PgOut* res_out = res.host(r_out);
	const uint32_t* res_counts = res.host(r_counts);
	for (size_t x = 0; x < ps.size(); x++) {
		if (!ps[x].n_counted) continue;
		out[x].out.assign(res_out + col_base[x], res_out + col_base[x + 1]);
		out[x].count.assign(res_counts + col_base[x], res_counts + col_base[x + 1]);
	}
	return WHAMD_OK;
}

}  // namespace whamd
