// priorgt_device.hip -- the prior genotype likelihoods on gfx950 (priorgt.h).  The reads arrive read-major, the distributions are per
// position: a scatter, done as count / scan / place like haplotagphase's -- but a column's chain rounds after every entry, so the order
// inside a run is part of the result and the runs are put into entry order before they are walked:
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

constexpr int NW = (int)PG_BLOCK / 64;
constexpr uint32_t PER_THREAD = PG_SCAN_TILE / PG_BLOCK;

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
	uint32_t* counts;             // [n_col] counted entries
	uint32_t* cursor;             // [n_col] zero before place
	uint32_t* local;              // [n_col] prefix of counts inside the tile
	uint32_t* tile_sums;          // [tiles] exclusive after the second scan launch
	uint32_t* list_n;             // [2] lengths of list b, list c
	uint32_t* list_b;             // [n_col]
	uint32_t* list_c;             // [n_col]
	uint32_t* placed;             // [n_placed] entry indices, runs in arrival order
	uint8_t* ordered;             // [n_placed] factor codes, runs in entry order
	PgOut* out;                   // [n_col]
	uint32_t n_col, n_entries, n_placed;
};

__device__ inline uint32_t run_begin(const uint32_t* local, const uint32_t* tile_sums, uint32_t c) { return local[c] + tile_sums[c / PG_SCAN_TILE]; }

// ---------------------------------------------------------------------------------------------- count, place
// Neighbouring lanes of a wave with the same column form a run: its first lane and its length.  Every lane of the wave calls this.
__device__ inline void lane_run(uint32_t c, uint32_t lane, uint32_t& head_lane, uint32_t& length) {
	const uint32_t prev = (uint32_t)__shfl_up((int)c, 1);
	const uint64_t heads = __ballot(lane == 0 || c != prev);
	head_lane = 63u - (uint32_t)__clzll((long long)(heads & ((2ull << lane) - 1)));
	const uint64_t rest = head_lane == 63u ? 0ull : heads >> (head_lane + 1);
	const uint32_t next = rest ? head_lane + (uint32_t)__ffsll((unsigned long long)rest) : 64u;
	length = next - head_lane;
}

__device__ inline uint32_t column_of(const PgArgs& a, uint32_t i) {
	if (i >= a.n_entries) return PG_NONE;
	const uint32_t c = a.entry_col[i];
	return c < a.n_col ? c : PG_NONE;
}

__global__ void __launch_bounds__(PG_BLOCK) priorgt_count_kernel(PgArgs a) {
	const uint32_t i = blockIdx.x * PG_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
	uint32_t head_lane, length;
	const uint32_t c = column_of(a, i);
	lane_run(c, lane, head_lane, length);
	if (c != PG_NONE && lane == head_lane) atomicAdd(a.counts + c, length);
}

__global__ void __launch_bounds__(PG_BLOCK) priorgt_place_kernel(PgArgs a) {
	const uint32_t i = blockIdx.x * PG_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
	uint32_t head_lane, length;
	const uint32_t c = column_of(a, i);
	lane_run(c, lane, head_lane, length);
	uint32_t base = 0;
	if (c != PG_NONE && lane == head_lane) base = atomicAdd(a.cursor + c, length);
	base = (uint32_t)__shfl((int)base, (int)head_lane);
	if (c == PG_NONE) return;
	const uint32_t at = run_begin(a.local, a.tile_sums, c) + base + (lane - head_lane);
	if (at < a.n_placed) a.placed[at] = i;
}

// ---------------------------------------------------------------------------------------------- scan
__device__ inline uint32_t wave_inclusive(uint32_t v, uint32_t lane) {
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t up = (uint32_t)__shfl_up((int)v, o);
		if (lane >= (uint32_t)o) v += up;
	}
	return v;
}

// The workgroup's exclusive prefix of `mine` (one value per thread, in thread order) and the workgroup's total.
__device__ inline uint32_t block_exclusive(uint32_t mine, uint32_t* wave_total, uint32_t& total) {
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t inc = wave_inclusive(mine, lane);
	if (lane == 63) wave_total[w] = inc;
	__syncthreads();
	uint32_t before = 0;
	total = 0;
#pragma unroll
	for (int ww = 0; ww < NW; ww++) {
		if ((uint32_t)ww < w) before += wave_total[ww];
		total += wave_total[ww];
	}
	__syncthreads();
	return before + inc - mine;
}

// counts[n] -> local[n] (prefix inside the tile), tile_sums[tile] (the tile's total); the columns beyond class a are appended to the lists.
__global__ void __launch_bounds__(PG_BLOCK) priorgt_scan_tiles_kernel(PgArgs a) {
	__shared__ uint32_t wave_total[NW];
	const uint32_t base = blockIdx.x * PG_SCAN_TILE + threadIdx.x * PER_THREAD;
	uint32_t val[PER_THREAD], mine = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		val[k] = base + k < a.n_col ? a.counts[base + k] : 0;
		mine += val[k];
	}
	uint32_t total;
	uint32_t at = block_exclusive(mine, wave_total, total);
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (base + k < a.n_col) {
			a.local[base + k] = at;
			if (val[k] > PG_CLASS_A_MAX) {
				if (val[k] <= PG_CLASS_B_MAX) a.list_b[atomicAdd(a.list_n, 1u)] = base + k;   // (the order of a list decides who takes a column, nothing else)
				else a.list_c[atomicAdd(a.list_n + 1, 1u)] = base + k;
			}
		}
		at += val[k];
	}
	if (threadIdx.x == 0) a.tile_sums[blockIdx.x] = total;
}

// tile_sums[n_tiles] exclusive in place by one workgroup.
__global__ void __launch_bounds__(PG_BLOCK) priorgt_scan_sums_kernel(uint32_t* tile_sums, uint32_t n_tiles) {
	__shared__ uint32_t wave_total[NW];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += PG_BLOCK) {
		const uint32_t x = base + threadIdx.x;
		const uint32_t mine = x < n_tiles ? tile_sums[x] : 0;
		uint32_t total;
		const uint32_t before = block_exclusive(mine, wave_total, total);
		if (x < n_tiles) tile_sums[x] = carry + before;
		carry += total;
	}
}

// ---------------------------------------------------------------------------------------------- order
// Entry `index`, the rank-th smallest of its run, hands its factor code to that place of the ordered run.
__device__ inline void put_ordered(const PgArgs& a, uint32_t begin, uint32_t n, uint32_t rank, uint32_t index) {
	const uint32_t at = begin + rank;
	if (rank < n && at < a.n_placed && index < a.n_entries) a.ordered[at] = a.entry_code[index];
}

// Class a: eight lanes per column, over all columns; those of more entries are left to the lists.  Lane l ranks entries l, l + 8, ...
// against the whole run, read straight from memory (the eight lanes read the same word).
__global__ void __launch_bounds__(PG_BLOCK) priorgt_order_a_kernel(PgArgs a) {
	const uint32_t l = threadIdx.x & (PG_SEGMENT - 1);
	const uint64_t c64 = (uint64_t)blockIdx.x * (PG_BLOCK / PG_SEGMENT) + threadIdx.x / PG_SEGMENT;
	if (c64 >= a.n_col) return;
	const uint32_t c = (uint32_t)c64, n = a.counts[c];
	if (n > PG_CLASS_A_MAX) return;
	const uint32_t begin = run_begin(a.local, a.tile_sums, c);
	if (begin + n > a.n_placed) return;
	const uint32_t* run = a.placed + begin;
	for (uint32_t e = l; e < n; e += PG_SEGMENT) {
		const uint32_t mine = run[e];
		uint32_t rank = 0;
		for (uint32_t j = 0; j < n; j++) rank += run[j] < mine ? 1u : 0u;
		put_ordered(a, begin, n, rank, mine);
	}
}

// Class b: one wave per listed column, the run in the wave's part of LDS.
__global__ void __launch_bounds__(PG_BLOCK) priorgt_order_b_kernel(PgArgs a) {
	__shared__ uint32_t keys[NW][PG_CLASS_B_MAX];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, n_list = a.list_n[0];
	for (uint32_t first = blockIdx.x * NW; first < n_list; first += gridDim.x * NW) {   // (the same trips for the four waves: the barriers are met by all)
		const uint32_t k = first + w;
		uint32_t n = 0, begin = 0;
		if (k < n_list) {
			const uint32_t c = a.list_b[k];
			n = min(a.counts[c], PG_CLASS_B_MAX);
			begin = run_begin(a.local, a.tile_sums, c);
			if ((uint64_t)begin + n > a.n_placed) n = 0;
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
// through LDS in tiles of PG_TILE; a pass ranks PG_BLOCK * PG_OWN entries.
__global__ void __launch_bounds__(PG_BLOCK) priorgt_order_c_kernel(PgArgs a) {
	__shared__ __align__(16) uint32_t keys[PG_TILE];
	const uint4* keys4 = reinterpret_cast<const uint4*>(keys);
	const uint32_t n_list = a.list_n[1];
	for (uint32_t k = blockIdx.x; k < n_list; k += gridDim.x) {   // (one column per workgroup: every thread takes the same branches, the barriers are met by all)
		const uint32_t c = a.list_c[k], n = a.counts[c];
		const uint32_t begin = run_begin(a.local, a.tile_sums, c);
		if ((uint64_t)begin + n > a.n_placed) continue;
		const uint32_t* run = a.placed + begin;
		for (uint64_t pass = 0; pass < n; pass += PG_BLOCK * PG_OWN) {
			uint32_t mine[PG_OWN], rank[PG_OWN];
#pragma unroll
			for (uint32_t o = 0; o < PG_OWN; o++) {
				const uint64_t e = pass + (uint64_t)o * PG_BLOCK + threadIdx.x;
				mine[o] = e < n ? run[e] : 0u;   // (beyond the run: ranked along, never written)
				rank[o] = 0;
			}
			for (uint32_t tile = 0; tile < n; tile += PG_TILE) {
				const uint32_t len = min(PG_TILE, n - tile), padded = (len + 3u) & ~3u;   // (PG_TILE is a multiple of four: padded <= PG_TILE)
				__syncthreads();
				for (uint32_t j = threadIdx.x; j < padded; j += PG_BLOCK) keys[j] = j < len ? run[tile + j] : PG_NONE;   // (the padding is below nobody)
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
				const uint64_t e = pass + (uint64_t)o * PG_BLOCK + threadIdx.x;
				if (e < n) put_ordered(a, begin, n, rank[o], mine[o]);
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------- chain
__global__ void __launch_bounds__(PG_BLOCK) priorgt_chain_kernel(PgArgs a) {
	__shared__ double table[3 * PG_CODES];
	for (uint32_t k = threadIdx.x; k < 3 * PG_CODES; k += PG_BLOCK) table[k] = a.table[k];
	__syncthreads();
	const uint64_t c64 = (uint64_t)blockIdx.x * PG_BLOCK + threadIdx.x;
	if (c64 >= a.n_col) return;
	const uint32_t c = (uint32_t)c64;
	uint32_t n = a.counts[c];
	const uint32_t begin = run_begin(a.local, a.tile_sums, c);
	if ((uint64_t)begin + n > a.n_placed) n = 0;
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
	const uint32_t n_tiles = (uint32_t)((n_col + PG_SCAN_TILE - 1) / PG_SCAN_TILE);
	ImageLayout in;
	const auto p_slot = in.add<uint32_t>(n_col);
	const auto p_params = in.add<PgParams>(n_in);
	const auto p_table = in.add<double>(3 * PG_CODES);
	const auto p_ecol = in.add<uint32_t>(n_entries);
	const auto p_ecode = in.add<uint8_t>(n_entries);
	// what the kernels make: the zeroed words first
	ImageLayout work;
	const auto w_counts = work.add<uint32_t>(n_col);
	const auto w_cursor = work.add<uint32_t>(n_col);
	const auto w_listn = work.add<uint32_t>(2);
	const auto w_ordered = work.add<uint8_t>(n_placed);   // (zeroed too: a code is always one of the table's)
	const size_t zeroed = work.total;
	const auto w_local = work.add<uint32_t>(n_col);
	const auto w_tiles = work.add<uint32_t>(n_tiles);
	const auto w_list_b = work.add<uint32_t>(n_col);
	const auto w_list_c = work.add<uint32_t>(n_col);
	const auto w_placed = work.add<uint32_t>(n_placed);
	const auto w_out = work.add<PgOut>(n_col);
	Session s;
	whamd_status_t st = s.open(device, 4, msg);
	if (st != WHAMD_OK) return st;
	Image im, wk;
	char* dev_work = nullptr;
	if ((st = s.stage(in, im, msg)) != WHAMD_OK) return st;
	if ((st = s.device_block(work.total, (void**)&dev_work, msg)) != WHAMD_OK) return st;
	wk.base = dev_work;
	wk.total = work.total;
	PgOut* res_out = nullptr;
	uint32_t* res_counts = nullptr;
	if ((st = s.pinned_block(n_col * sizeof(PgOut), (void**)&res_out, msg)) != WHAMD_OK) return st;
	if ((st = s.pinned_block(n_col * sizeof(uint32_t), (void**)&res_counts, msg)) != WHAMD_OK) return st;
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
	if ((st = s.upload(im, msg)) != WHAMD_OK) return st;
	HIP_TRY(hipMemsetAsync(dev_work, 0, zeroed, s.stream));
	PgArgs a{};
	a.col_slot = im.dev(p_slot);
	a.params = im.dev(p_params);
	a.table = im.dev(p_table);
	a.entry_col = im.dev(p_ecol);
	a.entry_code = im.dev(p_ecode);
	a.counts = wk.dev_out(w_counts);
	a.cursor = wk.dev_out(w_cursor);
	a.list_n = wk.dev_out(w_listn);
	a.local = wk.dev_out(w_local);
	a.tile_sums = wk.dev_out(w_tiles);
	a.list_b = wk.dev_out(w_list_b);
	a.list_c = wk.dev_out(w_list_c);
	a.placed = wk.dev_out(w_placed);
	a.ordered = wk.dev_out(w_ordered);
	a.out = wk.dev_out(w_out);
	a.n_col = (uint32_t)n_col;
	a.n_entries = (uint32_t)n_entries;
	a.n_placed = (uint32_t)n_placed;
	const dim3 block(PG_BLOCK);
	const dim3 per_entry((uint32_t)((n_entries + PG_BLOCK - 1) / PG_BLOCK)), per_segment((uint32_t)((n_col + PG_BLOCK / PG_SEGMENT - 1) / (PG_BLOCK / PG_SEGMENT))),
	    per_column((uint32_t)((n_col + PG_BLOCK - 1) / PG_BLOCK));
#define PG_LAUNCH(kernel, grid, ...)                                         \
	do {                                                                     \
		hipLaunchKernelGGL(kernel, grid, block, 0, s.stream, __VA_ARGS__);   \
		HIP_TRY(hipGetLastError());                                          \
		++times.launches;                                                    \
	} while (0)
	PG_LAUNCH(priorgt_count_kernel, per_entry, a);
	PG_LAUNCH(priorgt_scan_tiles_kernel, dim3(n_tiles), a);
	PG_LAUNCH(priorgt_scan_sums_kernel, dim3(1), a.tile_sums, n_tiles);
	PG_LAUNCH(priorgt_place_kernel, per_entry, a);
	PG_LAUNCH(priorgt_order_a_kernel, per_segment, a);
	PG_LAUNCH(priorgt_order_b_kernel, dim3(PG_LIST_GRID), a);
	PG_LAUNCH(priorgt_order_c_kernel, dim3(PG_LIST_GRID), a);
	PG_LAUNCH(priorgt_chain_kernel, per_column, a);
#undef PG_LAUNCH
	if ((st = s.kernels_done(msg)) != WHAMD_OK) return st;
	if ((st = s.fetch(res_out, a.out, n_col * sizeof(PgOut), msg)) != WHAMD_OK) return st;
	if ((st = s.fetch(res_counts, a.counts, n_col * sizeof(uint32_t), msg)) != WHAMD_OK) return st;
	if ((st = s.finish(times, msg)) != WHAMD_OK) return st;
	for (size_t x = 0; x < ps.size(); x++) {
		if (!ps[x].n_counted) continue;
		out[x].out.assign(res_out + col_base[x], res_out + col_base[x + 1]);
		out[x].count.assign(res_counts + col_base[x], res_counts + col_base[x + 1]);
	}
	return WHAMD_OK;
}

}  // namespace whamd
