// run_scatter.hip -- the scan of the shared transposition (run_scatter.h) and the host functions around the index's pieces.
#include "run_scatter.h"

namespace whamd {
namespace {

constexpr int NW = (int)RS_BLOCK / 64;
constexpr uint32_t PER_THREAD = RS_SCAN_TILE / RS_BLOCK;

// in[n] -> local[n] (prefix inside the tile), tile_sums[tile] (the tile's total).  With lists: the elements beyond class a are appended
// (the order of a list decides who takes a key, nothing else).
__global__ void __launch_bounds__(RS_BLOCK) run_scan_tiles_kernel(const uint32_t* in, uint32_t* local, uint32_t* tile_sums, uint32_t n, uint32_t* list_n,
                                                                  uint32_t* list_b, uint32_t* list_c, uint32_t a_max, uint32_t b_max) {
	__shared__ uint32_t wave_total[NW];
	const uint32_t base = blockIdx.x * RS_SCAN_TILE + threadIdx.x * PER_THREAD;
	uint32_t val[PER_THREAD], mine = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		val[k] = base + k < n ? in[base + k] : 0;
		mine += val[k];
	}
	uint32_t total;
	uint32_t at = block_exclusive(mine, wave_total, total);
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (base + k < n) {
			local[base + k] = at;
			if (list_n && val[k] > a_max) {
				if (val[k] <= b_max) list_b[atomicAdd(list_n, 1u)] = base + k;
				else list_c[atomicAdd(list_n + 1, 1u)] = base + k;
			}
		}
		at += val[k];
	}
	if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// tile_sums[n_tiles] exclusive in place by one workgroup; *total_out, if wanted, the sum of all.
__global__ void __launch_bounds__(RS_BLOCK) run_scan_sums_kernel(uint32_t* tile_sums, uint32_t n_tiles, uint32_t* total_out) {
	__shared__ uint32_t wave_total[NW];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += RS_BLOCK) {
		const uint32_t x = base + threadIdx.x;
		const uint32_t mine = x < n_tiles ? tile_sums[x] : 0;
		uint32_t total;
		const uint32_t before = block_exclusive(mine, wave_total, total);
		if (x < n_tiles) tile_sums[x] = carry + before;
		carry += total;
	}
	if (total_out && threadIdx.x == 0) *total_out = carry;
}

}  // namespace

void rs_add_zeroed(ImageLayout& work, uint64_t n_keys, RunPieces& p) {
	p.counts = work.add<uint32_t>(n_keys);
	p.cursor = work.add<uint32_t>(n_keys);
	p.list_n = work.add<uint32_t>(2);
}

void rs_add_rest(ImageLayout& work, uint64_t n_keys, RunPieces& p) {
	p.local = work.add<uint32_t>(n_keys);
	p.tile_sums = work.add<uint32_t>(rs_tiles(n_keys));
	p.list_b = work.add<uint32_t>(n_keys);
	p.list_c = work.add<uint32_t>(n_keys);
}

RunIndex rs_bind(const Image& work, const RunPieces& p, uint64_t n_keys, uint64_t n_placed, uint32_t a_max, uint32_t b_max) {
	return RunIndex{work.dev_out(p.counts), work.dev_out(p.cursor), work.dev_out(p.local), work.dev_out(p.tile_sums), work.dev_out(p.list_n), work.dev_out(p.list_b),
	                work.dev_out(p.list_c), (uint32_t)n_keys, (uint32_t)n_placed, a_max, b_max};
}

whamd_status_t rs_scan(Session& s, CallTimes& times, std::string& msg, const uint32_t* in, uint32_t* local, uint32_t* tile_sums, uint32_t n,
                       const RunIndex* lists, uint32_t* total_out) {
	const uint32_t n_tiles = rs_tiles(n);
	const RunIndex none{};
	const RunIndex& l = lists ? *lists : none;
	WHAMD_TRY(rs_launch(s, times, msg, run_scan_tiles_kernel, dim3(n_tiles), in, local, tile_sums, n, l.list_n, l.list_b, l.list_c, l.a_max, l.b_max));
	return rs_launch(s, times, msg, run_scan_sums_kernel, dim3(1), tile_sums, n_tiles, total_out);
}

}  // namespace whamd
