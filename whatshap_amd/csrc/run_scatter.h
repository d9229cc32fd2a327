// run_scatter.h -- the transposition the read-major layers share (tagphase_device.hip, priorgt_device.hip, polythread_device.hip):
// entries arrive in the order of the reads, results are per key (a variant, a column, a position), so every counted entry is moved into
// its key's run:
//   count     one thread per entry: an integer atomic on the key's counter -- one per run of neighbouring lanes with the same key.
//   scan      exclusive, two launches (run_scatter.hip): tiles of RS_SCAN_TILE counters (the tile's own prefix, the tile's total), then
//             the totals by one workgroup; run_begin() adds the two.  The first also appends every key of more than a_max / b_max
//             entries to the class b / c list.
//   place     one thread per entry again: a counted entry gets the slot run begin + atomic cursor of its key.  The order inside a run
//             is whatever the atomics give.
// The layer decides which entry counts and for which key, what it stores at the slot, and how a run is reduced or ordered (class a:
// RS_SEGMENT lanes per key over all keys; b and c: a fixed grid of RS_LIST_GRID workgroups that walks the list; what the teams that
// reduce a placed run share is run_teams.h).  Its count and place
// kernels compute the key and call scatter_count / scatter_place; its host code lays the pieces out, binds them and launches through
// the functions at the end.  Host code that is not HIP sees the constants only.
#pragma once
#include <cstdint>

namespace whamd {

constexpr uint32_t RS_BLOCK = 256;        // threads per workgroup, every kernel of a layer that scatters
constexpr uint32_t RS_SCAN_TILE = 2048;   // elements a workgroup of the scan takes
constexpr uint32_t RS_LIST_GRID = 1024;   // workgroups of the class b / c launches (they walk the device-made lists)
constexpr uint32_t RS_SEGMENT = 8;        // lanes per key in class a
constexpr uint32_t RS_NONE = 0xffffffffu; // key of an entry that is not counted; no slot

}  // namespace whamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <string>

#include "device_runtime.h"

namespace whamd {

// What count, scan and place make; embedded by value in a layer's kernel arguments.
struct RunIndex {
	uint32_t* counts;      // [n_keys] counted entries
	uint32_t* cursor;      // [n_keys] zero before place
	uint32_t* local;       // [n_keys] prefix of counts inside the tile
	uint32_t* tile_sums;   // [tiles] exclusive after the second scan launch
	uint32_t* list_n;      // [2] lengths of list b, list c
	uint32_t* list_b;      // [n_keys]
	uint32_t* list_c;      // [n_keys]
	uint32_t n_keys, n_placed, a_max, b_max;
};

__device__ inline uint32_t run_begin(const uint32_t* local, const uint32_t* tile_sums, uint32_t key) { return local[key] + tile_sums[key / RS_SCAN_TILE]; }

// ---------------------------------------------------------------------------------------------- count, place
// Neighbouring lanes of a wave with the same key form a run: its first lane and its length.  Every lane of the wave calls this.
__device__ inline void lane_run(uint32_t key, uint32_t lane, uint32_t& head_lane, uint32_t& length) {
	const uint32_t prev = (uint32_t)__shfl_up((int)key, 1);
	const uint64_t heads = __ballot(lane == 0 || key != prev);
	head_lane = 63u - (uint32_t)__clzll((long long)(heads & ((2ull << lane) - 1)));
	const uint64_t rest = head_lane == 63u ? 0ull : heads >> (head_lane + 1);
	const uint32_t next = rest ? head_lane + (uint32_t)__ffsll((unsigned long long)rest) : 64u;
	length = next - head_lane;
}

// Every lane of a wave must call the count / place functions together (key RS_NONE: the lane's entry is not counted).
__device__ inline void scatter_count(const RunIndex& x, uint32_t key, uint32_t lane) {
	uint32_t head_lane, length;
	lane_run(key, lane, head_lane, length);
	if (key != RS_NONE && lane == head_lane) atomicAdd(x.counts + key, length);
}

// The entry's slot among the n_placed; RS_NONE for an entry that is not counted and for a slot beyond them.
__device__ inline uint32_t scatter_place(const RunIndex& x, uint32_t key, uint32_t lane) {
	uint32_t head_lane, length;
	lane_run(key, lane, head_lane, length);
	uint32_t base = 0;
	if (key != RS_NONE && lane == head_lane) base = atomicAdd(x.cursor + key, length);
	base = (uint32_t)__shfl((int)base, (int)head_lane);
	if (key == RS_NONE) return RS_NONE;
	const uint32_t at = run_begin(x.local, x.tile_sums, key) + base + (lane - head_lane);
	return at < x.n_placed ? at : RS_NONE;
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

// The workgroup's exclusive prefix of `mine` (one value per thread, in thread order) and the workgroup's total; wave_total: LDS [RS_BLOCK / 64].
__device__ inline uint32_t block_exclusive(uint32_t mine, uint32_t* wave_total, uint32_t& total) {
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t inc = wave_inclusive(mine, lane);
	if (lane == 63) wave_total[w] = inc;
	__syncthreads();
	uint32_t before = 0;
	total = 0;
#pragma unroll
	for (int ww = 0; ww < (int)RS_BLOCK / 64; ww++) {
		if ((uint32_t)ww < w) before += wave_total[ww];
		total += wave_total[ww];
	}
	__syncthreads();
	return before + inc - mine;
}

// ---------------------------------------------------------------------------------------------- host
// The index's pieces of a call's work layout (Session::work()).  The call zeroes the front of its work image: rs_add_zeroed() first, then
// the layer's own zeroed pieces, then -- the layout's total is the number of bytes for Session::zero() -- rs_add_rest() and what else the
// layer makes.
struct RunPieces {
	Piece<uint32_t> counts, cursor, list_n, local, tile_sums, list_b, list_c;
};
inline uint32_t rs_tiles(uint64_t n) { return (uint32_t)((n + RS_SCAN_TILE - 1) / RS_SCAN_TILE); }
void rs_add_zeroed(ImageLayout& work, uint64_t n_keys, RunPieces& p);
void rs_add_rest(ImageLayout& work, uint64_t n_keys, RunPieces& p);
RunIndex rs_bind(const Image& work, const RunPieces& p, uint64_t n_keys, uint64_t n_placed, uint32_t a_max, uint32_t b_max);

// launch() (device_runtime.h) with RS_BLOCK threads per workgroup.
template <class... P>
whamd_status_t rs_launch(Session& s, CallTimes& times, std::string& msg, void (*kernel)(P...), dim3 grid, P... args) {
	return launch(s, times, msg, kernel, grid, dim3(RS_BLOCK), 0, args...);
}

// The two scan launches: in[n] -> local[n], tile_sums[rs_tiles(n)].  With `lists`: the elements of more than its a_max / b_max are
// appended to its list_b / list_c (lengths in its list_n).  With total_out: the sum of all goes there.
whamd_status_t rs_scan(Session& s, CallTimes& times, std::string& msg, const uint32_t* in, uint32_t* local, uint32_t* tile_sums, uint32_t n,
                       const RunIndex* lists, uint32_t* total_out);

}  // namespace whamd
#endif
