// realign_shape.h -- the launch shape of realign's long jobs (queries longer than 64): plain host code, shared by the drivers of
// realign_device.hip and by the debug library's export (whamd_debug_realign_long_shape), so that a test can hold the shape of a call.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace whamd {

constexpr uint32_t MAX_LONG_BLOCKS = 1024;
constexpr size_t LDS_LIMIT = 64 << 10;
constexpr size_t SCRATCH_BUDGET = (size_t)512 << 20;   // scratch rows of the long-job launch: the grid shrinks to stay within this (at least one block)

// Launch shape of the jobs with a query longer than 64 whose longest allele window is `max_target` bytes.
struct LongShape {
	uint32_t blocks = 0, block = 64;
	size_t lds = 0;           // dynamic LDS per block (affine rows in LDS)
	size_t scratch = 0;       // bytes of global scratch (unit carry rows, or affine rows that do not fit in LDS)
	uint32_t carry_words = 0, row_floats = 0;
	bool global_rows = false;
};
inline LongShape long_shape(bool affine, uint64_t n_long, uint32_t max_target) {
	LongShape s;
	if (n_long == 0) return s;   // no second launch
	if (affine) {
		s.row_floats = 3 * (max_target + 1);
		const size_t row = (size_t)s.row_floats * 4;
		s.block = row * 4 <= LDS_LIMIT ? 256 : 64;
		s.global_rows = row > LDS_LIMIT;
		const uint64_t waves = s.block / 64;
		uint64_t blocks = std::min<uint64_t>((n_long + waves - 1) / waves, MAX_LONG_BLOCKS);
		if (s.global_rows) blocks = std::max<uint64_t>(1, std::min<uint64_t>(blocks, SCRATCH_BUDGET / row));
		s.blocks = (uint32_t)blocks;
		s.lds = s.global_rows ? 0 : row * waves;
		s.scratch = s.global_rows ? row * blocks : 0;
	} else {
		s.carry_words = 2 * ((std::max(max_target, 1u) + 63) / 64);
		const size_t per_block = (size_t)s.block * s.carry_words * 8;
		s.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>((n_long + s.block - 1) / s.block, MAX_LONG_BLOCKS),
		                                                              SCRATCH_BUDGET / per_block));
		s.scratch = per_block * s.blocks;
	}
	return s;
}

// The long jobs of a raw distance batch (pairs whose query is longer than 64, in pair order) and their longest target; lengths below 2^32.
inline uint32_t long_pairs_of(uint64_t n_pairs, const uint64_t* query_ptr, const uint64_t* target_ptr, std::vector<uint32_t>& long_pairs) {
	uint32_t max_t_long = 0;
	for (uint64_t p = 0; p < n_pairs; ++p) {
		if (query_ptr[p + 1] - query_ptr[p] > 64) {
			long_pairs.push_back((uint32_t)p);
			max_t_long = (uint32_t)std::max<uint64_t>(max_t_long, target_ptr[p + 1] - target_ptr[p]);
		}
	}
	return max_t_long;
}

}  // namespace whamd
