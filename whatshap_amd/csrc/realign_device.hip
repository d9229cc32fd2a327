// realign_device.hip -- gfx950 kernels of allele detection by re-alignment (realign.h) and of the raw distance batch.
//
//   unit costs    edit_distance (whatshap/align.pyx:16-97): global Levenshtein distance, exact.  One lane per job; the lane runs its job's
//                 alleles one after the other and decides.  Common prefix and suffix are stripped first (they do not change a unit edit
//                 distance, and an SNV window of 21 bases keeps one or two columns), then bit-parallel Myers / Hyyro with 64-bit words: the
//                 query in words of 64 rows, one word after the other over the whole target, the horizontal deltas between two words kept
//                 as bit planes in a per-lane scratch row (queries longer than 64 only).  Match masks for A / C / G / T are built once per
//                 word; any other target byte (N, lower case, ...) scans the word's query bytes -- every comparison is byte-exact.
//   affine costs  edit_distance_affine_gap (:103-196): Gotoh restated operation by operation in f32 (no multiply in the recurrence, no
//                 fast-math: the sums are the reference's).  One wave per job, lane = query row, anti-diagonal sweep: at step s lane i
//                 computes column s - i from its own previous column, the value lane i-1 handed over (__shfl_up) and the one it handed
//                 over a step earlier (the diagonal).  Queries longer than 64 rows run in strips; the last row of a strip is kept for the
//                 first lane of the next one, in LDS when it fits (targets up to 5 460 bytes), else in a global scratch row of the wave.
//   long jobs     only jobs whose query is longer than 64 need a scratch row (Myers carry, Gotoh strip boundary).  They run in a launch of
//                 their own, whose rows are sized by their longest allele window and whose grid is capped by the scratch budget; the
//                 launch over all other jobs needs no scratch at all.  The shape of that launch is long_shape() of realign_shape.h: affine,
//                 four waves per workgroup with one LDS row each while the longest window is at most 1 364 bytes, one wave with one LDS
//                 row up to 5 460 (65 532 bytes), one wave with a global row beyond; unit, 64 lanes with 2 ceil(window / 64) carry words each.
//   decision      realign (variants.py:866-891): distances of the allowed alleles in index order, stable order by distance, the first
//                 allele iff it is alone or strictly best; quality 30 (unit) or d0 - d1 / d0 (affine).
// Only the per-job result (allele or -1, and the quality in affine mode) goes back to the host.
// Both host drivers at the end lay their arrays out as one image (call_image.h: typed pieces, one upload) and run through the steps of
// Session (device_runtime.h: stage, upload, kernels_done, fetch, finish); the raw distance batch keeps its result piece inside the image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "device_runtime.h"
#include "realign.h"
#include "realign_shape.h"

namespace whamd {
namespace {

// ---------------------------------------------------------------------------------------------- unit cost: Myers / Hyyro
constexpr uint64_t WORD_ONES = ~0ull;

template <class Q, class T>
__device__ __forceinline__ uint64_t match_scan(const Q& q, uint32_t q0, uint32_t rows, uint8_t c) {
	uint64_t eq = 0;
	for (uint32_t r = 0; r < rows; ++r) eq |= (uint64_t)(q(q0 + r) == c) << r;
	return eq;
}

// Levenshtein distance of q[qb, qb + m) and t[tb, tb + n); carry: 2 * ceil(n / 64) words of this lane (used when m > 64 after stripping)
template <class Q, class T>
__device__ int64_t unit_distance(const Q& q, uint32_t qb, uint32_t m, const T& t, uint32_t tb, uint32_t n, uint64_t* carry) {
	while (m > 0 && n > 0 && q(qb) == t(tb)) { ++qb; ++tb; --m; --n; }
	while (m > 0 && n > 0 && q(qb + m - 1) == t(tb + n - 1)) { --m; --n; }
	if (m == 0) return n;
	if (n == 0) return m;
	int64_t score = m;
	const uint32_t words = (m + 63) / 64;
	for (uint32_t w = 0; w < words; ++w) {
		const uint32_t q0 = qb + 64 * w, rows = min(64u, m - 64 * w);
		uint64_t pa = 0, pc = 0, pg = 0, pt = 0;
		for (uint32_t r = 0; r < rows; ++r) {
			const uint8_t c = q(q0 + r);
			const uint64_t bit = 1ull << r;
			pa |= c == 'A' ? bit : 0;
			pc |= c == 'C' ? bit : 0;
			pg |= c == 'G' ? bit : 0;
			pt |= c == 'T' ? bit : 0;
		}
		const uint64_t high = 1ull << (rows - 1);
		const bool last_word = w + 1 == words;
		uint64_t pv = WORD_ONES, mv = 0, in_p = 0, in_m = 0, out_p = 0, out_m = 0;
		for (uint32_t j = 0; j < n; ++j) {
			const uint32_t bit = j & 63;
			if (w > 0 && bit == 0) { in_p = carry[2 * (j >> 6)]; in_m = carry[2 * (j >> 6) + 1]; }
			const int hin = w == 0 ? 1 : ((in_p >> bit) & 1) ? 1 : ((in_m >> bit) & 1) ? -1 : 0;   // row 0 of the matrix: D[0][j] = j
			const uint8_t c = t(tb + j);
			uint64_t eq = c == 'A' ? pa : c == 'C' ? pc : c == 'G' ? pg : c == 'T' ? pt : match_scan<Q, T>(q, q0, rows, c);
			const uint64_t xv = eq | mv;
			if (hin < 0) eq |= 1;
			const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
			uint64_t ph = mv | ~(xh | pv);
			uint64_t mh = pv & xh;
			const int hout = (ph & high) ? 1 : (mh & high) ? -1 : 0;
			ph <<= 1;
			mh <<= 1;
			if (hin < 0) mh |= 1;
			else if (hin > 0) ph |= 1;
			pv = mh | ~(xv | ph);
			mv = ph & xv;
			if (last_word) {
				score += hout;
			} else {
				out_p |= (uint64_t)(hout > 0) << bit;
				out_m |= (uint64_t)(hout < 0) << bit;
				if (bit == 63 || j + 1 == n) { carry[2 * (j >> 6)] = out_p; carry[2 * (j >> 6) + 1] = out_m; out_p = out_m = 0; }
			}
		}
	}
	return score;
}

// ---------------------------------------------------------------------------------------------- affine cost: Gotoh, one wave
__device__ __forceinline__ float min2(float x, float y) { return y < x ? y : x; }
__device__ __forceinline__ float min3(float x, float y, float z) { return min2(min2(x, y), z); }

// edit_distance_affine_gap(q[qb, qb + m), t[tb, tb + n), cost, gap_start, gap_extend); cost(k) = mismatch_cost[k] of the unstripped query.
// Every lane of the wave calls it with the same arguments; bnd: 3 (n + 1) floats of this wave, in LDS or global memory (strips of more than 64 rows).
template <class Q, class T, class C>
__device__ int64_t affine_distance(const Q& q, uint32_t qb, uint32_t m, const T& t, uint32_t tb, uint32_t n, const C& cost, int32_t gs,
                                   int32_t ge, float* bnd, bool global_row) {
	const uint32_t lane = threadIdx.x & 63;
	uint32_t len_p = 0;
	while (m > 0 && n > 0 && q(qb + len_p) == t(tb + len_p)) { ++len_p; --m; --n; }
	while (m > 0 && n > 0 && q(qb + len_p + m - 1) == t(tb + len_p + n - 1)) { --m; --n; }
	if (m == 0 && n == 0) return 0;
	if (m == 0 || n == 0) return (int64_t)min2(affine_gap_f(m ? m : n, gs, ge), AFFINE_INF);   // min(INT_MAX, f(len), INT_MAX)
	const float fgs = (float)gs, fge = (float)ge;
	float result = 0.0f;
	for (uint32_t s0 = 0; s0 < m; s0 += 64) {
		const uint32_t rows = min(64u, m - s0);
		const uint32_t i = s0 + lane + 1;   // this lane's row
		const bool active = lane < rows;
		const bool last_strip = s0 + 64 >= m;
		const uint8_t qc = active ? q(qb + len_p + i - 1) : 0;
		const float mc = active ? cost(len_p + i - 1) : 0.0f;
		float ca = AFFINE_INF, cb = affine_gap_f(i, gs, ge), cc = AFFINE_INF;   // row i, column 0
		float ua = 0.0f, ub = 0.0f, uc = 0.0f;                                  // row i - 1, one column to the left (the diagonal)
		for (uint32_t step = 0; step < n + rows; ++step) {
			float na = __shfl_up(ca, 1, 64), nb = __shfl_up(cb, 1, 64), nc = __shfl_up(cc, 1, 64);   // row i - 1, this step's column
			const int j = (int)step - (int)lane;
			if (lane == 0 && j >= 0 && j <= (int)n) {
				if (s0 == 0) {
					if (j == 0) { na = 0.0f; nb = 0.0f; nc = 0.0f; }
					else { na = AFFINE_INF; nb = AFFINE_INF; nc = affine_gap_f(j, gs, ge); }
				} else {
					na = bnd[3 * j]; nb = bnd[3 * j + 1]; nc = bnd[3 * j + 2];
				}
			}
			if (active && j >= 1 && j <= (int)n) {
				const float m_c = qc == t(tb + len_p + j - 1) ? 0.0f : mc;
				const float c_a = min3(ua, ub, uc) + m_c;
				const float c_b = min3(na + fgs, nb + fge, nc + fgs);
				const float c_c = min3(ca + fgs, cb + fgs, cc + fge);
				ca = c_a;
				cb = c_b;
				cc = c_c;
			}
			ua = na;
			ub = nb;
			uc = nc;
			if (!last_strip && lane == 63 && j >= 0 && j <= (int)n) { bnd[3 * j] = ca; bnd[3 * j + 1] = cb; bnd[3 * j + 2] = cc; }
		}
		// the next strip's lane 0 reads what lane 63 wrote: in LDS that is program order, in a global scratch row the stores must be complete and
		// no earlier load of the row may be served from a cache line read before them (only between strips: one-strip queries pay nothing)
		if (!last_strip) {
			if (global_row) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
			else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
		}
		__builtin_amdgcn_wave_barrier();
		if (last_strip) result = __shfl(min3(ca, cb, cc), rows - 1, 64);
	}
	return (int64_t)result;   // int(...): toward zero
}

// ---------------------------------------------------------------------------------------------- realign: distances + decision
struct RealignArgs {
	const RealignJob* jobs;
	const RealignVariant* vars;
	const uint32_t* allow;
	const uint64_t* alt_off;
	const uint8_t* alt_bytes;
	const uint8_t* ref;
	const uint8_t* qbuf;
	const uint32_t* subset;    // the jobs of this launch (NULL: 0 .. n_items - 1)
	uint32_t n_items;
	uint32_t skip_long;        // 1: leave jobs with a query longer than 64 to the launch over `subset`
	uint64_t* carry;           // unit: carry_words per lane
	float* bnd;                // affine: rows_floats per wave in global memory, or NULL (rows in LDS)
	uint32_t carry_words, row_floats;
	int32_t gap_start, gap_extend;
	float mismatch;
	int32_t* allele_out;
	int64_t* quality_out;
};

struct BytesAt {
	const uint8_t* p;
	__device__ uint8_t operator()(uint32_t k) const { return p[k]; }
};
struct TargetAt {
	Target t;
	__device__ uint8_t operator()(uint32_t k) const { return t.at(k); }
};
struct ConstCost {
	float c;
	__device__ float operator()(uint32_t) const { return c; }
};
struct CostAt {
	const float* p;
	__device__ float operator()(uint32_t k) const { return p[k]; }
};

// the strip boundary row of wave `wave` of this block
__device__ __forceinline__ float* boundary_row(float* global_rows, uint32_t row_floats, float* lds) {
	const uint32_t wave = threadIdx.x >> 6;
	if (global_rows) return global_rows + ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * row_floats;
	return lds + (size_t)wave * row_floats;
}

__global__ void __launch_bounds__(256) realign_unit_kernel(RealignArgs a) {
	const uint32_t stride = gridDim.x * blockDim.x, tid = blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t* carry = a.carry ? a.carry + (uint64_t)tid * a.carry_words : nullptr;
	for (uint32_t k = tid; k < a.n_items; k += stride) {
		const uint32_t x = a.subset ? a.subset[k] : k;
		const RealignJob job = a.jobs[x];
		if (a.skip_long && job.q_len > 64) continue;
		const RealignVariant v = a.vars[job.variant];
		const BytesAt q{a.qbuf + job.q_off};
		int64_t d0 = INT64_MAX, d1 = INT64_MAX;
		int32_t best = -1;
		for (uint32_t i = 0; i < v.allow_n; ++i) {
			const uint32_t allele = a.allow[v.allow_off + i];
			const TargetAt t{allele_target(job, v, allele, a.ref, a.alt_off, a.alt_bytes)};
			const int64_t d = unit_distance(q, 0, job.q_len, t, 0, t.t.len(), carry);
			if (d < d0) { d1 = d0; d0 = d; best = (int32_t)allele; }
			else if (d < d1) d1 = d;
		}
		a.allele_out[x] = (v.allow_n == 1 || d0 < d1) ? best : -1;
	}
}

__global__ void __launch_bounds__(256) realign_affine_kernel(RealignArgs a) {
	extern __shared__ float lds[];
	const uint32_t waves = blockDim.x >> 6, lane = threadIdx.x & 63;
	float* bnd = boundary_row(a.bnd, a.row_floats, lds);
	for (uint32_t k = blockIdx.x * waves + (threadIdx.x >> 6); k < a.n_items; k += gridDim.x * waves) {
		const uint32_t x = a.subset ? a.subset[k] : k;
		const RealignJob job = a.jobs[x];
		if (a.skip_long && job.q_len > 64) continue;
		const RealignVariant v = a.vars[job.variant];
		const BytesAt q{a.qbuf + job.q_off};
		int64_t d0 = INT64_MAX, d1 = INT64_MAX;
		int32_t best = -1;
		for (uint32_t i = 0; i < v.allow_n; ++i) {
			const uint32_t allele = a.allow[v.allow_off + i];
			const TargetAt t{allele_target(job, v, allele, a.ref, a.alt_off, a.alt_bytes)};
			const int64_t d = affine_distance(q, 0, job.q_len, t, 0, t.t.len(), ConstCost{a.mismatch}, a.gap_start, a.gap_extend, bnd, a.bnd != nullptr);
			if (d < d0) { d1 = d0; d0 = d; best = (int32_t)allele; }
			else if (d < d1) d1 = d;
		}
		if (lane == 0) {
			a.allele_out[x] = (v.allow_n == 1 || d0 < d1) ? best : -1;
			a.quality_out[x] = v.allow_n > 1 ? d0 - d1 : d0;
		}
	}
}

// ---------------------------------------------------------------------------------------------- raw distance batch
struct PairArgs {
	const uint64_t* qptr;
	const uint8_t* q;
	const uint64_t* tptr;
	const uint8_t* t;
	const float* cost;
	const uint32_t* subset;
	uint32_t n_items;
	uint32_t skip_long;
	uint64_t* carry;
	float* bnd;
	uint32_t carry_words, row_floats;
	int32_t gap_start, gap_extend;
	int64_t* out;
};

__global__ void __launch_bounds__(256) distance_unit_kernel(PairArgs a) {
	const uint32_t stride = gridDim.x * blockDim.x, tid = blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t* carry = a.carry ? a.carry + (uint64_t)tid * a.carry_words : nullptr;
	for (uint32_t k = tid; k < a.n_items; k += stride) {
		const uint32_t x = a.subset ? a.subset[k] : k;
		const uint64_t q0 = a.qptr[x], t0 = a.tptr[x];
		const uint32_t m = (uint32_t)(a.qptr[x + 1] - q0);
		if (a.skip_long && m > 64) continue;
		a.out[x] = unit_distance(BytesAt{a.q + q0}, 0, m, BytesAt{a.t + t0}, 0, (uint32_t)(a.tptr[x + 1] - t0), carry);
	}
}

__global__ void __launch_bounds__(256) distance_affine_kernel(PairArgs a) {
	extern __shared__ float lds[];
	const uint32_t waves = blockDim.x >> 6, lane = threadIdx.x & 63;
	float* bnd = boundary_row(a.bnd, a.row_floats, lds);
	for (uint32_t k = blockIdx.x * waves + (threadIdx.x >> 6); k < a.n_items; k += gridDim.x * waves) {
		const uint32_t x = a.subset ? a.subset[k] : k;
		const uint64_t q0 = a.qptr[x], t0 = a.tptr[x];
		const uint32_t m = (uint32_t)(a.qptr[x + 1] - q0);
		if (a.skip_long && m > 64) continue;
		const int64_t d = affine_distance(BytesAt{a.q + q0}, 0, m, BytesAt{a.t + t0}, 0, (uint32_t)(a.tptr[x + 1] - t0), CostAt{a.cost + q0},
		                                  a.gap_start, a.gap_extend, bnd, a.bnd != nullptr);
		if (lane == 0) a.out[x] = d;
	}
}

// ---------------------------------------------------------------------------------------------- host driver
constexpr uint32_t BLOCK = 256, MAX_BLOCKS = 8192;   // (the long jobs' launch: realign_shape.h)

}  // namespace

whamd_status_t realign_device(const RealignBatch& b, int device, int32_t* allele_out, int64_t* quality_out, CallTimes& times, std::string& msg) {
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	const bool affine = b.params.use_affine != 0;
	// one image: jobs | query windows | long jobs | variants | allowed alleles | alt offsets | alt bytes | reference slice
	ImageLayout in;
	const auto p_jobs = in.add<RealignJob>(b.n_jobs);
	const auto p_q = in.add<uint8_t>(b.n_query_bytes);
	const auto p_long = in.add<uint32_t>(b.n_long);
	const auto p_var = in.add<RealignVariant>(b.variants.size());
	const auto p_allow = in.add<uint32_t>(b.allow.size());
	const auto p_alt = in.add<uint64_t>(b.alt_off.size());
	const auto p_altb = in.add<uint8_t>(b.n_alt_bytes);
	const auto p_ref = in.add<uint8_t>(b.ref_len);
	Image im;
	WHAMD_TRY(s.stage(in, im, msg));
	const uint32_t n_ranges = (uint32_t)b.range_jobs.size();
	parallel_ranges(n_ranges + 1, host_threads(n_ranges + 1, 1), [&](uint64_t begin, uint64_t end, uint32_t) {
		for (uint64_t r = begin; r < end; ++r) {
			if (r == n_ranges) {   // the small tables and the reference slice
				if (!b.variants.empty()) std::memcpy(im.host(p_var), b.variants.data(), p_var.bytes());
				if (!b.allow.empty()) std::memcpy(im.host(p_allow), b.allow.data(), p_allow.bytes());
				std::memcpy(im.host(p_alt), b.alt_off.data(), p_alt.bytes());
				if (b.n_alt_bytes) std::memcpy(im.host(p_altb), b.alt_bytes, b.n_alt_bytes);
				if (b.ref_len) std::memcpy(im.host(p_ref), b.ref, b.ref_len);
				continue;
			}
			RealignJob* dst = im.host(p_jobs) + b.range_job_base[r];
			const uint64_t qbase = b.range_query_base[r];
			for (const RealignJob& j : b.range_jobs[r]) {
				RealignJob k = j;
				k.q_off += qbase;
				*dst++ = k;
			}
			if (!b.range_query[r].empty()) std::memcpy(im.host(p_q) + qbase, b.range_query[r].data(), b.range_query[r].size());
			uint32_t* ldst = im.host(p_long) + b.range_long_base[r];
			for (uint32_t x : b.range_long[r]) *ldst++ = (uint32_t)(b.range_job_base[r] + x);
		}
	});
	// the results, a second image that only comes down: alleles | qualities
	ImageLayout out;
	const auto p_allele = out.add<int32_t>(b.n_jobs);
	const auto p_quality = out.add<int64_t>(affine ? b.n_jobs : 0);
	Image res;
	WHAMD_TRY(s.stage(out, res, msg));
	RealignArgs a{};
	a.jobs = im.dev(p_jobs);
	a.qbuf = im.dev(p_q);
	a.vars = im.dev(p_var);
	a.allow = im.dev(p_allow);
	a.alt_off = im.dev(p_alt);
	a.alt_bytes = im.dev(p_altb);
	a.ref = im.dev(p_ref);
	a.gap_start = b.params.gap_start;
	a.gap_extend = b.params.gap_extend;
	a.mismatch = b.params.default_mismatch;
	a.allele_out = res.dev_out(p_allele);
	a.quality_out = affine ? res.dev_out(p_quality) : nullptr;
	// the launch over every job with a query of at most 64 (no scratch), then the one over the long jobs
	RealignArgs shortj = a;
	shortj.n_items = (uint32_t)b.n_jobs;
	shortj.skip_long = b.n_long > 0;
	const dim3 short_blocks(grid_for(b.n_jobs, affine ? BLOCK / 64 : BLOCK, MAX_BLOCKS));
	RealignArgs longj = a;
	const LongShape ls = long_shape(affine, b.n_long, b.max_target_long);
	if (b.n_long) {
		longj.subset = im.dev(p_long);
		longj.n_items = (uint32_t)b.n_long;
		longj.carry_words = ls.carry_words;
		longj.row_floats = ls.row_floats;
		if (ls.scratch) {
			void* c = nullptr;
			WHAMD_TRY(s.device_block(ls.scratch, &c, msg));
			if (affine) longj.bnd = (float*)c;
			else longj.carry = (uint64_t*)c;
		}
	}
	WHAMD_TRY(s.upload(im, msg));
	const auto kernel = affine ? realign_affine_kernel : realign_unit_kernel;
	WHAMD_TRY(launch(s, times, msg, kernel, short_blocks, dim3(BLOCK), 0, shortj));
	if (b.n_long) WHAMD_TRY(launch(s, times, msg, kernel, dim3(ls.blocks), dim3(ls.block), ls.lds, longj));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res.stage, res.base, p_quality.end(), msg));   // (to the last byte in use)
	WHAMD_TRY(s.finish(times, msg));
	std::memcpy(allele_out, res.host(p_allele), p_allele.bytes());
	if (affine) std::memcpy(quality_out, res.host(p_quality), p_quality.bytes());
	return WHAMD_OK;
}

whamd_status_t edit_distance_device(uint64_t n_pairs, const uint64_t* query_ptr, const uint8_t* query, const uint64_t* target_ptr,
                                    const uint8_t* target, int use_affine, const float* mismatch_cost, int32_t gap_start, int32_t gap_extend,
                                    int device, int64_t* distance_out, std::string& msg) {
	if (n_pairs >= UINT32_MAX) { msg = "too many pairs for one call"; return WHAMD_ERR_INVALID; }
	for (uint64_t p = 0; p < n_pairs; ++p) {
		if (query_ptr[p + 1] < query_ptr[p] || target_ptr[p + 1] < target_ptr[p]) { msg = "query_ptr / target_ptr must not decrease"; return WHAMD_ERR_INVALID; }
		if (target_ptr[p + 1] - target_ptr[p] >= UINT32_MAX || query_ptr[p + 1] - query_ptr[p] >= UINT32_MAX) { msg = "sequence too long"; return WHAMD_ERR_INVALID; }
	}
	std::vector<uint32_t> long_pairs;
	const uint32_t max_t_long = long_pairs_of(n_pairs, query_ptr, target_ptr, long_pairs);
	Session s;
	WHAMD_TRY(s.open(device, 0, msg));   // (no events: the call reports no times)
	const uint64_t nq = query_ptr[n_pairs], nt = target_ptr[n_pairs], n_long = long_pairs.size();
	// one image: query offsets | target offsets | queries | targets | mismatch costs | long pairs | the distances (written by the kernels: not uploaded)
	ImageLayout in;
	const auto p_qp = in.add<uint64_t>(n_pairs + 1);
	const auto p_tp = in.add<uint64_t>(n_pairs + 1);
	const auto p_q = in.add<uint8_t>(nq);
	const auto p_t = in.add<uint8_t>(nt);
	const auto p_c = in.add<float>(use_affine ? nq : 0);
	const auto p_long = in.add<uint32_t>(n_long);
	const auto p_out = in.add<int64_t>(n_pairs);
	Image im;
	WHAMD_TRY(s.stage(in, im, msg));
	std::memcpy(im.host(p_qp), query_ptr, p_qp.bytes());
	std::memcpy(im.host(p_tp), target_ptr, p_tp.bytes());
	if (nq) std::memcpy(im.host(p_q), query, nq);
	if (nt) std::memcpy(im.host(p_t), target, nt);
	if (use_affine && nq) std::memcpy(im.host(p_c), mismatch_cost, p_c.bytes());
	if (n_long) std::memcpy(im.host(p_long), long_pairs.data(), p_long.bytes());
	PairArgs a{};
	a.qptr = im.dev(p_qp);
	a.tptr = im.dev(p_tp);
	a.q = im.dev(p_q);
	a.t = im.dev(p_t);
	a.cost = im.dev(p_c);
	a.gap_start = gap_start;
	a.gap_extend = gap_extend;
	a.out = im.dev_out(p_out);
	PairArgs shortp = a;
	shortp.n_items = (uint32_t)n_pairs;
	shortp.skip_long = n_long > 0;
	const dim3 short_blocks(grid_for(n_pairs, use_affine ? BLOCK / 64 : BLOCK, MAX_BLOCKS));
	PairArgs longp = a;
	const LongShape ls = long_shape(use_affine != 0, n_long, max_t_long);
	if (n_long) {
		longp.subset = im.dev(p_long);
		longp.n_items = (uint32_t)n_long;
		longp.carry_words = ls.carry_words;
		longp.row_floats = ls.row_floats;
		if (ls.scratch) {
			void* c = nullptr;
			WHAMD_TRY(s.device_block(ls.scratch, &c, msg));
			if (use_affine) longp.bnd = (float*)c;
			else longp.carry = (uint64_t*)c;
		}
	}
	WHAMD_TRY(s.upload(im, p_out.offset, msg));
	CallTimes unused;
	const auto kernel = use_affine ? distance_affine_kernel : distance_unit_kernel;
	WHAMD_TRY(launch(s, unused, msg, kernel, short_blocks, dim3(BLOCK), 0, shortp));
	if (n_long) WHAMD_TRY(launch(s, unused, msg, kernel, dim3(ls.blocks), dim3(ls.block), ls.lds, longp));
	WHAMD_TRY(s.fetch(im.host(p_out), im.dev(p_out), p_out.bytes(), msg));
	WHAMD_TRY(s.finish(unused, msg));
	std::memcpy(distance_out, im.host(p_out), p_out.bytes());
	return WHAMD_OK;
}

}  // namespace whamd
