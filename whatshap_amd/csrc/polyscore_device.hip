// polyscore_device.hip -- the pair loop of polyphase read scoring on gfx950 (polyscore.h).  A batch of matrices is one upload and one
// launch sequence:
//   1. poly_pair_kernel: one lane per candidate pair, from a flattened pair index (prefix sum of the window sizes over the anchors of every
//      matrix, so uneven windows cost nothing extra).  The lane finds its anchor by binary search, skips the anchor's entries before the
//      partner's first position (binary search), then merges the two sorted rows and adds the float terms in double in position order --
//      poly_pair_sum, the same code as the host loop, so the result is bit-identical to it.  Rows are read from global memory: any span
//      works, there is no LDS budget to fall back from.  It writes score[p] and keep[p] and counts overlapping / NaN pairs per matrix.
//   2. rocprim exclusive scan of keep (deterministic compaction).
//   3. poly_compact_kernel: kept pairs -> (key, score), key = max(id) * N + min(id) over global read ids: the triangular order per matrix.
//   4. rocprim radix sort of (key, score) on the bits the keys use.
// Only the sorted (key, score) pairs come back.  The upload is one image (call_image.h); the steps are Session's (device_runtime.h), with one
// its one wait (fetch_now) after step 2: the number of kept pairs sizes steps 3 and 4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "device_runtime.h"
#include "polyscore.h"

namespace whamd {
namespace {

constexpr uint32_t BLOCK = 256, MAX_BLOCKS = 16384;

struct PairArgs {
	uint64_t n_pairs;
	uint32_t n_anchors;              // every read of every uploaded matrix (global anchor index = read_base[m] + k)
	const uint64_t* pair_prefix;     // [n_anchors + 1]
	const uint32_t* order;           // [n_anchors] global read id of the k-th read of its matrix by first position
	const uint64_t* row_ptr;         // [n_anchors + 1] by global read id
	const uint32_t* row_pos;
	const uint8_t* row_allele;
	const uint32_t* anchor_mat;      // [n_anchors] matrix of the anchor
	const uint64_t* mat_term_off;    // per matrix: first term
	const uint32_t* mat_alleles;     // per matrix: max_allele
	const float* terms;
	uint32_t min_overlap;
	float offset;
	float* score;                    // [n_pairs]
	uint32_t* keep;                  // [n_pairs]
	unsigned long long* counts;      // [3 * n_mats]: overlapping, NaN, shared positions
};

__device__ inline uint32_t anchor_of(const uint64_t* prefix, uint32_t n, uint64_t p) {
	uint32_t lo = 0, hi = n;   // last a with prefix[a] <= p
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (prefix[mid] <= p) lo = mid;
		else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(BLOCK) poly_pair_kernel(PairArgs a) {
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t base = (uint64_t)blockIdx.x * BLOCK; base < a.n_pairs; base += stride) {
		const uint64_t p = base + threadIdx.x;
		const bool live = p < a.n_pairs;
		uint32_t mat = 0xffffffffu, ov = 0;
		bool over = false, nan = false;
		if (live) {
			const uint32_t k = anchor_of(a.pair_prefix, a.n_anchors, p);
			const uint32_t q = k + 1 + (uint32_t)(p - a.pair_prefix[k]);
			const uint32_t ra = a.order[k], rb = a.order[q];
			mat = a.anchor_mat[k];
			const uint64_t a0 = a.row_ptr[ra], a1 = a.row_ptr[ra + 1], b0 = a.row_ptr[rb], b1 = a.row_ptr[rb + 1];
			double sum = 0.0;
			ov = poly_pair_sum(a.row_pos + a0, a.row_allele + a0, a1 - a0, a.row_pos + b0, a.row_allele + b0, b1 - b0,
			                                  a.terms + a.mat_term_off[mat], a.mat_alleles[mat], &sum);
			uint32_t keep = 0;
			float out = 0.0f;
			if (ov >= a.min_overlap) {
				over = true;
				const float s = (float)sum;
				if (s != s) nan = true;
				else if (s != 0.0f) { keep = 1; out = s + a.offset; }
			}
			a.score[p] = out;
			a.keep[p] = keep;
		}
		// per-matrix counts: one atomic per wave when the whole wave is in one matrix (the usual case), else one per lane
		const uint32_t m0 = __shfl(mat, 0);
		const bool uniform = __all(!live || mat == m0);
		const uint64_t over_mask = __ballot(over), nan_mask = __ballot(nan);
		if (uniform) {
			unsigned long long ov_sum = ov;
			for (int d = 32; d >= 1; d >>= 1) ov_sum += __shfl_xor(ov_sum, d);
			if ((threadIdx.x & 63) == 0 && m0 != 0xffffffffu) {
				if (over_mask) atomicAdd(&a.counts[3 * m0], (unsigned long long)__popcll(over_mask));
				if (nan_mask) atomicAdd(&a.counts[3 * m0 + 1], (unsigned long long)__popcll(nan_mask));
				if (ov_sum) atomicAdd(&a.counts[3 * m0 + 2], ov_sum);
			}
		} else if (live) {
			if (over) atomicAdd(&a.counts[3 * mat], 1ull);
			if (nan) atomicAdd(&a.counts[3 * mat + 1], 1ull);
			if (ov) atomicAdd(&a.counts[3 * mat + 2], (unsigned long long)ov);
		}
	}
}

struct CompactArgs {
	uint64_t n_pairs;
	uint32_t n_anchors;
	const uint64_t* pair_prefix;
	const uint32_t* order;
	const float* score;
	const uint32_t* keep;
	const uint32_t* slot;            // exclusive scan of keep
	uint64_t* key;
	float* value;
};

__global__ void __launch_bounds__(BLOCK) poly_compact_kernel(CompactArgs a) {
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < a.n_pairs; p += stride) {
		if (!a.keep[p]) continue;
		const uint32_t k = anchor_of(a.pair_prefix, a.n_anchors, p);
		const uint32_t q = k + 1 + (uint32_t)(p - a.pair_prefix[k]);
		const uint32_t ra = a.order[k], rb = a.order[q];
		const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
		const uint32_t s = a.slot[p];
		a.key[s] = (uint64_t)hi * a.n_anchors + lo;
		a.value[s] = a.score[p];
	}
}

}  // namespace

whamd_status_t poly_score_device(const std::vector<PolyMatrix>& ms, uint32_t min_overlap, float offset, int device, std::vector<PolyResult>& out,
                                 CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(ms.size(), PolyResult{});
	// the matrices with candidate pairs, concatenated
	std::vector<uint32_t> up;
	uint64_t n_reads = 0, n_entries = 0, n_terms = 0, n_pairs = 0;
	for (uint32_t x = 0; x < ms.size(); x++) {
		if (!ms[x].n_candidates) continue;
		up.push_back(x);
		n_reads += ms[x].n_reads;
		n_entries += ms[x].row_pos.size();
		n_terms += ms[x].terms.size();
		n_pairs += ms[x].n_candidates;
	}
	if (!n_pairs) return WHAMD_OK;   // nothing to score: no device work at all
	if (n_pairs >= UINT32_MAX || n_reads >= UINT32_MAX) {
		msg = "more than 2^32 - 1 candidate pairs or reads in one call: split the batch";
		return WHAMD_ERR_UNSUPPORTED;
	}
	const uint32_t n_mats = (uint32_t)up.size(), N = (uint32_t)n_reads;
	// the image (one upload)
	ImageLayout in;
	const auto p_prefix = in.add<uint64_t>(N + 1);
	const auto p_order = in.add<uint32_t>(N);
	const auto p_rowptr = in.add<uint64_t>(N + 1);
	const auto p_pos = in.add<uint32_t>(n_entries);
	const auto p_all = in.add<uint8_t>(n_entries);
	const auto p_amat = in.add<uint32_t>(N);
	const auto p_toff = in.add<uint64_t>(n_mats);
	const auto p_na = in.add<uint32_t>(n_mats);
	const auto p_terms = in.add<float>(n_terms);
	const auto p_counts = in.add<unsigned long long>(3 * (size_t)n_mats);   // zeros; the pair kernel adds to them
	ImageLayout tail_layout;   // what comes down in the middle of the call
	const auto t_last = tail_layout.add<uint32_t>(2);   // keep and slot of the last pair
	const auto t_counts = tail_layout.add<unsigned long long>(p_counts.count);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im;
	WHAMD_TRY(s.stage(in, im, msg));
	std::vector<uint64_t> read_base(n_mats + 1, 0), entry_base(n_mats + 1, 0), term_base(n_mats + 1, 0), pair_base(n_mats + 1, 0);
	for (uint32_t u = 0; u < n_mats; u++) {
		const PolyMatrix& m = ms[up[u]];
		read_base[u + 1] = read_base[u] + m.n_reads;
		entry_base[u + 1] = entry_base[u] + m.row_pos.size();
		term_base[u + 1] = term_base[u] + m.terms.size();
		pair_base[u + 1] = pair_base[u] + m.n_candidates;
	}
	parallel_ranges(n_mats, std::min<uint32_t>(host_threads(n_reads, 1 << 15), n_mats), [&](uint64_t b, uint64_t e, uint32_t) {
		for (uint64_t u = b; u < e; u++) {
			const PolyMatrix& m = ms[up[u]];
			const uint64_t rb = read_base[u], eb = entry_base[u];
			uint64_t* prefix = im.host(p_prefix) + rb;
			uint32_t* order = im.host(p_order) + rb;
			uint64_t* rowptr = im.host(p_rowptr) + rb;
			uint32_t* amat = im.host(p_amat) + rb;
			uint64_t acc = pair_base[u];
			for (uint32_t k = 0; k < m.n_reads; k++) {
				prefix[k] = acc;
				acc += m.window_end[k] - (k + 1);
				order[k] = (uint32_t)(rb + m.order[k]);
				rowptr[k] = eb + m.row_ptr[k];
				amat[k] = (uint32_t)u;
			}
			if (!m.row_pos.empty()) {
				std::memcpy(im.host(p_pos) + eb, m.row_pos.data(), m.row_pos.size() * 4);
				std::memcpy(im.host(p_all) + eb, m.row_allele.data(), m.row_allele.size());
			}
			std::memcpy(im.host(p_terms) + term_base[u], m.terms.data(), m.terms.size() * 4);
			im.host(p_toff)[u] = term_base[u];
			im.host(p_na)[u] = m.max_allele;
		}
	});
	im.host(p_prefix)[N] = n_pairs;
	im.host(p_rowptr)[N] = n_entries;
	std::memset(im.host(p_counts), 0, p_counts.bytes());
	// pair buffers
	float* score = nullptr;
	uint32_t *keep = nullptr, *slot = nullptr;
	WHAMD_TRY(s.device_block(n_pairs * 4, (void**)&score, msg));
	WHAMD_TRY(s.device_block(n_pairs * 4, (void**)&keep, msg));
	WHAMD_TRY(s.device_block(n_pairs * 4, (void**)&slot, msg));
	size_t scan_tmp = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, scan_tmp, keep, slot, 0u, (size_t)n_pairs, rocprim::plus<uint32_t>(), s.stream));
	void* scan_buf = nullptr;
	WHAMD_TRY(s.device_block(scan_tmp, &scan_buf, msg));
	Image tail;
	WHAMD_TRY(s.results(tail_layout, tail, msg));

	PairArgs pa{};
	pa.n_pairs = n_pairs;
	pa.n_anchors = N;
	pa.pair_prefix = im.dev(p_prefix);
	pa.order = im.dev(p_order);
	pa.row_ptr = im.dev(p_rowptr);
	pa.row_pos = im.dev(p_pos);
	pa.row_allele = im.dev(p_all);
	pa.anchor_mat = im.dev(p_amat);
	pa.mat_term_off = im.dev(p_toff);
	pa.mat_alleles = im.dev(p_na);
	pa.terms = im.dev(p_terms);
	pa.min_overlap = min_overlap;
	pa.offset = offset;
	pa.score = score;
	pa.keep = keep;
	pa.counts = im.dev_out(p_counts);
	const dim3 blocks(grid_for(n_pairs, BLOCK, MAX_BLOCKS));

	WHAMD_TRY(s.upload(im, msg));
	WHAMD_TRY(launch(s, times, msg, poly_pair_kernel, blocks, dim3(BLOCK), 0, pa));
	HIP_TRY(rocprim::exclusive_scan(scan_buf, scan_tmp, keep, slot, 0u, (size_t)n_pairs, rocprim::plus<uint32_t>(), s.stream));
	++times.launches;
	// the number of kept pairs sizes what follows: three small results come down in the middle of the kernel phase
	WHAMD_TRY(s.fetch(tail.host(t_last), keep + (n_pairs - 1), 4, msg));
	WHAMD_TRY(s.fetch(tail.host(t_last) + 1, slot + (n_pairs - 1), 4, msg));
	WHAMD_TRY(s.fetch_now(tail, t_counts, im.dev(p_counts), msg));
	const uint64_t n_kept = (uint64_t)tail.host(t_last)[0] + tail.host(t_last)[1];
	const unsigned long long* counts = tail.host(t_counts);
	for (uint32_t u = 0; u < n_mats; u++) {
		out[up[u]].n_overlapping = counts[3 * u];
		out[up[u]].n_nan = counts[3 * u + 1];
		out[up[u]].n_pair_positions = counts[3 * u + 2];
	}
	if (n_kept) {
		uint64_t *key = nullptr, *key2 = nullptr;
		float *val = nullptr, *val2 = nullptr;
		WHAMD_TRY(s.device_block(n_kept * 8, (void**)&key, msg));
		WHAMD_TRY(s.device_block(n_kept * 8, (void**)&key2, msg));
		WHAMD_TRY(s.device_block(n_kept * 4, (void**)&val, msg));
		WHAMD_TRY(s.device_block(n_kept * 4, (void**)&val2, msg));
		unsigned end_bit = 1;
		const uint64_t max_key = (uint64_t)N * N;
		while (end_bit < 64 && (max_key >> end_bit)) ++end_bit;
		size_t sort_tmp = 0;
		HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_tmp, key, key2, val, val2, (size_t)n_kept, 0u, end_bit, s.stream));
		void* sort_buf = nullptr;
		WHAMD_TRY(s.device_block(sort_tmp, &sort_buf, msg));
		ImageLayout sorted;   // the second result image: sized by the wait
		const auto r_key = sorted.add<uint64_t>(n_kept);
		const auto r_val = sorted.add<float>(n_kept);
		Image res;
		WHAMD_TRY(s.results(sorted, res, msg));
		CompactArgs ca{n_pairs, N, pa.pair_prefix, pa.order, score, keep, slot, key, val};
		WHAMD_TRY(launch(s, times, msg, poly_compact_kernel, blocks, dim3(BLOCK), 0, ca));
		HIP_TRY(rocprim::radix_sort_pairs(sort_buf, sort_tmp, key, key2, val, val2, (size_t)n_kept, 0u, end_bit, s.stream));
		++times.launches;
		WHAMD_TRY(s.kernels_done(msg));
		WHAMD_TRY(s.fetch(res, r_key, key2, msg));
		WHAMD_TRY(s.fetch(res, r_val, val2, msg));
		WHAMD_TRY(s.finish(times, msg));
		// per matrix: its keys form one contiguous range (global ids of matrix u are read_base[u] ..)
		const uint64_t* keys = res.host(r_key);
		const float* vals = res.host(r_val);
		std::vector<uint64_t> cut(n_mats + 1);
		for (uint32_t u = 0; u <= n_mats; u++) cut[u] = (uint64_t)(std::lower_bound(keys, keys + n_kept, read_base[u] * N) - keys);
		parallel_ranges(n_mats, std::min<uint32_t>(host_threads(n_kept, 1 << 16), n_mats), [&](uint64_t b, uint64_t e, uint32_t) {
			for (uint64_t u = b; u < e; u++) {
				PolyResult& r = out[up[u]];
				const uint64_t c0 = cut[u], c1 = cut[u + 1], rb = read_base[u];
				r.i.resize(c1 - c0);
				r.j.resize(c1 - c0);
				r.score.resize(c1 - c0);
				for (uint64_t x = c0; x < c1; x++) {
					r.i[x - c0] = (uint32_t)(keys[x] / N - rb);
					r.j[x - c0] = (uint32_t)(keys[x] % N - rb);
					r.score[x - c0] = vals[x];
				}
			}
		});
	} else {   // nothing kept, nothing more to fetch
		WHAMD_TRY(s.kernels_done(msg));
		WHAMD_TRY(s.finish(times, msg, false));
	}
	return WHAMD_OK;
}

}  // namespace whamd
