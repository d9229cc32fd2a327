// progeny_device.hip -- the pair loop of progeny marker scoring on gfx950 (progeny.h).  A batch of problems is one upload, one launch and
// one download:
//   upload    per problem the table repacked to what the lanes read -- genotypes 0 .. 2 only, float, sample-major planes
//             T[(sample * 3 + genotype) * n_nodes + node] (rows beyond n_positions are zeros, as getGl returns there) -- and the entry list
//             (anchor, the partner node whose row is read, score kind) in triangular order, plus one descriptor with the weights.
//   progeny_pair_kernel   one lane per stored entry.  Consecutive entries share the partner hi and walk the anchors hi - s over the reversed
//             stride list, so in the stride-1 part of the window the lanes of a wave read consecutive floats of a plane and the partner's
//             values are one address for the whole wave.  The lane walks the samples in increasing order in double -- progeny_pair_score,
//             the same code as the host twin -- so nothing is reduced across lanes and no sum is reordered.
//   download  one double per entry; the float score is its rounding, taken on the host.
// progeny_types_kernel: one lane per (variant, parental type), samples in order (progeny_type_llh); the argmax is taken on the host.
// Both calls: the upload is one image of typed pieces (call_image.h), the call runs through the steps of Session (device_runtime.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>

#include "device_runtime.h"
#include "progeny.h"

namespace whamd {
namespace {

constexpr uint32_t BLOCK = 256, MAX_BLOCKS = 16384, PACK_NODES = 64;

struct DevProblem {
	uint64_t table_off;              // first float of this problem's planes
	uint32_t n_nodes, n_samples;
	double start;
	double same[3][6], diff[3][6];
};

struct PairArgs {
	uint64_t n_entries;
	uint32_t n_problems;
	const uint64_t* entry_prefix;    // [n_problems + 1]
	const DevProblem* problems;
	const float* table;
	const uint32_t* lo;              // [n_entries] anchor
	const uint32_t* eff;             // [n_entries] partner row
	const uint8_t* kind;             // [n_entries]
	double* score;                   // [n_entries]
};

__device__ inline uint32_t problem_of(const uint64_t* prefix, uint32_t n, uint64_t e) {
	uint32_t lo = 0, hi = n;   // last m with prefix[m] <= e
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (prefix[mid] <= e) lo = mid;
		else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(BLOCK) progeny_pair_kernel(PairArgs a) {
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.n_entries; e += stride) {
		const uint32_t kind = a.kind[e];
		double score = -HUGE_VAL;
		if (kind != PROGENY_KIND_INF) {
			const DevProblem& d = a.problems[problem_of(a.entry_prefix, a.n_problems, e)];
			const float* t = a.table + d.table_off;
			score = progeny_pair_score(t + a.lo[e], t + a.eff[e], 3 * (uint64_t)d.n_nodes, d.n_nodes, d.n_samples, d.same[kind], d.diff[kind],
			                           kind == PROGENY_KIND_SN ? 4 : 6, d.start);
		}
		a.score[e] = score;
	}
}

struct TypesKernelArgs {
	uint64_t n_lanes;                // n * n_types
	uint32_t n_types, n_samples, k1;
	const float* rows;               // [n][n_samples][k1]
	const double* prior;             // [n_types][k1]
	double* llh;                     // [n][n_types]
};

__global__ void __launch_bounds__(BLOCK) progeny_types_kernel(TypesKernelArgs a) {
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; x < a.n_lanes; x += stride) {
		const uint64_t v = x / a.n_types;
		const uint32_t ty = (uint32_t)(x - v * a.n_types);
		a.llh[x] = progeny_type_llh(a.rows + v * a.n_samples * a.k1, a.n_samples, a.k1, a.prior + (uint64_t)ty * a.k1);
	}
}

}  // namespace

whamd_status_t progeny_score_device(const std::vector<ProgenyProblem>& ps, int device, std::vector<ProgenyResult>& out, CallTimes& times,
                                    std::string& msg) {
	times = CallTimes{};
	out.assign(ps.size(), ProgenyResult{});
	// problems with something to compute go up; the others hold -inf entries only (or none) and are filled here
	std::vector<uint32_t> up;
	uint64_t n_entries = 0, n_floats = 0;
	for (uint32_t x = 0; x < ps.size(); x++) {
		const ProgenyProblem& p = ps[x];
		if (p.lo.size() == p.n_inf) {
			out[x].score.assign(p.lo.size(), -std::numeric_limits<double>::infinity());
			continue;
		}
		up.push_back(x);
		n_entries += p.lo.size();
		n_floats += 3 * (uint64_t)p.n_samples * p.n_nodes;
	}
	if (up.empty()) return WHAMD_OK;   // nothing to compute: no device work at all
	const uint32_t n_up = (uint32_t)up.size();
	std::vector<uint64_t> entry_base(n_up + 1, 0), table_base(n_up + 1, 0);
	struct PackJob { uint32_t u; uint64_t node0; };
	std::vector<PackJob> jobs;
	for (uint32_t u = 0; u < n_up; u++) {
		const ProgenyProblem& p = ps[up[u]];
		entry_base[u + 1] = entry_base[u] + p.lo.size();
		table_base[u + 1] = table_base[u] + 3 * (uint64_t)p.n_samples * p.n_nodes;
		if (p.n_samples)
			for (uint64_t node0 = 0; node0 < p.n_nodes; node0 += PACK_NODES) jobs.push_back(PackJob{u, node0});
	}
	// the image (one upload)
	ImageLayout in;
	const auto p_prefix = in.add<uint64_t>(n_up + 1);
	const auto p_desc = in.add<DevProblem>(n_up);
	const auto p_lo = in.add<uint32_t>(n_entries);
	const auto p_eff = in.add<uint32_t>(n_entries);
	const auto p_kind = in.add<uint8_t>(n_entries);
	const auto p_table = in.add<float>(std::max<uint64_t>(n_floats, 1));
	Session s;
	whamd_status_t st = s.open(device, 4, msg);
	if (st != WHAMD_OK) return st;
	Image im;
	double* score = nullptr;
	double* res = nullptr;
	if ((st = s.stage(in, im, msg)) != WHAMD_OK) return st;
	if ((st = s.device_block(n_entries * 8, (void**)&score, msg)) != WHAMD_OK) return st;
	if ((st = s.pinned_block(n_entries * 8, (void**)&res, msg)) != WHAMD_OK) return st;
	for (uint32_t u = 0; u < n_up; u++) {
		const ProgenyProblem& p = ps[up[u]];
		im.host(p_prefix)[u] = entry_base[u];
		DevProblem d{};
		d.table_off = table_base[u];
		d.n_nodes = (uint32_t)p.n_nodes;
		d.n_samples = p.n_samples;
		d.start = p.w.start;
		std::memcpy(d.same, p.w.same, sizeof(d.same));
		std::memcpy(d.diff, p.w.diff, sizeof(d.diff));
		im.host(p_desc)[u] = d;
	}
	im.host(p_prefix)[n_up] = n_entries;
	for (uint32_t u = 0; u < n_up; u++) {
		const ProgenyProblem& p = ps[up[u]];
		progeny_copy(im.host(p_lo) + entry_base[u], p.lo.data(), p.lo.size() * 4);
		progeny_copy(im.host(p_eff) + entry_base[u], p.eff.data(), p.eff.size() * 4);
		progeny_copy(im.host(p_kind) + entry_base[u], p.kind.data(), p.kind.size());
	}
	// the repack: a block of nodes at a time (its rows stay in the host cache while every plane takes its piece)
	parallel_ranges(jobs.size(), host_threads(n_floats, 1 << 18), [&](uint64_t b, uint64_t e, uint32_t) {
		for (uint64_t x = b; x < e; x++) {
			const ProgenyProblem& p = ps[up[jobs[x].u]];
			const uint64_t node0 = jobs[x].node0, node1 = std::min<uint64_t>(node0 + PACK_NODES, p.n_nodes);
			const uint64_t k1 = p.ploidy + 1, row = (uint64_t)p.n_samples * k1;
			float* t = im.host(p_table) + table_base[jobs[x].u];
			const uint64_t have = std::min<uint64_t>(node1, std::max<uint64_t>(p.n_positions, node0));   // nodes [node0, have) have rows
			for (uint64_t sm = 0; sm < p.n_samples; sm++) {
				for (uint32_t g = 0; g < 3; g++) {
					float* dst = t + (sm * 3 + g) * p.n_nodes;
					const float* src = p.gl + sm * k1 + g;
					for (uint64_t node = node0; node < have; node++) dst[node] = src[node * row];
					for (uint64_t node = have; node < node1; node++) dst[node] = 0.0f;
				}
			}
		}
	});

	PairArgs pa{};
	pa.n_entries = n_entries;
	pa.n_problems = n_up;
	pa.entry_prefix = im.dev(p_prefix);
	pa.problems = im.dev(p_desc);
	pa.lo = im.dev(p_lo);
	pa.eff = im.dev(p_eff);
	pa.kind = im.dev(p_kind);
	pa.table = im.dev(p_table);
	pa.score = score;
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_entries + BLOCK - 1) / BLOCK, MAX_BLOCKS);
	if ((st = s.upload(im, msg)) != WHAMD_OK) return st;
	hipLaunchKernelGGL(progeny_pair_kernel, dim3(blocks), dim3(BLOCK), 0, s.stream, pa);
	HIP_TRY(hipGetLastError());
	if ((st = s.kernels_done(msg)) != WHAMD_OK) return st;
	if ((st = s.fetch(res, score, n_entries * 8, msg)) != WHAMD_OK) return st;
	if ((st = s.finish(times, msg)) != WHAMD_OK) return st;
	times.launches = 1;
	for (uint32_t u = 0; u < n_up; u++) {
		RawVec<double>& dst = out[up[u]].score;
		dst.resize(entry_base[u + 1] - entry_base[u]);
		progeny_copy(dst.data(), res + entry_base[u], dst.size() * 8);
	}
	return WHAMD_OK;
}

whamd_status_t progeny_types_device(const float* rows, uint64_t n, uint32_t n_samples, uint32_t k1, const double* prior, int device, double* llh,
                                    std::string& msg) {
	const uint32_t n_types = k1 * (k1 + 1) / 2;
	const uint64_t n_lanes = n * n_types;
	if (!n_lanes) return WHAMD_OK;
	ImageLayout in;
	const auto p_prior = in.add<double>((size_t)n_types * k1);
	const auto p_rows = in.add<float>(n * n_samples * k1);
	Session s;
	whamd_status_t st = s.open(device, 0, msg);   // (no events: the call reports no times)
	if (st != WHAMD_OK) return st;
	Image im;
	double* out = nullptr;
	double* res = nullptr;
	if ((st = s.stage(in, im, msg)) != WHAMD_OK) return st;
	if ((st = s.device_block(n_lanes * 8, (void**)&out, msg)) != WHAMD_OK) return st;
	if ((st = s.pinned_block(n_lanes * 8, (void**)&res, msg)) != WHAMD_OK) return st;
	std::memcpy(im.host(p_prior), prior, p_prior.bytes());
	std::memcpy(im.host(p_rows), rows, p_rows.bytes());
	TypesKernelArgs ta{n_lanes, n_types, n_samples, k1, im.dev(p_rows), im.dev(p_prior), out};
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_lanes + BLOCK - 1) / BLOCK, MAX_BLOCKS);
	if ((st = s.upload(im, msg)) != WHAMD_OK) return st;
	hipLaunchKernelGGL(progeny_types_kernel, dim3(blocks), dim3(BLOCK), 0, s.stream, ta);
	HIP_TRY(hipGetLastError());
	CallTimes unused;
	if ((st = s.fetch(res, out, n_lanes * 8, msg)) != WHAMD_OK) return st;
	if ((st = s.finish(unused, msg)) != WHAMD_OK) return st;
	std::memcpy(llh, res, n_lanes * 8);
	return WHAMD_OK;
}

}  // namespace whamd
