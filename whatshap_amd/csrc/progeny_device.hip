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
// progeny_gl_kernel: the table itself from allele depths (progeny_gl_cell, the same code as the host twin): one lane per (sample, node)
//             cell of a batch.  The depths arrive sample-major, [n_samples][n_rows] uint32, and the nodes of one variant share a row through
//             node_row.  Writing the planes, the node runs fastest within a sample: a wave reads consecutive depth words and writes
//             consecutive floats of each plane T[(sample * 3 + genotype) * n_nodes + node] -- what progeny_pair_kernel reads, so depths to
//             scores is one upload (depths, entry lists), two launches, one download, and no table exists on the host.  Writing the full
//             table [n_nodes][n_samples][ploidy + 1] for download (and, when asked, the doubles it was rounded from), the sample runs
//             fastest within a node instead: a wave writes one contiguous stretch of 64 * (ploidy + 1) values (each store instruction
//             strided by ploidy + 1 values within it), but its two depth loads per lane are then n_rows words apart, a cache line
//             each.  That trades 2 scattered loads for ploidy + 1 (or, with the doubles, 3 (ploidy + 1)) gathered stores on a path
//             whose time is the download of the table; the choice is not measured.  A few hundred f64 multiplications per lane
//             against its stores: no LDS.
// All calls: the upload is one image of typed pieces (call_image.h), the call runs through the steps of Session (device_runtime.h).
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

// The problems of a batch that have something to compute, and what progeny_pair_kernel reads of them apart from the planes: prefix,
// descriptors and entry lists as pieces of the call's image.  The others hold -inf entries only (or none) and are filled at once.
struct PairBatch {
	const std::vector<ProgenyProblem>& ps;
	std::vector<uint32_t> up;
	std::vector<uint64_t> entry_base, table_base;   // [up.size() + 1]
	uint64_t n_entries = 0, n_floats = 0;
	Piece<uint64_t> p_prefix;
	Piece<DevProblem> p_desc;
	Piece<uint32_t> p_lo, p_eff;
	Piece<uint8_t> p_kind;

	PairBatch(const std::vector<ProgenyProblem>& problems, std::vector<ProgenyResult>& out) : ps(problems) {
		out.assign(ps.size(), ProgenyResult{});
		for (uint32_t x = 0; x < ps.size(); x++) {
			const ProgenyProblem& p = ps[x];
			if (p.lo.size() == p.n_inf) out[x].score.assign(p.lo.size(), -std::numeric_limits<double>::infinity());
			else up.push_back(x);
		}
		entry_base.assign(up.size() + 1, 0);
		table_base.assign(up.size() + 1, 0);
		for (uint32_t u = 0; u < up.size(); u++) {
			const ProgenyProblem& p = ps[up[u]];
			entry_base[u + 1] = entry_base[u] + p.lo.size();
			table_base[u + 1] = table_base[u] + 3 * (uint64_t)p.n_samples * p.n_nodes;
		}
		n_entries = entry_base.back();
		n_floats = table_base.back();
	}
	void add(ImageLayout& in) {
		p_prefix = in.add<uint64_t>(up.size() + 1);
		p_desc = in.add<DevProblem>(up.size());
		p_lo = in.add<uint32_t>(n_entries);
		p_eff = in.add<uint32_t>(n_entries);
		p_kind = in.add<uint8_t>(n_entries);
	}
	void fill(const Image& im) const {
		for (uint32_t u = 0; u < up.size(); u++) {
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
			progeny_copy(im.host(p_lo) + entry_base[u], p.lo.data(), p.lo.size() * 4);
			progeny_copy(im.host(p_eff) + entry_base[u], p.eff.data(), p.eff.size() * 4);
			progeny_copy(im.host(p_kind) + entry_base[u], p.kind.data(), p.kind.size());
		}
		im.host(p_prefix)[up.size()] = n_entries;
	}
	PairArgs args(const Image& im, const float* table, double* score) const {
		PairArgs pa{};
		pa.n_entries = n_entries;
		pa.n_problems = (uint32_t)up.size();
		pa.entry_prefix = im.dev(p_prefix);
		pa.problems = im.dev(p_desc);
		pa.lo = im.dev(p_lo);
		pa.eff = im.dev(p_eff);
		pa.kind = im.dev(p_kind);
		pa.table = table;
		pa.score = score;
		return pa;
	}
	dim3 blocks() const { return dim3(grid_for(n_entries, BLOCK, MAX_BLOCKS)); }
	void scatter(const double* res, std::vector<ProgenyResult>& out) const {
		for (uint32_t u = 0; u < up.size(); u++) {
			RawVec<double>& dst = out[up[u]].score;
			dst.resize(entry_base[u + 1] - entry_base[u]);
			progeny_copy(dst.data(), res + entry_base[u], dst.size() * 8);
		}
	}
};

constexpr uint64_t NO_PRIOR = ~(uint64_t)0;

struct DevDepths {
	uint64_t depth_off;              // first word of this problem's depths (ref and alt alike)
	uint64_t node_off;               // first entry of its node_row
	uint64_t row_off;                // first entry of its row_prior
	uint64_t prior_off;              // first double of its priors, NO_PRIOR: none
	uint64_t plane_off;              // first float of its planes
	uint64_t value_off;              // first value of its full table
	uint32_t n_rows, n_nodes, n_samples, ploidy;
	double error_rate;
};

struct GlArgs {
	uint64_t n_cells;
	uint32_t n_problems;
	const uint64_t* cell_prefix;     // [n_problems + 1]
	const DevDepths* problems;
	const uint32_t* ref;             // per problem [n_samples][n_rows]
	const uint32_t* alt;
	const uint32_t* node_row;        // per problem [n_nodes]
	const uint32_t* row_prior;       // per problem with priors [n_rows]
	const double* priors;
	float* planes;                   // nullptr: none; else per problem [n_samples][3][n_nodes], lanes in this order
	float* table;                    // nullptr: none; else per problem [n_nodes][n_samples][ploidy + 1]
	double* table_f64;
};

__global__ void __launch_bounds__(BLOCK) progeny_gl_kernel(GlArgs a) {
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; c < a.n_cells; c += stride) {
		const uint32_t m = problem_of(a.cell_prefix, a.n_problems, c);   // (a problem without cells is never the last with prefix <= c)
		const DevDepths& d = a.problems[m];
		const uint64_t local = c - a.cell_prefix[m];
		uint64_t sample, node;
		if (a.planes) {   // node fastest: consecutive depth words in, consecutive floats of a plane out
			sample = local / d.n_nodes;
			node = local - sample * d.n_nodes;
		} else {          // sample fastest: the wave's rows of the full table are one contiguous stretch (its depth loads are n_rows words apart)
			node = local / d.n_samples;
			sample = local - node * d.n_samples;
		}
		const uint32_t row = a.node_row[d.node_off + node];
		const uint64_t w = d.depth_off + sample * d.n_rows + row;
		const double* prior = d.prior_off == NO_PRIOR ? nullptr : a.priors + d.prior_off + a.row_prior[d.row_off + row];
		const uint64_t v = d.value_off + (node * d.n_samples + sample) * (d.ploidy + 1);
		progeny_gl_cell(a.ref[w], a.alt[w], d.ploidy, d.error_rate, prior, a.planes ? a.planes + d.plane_off + sample * 3 * d.n_nodes + node : nullptr,
		                d.n_nodes, a.table ? a.table + v : nullptr, a.table_f64 ? a.table_f64 + v : nullptr);
	}
}

// What progeny_gl_kernel reads of a batch of depth problems, as pieces of the call's image.
struct DepthBatch {
	std::vector<const ProgenyDepths*> ds;
	std::vector<uint64_t> cell_base, depth_base, node_base, row_base, prior_base, value_base;   // [ds.size() + 1]
	uint64_t n_cells = 0, n_values = 0;
	Piece<uint64_t> p_prefix;
	Piece<DevDepths> p_desc;
	Piece<uint32_t> p_ref, p_alt, p_node_row, p_row_prior;
	Piece<double> p_priors;

	explicit DepthBatch(std::vector<const ProgenyDepths*> problems) : ds(std::move(problems)) {
		const size_t n = ds.size();
		for (auto* v : {&cell_base, &depth_base, &node_base, &row_base, &prior_base, &value_base}) v->assign(n + 1, 0);
		for (size_t x = 0; x < n; x++) {
			const ProgenyDepths& p = *ds[x];
			const uint64_t k1 = p.ploidy + 1, cells = p.n_nodes * p.n_samples;
			cell_base[x + 1] = cell_base[x] + cells;
			depth_base[x + 1] = depth_base[x] + p.n_rows * p.n_samples;
			node_base[x + 1] = node_base[x] + p.n_nodes;
			row_base[x + 1] = row_base[x] + p.row_prior.size();
			prior_base[x + 1] = prior_base[x] + (p.priors ? k1 * k1 * k1 : 0);
			value_base[x + 1] = value_base[x] + cells * k1;
		}
		n_cells = cell_base.back();
		n_values = value_base.back();
	}
	void add(ImageLayout& in) {
		p_prefix = in.add<uint64_t>(ds.size() + 1);
		p_desc = in.add<DevDepths>(ds.size());
		p_ref = in.add<uint32_t>(depth_base.back());
		p_alt = in.add<uint32_t>(depth_base.back());
		p_node_row = in.add<uint32_t>(node_base.back());
		p_row_prior = in.add<uint32_t>(row_base.back());
		p_priors = in.add<double>(prior_base.back());
	}
	// plane_base: [ds.size()] the first float of every problem's planes, nullptr: no planes are written
	void fill(const Image& im, const uint64_t* plane_base) const {
		for (size_t x = 0; x < ds.size(); x++) {
			const ProgenyDepths& p = *ds[x];
			im.host(p_prefix)[x] = cell_base[x];
			DevDepths d{};
			d.depth_off = depth_base[x];
			d.node_off = node_base[x];
			d.row_off = row_base[x];
			d.prior_off = p.priors ? prior_base[x] : NO_PRIOR;
			d.plane_off = plane_base ? plane_base[x] : 0;
			d.value_off = value_base[x];
			d.n_rows = (uint32_t)p.n_rows;
			d.n_nodes = (uint32_t)p.n_nodes;
			d.n_samples = p.n_samples;
			d.ploidy = p.ploidy;
			d.error_rate = p.error_rate;
			im.host(p_desc)[x] = d;
			const uint64_t words = depth_base[x + 1] - depth_base[x];
			progeny_copy(im.host(p_ref) + depth_base[x], p.ref, words * 4);
			progeny_copy(im.host(p_alt) + depth_base[x], p.alt, words * 4);
			progeny_copy(im.host(p_node_row) + node_base[x], p.node_row, p.n_nodes * 4);
			progeny_copy(im.host(p_row_prior) + row_base[x], p.row_prior.data(), p.row_prior.size() * 4);
			if (p.priors) std::memcpy(im.host(p_priors) + prior_base[x], p.priors, (prior_base[x + 1] - prior_base[x]) * 8);
		}
		im.host(p_prefix)[ds.size()] = n_cells;
	}
	GlArgs args(const Image& im, float* planes, float* table, double* table_f64) const {
		GlArgs ga{};
		ga.n_cells = n_cells;
		ga.n_problems = (uint32_t)ds.size();
		ga.cell_prefix = im.dev(p_prefix);
		ga.problems = im.dev(p_desc);
		ga.ref = im.dev(p_ref);
		ga.alt = im.dev(p_alt);
		ga.node_row = im.dev(p_node_row);
		ga.row_prior = im.dev(p_row_prior);
		ga.priors = im.dev(p_priors);
		ga.planes = planes;
		ga.table = table;
		ga.table_f64 = table_f64;
		return ga;
	}
	dim3 blocks() const { return dim3(grid_for(n_cells, BLOCK, MAX_BLOCKS)); }
};

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
	PairBatch b(ps, out);
	if (b.up.empty()) return WHAMD_OK;   // nothing to compute: no device work at all
	const uint32_t n_up = (uint32_t)b.up.size();
	struct PackJob { uint32_t u; uint64_t node0; };
	std::vector<PackJob> jobs;
	for (uint32_t u = 0; u < n_up; u++) {
		const ProgenyProblem& p = ps[b.up[u]];
		if (p.n_samples)
			for (uint64_t node0 = 0; node0 < p.n_nodes; node0 += PACK_NODES) jobs.push_back(PackJob{u, node0});
	}
	// the image (one upload)
	ImageLayout in;
	b.add(in);
	const auto p_table = in.add<float>(std::max<uint64_t>(b.n_floats, 1));
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im;
	double* score = nullptr;
	double* res = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.device_block(b.n_entries * 8, (void**)&score, msg));
	WHAMD_TRY(s.pinned_block(b.n_entries * 8, (void**)&res, msg));
	b.fill(im);
	// the repack: a block of nodes at a time (its rows stay in the host cache while every plane takes its piece)
	parallel_ranges(jobs.size(), host_threads(b.n_floats, 1 << 18), [&](uint64_t jb, uint64_t je, uint32_t) {
		for (uint64_t x = jb; x < je; x++) {
			const ProgenyProblem& p = ps[b.up[jobs[x].u]];
			const uint64_t node0 = jobs[x].node0, node1 = std::min<uint64_t>(node0 + PACK_NODES, p.n_nodes);
			const uint64_t k1 = p.ploidy + 1, row = (uint64_t)p.n_samples * k1;
			float* t = im.host(p_table) + b.table_base[jobs[x].u];
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

	const PairArgs pa = b.args(im, im.dev(p_table), score);
	WHAMD_TRY(s.upload(im, msg));
	WHAMD_TRY(launch(s, times, msg, progeny_pair_kernel, b.blocks(), dim3(BLOCK), 0, pa));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, score, b.n_entries * 8, msg));
	WHAMD_TRY(s.finish(times, msg));
	b.scatter(res, out);
	return WHAMD_OK;
}

whamd_status_t progeny_gl_device(const std::vector<ProgenyDepths>& ds, int device, float* const* table_out, double* const* table_f64_out,
                                 std::string& msg) {
	bool want_f32 = false, want_f64 = false;
	std::vector<const ProgenyDepths*> list;
	for (size_t x = 0; x < ds.size(); x++) {
		list.push_back(&ds[x]);
		const bool cells = ds[x].n_nodes && ds[x].n_samples;
		want_f32 = want_f32 || (cells && table_out && table_out[x]);
		want_f64 = want_f64 || (cells && table_f64_out && table_f64_out[x]);
	}
	if (!want_f32 && !want_f64) return WHAMD_OK;   // nothing asked for, or no cells: no device work
	DepthBatch b(list);
	ImageLayout in;
	b.add(in);
	Session s;
	WHAMD_TRY(s.open(device, 0, msg));   // (no events: the call reports no times)
	Image im;
	float *t32 = nullptr, *r32 = nullptr;
	double *t64 = nullptr, *r64 = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	if (want_f32) WHAMD_TRY(s.device_block(b.n_values * 4, (void**)&t32, msg));
	if (want_f32) WHAMD_TRY(s.pinned_block(b.n_values * 4, (void**)&r32, msg));
	if (want_f64) WHAMD_TRY(s.device_block(b.n_values * 8, (void**)&t64, msg));
	if (want_f64) WHAMD_TRY(s.pinned_block(b.n_values * 8, (void**)&r64, msg));
	b.fill(im, nullptr);
	const GlArgs ga = b.args(im, nullptr, t32, t64);
	WHAMD_TRY(s.upload(im, msg));
	CallTimes unused;
	WHAMD_TRY(launch(s, unused, msg, progeny_gl_kernel, b.blocks(), dim3(BLOCK), 0, ga));
	if (want_f32) WHAMD_TRY(s.fetch(r32, t32, b.n_values * 4, msg));
	if (want_f64) WHAMD_TRY(s.fetch(r64, t64, b.n_values * 8, msg));
	WHAMD_TRY(s.finish(unused, msg));
	for (size_t x = 0; x < ds.size(); x++) {
		const uint64_t n = b.value_base[x + 1] - b.value_base[x];
		if (want_f32 && table_out[x]) progeny_copy(table_out[x], r32 + b.value_base[x], n * 4);
		if (want_f64 && table_f64_out[x]) progeny_copy(table_f64_out[x], r64 + b.value_base[x], n * 8);
	}
	return WHAMD_OK;
}

whamd_status_t progeny_score_depths_device(const std::vector<ProgenyDepths>& ds, const std::vector<ProgenyProblem>& ps, int device,
                                           std::vector<ProgenyResult>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	PairBatch b(ps, out);
	if (b.up.empty()) return WHAMD_OK;   // nothing to compute: no device work at all
	std::vector<const ProgenyDepths*> list;
	for (const uint32_t x : b.up) list.push_back(&ds[x]);
	DepthBatch d(list);
	// the image (one upload): entry lists and depths; the planes are the device's own
	ImageLayout in;
	b.add(in);
	d.add(in);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im;
	float* planes = nullptr;
	double* score = nullptr;
	double* res = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.device_block(std::max<uint64_t>(b.n_floats, 1) * 4, (void**)&planes, msg));
	WHAMD_TRY(s.device_block(b.n_entries * 8, (void**)&score, msg));
	WHAMD_TRY(s.pinned_block(b.n_entries * 8, (void**)&res, msg));
	b.fill(im);
	d.fill(im, b.table_base.data());
	const GlArgs ga = d.args(im, planes, nullptr, nullptr);
	const PairArgs pa = b.args(im, planes, score);
	WHAMD_TRY(s.upload(im, msg));
	if (d.n_cells) WHAMD_TRY(launch(s, times, msg, progeny_gl_kernel, d.blocks(), dim3(BLOCK), 0, ga));   // (entries between nodes of a problem without samples read no plane)
	WHAMD_TRY(launch(s, times, msg, progeny_pair_kernel, b.blocks(), dim3(BLOCK), 0, pa));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, score, b.n_entries * 8, msg));
	WHAMD_TRY(s.finish(times, msg));
	b.scatter(res, out);
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
	WHAMD_TRY(s.open(device, 0, msg));   // (no events: the call reports no times)
	Image im;
	double* out = nullptr;
	double* res = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.device_block(n_lanes * 8, (void**)&out, msg));
	WHAMD_TRY(s.pinned_block(n_lanes * 8, (void**)&res, msg));
	std::memcpy(im.host(p_prior), prior, p_prior.bytes());
	std::memcpy(im.host(p_rows), rows, p_rows.bytes());
	TypesKernelArgs ta{n_lanes, n_types, n_samples, k1, im.dev(p_rows), im.dev(p_prior), out};
	WHAMD_TRY(s.upload(im, msg));
	CallTimes unused;
	WHAMD_TRY(launch(s, unused, msg, progeny_types_kernel, dim3(grid_for(n_lanes, BLOCK, MAX_BLOCKS)), dim3(BLOCK), 0, ta));
	WHAMD_TRY(s.fetch(res, out, n_lanes * 8, msg));
	WHAMD_TRY(s.finish(unused, msg));
	std::memcpy(llh, res, n_lanes * 8);
	return WHAMD_OK;
}

}  // namespace whamd
