// polycompare_device.hip -- comparing polyploid phasings on gfx950 (polycompare.h).  A batch of jobs is one upload, one launch and one
// download:
//   upload    the records of the jobs that visit a position, and their phasings.
//   compare   one workgroup per job.  A lane owns the states lane, lane + 256, lane + 512 (720 states over 256 lanes at ploidy 6, one
//             state per lane up to ploidy 5) and keeps their permutations as packed nibbles in registers.  The previous column lives in
//             LDS, double-buffered, as score (f64), flips so far (u32) and switches so far (u32) per state, beside every state's
//             permutation: 2 x 720 x 16 + 720 x 4 + 720 x 8 bytes (the Hamming sums of the end) = 31 680 bytes.  Per visited column every
//             lane walks the previous states in increasing rank -- all lanes read the same address: a broadcast --, keeps the candidate
//             that is strictly smaller in (value, flips) (pc_consider), adds the flip term (pc_state_score), writes the other buffer;
//             one barrier per column.  matched_only columns are recognised by every lane from the same two words (pc_matched) and
//             skipped by the whole workgroup.  With want_path the predecessor ranks go to global memory, and lane 0 walks back after the
//             last barrier.  The end state is the minimum in (score, flips, rank); scalar results leave through lane 0's plain stores.
//   download  per job total, switches, flips and the minimum Hamming sum; the paths.
// (The upload is one image of typed pieces, call_image.h; the call runs through the steps of Session, device_runtime.h.)
#include <hip/hip_runtime.h>

#include <cstring>

#include "device_runtime.h"
#include "polycompare.h"

namespace whamd {
namespace {

struct PcArgs {
	const PcJob* jobs;
	const uint8_t* alleles;
	PcOut* out;
	uint16_t* pred;
	uint16_t* path;
};

struct PcShared {
	double score[2][PC_MAX_STATES];
	uint64_t ham[PC_MAX_STATES];
	uint32_t flips[2][PC_MAX_STATES];
	uint32_t sw[2][PC_MAX_STATES];
	uint32_t perm[PC_MAX_STATES];
};

// The forward pass of one job with ROWS states per lane; returns the buffer that holds the last column.
template <uint32_t ROWS>
__device__ uint32_t compare_forward(const PcArgs& a, const PcJob& job, PcShared& s) {
	const uint32_t k = job.k, n = job.n_states, lane = threadIdx.x;
	uint32_t perm[ROWS];
	uint64_t ham[ROWS];
#pragma unroll
	for (uint32_t j = 0; j < ROWS; j++) {
		const uint32_t r = lane + j * PC_BLOCK;
		perm[j] = pr_unrank(r < n ? r : 0, k);
		ham[j] = 0;
		if (r < n) s.perm[r] = perm[j];
	}
	__syncthreads();
	const uint8_t* p0 = a.alleles + job.p0_begin;
	const uint8_t* p1 = a.alleles + job.p1_begin;
	uint16_t* pred = a.pred + job.pred_begin;
	uint32_t cur = 0;
	uint64_t v = 0;
	uint64_t next0 = pc_column(p0, k), next1 = pc_column(p1, k);   // (n_pos >= n_visited >= 1)
	for (uint64_t x = 0; x < job.n_pos; x++) {
		const uint64_t c0 = next0, c1 = next1;
		if (x + 1 < job.n_pos) {   // the next column's alleles travel under this column's arithmetic
			next0 = pc_column(p0 + (x + 1) * k, k);
			next1 = pc_column(p1 + (x + 1) * k, k);
		}
		if (job.matched_only && !pc_matched(c0, c1, k)) continue;   // (the same for every lane: no lane waits at a barrier alone)
		if (v == job.n_visited) break;                              // (the host counted with the same function: the tables hold n_visited columns)
		PcBest best[ROWS];
		uint32_t f[ROWS];
#pragma unroll
		for (uint32_t j = 0; j < ROWS; j++) {
			best[j] = pc_best_none();
			f[j] = pc_flips(perm[j], c0, c1, k);
			ham[j] += f[j];
		}
		if (v)
			for (uint32_t q = 0; q < n; q++) {
				const double score_q = s.score[cur][q];
				const uint32_t flips_q = s.flips[cur][q], perm_q = s.perm[q];
#pragma unroll
				for (uint32_t j = 0; j < ROWS; j++) pc_consider(best[j], score_q, flips_q, q, job.switch_cost, pc_switches(perm[j], perm_q));
			}
#pragma unroll
		for (uint32_t j = 0; j < ROWS; j++) {
			const uint32_t r = lane + j * PC_BLOCK;
			if (r < n) {
				const uint32_t q = best[j].q;   // (0 in column 0; below n always)
				s.score[cur ^ 1][r] = pc_state_score(v == 0, best[j].value, job.flip_cost, f[j]);
				s.flips[cur ^ 1][r] = (v ? s.flips[cur][q] : 0u) + f[j];
				s.sw[cur ^ 1][r] = v ? s.sw[cur][q] + pc_switches(perm[j], s.perm[q]) : 0u;
				if (job.want_path && v) pred[v * n + r] = (uint16_t)q;
			}
		}
		__syncthreads();
		cur ^= 1;
		++v;
	}
#pragma unroll
	for (uint32_t j = 0; j < ROWS; j++) {
		const uint32_t r = lane + j * PC_BLOCK;
		if (r < n) s.ham[r] = ham[j];
	}
	__syncthreads();
	return cur;
}

__global__ void __launch_bounds__(PC_BLOCK) compare_kernel(PcArgs a) {
	__shared__ PcShared s;
	const PcJob job = a.jobs[blockIdx.x];
	const uint32_t n = job.n_states;
	const uint32_t cur = n <= PC_BLOCK ? compare_forward<1>(a, job, s) : compare_forward<PC_ROWS>(a, job, s);
	if (threadIdx.x) return;
	uint32_t end = 0;
	uint64_t min_ham = s.ham[0];
	for (uint32_t r = 1; r < n; r++) {
		if (pc_end_better(s.score[cur][r], s.flips[cur][r], s.score[cur][end], s.flips[cur][end])) end = r;
		if (s.ham[r] < min_ham) min_ham = s.ham[r];
	}
	a.out[blockIdx.x] = PcOut{s.score[cur][end], min_ham, pc_end_switches(job.n_visited, s.perm[end], s.sw[cur][end]), s.flips[cur][end]};
	if (job.want_path) {   // the predecessors were written by this workgroup before its last barrier
		const uint16_t* pred = a.pred + job.pred_begin;
		uint16_t* path = a.path + job.path_begin;
		uint32_t r = end;
		for (uint64_t y = job.n_visited; y-- > 0;) {
			path[y] = (uint16_t)r;
			if (y) r = pred[y * n + r];
		}
	}
}

}  // namespace

whamd_status_t compare_device(const std::vector<CompareJob>& jobs, int device, std::vector<CompareResult>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(jobs.size(), CompareResult{});
	// the jobs that visit a position, and where their pieces start
	std::vector<size_t> sent;
	uint64_t n_alleles = 0, n_pred = 0, n_path = 0;
	for (size_t x = 0; x < jobs.size(); x++)
		if (jobs[x].n_visited) sent.push_back(x);
	if (sent.empty()) return WHAMD_OK;   // nothing to visit anywhere: no device work at all
	if (sent.size() >= 0x80000000ull) {
		msg = "more than 2^31 - 1 jobs in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	std::vector<PcJob> recs(sent.size());
	for (size_t y = 0; y < sent.size(); y++) {
		const CompareJob& j = jobs[sent[y]];
		PcJob& rec = recs[y];
		rec.p0_begin = n_alleles;
		rec.p1_begin = n_alleles + j.n_pos * j.k;
		n_alleles += 2 * j.n_pos * j.k;
		rec.n_pos = j.n_pos;
		rec.n_visited = j.n_visited;
		rec.pred_begin = n_pred;
		rec.path_begin = n_path;
		if (j.want_path) {
			n_pred += j.n_visited * j.n_states;
			n_path += j.n_visited;
		}
		rec.switch_cost = j.switch_cost;
		rec.flip_cost = j.flip_cost;
		rec.k = j.k;
		rec.n_states = j.n_states;
		rec.matched_only = j.matched_only;
		rec.want_path = j.want_path;
	}
	ImageLayout in;
	const auto p_job = in.add<PcJob>(recs.size());
	const auto p_all = in.add<uint8_t>(n_alleles);
	ImageLayout res_layout;   // what the kernel writes and what comes back, in one copy: the results, then the paths
	const auto p_out = res_layout.add<PcOut>(recs.size());
	const auto p_path = res_layout.add<uint16_t>(n_path);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, res;
	uint16_t* dev_pred = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.stage(res_layout, res, msg));
	if (n_pred) WHAMD_TRY(s.device_block(n_pred * sizeof(uint16_t), (void**)&dev_pred, msg));
	std::memcpy(im.host(p_job), recs.data(), recs.size() * sizeof(PcJob));
	for (size_t y = 0; y < sent.size(); y++) {
		const CompareJob& j = jobs[sent[y]];
		std::memcpy(im.host(p_all) + recs[y].p0_begin, j.p0, j.n_pos * j.k);
		std::memcpy(im.host(p_all) + recs[y].p1_begin, j.p1, j.n_pos * j.k);
	}
	WHAMD_TRY(s.upload(im, msg));
	PcArgs a{im.dev(p_job), im.dev(p_all), res.dev_out(p_out), dev_pred, res.dev_out(p_path)};
	WHAMD_TRY(launch(s, times, msg, compare_kernel, dim3((uint32_t)recs.size()), dim3(PC_BLOCK), 0, a));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res.stage, res.base, res.total, msg));
	WHAMD_TRY(s.finish(times, msg));
	const PcOut* got = res.host(p_out);
	const uint16_t* paths = res.host(p_path);
	for (size_t y = 0; y < sent.size(); y++) {
		CompareResult& o = out[sent[y]];
		o.out = got[y];
		if (jobs[sent[y]].want_path) o.path.assign(paths + recs[y].path_begin, paths + recs[y].path_begin + recs[y].n_visited);
	}
	return WHAMD_OK;
}

}  // namespace whamd
