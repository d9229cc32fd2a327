// polyreorder_device.hip -- the link likelihoods of polyphase reordering on gfx950 (polyreorder.h).  A batch of problems is one upload,
// two launches and one download:
//   upload    the breakpoint records of all problems, the reads that count at each of them (items: breakpoint, where the read's row is),
//             the windows, the haplotypes and the matrix rows of the problems that have breakpoints, the breakpoint of every workgroup
//             of the permutation kernel.
//   table     one lane per item: the read's alleles at window positions against the k affected haplotypes, left and right of the
//             breakpoint, to the item's table row {left[k], right[k]} (pr_read_rows).  Skipped when no read counts anywhere.
//   permute   one workgroup per (breakpoint, 256 consecutive permutations), one lane per permutation: the lane unranks its permutation
//             (pr_unrank), the workgroup stages the breakpoint's table rows through LDS, PR_READ_TILE reads at a time, and every lane walks
//             the staged reads in order, adding the read's term (pr_read_term) to its sum -- sequential per permutation, so the bits are
//             those of the reference's loop.  All lanes read the same left values (broadcast) and one of k right values.
//   download  the sums, k! per breakpoint.
// (The upload is one image of typed pieces, call_image.h; the call runs through the steps of Session, device_runtime.h.)
// The window search and the read lists are host work (polyreorder.cpp): a scan that ends after 32 hits and a filter over cluster members.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_runtime.h"
#include "polyreorder.h"

namespace whamd {
namespace {

struct PrArgs {
	const PrBreakpoint* bps;
	const PrItem* items;
	const uint32_t* tile_bp;      // per workgroup of the permutation kernel: its breakpoint
	const uint32_t* win;
	const int8_t* hap;
	const uint32_t* row_pos;
	const uint8_t* row_allele;
	double* table;
	double* llh;
	uint64_t n_items;
	double log_match, log_err;
};

__global__ void __launch_bounds__(PR_BLOCK) reorder_table_kernel(PrArgs a) {
	const uint64_t x = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
	if (x >= a.n_items) return;
	const PrItem it = a.items[x];
	const PrBreakpoint& bp = a.bps[it.bp];
	pr_read_rows(a.row_pos + it.row_begin, a.row_allele + it.row_begin, it.row_n, a.win + bp.win_begin, bp.n_win, bp.pos, a.hap + bp.hap_base, bp.n_pos,
	             bp.affected, bp.k, a.log_match, a.log_err, a.table + bp.tab_begin + (x - bp.item_begin) * 2 * bp.k);
}

__global__ void __launch_bounds__(PR_BLOCK) reorder_permute_kernel(PrArgs a) {
	__shared__ double tile[PR_READ_TILE * 2 * PR_MAX_AFFECTED];
	const PrBreakpoint& bp = a.bps[a.tile_bp[blockIdx.x]];
	const uint32_t k = bp.k, w = 2 * k, n_items = bp.n_items;
	const uint32_t rank = (blockIdx.x - bp.tile_begin) * PR_BLOCK + threadIdx.x;
	const bool have = rank < bp.n_perm;
	const uint32_t perm = pr_unrank(have ? rank : 0, k);
	const double* rows = a.table + bp.tab_begin;
	double acc = 0.0;
	for (uint32_t r0 = 0; r0 < n_items; r0 += PR_READ_TILE) {   // (n_items is the workgroup's: every thread meets the barriers)
		const uint32_t n = min(PR_READ_TILE, n_items - r0);
		const double* src = rows + (uint64_t)r0 * w;
		for (uint32_t x = threadIdx.x; x < n * w; x += PR_BLOCK) tile[x] = src[x];
		__syncthreads();
		for (uint32_t r = 0; r < n; r++) acc += pr_read_term(tile + r * w, k, perm);
		__syncthreads();
	}
	if (have) a.llh[bp.llh_begin + rank] = acc;
}

}  // namespace

whamd_status_t reorder_score_device(const std::vector<ReorderProblem>& ps, double log_match, double log_err, int device, std::vector<ReorderScores>& out,
                                    CallTimes& times, std::string& msg) {
	times = CallTimes{};
	out.assign(ps.size(), ReorderScores{});
	// where every problem's pieces start
	struct Base { uint64_t bp, item, win, hap, row, tab, llh; };
	std::vector<Base> base(ps.size() + 1, Base{0, 0, 0, 0, 0, 0, 0});
	uint64_t n_tiles = 0;
	for (size_t x = 0; x < ps.size(); x++) {
		const ReorderProblem& p = ps[x];
		Base b = base[x];
		const uint64_t n_bp = p.n_breakpoints();
		out[x].llh.assign(p.llh_ptr.back(), 0.0);
		if (n_bp) {
			b.bp += n_bp;
			b.item += p.item_read.size();
			b.win += p.win.size();
			b.hap += (uint64_t)p.ploidy * p.n_pos;
			b.row += p.m.row_pos.size();
			b.llh += p.llh_ptr.back();
			for (uint64_t y = 0; y < n_bp; y++) {
				b.tab += (p.item_ptr[y + 1] - p.item_ptr[y]) * 2 * p.bp_k[y];
				n_tiles += (p.llh_ptr[y + 1] - p.llh_ptr[y] + PR_BLOCK - 1) / PR_BLOCK;
			}
		}
		base[x + 1] = b;
	}
	const Base total = base[ps.size()];
	if (!total.bp) return WHAMD_OK;   // no breakpoint anywhere: no device work at all
	if (total.bp >= 0x80000000ull || total.item >= 0x80000000ull * PR_BLOCK || n_tiles >= 0x80000000ull) {   // (grid sizes and tile_bp are uint32)
		msg = "more than 2^31 - 1 breakpoints or workgroups in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	ImageLayout in;
	const auto p_bp = in.add<PrBreakpoint>(total.bp);
	const auto p_item = in.add<PrItem>(total.item);
	const auto p_tile = in.add<uint32_t>(n_tiles);
	const auto p_win = in.add<uint32_t>(total.win);
	const auto p_hap = in.add<int8_t>(total.hap);
	const auto p_rpos = in.add<uint32_t>(total.row);
	const auto p_rall = in.add<uint8_t>(total.row);
	ImageLayout out_layout;   // what the kernels write and what comes back: the sums
	const auto p_llh = out_layout.add<double>(total.llh);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, res;
	double* dev_table = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	if (total.tab) WHAMD_TRY(s.device_block(total.tab * sizeof(double), (void**)&dev_table, msg));
	WHAMD_TRY(s.stage(out_layout, res, msg));
	uint32_t tile_at = 0;
	for (size_t x = 0; x < ps.size(); x++) {
		const ReorderProblem& p = ps[x];
		const Base& b = base[x];
		const uint64_t n_bp = p.n_breakpoints();
		if (!n_bp) continue;
		if (!p.win.empty()) std::memcpy(im.host(p_win) + b.win, p.win.data(), p.win.size() * sizeof(uint32_t));
		std::memcpy(im.host(p_hap) + b.hap, p.haplotypes, (size_t)p.ploidy * p.n_pos);
		if (!p.m.row_pos.empty()) {
			std::memcpy(im.host(p_rpos) + b.row, p.m.row_pos.data(), p.m.row_pos.size() * sizeof(uint32_t));
			std::memcpy(im.host(p_rall) + b.row, p.m.row_allele.data(), p.m.row_allele.size());
		}
		uint64_t tab = b.tab;
		for (uint64_t y = 0; y < n_bp; y++) {
			PrBreakpoint rec{};
			rec.hap_base = b.hap;
			rec.n_pos = p.n_pos;
			rec.win_begin = b.win + p.win_ptr[y];
			rec.item_begin = b.item + p.item_ptr[y];
			rec.tab_begin = tab;
			rec.llh_begin = b.llh + p.llh_ptr[y];
			rec.n_items = (uint32_t)(p.item_ptr[y + 1] - p.item_ptr[y]);
			rec.n_win = (uint32_t)(p.win_ptr[y + 1] - p.win_ptr[y]);
			rec.pos = p.bp_pos[y];
			rec.k = p.bp_k[y];
			rec.tile_begin = tile_at;
			rec.n_perm = (uint32_t)(p.llh_ptr[y + 1] - p.llh_ptr[y]);
			std::memcpy(rec.affected, p.bp_affected.data() + y * PR_MAX_AFFECTED, PR_MAX_AFFECTED);
			im.host(p_bp)[b.bp + y] = rec;
			tab += (uint64_t)rec.n_items * 2 * rec.k;
			for (uint32_t t = 0; t < (rec.n_perm + PR_BLOCK - 1) / PR_BLOCK; t++) im.host(p_tile)[tile_at++] = (uint32_t)(b.bp + y);
			for (uint64_t z = p.item_ptr[y]; z < p.item_ptr[y + 1]; z++) {
				const uint32_t r = p.item_read[z];
				im.host(p_item)[b.item + z] = PrItem{b.row + p.m.row_ptr[r], (uint32_t)(p.m.row_ptr[r + 1] - p.m.row_ptr[r]), (uint32_t)(b.bp + y)};
			}
		}
	}
	WHAMD_TRY(s.upload(im, msg));
	PrArgs a{im.dev(p_bp), im.dev(p_item), im.dev(p_tile), im.dev(p_win), im.dev(p_hap), im.dev(p_rpos), im.dev(p_rall), dev_table, res.dev_out(p_llh), total.item,
	         log_match, log_err};
	if (total.item) WHAMD_TRY(launch(s, times, msg, reorder_table_kernel, dim3(grid_for(total.item, PR_BLOCK)), dim3(PR_BLOCK), 0, a));
	WHAMD_TRY(launch(s, times, msg, reorder_permute_kernel, dim3((uint32_t)n_tiles), dim3(PR_BLOCK), 0, a));
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, p_llh, res.dev(p_llh), msg));
	WHAMD_TRY(s.finish(times, msg));
	for (size_t x = 0; x < ps.size(); x++)
		if (!out[x].llh.empty()) std::memcpy(out[x].llh.data(), res.host(p_llh) + base[x].llh, out[x].llh.size() * sizeof(double));
	return WHAMD_OK;
}

}  // namespace whamd
