// haplotag_device.hip -- the scoring of haplotagging on gfx950 (haplotag.h).  A batch of problems is one upload, one launch per class of
// group size that has groups (at most three) and one download:
//   upload    the variants of all problems {phase set id, haplotype masks}, the entries of all groups {variant | allele << 31, quality} --
//             every group's entries one contiguous run in processing order, the runs in the order of the group records -- and the records
//             {first entry, entries, ploidy}, sorted by class.
//   class a   (1 .. 64 entries)  eight lanes per group, eight groups per wave: consecutive records own consecutive runs, so a wave's loads
//             of a chunk are consecutive 64-byte pieces.
//   class b   (65 .. 4096)       one wave per group.
//   class c   (more)             one workgroup per group: every wave takes a contiguous quarter of the run, the quarters meet in LDS.
// (The upload is one image of three typed pieces, call_image.h; the call runs through the steps of Session, device_runtime.h.)
// A team (segment, wave) walks its run in chunks of its width, in order.  It keeps up to R = 4 phase sets in registers, in the order of
// their first matching entry (SlotNames of run_teams.h; its hook records the index of the entry that names a slot).  Every lane adds its
// entry's quality to the sums of its slot under the entry's haplotype mask (R x P predicated adds, P = the launch's ploidy rounded up to
// 2, 4, 8 or 16); the sums meet in a butterfly of the team.  A group with more than R phase sets takes the slower route: walk_ids of
// run_teams.h over its phase sets in the order of the ids, the body summing that phase set alone and keeping the index of its first
// matching entry (PsAcc, combined by the team's scope).  Both routes hand (sums, phase set, first index) to ht_consider (haplotag.h,
// shared with the host twin), which is independent of the order in which the phase sets arrive.  One lane per group writes the 16-byte
// result; nothing is reduced through global memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_runtime.h"
#include "haplotag.h"
#include "run_teams.h"

namespace whamd {
namespace {

constexpr int R = (int)HT_REG_PHASESETS;
constexpr int NW = RT_WAVES;
constexpr uint32_t NO_PS = RT_NONE;

struct HtArgs {
	const HtEntry* entries;
	const HtVariant* variants;
	const HtGroup* groups;      // the records of this launch's class
	HtOut* out;                 // parallel to groups
	uint32_t n_groups;
};

// The register route's phase sets (SlotNames, run_teams.h) with their sums and the index of their first matching entry.
template <int P>
struct Slots : SlotNames<R> {
	int64_t s[R][P];
	uint32_t first[R];
};

// One phase set on the pass-per-phase-set route: its sums and the index of its first matching entry.
template <int P>
struct PsAcc {
	int64_t s[P];
	uint32_t first;
	template <int W>
	__device__ void across() {
#pragma unroll
		for (int h = 0; h < P; h++) s[h] = team_sum<W>(s[h]);
		first = team_min<W>(first);
	}
	__device__ void merge(const PsAcc& o) {
#pragma unroll
		for (int h = 0; h < P; h++) s[h] += o.s[h];
		first = min(first, o.first);
	}
};

// Entry i of the run, or a no-match entry beyond it.
__device__ inline void load_entry(const HtArgs& a, const HtEntry* run, uint32_t i, uint32_t n, bool on, uint32_t& ps, uint32_t& match, int64_t& q) {
	ps = NO_PS;
	match = 0;
	q = 0;
	if (on && i < n) {
		const uint2 e = *(const uint2*)(run + i);
		const uint2 v = *(const uint2*)(a.variants + (e.x & 0x7fffffffu));
		ps = v.x;
		match = ht_match(e.x, v.y);
		q = (int64_t)(int32_t)e.y;
	}
}

// The register route over run[0, n) by the W lanes of a team (lane l of the team, the team's lanes `teammask`, its first lane `lane0`);
// index0: index, in the whole group, of run[0].  Every lane of the wave calls this together; n, index0 are the team's.
template <int P, int W>
__device__ inline void scan_run(const HtArgs& a, const HtEntry* run, uint32_t n, uint32_t index0, uint32_t l, uint64_t teammask, uint32_t lane0, Slots<P>& S) {
	S.clear();
#pragma unroll
	for (int s = 0; s < R; s++) {
		S.first[s] = 0;
#pragma unroll
		for (int h = 0; h < P; h++) S.s[s][h] = 0;
	}
	for (uint32_t base = 0; __any(base < n && !S.overflow); base += W) {   // (a team that has overflowed takes the other route: its sums are not used)
		uint32_t ps, match;
		int64_t q;
		load_entry(a, run, base + l, n, !S.overflow, ps, match, q);
		const int slot = S.claim(match != 0, ps, teammask, lane0 + l, [&](int s, uint32_t src) { S.first[s] = index0 + base + (src - lane0); });
#pragma unroll
		for (int s = 0; s < R; s++)
#pragma unroll
			for (int h = 0; h < P; h++) S.s[s][h] += (slot == s && (match >> h & 1)) ? q : 0;
	}
#pragma unroll
	for (int s = 0; s < R; s++)
		if (__any(S.n > (uint32_t)s)) {
#pragma unroll
			for (int h = 0; h < P; h++) S.s[s][h] = team_sum<W>(S.s[s][h]);
		}
}

// The pass-per-phase-set route for the owners with `need`: walk_ids over the phase sets with a matching entry; per phase set a second
// pass for its sums and first matching entry, which go to ht_consider.  Returns the number of phase sets.
template <int P, class Scope>
__device__ inline uint32_t pass_per_phase_set(const HtArgs& a, const HtEntry* run, uint32_t n, uint32_t ploidy, uint32_t l, bool need, const Scope& scope, HtBest& best) {
	const auto entry = [&](uint32_t i, uint32_t& match, int64_t& q) {
		uint32_t ps;
		load_entry(a, run, i, n, true, ps, match, q);
		return match ? ps : NO_PS;
	};
	return walk_ids(
	    scope, n, l, need,
	    [&](uint32_t i) {
		    uint32_t match;
		    int64_t q;
		    return entry(i, match, q);
	    },
	    [&](uint32_t next, bool active, uint32_t) {
		    PsAcc<P> acc;
#pragma unroll
		    for (int h = 0; h < P; h++) acc.s[h] = 0;
		    acc.first = NO_PS;
		    team_pass<Scope>(n, l, active, [&](uint32_t i) {
			    uint32_t match;
			    int64_t q;
			    if (entry(i, match, q) == next) {
				    acc.first = min(acc.first, i);
#pragma unroll
				    for (int h = 0; h < P; h++) acc.s[h] += (match >> h & 1) ? q : 0;
			    }
		    });
		    scope.combine(acc);
		    if (active) ht_consider<P>(best, acc.s, ploidy, next, acc.first);
	    });
}

// Classes a and b: W lanes per group.
template <int P, int W>
__global__ void __launch_bounds__(HT_BLOCK) haplotag_team_kernel(HtArgs a) {
	constexpr uint32_t TEAMS = HT_BLOCK / W;
	const uint32_t lane = threadIdx.x & 63u, l = threadIdx.x & (W - 1), lane0 = lane - l;
	const uint64_t teammask = (W == 64 ? ~0ull : ((1ull << W) - 1)) << lane0;
	const uint64_t g = (uint64_t)blockIdx.x * TEAMS + threadIdx.x / W;
	const bool have = g < a.n_groups;
	HtGroup grp{0, 0, 2};
	if (have) grp = a.groups[g];
	const HtEntry* run = a.entries + grp.begin;
	Slots<P> S;
	scan_run<P, W>(a, run, grp.n, 0, l, teammask, lane0, S);
	HtBest best{};
	uint32_t n_ps = 0;
	if (!S.overflow) {
#pragma unroll
		for (int s = 0; s < R; s++)
			if ((uint32_t)s < S.n) ht_consider<P>(best, S.s[s], grp.ploidy, S.ps[s], S.first[s]);
		n_ps = S.n;
	}
	if (__any(S.overflow)) n_ps += pass_per_phase_set<P>(a, run, grp.n, grp.ploidy, l, S.overflow, TeamScope<W>{}, best);
	if (have && l == 0) a.out[g] = ht_result(best, n_ps);
}

// Class c: one workgroup per group.
template <int P>
__global__ void __launch_bounds__(HT_BLOCK) haplotag_block_kernel(HtArgs a) {
	__shared__ int64_t w_sums[NW][R][P];
	__shared__ uint32_t w_ps[NW][R], w_first[NW][R], w_n[NW], w_overflow[NW];
	__shared__ PsAcc<P> r_part[NW];
	__shared__ uint32_t r_word[NW];
	__shared__ uint32_t go_slow;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const HtGroup grp = a.groups[blockIdx.x];
	const HtEntry* run = a.entries + grp.begin;
	// the waves' quarters: multiples of 64 entries, in order
	const uint32_t per = ((grp.n + NW - 1) / NW + 63u) & ~63u;
	const uint64_t b64 = (uint64_t)w * per;
	const uint32_t begin = (uint32_t)min(b64, (uint64_t)grp.n), end = (uint32_t)min(b64 + per, (uint64_t)grp.n);
	Slots<P> S;
	scan_run<P, 64>(a, run + begin, end - begin, begin, lane, ~0ull, 0, S);
	if (lane == 0) {
		w_n[w] = S.n;
		w_overflow[w] = S.overflow;
#pragma unroll
		for (int s = 0; s < R; s++) {
			w_ps[w][s] = S.ps[s];
			w_first[w][s] = S.first[s];
#pragma unroll
			for (int h = 0; h < P; h++) w_sums[w][s][h] = S.s[s][h];
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		// merge the waves' slots by phase set; more than R distinct ones: the slower route
		uint32_t m_ps[R], m_first[R], m_n = 0;
		int64_t m_sums[R][P];
		bool slow = false;
		for (int ww = 0; ww < NW && !slow; ww++) {
			if (w_overflow[ww]) slow = true;
			for (uint32_t s = 0; s < w_n[ww] && !slow; s++) {
				uint32_t at = m_n;
				for (uint32_t y = 0; y < m_n; y++)
					if (m_ps[y] == w_ps[ww][s]) at = y;
				if (at == m_n) {
					if (m_n == (uint32_t)R) {
						slow = true;
						break;
					}
					m_ps[at] = w_ps[ww][s];
					m_first[at] = w_first[ww][s];   // (the waves come in run order: the first to name a phase set saw it first)
					for (int h = 0; h < P; h++) m_sums[at][h] = 0;
					m_n++;
				}
				for (int h = 0; h < P; h++) m_sums[at][h] += w_sums[ww][s][h];
			}
		}
		go_slow = slow;
		if (!slow) {
			HtBest best{};
			for (uint32_t y = 0; y < m_n; y++) ht_consider<P>(best, m_sums[y], grp.ploidy, m_ps[y], m_first[y]);
			a.out[blockIdx.x] = ht_result(best, m_n);
		}
	}
	__syncthreads();
	if (!go_slow) return;
	HtBest best{};
	const uint32_t n_ps = pass_per_phase_set<P>(a, run, grp.n, grp.ploidy, threadIdx.x, true, BlockScope<PsAcc<P>>{r_word, r_part, lane, w}, best);
	if (threadIdx.x == 0) a.out[blockIdx.x] = ht_result(best, n_ps);
}

template <int P>
whamd_status_t launch_class(Session& s, CallTimes& times, std::string& msg, uint32_t cls, const HtArgs& a) {
	if (cls == 0) return launch(s, times, msg, haplotag_team_kernel<P, (int)HT_SEGMENT>, dim3(grid_for(a.n_groups, HT_BLOCK / HT_SEGMENT)), dim3(HT_BLOCK), 0, a);
	if (cls == 1) return launch(s, times, msg, haplotag_team_kernel<P, 64>, dim3(grid_for(a.n_groups, NW)), dim3(HT_BLOCK), 0, a);
	return launch(s, times, msg, haplotag_block_kernel<P>, dim3(a.n_groups), dim3(HT_BLOCK), 0, a);
}

}  // namespace

whamd_status_t haplotag_score_device(const std::vector<HaplotagProblem>& ps, int device, std::vector<HaplotagScores>& out, CallTimes& times,
                                     std::string& msg) {
	times = CallTimes{};
	out.assign(ps.size(), HaplotagScores{});
	// the records: groups with entries, by class, within a class in the order of the problems and of their groups
	uint64_t n_rec[3] = {0, 0, 0}, n_ent[3] = {0, 0, 0}, n_variants = 0;
	uint32_t max_ploidy[3] = {0, 0, 0};
	std::vector<uint64_t> var_base(ps.size() + 1, 0);
	for (size_t x = 0; x < ps.size(); x++) {
		const HaplotagProblem& p = ps[x];
		out[x].out.assign(p.n_groups(), HtOut{0, 0, 0});
		bool any = false;
		for (uint64_t g = 0; g < p.n_groups(); g++) {
			if (!p.group_entries[g]) continue;
			const uint32_t cls = haplotag_class_of(p.group_entries[g]);
			++n_rec[cls];
			n_ent[cls] += p.group_entries[g];
			max_ploidy[cls] = std::max(max_ploidy[cls], p.ploidy);
			any = true;
		}
		var_base[x + 1] = var_base[x] + (any ? p.variants.size() : 0);
	}
	n_variants = var_base[ps.size()];
	const uint64_t total_rec = n_rec[0] + n_rec[1] + n_rec[2], total_ent = n_ent[0] + n_ent[1] + n_ent[2];
	if (!total_rec) return WHAMD_OK;   // nothing to score: no device work at all
	if (n_variants >= 0x80000000ull || total_rec >= 0x80000000ull) {   // (the grid sizes are computed in uint32 with room to round up)
		msg = "more than 2^31 - 1 variants or groups in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	// where every record and its run go: first pass numbers them, second fills
	const uint64_t rec_base[3] = {0, n_rec[0], n_rec[0] + n_rec[1]};
	const uint64_t ent_base[3] = {0, n_ent[0], n_ent[0] + n_ent[1]};
	struct Slot { uint32_t problem; uint64_t group; uint64_t begin; };
	RawVec<Slot> slots(total_rec);
	{
		uint64_t rec_at[3] = {rec_base[0], rec_base[1], rec_base[2]}, ent_at[3] = {ent_base[0], ent_base[1], ent_base[2]};
		for (size_t x = 0; x < ps.size(); x++) {
			const HaplotagProblem& p = ps[x];
			for (uint64_t g = 0; g < p.n_groups(); g++) {
				if (!p.group_entries[g]) continue;
				const uint32_t cls = haplotag_class_of(p.group_entries[g]);
				slots[rec_at[cls]++] = Slot{(uint32_t)x, g, ent_at[cls]};
				ent_at[cls] += p.group_entries[g];
			}
		}
	}
	ImageLayout in;
	const auto p_var = in.add<HtVariant>(n_variants);
	const auto p_rec = in.add<HtGroup>(total_rec);
	const auto p_ent = in.add<HtEntry>(total_ent);
	const size_t total_out = total_rec * sizeof(HtOut);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im;
	HtOut* dev_out = nullptr;
	HtOut* res = nullptr;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.device_block(total_out, (void**)&dev_out, msg));
	WHAMD_TRY(s.pinned_block(total_out, (void**)&res, msg));
	for (size_t x = 0; x < ps.size(); x++)
		if (var_base[x + 1] > var_base[x]) std::memcpy(im.host(p_var) + var_base[x], ps[x].variants.data(), ps[x].variants.size() * sizeof(HtVariant));
	HtGroup* recs = im.host(p_rec);
	HtEntry* ents = im.host(p_ent);
	parallel_ranges(total_rec, host_threads(total_ent + total_rec, 1 << 16), [&](uint64_t b, uint64_t e, uint32_t) {
		for (uint64_t x = b; x < e; x++) {
			const Slot& sl = slots[x];
			const HaplotagProblem& p = ps[sl.problem];
			const uint32_t vb = (uint32_t)var_base[sl.problem];
			recs[x] = HtGroup{sl.begin, (uint32_t)p.group_entries[sl.group], p.ploidy};
			HtEntry* dst = ents + sl.begin;
			for (uint64_t m = p.group_ptr[sl.group]; m < p.group_ptr[sl.group + 1]; m++) {
				const uint32_t r = p.members[m];
				for (uint64_t y = p.read_ptr[r]; y < p.read_ptr[r + 1]; y++) *dst++ = HtEntry{p.entry_var[y] + vb, p.quality[y]};
			}
		}
	});
	WHAMD_TRY(s.upload(im, msg));
	for (uint32_t cls = 0; cls < 3; cls++) {
		if (!n_rec[cls]) continue;
		HtArgs a{im.dev(p_ent), im.dev(p_var), im.dev(p_rec) + rec_base[cls], dev_out + rec_base[cls], (uint32_t)n_rec[cls]};
		const uint32_t k = max_ploidy[cls];
		if (k <= 2) WHAMD_TRY(launch_class<2>(s, times, msg, cls, a));
		else if (k <= 4) WHAMD_TRY(launch_class<4>(s, times, msg, cls, a));
		else if (k <= 8) WHAMD_TRY(launch_class<8>(s, times, msg, cls, a));
		else WHAMD_TRY(launch_class<16>(s, times, msg, cls, a));
	}
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, dev_out, total_out, msg));
	WHAMD_TRY(s.finish(times, msg));
	parallel_ranges(total_rec, host_threads(total_rec, 1 << 16), [&](uint64_t b, uint64_t e, uint32_t) {
		for (uint64_t x = b; x < e; x++) out[slots[x].problem].out[slots[x].group] = res[x];
	});
	return WHAMD_OK;
}

}  // namespace whamd
