// readmerge_device.hip -- the pairs and the sums of the read merging on gfx950 (readmerge.h).
//   pairs     One lane per pair (j, i), pairs numbered in ascending (j, i): the lanes of a wave hold neighbouring pairs, mostly one j with
//             consecutive i -- j's words are one address for the wave, the i's lie next to each other in the packed array.  A lane walks
//             the overlap's words: j's funnel-shifted by start mod 64, XOR, the tail word masked, popcount (rm_mismatches, shared with the
//             host twin).  Long reads carry tens to a few hundred variants, so a pair is a handful of words: a wave per j with j's words
//             in registers would leave most of its lanes without a word.
//   flags     one thread per pair: its read j by search in pair_ptr, mismatches, the three tests (one IEEE f64 division) -- 0 / 1 per
//             pair (the scan's input) and the mismatches.
//   scan      the shared two-launch exclusive scan (run_scatter.hip), the total being the number of edges; the host waits for it once to
//             size the edge list.
//   edges     one thread per pair again: a blue pair writes {j, i, match, mismatch, flags} at its prefix.  The list is in ascending
//             (j, i) and no atomic decides any of it.
//   first     the entries of the merged reads lie component by component, member by member, a member's ascending in position.  One
//             thread per entry: it is flagged unless an earlier entry of its component has its position (a binary search per earlier
//             member).  A flagged entry is a slot: "touched" comes from the positions, never from a sum.
//   scan      of the flags, the shared one again; the total is the number of superread entries.
//   place     one thread per entry: its slot is the component's first slot plus the flagged entries of the component at smaller
//             positions (per member a search; the scan turns the place into the count), so a superread's positions ascend.  An integer
//             atomic adds the quality to the slot's sum of the allele.
//   decide    one thread per slot: allele and quality.
// RM_LAUNCHES_PAIRS + RM_LAUNCHES_SUMS launches per call, whatever the problems; a stage without work launches nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_runtime.h"
#include "readmerge.h"
#include "run_teams.h"

namespace whamd {
namespace {

struct RmPairArgs {
	// the image
	const RmRead* reads;          // [n_reads] word: in the call
	const uint64_t* words;        // [n_words]
	const uint32_t* pair_ptr;     // [n_reads + 1]
	const uint32_t* read_problem; // [n_reads] the problem's place among the call's
	const RmThresholds* thr;      // [problems of the call]
	// made on the device
	uint32_t* blue;               // [n_pairs] 0 / 1
	uint32_t* mismatch;           // [n_pairs]
	uint32_t* local;              // [n_pairs] the scan
	uint32_t* tile_sums;
	uint32_t* n_edges;            // [1]
	RmEdge* edges;
	uint32_t n_reads, n_pairs, edge_room;
};

__global__ void __launch_bounds__(RS_BLOCK) readmerge_flags_kernel(RmPairArgs a) {
	const uint32_t p = blockIdx.x * RS_BLOCK + threadIdx.x;
	if (p >= a.n_pairs) return;
	const uint32_t j = read_of_entry(a.pair_ptr, a.n_reads, a.n_pairs, p);
	const uint32_t i = j + 1 + (p - a.pair_ptr[j]);
	if (i >= a.n_reads) return;   // (never: the pairs of j end at hi_j)
	const RmRead rj = a.reads[j], ri = a.reads[i];
	uint32_t start;
	const uint32_t L = rm_overlap(rj, ri, start);
	const uint32_t mismatch = rm_mismatches(a.words, rj, ri, start, L);
	a.mismatch[p] = mismatch;
	a.blue[p] = rm_flags(L, mismatch, a.thr[a.read_problem[j]]) ? 1u : 0u;
}

__global__ void __launch_bounds__(RS_BLOCK) readmerge_edges_kernel(RmPairArgs a) {
	const uint32_t p = blockIdx.x * RS_BLOCK + threadIdx.x;
	if (p >= a.n_pairs || !a.blue[p]) return;
	const uint32_t j = read_of_entry(a.pair_ptr, a.n_reads, a.n_pairs, p);
	const uint32_t i = j + 1 + (p - a.pair_ptr[j]);
	if (i >= a.n_reads) return;
	uint32_t start;
	const uint32_t L = rm_overlap(a.reads[j], a.reads[i], start);
	const uint32_t mismatch = a.mismatch[p];
	const uint32_t at = run_begin(a.local, a.tile_sums, p);
	if (at < a.edge_room) a.edges[at] = RmEdge{j, i, L - mismatch, mismatch, rm_flags(L, mismatch, a.thr[a.read_problem[j]])};
}

// The merged components' entries, component by component, member by member, every member's entries ascending in position.
struct RmComp {
	uint32_t member_begin, member_end;   // into members
	uint32_t entry_begin;                // its first entry
};
struct RmMember {
	uint32_t entry_begin, len, comp;
};
struct RmSumArgs {
	// the image
	const RmComp* comps;
	const RmMember* members;
	const uint32_t* member_ptr;   // [n_members + 1] every member's first entry: the search for an entry's member
	const int64_t* position;      // [n_entries]
	const uint8_t* allele;
	const int64_t* quality;
	// made on the device
	uint32_t* first;              // [n_entries] 1: no earlier entry of the component has the position
	uint32_t* local;              // the scan of first
	uint32_t* tile_sums;
	uint32_t* n_slots;            // [1]
	uint32_t* comp_base;          // [n_comps] the component's first slot
	unsigned long long* sums;     // [n_entries][2] (room for a slot per entry) zero before place
	int64_t* slot_position;       // [n_entries]
	uint8_t* out_allele;
	int64_t* out_quality;
	uint32_t n_entries, n_members;
};

// The first entry of member m at a position >= p (the member's end: none).
__device__ inline uint32_t member_lower(const RmSumArgs& a, const RmMember& m, int64_t p) {
	uint32_t lo = m.entry_begin, hi = m.entry_begin + m.len;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (a.position[mid] < p) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// Flagged entries in front of entry x (x == n_entries: all of them).
__device__ inline uint32_t flagged_before(const RmSumArgs& a, uint32_t x) { return x < a.n_entries ? run_begin(a.local, a.tile_sums, x) : a.n_slots[0]; }

// One thread per entry: is it the first of its component at its position, in the order component, member, entry?
__global__ void __launch_bounds__(RS_BLOCK) readmerge_first_kernel(RmSumArgs a) {
	const uint32_t x = blockIdx.x * RS_BLOCK + threadIdx.x;
	if (x >= a.n_entries) return;
	const uint32_t m = read_of_entry(a.member_ptr, a.n_members, a.n_entries, x);
	const RmMember mine = a.members[m];
	const int64_t p = a.position[x];
	bool first = !(x > mine.entry_begin && a.position[x - 1] == p);
	for (uint32_t o = a.comps[mine.comp].member_begin; first && o < m; o++) {
		const RmMember other = a.members[o];
		const uint32_t k = member_lower(a, other, p);
		first = !(k < other.entry_begin + other.len && a.position[k] == p);
	}
	a.first[x] = first ? 1u : 0u;
}

// One thread per entry again: its slot is its component's first slot plus the flagged entries of the component at smaller positions --
// per member a search, the scan gives the count.  The quality goes to the slot's sum of the allele; the flagged entry names the slot's
// position, the component's first entry the component's first slot.
__global__ void __launch_bounds__(RS_BLOCK) readmerge_place_kernel(RmSumArgs a) {
	const uint32_t x = blockIdx.x * RS_BLOCK + threadIdx.x;
	if (x >= a.n_entries) return;
	const uint32_t m = read_of_entry(a.member_ptr, a.n_members, a.n_entries, x);
	const RmMember mine = a.members[m];
	const RmComp comp = a.comps[mine.comp];
	const int64_t p = a.position[x];
	uint32_t slot = flagged_before(a, comp.entry_begin);
	if (x == comp.entry_begin) a.comp_base[mine.comp] = slot;
	for (uint32_t o = comp.member_begin; o < comp.member_end; o++) {
		const RmMember other = a.members[o];
		slot += flagged_before(a, member_lower(a, other, p)) - flagged_before(a, other.entry_begin);
	}
	if (slot >= a.n_entries) return;   // (never: a component has at most as many positions as entries)
	atomicAdd(a.sums + 2ull * slot + (a.allele[x] & 1u), (unsigned long long)a.quality[x]);   // (two's complement: the sum of the int64 values)
	if (a.first[x]) a.slot_position[slot] = p;
}

__global__ void __launch_bounds__(RS_BLOCK) readmerge_decide_kernel(RmSumArgs a) {
	const uint32_t s = blockIdx.x * RS_BLOCK + threadIdx.x;
	if (s >= a.n_slots[0] || s >= a.n_entries) return;
	uint8_t allele;
	int64_t quality;
	rm_decide((int64_t)a.sums[2ull * s], (int64_t)a.sums[2ull * s + 1], allele, quality);
	a.out_allele[s] = allele;
	a.out_quality[s] = quality;
}

}  // namespace

whamd_status_t readmerge_pairs_device(const std::vector<ReadmergeProblem>& ps, int device, std::vector<ReadmergeScores>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	// the problems with a pair are the call's: their reads, words and pairs one after the other
	std::vector<uint64_t> read_base(ps.size() + 1, 0), word_base(ps.size() + 1, 0), pair_base(ps.size() + 1, 0), slot(ps.size() + 1, 0);
	for (size_t x = 0; x < ps.size(); x++) {
		const bool in = !ps[x].given && ps[x].n_pairs > 0;
		read_base[x + 1] = read_base[x] + (in ? ps[x].n_reads : 0);
		word_base[x + 1] = word_base[x] + (in ? ps[x].n_words : 0);
		pair_base[x + 1] = pair_base[x] + (in ? ps[x].n_pairs : 0);
		slot[x + 1] = slot[x] + (in ? 1 : 0);
	}
	const uint64_t n_reads = read_base[ps.size()], n_words = word_base[ps.size()], n_pairs = pair_base[ps.size()], n_in = slot[ps.size()];
	if (!n_pairs) return WHAMD_OK;   // no pair in the whole call: nothing touches the device
	if (n_reads >= RM_MAX_COUNT || n_words >= RM_MAX_COUNT || n_pairs >= RM_MAX_COUNT) {
		msg = "2^32 - 4096 or more reads, entries or pairs in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	ImageLayout in;
	const auto p_reads = in.add<RmRead>(n_reads);
	const auto p_words = in.add<uint64_t>(n_words);
	const auto p_pairs = in.add<uint32_t>(n_reads + 1);
	const auto p_problem = in.add<uint32_t>(n_reads);
	const auto p_thr = in.add<RmThresholds>(n_in);
	ImageLayout work;
	const auto w_blue = work.add<uint32_t>(n_pairs);
	const auto w_mismatch = work.add<uint32_t>(n_pairs);
	const auto w_local = work.add<uint32_t>(n_pairs);
	const auto w_tiles = work.add<uint32_t>(rs_tiles(n_pairs));
	const auto w_n_edges = work.add<uint32_t>(1);
	ImageLayout results;
	const auto r_n_edges = results.add<uint32_t>(1);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, wk, res, table;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.work(work, wk, msg));
	WHAMD_TRY(s.results(results, res, msg));
	for (size_t x = 0; x < ps.size(); x++) {
		const ReadmergeProblem& p = ps[x];
		if (p.given || !p.n_pairs) continue;
		im.host(p_thr)[slot[x]] = p.thr;
		RmRead* reads = im.host(p_reads) + read_base[x];
		uint32_t* pairs = im.host(p_pairs) + read_base[x];
		uint32_t* problem = im.host(p_problem) + read_base[x];
		for (uint64_t r = 0; r < p.n_reads; r++) {
			reads[r] = RmRead{p.reads[r].begin, p.reads[r].len, (uint32_t)(word_base[x] + p.reads[r].word)};
			pairs[r] = (uint32_t)(pair_base[x] + p.pair_ptr[r]);
			problem[r] = (uint32_t)slot[x];
		}
		std::memcpy(im.host(p_words) + word_base[x], p.words.data(), p.n_words * sizeof(uint64_t));
	}
	im.host(p_pairs)[n_reads] = (uint32_t)n_pairs;
	WHAMD_TRY(s.upload(im, msg));
	RmPairArgs a{};
	a.reads = im.dev(p_reads);
	a.words = im.dev(p_words);
	a.pair_ptr = im.dev(p_pairs);
	a.read_problem = im.dev(p_problem);
	a.thr = im.dev(p_thr);
	a.blue = wk.dev_out(w_blue);
	a.mismatch = wk.dev_out(w_mismatch);
	a.local = wk.dev_out(w_local);
	a.tile_sums = wk.dev_out(w_tiles);
	a.n_edges = wk.dev_out(w_n_edges);
	a.edges = nullptr;
	a.n_reads = (uint32_t)n_reads;
	a.n_pairs = (uint32_t)n_pairs;
	a.edge_room = 0;
	const dim3 per_pair(grid_for(n_pairs, RS_BLOCK));
	WHAMD_TRY(rs_launch(s, times, msg, readmerge_flags_kernel, per_pair, a));
	WHAMD_TRY(rs_scan(s, times, msg, a.blue, a.local, a.tile_sums, a.n_pairs, nullptr, a.n_edges));
	WHAMD_TRY(s.fetch_now(res, r_n_edges, a.n_edges, msg));   // the edge list's size
	const uint64_t n_edges = *res.host(r_n_edges);
	if (n_edges > n_pairs) {
		msg = "internal error: more blue edges than pairs";
		return WHAMD_ERR_DEVICE;
	}
	ImageLayout edge_layout;   // the second result image: sized by the wait
	const auto r_edges = edge_layout.add<RmEdge>(n_edges);
	WHAMD_TRY(s.stage(edge_layout, table, msg));
	a.edges = table.dev_out(r_edges);
	a.edge_room = (uint32_t)n_edges;
	WHAMD_TRY(rs_launch(s, times, msg, readmerge_edges_kernel, per_pair, a));   // (also without an edge: the launches of a call are a constant)
	WHAMD_TRY(s.kernels_done(msg));
	if (n_edges) WHAMD_TRY(s.fetch(table, r_edges, a.edges, msg));
	WHAMD_TRY(s.finish(times, msg));
	// back to the problems: the edges of a problem are those whose j is one of its reads; ids become local
	const RmEdge* edges = table.host(r_edges);
	uint64_t at = 0;
	for (size_t x = 0; x < ps.size(); x++) {
		if (ps[x].given || !ps[x].n_pairs) continue;
		const uint64_t lo = read_base[x], hi = read_base[x + 1];
		while (at < n_edges && edges[at].j < hi) {
			const RmEdge& e = edges[at++];
			if (e.j < lo || e.i < lo || e.i >= hi || e.j >= e.i) {
				msg = "internal error: an edge outside its problem";
				return WHAMD_ERR_DEVICE;
			}
			out[x].edges.push_back(RmEdge{(uint32_t)(e.j - lo), (uint32_t)(e.i - lo), e.match, e.mismatch, e.flags});
		}
	}
	if (at != n_edges) {
		msg = "internal error: the edge list and the problems disagree";
		return WHAMD_ERR_DEVICE;
	}
	return WHAMD_OK;
}

whamd_status_t readmerge_sums_device(const std::vector<ReadmergeProblem>& ps, int device, std::vector<ReadmergeScores>& out, CallTimes& times, std::string& msg) {
	times = CallTimes{};
	for (size_t x = 0; x < ps.size(); x++) out[x].super_ptr.assign(ps[x].n_reads + 1, 0);
	std::vector<uint64_t> ent_base(ps.size() + 1, 0), mem_base(ps.size() + 1, 0), comp_base(ps.size() + 1, 0);
	for (size_t x = 0; x < ps.size(); x++) {
		ent_base[x + 1] = ent_base[x] + out[x].n_merged_entries;
		mem_base[x + 1] = mem_base[x] + out[x].members.size();
		comp_base[x + 1] = comp_base[x] + out[x].merged_reps.size();
	}
	const uint64_t n_entries = ent_base[ps.size()], n_members = mem_base[ps.size()], n_comps = comp_base[ps.size()];
	if (!n_entries) return WHAMD_OK;   // no read is merged: nothing touches the device
	if (n_entries >= RM_MAX_COUNT) {
		msg = "2^32 - 4096 or more entries of merged reads in one call";
		return WHAMD_ERR_UNSUPPORTED;
	}
	ImageLayout in;
	const auto p_comps = in.add<RmComp>(n_comps);
	const auto p_members = in.add<RmMember>(n_members);
	const auto p_member_ptr = in.add<uint32_t>(n_members + 1);
	const auto p_position = in.add<int64_t>(n_entries);
	const auto p_quality = in.add<int64_t>(n_entries);
	const auto p_allele = in.add<uint8_t>(n_entries);
	ImageLayout work;
	const auto w_sums = work.add<unsigned long long>(2 * n_entries);
	const size_t zeroed = work.total;
	const auto w_first = work.add<uint32_t>(n_entries);
	const auto w_local = work.add<uint32_t>(n_entries);
	const auto w_tiles = work.add<uint32_t>(rs_tiles(n_entries));
	const auto w_n_slots = work.add<uint32_t>(1);
	const auto w_comp_base = work.add<uint32_t>(n_comps);
	const auto w_position = work.add<int64_t>(n_entries);
	const auto w_allele = work.add<uint8_t>(n_entries);
	const auto w_quality = work.add<int64_t>(n_entries);
	ImageLayout results;
	const auto r_n_slots = results.add<uint32_t>(1);
	const auto r_comp_base = results.add<uint32_t>(n_comps);
	Session s;
	WHAMD_TRY(s.open(device, 4, msg));
	Image im, wk, res, slots;
	WHAMD_TRY(s.stage(in, im, msg));
	WHAMD_TRY(s.work(work, wk, msg));
	WHAMD_TRY(s.results(results, res, msg));
	// the image: a member's entries as the caller holds them if they ascend in position, else sorted (stable) by it
	std::vector<uint64_t> order;
	for (size_t x = 0; x < ps.size(); x++) {
		const whamd_readmerge_view& v = *ps[x].view;
		const ReadmergeScores& sc = out[x];
		uint64_t at = ent_base[x];
		for (size_t c = 0; c < sc.merged_reps.size(); c++) {
			im.host(p_comps)[comp_base[x] + c] = RmComp{(uint32_t)(mem_base[x] + sc.member_ptr[c]), (uint32_t)(mem_base[x] + sc.member_ptr[c + 1]), (uint32_t)at};
			for (uint64_t m = sc.member_ptr[c]; m < sc.member_ptr[c + 1]; m++) {
				const uint64_t b = v.read_ptr[sc.members[m]], len = v.read_ptr[sc.members[m] + 1] - b;
				im.host(p_members)[mem_base[x] + m] = RmMember{(uint32_t)at, (uint32_t)len, (uint32_t)(comp_base[x] + c)};
				im.host(p_member_ptr)[mem_base[x] + m] = (uint32_t)at;
				order.resize(len);
				for (uint64_t k = 0; k < len; k++) order[k] = b + k;
				if (!std::is_sorted(v.entry_position + b, v.entry_position + b + len))
					std::stable_sort(order.begin(), order.end(), [&](uint64_t l, uint64_t r) { return v.entry_position[l] < v.entry_position[r]; });
				for (uint64_t k = 0; k < len; k++) {
					im.host(p_position)[at + k] = v.entry_position[order[k]];
					im.host(p_quality)[at + k] = v.entry_quality[order[k]];
					im.host(p_allele)[at + k] = v.entry_allele[order[k]];
				}
				at += len;
			}
		}
	}
	im.host(p_member_ptr)[n_members] = (uint32_t)n_entries;
	WHAMD_TRY(s.upload(im, msg));
	WHAMD_TRY(s.zero(wk, zeroed, msg));
	RmSumArgs a{};
	a.comps = im.dev(p_comps);
	a.members = im.dev(p_members);
	a.member_ptr = im.dev(p_member_ptr);
	a.position = im.dev(p_position);
	a.allele = im.dev(p_allele);
	a.quality = im.dev(p_quality);
	a.first = wk.dev_out(w_first);
	a.local = wk.dev_out(w_local);
	a.tile_sums = wk.dev_out(w_tiles);
	a.n_slots = wk.dev_out(w_n_slots);
	a.comp_base = wk.dev_out(w_comp_base);
	a.sums = wk.dev_out(w_sums);
	a.slot_position = wk.dev_out(w_position);
	a.out_allele = wk.dev_out(w_allele);
	a.out_quality = wk.dev_out(w_quality);
	a.n_entries = (uint32_t)n_entries;
	a.n_members = (uint32_t)n_members;
	const dim3 per_entry(grid_for(n_entries, RS_BLOCK));
	WHAMD_TRY(rs_launch(s, times, msg, readmerge_first_kernel, per_entry, a));
	WHAMD_TRY(rs_scan(s, times, msg, a.first, a.local, a.tile_sums, a.n_entries, nullptr, a.n_slots));
	WHAMD_TRY(rs_launch(s, times, msg, readmerge_place_kernel, per_entry, a));
	WHAMD_TRY(rs_launch(s, times, msg, readmerge_decide_kernel, per_entry, a));   // (a slot per entry at most; the kernel reads the count)
	WHAMD_TRY(s.kernels_done(msg));
	WHAMD_TRY(s.fetch(res, r_comp_base, a.comp_base, msg));
	WHAMD_TRY(s.fetch_now(res, r_n_slots, a.n_slots, msg));   // the superreads' size
	const uint64_t n_slots = *res.host(r_n_slots);
	if (n_slots > n_entries || n_slots < n_comps) {
		msg = "internal error: the superreads' entries and the merged reads' entries disagree";
		return WHAMD_ERR_DEVICE;
	}
	ImageLayout slot_layout;   // the second result image: sized by the wait
	const auto r_sums = slot_layout.add<unsigned long long>(2 * n_slots);
	const auto r_position = slot_layout.add<int64_t>(n_slots);
	const auto r_allele = slot_layout.add<uint8_t>(n_slots);
	const auto r_quality = slot_layout.add<int64_t>(n_slots);
	WHAMD_TRY(s.results(slot_layout, slots, msg));
	WHAMD_TRY(s.fetch(slots, r_sums, a.sums, msg));
	WHAMD_TRY(s.fetch(slots, r_position, a.slot_position, msg));
	WHAMD_TRY(s.fetch(slots, r_allele, a.out_allele, msg));
	WHAMD_TRY(s.fetch(slots, r_quality, a.out_quality, msg));
	WHAMD_TRY(s.finish(times, msg));
	// back to the problems: a component's slots run from its base to the next one's
	const uint32_t* base = res.host(r_comp_base);
	for (size_t x = 0; x < ps.size(); x++) {
		ReadmergeScores& sc = out[x];
		if (sc.merged_reps.empty()) continue;
		const uint64_t lo = base[comp_base[x]], hi = comp_base[x + 1] < n_comps ? base[comp_base[x + 1]] : n_slots;
		if (lo > hi || hi > n_slots) {
			msg = "internal error: the components' first slots do not ascend";
			return WHAMD_ERR_DEVICE;
		}
		for (size_t c = 0; c < sc.merged_reps.size(); c++) {
			const uint64_t b = base[comp_base[x] + c], e = comp_base[x] + c + 1 < n_comps ? base[comp_base[x] + c + 1] : n_slots;
			if (b < lo || e < b || e > hi) {
				msg = "internal error: the components' first slots do not ascend";
				return WHAMD_ERR_DEVICE;
			}
			sc.super_ptr[sc.merged_reps[c] + 1] = e - b;
		}
		for (uint64_t r = 0; r < ps[x].n_reads; r++) sc.super_ptr[r + 1] += sc.super_ptr[r];
		const unsigned long long* sums = slots.host(r_sums);
		sc.sums.resize(2 * (hi - lo));
		for (uint64_t k = 0; k < 2 * (hi - lo); k++) sc.sums[k] = (int64_t)sums[2 * lo + k];
		sc.slot_position.assign(slots.host(r_position) + lo, slots.host(r_position) + hi);
		sc.allele.assign(slots.host(r_allele) + lo, slots.host(r_allele) + hi);
		sc.quality.assign(slots.host(r_quality) + lo, slots.host(r_quality) + hi);
	}
	return WHAMD_OK;
}

}  // namespace whamd
