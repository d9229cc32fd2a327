// haplotag.h -- the assignment step of `whatshap haplotag`: prepare_haplotag_information (whatshap/cli/haplotag.py:322-427), restated from its
// behaviour.  The host (haplotag.cpp) validates, turns phase sets into dense ids and phasings into haplotype masks, forms the groups of reads
// that are scored together (the sequential part: first read of a representation seeds, linked reads of the same BX tag within the cutoff join)
// and lays every group's entries out as one contiguous run in processing order: seed first, then the other members in read-set order, each
// read's variants as listed.  The device (haplotag_device.hip) sums, per group and phase set, the qualities per haplotype and picks the
// phase set and the haplotype; the debug library does the same on one host thread with the same selection functions.
//
// What counts as "encountered": the reference creates a phase set's cost row when a haplotype first MATCHES the read's allele, so an entry
// whose allele matches no haplotype of its variant's phasing (phasing alleles outside {0, 1}, or all of the other allele) neither creates
// nor orders a phase set.  Ties between phase sets on the largest haplotype sum go to the one whose first matching entry comes first in
// the group's run.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "host_parallel.h"
#include "run_scatter.h"

#if defined(__HIPCC__)
#define WHAMD_HD __host__ __device__
#else
#define WHAMD_HD
#endif

namespace whamd {

constexpr uint32_t HT_MAX_PLOIDY = 16;
constexpr uint32_t HT_REG_PHASESETS = 4;          // R: phase sets a team keeps in registers; a group with more takes the pass-per-phase-set route
constexpr uint32_t HT_SEGMENT = 8;                // lanes per group in class a
constexpr uint32_t HT_CLASS_A_MAX = 64;           // class a: 1 .. 64 entries (at most 8 per lane of a segment)
constexpr uint32_t HT_CLASS_B_MAX = 4096;         // class b: 65 .. 4096 entries (one wave, at most 64 per lane); class c beyond (one workgroup)
constexpr uint32_t HT_BLOCK = 256;                // threads per workgroup, all classes
static_assert(HT_BLOCK == RS_BLOCK, "class c's workgroup is the shared teams' (run_teams.h BlockScope)");
constexpr uint32_t HT_MAX_PHASESETS = 1u << 27;   // per problem (the count shares a word with the haplotype in HtOut)
constexpr uint32_t HT_NO_BX = 0xffffffffu;

struct HtEntry {
	uint32_t var;      // variant index of the batch; bit 31: the read's allele
	int32_t quality;
};
struct HtVariant {
	uint32_t ps;       // phase set, dense id of its problem
	uint32_t masks;    // bit h: haplotype h carries allele 1; bit 16 + h: haplotype h carries allele 0
};
struct HtGroup {
	uint64_t begin;    // first entry
	uint32_t n;        // entries (>= 1: groups without entries never reach the device)
	uint32_t ploidy;
};
struct alignas(16) HtOut {
	int64_t quality;   // best - second best haplotype sum of the winning phase set; 0: unassigned
	uint32_t ps;       // the winning phase set
	uint32_t hap_nps;  // bits 0 .. 4: haplotype + 1 (0: unassigned); bits 5 ..: phase sets with a matching entry
};

// The running choice among a group's phase sets.
struct HtBest {
	int64_t max, quality;
	uint32_t first, ps;
	int32_t hap;
	uint32_t any;
};

// One phase set's sums enter the choice: larger maximum wins, equal maxima go to the smaller `first` (index, in the group's run, of its
// first matching entry).  Best haplotype: lowest index among the maxima; second: the maximum of the others (the next of a stable
// descending sort).
template <int P>
WHAMD_HD inline void ht_consider(HtBest& b, const int64_t (&sums)[P], uint32_t ploidy, uint32_t ps, uint32_t first) {
	int64_t m = sums[0];
	int32_t hap = 0;
#pragma unroll
	for (int h = 1; h < P; h++)
		if ((uint32_t)h < ploidy && sums[h] > m) {
			m = sums[h];
			hap = h;
		}
	if (b.any && !(m > b.max || (m == b.max && first < b.first))) return;
	int64_t second = INT64_MIN;
#pragma unroll
	for (int h = 0; h < P; h++)
		if ((uint32_t)h < ploidy && h != hap && sums[h] > second) second = sums[h];
	b.max = m;
	b.quality = (int64_t)((uint64_t)m - (uint64_t)second);
	b.first = first;
	b.ps = ps;
	b.hap = hap;
	b.any = 1;
}

WHAMD_HD inline HtOut ht_result(const HtBest& b, uint32_t n_ps) {
	HtOut o;
	const bool assigned = b.any && b.quality != 0;
	o.quality = assigned ? b.quality : 0;
	o.ps = b.any ? b.ps : 0;
	o.hap_nps = (n_ps << 5) | (assigned ? (uint32_t)b.hap + 1 : 0);
	return o;
}

// The haplotypes an entry adds its quality to.
WHAMD_HD inline uint32_t ht_match(uint32_t entry_var, uint32_t masks) { return (entry_var >> 31) ? (masks & 0xffffu) : (masks >> 16); }

// One validated problem: variants, the groups in processing order and their members.
struct HaplotagProblem {
	uint32_t ploidy = 0;
	uint64_t n_reads = 0, n_entries = 0;
	const uint64_t* read_ptr = nullptr;       // the caller's
	const int32_t* quality = nullptr;         // the caller's, per entry in read order
	const int64_t* read_start = nullptr;      // the caller's
	RawVec<uint32_t> entry_var;               // per entry in read order: variant index of the problem, bit 31 the allele
	std::vector<HtVariant> variants;
	std::vector<int64_t> phaseset;            // dense id -> the caller's phase set
	std::vector<uint64_t> group_ptr;          // [n_groups + 1] into members
	RawVec<uint32_t> members;                 // read indices: seed first, then read-set order
	RawVec<uint32_t> group_bx;                // the seed's BX id where the group was formed as a linked-read group, else HT_NO_BX
	RawVec<uint64_t> group_entries;           // entries of all members
	uint64_t n_groups() const { return group_bx.size(); }
};

struct HaplotagScores {
	RawVec<HtOut> out;                        // per group (groups without entries: zeros)
};

whamd_status_t haplotag_prepare(const whamd_haplotag_view& v, HaplotagProblem& p, std::string& msg);

// The class boundaries of the call in progress: HT_CLASS_A_MAX / HT_CLASS_B_MAX.  In the debug library only, every call re-reads them from
// WHAMD_HT_CLASS_A_MAX / WHAMD_HT_CLASS_B_MAX first (scripts/gpu_haplotag_bench.py --sweep: every kernel is correct for any group size, so the
// boundaries are a matter of speed alone).
struct HtBounds { uint32_t a_max, b_max; };
const HtBounds& haplotag_bounds();
inline uint32_t haplotag_class_of(uint64_t n_entries) {
	const HtBounds& b = haplotag_bounds();
	return n_entries <= b.a_max ? 0 : n_entries <= b.b_max ? 1 : 2;
}

// All problems of a call: one upload, one launch per class that has groups (at most three, whatever the number of problems), one download.
// Nothing to score: nothing touches the device (launches = 0).
whamd_status_t haplotag_score_device(const std::vector<HaplotagProblem>& ps, int device, std::vector<HaplotagScores>& out, CallTimes& times,
                                     std::string& msg);

}  // namespace whamd
