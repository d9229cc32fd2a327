// tagphase.h -- the compute of `whatshap haplotagphase`: compute_votes, consensus and best_candidate (whatshap/cli/haplotagphase.py:347-395,
// 203-263, 266-304), restated from their behaviour.  Haplotagged reads vote, per variant, for (phase set, haplotype): a counted read (phase
// set >= 0, haplotype 0 or 1) adds every entry's quality to votes[variant][(ps, hp ^ id)], id the index of the read's allele in the
// genotype vector; entries at homozygous variants do not vote.  The winner of a variant is the key with the largest sum; ties go to the
// phase set first met earliest at that variant, within a phase set to haplotype 0.
//
// The reads arrive read-major, the sums are per variant: the transposition runs on the device (tagphase_device.hip) as count, scan, place
// and one team per variant that reduces its run and decides.  The order inside a run is whatever the atomics gave; sums are integer and
// "first" is a minimum over entry indices, so every result is a function of the input alone.  The host (tagphase.cpp) validates, maps every
// problem's phase sets to dense ids (per read) and assembles the results; the debug library does the voting on one host thread with the
// same selection function (tp_consider).
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

constexpr uint32_t TP_REG_PHASESETS = 4;          // R: phase sets a team keeps in registers; a variant with more takes the pass-per-phase-set route
constexpr uint32_t TP_SEGMENT = 8;                // lanes per variant in class a (the tests read this line, so it is no alias)
static_assert(TP_SEGMENT == RS_SEGMENT, "class a teams are the shared scatter's");
constexpr uint32_t TP_CLASS_A_MAX = 64;           // class a: 0 .. 64 placed entries (at most 8 per lane of a segment)
constexpr uint32_t TP_CLASS_B_MAX = 4096;         // class b: 65 .. 4096 (one wave); class c beyond (one workgroup)
constexpr uint32_t TP_LAUNCHES = 7;               // count, scan (2), place, reduce a / b / c
constexpr uint32_t TP_LAUNCHES_TABLE = 11;        // ... and with want_table: scan of the row counts (2), rows a, rows b + c
constexpr uint32_t TP_MAX_PHASESETS = 1u << 30;   // per problem (the dense id shares a word with the haplotype)
constexpr uint32_t TP_NOT_COUNTED = 0xffffffffu;  // TpRead::code of a read that does not vote
constexpr uint32_t TP_NONE = RS_NONE;
constexpr int64_t TP_MAX_MAGNITUDE = (int64_t)1 << 53;   // sum of |quality| of a problem's voting entries: up to here (double)score / (double)total is Python's score / total

enum : uint32_t { TP_HOMOZYGOUS = 1, TP_PHASED = 2, TP_SNV = 4, TP_ONLY_INDELS = 8 };   // the word per variant: bits 0 .. 3 (bit 3: the problem's only_indels); bits 8 ..: the problem's place in the call
enum : uint32_t { TP_BEST_ID = 1, TP_VOTED = 2, TP_KEPT = 4, TP_ZERO_TOTAL = 8 };        // TpOut::flags

struct TpRead {
	uint32_t code;      // dense phase set << 1 | haplotype, TP_NOT_COUNTED: the read does not vote
	uint32_t var_base;  // first variant of the read's problem in the call
};
struct TpPlaced {
	uint32_t key;       // dense phase set << 1 | (haplotype ^ id)
	int32_t quality;
	uint32_t index;     // the entry's index in the call
};
struct alignas(16) TpOut {
	int64_t score, total;
	uint32_t best_ps;   // dense id
	uint32_t first;     // smallest index, in the call, of a voting entry (TP_NONE: none)
	uint32_t n_ps;
	uint32_t flags;
};
struct alignas(16) TpRow {
	int64_t sum0, sum1;
	uint32_t ps;        // dense id
	uint32_t first;
	uint32_t pad[2];
};

// The running choice among a variant's (phase set, haplotype) keys.
struct TpBest {
	int64_t score, total;
	uint32_t first, ps, id, n_ps, min_first;
};
WHAMD_HD inline TpBest tp_start() { return TpBest{0, 0, 0, 0, 0, 0, TP_NONE}; }

// One phase set's two sums enter the choice: the larger sum wins; equal sums go to the phase set with the smaller `first` (index of its
// first voting entry at the variant), within a phase set to haplotype 0 (the reference's stable descending sort over a dict that received
// (ps, 0), (ps, 1) when ps was first met).  Independent of the order in which the phase sets arrive.
WHAMD_HD inline void tp_consider(TpBest& b, int64_t sum0, int64_t sum1, uint32_t ps, uint32_t first) {
	const uint32_t id = sum1 > sum0 ? 1u : 0u;
	const int64_t m = id ? sum1 : sum0;
	b.total += sum0 + sum1;
	b.min_first = first < b.min_first ? first : b.min_first;
	if (!b.n_ps++ || m > b.score || (m == b.score && first < b.first)) {
		b.score = m;
		b.first = first;
		b.ps = ps;
		b.id = id;
	}
}

// The consensus filters (gap threshold and only_indels where the variant is not phased yet; the homopolymer filter can drop nothing).
WHAMD_HD inline TpOut tp_result(const TpBest& b, uint32_t info, double gap_threshold) {
	TpOut o{0, 0, 0, TP_NONE, b.n_ps, 0};
	if (!b.n_ps) return o;
	o.score = b.score;
	o.total = b.total;
	o.best_ps = b.ps;
	o.first = b.min_first;
	o.flags = TP_VOTED | (b.id ? TP_BEST_ID : 0);
	if (b.total == 0) {
		o.flags |= TP_ZERO_TOTAL;
		return o;
	}
	bool kept = true;
	if (!(info & TP_PHASED)) {
		const double fraction = (double)b.score / (double)b.total;
		if (100.0 * fraction < gap_threshold) kept = false;
		if ((info & TP_ONLY_INDELS) && (info & TP_SNV)) kept = false;
	}
	if (kept) o.flags |= TP_KEPT;
	return o;
}

// One validated problem.
struct TagphaseProblem {
	const whamd_tagphase_view* view = nullptr;
	uint64_t n_reads = 0, n_entries = 0, n_variants = 0;
	uint64_t n_skipped = 0;
	uint64_t n_voting = 0;                    // entries of counted reads at variants that are not homozygous
	std::vector<uint32_t> read_code;          // per read: TpRead::code
	std::vector<int64_t> phaseset;            // dense id -> the caller's phase set
	bool want_table = false;
};

struct TagphaseScores {
	std::vector<TpOut> out;                   // per variant; first is local to the problem
	std::vector<uint32_t> count;              // per variant: voting entries
	std::vector<uint64_t> row_ptr;            // want_table: [n_variants + 1]
	std::vector<TpRow> rows;                  // per variant in the order of the dense ids (the assembly orders them by first)
};

whamd_status_t tagphase_prepare(const whamd_tagphase_view& v, TagphaseProblem& p, std::string& msg);

// All problems of a call: one upload, TP_LAUNCHES launches (TP_LAUNCHES_TABLE with a table), whatever the problems.  No voting entry in
// the whole call: nothing touches the device (launches = 0).
whamd_status_t tagphase_device(const std::vector<TagphaseProblem>& ps, int device, std::vector<TagphaseScores>& out, CallTimes& times, std::string& msg);

}  // namespace whamd
