// realign.h -- allele detection by re-alignment (ReadSetReader.realign / detect_alleles_by_alignment, whatshap/variants.py:685-912).
// The host walks the CIGARs (realign.cpp: _iterate_cigar, split_cigar_left / _right, cigar_prefix_length and the window arithmetic of
// realign) and writes one 32-byte descriptor per (alignment, variant) job; the allele windows are never built on the host: allele 0 is
// the reference window itself, allele a > 0 is left pad + alt bytes + right pad, read by the kernels straight from the uploaded
// reference slice and the alt bytes (Target below).  realign_device.hip computes the distances and the decision per job.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whatshap_amd.h"
#include "call_image.h"
#include "host_parallel.h"

namespace whamd {

struct RealignJob {
	uint64_t q_off;       // the query window: bytes q_off .. q_off + q_len - 1 of the uploaded window buffer
	uint64_t win_start;   // variant.position - left_ref_bases, relative to the uploaded reference slice
	uint32_t q_len;
	uint32_t variant;
	uint32_t left;        // left_ref_bases: length of the left pad
	uint32_t right;       // right_ref_bases: allele 0 is reference[win_start, win_start + left + right)
};
static_assert(sizeof(RealignJob) == 32, "one descriptor is 32 bytes");

struct RealignVariant {
	uint32_t ref_len;     // len(variant.reference_allele)
	uint32_t allow_off;   // the alleles realign compares, in index order: allow[allow_off .. allow_off + allow_n - 1]
	uint32_t allow_n;
	uint32_t alt_first;   // alt allele a (1-based) has bytes alt_off[alt_first + a - 1] .. alt_off[alt_first + a] - 1
};

// A padded allele window as three byte ranges: s1 (reference), s2 (alt allele), s3 (reference).
struct Target {
	const uint8_t* s1;
	const uint8_t* s2;
	const uint8_t* s3;
	uint32_t l1, l2, l3;
	__host__ __device__ uint32_t len() const { return l1 + l2 + l3; }
	__host__ __device__ uint8_t at(uint32_t j) const {
		if (j < l1) return s1[j];
		j -= l1;
		if (j < l2) return s2[j];
		return s3[j - l2];
	}
};

__host__ __device__ inline Target allele_target(const RealignJob& job, const RealignVariant& v, uint32_t allele, const uint8_t* ref,
                                                const uint64_t* alt_off, const uint8_t* alt_bytes) {
	Target t;
	const uint8_t* w = ref + job.win_start;
	if (allele == 0) {
		t.s1 = w; t.l1 = job.left + job.right;
		t.s2 = w; t.l2 = 0;
		t.s3 = w; t.l3 = 0;
		return t;
	}
	const uint64_t a0 = alt_off[v.alt_first + allele - 1], a1 = alt_off[v.alt_first + allele];
	t.s1 = w; t.l1 = job.left;
	t.s2 = alt_bytes + a0; t.l2 = (uint32_t)(a1 - a0);
	t.s3 = w + job.left + v.ref_len; t.l3 = job.right > v.ref_len ? job.right - v.ref_len : 0;   // reference[pos + len(ref) : pos + right]
	return t;
}

// f(l) = gap_start + (l - 1) * gap_extend (align.pyx:100-101), a Python int stored into the float table (through a double)
__host__ __device__ inline float affine_gap_f(int64_t l, int32_t gap_start, int32_t gap_extend) {
	return (float)(double)((int64_t)gap_start + (l - 1) * (int64_t)gap_extend);
}
constexpr float AFFINE_INF = 2147483648.0f;   // limits.INT_MAX stored as a float

// What the host walk hands the device: descriptors and query windows per walk range (alignment order), the variant tables.
struct RealignBatch {
	std::vector<RawVec<RealignJob>> range_jobs;
	std::vector<RawVec<uint8_t>> range_query;
	std::vector<uint64_t> range_job_base, range_query_base;   // where range r's jobs / bytes start in the concatenation
	std::vector<RawVec<uint32_t>> range_long;                  // jobs of range r whose query is longer than 64 (index within the range)
	std::vector<uint64_t> range_long_base;
	std::vector<uint32_t> jobs_of;                             // [n_alignments] jobs per alignment
	uint64_t n_jobs = 0, n_query_bytes = 0, n_pairs = 0, n_long = 0;
	uint32_t max_target_long = 0;                              // longest allele window of a job whose query is longer than 64 (what sizes the scratch rows)
	std::vector<RealignVariant> variants;
	std::vector<uint64_t> alt_off;
	std::vector<uint32_t> allow;
	const uint8_t* alt_bytes = nullptr;
	uint64_t n_alt_bytes = 0;
	const uint8_t* ref = nullptr;    // the caller's slice
	uint64_t ref_len = 0;
	whamd_realign_params params{};
};

// The host walk (realign.cpp).  WHAMD_ERR_INVALID with the reference's exception in `msg` (see whatshap_amd.h).
whamd_status_t realign_walk(const whamd_realign_alignments_view& al, const whamd_realign_variants_view& var,
                            const whamd_realign_reference_view& ref, const whamd_realign_params& params, RealignBatch& out,
                            std::string& msg);

// Distances and decisions on `device` (realign_device.hip): allele_out[job] = the detected allele or -1, quality_out[job] (affine: d0 - d1 or
// d0; unit: 30).  Times in ms of HIP events.
whamd_status_t realign_device(const RealignBatch& b, int device, int32_t* allele_out, int64_t* quality_out, CallTimes& times,
                              std::string& msg);

whamd_status_t edit_distance_device(uint64_t n_pairs, const uint64_t* query_ptr, const uint8_t* query, const uint64_t* target_ptr,
                                    const uint8_t* target, int use_affine, const float* mismatch_cost, int32_t gap_start, int32_t gap_extend,
                                    int device, int64_t* distance_out, std::string& msg);

}  // namespace whamd
