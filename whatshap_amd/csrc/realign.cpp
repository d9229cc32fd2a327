// realign.cpp -- the host side of allele detection by re-alignment: the CIGAR walk of _iterate_cigar (whatshap/_variants.pyx:10-81) and the
// window construction of ReadSetReader.realign (split_cigar_left / split_cigar_right / cigar_prefix_length, whatshap/variants.py:597-683,
// :731-847), restated from their behaviour, on a few host threads (one range of alignments each); the C ABI of whatshap_amd.h's realign
// section; and, in the debug library only, the host restatement of both distances and of the decision (whamd_debug_*).
#include "realign.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/whatshap_amd_debug.h"
#include "api_guard.h"
#include "debug_build.h"
#include "realign_shape.h"

using namespace whamd;

namespace {

bool is_match_op(uint32_t op) { return op == 0 || op == 7 || op == 8; }   // M, =, X

// cigar_prefix_length over a split iterator: `next(k, op, len)` gives the k-th element or false at the end.
template <class Next>
bool cigar_prefix_length(Next&& next, int64_t reference_bases, int64_t& ref_out, int64_t& query_out, std::string& msg) {
	int64_t ref_pos = 0, query_pos = 0;
	uint32_t op = 0;
	int64_t length = 0;
	for (uint64_t k = 0; next(k, op, length); ++k) {
		if (is_match_op(op)) {
			ref_pos += length;
			query_pos += length;
			if (ref_pos >= reference_bases) { ref_out = reference_bases; query_out = query_pos + reference_bases - ref_pos; return true; }
		} else if (op == 2) {
			ref_pos += length;
			if (ref_pos >= reference_bases) { ref_out = reference_bases; query_out = query_pos; return true; }
		} else if (op == 1) {
			query_pos += length;
		} else if (op == 4 || op == 5) {
		} else if (op == 3) {
			ref_out = reference_bases; query_out = query_pos;   // reference skips end the read
			return true;
		} else {
			msg = "AssertionError: unknown CIGAR operator";
			return false;
		}
	}
	if (!(ref_pos < reference_bases)) { msg = "AssertionError: assert ref_pos < reference_bases"; return false; }
	ref_out = ref_pos;
	query_out = query_pos;
	return true;
}

struct Walker {
	const whamd_realign_alignments_view& al;
	const whamd_realign_variants_view& var;
	const whamd_realign_reference_view& ref;
	const whamd_realign_params& params;
	const RealignBatch& b;
	RawVec<RealignJob>& jobs;
	RawVec<uint8_t>& query;
	RawVec<uint32_t>& long_jobs;
	const bool sorted;   // positions non-decreasing: the skip of the variants left of the read is a binary search
	uint32_t max_target_long = 0;
	uint64_t pairs = 0;

	// realign() for job (v, i, consumed, query_pos) of alignment a: false with `msg` on an exception
	bool realign(uint64_t a, uint64_t v, uint64_t i, int64_t consumed, int64_t query_pos, std::string& msg) {
		for (uint64_t x = var.alt_ptr[v]; x < var.alt_ptr[v + 1]; ++x)   // symbolic alleles (<DEL>, ...): no decision, no error
			if (var.alt_byte_ptr[x + 1] > var.alt_byte_ptr[x] && var.alt_bytes[var.alt_byte_ptr[x]] == '<') return true;
		const uint64_t c0 = al.cigar_ptr[a], nc = al.cigar_ptr[a + 1] - c0;
		const uint32_t* ops = al.cigar_op + c0;
		const uint32_t* lens = al.cigar_len + c0;
		const int64_t middle = lens[i];
		if (!(consumed <= middle)) { msg = "AssertionError: assert consumed <= middle_length"; return false; }
		auto left = [&](uint64_t k, uint32_t& op, int64_t& len) {   // (op_i, consumed) if consumed > 0, then cigar[i-1] .. cigar[0]
			if (consumed > 0) {
				if (k == 0) { op = ops[i]; len = consumed; return true; }
				--k;
			}
			if (k >= i) return false;
			op = ops[i - 1 - k]; len = lens[i - 1 - k];
			return true;
		};
		auto right = [&](uint64_t k, uint32_t& op, int64_t& len) {   // (op_i, length - consumed) if that is > 0, then cigar[i+1] ..
			if (consumed < middle) {
				if (k == 0) { op = ops[i]; len = middle - consumed; return true; }
				--k;
			}
			if (i + 1 + k >= nc) return false;
			op = ops[i + 1 + k]; len = lens[i + 1 + k];
			return true;
		};
		const int64_t ref_len = (int64_t)(var.ref_ptr[v + 1] - var.ref_ptr[v]);
		int64_t left_ref = 0, left_query = 0, right_ref = 0, right_query = 0;
		if (!cigar_prefix_length(left, params.overhang, left_ref, left_query, msg)) return false;
		if (!cigar_prefix_length(right, ref_len + params.overhang, right_ref, right_query, msg)) return false;
		const int64_t pos = var.position[v];
		if (!(pos - left_ref >= 0)) { msg = "AssertionError: assert variant.position - left_ref_bases >= 0"; return false; }
		if (!(pos + right_ref <= (int64_t)ref.chromosome_length)) { msg = "AssertionError: assert variant.position + right_ref_bases <= len(reference)"; return false; }
		if (al.seq_present && !al.seq_present[a]) { msg = "TypeError: 'NoneType' object is not subscriptable"; return false; }
		if (params.use_affine && params.affine_unset) { msg = "AssertionError: assert gap_start is not None"; return false; }
		// query_sequence[query_pos - left_query_bases : query_pos + right_query_bases] (Python slice: clamped to the sequence)
		const int64_t seq_len = (int64_t)(al.seq_ptr[a + 1] - al.seq_ptr[a]);
		auto clamp = [&](int64_t x) { return x < 0 ? std::max<int64_t>(0, seq_len + x) : std::min(x, seq_len); };
		const int64_t q0 = clamp(query_pos - left_query), q1 = clamp(query_pos + right_query);
		const int64_t q_len = std::max<int64_t>(0, q1 - q0);
		const RealignVariant& rv = b.variants[v];
		if (rv.allow_n == 0) { msg = "IndexError: list index out of range"; return false; }
		const int64_t w0 = pos - left_ref, w1 = pos + right_ref;
		if (w0 < (int64_t)ref.offset || (w1 > w0 && (uint64_t)w1 > ref.offset + ref.length)) {
			msg = "reference slice [" + std::to_string(ref.offset) + ", " + std::to_string(ref.offset + ref.length) + ") does not cover the window [" +
			      std::to_string(w0) + ", " + std::to_string(w1) + ") of variant " + std::to_string(v);
			return false;
		}
		if (q_len > (int64_t)UINT32_MAX / 2 || left_ref > (int64_t)UINT32_MAX / 4 || right_ref > (int64_t)UINT32_MAX / 4) { msg = "window too long"; return false; }
		RealignJob job;
		job.q_off = query.size();
		job.win_start = (uint64_t)(w0 - (int64_t)ref.offset);
		job.q_len = (uint32_t)q_len;
		job.variant = (uint32_t)v;
		job.left = (uint32_t)left_ref;
		job.right = (uint32_t)right_ref;
		if (job.q_len > 64) {   // more than one query word / strip: the kernels need a scratch row as long as the longest allele window
			long_jobs.push_back((uint32_t)jobs.size());
			for (uint32_t k = 0; k < rv.allow_n; ++k) {
				const uint32_t allele = b.allow[rv.allow_off + k];
				uint64_t t = job.left + job.right;
				if (allele > 0) t = job.left + (b.alt_off[rv.alt_first + allele] - b.alt_off[rv.alt_first + allele - 1]) + (job.right > rv.ref_len ? job.right - rv.ref_len : 0);
				max_target_long = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(max_target_long, t), UINT32_MAX);
			}
		}
		jobs.push_back(job);
		query.insert(query.end(), al.seq + al.seq_ptr[a] + q0, al.seq + al.seq_ptr[a] + q0 + q_len);
		pairs += rv.allow_n;
		return true;
	}

	// _iterate_cigar + realign for alignment a: the jobs it makes, false with `msg` at its first exception
	bool walk(uint64_t a, uint32_t& n_jobs, std::string& msg) {
		const uint64_t before = jobs.size();
		const uint64_t c0 = al.cigar_ptr[a], nc = al.cigar_ptr[a + 1] - c0;
		n_jobs = 0;
		if (nc == 0) return true;   // `if not cigartuples: return`
		const uint64_t n = var.n_variants;
		int64_t ref_pos = al.reference_start[a], query_pos = 0, v_position = 0;
		uint64_t j = al.first_variant ? al.first_variant[a] : 0;
		if (sorted) j = (uint64_t)(std::lower_bound(var.position + std::min(j, n), var.position + n, ref_pos) - var.position);   // (same j as the scan below)
		while (j < n && var.position[j] < ref_pos) ++j;
		bool ok = true;
		for (uint64_t i = 0; i < nc && ok; ++i) {
			const uint32_t op = al.cigar_op[c0 + i];
			const int64_t length = al.cigar_len[c0 + i];
			if (j < n) v_position = var.position[j];
			if (is_match_op(op) || op == 2 || op == 3) {
				while (ok && j < n && v_position < ref_pos + length) {
					if (!(v_position >= ref_pos)) { msg = "AssertionError: assert v_position >= ref_pos"; ok = false; break; }
					if (op != 3) ok = realign(a, j, i, v_position - ref_pos, op == 2 ? query_pos : query_pos + v_position - ref_pos, msg);
					++j;
					if (j < n) v_position = var.position[j];
				}
				if (op != 2 && op != 3) query_pos += length;
				ref_pos += length;
			} else if (op == 1) {
				if (j < n && v_position == ref_pos) {
					ok = realign(a, j, i, 0, query_pos, msg);
					++j;
				}
				query_pos += length;
			} else if (op == 4) {
				query_pos += length;
			} else if (op == 5 || op == 6) {
			} else {
				msg = "ValueError: Unsupported CIGAR operation: " + std::to_string(op);
				ok = false;
			}
		}
		n_jobs = (uint32_t)(jobs.size() - before);
		return ok;
	}
};

}  // namespace

namespace whamd {

whamd_status_t realign_walk(const whamd_realign_alignments_view& al, const whamd_realign_variants_view& var,
                            const whamd_realign_reference_view& ref, const whamd_realign_params& params, RealignBatch& b, std::string& msg) {
	const uint64_t nv = var.n_variants, na = al.n_alignments;
	if (nv >= UINT32_MAX) { msg = "too many variants for one call"; return WHAMD_ERR_INVALID; }
	if ((na && (!al.reference_start || !al.cigar_ptr || !al.seq_ptr)) || (nv && (!var.position || !var.ref_ptr || !var.alt_ptr || !var.alt_byte_ptr)) ||
	    (ref.length && !ref.bytes)) {
		msg = "null array in a realign view";
		return WHAMD_ERR_INVALID;
	}
	b.params = params;
	b.ref = ref.bytes;
	b.ref_len = ref.length;
	// the variant tables: allowed alleles (`i in restricted_variants.as_vector()` for i in 0 .. k, in index order)
	b.variants.resize(nv);
	if (nv) b.alt_off.assign(var.alt_byte_ptr, var.alt_byte_ptr + var.alt_ptr[nv] + 1);
	else b.alt_off.assign(1, 0);
	b.alt_bytes = var.alt_bytes;
	b.n_alt_bytes = b.alt_off.back();
	b.allow.clear();
	for (uint64_t v = 0; v < nv; ++v) {
		RealignVariant& rv = b.variants[v];
		rv.ref_len = (uint32_t)(var.ref_ptr[v + 1] - var.ref_ptr[v]);
		rv.alt_first = (uint32_t)var.alt_ptr[v];
		rv.allow_off = (uint32_t)b.allow.size();
		const uint32_t k = (uint32_t)(var.alt_ptr[v + 1] - var.alt_ptr[v]);
		const bool restricted = var.restrict_ptr && (!var.restrict_present || var.restrict_present[v]);
		for (uint32_t i = 0; i <= k; ++i) {
			bool in = true;
			if (restricted) {
				in = false;
				for (uint64_t x = var.restrict_ptr[v]; x < var.restrict_ptr[v + 1] && !in; ++x) in = var.restrict_alleles[x] == (int64_t)i;
			}
			if (in) b.allow.push_back(i);
		}
		rv.allow_n = (uint32_t)(b.allow.size() - rv.allow_off);
	}
	// the walk: ranges of alignments on the host pool
	const uint32_t n_threads = host_threads(na, 256);
	b.range_jobs.assign(n_threads, {});
	b.range_query.assign(n_threads, {});
	b.range_long.assign(n_threads, {});
	bool sorted = true;
	for (uint64_t v = 1; v < nv && sorted; ++v) sorted = var.position[v - 1] <= var.position[v];
	b.jobs_of.assign(na, 0);
	std::vector<uint64_t> fail_at(n_threads, UINT64_MAX), range_pairs(n_threads, 0);
	std::vector<std::string> fail_msg(n_threads);
	std::vector<uint32_t> mt(n_threads, 0);
	parallel_ranges(na, n_threads, [&](uint64_t begin, uint64_t end, uint32_t t) {
		b.range_jobs[t].reserve((end - begin) * 8);
		Walker w{al, var, ref, params, b, b.range_jobs[t], b.range_query[t], b.range_long[t], sorted};
		for (uint64_t a = begin; a < end; ++a) {
			if (!w.walk(a, b.jobs_of[a], fail_msg[t])) { fail_at[t] = a; break; }
		}
		mt[t] = w.max_target_long;
		range_pairs[t] = w.pairs;
	});
	for (uint32_t t = 0; t < n_threads; ++t)
		if (fail_at[t] != UINT64_MAX) { msg = fail_msg[t]; return WHAMD_ERR_INVALID; }   // (ranges are in alignment order: the first failing range has the first failure)
	b.range_job_base.assign(n_threads, 0);
	b.range_query_base.assign(n_threads, 0);
	b.range_long_base.assign(n_threads, 0);
	b.n_jobs = b.n_query_bytes = b.n_pairs = b.n_long = 0;
	b.max_target_long = 0;
	for (uint32_t t = 0; t < n_threads; ++t) {
		b.range_job_base[t] = b.n_jobs;
		b.range_query_base[t] = b.n_query_bytes;
		b.range_long_base[t] = b.n_long;
		b.n_jobs += b.range_jobs[t].size();
		b.n_query_bytes += b.range_query[t].size();
		b.n_long += b.range_long[t].size();
		b.n_pairs += range_pairs[t];
		b.max_target_long = std::max(b.max_target_long, mt[t]);
	}
	if (b.n_jobs >= UINT32_MAX) { msg = "too many (alignment, variant) jobs for one call"; return WHAMD_ERR_INVALID; }
	return WHAMD_OK;
}

}  // namespace whamd

// ------------------------------------------------------------------------------------------------- host restatement (debug library)
#ifdef WHAMD_DEBUG_BUILD
namespace {

// edit_distance(s, t), maxdiff = -1 (align.pyx:16-97): prefix / suffix stripping and the column DP, as written there
template <class Q, class T>
int64_t host_edit_distance(const Q& s, uint32_t m, const T& t, uint32_t n) {
	uint32_t p = 0;
	while (m > 0 && n > 0 && s(p) == t(p)) { ++p; --m; --n; }
	while (m > 0 && n > 0 && s(p + m - 1) == t(p + n - 1)) { --m; --n; }
	std::vector<int64_t> costs(m + 1);
	for (uint32_t i = 0; i <= m; ++i) costs[i] = i;
	for (uint32_t j = 1; j <= n; ++j) {
		int64_t prev = costs[0];
		costs[0] += 1;
		for (uint32_t i = 1; i <= m; ++i) {
			const int64_t match = s(p + i - 1) == t(p + j - 1);
			const int64_t c = std::min({prev + 1 - match, costs[i] + 1, costs[i - 1] + 1});
			prev = costs[i];
			costs[i] = c;
		}
	}
	return costs[m];
}

// edit_distance_affine_gap(query, ref, mismatch_cost, gap_start, gap_extend) (align.pyx:103-196), f32 operation by operation
template <class Q, class T, class M>
int64_t host_affine(const Q& s, uint32_t m, const T& t, uint32_t n, const M& cost, int32_t gs, int32_t ge) {
	uint32_t len_p = 0;
	while (m > 0 && n > 0 && s(len_p) == t(len_p)) { ++len_p; --m; --n; }
	while (m > 0 && n > 0 && s(len_p + m - 1) == t(len_p + n - 1)) { --m; --n; }
	std::vector<float> a(m + 1), bb(m + 1), c(m + 1);
	a[0] = bb[0] = c[0] = 0.0f;
	for (uint32_t i = 1; i <= m; ++i) {
		a[i] = AFFINE_INF;
		bb[i] = affine_gap_f(i, gs, ge);
		c[i] = AFFINE_INF;
	}
	const float fgs = (float)gs, fge = (float)ge;
	for (uint32_t j = 1; j <= n; ++j) {
		float prev_a = a[0], prev_b = bb[0], prev_c = c[0];
		a[0] = AFFINE_INF;
		bb[0] = AFFINE_INF;
		c[0] = affine_gap_f(j, gs, ge);
		for (uint32_t i = 1; i <= m; ++i) {
			float m_c = cost(i - 1 + len_p);
			if (s(len_p + i - 1) == t(len_p + j - 1)) m_c = 0.0f;
			const float c_a = std::min({prev_a, prev_b, prev_c}) + m_c;
			const float c_b = std::min({a[i - 1] + fgs, bb[i - 1] + fge, c[i - 1] + fgs});
			const float c_c = std::min({a[i] + fgs, bb[i] + fgs, c[i] + fge});
			prev_a = a[i];
			prev_b = bb[i];
			prev_c = c[i];
			a[i] = c_a;
			bb[i] = c_b;
			c[i] = c_c;
		}
	}
	return (int64_t)std::min({a[m], bb[m], c[m]});
}

// distances of one job's allowed alleles, then realign's decision: stable sort by distance, first allele iff it is alone or strictly best
void host_decide(const RealignBatch& b, const RealignJob& job, const uint8_t* q, int32_t& allele_out, int64_t& quality_out) {
	const RealignVariant& rv = b.variants[job.variant];
	std::vector<std::pair<int64_t, uint32_t>> d;   // (distance, allele)
	auto qa = [&](uint32_t i) { return q[i]; };
	for (uint32_t k = 0; k < rv.allow_n; ++k) {
		const uint32_t allele = b.allow[rv.allow_off + k];
		const Target t = allele_target(job, rv, allele, b.ref, b.alt_off.data(), b.alt_bytes);
		auto ta = [&](uint32_t j) { return t.at(j); };
		const float mm = b.params.default_mismatch;
		auto cost = [&](uint32_t) { return mm; };
		d.emplace_back(b.params.use_affine ? host_affine(qa, job.q_len, ta, t.len(), cost, b.params.gap_start, b.params.gap_extend)
		                                   : host_edit_distance(qa, job.q_len, ta, t.len()), allele);
	}
	std::stable_sort(d.begin(), d.end(), [](const std::pair<int64_t, uint32_t>& x, const std::pair<int64_t, uint32_t>& y) { return x.first < y.first; });
	quality_out = b.params.use_affine ? (d.size() > 1 ? d[0].first - d[1].first : d[0].first) : 30;
	allele_out = (d.size() == 1 || d[0].first < d[1].first) ? (int32_t)d[0].second : -1;
}

}  // namespace
#endif

struct whamd_realign {
	RawVec<uint64_t> ptr;
	RawVec<uint64_t> variant;
	RawVec<int32_t> allele;
	RawVec<int64_t> quality;
	whamd_realign_stats stats{};
};

namespace {

// the per-alignment result lists out of the per-job decisions
void compact(const RealignBatch& b, uint64_t n_alignments, const int32_t* allele, const int64_t* quality, whamd_realign& r) {
	r.ptr.resize(n_alignments + 1);
	const uint32_t n_threads = host_threads(n_alignments, 4096);
	std::vector<uint64_t> first_job(n_threads + 1, 0), count(n_threads + 1, 0);
	std::vector<uint64_t> job_base(n_alignments + 1);
	{
		uint64_t s = 0;
		for (uint64_t a = 0; a < n_alignments; ++a) { job_base[a] = s; s += b.jobs_of[a]; }
		job_base[n_alignments] = s;
	}
	parallel_ranges(n_alignments, n_threads, [&](uint64_t begin, uint64_t end, uint32_t t) {
		uint64_t c = 0;
		for (uint64_t x = job_base[begin]; x < job_base[end]; ++x) c += allele[x] >= 0;
		count[t] = c;
	});
	std::vector<uint64_t> out_base(n_threads + 1, 0);
	for (uint32_t t = 0; t < n_threads; ++t) out_base[t + 1] = out_base[t] + count[t];
	const uint64_t total = out_base[n_threads];
	r.variant.resize(total);
	r.allele.resize(total);
	r.quality.resize(total);
	parallel_ranges(n_alignments, n_threads, [&](uint64_t begin, uint64_t end, uint32_t t) {
		uint64_t o = out_base[t];
		for (uint64_t a = begin; a < end; ++a) {
			r.ptr[a] = o;
			for (uint64_t x = job_base[a]; x < job_base[a + 1]; ++x) {
				if (allele[x] < 0) continue;
				const uint64_t range = (uint64_t)(std::upper_bound(b.range_job_base.begin(), b.range_job_base.end(), x) - b.range_job_base.begin()) - 1;   // the walk range that made the job
				r.variant[o] = b.range_jobs[range][x - b.range_job_base[range]].variant;
				r.allele[o] = allele[x];
				r.quality[o] = quality ? quality[x] : 30;
				++o;
			}
		}
	});
	r.ptr[n_alignments] = total;
	r.stats.n_results = total;
}

whamd_status_t detect(const whamd_realign_alignments_view* alignments, const whamd_realign_variants_view* variants,
                      const whamd_realign_reference_view* reference, const whamd_realign_params* params, int device, bool host,
                      whamd_realign** out) {
	if (!alignments || !variants || !reference || !params || !out) return fail(WHAMD_ERR_INVALID, "null argument");
	*out = nullptr;
	const double t0 = now_ms();
	RealignBatch b;
	std::string msg;
	whamd_status_t st = realign_walk(*alignments, *variants, *reference, *params, b, msg);
	if (st != WHAMD_OK) return fail(st, msg);
	const double t1 = now_ms();
	std::unique_ptr<whamd_realign> r(new whamd_realign());
	r->stats.n_alignments = alignments->n_alignments;
	r->stats.n_jobs = b.n_jobs;
	r->stats.n_pairs = b.n_pairs;
	r->stats.host_walk_ms = t1 - t0;
	RawVec<int32_t> allele(b.n_jobs);
	RawVec<int64_t> quality(params->use_affine ? b.n_jobs : 0);
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		for (size_t t = 0; t < b.range_jobs.size(); ++t) {
			const uint8_t* q = b.range_query[t].data();
			for (size_t k = 0; k < b.range_jobs[t].size(); ++k) {
				const RealignJob& job = b.range_jobs[t][k];
				int64_t qual = 0;
				host_decide(b, job, q + job.q_off, allele[b.range_job_base[t] + k], qual);
				if (params->use_affine) quality[b.range_job_base[t] + k] = qual;
			}
		}
#endif
	} else if (b.n_jobs) {
		CallTimes times;
		st = realign_device(b, device, allele.data(), params->use_affine ? quality.data() : nullptr, times, msg);
		if (st != WHAMD_OK) return fail(st, msg);
		r->stats.upload_ms = times.upload_ms;
		r->stats.kernel_ms = times.kernel_ms;
		r->stats.download_ms = times.download_ms;
	}
	const double t2 = now_ms();
	compact(b, alignments->n_alignments, allele.data(), params->use_affine ? quality.data() : nullptr, *r);
	const double t3 = now_ms();
	r->stats.host_finish_ms = t3 - t2;
	r->stats.total_ms = t3 - t0;
	*out = r.release();
	return WHAMD_OK;
}

}  // namespace

extern "C" {

whamd_status_t whamd_realign_detect(const whamd_realign_alignments_view* alignments, const whamd_realign_variants_view* variants,
                                    const whamd_realign_reference_view* reference, const whamd_realign_params* params, int device,
                                    whamd_realign** out) {
	return guarded([&]() -> whamd_status_t { return detect(alignments, variants, reference, params, device, false, out); });
}

uint64_t whamd_realign_result_count(const whamd_realign* r) { return r ? r->variant.size() : 0; }

whamd_status_t whamd_realign_get(const whamd_realign* r, uint64_t* ptr_out, uint64_t* variant_out, int32_t* allele_out, int64_t* quality_out) {
	if (!r) return fail(WHAMD_ERR_INVALID, "null argument");
	if (ptr_out) std::copy(r->ptr.begin(), r->ptr.end(), ptr_out);
	if (variant_out) std::copy(r->variant.begin(), r->variant.end(), variant_out);
	if (allele_out) std::copy(r->allele.begin(), r->allele.end(), allele_out);
	if (quality_out) std::copy(r->quality.begin(), r->quality.end(), quality_out);
	return WHAMD_OK;
}

whamd_status_t whamd_realign_get_stats(const whamd_realign* r, whamd_realign_stats* stats_out) {
	if (!r || !stats_out) return fail(WHAMD_ERR_INVALID, "null argument");
	*stats_out = r->stats;
	return WHAMD_OK;
}

void whamd_realign_destroy(whamd_realign* r) { delete r; }

whamd_status_t whamd_edit_distance_batch(uint64_t n_pairs, const uint64_t* query_ptr, const uint8_t* query, const uint64_t* target_ptr,
                                         const uint8_t* target, int use_affine, const float* mismatch_cost, int32_t gap_start,
                                         int32_t gap_extend, int device, int64_t* distance_out) {
	return guarded([&]() -> whamd_status_t {
		if (n_pairs == 0) return WHAMD_OK;
		if (!query_ptr || !target_ptr || !distance_out || (use_affine && !mismatch_cost)) return fail(WHAMD_ERR_INVALID, "null argument");
		std::string msg;
		const whamd_status_t st = edit_distance_device(n_pairs, query_ptr, query, target_ptr, target, use_affine, mismatch_cost, gap_start, gap_extend,
		                                               device, distance_out, msg);
		return st == WHAMD_OK ? st : fail(st, msg);
	});
}

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_realign_detect_host(const whamd_realign_alignments_view* alignments, const whamd_realign_variants_view* variants,
                                               const whamd_realign_reference_view* reference, const whamd_realign_params* params,
                                               whamd_realign** out) {
	return guarded([&]() -> whamd_status_t { return detect(alignments, variants, reference, params, 0, true, out); });
}

whamd_status_t whamd_debug_edit_distance_host(uint64_t n_pairs, const uint64_t* query_ptr, const uint8_t* query, const uint64_t* target_ptr,
                                              const uint8_t* target, int use_affine, const float* mismatch_cost, int32_t gap_start,
                                              int32_t gap_extend, int64_t* distance_out) {
	return guarded([&]() -> whamd_status_t {
		if (n_pairs == 0) return WHAMD_OK;
		if (!query_ptr || !target_ptr || !distance_out || (use_affine && !mismatch_cost)) return fail(WHAMD_ERR_INVALID, "null argument");
		for (uint64_t p = 0; p < n_pairs; ++p) {
			const uint8_t* q = query + query_ptr[p];
			const uint8_t* t = target + target_ptr[p];
			const float* c = use_affine ? mismatch_cost + query_ptr[p] : nullptr;
			const uint32_t m = (uint32_t)(query_ptr[p + 1] - query_ptr[p]), n = (uint32_t)(target_ptr[p + 1] - target_ptr[p]);
			auto qa = [&](uint32_t i) { return q[i]; };
			auto ta = [&](uint32_t j) { return t[j]; };
			auto ca = [&](uint32_t i) { return c[i]; };
			distance_out[p] = use_affine ? host_affine(qa, m, ta, n, ca, gap_start, gap_extend) : host_edit_distance(qa, m, ta, n);
		}
		return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_realign_long_shape(int use_affine, uint64_t n_long, uint32_t max_target, whamd_debug_realign_shape* out) {
	return guarded([&]() -> whamd_status_t {
		if (!out) return fail(WHAMD_ERR_INVALID, "null argument");
		const LongShape s = long_shape(use_affine != 0, n_long, max_target);
		out->blocks = s.blocks;
		out->block = s.block;
		out->lds_bytes = s.lds;
		out->scratch_bytes = s.scratch;
		out->carry_words = s.carry_words;
		out->row_floats = s.row_floats;
		out->global_rows = s.global_rows ? 1 : 0;
		out->reserved = 0;
		return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_realign_walk_counts(const whamd_realign_alignments_view* alignments, const whamd_realign_variants_view* variants,
                                               const whamd_realign_reference_view* reference, const whamd_realign_params* params,
                                               uint64_t* n_jobs_out, uint64_t* n_long_out, uint32_t* max_target_long_out) {
	return guarded([&]() -> whamd_status_t {
		if (!alignments || !variants || !reference || !params) return fail(WHAMD_ERR_INVALID, "null argument");
		RealignBatch b;
		std::string msg;
		const whamd_status_t st = realign_walk(*alignments, *variants, *reference, *params, b, msg);
		if (st != WHAMD_OK) return fail(st, msg);
		if (n_jobs_out) *n_jobs_out = b.n_jobs;
		if (n_long_out) *n_long_out = b.n_long;
		if (max_target_long_out) *max_target_long_out = b.max_target_long;
		return WHAMD_OK;
	});
}

whamd_status_t whamd_debug_edit_distance_long_counts(uint64_t n_pairs, const uint64_t* query_ptr, const uint64_t* target_ptr, uint64_t* n_long_out,
                                                     uint32_t* max_target_long_out) {
	return guarded([&]() -> whamd_status_t {
		if (n_pairs && (!query_ptr || !target_ptr)) return fail(WHAMD_ERR_INVALID, "null argument");
		std::vector<uint32_t> long_pairs;
		const uint32_t max_t = n_pairs ? long_pairs_of(n_pairs, query_ptr, target_ptr, long_pairs) : 0;
		if (n_long_out) *n_long_out = long_pairs.size();
		if (max_target_long_out) *max_target_long_out = max_t;
		return WHAMD_OK;
	});
}
#endif

}  // extern "C"
