// polyscore.cpp -- the host side of polyphase read scoring: the AlleleMatrix of src/polyphase/allelematrix.cpp, the genotype likelihoods,
// error-rate estimate and allele-pair tables of src/polyphase/readscoring.cpp, restated from their behaviour (quirks included, see
// computeGenotypeLikelihoods below), folded into one float term per (position, allele, allele); the candidate windows of the pair loop;
// the C ABI of whatshap_amd.h's polyphase section; and, in the debug library only, the host pair loop (whamd_debug_poly_score_host).
#include "polyscore.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <memory>
#include <unordered_map>

#include "batch_call.h"
#include "debug_build.h"

using namespace whamd;

namespace {

// ---------------------------------------------------------------------------------------------- binomial.cpp / multinomial.cpp semantics
int binomial_coefficient(int n, int k) {
	if (k < 0 || n < 0 || n < k) return 0;
	int result = 1;
	if (k > n - k) k = n - k;
	for (int i = 0; i < k; i++) {
		result *= (n - i);
		result /= (i + 1);
	}
	return result;
}

// log C(n, k) as a running product that is logged only when it would overflow
double binomial_coefficient_log(int n, int k) {
	if (k < 0 || n < 0 || n < k) return 0;
	if (k > n - k) k = n - k;
	double result = 0.0, buffer = 1.0;
	for (int i = 0; i < k; i++) {
		const double addition = (double)(n - i) / (double)(i + 1);
		if (buffer * addition > std::numeric_limits<double>::max()) {
			result += std::log(buffer);
			buffer = addition;
		} else {
			buffer *= addition;
		}
	}
	return result + std::log(buffer);
}

double log_binom_pmf(int n, int k, double p) { return binomial_coefficient_log(n, k) + k * std::log(p) + (n - k) * std::log(1 - p); }

// The reference's log multinomial coefficient: every factor of the smaller counts divides (total - largest count), not a falling
// product -- restated as it computes.
double log_multinomial_coefficient(const std::vector<uint32_t>& n) {
	std::vector<uint32_t> s(n.begin(), n.end());
	std::sort(s.begin(), s.end(), [](uint32_t a, uint32_t b) { return a > b; });
	uint32_t sum = s[0];
	std::vector<uint32_t> factors;
	for (size_t i = 1; i < s.size(); i++) {
		sum += s[i];
		for (uint32_t j = 2; j <= s[i]; j++) factors.push_back(j);
	}
	double result = 0.0, buffer = 1.0;
	for (uint32_t f : factors) {
		const double addition = (double)(sum - s[0]) / (double)f;
		if (buffer * addition > std::numeric_limits<double>::max()) {
			result += std::log(buffer);
			buffer = addition;
		} else {
			buffer *= addition;
		}
	}
	return result + std::log(buffer);
}

// (only called with three or more counts: the binomial shortcut of the reference never applies here)
double log_multinom_pmf(const std::vector<uint32_t>& n, const std::vector<double>& p) {
	double sum = p[0];
	for (size_t i = 1; i < p.size(); i++) sum += p[i];
	if (sum != 1.0) return 0;   // the reference's exact check: probabilities that do not add up to 1.0 give l = 0
	double result = log_multinomial_coefficient(n);
	for (size_t i = 0; i < p.size(); i++) result += std::log(p[i]);   // (sic: log p, not n * log p)
	return result;
}

// ---------------------------------------------------------------------------------------------- genotypes
// Genotypes of one ploidy by canonical index (src/genotype.h:18-47), alleles as Genotype::as_vector() returns them (largest first).
struct GenotypeTable {
	uint32_t ploidy = 0, n_alleles = 0;
	std::vector<std::vector<uint32_t>> alleles;   // [C(ploidy + n_alleles - 1, n_alleles - 1)]
	std::vector<uint64_t> code;                   // Genotype::get_code(): allele i in bits 4 i .. 4 i + 3, the ploidy in bits 60 .. 63
	void build(uint32_t p, uint32_t a) {
		ploidy = p;
		n_alleles = a;
		const int n = a ? binomial_coefficient((int)(p + a - 1), (int)a - 1) : 0;
		alleles.assign(n, {});
		code.assign(n, 0);
		if (!n) return;
		std::vector<uint32_t> cur(p, 0);   // ascending
		// every multiset of size p over [0, a): index = sum_i C(cur[i] + i, i + 1)
		std::function<void(uint32_t, uint32_t)> rec = [&](uint32_t slot, uint32_t from) {
			if (slot == p) {
				uint64_t index = 0;
				for (uint32_t i = 0; i < p; i++) index += (uint64_t)binomial_coefficient((int)(cur[i] + i), (int)(i + 1));
				alleles[index].assign(cur.rbegin(), cur.rend());
				code[index] = (uint64_t)p << 60;
				for (uint32_t i = 0; i < p; i++) code[index] |= (uint64_t)alleles[index][i] << (4 * i);
				return;
			}
			for (uint32_t x = from; x < a; x++) {
				cur[slot] = x;
				rec(slot + 1, x);
			}
		};
		rec(0, 0);
	}
};

// The order in which the reference walks the genotypes of one position: that of its std::unordered_map<Genotype, double>, filled in
// increasing index and hashed by the genotype's code.  The sums over a position's genotypes (the normalising weight here, same / diff in
// poly_prepare) run in it, and it decides more than a last bit: where same / diff is 1 but for rounding (two different alleles at a
// position with six alleles present and err = 0.2), the term is 0.0 in one order and 1e-16 in another, and a pair whose terms are all
// 0.0 is not stored.  Restated for GNU libstdc++, which the reference is built with on Linux: buckets are code % count, the count grows
// 1 -> 13 -> 29 -> ... whenever the elements would outnumber it, a node enters at the front of its bucket's stretch of the one list, or
// at the list's head when the bucket is empty, and a growth re-enters every node that way in list order.
void hash_order(const std::vector<uint64_t>& code, std::vector<std::pair<uint32_t, double>>& gl) {
	static const uint32_t COUNTS[] = {13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753, 42043, 85229, 172933, 351061, 712697, 1447153};
	const uint32_t n = (uint32_t)gl.size();
	if (n < 2 || n > COUNTS[sizeof(COUNTS) / sizeof(COUNTS[0]) - 1]) return;   // (more genotypes than any real call has: index order)
	constexpr int32_t NONE = -1, EMPTY = -2, HEAD = -1;   // a bucket holds the node before its first one (HEAD: the list's head)
	std::vector<int32_t> next(n, NONE), before;
	int32_t head = NONE;
	uint32_t n_buckets = 1, grown = 0;
	before.assign(1, EMPTY);
	auto key = [&](int32_t node) { return code[gl[node].first]; };
	auto enter = [&](int32_t node, uint32_t& head_bucket, bool rehash) {
		const uint32_t b = (uint32_t)(key(node) % n_buckets);
		if (before[b] != EMPTY) {
			int32_t& after = before[b] == HEAD ? head : next[before[b]];
			next[node] = after;
			after = node;
			return;
		}
		next[node] = head;
		head = node;
		before[b] = HEAD;
		if (next[node] != NONE) before[rehash ? head_bucket : (uint32_t)(key(next[node]) % n_buckets)] = node;
		head_bucket = b;
	};
	for (uint32_t k = 0; k < n; k++) {
		if (k + 1 > n_buckets || k == 0) {   // (the first element already finds one bucket too few: libstdc++ starts at 13)
			n_buckets = COUNTS[grown++];
			before.assign(n_buckets, EMPTY);
			int32_t node = head;
			head = NONE;
			uint32_t head_bucket = 0;
			while (node != NONE) {
				const int32_t following = next[node];
				enter(node, head_bucket, true);
				node = following;
			}
		}
		uint32_t unused = 0;
		enter((int32_t)k, unused, false);
	}
	std::vector<std::pair<uint32_t, double>> walked;
	walked.reserve(n);
	for (int32_t node = head; node != NONE; node = next[node]) walked.push_back(gl[node]);
	gl.swap(walked);
}

// computeGenotypeLikelihoods (readscoring.cpp:123-191): (genotype index, likelihood) of the reachable genotypes, in the reference's
// order (hash_order).  Quirks kept: one present allele -> 1, then exp(1 - 0) / (1 + e) after normalisation; two present alleles ->
// fracAlt = index / ploidy (the enumeration index, not the alt count); any exp that overflows (or is NaN) -> every depth halved, all of
// it again.
void genotype_likelihoods(const GenotypeTable& gt, const uint32_t* depth_in, double err, std::vector<std::pair<uint32_t, double>>& gl) {
	const uint32_t n_alleles = gt.n_alleles, ploidy = gt.ploidy;
	std::vector<uint32_t> depth(depth_in, depth_in + n_alleles);
	for (;;) {
		gl.clear();
		std::vector<uint32_t> present;
		for (uint32_t a = 0; a < n_alleles; a++)
			if (depth[a] > 0) present.push_back(a);
		const uint32_t n_ex = (uint32_t)present.size();
		double weight = 0.0, lowest = 0.0;
		for (uint32_t index = 0; index < gt.alleles.size(); index++) {
			const std::vector<uint32_t>& g = gt.alleles[index];
			bool reachable = true;
			for (uint32_t a : g) reachable &= depth[a] > 0;
			if (!reachable) continue;
			if (n_ex == 1) {
				weight += 1;
				gl.emplace_back(index, 1.0);
			} else if (n_ex == 2) {
				const double frac_alt = (double)index / (double)ploidy;
				const double l = log_binom_pmf((int)(depth[present[0]] + depth[present[1]]), (int)depth[present[1]], (1 - frac_alt) * err + frac_alt * (1 - err));
				lowest = std::min(lowest, l);
				gl.emplace_back(index, l);
			} else {
				std::vector<double> p(n_ex);
				std::vector<uint32_t> n(n_ex);
				for (uint32_t a = 0; a < n_ex; a++) {
					double num = 0;
					for (uint32_t x : g)
						if (x == present[a]) num += 1.0;
					const double freq = num / ploidy;
					p[a] = freq * (1 - err * (n_ex - 1)) + (1 - freq) * err;
					n[a] = depth[present[a]];
				}
				const double l = log_multinom_pmf(n, p);
				lowest = std::min(lowest, l);
				gl.emplace_back(index, l);
			}
		}
		hash_order(gt.code, gl);
		bool overflow = false;
		for (auto& e : gl) {
			const double l = std::exp(e.second - lowest);
			e.second = l;
			weight += l;
			if (!(l <= std::numeric_limits<double>::max())) overflow = true;
		}
		if (!overflow) {
			for (auto& e : gl) e.second = e.second / weight;
			return;
		}
		for (uint32_t& d : depth) d /= 2;
	}
}

// evaluateGenotypeLikelihoods (readscoring.cpp:109-121) of one position: log of the largest likelihood (0 when there is none)
double log_best(const std::vector<std::pair<uint32_t, double>>& gl) {
	double best = 0.0;
	for (const auto& e : gl)
		if (e.second > best) best = e.second;
	return std::log(best);
}

// computeAllelePairLikelihoods (readscoring.cpp:193-225) of one genotype: apls / apld[a1 * n_alleles + a2]
void allele_pair_likelihoods(const std::vector<uint32_t>& gv, uint32_t n_alleles, double err, double* apls, double* apld) {
	for (uint32_t a1 = 0; a1 < n_alleles; a1++) {
		for (uint32_t a2 = a1; a2 < n_alleles; a2++) {
			double l_equal = 0.0, l_diff = 0.0;
			for (size_t g1 = 0; g1 < gv.size(); g1++) {
				for (size_t g2 = 0; g2 < gv.size(); g2++) {
					double l = (1 - err) * (gv[g1] == a1) + err * (gv[g1] != a1);
					l *= (1 - err) * (gv[g2] == a2) + err * (gv[g2] != a2);
					if (g1 == g2) l_equal += l;
					else l_diff += l;
				}
			}
			apls[a1 * n_alleles + a2] = apls[a2 * n_alleles + a1] = l_equal / gv.size();
			apld[a1 * n_alleles + a2] = apld[a2 * n_alleles + a1] = l_diff / (gv.size() * (gv.size() - 1));
		}
	}
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the matrix
whamd_status_t whamd::poly_build_matrix(const whamd_poly_matrix_view& v, PolyMatrix& m, std::string& msg) {
	const uint64_t n = v.n_reads;
	if (n >= UINT32_MAX) { msg = "too many reads in one matrix"; return WHAMD_ERR_INVALID; }
	if (n && !v.read_ptr) { msg = "null read_ptr"; return WHAMD_ERR_INVALID; }
	const uint64_t n_entries = n ? v.read_ptr[n] : 0;
	if (n_entries && (!v.position || !v.allele)) { msg = "null position / allele array"; return WHAMD_ERR_INVALID; }
	for (uint64_t r = 0; r < n; r++)
		if (v.read_ptr[r] > v.read_ptr[r + 1]) { msg = "read_ptr is not non-decreasing"; return WHAMD_ERR_INVALID; }
	if (n && v.read_ptr[0] != 0) { msg = "read_ptr[0] must be 0"; return WHAMD_ERR_INVALID; }
	int max_allele = -1;
	std::vector<uint32_t> glob(n_entries);
	for (uint64_t e = 0; e < n_entries; e++) {
		const int a = v.allele[e];
		if (a < 0) {
			msg = "negative allele " + std::to_string(a) + " (entry " + std::to_string(e) + "): the reference's AlleleMatrix is undefined on it";
			return WHAMD_ERR_INVALID;
		}
		if (a > 15) { msg = "allele " + std::to_string(a) + " above 15: the reference's Genotype holds at most 16 alleles"; return WHAMD_ERR_INVALID; }
		max_allele = std::max(max_allele, a);
		if (v.position[e] < 0 || v.position[e] > (int64_t)UINT32_MAX) { msg = "position outside [0, 2^32)"; return WHAMD_ERR_INVALID; }
		glob[e] = (uint32_t)v.position[e];
	}
	m.n_reads = (uint32_t)n;
	m.max_allele = (uint32_t)(max_allele + 1);
	// the sorted distinct positions and every entry's local index.  Where the positions span little more than there are entries (a
	// block, a chromosome) a bitmap of the span gives both in two passes; else a sort and a search per entry.
	std::vector<uint32_t> local(n_entries);
	uint32_t lo = UINT32_MAX, hi = 0;
	for (uint64_t e = 0; e < n_entries; e++) {
		lo = std::min(lo, glob[e]);
		hi = std::max(hi, glob[e]);
	}
	const uint64_t span = n_entries ? (uint64_t)hi - lo + 1 : 0;
	m.positions.clear();
	if (n_entries && span <= 64 * n_entries + (1u << 20)) {
		std::vector<uint64_t> bits((span + 63) / 64, 0);
		for (uint64_t e = 0; e < n_entries; e++) bits[(glob[e] - lo) >> 6] |= 1ull << ((glob[e] - lo) & 63u);
		std::vector<uint32_t> before(bits.size() + 1, 0);
		for (size_t w = 0; w < bits.size(); w++) before[w + 1] = before[w] + (uint32_t)__builtin_popcountll(bits[w]);
		m.positions.reserve(before[bits.size()]);
		for (size_t w = 0; w < bits.size(); w++)
			for (uint64_t rest = bits[w]; rest; rest &= rest - 1) m.positions.push_back(lo + (uint32_t)(w * 64) + (uint32_t)__builtin_ctzll(rest));
		for (uint64_t e = 0; e < n_entries; e++) {
			const uint32_t off = glob[e] - lo;
			local[e] = before[off >> 6] + (uint32_t)__builtin_popcountll(bits[off >> 6] & ((1ull << (off & 63u)) - 1));
		}
	} else {
		m.positions = glob;
		std::sort(m.positions.begin(), m.positions.end());
		m.positions.erase(std::unique(m.positions.begin(), m.positions.end()), m.positions.end());
		for (uint64_t e = 0; e < n_entries; e++) local[e] = (uint32_t)(std::lower_bound(m.positions.begin(), m.positions.end(), glob[e]) - m.positions.begin());
	}
	m.n_positions = (uint32_t)m.positions.size();
	m.depths.assign((size_t)m.n_positions * m.max_allele, 0);
	m.row_ptr.assign(n + 1, 0);
	m.row_pos.clear();
	m.row_allele.clear();
	m.row_pos.reserve(n_entries);
	m.row_allele.reserve(n_entries);
	m.first.assign(n, UINT32_MAX);
	m.last.assign(n, 0);
	std::vector<std::pair<uint32_t, uint32_t>> row;   // (local position, listed index)
	for (uint64_t r = 0; r < n; r++) {
		const uint64_t b = v.read_ptr[r], e = v.read_ptr[r + 1];
		row.clear();
		bool increasing = true;
		for (uint64_t x = b; x < e; x++) {
			const uint32_t p = local[x];
			increasing = increasing && (x == b || p > local[x - 1]);
			m.depths[(size_t)p * m.max_allele + (uint8_t)v.allele[x]] += 1;
		}
		if (increasing) {   // (the usual read: already in row order, nothing listed twice)
			for (uint64_t x = b; x < e; x++) {
				m.row_pos.push_back(local[x]);
				m.row_allele.push_back((uint8_t)v.allele[x]);
			}
			if (e > b) {
				m.first[r] = local[b];
				m.last[r] = local[e - 1];
			}
			m.row_ptr[r + 1] = m.row_pos.size();
			continue;
		}
		for (uint64_t x = b; x < e; x++) row.emplace_back(local[x], (uint32_t)(x - b));
		if (!row.empty()) {
			m.first[r] = row.front().first;
			m.last[r] = row.back().first;
		}
		std::sort(row.begin(), row.end());
		for (size_t k = 0; k < row.size(); k++) {
			if (k + 1 < row.size() && row[k + 1].first == row[k].first) continue;   // the allele listed last wins (m[i][p] = a)
			m.row_pos.push_back(row[k].first);
			m.row_allele.push_back((uint8_t)v.allele[b + row[k].second]);
		}
		m.row_ptr[r + 1] = m.row_pos.size();
	}
	return WHAMD_OK;
}

double whamd::poly_estimate_error_rate(const PolyMatrix& m, uint32_t ploidy) {
	GenotypeTable gt;
	gt.build(ploidy, m.max_allele);
	std::vector<double> best(m.n_positions);
	double best_err = 0.0, best_sum = -std::numeric_limits<double>::infinity();
	const uint32_t n_threads = host_threads(m.n_positions, 2048);
	for (double err = 0.01; err < 0.2; err += 0.01) {   // the reference's accumulating loop (20 values, the last one 0.19999999999999998)
		parallel_ranges(m.n_positions, n_threads, [&](uint64_t b, uint64_t e, uint32_t) {
			std::vector<std::pair<uint32_t, double>> gl;
			for (uint64_t p = b; p < e; p++) {
				genotype_likelihoods(gt, m.depths.data() + p * m.max_allele, err, gl);
				best[p] = log_best(gl);
			}
		});
		double sum = 0.0;
		for (double x : best) sum += x;
		if (sum > best_sum) {
			best_sum = sum;
			best_err = err;
		}
	}
	return best_err;
}

float whamd::poly_offset(uint32_t ploidy) { return -std::log(ploidy * (1.0 - 1.0 / ploidy)); }

void whamd::poly_prepare(PolyMatrix& m, uint32_t min_overlap, uint32_t ploidy, double err) {
	if (err == 0.0) err = poly_estimate_error_rate(m, ploidy);
	m.err = err;
	const uint32_t A = m.max_allele, P = m.n_positions;
	GenotypeTable gt;
	gt.build(ploidy, A);
	// allele-pair tables of every genotype (the reference builds them for the genotypes that occur; the values do not depend on which)
	const size_t G = gt.alleles.size(), AA = (size_t)A * A;
	std::vector<double> apls(G * AA), apld(G * AA);
	std::vector<uint8_t> have(G, 0);
	std::vector<std::vector<std::pair<uint32_t, double>>> gls(P);
	const uint32_t n_threads = host_threads(P, 2048);
	parallel_ranges(P, n_threads, [&](uint64_t b, uint64_t e, uint32_t) {
		for (uint64_t p = b; p < e; p++) genotype_likelihoods(gt, m.depths.data() + p * A, err, gls[p]);
	});
	for (const auto& gl : gls)
		for (const auto& x : gl) have[x.first] = 1;
	for (size_t g = 0; g < G; g++)
		if (have[g]) allele_pair_likelihoods(gt.alleles[g], A, err, apls.data() + g * AA, apld.data() + g * AA);
	// computeLogScoreSinglePos (readscoring.cpp:255-279) for every (position, a1, a2), genotypes in the order of genotype_likelihoods
	m.terms.assign((size_t)P * AA, 0.0f);
	parallel_ranges(P, n_threads, [&](uint64_t b, uint64_t e, uint32_t) {
		for (uint64_t p = b; p < e; p++) {
			for (uint32_t a1 = 0; a1 < A; a1++) {
				for (uint32_t a2 = 0; a2 < A; a2++) {
					double same = 0.0, diff = 0.0;
					for (const auto& x : gls[p]) {
						same += x.second * apls[x.first * AA + a1 * A + a2];
						diff += x.second * apld[x.first * AA + a1 * A + a2];
					}
					m.terms[p * AA + a1 * A + a2] = (same * diff <= 0.0) ? 0.0f : (float)std::log(same / diff);   // NaN stays NaN
				}
			}
		}
	});
	// The reference's loop (readscoring.cpp:55-78): reads by first position; anchor k is paired with every later read whose first position
	// is at most terminal = last - minOverlap + 1 (uint32 arithmetic: it wraps when last < minOverlap - 1).  std::sort leaves the order of
	// reads with equal first positions open; here ties go by read id.  The STORED set does not depend on that choice: a pair that shares at
	// least max(minOverlap, 1) positions (a stored score needs one shared position) has, for whichever of the two comes first in the order,
	// first(partner) <= the last shared position - minOverlap + 1 <= last(anchor) - minOverlap + 1 (rows sorted by position), so it lies
	// inside the anchor's window whatever the tie order, and its score is the same from either side (the terms are symmetric in a1, a2
	// and the shared positions are summed in increasing order).  Only n_candidates depends on the tie order.
	const uint32_t n = m.n_reads;
	m.order.resize(n);
	for (uint32_t r = 0; r < n; r++) m.order[r] = r;
	std::stable_sort(m.order.begin(), m.order.end(), [&](uint32_t a, uint32_t b) { return m.first[a] < m.first[b]; });
	std::vector<uint32_t> sorted_first(n);
	for (uint32_t k = 0; k < n; k++) sorted_first[k] = m.first[m.order[k]];
	m.window_end.resize(n);
	m.n_candidates = 0;
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t terminal = m.last[m.order[k]] - min_overlap + 1;
		const uint32_t end = (uint32_t)(std::upper_bound(sorted_first.begin() + k + 1, sorted_first.end(), terminal) - sorted_first.begin());
		m.window_end[k] = std::max(end, k + 1);
		m.n_candidates += m.window_end[k] - (k + 1);
	}
}

// ---------------------------------------------------------------------------------------------- host pair loop (debug library)
void whamd::poly_score_host(const PolyMatrix& m, uint32_t min_overlap, float offset, PolyResult& out) {
	std::vector<std::pair<uint64_t, float>> kept;
	out.n_overlapping = out.n_nan = out.n_pair_positions = 0;
	const uint32_t n = m.n_reads;
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t a = m.order[k];
		for (uint32_t q = k + 1; q < m.window_end[k]; q++) {
			const uint32_t b = m.order[q];
			double sum = 0.0;
			const uint32_t ov = poly_pair_sum(m.row_pos.data() + m.row_ptr[a], m.row_allele.data() + m.row_ptr[a], m.row_ptr[a + 1] - m.row_ptr[a],
			                                  m.row_pos.data() + m.row_ptr[b], m.row_allele.data() + m.row_ptr[b], m.row_ptr[b + 1] - m.row_ptr[b],
			                                  m.terms.data(), m.max_allele, &sum);
			out.n_pair_positions += ov;
			if (ov < min_overlap) continue;
			++out.n_overlapping;
			const float score = (float)sum;
			if (std::isnan(score)) { ++out.n_nan; continue; }
			if (score == 0.0f) continue;
			const uint32_t hi = std::max(a, b), lo = std::min(a, b);
			kept.emplace_back((uint64_t)hi * n + lo, score + offset);
		}
	}
	std::sort(kept.begin(), kept.end(), [](const std::pair<uint64_t, float>& x, const std::pair<uint64_t, float>& y) { return x.first < y.first; });
	out.i.resize(kept.size());
	out.j.resize(kept.size());
	out.score.resize(kept.size());
	for (size_t x = 0; x < kept.size(); x++) {
		out.i[x] = (uint32_t)(kept[x].first / n);
		out.j[x] = (uint32_t)(kept[x].first % n);
		out.score[x] = kept[x].second;
	}
}

// ---------------------------------------------------------------------------------------------- C ABI
struct whamd_poly_scores {
	std::vector<PolyResult> results;
	std::vector<whamd_poly_score_stats> stats;
};

namespace {

whamd_status_t score(const whamd_poly_matrix_view* views, uint64_t n_matrices, uint32_t min_overlap, uint32_t ploidy, double err, int device, bool host,
                     whamd_poly_scores** out) {
	if (!out || (n_matrices && !views)) return fail(WHAMD_ERR_INVALID, "null argument");
	*out = nullptr;
	BatchClock clock;
	clock.t0 = now_ms();
	if (ploidy > 15) return fail(WHAMD_ERR_INVALID, "ploidy " + std::to_string(ploidy) + " above 15: the reference's Genotype holds at most 15 alleles");
	std::vector<PolyMatrix> ms(n_matrices);
	std::string msg;
	for (uint64_t x = 0; x < n_matrices; x++) {
		const whamd_status_t st = poly_build_matrix(views[x], ms[x], msg);
		if (st != WHAMD_OK) return fail(st, "matrix " + std::to_string(x) + ": " + msg);
	}
	std::unique_ptr<whamd_poly_scores> r(new whamd_poly_scores());
	r->results.resize(n_matrices);
	r->stats.assign(n_matrices, whamd_poly_score_stats{});
	const bool scored = ploidy >= 2;   // ploidy < 2: empty result (readscoring.cpp:19-22)
	if (scored) {
		// (large matrices prepare on the worker pool inside; many small ones run side by side)
		const uint32_t n_threads = host_threads(n_matrices, 8);
		parallel_ranges(n_matrices, n_threads, [&](uint64_t b, uint64_t e, uint32_t) {
			for (uint64_t x = b; x < e; x++) poly_prepare(ms[x], min_overlap, ploidy, err);
		});
	}
	clock.t1 = now_ms();
	CallTimes times;
	if (scored) {
		const float offset = poly_offset(ploidy);
		if (host) {
#ifdef WHAMD_DEBUG_BUILD
			for (uint64_t x = 0; x < n_matrices; x++) poly_score_host(ms[x], min_overlap, offset, r->results[x]);
#endif
		} else {
			const whamd_status_t st = poly_score_device(ms, min_overlap, offset, device, r->results, times, msg);
			if (st != WHAMD_OK) return fail(st, msg);
		}
	}
	clock.t2 = clock.t3 = now_ms();   // (nothing is assembled: the results are the scores)
	for (uint64_t x = 0; x < n_matrices; x++) {
		whamd_poly_score_stats& s = r->stats[x];
		s.err = scored ? ms[x].err : err;
		s.n_reads = ms[x].n_reads;
		s.n_positions = ms[x].n_positions;
		s.n_candidates = ms[x].n_candidates;
		s.n_overlapping = r->results[x].n_overlapping;
		s.n_entries = r->results[x].score.size();
		s.n_nan = r->results[x].n_nan;
		s.n_pair_positions = r->results[x].n_pair_positions;
		stamp_times(s, times, clock);
	}
	*out = r.release();
	return WHAMD_OK;
}

}  // namespace

extern "C" {

whamd_status_t whamd_poly_score(const whamd_poly_matrix_view* matrices, uint64_t n_matrices, uint32_t min_overlap, uint32_t ploidy, double err,
                                int device, whamd_poly_scores** out) {
	return guarded([&]() -> whamd_status_t { return score(matrices, n_matrices, min_overlap, ploidy, err, device, false, out); });
}

uint64_t whamd_poly_score_matrix_count(const whamd_poly_scores* s) { return s ? s->results.size() : 0; }

uint64_t whamd_poly_score_count(const whamd_poly_scores* s, uint64_t m) { return s && m < s->results.size() ? s->results[m].score.size() : 0; }

whamd_status_t whamd_poly_score_get(const whamd_poly_scores* s, uint64_t m, uint32_t* i_out, uint32_t* j_out, float* score_out) {
	if (!s) return fail(WHAMD_ERR_INVALID, "null argument");
	if (m >= s->results.size()) return fail(WHAMD_ERR_INVALID, "matrix index out of range");
	const PolyResult& r = s->results[m];
	if (i_out) std::copy(r.i.begin(), r.i.end(), i_out);
	if (j_out) std::copy(r.j.begin(), r.j.end(), j_out);
	if (score_out) std::copy(r.score.begin(), r.score.end(), score_out);
	return WHAMD_OK;
}

whamd_status_t whamd_poly_score_get_stats(const whamd_poly_scores* s, uint64_t m, whamd_poly_score_stats* stats_out) {
	if (!s || !stats_out) return fail(WHAMD_ERR_INVALID, "null argument");
	if (m >= s->stats.size()) return fail(WHAMD_ERR_INVALID, "matrix index out of range");
	*stats_out = s->stats[m];
	return WHAMD_OK;
}

void whamd_poly_score_destroy(whamd_poly_scores* s) { delete s; }

whamd_status_t whamd_poly_estimate_error_rate(const whamd_poly_matrix_view* matrix, uint32_t ploidy, double* err_out) {
	return guarded([&]() -> whamd_status_t {
		if (!matrix || !err_out) return fail(WHAMD_ERR_INVALID, "null argument");
		if (ploidy < 1) return fail(WHAMD_ERR_INVALID, "ploidy must be at least 1");
		if (ploidy > 15) return fail(WHAMD_ERR_INVALID, "ploidy " + std::to_string(ploidy) + " above 15: the reference's Genotype holds at most 15 alleles");
		PolyMatrix m;
		std::string msg;
		const whamd_status_t st = poly_build_matrix(*matrix, m, msg);
		if (st != WHAMD_OK) return fail(st, msg);
		*err_out = poly_estimate_error_rate(m, ploidy);
		return WHAMD_OK;
	});
}

#ifdef WHAMD_DEBUG_BUILD
whamd_status_t whamd_debug_poly_score_host(const whamd_poly_matrix_view* matrices, uint64_t n_matrices, uint32_t min_overlap, uint32_t ploidy,
                                           double err, whamd_poly_scores** out) {
	return guarded([&]() -> whamd_status_t { return score(matrices, n_matrices, min_overlap, ploidy, err, 0, true, out); });
}
#endif

}  // extern "C"
