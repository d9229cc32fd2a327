// batch_call.h -- the host side every batch layer shares: the driver of a call over n problems (run_batch), the six time and launch
// fields of every stats struct (stamp_times), the check of an offsets array (check_offsets) and what the getters of a result repeat
// (problem_of, no_problem, get_stats_of, copy_out).  Plain function templates, host only: no .hip file includes this.
//
// A layer's driver names its four steps and nothing else:
//     return run_batch<Problem, Scores>(views, n, host, out, prepare, twin, device, assemble);
// and its result type is   struct Result { struct Problem { ...; Stats stats; }; std::vector<Problem> problems; };
#pragma once
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "api_guard.h"
#include "call_image.h"

namespace whamd {

inline std::string not_from_zero(const char* array) { return std::string(array) + " does not start at 0"; }

// An offsets array of n items (n + 1 values): it starts at 0 and does not decrease.  `array` and `item` name it in the message
// ("read_ptr decreases at read 3").
inline bool check_offsets(const uint64_t* ptr, uint64_t n, const char* array, const char* item, std::string& msg) {
	if (n && ptr[0] != 0) {
		msg = not_from_zero(array);
		return false;
	}
	for (uint64_t k = 0; k < n; k++)
		if (ptr[k] > ptr[k + 1]) {
			msg = std::string(array) + " decreases at " + item + " " + std::to_string(k);
			return false;
		}
	return true;
}

// A getter's vector into the caller's array, if the caller gave one.
template <class T>
void copy_out(T* dst, const std::vector<T>& src) {
	if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(T));
}

// Problem m of a result, nullptr if there is none (no result, or m beyond its problems); no_problem() is then the getter's failure.
template <class Result>
const typename Result::Problem* problem_of(const Result* r, uint64_t m) {
	return r && m < r->problems.size() ? &r->problems[m] : nullptr;
}

template <class Result>
whamd_status_t no_problem(const Result* r) {
	return fail(WHAMD_ERR_INVALID, r ? "problem index out of range" : "null argument");
}

// The body of a layer's *_get_stats.
template <class Result, class Stats>
whamd_status_t get_stats_of(const Result* r, uint64_t m, Stats* stats_out) {
	if (!r || !stats_out) return fail(WHAMD_ERR_INVALID, "null argument");
	const auto* p = problem_of(r, m);
	if (!p) return no_problem(r);
	*stats_out = p->stats;
	return WHAMD_OK;
}

// The points of a call on the host's clock (now_ms): start, problems prepared, device or twin done, results assembled.
struct BatchClock {
	double t0 = 0, t1 = 0, t2 = 0, t3 = 0;
};

// The six fields every stats struct has.  host_ms is the preparation, total_ms the whole call.
template <class Stats>
void stamp_times(Stats& s, const CallTimes& times, const BatchClock& clock) {
	s.launches = times.launches;
	s.host_ms = clock.t1 - clock.t0;
	s.upload_ms = times.upload_ms;
	s.kernel_ms = times.kernel_ms;
	s.download_ms = times.download_ms;
	s.total_ms = clock.t3 - clock.t0;
}

// One call over n problems.  The layer gives
//     prepare(view, problem, msg) -> status       validates one view into one Problem
//     twin(problems, scores)                      the host twin of the kernels over all problems (host calls of the debug library)
//     device(problems, scores, times, msg) -> st  the kernels over all problems
//     assemble(problem, scores, result_problem)   one problem's part of the result (it may move out of problem and scores)
// and this owns the rest: the null check, "problem k: " in front of a prepare's message when the call has more than one problem, the
// clock, the result's allocation and release (*out stays null on every failure), stamp_times for every problem.  The returned clock
// is for the fields only one layer has (fill_ms, map_ms).
// `twin` is written as a generic lambda (auto& parameters): it is instantiated only where it is called, so the product build, in which a
// host call computes nothing and assembles empty scores, never needs the twins that its body names to exist.
template <class Problem, class Scores, class View, class Result, class Prepare, class Twin, class Device, class Assemble>
whamd_status_t run_batch(const View* views, uint64_t n, bool host, Result** out, Prepare&& prepare, Twin&& twin, Device&& device, Assemble&& assemble,
                         BatchClock* clock_out = nullptr) {
	if (!out || (n && !views)) return fail(WHAMD_ERR_INVALID, "null argument");
	*out = nullptr;
	BatchClock clock;
	clock.t0 = now_ms();
	std::vector<Problem> problems(n);
	std::vector<Scores> scores(n);
	std::string msg;
	for (uint64_t x = 0; x < n; x++) {
		const whamd_status_t st = prepare(views[x], problems[x], msg);
		if (st != WHAMD_OK) return fail(st, n > 1 ? "problem " + std::to_string(x) + ": " + msg : msg);
	}
	clock.t1 = now_ms();
	CallTimes times;
	if (host) {
#ifdef WHAMD_DEBUG_BUILD
		twin(problems, scores);
#endif
	} else {
		const whamd_status_t st = device(problems, scores, times, msg);
		if (st != WHAMD_OK) return fail(st, msg);
	}
	clock.t2 = now_ms();
	std::unique_ptr<Result> r(new Result());
	r->problems.resize(n);
	for (uint64_t x = 0; x < n; x++) assemble(problems[x], scores[x], r->problems[x]);
	clock.t3 = now_ms();
	for (uint64_t x = 0; x < n; x++) stamp_times(r->problems[x].stats, times, clock);
	if (clock_out) *clock_out = clock;
	*out = r.release();
	return WHAMD_OK;
}

}  // namespace whamd
