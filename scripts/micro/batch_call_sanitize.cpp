// CPU only: the shared host driver of the batch layers (whatshap_amd/csrc/batch_call.h) with a toy layer under AddressSanitizer + UBSan
// (the leak check runs at exit): check_offsets, copy_out, problem_of / no_problem / get_stats_of, and run_batch on its three ways out --
// success (host twin and "device"), a prepare that fails on problem 1 of 3, a device that fails.  After a failure *out is null and
// nothing that the earlier problems prepared is left behind.
// Build and run (from the repository root; the debug define makes the host path call the twin):
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -DWHAMD_DEBUG_BUILD -o /tmp/batch_call_sanitize scripts/micro/batch_call_sanitize.cpp
//   /tmp/batch_call_sanitize
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "../../whatshap_amd/csrc/batch_call.h"

using namespace whamd;

static std::string g_error;
void whamd::set_last_error(const std::string& msg) { g_error = msg; }   // (c_api.cpp's, for this program)

#define CHECK(cond)                                                          \
	do {                                                                     \
		if (!(cond)) {                                                       \
			std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
			std::exit(1);                                                    \
		}                                                                    \
	} while (0)

namespace {

// The toy layer: a problem is an offsets array, its scores the lengths of the items, its result their running sums.
struct ToyView {
	const uint64_t* ptr;
	uint64_t n;
};
struct ToyProblem {
	std::vector<uint64_t> ptr;
};
struct ToyScores {
	std::vector<uint64_t> len;
};
struct ToyStats {
	uint64_t n_items;
	uint32_t launches;
	double host_ms, upload_ms, kernel_ms, download_ms, total_ms;
};
struct ToyResult {
	struct Problem {
		std::vector<uint64_t> sums;
		ToyStats stats{};
	};
	std::vector<Problem> problems;
};

whamd_status_t toy_prepare(const ToyView& v, ToyProblem& p, std::string& msg) {
	if (!check_offsets(v.ptr, v.n, "item_ptr", "item", msg)) return WHAMD_ERR_INVALID;
	p.ptr.assign(v.ptr, v.ptr + v.n + 1);
	return WHAMD_OK;
}

void toy_lengths(const ToyProblem& p, ToyScores& sc) {
	sc.len.resize(p.ptr.size() - 1);
	for (size_t x = 0; x + 1 < p.ptr.size(); x++) sc.len[x] = p.ptr[x + 1] - p.ptr[x];
}

whamd_status_t toy(const ToyView* views, uint64_t n, bool host, bool device_fails, ToyResult** out, BatchClock* clock = nullptr) {
	return run_batch<ToyProblem, ToyScores>(
		views, n, host, out, toy_prepare,
		[](auto& problems, auto& scores) {
			for (size_t x = 0; x < problems.size(); x++) toy_lengths(problems[x], scores[x]);
		},
		[&](auto& problems, auto& scores, CallTimes& times, std::string& msg) {
			if (device_fails) {
				msg = "no device";
				return WHAMD_ERR_DEVICE;
			}
			for (size_t x = 0; x < problems.size(); x++) toy_lengths(problems[x], scores[x]);
			times.launches = 3;
			times.kernel_ms = 0.5;
			return WHAMD_OK;
		},
		[](ToyProblem& p, ToyScores& sc, ToyResult::Problem& o) {
			o.stats.n_items = sc.len.size();
			o.sums = std::move(sc.len);   // (an assemble may move out of the scores)
			std::partial_sum(o.sums.begin(), o.sums.end(), o.sums.begin());
			p.ptr.clear();
		},
		clock);
}

}  // namespace

int main() {
	std::string msg;
	const uint64_t good[] = {0, 2, 2, 5}, late[] = {1, 2, 3}, down[] = {0, 4, 3, 6};
	CHECK(check_offsets(good, 3, "a_ptr", "a", msg) && msg.empty());
	CHECK(check_offsets(nullptr, 0, "a_ptr", "a", msg));
	CHECK(!check_offsets(late, 2, "a_ptr", "a", msg) && msg == "a_ptr does not start at 0");
	CHECK(!check_offsets(down, 3, "b_ptr", "thing", msg) && msg == "b_ptr decreases at thing 1");
	CHECK(not_from_zero("pc_ptr") == "pc_ptr does not start at 0");

	const std::vector<uint32_t> src = {7, 8, 9}, none;
	uint32_t dst[4] = {1, 1, 1, 1};
	copy_out<uint32_t>(nullptr, src);
	copy_out(dst, none);
	CHECK(dst[0] == 1);
	copy_out(dst, src);
	CHECK(dst[0] == 7 && dst[2] == 9 && dst[3] == 1);

	const ToyView ok3[3] = {{good, 3}, {good, 1}, {good, 0}}, bad3[3] = {{good, 3}, {down, 3}, {good, 3}};
	for (const bool host : {true, false}) {
		ToyResult* r = nullptr;
		BatchClock clock;
		CHECK(toy(ok3, 3, host, false, &r, &clock) == WHAMD_OK && r && r->problems.size() == 3);
		CHECK((r->problems[0].sums == std::vector<uint64_t>{2, 2, 5}) && (r->problems[1].sums == std::vector<uint64_t>{2}) && r->problems[2].sums.empty());
		CHECK(clock.t0 <= clock.t1 && clock.t1 <= clock.t2 && clock.t2 <= clock.t3);
		for (const ToyResult::Problem& p : r->problems) {
			CHECK(p.stats.launches == (host ? 0u : 3u) && p.stats.kernel_ms == (host ? 0.0 : 0.5) && p.stats.upload_ms == 0.0 && p.stats.download_ms == 0.0);
			CHECK(p.stats.host_ms == clock.t1 - clock.t0 && p.stats.total_ms == clock.t3 - clock.t0 && p.stats.host_ms <= p.stats.total_ms);
		}
		ToyStats s{};
		CHECK(get_stats_of(r, 1, &s) == WHAMD_OK && s.n_items == 1);
		CHECK(get_stats_of(r, 3, &s) == WHAMD_ERR_INVALID && g_error == "problem index out of range");
		CHECK(get_stats_of(r, 0, (ToyStats*)nullptr) == WHAMD_ERR_INVALID && g_error == "null argument");
		CHECK(get_stats_of((const ToyResult*)nullptr, 0, &s) == WHAMD_ERR_INVALID && g_error == "null argument");
		CHECK(problem_of(r, 2) == &r->problems[2] && !problem_of(r, 3) && !problem_of((const ToyResult*)nullptr, 0));
		CHECK(no_problem(r) == WHAMD_ERR_INVALID && g_error == "problem index out of range");
		delete r;

		r = reinterpret_cast<ToyResult*>(&msg);   // (anything but null: the driver must clear it)
		CHECK(toy(bad3, 3, host, false, &r) == WHAMD_ERR_INVALID && r == nullptr && g_error == "problem 1: item_ptr decreases at item 1");
		r = reinterpret_cast<ToyResult*>(&msg);
		CHECK(toy(bad3 + 1, 1, host, false, &r) == WHAMD_ERR_INVALID && r == nullptr && g_error == "item_ptr decreases at item 1");
	}
	ToyResult* r = reinterpret_cast<ToyResult*>(&msg);
	CHECK(toy(ok3, 3, false, true, &r) == WHAMD_ERR_DEVICE && r == nullptr && g_error == "no device");
	CHECK(toy(ok3, 0, true, false, &r) == WHAMD_OK && r && r->problems.empty());
	delete r;
	CHECK(toy(nullptr, 0, true, false, &r) == WHAMD_OK && r && r->problems.empty());
	delete r;
	CHECK(toy(nullptr, 1, true, false, &r) == WHAMD_ERR_INVALID && g_error == "null argument");
	CHECK(toy(ok3, 3, true, false, nullptr) == WHAMD_ERR_INVALID && g_error == "null argument");
	std::puts("batch_call.h: ok");
	return 0;
}
