// api_guard.h -- what every file with extern "C" entry points uses at the boundary: the error message of whamd_last_error(), the guard that
// lets no C++ exception through, and the clock of the host times in the statistics.  Host only.
#pragma once
#include <chrono>
#include <exception>
#include <new>
#include <string>

#include "../../include/whatshap_amd.h"

namespace whamd {

void set_last_error(const std::string& msg);   // c_api.cpp: the calling thread's message

inline whamd_status_t fail(whamd_status_t st, const std::string& msg) {
	set_last_error(msg);
	return st;
}

// No C++ exception crosses the C boundary: std::bad_alloc of the flatten / plan vectors, std::system_error of a worker thread that could not
// be started, anything a worker carried over (host_parallel.h) become WHAMD_ERR_HOST with the exception's message.
template <class F>
whamd_status_t guarded(F&& body) {
	try {
		return body();
	} catch (const std::bad_alloc&) {
		return fail(WHAMD_ERR_HOST, "out of host memory");
	} catch (const std::exception& e) {
		return fail(WHAMD_ERR_HOST, std::string("host-side failure: ") + e.what());
	} catch (...) {
		return fail(WHAMD_ERR_HOST, "host-side failure (unknown exception)");
	}
}

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace whamd
