"""The image layout and the grid arithmetic of the batch calls (whatshap_amd/csrc/call_image.h), on the host alone: a stand-alone C++
program built with the address and undefined-behaviour sanitizers lays pieces out, writes every piece to its full count and checks
offsets, total and pointers, and checks grid_for at its edges.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whatshap_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "call_image.h"

using namespace whamd;

#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond)) {                                                     \
			std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
			return 1;                                                      \
		}                                                                  \
	} while (0)

// host() and dev() of one piece: the same element type, mutable on the host and const on the device
static_assert(std::is_same<decltype(Image().host(Piece<uint64_t>())), uint64_t*>::value, "host() of a Piece<T> is T*");
static_assert(std::is_same<decltype(Image().dev(Piece<uint64_t>())), const uint64_t*>::value, "dev() of a Piece<T> is const T*");
static_assert(std::is_same<decltype(Image().host(Piece<float>())), float*>::value, "host() of a Piece<T> is T*");
static_assert(std::is_same<decltype(Image().dev(Piece<float>())), const float*>::value, "dev() of a Piece<T> is const T*");

int main() {
	{   // nothing added: no bytes
		ImageLayout l;
		CHECK(l.total == 0);
	}
	ImageLayout l;
	const auto bytes = l.add<uint8_t>(257);     // ends at 257: the next piece starts at 512
	const auto words = l.add<uint64_t>(5);      // 512 .. 552
	const auto none = l.add<uint32_t>(0);       // takes no bytes
	const auto floats = l.add<float>(64);       // exactly 256 bytes: 768 .. 1024
	const auto last = l.add<uint16_t>(3);       // 1024 .. 1030
	CHECK(bytes.offset == 0);
	CHECK(words.offset == 512);
	CHECK(none.offset == 768 && none.bytes() == 0);
	CHECK(floats.offset == none.offset);
	CHECK(last.offset == 1024);
	CHECK(last.end() == 1030);
	CHECK(l.total == 1280);                     // the end of the last piece, rounded up
	for (size_t o : {bytes.offset, words.offset, none.offset, floats.offset, last.offset, l.total}) CHECK(o % 256 == 0);

	{   // progeny_types_device for n = 3, n_samples = 2, k1 = 3: six types
		const uint32_t n = 3, n_samples = 2, k1 = 3, n_types = k1 * (k1 + 1) / 2;
		ImageLayout t;
		const auto prior = t.add<double>((size_t)n_types * k1);
		const auto rows = t.add<float>((size_t)n * n_samples * k1);
		CHECK(prior.offset == 0 && prior.bytes() == 144);
		CHECK(rows.offset == 256 && rows.bytes() == 72);
		CHECK(t.total == 512);
	}

	// two blocks of exactly the layout's total (the sanitizer sees a write past either); every piece written to its full count
	Image im;
	im.total = l.total;
	im.stage = (char*)std::malloc(l.total);
	im.base = (char*)std::malloc(l.total);
	CHECK(im.stage && im.base);
	std::memset(im.stage, 0, l.total);
	for (size_t k = 0; k < bytes.count; k++) im.host(bytes)[k] = 0xab;
	for (size_t k = 0; k < words.count; k++) im.host(words)[k] = ~0ull;
	for (size_t k = 0; k < floats.count; k++) im.host(floats)[k] = 1.0f;
	for (size_t k = 0; k < last.count; k++) im.host(last)[k] = 0xcdcd;
	// adjacent pieces do not overlap: each still holds what was written to it
	CHECK((char*)(im.host(bytes) + bytes.count) <= (char*)im.host(words));
	CHECK((char*)(im.host(words) + words.count) <= (char*)im.host(floats));
	CHECK((char*)(im.host(floats) + floats.count) <= (char*)im.host(last));
	CHECK((char*)(im.host(last) + last.count) <= im.stage + l.total);
	for (size_t k = 0; k < bytes.count; k++) CHECK(im.host(bytes)[k] == 0xab);
	for (size_t k = 0; k < words.count; k++) CHECK(im.host(words)[k] == ~0ull);
	for (size_t k = 0; k < floats.count; k++) CHECK(im.host(floats)[k] == 1.0f);
	for (size_t k = 0; k < last.count; k++) CHECK(im.host(last)[k] == 0xcdcd);
	// host and device pointer of a piece differ by the two bases, for every piece
	const ptrdiff_t delta = im.base - im.stage;
	CHECK((const char*)im.dev(bytes) - (char*)im.host(bytes) == delta);
	CHECK((const char*)im.dev(words) - (char*)im.host(words) == delta);
	CHECK((const char*)im.dev(floats) - (char*)im.host(floats) == delta);
	CHECK((const char*)im.dev(last) - (char*)im.host(last) == delta);
	CHECK((const char*)im.dev_out(last) == (const char*)im.dev(last));
	// what an upload copies: the whole image, readable to its last byte
	std::memcpy(im.base, im.stage, im.total);
	CHECK(im.dev(last)[last.count - 1] == 0xcdcd);
	std::free(im.stage);
	std::free(im.base);

	{   // a piece of a result image: what a typed fetch copies (p.bytes() to host(p)) lies inside the image, behind the piece before it
		ImageLayout r;
		const auto out = r.add<double>(33);
		const auto counts = r.add<uint32_t>(33);
		const auto n_rows = r.add<uint32_t>(1);
		CHECK(out.bytes() == 264 && counts.offset == 512 && n_rows.offset == 768 && r.total == 1024);
		CHECK(counts.offset >= out.end() && n_rows.offset >= counts.end() && n_rows.end() <= r.total);
	}
	{   // grid_for: the rounded-up quotient in 64 bits, capped
		CHECK(grid_for(0, 256) == 0);
		CHECK(grid_for(1, 256) == 1 && grid_for(256, 256) == 1 && grid_for(257, 256) == 2);
		CHECK(grid_for(257, 256 / 8) == 9);                                // eight lanes per key
		CHECK(grid_for(5, 4) == 2);                                        // one wave per item, four waves per workgroup
		CHECK(grid_for(0xffffefffull, 256) == 0x00fffff0u);                // the largest count a scatter layer accepts
		CHECK(grid_for(0x7fffffffull * 256, 256) == 0x7fffffffu);
		CHECK(grid_for(1ull << 40, 256, 16384) == 16384);                  // a grid-stride kernel's cap
		CHECK(grid_for(16384ull * 256, 256, 16384) == 16384 && grid_for(16384ull * 256 - 256, 256, 16384) == 16383);
		CHECK(grid_for(~0ull - 255, 256) == 0xffffffffu);                  // (n + block - 1 does not wrap below 2^64 - block; the default cap)
	}
	std::printf("ok\n");
	return 0;
}
"""


def _compiler():
    for name in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def test_layout_program_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "call_image_check.cpp"
    exe = tmp_path / "call_image_check"
    src.write_text(PROGRAM)
    # (g++ links the sanitizers' runtimes as shared libraries unless told otherwise; linked in, they start first whatever else the process loads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                   ["-I" + CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
