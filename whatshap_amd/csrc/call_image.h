// call_image.h -- the image a batch call uploads in one copy, the grid of a launch and the times the call reports.  Host only (no HIP):
// the arithmetic is tested on its own (tests/test_call_image_host.py).  A call adds its pieces to an ImageLayout, Session::stage()
// (device_runtime.h) takes the pinned and the device block of the layout's total, and the call fills image.host(piece) and hands
// image.dev(piece) to its kernels: the type and the offset of a piece are written once.
#pragma once
#include <cstddef>
#include <cstdint>

namespace whamd {

// `count` elements of T at byte `offset` of an image.
template <class T>
struct Piece {
	size_t offset = 0, count = 0;
	size_t bytes() const { return count * sizeof(T); }
	size_t end() const { return offset + bytes(); }   // (the next piece starts at the next multiple of IMAGE_ALIGN)
};

constexpr size_t IMAGE_ALIGN = 256;   // every piece starts at a multiple of this: any vector load of a kernel is aligned

struct ImageLayout {
	size_t total = 0;   // bytes of the image so far: a multiple of IMAGE_ALIGN
	// The next piece, in the order of the calls.  A piece of no elements takes no bytes.
	template <class T>
	Piece<T> add(size_t count) {
		const Piece<T> p{total, count};
		total = (p.end() + IMAGE_ALIGN - 1) & ~(IMAGE_ALIGN - 1);
		return p;
	}
};

// A layout's two blocks: `stage` in pinned host memory, `base` on the device (Session::stage()).
struct Image {
	char* stage = nullptr;
	char* base = nullptr;
	size_t total = 0;
	template <class T>
	T* host(const Piece<T>& p) const { return reinterpret_cast<T*>(stage + p.offset); }
	template <class T>
	const T* dev(const Piece<T>& p) const { return reinterpret_cast<const T*>(base + p.offset); }
	template <class T>
	T* dev_out(const Piece<T>& p) const { return reinterpret_cast<T*>(base + p.offset); }   // a piece the kernels write
};

// Workgroups of a launch over n items, `block` items per workgroup; a grid-stride kernel caps them.
inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t cap = UINT32_MAX) { return (uint32_t)((n + block - 1) / block < cap ? (n + block - 1) / block : cap); }

// What a call reports: ms between HIP events of its stream (Session::finish()), and the kernels it launched.
struct CallTimes {
	double upload_ms = 0, kernel_ms = 0, download_ms = 0;
	uint32_t launches = 0;
};

}  // namespace whamd
