// run_teams.h -- what a team of lanes needs to reduce a run of entries id by id; shared by haplotag_device.hip, tagphase_device.hip and
// polythread_device.hip.  A team is RS_SEGMENT lanes (class a), a wave (class b) or a workgroup of RS_BLOCK threads (class c); lane l of
// a team takes entries l, l + STRIDE, ... of its run.  Every lane of a wave (of the workgroup, for BlockScope) calls these functions
// together: a team without a run, or one that is done, walks along idle so that every shuffle, ballot and barrier is met by all.
//   lane reductions   team_sum, team_min over W neighbouring lanes.
//   read lookup       read_of_entry: the read of an entry of a read-major layer, searched among the reads of the workgroup's entries.
//   scopes            TeamScope<W>, BlockScope<Acc>: STRIDE, all_min, and combine() of a layer-defined accumulator -- a POD with
//                     across<W>() (reduce yourself over W lanes) and merge(other).
//   walk_ids          the distinct ids of a run in ascending order: per id one pass for the smallest id not below the last one's
//                     successor, then the layer's body (its second pass and what it does with the result).
//   SlotNames<R>      the register route's slot naming: up to R ids in the order of their first encounter, named by ballot.
//   segment_key       class a's key: which key a segment of a per-key launch owns, and whether it is class a's.
#pragma once
#include "run_scatter.h"

#if defined(__HIPCC__)
namespace whamd {

constexpr int RT_WAVES = (int)RS_BLOCK / 64;   // waves of a workgroup
constexpr uint32_t RT_NONE = RS_NONE;          // no id: never the next one, never named

// ---------------------------------------------------------------------------------------------- lane reductions
template <int W, class T>
__device__ inline T team_sum(T v) {
#pragma unroll
	for (int o = W / 2; o; o >>= 1) v += __shfl_xor(v, o);
	return v;
}
template <int W>
__device__ inline uint32_t team_min(uint32_t v) {
#pragma unroll
	for (int o = W / 2; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
	return v;
}

// ---------------------------------------------------------------------------------------------- read lookup
// The largest r in [lo, hi] with read_ptr[r] <= i (read_ptr[lo] <= i).
__device__ inline uint32_t find_read(const uint32_t* read_ptr, uint32_t lo, uint32_t hi, uint32_t i) {
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo + 1) / 2;
		if (read_ptr[mid] <= i) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

// The read of entry i < n_entries in a launch of one thread per entry, RS_BLOCK per workgroup: the search is narrowed to the reads of
// the workgroup's entries.  Reads without entries are skipped: the last read that begins at or before i is the one that holds it.
__device__ inline uint32_t read_of_entry(const uint32_t* read_ptr, uint32_t n_reads, uint32_t n_entries, uint32_t i) {
	const uint32_t i0 = blockIdx.x * RS_BLOCK, i1 = min(i0 + RS_BLOCK - 1, n_entries - 1);
	const uint32_t lo = find_read(read_ptr, 0, n_reads - 1, i0), hi = find_read(read_ptr, lo, n_reads - 1, i1);
	return find_read(read_ptr, lo, hi, i);
}

// ---------------------------------------------------------------------------------------------- scopes
// Who owns a run: how far apart its lanes' entries lie and how its lanes combine a minimum and an accumulator.
template <int W>
struct TeamScope {
	static constexpr uint32_t STRIDE = W;
	__device__ uint32_t all_min(uint32_t v) const { return team_min<W>(v); }
	template <class Acc>
	__device__ void combine(Acc& acc) const { acc.template across<W>(); }
};
template <class Acc>
struct BlockScope {   // (one run per workgroup: every thread takes the same branches, so the barriers are met by all)
	static constexpr uint32_t STRIDE = RS_BLOCK;
	uint32_t* word;   // LDS [RT_WAVES]
	Acc* part;        // LDS [RT_WAVES]
	uint32_t lane, w;
	__device__ uint32_t all_min(uint32_t v) const {
		v = team_min<64>(v);
		if (lane == 0) word[w] = v;
		__syncthreads();
		v = word[0];
#pragma unroll
		for (int ww = 1; ww < RT_WAVES; ww++) v = min(v, word[ww]);
		__syncthreads();
		return v;
	}
	__device__ void combine(Acc& acc) const {   // one butterfly in the wave, two barriers
		acc.template across<64>();
		if (lane == 0) part[w] = acc;
		__syncthreads();
		acc = part[0];
#pragma unroll
		for (int ww = 1; ww < RT_WAVES; ww++) acc.merge(part[ww]);
		__syncthreads();
	}
};

// ---------------------------------------------------------------------------------------------- the ascending-id walk
// One pass over run[0, n) by the owners that are `active`: f(i) for every entry i of the calling lane.  (Inlined before anything else
// is done to it: f accumulates into its caller's registers.)
template <class Scope, class F>
__device__ __forceinline__ void team_pass(uint32_t n, uint32_t l, bool active, const F& f) {
	for (uint32_t base = 0; __any(active && base < n); base += Scope::STRIDE) {
		const uint32_t i = base + l;
		if (active && i < n) f(i);
	}
}

// The distinct ids of run[0, n) in ascending order, for the owners with `need`.  id_of(i): the id of entry i, or RT_NONE.  All lanes
// call body(id, active, ordinal) together once per trip -- on an owner's last trip `active` has just turned false and id is RT_NONE --
// so the collectives inside the body are met by every lane.  Returns the number of ids.
template <class Scope, class IdOf, class Body>
__device__ inline uint32_t walk_ids(const Scope& scope, uint32_t n, uint32_t l, bool need, IdOf id_of, Body body) {
	bool active = need;
	uint32_t lower = 0, ordinal = 0;
	while (__any(active)) {
		uint32_t next = RT_NONE;
		team_pass<Scope>(n, l, active, [&](uint32_t i) {
			const uint32_t id = id_of(i);
			if (id >= lower) next = min(next, id);
		});
		next = scope.all_min(next);
		if (next == RT_NONE) active = false;
		body(next, active, ordinal);
		if (active) {
			ordinal++;
			lower = next + 1;
		}
	}
	return ordinal;
}

// ---------------------------------------------------------------------------------------------- slot naming
// Up to R ids kept in registers, in the order of their first encounter by a team that walks its run in chunks of its width.
template <int R>
struct SlotNames {
	uint32_t ps[R];
	uint32_t n;
	bool overflow;   // more than R ids: the team takes walk_ids instead
	__device__ void clear() {
		n = 0;
		overflow = false;
#pragma unroll
		for (int s = 0; s < R; s++) ps[s] = RT_NONE;
	}
	// One chunk: the slot of the lane's entry (valid, id), -1 for none.  The lanes of the chunk whose id has no slot yet are found with a
	// ballot; the lowest of them names the next slot (a chunk is consecutive entries, so the lowest lane is the first encounter) and
	// named(slot, source lane) fires.  teammask: the team's lanes in the wave; self: the calling lane.
	template <class Named>
	__device__ int claim(bool valid, uint32_t id, uint64_t teammask, uint32_t self, Named named) {
		SlotNames t = *this;   // (a copy of its own: the caller's may sit behind a reference, and the loop is to run in registers)
		int slot = -1;
#pragma unroll
		for (int s = 0; s < R; s++)
			if (valid && t.ps[s] == id) slot = s;
		for (;;) {
			const uint64_t un = __ballot(valid && slot < 0 && !t.overflow) & teammask;
			if (!__any(un != 0)) break;
			const uint32_t src = un ? (uint32_t)__ffsll((unsigned long long)un) - 1 : self;
			const uint32_t fresh = (uint32_t)__shfl((int)id, (int)src);
			if (un) {
				if (t.n < (uint32_t)R) {
#pragma unroll
					for (int s = 0; s < R; s++)
						if (t.n == (uint32_t)s) {
							t.ps[s] = fresh;
							named(s, src);
						}
					if (valid && id == fresh) slot = (int)t.n;
					t.n++;
				} else {
					t.overflow = true;
				}
			}
		}
		*this = t;
		return slot;
	}
};

// ---------------------------------------------------------------------------------------------- class a's key
// A launch of RS_SEGMENT lanes per key over all keys: the segment's key v, the lane l in the segment, and have: the key exists and
// its run is class a's (the longer ones are left to the lists).
struct SegmentKey {
	uint32_t v, l;
	bool have;
};
__device__ inline SegmentKey segment_key(const RunIndex& x) {
	const uint64_t v64 = (uint64_t)blockIdx.x * (RS_BLOCK / RS_SEGMENT) + threadIdx.x / RS_SEGMENT;
	return SegmentKey{(uint32_t)v64, threadIdx.x & (RS_SEGMENT - 1), v64 < x.n_keys && x.counts[v64] <= x.a_max};
}

}  // namespace whamd
#endif
