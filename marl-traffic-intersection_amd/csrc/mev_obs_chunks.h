// mev_obs_chunks.h — how a run of floats inside an observation row is cut into
// 16-byte stores: pure arithmetic, no HIP.  tests/native/obs_chunks_check.cpp proves
// it over every row phase.  No kernel stores by it today: the 16-byte row stores it
// was written for lost to one dword per lane, plain or write-through (DESIGN.md 9,
// "Observation rows: write-through, 16-byte and non-temporal stores"); it stays for
// the next store shape that needs rows cut by address.
#pragma once

#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)  // a plain C++ compiler
#define __host__
#define __device__
#endif

namespace mev {

// A slice of `len` floats whose first float sits at byte address `addr` (a
// multiple of 4), cut by absolute address: floats [0, prefix) and
// [prefix + 4 * chunks, len) are single-float stores (at most 3 each), and chunk
// c covers floats [prefix + 4 c, prefix + 4 c + 4), at a 16-byte aligned address
// and wholly inside the slice.  It depends on nothing but the address and the
// length, so it holds for any caller's buffer, row stride or beam count.
struct ObsSplit {
    int prefix;  // single floats before the first chunk (= the first chunk's float offset)
    int chunks;  // whole 16-byte chunks
    int suffix;  // single floats after the last chunk
};

__host__ __device__ inline ObsSplit obs_split(uint64_t addr, int len) {
    ObsSplit s;
    const int lead = (int)((0u - (uint32_t)(addr >> 2)) & 3u);  // floats up to the next 16-byte boundary
    s.prefix = lead < len ? lead : len;
    s.chunks = (len - s.prefix) >> 2;
    s.suffix = len - s.prefix - 4 * s.chunks;
    return s;
}

// The single floats of a slice in one index space [0, 6): slots 0-2 the prefix,
// 3-5 the suffix.  Returns the float's offset in the slice, or -1 for a slot
// that the slice does not use.
__host__ __device__ inline int obs_split_single(const ObsSplit& s, int slot) {
    if (slot < 3) return slot < s.prefix ? slot : -1;
    return slot - 3 < s.suffix ? s.prefix + 4 * s.chunks + (slot - 3) : -1;
}

}  // namespace mev
