// merge_path.hpp -- the arithmetic of MERGE (merge_kernels.hpp, glu_merge.hip) in plain C++: the tile of a call, the split of a
// diagonal between two sorted arrays, the ranges of a tile with their clamps, the split of a tile among its threads and the serial
// merge of one thread.  Both merge kernels include this header, and tests/test_merge_path.py includes it with a host compiler and
// merges whole arrays through it: what holds there (every range inside its array, the outputs tiling [0, total) exactly, whatever
// the keys hold) holds on the device.
//
// The order is the one of the ENCODED keys (unsigned); the accessors hand out encoded keys.  A comes first on ties.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GLU_MERGE_FN __host__ __device__ __forceinline__
#define GLU_MERGE_UNROLL _Pragma("unroll")
#else
#define GLU_MERGE_FN inline // (a host compiler: the test program)
#define GLU_MERGE_UNROLL
#endif

namespace glu_hip
{
constexpr uint32_t kMergeThreads = 256;

// Outputs per thread and tile, fixed once per key width (the same with and without values).  Odd: neighbouring lanes start their
// serial merge ITEMS words apart in LDS.  256 x 11 4-byte keys and values are 22 KiB of LDS, 256 x 7 8-byte keys and their values 21.
constexpr uint32_t merge_items(uint32_t key_bytes, bool /*with_vals*/) { return key_bytes == 4 ? 11u : 7u; }
constexpr uint32_t merge_tile(uint32_t key_bytes, bool with_vals) { return kMergeThreads * merge_items(key_bytes, with_vals); }

// trips of the split loop over a range of `len` candidates: the split is one of 0 .. len  (search_steps of sorted search)
GLU_MERGE_FN uint32_t merge_steps(uint32_t len) { return len ? 32u - (uint32_t) __builtin_clz(len) : 0u; }

// The first `d` outputs of the merge of A (na keys) and B (nb keys) hold how many keys of A?  d <= na + nb.  The answer lies in
// [max(0, d - nb), min(d, na)], a range of at most min(na, nb) candidates, and it is built bit by bit from the top as the bounds
// of sorted search are: m more keys of A belong in front of the diagonal iff enc(A[m - 1]) <= enc(B[d - m]) (A first on ties).
// `steps`: merge_steps of anything >= the range's length (kernel-uniform: merge_steps(min(na, nb))).  Every probe is clamped into
// its array: a_at(i, any) and b_at(j, any) are called with i < na and j < nb where `any`, and must not read where !any.  Inputs
// that are not sorted give some split inside the range and never a read outside.
template<typename KeyA, typename KeyB>
GLU_MERGE_FN uint32_t merge_diag_split(uint32_t d, uint32_t na, uint32_t nb, uint32_t steps, KeyA a_at, KeyB b_at)
{
    const uint32_t lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    const uint32_t len = hi - lo; // (lo <= hi because d <= na + nb)
    const bool any = len != 0u;
    uint32_t pos = 0;
    for (uint32_t step = steps ? 1u << (steps - 1) : 0u; step; step >>= 1)
    {
        const uint32_t next = pos + step;
        const uint32_t probe = next < len ? next : len; // clamped: 1 <= probe <= len where any
        const uint32_t ia = any ? lo + probe - 1u : 0u; // lo <= ia < hi <= na
        const uint32_t ib = any ? d - 1u - ia : 0u;     // d - hi <= ib <= d - 1 - lo: 0 <= ib < nb
        const bool passes = a_at(ia, any) <= b_at(ib, any);
        pos = (next <= len && passes) ? next : pos;
    }
    return lo + pos;
}

// The outputs [d0, d1) of a tile are A[a0, a1) and B[b0, b1) merged.  split0 and split1 are the splits of the diagonals d0 and d1
// (merge_diag_split: max(0, d - nb) <= split <= min(d, na)).  With sorted inputs 0 <= split1 - split0 <= d1 - d0 by itself; the
// clamp enforces it, and then all four ends lie inside A and B whatever the keys hold:
//   a1 = split0 <= na, b1 = d1 - split0 < nb   where split1 < split0   (split0 > split1 >= d1 - nb)
//   a1 < split1 <= na, b1 = b0 <= nb           where split1 > split0 + (d1 - d0)   (split0 >= d0 - nb)
struct MergeRanges
{
    uint32_t a0, a1, b0, b1;
};
GLU_MERGE_FN MergeRanges merge_tile_ranges(uint32_t split0, uint32_t split1, uint32_t d0, uint32_t d1)
{
    MergeRanges r;
    const uint32_t most = split0 + (d1 - d0); // (split0 <= d0: no overflow)
    r.a0 = split0;
    r.a1 = split1 < split0 ? split0 : (split1 > most ? most : split1);
    r.b0 = d0 - r.a0;
    r.b1 = d1 - r.a1;
    return r;
}

// the diagonal of thread `tid` inside a tile of `count` outputs, ITEMS consecutive outputs per thread
GLU_MERGE_FN uint32_t merge_thread_diag(uint32_t tid, uint32_t items, uint32_t count) { return tid * items < count ? tid * items : count; }

// One thread's outputs: `todo` (<= ITEMS) steps from (i, j), i of the tile's na keys of A and j of its nb keys of B already in front
// of it, i + j + todo <= na + nb.  The tile's keys lie side by side: key_at(x, any) is key x of A for x < na and key x - na of B for
// na <= x < na + nb, read only where any.  emit(s, x, key, live) for s = 0 .. ITEMS - 1: output s of the thread is key x (live), or
// the thread has no output s.  One key is read per step; every x read or emitted is below na + nb whatever the keys hold, because a
// side that has run out is never taken.
template<uint32_t ITEMS, typename K, typename KeyAt, typename Emit>
GLU_MERGE_FN void merge_serial(uint32_t i, uint32_t j, uint32_t na, uint32_t nb, uint32_t todo, KeyAt key_at, Emit emit)
{
    K ka = key_at(i, todo != 0u && i < na), kb = key_at(na + j, todo != 0u && j < nb);
    GLU_MERGE_UNROLL
    for (uint32_t s = 0; s < ITEMS; s++)
    {
        const bool live = s < todo;
        const bool take_a = live && (j >= nb || (i < na && ka <= kb)); // (live: i < na or j < nb)
        emit(s, take_a ? i : na + j, take_a ? ka : kb, live);
        i += take_a ? 1u : 0u;
        j += (live && !take_a) ? 1u : 0u;
        const bool more = s + 1u < todo && (take_a ? i < na : j < nb);
        const K next = key_at(take_a ? i : na + j, more);
        ka = take_a ? next : ka;
        kb = take_a ? kb : next;
    }
}

} // namespace glu_hip
