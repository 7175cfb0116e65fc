// topk_pick.hpp -- the arithmetic of TOP-K (topk_kernels.hpp, glu_top_k.hip) in plain C++: the digit windows of a radix select per
// key width, the digit at which the cumulative count first reaches what is still needed, the update of the state after a round, the
// choice between the two paths and the plan of a call.  The kernels include this header, and tests/test_top_k_pick.py includes it with
// a host compiler and runs whole selects through it: what holds there (1 <= need <= count[d] after every round, less + need == k at
// the end) holds on the device.
//
// A select works on CODE WORDS: c = KeyCodec::encode(key), complemented for `largest`, so that every case is "the k smallest unsigned
// words".  Digits are taken from the top, 11 bits each: 11 + 11 + 10 for 4-byte keys, 5 x 11 + 9 for 8-byte keys.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define GLU_TOPK_FN __host__ __device__ __forceinline__
#else
#define GLU_TOPK_FN inline // (a host compiler: the test program)
#endif

namespace glu_hip
{
constexpr uint32_t kTopkDigitBits = 11;
constexpr uint32_t kTopkBins = 1u << kTopkDigitBits;  // counters of a table at the most
constexpr uint32_t kTopkMinCapacity = 1u << 16;       // candidates the object keeps at the least
constexpr uint32_t kTopkCapacityShare = 512;          // default capacity: ceil(count / 512); uniform keys fill count / 2048
constexpr uint32_t kTopkThreads = 256, kTopkPacks = 4; // a tile of the streaming kernels: select's and the even histogram's
constexpr uint32_t kTopkGroupsMax = 1024;             // rows of the partial table at the most (the even histogram's)
constexpr uint32_t kTopkPickThreads = 1024;           // the one workgroup that picks: two counters a thread

enum
{
    TOPK_PATH_AUTO = 0,   // an option only: CANDIDATES where the bucket fits
    TOPK_PATH_CANDIDATES, // the bucket of round 1 was collected; the remaining rounds read the candidates
    TOPK_PATH_FULL        // the remaining rounds read the input again, filtered by the prefix
};

GLU_TOPK_FN uint32_t topk_rounds(uint32_t key_bytes) { return key_bytes == 4 ? 3u : 6u; }
// round r takes the bits [shift, shift + bits) of the code word
GLU_TOPK_FN uint32_t topk_shift(uint32_t key_bytes, uint32_t r)
{
    const uint32_t key_bits = key_bytes * 8u, top = kTopkDigitBits * (r + 1u);
    return top < key_bits ? key_bits - top : 0u;
}
GLU_TOPK_FN uint32_t topk_bits(uint32_t key_bytes, uint32_t r)
{
    const uint32_t left = key_bytes * 8u - kTopkDigitBits * r;
    return left < kTopkDigitBits ? left : kTopkDigitBits;
}
template<typename W>
GLU_TOPK_FN uint32_t topk_digit(W code, uint32_t shift, uint32_t bits)
{
    return (uint32_t) (code >> shift) & ((1u << bits) - 1u);
}

// The record a select keeps on the device.  `prefix` holds the digits fixed so far and `mask` their bits: a code word c is still in
// the running iff (c & mask) == prefix.  Among those, `need` are still to be taken (the `need` smallest); `less` words lie in front
// of the prefix and are taken whatever follows; `bucket` words match the prefix.  After the last round prefix is the threshold word
// T, bucket the number of words equal to T and need the number of ties taken.
struct TopkState
{
    uint64_t prefix, mask;
    uint32_t need, less, bucket;
    uint32_t path;   // TOPK_PATH_CANDIDATES or _FULL once round 1 has been picked
    uint32_t cand;   // candidates collected (the one word added to with an atomic)
    uint32_t totals[2]; // the sums of the two count scans of the compaction (the write kernel's last tile reads them)
    uint32_t pad_;
};

GLU_TOPK_FN TopkState topk_begin(uint32_t count, uint32_t k)
{
    TopkState s = {};
    s.need = k;
    s.bucket = count;
    s.path = TOPK_PATH_AUTO;
    return s;
}

// `before` words lie in the digits in front of this one and `c` in it: the cumulative count first reaches `need` here
GLU_TOPK_FN bool topk_crosses(uint32_t before, uint32_t c, uint32_t need) { return before < need && need - before <= c; }

// the crossing digit of a table, one counter after the other (the host and the test; the device asks topk_crosses of every digit at
// once).  `*before`: the words in front of it.  1 <= need <= the sum of the table.
template<typename CountAt>
GLU_TOPK_FN uint32_t topk_find_digit(uint32_t bins, uint32_t need, CountAt count_at, uint32_t* before)
{
    uint32_t run = 0;
    for (uint32_t d = 0; d + 1u < bins; d++)
    {
        const uint32_t c = count_at(d);
        if (topk_crosses(run, c, need))
        {
            *before = run;
            return d;
        }
        run += c;
    }
    *before = run;
    return bins - 1u;
}

// round r ended at digit d, which holds count_d words behind `before` others: 1 <= need <= count_d afterwards
GLU_TOPK_FN void topk_advance(TopkState& s, uint32_t key_bytes, uint32_t r, uint32_t d, uint32_t before, uint32_t count_d)
{
    const uint32_t shift = topk_shift(key_bytes, r), bits = topk_bits(key_bytes, r);
    s.prefix |= (uint64_t) d << shift;
    s.mask |= (uint64_t) ((1u << bits) - 1u) << shift;
    s.less += before;
    s.need -= before;
    s.bucket = count_d;
}

GLU_TOPK_FN bool topk_matches(const TopkState& s, uint64_t code) { return (code & s.mask) == s.prefix; }

// after round 1: the candidates are collected iff the option allows it and the bucket fits (a forced CANDIDATES that does not fit is FULL)
GLU_TOPK_FN uint32_t topk_choose_path(uint32_t option, uint32_t bucket, uint32_t capacity)
{
    return option != (uint32_t) TOPK_PATH_FULL && bucket <= capacity ? (uint32_t) TOPK_PATH_CANDIDATES : (uint32_t) TOPK_PATH_FULL;
}

inline uint32_t topk_default_capacity(uint64_t count)
{
    const uint64_t share = (count + kTopkCapacityShare - 1) / kTopkCapacityShare;
    return (uint32_t) (share > kTopkMinCapacity ? share : kTopkMinCapacity);
}

// ---- the plan of a call: what the host enqueues, from the sizes, the outputs and the options alone
struct TopkPlan
{
    uint32_t rounds, tile, tiles, groups, capacity, kernels;
    size_t scratch_bytes;
};

// arrays: out_keys or out_indices is given; option: TOPK_PATH_*; capacity: 0 = the default.  Kernels of a call with k > 0:
//   round 1 over the input                 count, sum, pick                            3
//   the candidates (option != FULL)        collect, the remaining rounds in one        2
//   the input again (both chains always)   count, sum, pick for each remaining round   3 * (rounds - 1)
//   the compaction (arrays)                count, two count scans, write               4
//   the ordering (arrays and sorted)       the library's sort of k pairs (counted as one), decode   2
inline TopkPlan topk_plan(uint64_t count, uint64_t max_k, uint32_t key_bytes, bool arrays, bool sorted, uint32_t option, uint32_t capacity)
{
    TopkPlan p;
    p.rounds = topk_rounds(key_bytes);
    p.tile = kTopkThreads * kTopkPacks * (16u / key_bytes);
    p.tiles = (uint32_t) ((count + p.tile - 1) / p.tile);
    p.groups = p.tiles < kTopkGroupsMax ? p.tiles : kTopkGroupsMax;
    p.capacity = capacity ? capacity : topk_default_capacity(count);
    p.kernels = 0;
    if (count && max_k)
        p.kernels = 3u + (option != (uint32_t) TOPK_PATH_FULL ? 2u : 0u) + 3u * (p.rounds - 1u) + (arrays ? 4u : 0u) + (arrays && sorted ? 2u : 0u);
    // the state and the column sums; the partial rows; the candidates; two arrays of tile counts (one tile more: tile_span.hpp);
    // the (code word, index) pairs of the ordering
    p.scratch_bytes = count ? sizeof(TopkState) + kTopkBins * sizeof(uint32_t) + (size_t) p.groups * kTopkBins * sizeof(uint32_t) +
                                  (size_t) p.capacity * key_bytes + 2 * ((size_t) p.tiles + 1) * sizeof(uint32_t) +
                                  (size_t) max_k * (key_bytes + sizeof(uint32_t))
                            : 0;
    return p;
}

} // namespace glu_hip
