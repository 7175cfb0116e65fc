// bucket_order.hpp -- step 3 of the in-LDS pass (radix_lds_bucket.hpp) as plain C++: one thread puts each of its buckets of two
// words or more in order, in the stage.  __host__ __device__, templated on the word type, no LDS and no lane in sight: the kernel
// passes a pointer to its stage and a function that reads the thread's table entries, tests/cpp/test_bucket_order.cpp does the
// same on the host (every 0-1 input and every permutation of the networks, the mask walk against std::sort).
//
// Words are UNIQUE (every word carries its slot), so min / max networks order them exactly, and the pad ~0 is larger than every word.
//
// The walk.  A thread owns BPT buckets; entry(j) is bucket j's `start | length << 16`.  With uniformly drawn keys a bucket holds a
// Poisson(1) number of words: 26 % of them two or more, 0.37 % five or more.  A loop over all BPT buckets runs the 4-word body BPT
// times per wave with a quarter of the lanes at work, and the 8-word body whenever one lane of 64 needs it.  Here each thread keeps
// two bit masks of BPT bits -- buckets of two words or more, buckets of five or more -- and visits only the set bits: a wave makes
// as many trips as its busiest lane has such buckets (about 9 of 16), and the rare long buckets have left the common loop.
// The next entry is read before the current bucket is ordered, so a trip's table read is off its chain of LDS round trips.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GLU_BUCKET_HD __host__ __device__ __forceinline__
#else
#define GLU_BUCKET_HD inline
#endif

namespace glu_hip
{
// a bucket longer than this makes the run a crowded one (radix_lds_bucket.hpp): the insertion below is quadratic, one lane at work
constexpr uint32_t kBucketMaxLen = 24;

template<typename WordT>
GLU_BUCKET_HD void bucket_cx(WordT& a, WordT& b)
{
    const WordT lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo, b = hi;
}

// m = 2 .. 4 words at p.  All four places are read: p[2] and p[3] of a shorter bucket are the next buckets' first words, or the
// stage's pad behind the last bucket (the caller's stage has three words to spare there) -- words that the threads owning those
// buckets may be writing at this moment.  Whatever is read there is replaced by the pad before it is used and never written back,
// so the result does not depend on it; the loads stay unconditional because a select is cheaper than a branch around a load.
template<typename WordT>
GLU_BUCKET_HD void bucket_order4(WordT* p, uint32_t m)
{
    constexpr WordT PAD = (WordT) ~(WordT) 0;
    WordT x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
    x2 = m > 2u ? x2 : PAD;
    x3 = m > 3u ? x3 : PAD;
    bucket_cx(x0, x1), bucket_cx(x2, x3), bucket_cx(x0, x2), bucket_cx(x1, x3), bucket_cx(x1, x2);
    p[0] = x0, p[1] = x1;
    if (m > 2u) p[2] = x2;
    if (m > 3u) p[3] = x3;
}

// m = 5 .. 8 words at p (places behind the bucket: as above); odd-even merge sort of 8, 19 exchanges
template<typename WordT>
GLU_BUCKET_HD void bucket_order8(WordT* p, uint32_t m)
{
    constexpr WordT PAD = (WordT) ~(WordT) 0;
    WordT x[8];
#pragma unroll
    for (int e = 0; e < 8; e++) x[e] = p[e];
#pragma unroll
    for (int e = 5; e < 8; e++) x[e] = m > (uint32_t) e ? x[e] : PAD;
    bucket_cx(x[0], x[1]), bucket_cx(x[2], x[3]), bucket_cx(x[4], x[5]), bucket_cx(x[6], x[7]);
    bucket_cx(x[0], x[2]), bucket_cx(x[1], x[3]), bucket_cx(x[4], x[6]), bucket_cx(x[5], x[7]);
    bucket_cx(x[1], x[2]), bucket_cx(x[5], x[6]);
    bucket_cx(x[0], x[4]), bucket_cx(x[1], x[5]), bucket_cx(x[2], x[6]), bucket_cx(x[3], x[7]);
    bucket_cx(x[2], x[4]), bucket_cx(x[3], x[5]);
    bucket_cx(x[1], x[2]), bucket_cx(x[3], x[4]), bucket_cx(x[5], x[6]);
#pragma unroll
    for (int e = 0; e < 8; e++)
        if (m > (uint32_t) e) p[e] = x[e];
}

// any m (9 .. kBucketMaxLen in the walk: one bucket in 10^6 for uniformly drawn keys): insertion in the stage, inside [p, p + m)
template<typename WordT>
GLU_BUCKET_HD void bucket_order_insertion(WordT* p, uint32_t m)
{
    for (uint32_t a = 1u; a < m; a++)
    {
        const WordT x = p[a];
        uint32_t b = a;
        while (b > 0u)
        {
            const WordT y = p[b - 1u];
            if (y < x) break;
            p[b] = y;
            b--;
        }
        p[b] = x;
    }
}

// The first mask of a thread's BPT entries: bit j = bucket j holds two words or more.  (One compare per entry: which of these hold five
// or more is found where the entry is in hand anyway, in the walk.)
template<int BPT, typename EntryFn>
GLU_BUCKET_HD uint32_t bucket_order_mask(EntryFn entry)
{
    static_assert(BPT >= 1 && BPT <= 32, "one mask bit per bucket of the thread");
    uint32_t todo = 0u;
#pragma unroll
    for (int j = 0; j < BPT; j++) todo |= (entry(j) >= (2u << 16) ? 1u : 0u) << j;
    return todo;
}

// One thread's buckets: entry(j), j < BPT, is `start | length << 16` of its j-th bucket in `stage`.  Two worklists, as bit masks:
// first every bucket of two words or more takes the 4-word network -- one of five or more on its first four words, which does no
// harm, sets its bit in the second mask and so keeps the branch out of the common loop --, then the second mask takes the 8-word
// network or the insertion.
template<int BPT, typename WordT, typename EntryFn>
GLU_BUCKET_HD void bucket_order_walk(WordT* stage, EntryFn entry)
{
    uint32_t todo = bucket_order_mask<BPT>(entry), many = 0u;
    // (entry(0) where the mask is empty: a read nobody uses, in place of a branch)
    uint32_t j_next = todo ? (uint32_t) __builtin_ctz(todo) : 0u, hm_next = entry((int) j_next);
    while (todo != 0u)
    {
        const uint32_t hm = hm_next, j = j_next, m = hm >> 16;
        todo &= todo - 1u;
        if (todo != 0u) j_next = (uint32_t) __builtin_ctz(todo), hm_next = entry((int) j_next);
        many |= (m > 4u ? 1u : 0u) << j;
        bucket_order4(stage + (hm & 0xFFFFu), m < 4u ? m : 4u);
    }
    while (many != 0u)
    {
        const uint32_t hm = entry(__builtin_ctz(many)), m = hm >> 16;
        many &= many - 1u;
        if (m <= 8u)
            bucket_order8(stage + (hm & 0xFFFFu), m);
        else
            bucket_order_insertion(stage + (hm & 0xFFFFu), m);
    }
}

} // namespace glu_hip
