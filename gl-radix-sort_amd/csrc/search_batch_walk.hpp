// search_batch_walk.hpp -- the arithmetic of the BATCHED SORTED SEARCH (sorted_search_batch_kernels.hpp, glu_sorted_search.hip) in
// plain C++: which needles a tile holds, the first and the last segment of a tile, the segment of a needle between them, whether a
// needle is covered, the range of a segment's haystack with its clamps, whether the haystacks of a tile are staged in LDS, where a
// needle's haystack lies in the staged window or in global memory, the equal-rows arithmetic and the plan.  The kernel includes
// this header, and tests/test_search_batch_walk.py includes it with a host compiler and performs whole calls through it, tile by
// tile, at small tiles and windows as well as the real ones: what holds there (every index into the two offsets arrays at most
// num_segments, every key read inside [0, hay_total) or inside the window, every needle written at most once, whatever the offsets
// hold) holds on the device.
//
// A call: S = num_segments segments.  Segment s has the haystack [hb, he) of `hay` and the needles [nb, ne) of `needles`; either
// side is given by device offsets (S + 1 words, non-decreasing, never read by the host) or by equal rows (s * count).  The kernel is
// load-balanced over the NEEDLES: a tile is a run of consecutive needles, whatever segments they belong to.
#pragma once

#include "histogram_bins.hpp" // the exact quotient by a kernel-uniform divisor (hist_div), hist_steps
#include "tile_span.hpp"

namespace glu_hip
{
constexpr uint32_t kSearchBatchPacks = 2;           // 16-byte packs of needles per thread and tile (kSearchPacks of the single search)
constexpr uint32_t kSearchBatchLdsBytes = 32768;    // the staged window at the most: 8192 4-byte or 4096 8-byte keys
constexpr uint32_t kSearchBatchMinWindow = 16;      // a window is 0 (never stage) or at least this many keys
constexpr uint32_t kSearchBatchWindowUnset = 0xFFFFFFFFu; // the object's window before set_batch_window: the maximum of the call's key width

constexpr uint32_t search_batch_tile(uint32_t key_bytes) { return tile_elems(key_bytes, kSearchBatchPacks); }
constexpr uint32_t search_batch_max_window(uint32_t key_bytes) { return kSearchBatchLdsBytes / key_bytes; }

// tile = needles per workgroup and tile, tiles = ceil(needle_total / tile) (one more where the needles start inside a pack and
// their end crosses into another tile), window = the window in keys as the kernel uses it, one kernel unless there is no needle
struct SearchBatchPlan
{
    uint32_t tile, tiles, window, kernels;
};
// window_keys: 0, kSearchBatchWindowUnset or a value the caller has checked against search_batch_window_ok
inline SearchBatchPlan search_batch_plan(uint64_t needle_total, uint32_t key_bytes, uint32_t window_keys)
{
    SearchBatchPlan p;
    const TilePlan t = tile_plan(needle_total, key_bytes, kSearchBatchPacks);
    p.tile = t.tile;
    p.tiles = t.tiles;
    p.window = window_keys == kSearchBatchWindowUnset ? search_batch_max_window(key_bytes) : window_keys;
    p.kernels = needle_total ? 1u : 0u;
    return p;
}
inline bool search_batch_window_ok(uint64_t keys, uint32_t key_bytes)
{
    return keys == 0 || (keys >= kSearchBatchMinWindow && keys <= search_batch_max_window(key_bytes));
}

// ---- the needles of a tile ---------------------------------------------------------------------------------------------------------
// Tile t holds the elements [t * tile, (t + 1) * tile) of the span's base, of which [lo, hi) are the array (tile_span.hpp): the
// needles [*j0, *j1) of the array, j1 <= needle_total.  False where it holds none (no tile below the span's `tiles` does).
GLU_HIST_FN bool search_batch_tile_needles(uint32_t t, uint32_t tile, uint64_t lo, uint64_t hi, uint32_t* j0, uint32_t* j1)
{
    const uint64_t first = (uint64_t) t * tile, end = first + tile;
    const uint64_t a = first > lo ? first : lo, b = end < hi ? end : hi;
    *j0 = a < b ? (uint32_t) (a - lo) : 0u;
    *j1 = a < b ? (uint32_t) (b - lo) : 0u;
    return a < b;
}

// ---- segments from device offsets ---------------------------------------------------------------------------------------------------
// The clamped bound: how many of the `len` keys at(base), at(base + 1), .. lie in front of the bound of x (UPPER: the keys <= x,
// else the keys < x), built bit by bit from the top as the single search builds it (search_range of sorted_search_kernels.hpp with
// one needle: the same trips, probes and clamp).  `steps` = hist_steps of a length >= len, the same for the callers that run side by
// side.  at(i) is called with base <= i < base + len only; keys that are not sorted give some count in 0 .. len.
template<bool UPPER, typename X, typename At>
GLU_HIST_FN uint32_t search_batch_bound(X x, uint32_t base, uint32_t len, uint32_t steps, At at)
{
    uint32_t pos = 0;
    for (uint32_t step = steps ? 1u << (steps - 1) : 0u; step; step >>= 1)
    {
        const uint32_t next = pos + step;
        const uint32_t probe = next < len ? next : len; // 1 <= probe <= len where len > 0
        const X key = len ? at(base + probe - 1u) : (X) 0;
        pos = (next <= len && (UPPER ? key <= x : key < x)) ? next : pos;
    }
    return pos;
}
// over offsets: how many of them are <= x
template<typename At>
GLU_HIST_FN uint32_t search_batch_upper_bound(uint32_t x, uint32_t base, uint32_t len, uint32_t steps, At at)
{
    return search_batch_bound<true, uint32_t>(x, base, len, steps, at);
}

// trips of the bound over all S + 1 offsets (num_segments <= 2^24)
GLU_HIST_FN uint32_t search_batch_end_steps(uint32_t num_segments) { return hist_steps(num_segments + 1u); }

// The segment of an END of a tile (its first or its last needle j): the last segment that begins at or in front of j, held into
// [0, num_segments - 1]: a needle in front of offsets[0] gets segment 0 and one behind offsets[S] segment S - 1, and neither is
// covered (search_batch_covered).  num_segments >= 1.  offset_at(i): i <= num_segments.
template<typename OffsetAt>
GLU_HIST_FN uint32_t search_batch_end_segment(uint32_t j, uint32_t num_segments, OffsetAt offset_at)
{
    const uint32_t c = search_batch_upper_bound(j, 0u, num_segments + 1u, search_batch_end_steps(num_segments), offset_at);
    const uint32_t s = c ? c - 1u : 0u;
    return s < num_segments ? s : num_segments - 1u;
}

// the last segment of a tile is never in front of its first (offsets that are not sorted could say so)
GLU_HIST_FN uint32_t search_batch_last_segment(uint32_t s_first, uint32_t s_last) { return s_last > s_first ? s_last : s_first; }

// The segment of a needle of the tile lies in [s_first, s_last]: s_first + the offsets among offsets[s_first + 1 .. s_last] that
// are <= j.  These give the range and the trips of that bound: no trip where the tile lies inside one segment.  A run of empty
// segments drops out by itself, since the bound steps over all the offsets equal to j at once.
GLU_HIST_FN uint32_t search_batch_inner_base(uint32_t s_first) { return s_first + 1u; }
GLU_HIST_FN uint32_t search_batch_inner_len(uint32_t s_first, uint32_t s_last) { return s_last - s_first; }
GLU_HIST_FN uint32_t search_batch_inner_steps(uint32_t s_first, uint32_t s_last) { return hist_steps(s_last - s_first); }
// `count` = the bound's answer, 0 .. s_last - s_first; the segment is at most s_last <= num_segments - 1 whatever it is
GLU_HIST_FN uint32_t search_batch_inner_segment(uint32_t s_first, uint32_t s_last, uint32_t count)
{
    const uint32_t len = s_last - s_first;
    return s_first + (count < len ? count : len);
}

// needle j belongs to its segment [nb, ne) of the needle offsets: expand's rule (needles in front of offsets[0] or at or behind
// offsets[S] belong to none and are not touched)
GLU_HIST_FN bool search_batch_covered(uint32_t j, uint32_t nb, uint32_t ne) { return nb <= j && j < ne; }

// ---- equal rows ---------------------------------------------------------------------------------------------------------------------
// Needle j of rows of m needles: segment j / m, by histogram's multiplication, exact for every j < 2^32 and every m >= 1.
struct SearchBatchRows
{
    HistEvenInt by_m;  // magic and w_is_one for W = m; lo and span unused
    uint32_t m;        // needles of a row, >= 1 (0 where the needles come from offsets)
    uint32_t hay_count; // equal partitions: keys of a row of the haystack (unused where the haystack comes from offsets)
};
inline SearchBatchRows search_batch_make_rows(uint32_t m, uint32_t hay_count)
{
    SearchBatchRows r = {};
    r.by_m.lo = 0u;
    r.by_m.span = 0xFFFFFFFFu;
    r.by_m.w_is_one = m <= 1u ? 1u : 0u;
    r.by_m.magic = m <= 1u ? 0ull : 0xFFFFFFFFFFFFFFFFull / m + 1ull; // ceil(2^64 / m) for m >= 2
    r.m = m;
    r.hay_count = hay_count;
    return r;
}
// j < num_segments * m, so the row is below num_segments; held there all the same
GLU_HIST_FN uint32_t search_batch_row(uint32_t j, const SearchBatchRows& r, uint32_t num_segments)
{
    const uint32_t s = hist_div(j, r.by_m);
    return s < num_segments ? s : num_segments - 1u;
}

// ---- the haystack of a segment ------------------------------------------------------------------------------------------------------
// Segment [b, e) of device offsets, which the host cannot check: one that ends below its begin or beyond `total` is empty
// (batch_offsets_segment of batch_lists.hpp, on the two words already loaded).  Then begin + len <= total.
GLU_HIST_FN void search_batch_offsets_segment(uint32_t b, uint32_t e, uint32_t total, uint32_t* begin, uint32_t* len)
{
    if (e < b || e > total) e = b;
    *begin = b;
    *len = e - b;
}

// The haystacks of the segments s_first .. s_last are the range [w0, w1) of `hay`, w0 the begin of the first and w1 the end of the
// last.  It is staged in LDS iff it is a range of [0, hay_total) of at most `window` keys (window 0: never).  Workgroup-uniform.
GLU_HIST_FN bool search_batch_staged(uint32_t w0, uint32_t w1, uint32_t hay_total, uint32_t window)
{
    return window != 0u && w0 <= w1 && w1 <= hay_total && w1 - w0 <= window;
}

// Staged: the haystack [begin, begin + len) of a needle as keys [*base, *base + *len) of the window of n = w1 - w0 keys, held
// inside it whatever the offsets say: *base + *len <= n.
GLU_HIST_FN void search_batch_window_range(uint32_t begin, uint32_t len, uint32_t w0, uint32_t w1, uint32_t* base, uint32_t* out_len)
{
    const uint32_t n = w1 - w0;
    const uint32_t b = begin < w0 ? 0u : (begin - w0 < n ? begin - w0 : n);
    *base = b;
    *out_len = len < n - b ? len : n - b;
}

// Not staged: the same inside [0, hay_total): *base + *len <= hay_total.
GLU_HIST_FN void search_batch_global_range(uint32_t begin, uint32_t len, uint32_t hay_total, uint32_t* base, uint32_t* out_len)
{
    const uint32_t b = begin < hay_total ? begin : hay_total;
    *base = b;
    *out_len = len < hay_total - b ? len : hay_total - b;
}

} // namespace glu_hip
