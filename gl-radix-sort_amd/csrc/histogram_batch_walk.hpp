// histogram_batch_walk.hpp -- what decides which memory the BATCHED HISTOGRAM (histogram_batch_kernels.hpp, glu_histogram.hip)
// touches, in plain C++: the segment of an index with its clamp, the class of a length, the 16-byte packs of a segment's span and
// which of their samples are the segment's, the chunks of a long segment and its run of slots in the scratch, the row of a segment
// in out_counts.  The kernels include this header, and tests/test_histogram_batch_walk.py includes it with a host compiler and
// performs whole calls through it: what holds there (every sample index inside [0, total), every sample of a well-formed segment
// visited once, every row inside the num_segments * bins counts, every slot inside the reserved scratch, whatever the offsets hold)
// holds on the device.
#pragma once

#include "batch_lists.hpp"
#include "histogram_bins.hpp"
#include "tile_span.hpp"

namespace glu_hip
{
// ---- the segments ---------------------------------------------------------------------------------------------------------------
// Segment `seg` of a call: [offsets[seg], offsets[seg + 1]) under the shared layer's clamp (batch_clamp_segment: a segment that ends
// below its begin or beyond `total` is empty), or [seg * count, (seg + 1) * count) of equal partitions.  offset_at(i): i <= num_segments.
template<typename OffsetAt>
GLU_HIST_FN void hist_batch_segment(bool with_offsets, OffsetAt offset_at, uint64_t count, const uint32_t& total, uint32_t seg, uint64_t& begin,
                                    uint64_t& len)
{
    if (with_offsets) batch_clamp_segment(offset_at(seg), offset_at(seg + 1u), total, begin, len);
    else
    {
        begin = (uint64_t) seg * count;
        len = count;
    }
}

// the class of a segment of `len` samples under the limits of a call: -1 = empty (in no list), else the list it is appended to
GLU_HIST_FN int hist_batch_class(uint64_t len, uint32_t wave_limit, uint32_t block_limit)
{
    return len == 0 ? -1 : len <= wave_limit ? (int) BATCH_LIST_SHORT4 : len <= block_limit ? (int) BATCH_LIST_BLOCK : (int) BATCH_LIST_LONG;
}

// What a call says about its classes to the shared layer: list 0 is the wave class, lists 1 and 2 hold nothing (their limits are
// list 0's, and a segment goes to the FIRST list whose limit it fits), list 3 is the block class; wide long and chunk lists.
inline BatchClasses hist_batch_classes(uint32_t bins, uint32_t key_bytes)
{
    const uint32_t w = hist_batch_wave_limit(bins, key_bytes);
    return {1, {w, w, w, hist_batch_block_limit(bins, key_bytes)}, hist_batch_chunk(bins, key_bytes), true};
}

// ---- the span of a range of samples -----------------------------------------------------------------------------------------------
// The samples [begin, begin + len) of the array at `samples` as the elements [lo, hi) of the 16-byte boundary at or below their
// first one (tile_span.hpp's TileSpan; lo < 16 / sizeof(T)); `tiles` counts the 16-byte PACKS that hold them.  Pack p is the
// elements [p * VEC, (p + 1) * VEC) of the base; its element v is the segment's iff lo <= v < hi, and is not read otherwise.
template<typename T>
GLU_HIST_FN TileSpan<T> hist_batch_span(const T* samples, uint64_t begin, uint64_t len)
{
    constexpr uint32_t VEC = 16 / sizeof(T);
    const T* first = samples + begin;
    TileSpan<T> s;
    s.lo = ((uintptr_t) first & 15u) / sizeof(T);
    s.hi = s.lo + len;
    s.base = first - s.lo;
    s.tiles = len ? (uint32_t) ((s.hi + VEC - 1) / VEC) : 0u; // (len <= a chunk or a limit: far below 2^32 packs)
    return s;
}

// ---- the chunks of a long segment ---------------------------------------------------------------------------------------------------
GLU_HIST_FN uint32_t hist_batch_chunks(uint64_t len, uint32_t chunk) { return (uint32_t) ((len + chunk - 1) / chunk); }

// chunk c of a segment of `len` samples: the samples [at, at + n) of the segment, n == 0 where the chunk lies behind its end (an
// entry of the chunk list that a malformed batch left stale)
GLU_HIST_FN void hist_batch_chunk_range(uint64_t len, uint32_t c, uint32_t chunk, uint64_t& at, uint32_t& n)
{
    at = (uint64_t) c * chunk;
    const uint64_t left = at < len ? len - at : 0u;
    n = left < chunk ? (uint32_t) left : chunk;
}

// Rows of partial[slot][bins] a batch of `num_segments` segments inside `total` samples can ask for: the chunk list's capacity in
// the shared layout, a chunk per whole chunk of `total` and one more per long segment, which is longer than block_limit (a chunk).
inline uint64_t hist_batch_slots(uint64_t total, uint64_t num_segments, uint32_t block_limit, uint32_t chunk)
{
    const uint64_t most_long = total / ((uint64_t) block_limit + 1u);
    const uint64_t longs = num_segments < most_long ? num_segments : most_long;
    return longs ? total / chunk + longs : 0u;
}

// ---- the rows -----------------------------------------------------------------------------------------------------------------------
// first counter of row `row` (a segment's in out_counts, a slot's in the scratch), indexed with 64 bits
GLU_HIST_FN uint64_t hist_batch_row(uint64_t row, uint32_t bins) { return row * bins; }

} // namespace glu_hip
