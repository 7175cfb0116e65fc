// merge_batch_path.hpp -- the arithmetic of the BATCHED MERGE (merge_batch_kernels.hpp, glu_merge.hip) in plain C++: the two sides
// of a call with their clamps, the segment of a diagonal, the boundary of a tile (global split and segment), the tile's ranges and
// its path from two stored boundaries, the segment of a staged element and the composite (segment, key).  Both kernels include this
// header, and tests/test_merge_batch_path.py includes it with a host compiler and walks whole calls through it: what holds there
// (every index inside its array, every output written once, every out_offsets entry at most a_total + b_total, whatever the offsets
// and the keys hold) holds on the device.
//
// A batched merge is ONE merge path over all of A and all of B in the composite order (segment, enc(key)): both arrays are sorted
// in that order already.  With oa[s], ob[s] the offsets relative to the side's first, segment s owns the outputs
// [oa[s] + ob[s], oa[s + 1] + ob[s + 1]).  The offsets live on the device and cannot be checked: every function here takes them
// through merge_batch_rel, which pins an offset into its side, so that whatever they hold the arithmetic stays inside
// [0, a_total), [0, b_total) and out[0, a_total + b_total).
#pragma once

#include "batch_lists.hpp"
#include "merge_path.hpp"

namespace glu_hip
{
// One side of a call: the elements [begin, begin + len) of its array, from the side's first and last offset by the family's clamp
// (batch_clamp_segment: b <= e <= total, else empty at b).  len <= total; nothing is read where len == 0.
struct MergeBatchSide
{
    uint32_t begin, len;
};
template<typename Off>
GLU_MERGE_FN MergeBatchSide merge_batch_side(Off off, uint32_t num_segments, uint32_t total)
{
    MergeBatchSide side;
    batch_clamp_segment(off(0u), off(num_segments), total, side.begin, side.len);
    return side;
}

// an offset relative to its side's begin, pinned into [0, len]  (sorted offsets inside the total: off - begin)
GLU_MERGE_FN uint32_t merge_batch_rel(uint32_t off, const MergeBatchSide& side)
{
    const uint32_t r = off > side.begin ? off - side.begin : 0u;
    return r < side.len ? r : side.len;
}

// How many of the `len` entries at(1) .. at(len) are <= x (an upper bound, built bit by bit from the top as merge_diag_split
// builds its split): `steps` = merge_steps of anything >= len, uniform.  Every probe is one of 1 .. len (at(0) is asked where len
// is 0 and its answer dropped); entries that are not sorted give some count in [0, len].
template<typename At>
GLU_MERGE_FN uint32_t merge_batch_count_le(uint32_t x, uint32_t len, uint32_t steps, At at)
{
    const bool any = len != 0u;
    uint32_t pos = 0;
    for (uint32_t step = steps ? 1u << (steps - 1) : 0u; step; step >>= 1)
    {
        const uint32_t next = pos + step;
        const uint32_t probe = any ? (next < len ? next : len) : 0u;
        const bool passes = at(probe) <= x;
        pos = (next <= len && passes) ? next : pos;
    }
    return pos;
}

// The segment of diagonal d: the last of 0 .. num_segments - 1 (>= 1 segments) whose first output is at or in front of d,
// out_off(s) = oa[s] + ob[s]: empty segments at d are passed over, and d = the total lands in the last segment.
// `steps`: merge_steps(num_segments - 1).
template<typename OutOff>
GLU_MERGE_FN uint32_t merge_batch_diag_segment(uint32_t d, uint32_t num_segments, uint32_t steps, OutOff out_off)
{
    return merge_batch_count_le(d, num_segments - 1u, steps, out_off);
}

// What the partition kernel stores per tile boundary: the elements of the side A in front of the diagonal, and its segment.
struct MergeBatchBoundary
{
    uint32_t split, seg;
};

// The boundary of diagonal d <= a.len + b.len: its segment by merge_batch_diag_segment (log S probes of two offsets), then
// merge_diag_split inside that one segment with the local diagonal (log n probes of two keys).  off_a(s), off_b(s): the offset
// words, s <= num_segments; a_at(i, any), b_at(j, any): encoded keys by ABSOLUTE index, read only where any.  `split_steps`:
// merge_steps of anything >= the shorter side of every segment (the host: merge_steps(min(a_total, b_total))).
// Whatever offsets and keys hold: seg < num_segments, max(0, d - b.len) <= split <= min(d, a.len) (the last clamp), and every
// key index lies inside its side.
template<typename OffA, typename OffB, typename KeyA, typename KeyB>
GLU_MERGE_FN MergeBatchBoundary merge_batch_boundary(uint32_t d, uint32_t num_segments, const MergeBatchSide& a, const MergeBatchSide& b,
                                                     uint32_t seg_steps, uint32_t split_steps, OffA off_a, OffB off_b, KeyA a_at, KeyB b_at)
{
    MergeBatchBoundary r;
    r.seg = merge_batch_diag_segment(d, num_segments, seg_steps,
                                     [&](uint32_t s) { return merge_batch_rel(off_a(s), a) + merge_batch_rel(off_b(s), b); });
    uint32_t a0, na, b0, nb; // the segment's runs, relative to the sides
    batch_clamp_segment(merge_batch_rel(off_a(r.seg), a), merge_batch_rel(off_a(r.seg + 1u), a), a.len, a0, na);
    batch_clamp_segment(merge_batch_rel(off_b(r.seg), b), merge_batch_rel(off_b(r.seg + 1u), b), b.len, b0, nb);
    const uint32_t first = a0 + b0;
    uint32_t local = d > first ? d - first : 0u;
    local = local < na + nb ? local : na + nb;
    const uint32_t i = merge_diag_split(
        local, na, nb, split_steps, [&](uint32_t x, bool any) { return a_at(a.begin + a0 + x, any); },
        [&](uint32_t x, bool any) { return b_at(b.begin + b0 + x, any); });
    const uint32_t lo = d > b.len ? d - b.len : 0u, hi = d < a.len ? d : a.len; // (lo <= hi because d <= a.len + b.len)
    const uint32_t split = a0 + i;
    r.split = split < lo ? lo : (split > hi ? hi : split);
    return r;
}

// A tile from the boundaries of its two diagonals d0 < d1: its ranges relative to the sides (merge_tile_ranges' clamp: inside the
// sides whatever the splits hold, na + nb = d1 - d0), the segments it spans, and whether it lies inside one segment: the stored
// segments agree, or the first one reaches the tile's end (out_next(s) = oa[s + 1] + ob[s + 1], asked only where they differ).
struct MergeBatchTile
{
    MergeRanges r;
    uint32_t seg0, span; // its elements lie in the segments seg0 .. seg0 + span
    bool one;
};
template<typename OutNext>
GLU_MERGE_FN MergeBatchTile merge_batch_tile(const MergeBatchBoundary& b0, const MergeBatchBoundary& b1, uint32_t d0, uint32_t d1,
                                             uint32_t num_segments, OutNext out_next)
{
    MergeBatchTile t;
    t.r = merge_tile_ranges(b0.split, b1.split, d0, d1);
    t.seg0 = b0.seg < num_segments ? b0.seg : num_segments - 1u;
    const uint32_t last = b1.seg < num_segments ? b1.seg : num_segments - 1u;
    t.span = last > t.seg0 ? last - t.seg0 : 0u;
    t.one = t.span == 0u || out_next(t.seg0) >= d1;
    return t;
}

// The segment, relative to seg0, of the staged element `at` of a side (relative to the side's begin): the last of seg0 .. seg0 + span
// that begins at or in front of it, rel(s) = the side's relative offset s.  One bound over the tile's offsets per element -- never
// a loop over the tile's segments: 2^24 empty segments at one position are 24 probes.  `steps`: merge_steps(span).
template<typename Rel>
GLU_MERGE_FN uint32_t merge_batch_element_segment(uint32_t at, uint32_t seg0, uint32_t span, uint32_t steps, Rel rel)
{
    return merge_batch_count_le(at, span, steps, [&](uint32_t s) { return rel(seg0 + s); });
}

// The composite (segment, key) that merge_diag_split and merge_serial order a tile of several segments by: they are templates over
// what the accessors return and ask for `<=` and a zero alone.  One unsigned word of twice the key's width, the segment on top (a
// struct of two members is ordered as well, but the selects of the serial merge send it through memory: 56 bytes of scratch a lane).
template<typename K>
struct MergeBatchComposite;
template<>
struct MergeBatchComposite<uint32_t>
{
    typedef uint64_t type;
    static GLU_MERGE_FN type make(uint32_t seg, uint32_t key) { return (uint64_t) seg << 32 | key; }
    static GLU_MERGE_FN uint32_t key(const type& c) { return (uint32_t) c; }
};
template<>
struct MergeBatchComposite<uint64_t>
{
    typedef unsigned __int128 type;
    static GLU_MERGE_FN type make(uint32_t seg, uint64_t key) { return (type) seg << 64 | key; }
    static GLU_MERGE_FN uint64_t key(const type& c) { return (uint64_t) c; }
};

} // namespace glu_hip
