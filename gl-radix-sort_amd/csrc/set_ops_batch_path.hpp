// set_ops_batch_path.hpp -- the arithmetic of the BATCHED SET OPERATIONS (set_ops_batch_kernels.hpp, glu_merge.hip) in plain C++, on
// top of merge_batch_path.hpp (the order (segment, enc(key)), the boundary's segment and split, the tile's ranges and path) and
// set_ops_path.hpp (the rank rule): the boundary of a tile with the starts of its first key inside the boundary's segment, the tile
// as the walk sees it, the walk of a tile over several segments, the word a thread leaves per tile (its kept outputs as bits, and
// how many outputs the tile keeps in front of it) and the out_offsets entry of a segment from those words.  The kernels include
// this header, and tests/test_set_ops_batch_path.py includes it with a host compiler and walks whole calls through it: what holds
// there (every index inside its array, a tile's kept count at most its outputs, every entry at most its limit, whatever offsets and
// keys hold) holds on the device.
//
// A batched set operation is the single call's rule under the composite key (segment, enc(key)): both inputs are sorted by it
// already.  A[i] of segment s with key k is matched iff its rank among the copies of (s, k) in A is below the number of copies of
// (s, k) in B: iff its partner B[lower_bound(B, (s, k)) + rank] lies in front of the END OF SEGMENT s's RUN OF B and holds k.  The
// lower bound is never in front of the run's begin, so the test against the end is the whole test of the segment: the partner's own
// segment is never searched.  All indices are relative to the sides (merge_batch_side).
#pragma once

#include "merge_batch_path.hpp"
#include "set_ops_path.hpp"

namespace glu_hip
{
// What the bounds kernel keeps per tile boundary: the batched merge's boundary, and for the first key k0 behind it where k0's copies
// start in A and in B, searched inside the boundary's segment alone.  Four words.
struct SetBatchBounds
{
    uint32_t split, seg, start_a, start_b;
};

// The boundary of diagonal d <= a.len + b.len: merge_batch_boundary's steps (the segment, its runs, the local diagonal, the last
// clamp of the split into the sides) around set_ops_boundary inside that one segment.  steps_a, steps_b: merge_steps of anything >=
// the longest run of a side (the host: merge_steps(a_total), merge_steps(b_total)).  Whatever offsets and keys hold: seg <
// num_segments, the split in merge_batch_boundary's range, start_a <= a.len, start_b <= b.len, every key index inside its side.
template<typename K, typename OffA, typename OffB, typename KeyA, typename KeyB>
GLU_MERGE_FN SetBatchBounds set_ops_batch_boundary(uint32_t d, uint32_t num_segments, const MergeBatchSide& a, const MergeBatchSide& b,
                                                   uint32_t seg_steps, uint32_t split_steps, uint32_t steps_a, uint32_t steps_b, OffA off_a,
                                                   OffB off_b, KeyA a_at, KeyB b_at)
{
    SetBatchBounds r;
    r.seg = merge_batch_diag_segment(d, num_segments, seg_steps,
                                     [&](uint32_t s) { return merge_batch_rel(off_a(s), a) + merge_batch_rel(off_b(s), b); });
    uint32_t a0, na, b0, nb; // the segment's runs, relative to the sides
    batch_clamp_segment(merge_batch_rel(off_a(r.seg), a), merge_batch_rel(off_a(r.seg + 1u), a), a.len, a0, na);
    batch_clamp_segment(merge_batch_rel(off_b(r.seg), b), merge_batch_rel(off_b(r.seg + 1u), b), b.len, b0, nb);
    const uint32_t first = a0 + b0;
    uint32_t local = d > first ? d - first : 0u;
    local = local < na + nb ? local : na + nb;
    const SetBounds in = set_ops_boundary<K>(
        local, na, nb, split_steps, steps_a, steps_b, [&](uint32_t x, bool any) { return a_at(a.begin + a0 + x, any); },
        [&](uint32_t x, bool any) { return b_at(b.begin + b0 + x, any); });
    const uint32_t lo = d > b.len ? d - b.len : 0u, hi = d < a.len ? d : a.len; // (lo <= hi because d <= a.len + b.len)
    const uint32_t split = a0 + in.split;
    r.split = split < lo ? lo : (split > hi ? hi : split);
    r.start_a = a0 + in.start_a; // <= a0 + na <= a.len
    r.start_b = b0 + in.start_b;
    return r;
}

// A tile from its two stored boundaries: the batched merge's tile (ranges inside the sides, the segments it spans, whether it lies
// inside one), and the SetTile of the walk.  nb_all is the end of the FIRST segment's run of B (end_b(s) = the side's relative
// offset s + 1): what the partner of a tile inside one segment is tested against.  A tile over several segments asks end_b per
// segment (set_ops_batch_thread).
struct SetBatchTile
{
    SetTile t;
    uint32_t seg0, span;
    bool one;
};
template<typename OutNext, typename EndB>
GLU_MERGE_FN SetBatchTile set_ops_batch_tile(const SetBatchBounds& b0, const SetBatchBounds& b1, uint32_t d0, uint32_t d1,
                                             uint32_t num_segments, OutNext out_next, EndB end_b)
{
    const MergeBatchBoundary m0 = {b0.split, b0.seg}, m1 = {b1.split, b1.seg};
    const MergeBatchTile m = merge_batch_tile(m0, m1, d0, d1, num_segments, out_next);
    SetBatchTile r;
    r.t.a0 = m.r.a0, r.t.na = m.r.a1 - m.r.a0, r.t.b0 = m.r.b0, r.t.nb = m.r.b1 - m.r.b0; // na + nb == d1 - d0
    r.t.nb_all = end_b(m.seg0);
    r.t.start_a = b0.start_a, r.t.start_b = b0.start_b;
    r.seg0 = m.seg0, r.span = m.span, r.one = m.one;
    return r;
}

// the segment word of a composite (MergeBatchComposite<K>::make put it on top)
template<typename K>
GLU_MERGE_FN uint32_t set_batch_composite_seg(const typename MergeBatchComposite<K>::type& c)
{
    return (uint32_t) (c >> (8 * sizeof(K)));
}

// set_ops_thread for a tile over several segments.  The staged keys are composites (segment relative to the tile's first, key):
// key_at(x, any) hands them out, and splits, order, lower bounds and equality are the composite's, so copies are counted inside
// their segment alone.  What differs from set_ops_thread is the partner's test:
//   end_b(seg)    the end of the run of B of the tile's segment `seg` (relative to the side, <= b.len whatever the offsets hold);
//                 asked once per segment a thread meets
//   b_at(j, any)  the PLAIN encoded key j of the side B (j < end_b where any): from the staged part where it lies there, otherwise
//                 from memory
// keep(s, x, composite, kept) as set_ops_thread's.  Returns the number kept, at most todo.
template<uint32_t ITEMS, typename K, typename KeyAt, typename BAt, typename EndB, typename Keep>
GLU_MERGE_FN uint32_t set_ops_batch_thread(uint32_t op, const SetTile& r, uint32_t diag, uint32_t i0, uint32_t todo, uint32_t steps_a,
                                           uint32_t steps_b, KeyAt key_at, BAt b_at, EndB end_b, Keep keep)
{
    typedef typename MergeBatchComposite<K>::type C;
    const uint32_t na = r.na, nb = r.nb;
    // the tile's first key (merge_serial's rule at (0, 0))
    const C fa = key_at(0u, na != 0u), fb = key_at(nb ? na : 0u, nb != 0u);
    const C k0 = (nb == 0u || (na != 0u && fa <= fb)) ? fa : fb;
    const bool a_when_matched = op == kSetUnion || op == kSetIntersection, a_when_not = op != kSetIntersection;
    const bool b_when_not = set_op_keeps_b(op);
    const bool a_needs_match = a_when_matched != a_when_not; // (union keeps A either way: no look into B)
    uint32_t lb_a = 0, lb_b = 0, run_end = 0, kept_count = 0;
    C prev = (C) 0;
    merge_serial<ITEMS, C>(i0, diag - i0, na, nb, todo, key_at, [&](uint32_t s, uint32_t x, C key, bool live) {
        const bool from_a = x < na;
        // the cursors in front of this output: i + j = diag + s
        const uint32_t i = from_a ? x : diag + s - (x - na), j = diag + s - i;
        const uint32_t seg = set_batch_composite_seg<K>(key);
        if (s == 0u)
        {
            const uint32_t la = set_lower_bound<C>(key, na, steps_a, [&](uint32_t p, bool any) { return key_at(p, any && live); });
            const uint32_t lb = set_lower_bound<C>(key, nb, steps_b, [&](uint32_t p, bool any) { return key_at(any ? na + p : 0u, any && live); });
            const bool first = key == k0;
            lb_a = first ? r.start_a : r.a0 + la;
            lb_b = first ? r.start_b : r.b0 + lb;
            run_end = (live && a_needs_match) ? end_b(seg) : 0u;
        }
        else if (key != prev)
        {
            lb_a = r.a0 + i;
            lb_b = r.b0 + j;
            if (live && a_needs_match && seg != set_batch_composite_seg<K>(prev)) run_end = end_b(seg);
        }
        prev = key;
        bool kept;
        if (from_a)
        {
            const uint32_t partner = lb_b + (r.a0 + i - lb_a); // where A[i]'s match lies in B, if it has one
            const bool look = live && a_needs_match && partner < run_end; // the end of THIS segment's run: never B's whole length
            const bool matched = look && b_at(look ? partner : 0u, look) == MergeBatchComposite<K>::key(key);
            kept = matched ? a_when_matched : a_when_not;
        }
        else
        {
            const bool matched = r.b0 + j - lb_b < r.a0 + i - lb_a; // rank in B < copies in A (upper_bound(A, key) = a0 + i)
            kept = !matched && b_when_not;
        }
        kept = kept && live;
        kept_count += kept ? 1u : 0u;
        keep(s, live ? x : 0u, key, kept);
    });
    return kept_count;
}

// What a thread of the count kernel leaves for the offsets and the write kernel, one word per thread and tile: the tile's kept
// outputs in front of the thread's first (at most the tile: 12 bits) above the thread's kept outputs as bits (ITEMS <= 11 of them).
constexpr uint32_t kSetBatchWordShift = 16;
GLU_MERGE_FN uint32_t set_batch_word(uint32_t kept_in_front, uint32_t mask) { return kept_in_front << kSetBatchWordShift | mask; }
GLU_MERGE_FN uint32_t set_batch_word_rank(uint32_t word) { return word >> kSetBatchWordShift; }
GLU_MERGE_FN uint32_t set_batch_word_mask(uint32_t word) { return word & ((1u << kSetBatchWordShift) - 1u); }
GLU_MERGE_FN uint32_t set_batch_word_kept(uint32_t word) { return (uint32_t) __builtin_popcount(set_batch_word_mask(word)); }

// The kept outputs in front of the merged position d: those of the tiles in front (scanned(t), the scanned tile counts), of the
// threads in front inside the tile and of the thread's own outputs in front: one word read (word(t * kMergeThreads + q)), never a
// loop.  d >= total (the device's total): everything kept, `all` (*num_out).
template<typename Scanned, typename Word>
GLU_MERGE_FN uint32_t set_ops_batch_kept_before(uint32_t d, uint32_t total, uint32_t tile, uint32_t items, uint32_t all, Scanned scanned,
                                                Word word)
{
    const bool inside = d < total;
    const uint32_t t = inside ? d / tile : 0u, r = inside ? d % tile : 0u;
    const uint32_t w = inside ? word((uint64_t) t * kMergeThreads + r / items) : 0u;
    const uint32_t in_front = set_batch_word_rank(w) + (uint32_t) __builtin_popcount(set_batch_word_mask(w) & ((1u << (r % items)) - 1u));
    return inside ? scanned(t) + in_front : all;
}

// An out_offsets entry: the kept outputs in front of the segment's first merged position, held to `limit`: min(max_out, bound) where
// arrays are written (the entries describe what was written), the bound alone in a call that only counts.
GLU_MERGE_FN uint32_t set_ops_batch_entry(uint32_t kept_before, uint32_t limit) { return kept_before < limit ? kept_before : limit; }

} // namespace glu_hip
