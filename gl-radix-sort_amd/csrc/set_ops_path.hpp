// set_ops_path.hpp -- the arithmetic of SET OPERATIONS (set_ops_kernels.hpp, glu_merge.hip) in plain C++, on top of merge_path.hpp:
// which elements of the merged order of two sorted arrays an operation keeps.  The kernels include this header, and
// tests/test_set_ops_path.py includes it with a host compiler and runs whole calls through it: what holds there (every index inside
// its array or its staged range, a tile's kept count at most its outputs, whatever the keys hold) holds on the device.
//
// The order and the equality are those of the ENCODED keys (unsigned); the accessors hand out encoded keys.  A comes first on ties.
// For A[i] with key k: rank rA = i - lower_bound(A, k), copies in B mB = upper_bound(B, k) - lower_bound(B, k); A[i] is MATCHED iff
// rA < mB, that is iff B[lower_bound(B, k) + rA] exists and holds k.  B[j] is matched iff j - lower_bound(B, k) < mA, and at B[j]'s
// place in the merged order every copy of k in A has gone by: upper_bound(A, k) = the A cursor.
//   union                 every element of A, the unmatched of B        intersection  the matched of A
//   difference            the unmatched of A                            symmetric difference  the unmatched of A and of B
#pragma once

#include "merge_path.hpp"

namespace glu_hip
{
// (the values of glu_set_op in glu_hip.h; glu_merge.hip holds them equal)
constexpr uint32_t kSetUnion = 0, kSetIntersection = 1, kSetDifference = 2, kSetSymmetricDifference = 3, kSetOpCount = 4;

// can the operation keep an element of B (then B's values are read)?
constexpr bool set_op_keeps_b(uint32_t op) { return op == kSetUnion || op == kSetSymmetricDifference; }

// the most outputs of an operation: what the host's overlap test covers and what *num_out never exceeds
GLU_MERGE_FN uint64_t set_op_bound(uint32_t op, uint64_t na, uint64_t nb)
{
    return set_op_keeps_b(op) ? na + nb : (op == kSetDifference ? na : (na < nb ? na : nb));
}

// The number of keys below `key` among `len` sorted keys, built bit by bit from the top as merge_diag_split is.  `steps`:
// merge_steps of anything >= len (uniform over the kernel or the workgroup).  at(i, any) is called with i < len where `any`, and
// must not read where !any.  Keys that are not sorted give some value in 0 .. len and never a read outside.
template<typename K, typename At>
GLU_MERGE_FN uint32_t set_lower_bound(K key, uint32_t len, uint32_t steps, At at)
{
    const bool any = len != 0u;
    uint32_t pos = 0;
    for (uint32_t step = steps ? 1u << (steps - 1) : 0u; step; step >>= 1)
    {
        const uint32_t next = pos + step;
        const uint32_t probe = next < len ? next : len; // clamped: 1 <= probe <= len where any
        const bool below = at(any ? probe - 1u : 0u, any) < key;
        pos = (next <= len && below) ? next : pos;
    }
    return pos;
}

// What the bounds kernel keeps per tile boundary: the split of the diagonal and, for the first key k0 behind it, where k0's copies
// start in A and in B.
struct SetBounds
{
    uint32_t split, start_a, start_b;
};

// The boundary at diagonal d <= na + nb.  steps_split = merge_steps(min(na, nb)), steps_a = merge_steps(na), steps_b = merge_steps(nb):
// kernel-uniform.  a_at(i, any) / b_at(j, any) as in merge_diag_split.  With d == na + nb there is no key behind: the starts are
// na and nb.  Every value lies inside: split as merge's, start_a <= na, start_b <= nb.
template<typename K, typename KeyA, typename KeyB>
GLU_MERGE_FN SetBounds set_ops_boundary(uint32_t d, uint32_t na, uint32_t nb, uint32_t steps_split, uint32_t steps_a, uint32_t steps_b,
                                        KeyA a_at, KeyB b_at)
{
    SetBounds r;
    r.split = merge_diag_split(d, na, nb, steps_split, a_at, b_at);
    const uint32_t i = r.split, j = d - r.split; // i <= na, j <= nb
    const bool has_a = i < na, has_b = j < nb;
    const K ka = a_at(has_a ? i : 0u, has_a), kb = b_at(has_b ? j : 0u, has_b);
    const bool take_a = !has_b || (has_a && ka <= kb); // (merge_serial's rule)
    const K k0 = take_a ? ka : kb;
    const bool any = has_a || has_b;
    const uint32_t la = set_lower_bound<K>(k0, na, steps_a, a_at), lb = set_lower_bound<K>(k0, nb, steps_b, b_at);
    r.start_a = any ? la : na;
    r.start_b = any ? lb : nb;
    return r;
}

// A tile as its threads see it: A[a0, a0 + na) and B[b0, b0 + nb) staged side by side (merge_tile_ranges), B's whole length, and the
// boundary's starts of the tile's first key.
struct SetTile
{
    uint32_t a0, na, b0, nb, nb_all, start_a, start_b;
};

// One thread's outputs of the merged order, as merge_serial walks them from (i, j) = (i0, diag - i0), and for each whether the
// operation keeps it: keep(s, x, key, kept) for s = 0 .. ITEMS - 1, x the staged index it came from (0 where the thread has no output
// s, and then kept is false).  Returns the number kept, at most todo.
//   key_at(x, any)  the staged key x < na + nb, read only where any
//   b_at(j, any)    key j of ALL of B (j < nb_all where any): from the staged part where it lies there, otherwise from memory
// steps_a, steps_b: merge_steps of the tile's na and nb (workgroup-uniform), for the two searches of the key that is already
// running at the thread's diagonal; the first element of every later key finds its bounds in the two cursors.  For the tile's first
// key the bounds are the boundary's.  All bounds are global indices; with keys that are not sorted they are anything, and the one
// index made from them is tested against nb_all before it is used.
template<uint32_t ITEMS, typename K, typename KeyAt, typename BAt, typename Keep>
GLU_MERGE_FN uint32_t set_ops_thread(uint32_t op, const SetTile& r, uint32_t diag, uint32_t i0, uint32_t todo, uint32_t steps_a,
                                     uint32_t steps_b, KeyAt key_at, BAt b_at, Keep keep)
{
    const uint32_t na = r.na, nb = r.nb;
    // the tile's first key (merge_serial's rule at (0, 0))
    const K fa = key_at(0u, na != 0u), fb = key_at(nb ? na : 0u, nb != 0u);
    const K k0 = (nb == 0u || (na != 0u && fa <= fb)) ? fa : fb;
    const bool a_when_matched = op == kSetUnion || op == kSetIntersection, a_when_not = op != kSetIntersection;
    const bool b_when_not = set_op_keeps_b(op);
    const bool a_needs_match = a_when_matched != a_when_not; // (union keeps A either way: no look into B)
    uint32_t lb_a = 0, lb_b = 0, kept_count = 0;
    K prev = (K) 0;
    merge_serial<ITEMS, K>(i0, diag - i0, na, nb, todo, key_at, [&](uint32_t s, uint32_t x, K key, bool live) {
        const bool from_a = x < na;
        // the cursors in front of this output: i + j = diag + s
        const uint32_t i = from_a ? x : diag + s - (x - na), j = diag + s - i;
        if (s == 0u)
        {
            const uint32_t la = set_lower_bound<K>(key, na, steps_a, [&](uint32_t p, bool any) { return key_at(p, any && live); });
            const uint32_t lb = set_lower_bound<K>(key, nb, steps_b, [&](uint32_t p, bool any) { return key_at(any ? na + p : 0u, any && live); });
            const bool first = key == k0;
            lb_a = first ? r.start_a : r.a0 + la;
            lb_b = first ? r.start_b : r.b0 + lb;
        }
        else if (key != prev)
        {
            lb_a = r.a0 + i;
            lb_b = r.b0 + j;
        }
        prev = key;
        bool kept;
        if (from_a)
        {
            const uint32_t partner = lb_b + (r.a0 + i - lb_a); // where A[i]'s match lies in B, if it has one
            const bool look = live && a_needs_match && partner < r.nb_all;
            const bool matched = look && b_at(look ? partner : 0u, look) == key;
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

// *num_out of a call: the kept elements of all tiles, and never more than the operation's bound (keys that are not sorted)
GLU_MERGE_FN uint32_t set_ops_total(uint64_t kept, uint64_t bound) { return (uint32_t) (kept < bound ? kept : bound); }

} // namespace glu_hip
