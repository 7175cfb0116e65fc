// set_ops_batch_kernels.hpp -- gfx950 kernels of the BATCHED SET OPERATIONS (glu_set_ops_run_batch_offsets_ptr,
// glu_set_ops_run_batch_ptr): union, intersection, difference and symmetric difference of the two sorted runs of every segment, all
// segments in one call, over device offsets.  Not in the reference.
//
// The single call's rule (set_ops_kernels.hpp) under the composite key (segment, enc(key)), on the batched merge's tiles
// (merge_batch_kernels.hpp); the arithmetic is set_ops_batch_path.hpp (plain C++, walked on the host by
// tests/test_set_ops_batch_path.py).
//   bounds   set_batch_bounds_kernel: one thread per tile boundary d = t * TILE (clamped to the device total): the batched merge's
//            boundary (segment, split) and, for the first key behind it, where its copies start in A and in B, searched inside that
//            segment's runs alone.  Four words per boundary.
//   count    set_batch_count_kernel: one workgroup of 256 per tile.  A tile inside one segment runs the single call's walk with
//            that segment's ranges (the partner is tested against the end of the segment's run of B).  A tile over several segments
//            gives every staged element its segment word and walks the composite; the partner is tested against the end of the run of
//            B of ITS segment.  The workgroup's kept count goes to tile_counts[t]; every thread leaves one word: its kept outputs as
//            bits and the tile's kept outputs in front of it (skipped where nobody reads them: a count without out_offsets).
//   scan     key_runs_scan_kernel (tile_count_scan_kernel.hpp), unchanged: the counts scanned, *num_out their sum held to the bound.
//   offsets  set_batch_offsets_kernel: one thread per segment boundary: the scanned count of the boundary's tile + the kept
//            outputs in front of the boundary inside the tile, from ONE word of the count kernel.  Never a loop over segments.
//   write    set_batch_write_kernel: the batched merge's tile walk for the ORDER (no second decision: the threads' bits and
//            ranks are the count kernel's words), kept keys and values to LDS in output order, out through merge_store_tile; what
//            lies at or behind `room` is dropped.
// LDS: the segment words lie where the values are staged, as in the batched merge: every instantiation stays inside the merge tile
// kernel's footprint.  No atomics, nothing waits for another workgroup, the grids follow from the host-known totals alone.
// Offsets that decrease or leave their total and inputs that are not sorted give unspecified contents; every index still lies
// inside its array, a tile keeps at most its outputs and nothing is written at or behind out[room].
#pragma once

#include "merge_batch_kernels.hpp"
#include "set_ops_batch_path.hpp"
#include "set_ops_kernels.hpp"

namespace glu_hip
{
template<typename K>
struct SetOpsBatchArgs
{
    const K* a_keys;
    const K* b_keys;
    const uint32_t* a_vals;
    const uint32_t* b_vals; // NULL where the operation keeps nothing of B
    K* out_keys;
    uint32_t* out_vals;
    const uint32_t* a_offsets; // num_segments + 1 words, or NULL: a_offsets[s] = s * a_len
    const uint32_t* b_offsets;
    uint32_t a_len, b_len;
    uint32_t a_total, b_total; // the arrays' lengths: every access lies below them
    uint32_t num_segments;     // >= 1
    uint32_t xf;               // KeyTransform of the key type
    uint32_t op;               // kSetUnion ..
    uint32_t tiles;            // ceil((a_total + b_total) / TILE)
    uint32_t seg_steps;        // merge_steps(num_segments - 1)
    uint32_t split_steps;      // merge_steps(min(a_total, b_total))
    uint32_t room;             // outputs that may be written: min(max_out, the operation's bound); 0: the call only counts
    uint32_t limit;            // what an out_offsets entry is held to: room, or the bound in a call that only counts
    SetBatchBounds* bounds;    // tiles + 1
    uint32_t* tile_counts;     // tiles: kept per tile, then their exclusive scan
    uint32_t* words;           // tiles * 256 (set_batch_word), or NULL: nobody reads them
    uint32_t* out_offsets;     // num_segments + 1 words, or NULL
    const uint32_t* num_out;   // what the scan wrote: everything kept

    __device__ __forceinline__ uint32_t off_a(uint32_t s) const { return a_offsets ? a_offsets[s] : s * a_len; }
    __device__ __forceinline__ uint32_t off_b(uint32_t s) const { return b_offsets ? b_offsets[s] : s * b_len; }
};

template<typename K>
__global__ __launch_bounds__(kMergeThreads) void set_batch_bounds_kernel(SetOpsBatchArgs<K> m, uint32_t tile)
{
    const KeyCodec<K, true> codec(m.xf);
    const uint32_t g = blockIdx.x * kMergeThreads + threadIdx.x;
    if (g > m.tiles) return;
    const auto off_a = [&](uint32_t s) { return m.off_a(s); };
    const auto off_b = [&](uint32_t s) { return m.off_b(s); };
    const MergeBatchSide a = merge_batch_side(off_a, m.num_segments, m.a_total), b = merge_batch_side(off_b, m.num_segments, m.b_total);
    const uint32_t total = a.len + b.len; // (the host: a_total + b_total < 2^32)
    const uint64_t d64 = (uint64_t) g * tile;
    const uint32_t d = d64 < total ? (uint32_t) d64 : total;
    m.bounds[g] = set_ops_batch_boundary<K>(
        d, m.num_segments, a, b, m.seg_steps, m.split_steps, merge_steps(m.a_total), merge_steps(m.b_total), off_a, off_b,
        [&](uint32_t i, bool any) { return any ? codec.encode(m.a_keys[i]) : (K) 0; },
        [&](uint32_t j, bool any) { return any ? codec.encode(m.b_keys[j]) : (K) 0; });
}

// The tile of workgroup t (d0 < the device total) as the count and the write kernel see it.
template<typename K>
__device__ __forceinline__ SetBatchTile set_ops_batch_tile_of(const SetOpsBatchArgs<K>& m, const MergeBatchSide& a, const MergeBatchSide& b,
                                                              uint32_t t, uint32_t d0, uint32_t count)
{
    return set_ops_batch_tile(
        m.bounds[t], m.bounds[t + 1], d0, d0 + count, m.num_segments,
        [&](uint32_t s) { return merge_batch_rel(m.off_a(s + 1u), a) + merge_batch_rel(m.off_b(s + 1u), b); },
        [&](uint32_t s) { return merge_batch_rel(m.off_b(s + 1u), b); });
}

// Stage x of the tile: its key (encoded) to lk, and in a tile over several segments its segment word (relative to seg0) to lseg.
// Returns the element's index in its array.
template<typename K>
__device__ __forceinline__ size_t set_ops_batch_stage(const SetOpsBatchArgs<K>& m, const KeyCodec<K, true>& codec, const MergeBatchSide& a,
                                                      const MergeBatchSide& b, const SetBatchTile& tile, uint32_t seg_steps, uint32_t x, K* lk,
                                                      uint32_t* lseg)
{
    const SetTile& r = tile.t;
    const bool from_a = x < r.na;
    const uint32_t rel = from_a ? r.a0 + x : r.b0 + (x - r.na); // (inside the side)
    const size_t at = (size_t) (from_a ? a.begin : b.begin) + rel;
    lk[x] = codec.encode(from_a ? m.a_keys[at] : m.b_keys[at]);
    if (!tile.one)
        lseg[x] = from_a ? merge_batch_element_segment(rel, tile.seg0, tile.span, seg_steps, [&](uint32_t s) { return merge_batch_rel(m.off_a(s), a); })
                         : merge_batch_element_segment(rel, tile.seg0, tile.span, seg_steps, [&](uint32_t s) { return merge_batch_rel(m.off_b(s), b); });
    return at;
}

template<typename K>
__global__ __launch_bounds__(kMergeThreads) void set_batch_count_kernel(SetOpsBatchArgs<K> m)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), true), TILE = merge_tile(sizeof(K), true);
    constexpr uint32_t KVEC = 16 / sizeof(K), WAVES = kMergeThreads / kWave;
    typedef MergeBatchComposite<K> Composite;
    typedef typename Composite::type C;
    static_assert(ITEMS < kSetBatchWordShift && TILE < (1u << (32 - kSetBatchWordShift)), "a thread's bits and its rank share a word");
    __shared__ Pack<K, KVEC> key_packs[TILE / KVEC];
    __shared__ uint32_t lseg[TILE];
    __shared__ uint32_t wave_kept[WAVES];
    K* lk = &key_packs[0].v[0];

    const KeyCodec<K, true> codec(m.xf);
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const auto off_a = [&](uint32_t s) { return m.off_a(s); };
    const auto off_b = [&](uint32_t s) { return m.off_b(s); };
    const MergeBatchSide a = merge_batch_side(off_a, m.num_segments, m.a_total), b = merge_batch_side(off_b, m.num_segments, m.b_total);
    const uint32_t total = a.len + b.len;
    const uint32_t d0 = t * TILE; // (t < tiles: d0 < a_total + b_total)
    if (d0 >= total)              // (workgroup-uniform) behind the device total: the scan still reads this tile's count
    {
        if (tid == 0) m.tile_counts[t] = 0u;
        return;
    }
    const uint32_t count = total - d0 < TILE ? total - d0 : TILE;
    const SetBatchTile tile = set_ops_batch_tile_of(m, a, b, t, d0, count);
    const SetTile r = tile.t;
    const uint32_t seg_steps = merge_steps(tile.span);
#pragma unroll
    for (uint32_t g = 0; g < ITEMS; g++)
    {
        const uint32_t x = g * kMergeThreads + tid;
        if (x < count) set_ops_batch_stage(m, codec, a, b, tile, seg_steps, x, lk, lseg);
    }
    __syncthreads();

    const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
    const uint32_t todo = count - diag < ITEMS ? count - diag : ITEMS;
    const uint32_t steps = merge_steps(r.na < r.nb ? r.na : r.nb); // (workgroup-uniform)
    // key j of the side B, j in front of the end of a run: staged (b0 <= j < b0 + nb) or from memory
    const auto b_at = [&](uint32_t j, bool any) {
        const uint32_t local = j - r.b0;
        if (!any) return (K) 0;
        return local < r.nb ? lk[r.na + local] : codec.encode(m.b_keys[(size_t) b.begin + j]);
    };
    uint32_t mask = 0, kept;
    if (tile.one) // (workgroup-uniform) the single call's walk inside the segment
    {
        const uint32_t i0 = merge_diag_split(
            diag, r.na, r.nb, steps, [&](uint32_t i, bool any) { return any ? lk[i] : (K) 0; },
            [&](uint32_t j, bool any) { return any ? lk[r.na + j] : (K) 0; });
        kept = set_ops_thread<ITEMS, K>(
            m.op, r, diag, i0, todo, merge_steps(r.na), merge_steps(r.nb), [&](uint32_t x, bool any) { return any ? lk[x] : (K) 0; }, b_at,
            [&](uint32_t s, uint32_t, K, bool keep) { mask |= keep ? 1u << s : 0u; });
    }
    else
    {
        const auto both = [&](uint32_t x, bool any) { return any ? Composite::make(lseg[x], lk[x]) : (C) 0; };
        const uint32_t i0 = merge_diag_split(
            diag, r.na, r.nb, steps, [&](uint32_t i, bool any) { return both(i, any); }, [&](uint32_t j, bool any) { return both(any ? r.na + j : 0u, any); });
        kept = set_ops_batch_thread<ITEMS, K>(
            m.op, r, diag, i0, todo, merge_steps(r.na), merge_steps(r.nb), both, b_at,
            [&](uint32_t seg) { return merge_batch_rel(m.off_b(tile.seg0 + seg + 1u), b); },
            [&](uint32_t s, uint32_t, C, bool keep) { mask |= keep ? 1u << s : 0u; });
    }
    uint32_t wave_total;
    uint32_t rank = wave_exclusive_sum(kept, tid % kWave, wave_total);
    if (tid % kWave == 0) wave_kept[tid / kWave] = wave_total;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++)
    {
        rank += w < tid / kWave ? wave_kept[w] : 0u;
        sum += wave_kept[w];
    }
    if (m.words) m.words[(size_t) t * kMergeThreads + tid] = set_batch_word(rank, mask);
    if (tid == 0) m.tile_counts[t] = sum < count ? sum : count; // (at most the tile's outputs by construction; held to it all the same)
}

// One thread per out_offsets entry, after the scan.
template<typename K>
__global__ __launch_bounds__(kMergeThreads) void set_batch_offsets_kernel(SetOpsBatchArgs<K> m, uint32_t tile, uint32_t items)
{
    const uint32_t g = blockIdx.x * kMergeThreads + threadIdx.x;
    if (g > m.num_segments) return;
    const auto off_a = [&](uint32_t s) { return m.off_a(s); };
    const auto off_b = [&](uint32_t s) { return m.off_b(s); };
    const MergeBatchSide a = merge_batch_side(off_a, m.num_segments, m.a_total), b = merge_batch_side(off_b, m.num_segments, m.b_total);
    const uint32_t d = merge_batch_rel(off_a(g), a) + merge_batch_rel(off_b(g), b); // the segment's first merged position
    const uint32_t kept = set_ops_batch_kept_before(
        d, a.len + b.len, tile, items, *m.num_out, [&](uint32_t t) { return m.tile_counts[t]; }, [&](uint64_t w) { return m.words[w]; });
    m.out_offsets[g] = set_ops_batch_entry(kept, m.limit);
}

// (seven waves a SIMD, what the LDS allows: the batched merge's tile kernel, whose walk this is)
template<typename K, bool WITH_VALS>
__global__ __launch_bounds__(kMergeThreads, 7) void set_batch_write_kernel(SetOpsBatchArgs<K> m)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), WITH_VALS), TILE = merge_tile(sizeof(K), WITH_VALS);
    constexpr uint32_t KVEC = 16 / sizeof(K), VVEC = 4;
    typedef MergeBatchComposite<K> Composite;
    static_assert((TILE + KVEC) * sizeof(K) + (TILE + VVEC) * 4 <= 32768, "five workgroups to the CU");
    // one pack more than the tile: the outputs lie up to a pack's length behind the start
    __shared__ Pack<K, KVEC> key_packs[TILE / KVEC + 1];
    __shared__ Pack<uint32_t, VVEC> val_packs[TILE / VVEC + 1]; // the values; in a tile of several segments the segment words first
    K* lk = &key_packs[0].v[0];
    uint32_t* lv = &val_packs[0].v[0];

    const KeyCodec<K, true> codec(m.xf);
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const uint32_t first = m.tile_counts[t]; // the tile's first output
    if (first >= m.room) return;             // (workgroup-uniform) nothing of this tile may be written
    const auto off_a = [&](uint32_t s) { return m.off_a(s); };
    const auto off_b = [&](uint32_t s) { return m.off_b(s); };
    const MergeBatchSide a = merge_batch_side(off_a, m.num_segments, m.a_total), b = merge_batch_side(off_b, m.num_segments, m.b_total);
    const uint32_t total = a.len + b.len;
    const uint32_t d0 = t * TILE; // (t < tiles: d0 < a_total + b_total)
    if (d0 >= total) return;      // (workgroup-uniform)
    const uint32_t count = total - d0 < TILE ? total - d0 : TILE;
    const SetBatchTile tile = set_ops_batch_tile_of(m, a, b, t, d0, count);
    const uint32_t na = tile.t.na, nb = tile.t.nb;
    const bool several = !tile.one; // (workgroup-uniform)
    const uint32_t seg_steps = merge_steps(tile.span);
    const bool b_too = m.b_vals != nullptr; // (kernel-uniform)

    uint32_t held[ITEMS]; // several segments: the values wait here for the segment words' place
#pragma unroll
    for (uint32_t g = 0; g < ITEMS; g++)
    {
        const uint32_t x = g * kMergeThreads + tid;
        held[g] = 0u;
        if (x < count)
        {
            const size_t at = set_ops_batch_stage(m, codec, a, b, tile, seg_steps, x, lk, lv);
            uint32_t v = 0u;
            if (WITH_VALS) v = x < na ? m.a_vals[at] : (b_too ? m.b_vals[at] : 0u);
            if (several)
                held[g] = v;
            else if (WITH_VALS)
                lv[x] = v;
        }
    }
    __syncthreads();

    const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
    const uint32_t todo = count - diag < ITEMS ? count - diag : ITEMS;
    K key[ITEMS];
    uint32_t from[ITEMS];
    if (several)
    {
        typename Composite::type both[ITEMS];
        merge_batch_thread<ITEMS>(diag, todo, na, nb, [&](uint32_t x) { return Composite::make(lv[x], lk[x]); }, both, from);
#pragma unroll
        for (uint32_t s = 0; s < ITEMS; s++) key[s] = Composite::key(both[s]);
        if (WITH_VALS)
        {
            __syncthreads(); // every thread has read its segment words: the values take their place
#pragma unroll
            for (uint32_t g = 0; g < ITEMS; g++)
            {
                const uint32_t x = g * kMergeThreads + tid;
                if (x < count) lv[x] = held[g];
            }
            __syncthreads();
        }
    }
    else
        merge_batch_thread<ITEMS>(diag, todo, na, nb, [&](uint32_t x) { return lk[x]; }, key, from);
    // what the count kernel decided: this thread's kept outputs and their first rank in the tile; the tile's kept outputs
    const uint32_t word = m.words[(size_t) t * kMergeThreads + tid], last = m.words[(size_t) t * kMergeThreads + kMergeThreads - 1u];
    const uint32_t mask = set_batch_word_mask(word) & ((1u << todo) - 1u);
    uint32_t rank = set_batch_word_rank(word);
    uint32_t tile_kept = set_batch_word_rank(last) + set_batch_word_kept(last);
    tile_kept = tile_kept < count ? tile_kept : count;
    uint32_t val[ITEMS];
    if (WITH_VALS)
    {
#pragma unroll
        for (uint32_t s = 0; s < ITEMS; s++) val[s] = (mask >> s & 1u) ? lv[from[s]] : 0u;
    }
    __syncthreads(); // every thread has read what it merges

    K* out_keys = m.out_keys + (size_t) first;
    uint32_t* out_vals = WITH_VALS ? m.out_vals + (size_t) first : nullptr;
    const uint32_t klo = merge_pack_offset(out_keys), vlo = WITH_VALS ? merge_pack_offset(out_vals) : 0u;
#pragma unroll
    for (uint32_t s = 0; s < ITEMS; s++)
        if ((mask >> s & 1u) && rank < count) // (rank < diag + s by construction; held to the tile all the same)
        {
            lk[klo + rank] = codec.decode(key[s]);
            if (WITH_VALS) lv[vlo + rank] = val[s];
            rank++;
        }
    __syncthreads();
    const uint32_t room = m.room - first; // > 0
    const uint32_t n = tile_kept < room ? tile_kept : room;
    merge_store_tile(lk, klo, n, out_keys);
    if (WITH_VALS) merge_store_tile(lv, vlo, n, out_vals);
}

} // namespace glu_hip
