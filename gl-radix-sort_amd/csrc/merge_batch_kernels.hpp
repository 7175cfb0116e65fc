// merge_batch_kernels.hpp -- gfx950 kernels of the BATCHED MERGE (glu_merge_run_batch_offsets_ptr, glu_merge_run_batch_ptr): the
// two sorted runs of every segment into one, all segments in one call, over device offsets.  Not in the reference.
//
// One merge path over all of A and all of B under the composite order (segment, enc(key)); its arithmetic is merge_batch_path.hpp
// (plain C++, walked on the host by tests/test_merge_batch_path.py).  The work is balanced over the OUTPUTS: one long segment fills
// the device, and any number of empty segments costs a tile nothing but a few more probes of its bounds.
//   partition  merge_batch_partition_kernel: one thread per tile boundary d = t * TILE (clamped to the device total): the boundary's
//              segment by an upper bound over oa[s] + ob[s] (two offset loads a probe, kernel-uniform trip count), then the split of
//              the local diagonal inside that one segment; (split, segment) to scratch, (tiles + 1) * 8 bytes.  The same threads
//              write out_offsets, one entry each (the grid covers the longer of the two).
//   tile       merge_batch_tile_kernel: one workgroup of 256 per tile, the single merge's TILE.  A tile's elements of A are one
//              contiguous range of a_keys and its elements of B one of b_keys, also across segments (adjacent segments touch): the
//              staging is the single kernel's.  A tile inside one segment (workgroup-uniform, from the two stored segments and one
//              pair of offsets) then runs the single merge's body.  A tile over several segments gives every staged element its
//              segment relative to the tile's first (one bound over the tile's offsets per element, never a loop over segments) in
//              a word beside its key, and splits and merges by the composite (segment, key).  Both leave through merge_store_tile.
// LDS: the segment words lie where the values are staged.  A tile of several segments holds its values in registers (ITEMS a thread)
// while it merges and stages them behind one more barrier, so every instantiation keeps the single kernel's footprint with values
// (22 560 bytes for 4-byte keys, 21 536 for 8-byte keys) and its five workgroups to the CU.
// No atomics, no look-back, nothing waits for another workgroup.  Offsets that decrease or leave their total and inputs that are
// not sorted give unspecified contents; every index still lies inside its array and every output is written by one tile alone.
#pragma once

#include "merge_batch_path.hpp"
#include "merge_kernels.hpp"

namespace glu_hip
{
template<typename K>
struct MergeBatchArgs
{
    const K* a_keys;
    const K* b_keys;
    const uint32_t* a_vals;
    const uint32_t* b_vals;
    K* out_keys;
    uint32_t* out_vals;
    const uint32_t* a_offsets; // num_segments + 1 words, or NULL: a_offsets[s] = s * a_len
    const uint32_t* b_offsets;
    uint32_t a_len, b_len;
    uint32_t a_total, b_total; // the arrays' lengths: every access lies below them
    uint32_t num_segments;     // >= 1
    uint32_t xf;               // KeyTransform of the key type
    uint32_t tiles;            // ceil((a_total + b_total) / TILE)
    uint32_t seg_steps;        // merge_steps(num_segments - 1)
    uint32_t split_steps;      // merge_steps(min(a_total, b_total))
    MergeBatchBoundary* bounds; // tiles + 1 boundaries
    uint32_t* out_offsets;     // num_segments + 1 words, or NULL

    __device__ __forceinline__ uint32_t off_a(uint32_t s) const { return a_offsets ? a_offsets[s] : s * a_len; }
    __device__ __forceinline__ uint32_t off_b(uint32_t s) const { return b_offsets ? b_offsets[s] : s * b_len; }
};

template<typename K>
__global__ __launch_bounds__(kMergeThreads) void merge_batch_partition_kernel(MergeBatchArgs<K> m, uint32_t tile)
{
    const KeyCodec<K, true> codec(m.xf);
    const uint32_t g = blockIdx.x * kMergeThreads + threadIdx.x;
    const auto off_a = [&](uint32_t s) { return m.off_a(s); };
    const auto off_b = [&](uint32_t s) { return m.off_b(s); };
    const MergeBatchSide a = merge_batch_side(off_a, m.num_segments, m.a_total), b = merge_batch_side(off_b, m.num_segments, m.b_total);
    if (m.out_offsets && g <= m.num_segments) m.out_offsets[g] = merge_batch_rel(off_a(g), a) + merge_batch_rel(off_b(g), b);
    if (g > m.tiles) return;
    const uint32_t total = a.len + b.len; // (the host: a_total + b_total < 2^32)
    const uint64_t d64 = (uint64_t) g * tile;
    const uint32_t d = d64 < total ? (uint32_t) d64 : total;
    m.bounds[g] = merge_batch_boundary(
        d, m.num_segments, a, b, m.seg_steps, m.split_steps, off_a, off_b, [&](uint32_t i, bool any) { return any ? codec.encode(m.a_keys[i]) : (K) 0; },
        [&](uint32_t j, bool any) { return any ? codec.encode(m.b_keys[j]) : (K) 0; });
}

// One thread's ITEMS outputs of a tile whose keys at(x) lie side by side (na of A, then nb of B): key[s] and the LDS index from[s].
template<uint32_t ITEMS, typename C, typename At>
__device__ __forceinline__ void merge_batch_thread(uint32_t diag, uint32_t todo, uint32_t na, uint32_t nb, At at, C (&key)[ITEMS], uint32_t (&from)[ITEMS])
{
    const uint32_t steps = merge_steps(na < nb ? na : nb); // (workgroup-uniform)
    const uint32_t i0 = merge_diag_split(
        diag, na, nb, steps, [&](uint32_t i, bool any) { return any ? at(i) : C(); }, [&](uint32_t j, bool any) { return any ? at(na + j) : C(); });
    merge_serial<ITEMS, C>(
        i0, diag - i0, na, nb, todo, [&](uint32_t x, bool any) { return any ? at(x) : C(); },
        [&](uint32_t s, uint32_t x, C k, bool live) {
            key[s] = k;
            from[s] = live ? x : 0u;
        });
}

// (seven waves a SIMD, what the LDS allows: left alone the 4-byte pairs take 74 registers, six waves, and the one-segment row 13 % more
// than the single merge instead of its own spread)
template<typename K, bool WITH_VALS>
__global__ __launch_bounds__(kMergeThreads, 7) void merge_batch_tile_kernel(MergeBatchArgs<K> m)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), WITH_VALS), TILE = merge_tile(sizeof(K), WITH_VALS);
    constexpr uint32_t KVEC = 16 / sizeof(K), VVEC = 4;
    typedef MergeBatchComposite<K> Composite;
    static_assert(ITEMS % 2 == 1, "neighbouring lanes start their serial merge an odd number of words apart");
    static_assert(TILE % KVEC == 0 && TILE % VVEC == 0, "every tile of out starts as far behind a 16-byte boundary as out does");
    static_assert((TILE + KVEC) * sizeof(K) + (TILE + VVEC) * 4 <= 32768, "five workgroups to the CU");
    // one pack more than the tile: the outputs lie up to a pack's length behind the start
    __shared__ Pack<K, KVEC> key_packs[TILE / KVEC + 1];
    __shared__ Pack<uint32_t, VVEC> val_packs[TILE / VVEC + 1]; // the values; in a tile of several segments the segment words first
    K* lk = &key_packs[0].v[0];
    uint32_t* lv = &val_packs[0].v[0];

    const KeyCodec<K, true> codec(m.xf);
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const auto off_a = [&](uint32_t s) { return m.off_a(s); };
    const auto off_b = [&](uint32_t s) { return m.off_b(s); };
    const MergeBatchSide a = merge_batch_side(off_a, m.num_segments, m.a_total), b = merge_batch_side(off_b, m.num_segments, m.b_total);
    const uint32_t total = a.len + b.len;
    const uint32_t d0 = t * TILE; // (t < tiles: d0 < a_total + b_total)
    if (d0 >= total) return;      // (workgroup-uniform)
    const uint32_t count = total - d0 < TILE ? total - d0 : TILE;
    const MergeBatchTile tile = merge_batch_tile(m.bounds[t], m.bounds[t + 1], d0, d0 + count, m.num_segments, [&](uint32_t s) {
        return merge_batch_rel(off_a(s + 1u), a) + merge_batch_rel(off_b(s + 1u), b);
    });
    const MergeRanges r = tile.r;
    const uint32_t na = r.a1 - r.a0, nb = r.b1 - r.b0; // na + nb == count
    const bool several = !tile.one;                    // (workgroup-uniform)
    const uint32_t seg_steps = merge_steps(tile.span);

    // stage: the keys of A, then the keys of B, encoded; beside them the values, or (several segments) each element's segment
    uint32_t held[ITEMS]; // several segments: the values wait here for the segment words' place
#pragma unroll
    for (uint32_t g = 0; g < ITEMS; g++)
    {
        const uint32_t x = g * kMergeThreads + tid;
        held[g] = 0u;
        if (x < count)
        {
            const bool from_a = x < na;
            const uint32_t rel = from_a ? r.a0 + x : r.b0 + (x - na); // (inside the side)
            const size_t at = (size_t) (from_a ? a.begin : b.begin) + rel;
            lk[x] = codec.encode(from_a ? m.a_keys[at] : m.b_keys[at]);
            uint32_t v = 0u;
            if (WITH_VALS) v = from_a ? m.a_vals[at] : m.b_vals[at];
            if (several)
            {
                held[g] = v;
                lv[x] = from_a ? merge_batch_element_segment(rel, tile.seg0, tile.span, seg_steps, [&](uint32_t s) { return merge_batch_rel(off_a(s), a); })
                               : merge_batch_element_segment(rel, tile.seg0, tile.span, seg_steps, [&](uint32_t s) { return merge_batch_rel(off_b(s), b); });
            }
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
    uint32_t val[ITEMS];
    if (WITH_VALS)
    {
#pragma unroll
        for (uint32_t s = 0; s < ITEMS; s++) val[s] = s < todo ? lv[from[s]] : 0u;
    }
    __syncthreads(); // every thread has read what it merges

    K* out_keys = m.out_keys + (size_t) d0;
    uint32_t* out_vals = WITH_VALS ? m.out_vals + (size_t) d0 : nullptr;
    const uint32_t klo = merge_pack_offset(out_keys), vlo = WITH_VALS ? merge_pack_offset(out_vals) : 0u;
#pragma unroll
    for (uint32_t s = 0; s < ITEMS; s++)
        if (s < todo)
        {
            lk[klo + diag + s] = codec.decode(key[s]);
            if (WITH_VALS) lv[vlo + diag + s] = val[s];
        }
    __syncthreads();
    merge_store_tile(lk, klo, count, out_keys);
    if (WITH_VALS) merge_store_tile(lv, vlo, count, out_vals);
}

} // namespace glu_hip
