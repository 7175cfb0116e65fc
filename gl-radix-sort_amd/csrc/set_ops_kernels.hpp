// set_ops_kernels.hpp -- gfx950 kernels of SET OPERATIONS (glu_set_ops_run_ptr): union, intersection, difference and symmetric
// difference of two sorted arrays of keys, with or without 4-byte values, with multiset semantics.  Not in the reference.
//
// The output is a subsequence of merge's output (merge_kernels.hpp): the stable merge of A || B with the elements an operation does
// not keep left out.  Which are kept is set_ops_path.hpp (plain C++, tested on the host).  The tiles are merge's tiles.
//   bounds  set_ops_bounds_kernel: one thread per tile boundary d = t * TILE, t = 0 .. tiles: merge's split, and for the first key
//           behind the boundary where its copies start in A and in B (two more searches over global memory, kernel-uniform trip
//           counts, every probe clamped).  Three words per boundary.
//   count   set_ops_count_kernel: one workgroup of 256 per tile.  The tile's keys are staged in LDS as merge stages them; every
//           thread walks its ITEMS outputs of the merged order and decides for each whether it is kept; the workgroup's number of
//           kept outputs goes to tile_counts[t].  Keys only.
//   scan    key_runs_scan_kernel (tile_count_scan_kernel.hpp): the counts scanned in place, *num_out their sum, held to the bound.
//   write   set_ops_write_kernel: the same walk with the values staged too; a workgroup scan of the threads' kept counts ranks every
//           kept output in the tile; kept keys (decoded) and values go to LDS in output order, shifted so that the 16-byte packs of
//           LDS are the packs of out + tile_counts[t], and leave through merge_store_tile.  What lies at or behind `room`
//           (min(max_out, the operation's bound)) is dropped.
// A kept element of A may have its match in B behind or in front of the tile's staged part: one clamped global load.  No atomics,
// nothing waits for another workgroup, grids follow from the counts alone.  Inputs that are not sorted give unspecified contents,
// but every tile reads only inside A and B, keeps at most its outputs, and the count and the write kernel decide alike.
#pragma once

#include "merge_kernels.hpp"
#include "set_ops_path.hpp"

namespace glu_hip
{
template<typename K>
struct SetOpsArgs
{
    const K* a_keys;
    const K* b_keys;
    const uint32_t* a_vals;
    const uint32_t* b_vals; // NULL where the operation keeps nothing of B
    K* out_keys;
    uint32_t* out_vals;
    uint32_t na, nb;
    uint32_t xf;    // KeyTransform of the key type
    uint32_t op;    // kSetUnion ..
    uint32_t tiles; // ceil((na + nb) / TILE)
    uint32_t room;  // outputs that may be written: min(max_out, the operation's bound)
    SetBounds* bounds;     // tiles + 1
    uint32_t* tile_counts; // tiles: kept per tile, then their exclusive scan
};

template<typename K>
__global__ __launch_bounds__(kMergeThreads) void set_ops_bounds_kernel(SetOpsArgs<K> m, uint32_t tile)
{
    const KeyCodec<K, true> codec(m.xf);
    const uint32_t t = blockIdx.x * kMergeThreads + threadIdx.x;
    if (t > m.tiles) return;
    const uint32_t total = m.na + m.nb; // (the host: na + nb < 2^32)
    const uint64_t d64 = (uint64_t) t * tile;
    const uint32_t d = d64 < total ? (uint32_t) d64 : total;
    m.bounds[t] = set_ops_boundary<K>(
        d, m.na, m.nb, merge_steps(m.na < m.nb ? m.na : m.nb), merge_steps(m.na), merge_steps(m.nb),
        [&](uint32_t i, bool any) { return any ? codec.encode(m.a_keys[i]) : (K) 0; },
        [&](uint32_t j, bool any) { return any ? codec.encode(m.b_keys[j]) : (K) 0; });
}

// The tile of workgroup t: its ranges as merge cuts them, its first key's starts.
template<typename K>
__device__ __forceinline__ SetTile set_ops_tile(const SetOpsArgs<K>& m, uint32_t t, uint32_t d0, uint32_t count)
{
    const SetBounds b0 = m.bounds[t], b1 = m.bounds[t + 1];
    const MergeRanges r = merge_tile_ranges(b0.split, b1.split, d0, d0 + count);
    SetTile s;
    s.a0 = r.a0, s.na = r.a1 - r.a0, s.b0 = r.b0, s.nb = r.b1 - r.b0; // na + nb == count
    s.nb_all = m.nb;
    s.start_a = b0.start_a, s.start_b = b0.start_b;
    return s;
}

// One thread's walk over the staged tile lk (encoded keys, A's then B's): set_ops_thread with its accessors.
template<uint32_t ITEMS, typename K, typename Keep>
__device__ __forceinline__ uint32_t set_ops_walk(const SetOpsArgs<K>& m, const KeyCodec<K, true>& codec, const SetTile& r, const K* lk,
                                                 uint32_t count, uint32_t diag, Keep keep)
{
    const uint32_t todo = count - diag < ITEMS ? count - diag : ITEMS;
    const uint32_t steps = merge_steps(r.na < r.nb ? r.na : r.nb); // (workgroup-uniform)
    const auto key_at = [&](uint32_t x, bool any) { return any ? lk[x] : (K) 0; };
    const uint32_t i0 = merge_diag_split(
        diag, r.na, r.nb, steps, [&](uint32_t i, bool any) { return any ? lk[i] : (K) 0; },
        [&](uint32_t j, bool any) { return any ? lk[r.na + j] : (K) 0; });
    return set_ops_thread<ITEMS, K>(
        m.op, r, diag, i0, todo, merge_steps(r.na), merge_steps(r.nb), key_at,
        [&](uint32_t j, bool any) {
            // (j < nb_all where any) staged: b0 <= j < b0 + nb
            const uint32_t local = j - r.b0;
            if (!any) return (K) 0;
            return local < r.nb ? lk[r.na + local] : codec.encode(m.b_keys[j]);
        },
        keep);
}

template<typename K>
__device__ __forceinline__ void set_ops_stage_keys(const SetOpsArgs<K>& m, const KeyCodec<K, true>& codec, const SetTile& r, K* lk,
                                                   uint32_t count, uint32_t items)
{
    for (uint32_t g = 0; g < items; g++)
    {
        const uint32_t x = g * kMergeThreads + threadIdx.x;
        if (x < count)
        {
            const bool from_a = x < r.na;
            const size_t at = from_a ? (size_t) r.a0 + x : (size_t) r.b0 + (x - r.na);
            lk[x] = codec.encode(from_a ? m.a_keys[at] : m.b_keys[at]);
        }
    }
}

template<typename K>
__global__ __launch_bounds__(kMergeThreads) void set_ops_count_kernel(SetOpsArgs<K> m)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), true), TILE = merge_tile(sizeof(K), true);
    constexpr uint32_t KVEC = 16 / sizeof(K), WAVES = kMergeThreads / kWave;
    __shared__ Pack<K, KVEC> key_packs[TILE / KVEC];
    __shared__ uint32_t wave_kept[WAVES];
    K* lk = &key_packs[0].v[0];

    const KeyCodec<K, true> codec(m.xf);
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const uint32_t total = m.na + m.nb;
    const uint32_t d0 = t * TILE; // (t < tiles: d0 < total)
    const uint32_t count = total - d0 < TILE ? total - d0 : TILE;
    const SetTile r = set_ops_tile(m, t, d0, count);
    set_ops_stage_keys(m, codec, r, lk, count, ITEMS);
    __syncthreads();

    const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
    const uint32_t kept = set_ops_walk<ITEMS, K>(m, codec, r, lk, count, diag, [](uint32_t, uint32_t, K, bool) {});
    uint32_t wave_total;
    wave_exclusive_sum(kept, tid % kWave, wave_total);
    if (tid % kWave == 0) wave_kept[tid / kWave] = wave_total;
    __syncthreads();
    if (tid == 0)
    {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < WAVES; w++) sum += wave_kept[w];
        m.tile_counts[t] = sum < count ? sum : count; // (at most the tile's outputs by construction; held to it all the same)
    }
}

template<typename K, bool WITH_VALS>
__global__ __launch_bounds__(kMergeThreads) void set_ops_write_kernel(SetOpsArgs<K> m)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), WITH_VALS), TILE = merge_tile(sizeof(K), WITH_VALS);
    constexpr uint32_t KVEC = 16 / sizeof(K), VVEC = 4, WAVES = kMergeThreads / kWave;
    static_assert(ITEMS <= 32, "a thread's kept outputs are the bits of a word");
    static_assert((TILE + KVEC) * sizeof(K) + (WITH_VALS ? (TILE + VVEC) * 4 : 0) + WAVES * 4 <= 32768, "five workgroups to the CU");
    // one pack more than the tile: the outputs lie up to a pack's length behind the start
    __shared__ Pack<K, KVEC> key_packs[TILE / KVEC + 1];
    __shared__ Pack<uint32_t, VVEC> val_packs[WITH_VALS ? TILE / VVEC + 1 : 1];
    __shared__ uint32_t wave_kept[WAVES];
    K* lk = &key_packs[0].v[0];
    uint32_t* lv = &val_packs[0].v[0];

    const KeyCodec<K, true> codec(m.xf);
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const uint32_t total = m.na + m.nb;
    const uint32_t d0 = t * TILE; // (t < tiles: d0 < total)
    const uint32_t count = total - d0 < TILE ? total - d0 : TILE;
    const uint32_t first = m.tile_counts[t]; // the tile's first output
    if (first >= m.room) return;             // (workgroup-uniform) nothing of this tile may be written
    const SetTile r = set_ops_tile(m, t, d0, count);
    set_ops_stage_keys(m, codec, r, lk, count, ITEMS);
    if (WITH_VALS)
    {
        const bool b_too = m.b_vals != nullptr; // (kernel-uniform)
#pragma unroll
        for (uint32_t g = 0; g < ITEMS; g++)
        {
            const uint32_t x = g * kMergeThreads + tid;
            if (x < count)
            {
                const bool from_a = x < r.na;
                const size_t at = from_a ? (size_t) r.a0 + x : (size_t) r.b0 + (x - r.na);
                lv[x] = from_a ? m.a_vals[at] : (b_too ? m.b_vals[at] : 0u);
            }
        }
    }
    __syncthreads();

    const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
    K key[ITEMS];
    uint32_t from[ITEMS];
    uint32_t mask = 0;
    const uint32_t kept = set_ops_walk<ITEMS, K>(m, codec, r, lk, count, diag, [&](uint32_t s, uint32_t x, K k, bool keep) {
        key[s] = k;
        from[s] = x;
        mask |= keep ? 1u << s : 0u;
    });
    uint32_t val[ITEMS];
    if (WITH_VALS)
    {
#pragma unroll
        for (uint32_t s = 0; s < ITEMS; s++) val[s] = (mask >> s & 1u) ? lv[from[s]] : 0u;
    }
    // the rank of the thread's first kept output in the tile
    uint32_t wave_total;
    uint32_t rank = wave_exclusive_sum(kept, tid % kWave, wave_total);
    if (tid % kWave == 0) wave_kept[tid / kWave] = wave_total;
    __syncthreads(); // every thread has read what it walks, too
    uint32_t tile_kept = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++)
    {
        rank += w < tid / kWave ? wave_kept[w] : 0u;
        tile_kept += wave_kept[w];
    }
    tile_kept = tile_kept < count ? tile_kept : count;

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
