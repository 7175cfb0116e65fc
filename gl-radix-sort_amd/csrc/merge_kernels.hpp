// merge_kernels.hpp -- gfx950 kernels of MERGE (glu_merge_run_ptr): two sorted arrays of keys, with or without 4-byte values, into
// one, stable.  Not in the reference.
//
// With enc = the sort's KeyCodec::encode (radix_sort_kernels.hpp): out = the stable sort of the concatenation A || B by enc(key).
// Among equal keys every element of A lies in front of every element of B and each side keeps its order: A[i] lands at
// i + #{j : enc(B[j]) < enc(A[i])} (sorted search's lower bound), B[j] at j + #{i : enc(A[i]) <= enc(B[j])} (its upper bound).
//
// The algorithm is merge path; its arithmetic is merge_path.hpp (plain C++, tested on the host).
//   partition  merge_partition_kernel: one thread per tile boundary d = t * TILE, t = 0 .. tiles: split[t] = the keys of A among
//              the first d outputs, by the split loop over global memory (kernel-uniform trip count, every probe clamped).
//   tile       merge_tile_kernel: one workgroup of 256 per tile.  The tile's keys of A and of B are loaded by contiguous lanes and
//              laid side by side in LDS, encoded; every thread finds the split of its own diagonal (ITEMS outputs apart) in LDS and
//              merges ITEMS steps serially, keeping the keys and the LDS index each came from; the values, staged in LDS the same
//              way, are gathered by those indices.  Keys (decoded) and values then go back to LDS in OUTPUT order, shifted so that
//              the 16-byte packs of LDS are the 16-byte packs of `out`, and leave as whole packs by contiguous lanes (the packs
//              that hold the first and the last output of the tile go element by element): no store strides ITEMS elements
//              between lanes.
// No atomics, no look-back, nothing waits for another workgroup.  Inputs that are not sorted give unspecified contents, but every
// tile still reads only its ranges of A and B (merge_tile_ranges' clamp) and writes exactly its outputs.
#pragma once

#include "merge_path.hpp"
#include "radix_sort_kernels.hpp"
#include "scan_reduce_kernels.hpp"

namespace glu_hip
{
template<typename K>
struct MergeArgs
{
    const K* a_keys;
    const K* b_keys;
    const uint32_t* a_vals;
    const uint32_t* b_vals;
    K* out_keys;
    uint32_t* out_vals;
    uint32_t na, nb;
    uint32_t xf;    // KeyTransform of the key type
    uint32_t tiles; // ceil((na + nb) / TILE)
    uint32_t* split; // tiles + 1 words
};

template<typename K>
__global__ __launch_bounds__(kMergeThreads) void merge_partition_kernel(MergeArgs<K> m, uint32_t tile)
{
    const KeyCodec<K, true> codec(m.xf);
    const uint32_t t = blockIdx.x * kMergeThreads + threadIdx.x;
    if (t > m.tiles) return;
    const uint32_t total = m.na + m.nb; // (the host: na + nb < 2^32)
    const uint64_t d64 = (uint64_t) t * tile;
    const uint32_t d = d64 < total ? (uint32_t) d64 : total;
    const uint32_t steps = merge_steps(m.na < m.nb ? m.na : m.nb); // (kernel-uniform)
    m.split[t] = merge_diag_split(
        d, m.na, m.nb, steps, [&](uint32_t i, bool any) { return any ? codec.encode(m.a_keys[i]) : (K) 0; },
        [&](uint32_t j, bool any) { return any ? codec.encode(m.b_keys[j]) : (K) 0; });
}

// `count` elements in output order, lds[lo + e] = element e, to out[0 .. count), lo = the elements between the 16-byte boundary at
// or below `out` and `out`: pack p of LDS is pack p from that boundary.
template<typename T>
__device__ __forceinline__ void merge_store_tile(const T* lds, uint32_t lo, uint32_t count, T* out)
{
    constexpr uint32_t VEC = 16 / sizeof(T);
    T* base = out - lo;
    const uint32_t hi = lo + count, packs = (hi + VEC - 1) / VEC;
    for (uint32_t p = threadIdx.x; p < packs; p += kMergeThreads)
    {
        const uint32_t e0 = p * VEC;
        if (e0 >= lo && e0 + VEC <= hi)
            *reinterpret_cast<Pack<T, VEC>*>(base + e0) = *reinterpret_cast<const Pack<T, VEC>*>(lds + e0);
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++)
                if (e0 + k >= lo && e0 + k < hi) base[e0 + k] = lds[e0 + k];
        }
    }
}

template<typename T>
__device__ __forceinline__ uint32_t merge_pack_offset(const T* p)
{
    return (uint32_t) (((uintptr_t) p & 15u) / sizeof(T));
}

template<typename K, bool WITH_VALS>
__global__ __launch_bounds__(kMergeThreads) void merge_tile_kernel(MergeArgs<K> m)
{
    constexpr uint32_t ITEMS = merge_items(sizeof(K), WITH_VALS), TILE = merge_tile(sizeof(K), WITH_VALS);
    constexpr uint32_t KVEC = 16 / sizeof(K), VVEC = 4;
    static_assert(ITEMS % 2 == 1, "neighbouring lanes start their serial merge an odd number of words apart");
    static_assert(TILE % KVEC == 0 && TILE % VVEC == 0, "every tile of out starts as far behind a 16-byte boundary as out does");
    static_assert((TILE + KVEC) * sizeof(K) + (WITH_VALS ? (TILE + VVEC) * 4 : 0) <= 32768, "five workgroups to the CU");
    // one pack more than the tile: the outputs lie up to a pack's length behind the start
    __shared__ Pack<K, KVEC> key_packs[TILE / KVEC + 1];
    __shared__ Pack<uint32_t, VVEC> val_packs[WITH_VALS ? TILE / VVEC + 1 : 1];
    K* lk = &key_packs[0].v[0];
    uint32_t* lv = &val_packs[0].v[0];

    const KeyCodec<K, true> codec(m.xf);
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const uint32_t total = m.na + m.nb;
    const uint32_t d0 = t * TILE; // (t < tiles: d0 < total)
    const uint32_t count = total - d0 < TILE ? total - d0 : TILE;
    const MergeRanges r = merge_tile_ranges(m.split[t], m.split[t + 1], d0, d0 + count);
    const uint32_t na = r.a1 - r.a0, nb = r.b1 - r.b0; // na + nb == count

    // stage: the keys of A, then the keys of B, encoded; the values beside them
#pragma unroll
    for (uint32_t g = 0; g < ITEMS; g++)
    {
        const uint32_t x = g * kMergeThreads + tid;
        if (x < count)
        {
            const bool from_a = x < na;
            const size_t at = from_a ? (size_t) r.a0 + x : (size_t) r.b0 + (x - na);
            lk[x] = codec.encode(from_a ? m.a_keys[at] : m.b_keys[at]);
            if (WITH_VALS) lv[x] = from_a ? m.a_vals[at] : m.b_vals[at];
        }
    }
    __syncthreads();

    const uint32_t diag = merge_thread_diag(tid, ITEMS, count);
    const uint32_t todo = count - diag < ITEMS ? count - diag : ITEMS;
    const uint32_t steps = merge_steps(na < nb ? na : nb); // (workgroup-uniform)
    const uint32_t i0 = merge_diag_split(
        diag, na, nb, steps, [&](uint32_t i, bool any) { return any ? lk[i] : (K) 0; },
        [&](uint32_t j, bool any) { return any ? lk[na + j] : (K) 0; });
    K key[ITEMS];
    uint32_t from[ITEMS];
    merge_serial<ITEMS, K>(
        i0, diag - i0, na, nb, todo, [&](uint32_t x, bool any) { return any ? lk[x] : (K) 0; },
        [&](uint32_t s, uint32_t x, K k, bool live) {
            key[s] = k;
            from[s] = live ? x : 0u;
        });
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
