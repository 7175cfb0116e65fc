// sorted_search_batch_kernels.hpp -- the gfx950 kernel of the BATCHED SORTED SEARCH (glu_sorted_search_run_batch_ptr,
// glu_sorted_search_run_batch_offsets_ptr): every segment's needles searched in that segment's own haystack, in one launch.
// torch.searchsorted with a batched sorted sequence, and its ragged form over device offsets.  Not in the reference.
//
// One kernel, load-balanced over the NEEDLES: a workgroup walks tiles of consecutive needles (the tiles of tile_span.hpp, as the
// single search's search_tile walks them), whatever segments they belong to, so that one segment with all the needles fills the
// device and any number of segments without needles costs nothing.  Per tile (the arithmetic is search_batch_walk.hpp's):
//   ends     the segments s_first and s_last of the tile's first and last needle: two lanes of every wave, a clamped upper bound
//            over all the needle offsets (equal rows: a quotient);
//   segment  every needle's own segment, search_range over needle_offsets[s_first + 1 .. s_last]: no trip where the tile lies
//            inside one segment (equal rows: a multiplication);
//   window   the haystacks of s_first .. s_last are one range [w0, w1) of `hay`.  Where it has at most `window` keys the workgroup
//            copies it into LDS, ENCODED, contiguous lanes reading contiguous keys, and every probe of the tile goes there;
//            otherwise the probes go to global memory, which is the DIRECT kernel's loop with a base and a length per needle.
//            The decision is workgroup-uniform.  32 KiB of static LDS: five workgroups to the CU by LDS, 20 waves.
//   bounds   search_range over the needle's own (base, len), clamped into the window or into [0, hay_total).  The trip count is
//            WAVE-uniform: search_steps of the longest haystack among the wave's needles (the OR of the lengths has the same top
//            bit as their maximum), never a loop per lane and never search_steps(hay_total).
// The positions are local to the segment.  No atomics, nothing waits for another workgroup, no scratch.
#pragma once

#include "search_batch_walk.hpp"
#include "sorted_search_kernels.hpp"

namespace glu_hip
{
static_assert(kSearchBatchPacks == kSearchPacks, "the batched search walks the single search's tiles");
static_assert(kSearchBatchLdsBytes == kSearchLdsBytes, "the window is the LDS the indexed search gives its top level");

template<typename K>
struct SearchBatchArgs
{
    const K* hay;
    const uint32_t* hay_offsets;    // NULL: equal partitions of rows.hay_count keys
    const uint32_t* needle_offsets; // NULL: equal rows of rows.m needles
    uint32_t* out_lower;
    uint32_t* out_upper;
    TileSpan<K> needles;
    SearchBatchRows rows;
    uint32_t hay_total, num_segments; // num_segments >= 1
    uint32_t window;                  // keys; 0: never stage
    uint32_t xf;                      // KeyTransform of the key type
};

// The OR of v over the wave, in every lane's hands as a scalar.  DPP moves as in wave_exclusive_sum (radix_sort_kernels.hpp): a
// lane without a source reads 0.  Every lane of the wave must be here.
__device__ __forceinline__ uint32_t search_batch_wave_or(uint32_t v)
{
    int m = (int) v;
    m |= __builtin_amdgcn_update_dpp(0, m, 0x111, 0xf, 0xf, false); // row_shr:1
    m |= __builtin_amdgcn_update_dpp(0, m, 0x112, 0xf, 0xf, false); // row_shr:2
    m |= __builtin_amdgcn_update_dpp(0, m, 0x114, 0xf, 0xf, false); // row_shr:4
    m |= __builtin_amdgcn_update_dpp(0, m, 0x118, 0xf, 0xf, false); // row_shr:8   -> lane 15 of a row holds the row
    m |= __builtin_amdgcn_update_dpp(0, m, 0x142, 0xa, 0xf, false); // row_bcast:15 into rows 1 and 3
    m |= __builtin_amdgcn_update_dpp(0, m, 0x143, 0xc, 0xf, false); // row_bcast:31 into rows 2 and 3
    return (uint32_t) __builtin_amdgcn_readlane(m, 63);
}

// NEEDLE_OFFSETS: the needles' segments come from a.needle_offsets, else from equal rows.
template<typename K, int BOUNDS, bool NEEDLE_OFFSETS>
__global__ __launch_bounds__(kTileThreads) void sorted_search_batch_kernel(SearchBatchArgs<K> a)
{
    using C = SearchCfg<K>;
    constexpr uint32_t N = C::PACKS * C::VEC, STAGE_VEC = 16 / sizeof(K);
    __shared__ Pack<K, STAGE_VEC> window_packs[kSearchBatchLdsBytes / 16];
    K* staged_keys = &window_packs[0].v[0];
    const KeyCodec<K, true> codec(a.xf);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t S = a.num_segments;
    const uint32_t* __restrict__ noff = a.needle_offsets;
    const uint32_t* __restrict__ hoff = a.hay_offsets;
    const K* __restrict__ hay = a.hay;

    for (uint32_t t = blockIdx.x; t < a.needles.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        uint32_t j0, j1;
        if (!search_batch_tile_needles(t, C::TILE, a.needles.lo, a.needles.hi, &j0, &j1)) continue;

        // ---- the tile's first and last segment
        uint32_t s_first, s_last;
        if (NEEDLE_OFFSETS)
        {
            uint32_t s = 0;
            if (lane < 2) s = search_batch_end_segment(lane == 0 ? j0 : j1 - 1u, S, [&](uint32_t i) { return noff[i]; });
            s_first = (uint32_t) __builtin_amdgcn_readlane((int) s, 0);
            s_last = search_batch_last_segment(s_first, (uint32_t) __builtin_amdgcn_readlane((int) s, 1));
        }
        else
        {
            s_first = search_batch_row(j0, a.rows, S);
            s_last = search_batch_row(j1 - 1u, a.rows, S);
        }

        // ---- the window
        const uint32_t w0 = hoff ? hoff[s_first] : s_first * a.rows.hay_count;
        const uint32_t w1 = hoff ? hoff[s_last + 1u] : (s_last + 1u) * a.rows.hay_count;
        const bool staged = search_batch_staged(w0, w1, a.hay_total, a.window);
        if (staged)
        {
            __syncthreads(); // the probes of the tile before are done
            const uint32_t n = w1 - w0;
#pragma unroll 4
            for (uint32_t i = threadIdx.x; i < n; i += kTileThreads) staged_keys[i] = codec.encode(hay[w0 + i]);
            __syncthreads();
        }

        // ---- the needles of the calling lane
        const uint64_t first = (uint64_t) t * C::TILE + wave * C::WAVE_ELEMS + lane * C::VEC;
        K x[N];
        uint32_t inside = 0;
#pragma unroll
        for (uint32_t g = 0; g < C::PACKS; g++)
            tile_load_pack<C::VEC>(a.needles, first + g * C::PACK_STRIDE, [&](uint32_t k, K key, bool in) {
                x[g * C::VEC + k] = codec.encode(key);
                inside |= (in ? 1u : 0u) << (g * C::VEC + k);
            });
        uint32_t j[N]; // the needle as an element of its array (0 outside it)
#pragma unroll
        for (uint32_t g = 0; g < C::PACKS; g++)
#pragma unroll
            for (uint32_t k = 0; k < C::VEC; k++)
            {
                const uint32_t e = g * C::VEC + k;
                j[e] = (inside >> e) & 1u ? (uint32_t) (first + g * C::PACK_STRIDE + k - a.needles.lo) : 0u;
            }

        // ---- their segments, and which of them are covered
        uint32_t seg[N], covered = inside;
        if (NEEDLE_OFFSETS)
        {
            uint32_t sb[N], sl[N], c[N];
#pragma unroll
            for (uint32_t e = 0; e < N; e++)
            {
                sb[e] = search_batch_inner_base(s_first);
                sl[e] = (inside >> e) & 1u ? search_batch_inner_len(s_first, s_last) : 0u;
            }
            search_range<true>(j, sb, sl, search_batch_inner_steps(s_first, s_last), c, [&](uint32_t i, bool any) { return any ? noff[i] : 0u; });
#pragma unroll
            for (uint32_t e = 0; e < N; e++)
            {
                seg[e] = search_batch_inner_segment(s_first, s_last, c[e] - sb[e]);
                if ((inside >> e) & 1u)
                {
                    if (!search_batch_covered(j[e], noff[seg[e]], noff[seg[e] + 1u])) covered &= ~(1u << e);
                }
            }
        }
        else
        {
#pragma unroll
            for (uint32_t e = 0; e < N; e++) seg[e] = search_batch_row(j[e], a.rows, S);
        }

        // ---- their haystacks, held inside the window or the array
        uint32_t base[N], len[N], longest = 0;
#pragma unroll
        for (uint32_t e = 0; e < N; e++)
        {
            uint32_t begin = seg[e] * a.rows.hay_count, count = a.rows.hay_count;
            if (hoff)
            {
                const bool live = (covered >> e) & 1u;
                search_batch_offsets_segment(live ? hoff[seg[e]] : 0u, live ? hoff[seg[e] + 1u] : 0u, a.hay_total, &begin, &count);
            }
            if (!((covered >> e) & 1u)) count = 0u;
            if (staged)
                search_batch_window_range(begin, count, w0, w1, &base[e], &len[e]);
            else
                search_batch_global_range(begin, count, a.hay_total, &base[e], &len[e]);
            longest |= len[e];
        }
        const uint32_t steps = search_steps(search_batch_wave_or(longest)); // (wave-uniform)

        // ---- the bounds, local to the segment
        const auto bounds = [&](auto key_at) {
            uint32_t pos[N];
            if (BOUNDS & SEARCH_LOWER)
            {
                search_range<false>(x, base, len, steps, pos, key_at);
#pragma unroll
                for (uint32_t e = 0; e < N; e++)
                    if ((covered >> e) & 1u) a.out_lower[j[e]] = pos[e] - base[e];
            }
            if (BOUNDS & SEARCH_UPPER)
            {
                search_range<true>(x, base, len, steps, pos, key_at);
#pragma unroll
                for (uint32_t e = 0; e < N; e++)
                    if ((covered >> e) & 1u) a.out_upper[j[e]] = pos[e] - base[e];
            }
        };
        if (staged) // (workgroup-uniform)
            bounds([&](uint32_t i, bool any) { return any ? staged_keys[i] : (K) 0; }); // (no keys: base may be the window's end)
        else
            bounds([&](uint32_t i, bool any) { return any ? codec.encode(hay[i]) : (K) 0; });
    }
}

} // namespace glu_hip
