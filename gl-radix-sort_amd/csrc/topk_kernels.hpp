// topk_kernels.hpp -- gfx950 kernels of TOP-K (glu_top_k_run_ptr): the k smallest or largest keys and their indices by a radix
// select.  Not in the reference.
//
// The arithmetic of a select (the digit windows, the crossing digit, the state and its update, the choice of the path) is
// topk_pick.hpp, plain C++ that a host test runs whole selects through.  The kernels work on code words c = KeyCodec::encode(key),
// complemented for `largest` (TopkCode): "the k smallest unsigned words" in every case, in the order of the sort.
//   round 1      topk_count_kernel over the input: `groups` workgroups count the top digit of every key into a table of 2048 counters in
//                LDS (histogram_walk.hpp: whole 16-byte packs, ends masked, one add per wave where the keys are one value) and store it
//                as a row of partial[groups][2048] by plain stores; topk_sum_kernel sums the columns; topk_pick_kernel, one workgroup,
//                scans the 2048 sums, finds the crossing digit, updates the state and chooses the path.
//   CANDIDATES   topk_collect_kernel reads the input once more and appends the code words that match the prefix to the candidate
//                buffer; topk_cand_rounds_kernel, one workgroup, runs every remaining round over the candidates.
//   FULL         count, sum and pick again for every remaining round, over the input, filtered by the prefix.
//                Both chains are always enqueued: a kernel of the chain not taken reads the state and returns at once.
//   compaction   topk_flag_count_kernel: per tile, the keys below the threshold word T and the keys equal to it; the count scan of key
//                runs and select over each array; topk_write_kernel flags the tiles again and emits every c < T and the first `need`
//                c == T at the rank less_before + min(ties_before, need): ascending indices, exactly k of them.
//   ordering     the write kernel stores (code word, index) pairs, the library's sort orders them, topk_decode_kernel writes the outputs.
// THE ONE ATOMIC ON DEVICE MEMORY is the append of topk_collect_kernel: one atomicAdd per workgroup whenever it holds more than a
// tile's worth of candidates in LDS, and at its end.  The candidates arrive in arbitrary order, and that does not matter: only counts are taken from them, and integer counts
// commute.  Everything a caller sees is written at ranks that follow from counts alone: the same input gives the same bits.
#pragma once

#include "histogram_walk.hpp"
#include "radix_sort_kernels.hpp"
#include "topk_pick.hpp"

namespace glu_hip
{
static_assert(kTopkThreads == kTileThreads && kTopkThreads == hist_threads(4, HIST_EVEN) && kTopkPacks == kHistPacks,
              "topk_pick.hpp states the tile of select and of the even histogram for itself");

// the key of a call as a code word and back
template<typename K>
struct TopkCode
{
    uint32_t xf;     // KEY_XF_*
    uint32_t largest; // != 0: the code is complemented
    __device__ __forceinline__ K flip() const { return largest ? (K) ~(K) 0 : (K) 0; }
    __device__ __forceinline__ K encode(K key) const { return KeyCodec<K>(xf).encode(key) ^ flip(); }
    __device__ __forceinline__ K decode(K code) const { return KeyCodec<K>(xf).decode(code ^ flip()); }
};

// What a call passes to its streaming kernels.  K: the keys as unsigned words of their width.
template<typename K>
struct TopkArgs
{
    TileSpan<K> keys;
    TopkCode<K> code;
};

// the rule of the counting walk: the digit of a key that matches the prefix
template<typename K>
struct TopkDigit
{
    TopkCode<K> code;
    K prefix, mask;
    uint32_t shift, bits;
};
template<typename K>
__device__ __forceinline__ uint32_t hist_bin_of(const TopkDigit<K>& r, K x, const K*)
{
    const K c = r.code.encode(x);
    return (c & r.mask) == r.prefix ? topk_digit(c, r.shift, r.bits) : kHistNoBin;
}

// One round over the input: row blockIdx.x of partial[gridDim.x][kTopkBins].  round > 0 belongs to the FULL chain.
template<typename K>
__global__ __launch_bounds__(kTopkThreads) void topk_count_kernel(TopkArgs<K> a, uint32_t round, const TopkState* __restrict__ state,
                                                                  uint32_t* __restrict__ partial)
{
    __shared__ uint32_t table[kTopkBins];
    HistArgs<K, TopkDigit<K>> h;
    h.samples = a.keys;
    h.rule.code = a.code;
    h.rule.prefix = h.rule.mask = (K) 0;
    if (round)
    {
        if (state->path != (uint32_t) TOPK_PATH_FULL) return; // (workgroup-uniform)
        h.rule.prefix = (K) state->prefix;
        h.rule.mask = (K) state->mask;
    }
    h.rule.shift = topk_shift(sizeof(K), round);
    h.rule.bits = topk_bits(sizeof(K), round);
    h.bins = kTopkBins;
    h.dst = partial;
    for (uint32_t b = threadIdx.x; b < kTopkBins; b += kTopkThreads) table[b] = 0u;
    __syncthreads();
    hist_walk<K, kTopkThreads>(h, (const K*) nullptr, [&](uint32_t bin, uint32_t n) {
        if (bin < kTopkBins) atomicAdd(&table[bin], n);
    });
    __syncthreads();
    uint32_t* row = partial + (size_t) blockIdx.x * kTopkBins;
    for (uint32_t b = threadIdx.x; b < kTopkBins; b += kTopkThreads) row[b] = table[b];
}

// sums[b] = the sum of column b of partial[groups][kTopkBins]: 64 columns to the workgroup, its four waves taking the rows w, w + 4, ...
constexpr uint32_t kTopkSumThreads = 256, kTopkSumCols = 64;
__global__ __launch_bounds__(kTopkSumThreads) void topk_sum_kernel(const uint32_t* __restrict__ partial, uint32_t groups, uint32_t round,
                                                                   const TopkState* __restrict__ state, uint32_t* __restrict__ sums)
{
    constexpr uint32_t SLICES = kTopkSumThreads / kTopkSumCols;
    __shared__ uint32_t part[SLICES][kTopkSumCols];
    if (round && state->path != (uint32_t) TOPK_PATH_FULL) return; // (workgroup-uniform)
    const uint32_t col = threadIdx.x % kTopkSumCols, slice = threadIdx.x / kTopkSumCols;
    const uint32_t b = blockIdx.x * kTopkSumCols + col; // (below kTopkBins: the grid)
    uint32_t sum = 0;
#pragma unroll 4
    for (uint32_t g = slice; g < groups; g += SLICES) sum += partial[(size_t) g * kTopkBins + b];
    part[slice][col] = sum;
    __syncthreads();
    if (slice == 0)
    {
#pragma unroll
        for (uint32_t s = 1; s < SLICES; s++) sum += part[s][col];
        sums[b] = sum;
    }
}

// The crossing digit of a table of kTopkBins counters, by the kTopkPickThreads threads of a workgroup: thread t holds the counters
// c0 = table[2t] and c1 = table[2t + 1].  result[0 .. 3) = the digit, the words in front of it, the words in it.  Ends with a barrier.
__device__ __forceinline__ void topk_block_pick(uint32_t c0, uint32_t c1, uint32_t need, uint32_t* wave_sums, uint32_t* result)
{
    constexpr uint32_t WAVES = kTopkPickThreads / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t total;
    uint32_t before = wave_exclusive_sum(c0 + c1, lane, total);
    if (lane == 0) wave_sums[wave] = total;
    __syncthreads();
    before += sum_of_preceding_waves(wave_sums, (int) WAVES, wave, lane);
    if (topk_crosses(before, c0, need))
    {
        result[0] = 2u * threadIdx.x;
        result[1] = before;
        result[2] = c0;
    }
    else if (topk_crosses(before + c0, c1, need))
    {
        result[0] = 2u * threadIdx.x + 1u;
        result[1] = before + c0;
        result[2] = c1;
    }
    __syncthreads();
}

// One workgroup: the state after a round over the input.  round 0 starts the state and chooses the path; the last round of the FULL
// chain stores the k-th key.
template<typename K>
__global__ __launch_bounds__(kTopkPickThreads) void topk_pick_kernel(const uint32_t* __restrict__ sums, uint32_t round, uint32_t count, uint32_t k,
                                                                     uint32_t option, uint32_t capacity, TopkCode<K> code,
                                                                     TopkState* __restrict__ state, K* __restrict__ out_kth)
{
    __shared__ uint32_t wave_sums[kTopkPickThreads / 64], result[3];
    __shared__ TopkState s;
    if (round && state->path != (uint32_t) TOPK_PATH_FULL) return; // (workgroup-uniform)
    if (threadIdx.x == 0)
    {
        s = round ? *state : topk_begin(count, k);
        result[0] = result[1] = result[2] = 0u;
    }
    __syncthreads();
    const uint2 c = reinterpret_cast<const uint2*>(sums)[threadIdx.x];
    topk_block_pick(c.x, c.y, s.need, wave_sums, result);
    if (threadIdx.x == 0)
    {
        topk_advance(s, sizeof(K), round, result[0], result[1], result[2]);
        if (round == 0) s.path = topk_choose_path(option, s.bucket, capacity);
        *state = s;
        if (out_kth && round + 1u == topk_rounds(sizeof(K))) *out_kth = code.decode((K) s.prefix);
    }
}

// CANDIDATES: the code words of the input that match the prefix of round 1, appended to cand[0 .. capacity) in arbitrary order.
// A workgroup keeps its candidates in LDS (room for two tiles) and appends them with ONE device-scope atomicAdd whenever more than a
// tile's worth is held, and at its end: with uniform keys that is one atomic a workgroup.  (One atomic per wave and tile was measured
// first: 2^18 adds to one address took 1.9 ms of a 3.0 ms call at 2^28 keys, 7 ns each, one after the other.)
template<typename K>
__global__ __launch_bounds__(kTopkThreads) void topk_collect_kernel(TopkArgs<K> a, TopkState* __restrict__ state, K* __restrict__ cand,
                                                                    uint32_t capacity)
{
    using C = TileCfg<sizeof(K), kTopkPacks>;
    constexpr uint32_t ROOM = 2u * C::TILE;
    __shared__ K held[ROOM];
    __shared__ uint32_t fill, base;
    if (state->path != (uint32_t) TOPK_PATH_CANDIDATES) return; // (workgroup-uniform)
    const K prefix = (K) state->prefix, mask = (K) state->mask;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // held[0 .. n) to the candidate buffer; every thread calls it with the same n, behind a barrier
    const auto flush = [&](uint32_t n) {
        if (threadIdx.x == 0)
        {
            base = atomicAdd(&state->cand, n);
            fill = 0u;
        }
        __syncthreads();
        const uint32_t at = base;
        for (uint32_t i = threadIdx.x; i < n; i += kTopkThreads)
            if (at + i < capacity) cand[at + i] = held[i]; // (the bucket fits by the choice of the path; held once more in front of the store)
        __syncthreads();
    };
    if (threadIdx.x == 0) fill = 0u;
    for (uint32_t t = blockIdx.x; t < a.keys.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        __syncthreads(); // the candidates of the tiles before are held
        const uint32_t have = fill;
        __syncthreads(); // (every wave has read `fill` before one adds to it again)
        if (have > C::TILE) flush(have); // (workgroup-uniform) room for this tile: at most TILE are held afterwards
        const uint64_t first = (uint64_t) t * C::TILE + wave * C::WAVE_ELEMS + lane * C::VEC;
        K c[C::PACKS * C::VEC];
        uint32_t f = 0;
#pragma unroll
        for (uint32_t g = 0; g < C::PACKS; g++)
            tile_load_pack<C::VEC>(a.keys, first + g * C::PACK_STRIDE, [&](uint32_t e, K x, bool inside) {
                c[g * C::VEC + e] = a.code.encode(x);
                f |= (inside && (c[g * C::VEC + e] & mask) == prefix ? 1u : 0u) << (g * C::VEC + e);
            });
        if (__ballot(f != 0u) == 0) continue; // (wave-uniform) no candidate in this wave's part of the tile
        uint32_t total;
        const uint32_t below = wave_exclusive_sum((uint32_t) __popc(f), lane, total);
        uint32_t slot = 0;
        if (lane == 0) slot = atomicAdd(&fill, total); // (LDS)
        uint32_t at = (uint32_t) __builtin_amdgcn_readfirstlane((int) slot) + below;
#pragma unroll
        for (uint32_t e = 0; e < C::PACKS * C::VEC; e++)
            if ((f >> e) & 1u)
            {
                if (at < ROOM) held[at] = c[e]; // (at most TILE held + TILE of this tile)
                at++;
            }
    }
    __syncthreads();
    const uint32_t have = fill;
    __syncthreads();
    if (have) flush(have); // (workgroup-uniform)
}

// CANDIDATES: one workgroup runs every remaining round over the candidates, which come from L2 or the Infinity Cache, and stores the
// k-th key.  A wave whose candidates of a step share one digit adds their number once.
template<typename K>
__global__ __launch_bounds__(kTopkPickThreads) void topk_cand_rounds_kernel(const K* __restrict__ cand, uint32_t capacity, TopkCode<K> code,
                                                                            TopkState* __restrict__ state, K* __restrict__ out_kth)
{
    __shared__ uint32_t table[kTopkBins];
    __shared__ uint32_t wave_sums[kTopkPickThreads / 64], result[3];
    __shared__ TopkState s;
    if (state->path != (uint32_t) TOPK_PATH_CANDIDATES) return; // (workgroup-uniform)
    if (threadIdx.x == 0) s = *state;
    __syncthreads();
    constexpr uint32_t LOADS = 8;
    const uint32_t n = s.cand < capacity ? s.cand : capacity;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t round = 1; round < topk_rounds(sizeof(K)); round++)
    {
        const K prefix = (K) s.prefix, mask = (K) s.mask;
        const uint32_t need = s.need, shift = topk_shift(sizeof(K), round), bits = topk_bits(sizeof(K), round);
        table[2u * threadIdx.x] = table[2u * threadIdx.x + 1u] = 0u;
        if (threadIdx.x == 0) result[0] = result[1] = result[2] = 0u;
        __syncthreads();
        for (uint32_t i0 = 0; i0 < n; i0 += LOADS * kTopkPickThreads) // (workgroup-uniform: whole waves reach the ballots)
        {
            K c[LOADS]; // (all loads of a step in flight before the first is counted: one workgroup hides latency by itself)
#pragma unroll
            for (uint32_t u = 0; u < LOADS; u++)
            {
                const uint32_t i = i0 + u * kTopkPickThreads + threadIdx.x;
                c[u] = i < n ? cand[i] : (K) 0;
            }
#pragma unroll
            for (uint32_t u = 0; u < LOADS; u++)
            {
                const bool counted = i0 + u * kTopkPickThreads + threadIdx.x < n && (c[u] & mask) == prefix;
                const uint32_t d = topk_digit(c[u], shift, bits);
                const uint64_t lanes = __ballot(counted);
                if (lanes != 0) // (wave-uniform)
                {
                    const uint32_t first = (uint32_t) __builtin_amdgcn_readlane((int) d, (int) __builtin_ctzll(lanes));
                    if (__ballot(counted && d != first) == 0)
                    {
                        if (lane == 0) atomicAdd(&table[first], (uint32_t) __popcll(lanes));
                    }
                    else if (counted)
                        atomicAdd(&table[d], 1u);
                }
            }
        }
        __syncthreads();
        topk_block_pick(table[2u * threadIdx.x], table[2u * threadIdx.x + 1u], need, wave_sums, result);
        if (threadIdx.x == 0) topk_advance(s, sizeof(K), round, result[0], result[1], result[2]);
        __syncthreads();
    }
    if (threadIdx.x == 0)
    {
        *state = s;
        if (out_kth) *out_kth = code.decode((K) s.prefix);
    }
}

// The code words of the calling lane's elements of a tile and two flag words: below the threshold word, equal to it.  Elements outside
// the array have neither flag.
template<typename K>
__device__ __forceinline__ void topk_flags(const TopkArgs<K>& a, uint64_t first, K threshold, K (&x)[kTopkPacks * (16 / sizeof(K))], uint32_t& less,
                                           uint32_t& equal)
{
    using C = TileCfg<sizeof(K), kTopkPacks>;
    less = equal = 0;
#pragma unroll
    for (uint32_t g = 0; g < C::PACKS; g++)
        tile_load_pack<C::VEC>(a.keys, first + g * C::PACK_STRIDE, [&](uint32_t e, K v, bool inside) {
            const K c = a.code.encode(v);
            x[g * C::VEC + e] = v;
            less |= (inside && c < threshold ? 1u : 0u) << (g * C::VEC + e);
            equal |= (inside && c == threshold ? 1u : 0u) << (g * C::VEC + e);
        });
}

template<typename K>
__global__ __launch_bounds__(kTopkThreads) void topk_flag_count_kernel(TopkArgs<K> a, const TopkState* __restrict__ state,
                                                                       uint32_t* __restrict__ less_counts, uint32_t* __restrict__ tie_counts)
{
    using C = TileCfg<sizeof(K), kTopkPacks>;
    const K threshold = (K) state->prefix;
    TileWalk<C> w; // (one walk, two counts a tile: each takes the other row of LDS than the one before, and a barrier)
    for (uint32_t t = blockIdx.x; t < a.keys.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        K x[C::PACKS * C::VEC];
        uint32_t less, equal;
        topk_flags(a, w.first(t), threshold, x, less, equal);
        tile_count(w, t, less, less_counts);
        tile_count(w, t, equal, tie_counts);
    }
}

// SORTED: (code word, index) pairs into pair_codes / pair_indices; else the keys bit for bit and the indices into the caller's arrays
// (either may be NULL).  The two flag sets of a tile are ranked here, side by side, with one barrier a tile (tile_compact ranks one).
// The scanned counts say which tiles hold an element that is taken; the others are skipped unread: for a small k nearly all of them.
template<typename K, bool SORTED>
__global__ __launch_bounds__(kTopkThreads) void topk_write_kernel(TopkArgs<K> a, const TopkState* __restrict__ state,
                                                                  const uint32_t* __restrict__ less_counts, const uint32_t* __restrict__ tie_counts,
                                                                  uint32_t k, K* __restrict__ out_keys, uint32_t* __restrict__ out_indices)
{
    using C = TileCfg<sizeof(K), kTopkPacks>;
    __shared__ uint32_t wsum[2][kTileWaves][2];
    const K threshold = (K) state->prefix;
    const uint32_t need = state->need;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t phase = 0;
    for (uint32_t t = blockIdx.x; t < a.keys.tiles; t += gridDim.x) // (workgroup-uniform)
    {
        // a tile of which nothing is taken is not read: no key below the threshold, and no tie or `need` ties in front of it already
        const bool last = t + 1u == a.keys.tiles;
        const uint32_t ties_in_front = tie_counts[t];
        const uint32_t tile_less = (last ? state->totals[0] : less_counts[t + 1u]) - less_counts[t];
        const uint32_t tile_ties = (last ? state->totals[1] : tie_counts[t + 1u]) - ties_in_front;
        if (tile_less == 0u && (tile_ties == 0u || ties_in_front >= need)) continue; // (workgroup-uniform)
        const uint64_t first = (uint64_t) t * C::TILE + wave * C::WAVE_ELEMS + lane * C::VEC;
        K x[C::PACKS * C::VEC];
        uint32_t less, equal;
        topk_flags(a, first, threshold, x, less, equal);
        uint32_t less_below[C::PACKS], ties_below[C::PACKS]; // flags of the wave in front of the lane's pack g
        uint32_t wave_less = 0, wave_ties = 0;
#pragma unroll
        for (uint32_t g = 0; g < C::PACKS; g++)
        {
            uint32_t mine_l = 0, all_l = 0, mine_e = 0, all_e = 0;
#pragma unroll
            for (uint32_t e = 0; e < C::VEC; e++)
            {
                const uint64_t bl = __ballot((less >> (g * C::VEC + e)) & 1u), be = __ballot((equal >> (g * C::VEC + e)) & 1u);
                mine_l += __builtin_amdgcn_mbcnt_hi((uint32_t) (bl >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) bl, 0u));
                mine_e += __builtin_amdgcn_mbcnt_hi((uint32_t) (be >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) be, 0u));
                all_l += (uint32_t) __popcll(bl);
                all_e += (uint32_t) __popcll(be);
            }
            less_below[g] = wave_less + mine_l;
            ties_below[g] = wave_ties + mine_e;
            wave_less += all_l;
            wave_ties += all_e;
        }
        uint32_t(*row)[2] = wsum[phase++ & 1u]; // (the other row than the tile before: one barrier a tile)
        if (lane == 0)
        {
            row[wave][0] = wave_less;
            row[wave][1] = wave_ties;
        }
        __syncthreads();
        uint32_t base_less = less_counts[t], base_ties = tie_counts[t];
#pragma unroll
        for (uint32_t i = 0; i < kTileWaves; i++)
            if (i < wave)
            {
                base_less += row[i][0];
                base_ties += row[i][1];
            }
        const uint32_t i0 = (uint32_t) (first - a.keys.lo); // the lane's pack 0 as an element of the array (modulo 2^32 in front of it)
#pragma unroll
        for (uint32_t g = 0; g < C::PACKS; g++)
        {
            uint32_t before_less = base_less + less_below[g], before_ties = base_ties + ties_below[g];
#pragma unroll
            for (uint32_t e = 0; e < C::VEC; e++)
            {
                const uint32_t bit = g * C::VEC + e;
                const bool is_less = (less >> bit) & 1u, is_tie = (equal >> bit) & 1u;
                // the elements in front that are taken: every one below the threshold and the first `need` equal to it
                const uint32_t rank = before_less + (before_ties < need ? before_ties : need);
                if ((is_less || (is_tie && before_ties < need)) && rank < k)
                {
                    if (out_keys) out_keys[rank] = SORTED ? a.code.encode(x[bit]) : x[bit];
                    if (out_indices) out_indices[rank] = i0 + g * C::PACK_STRIDE + e;
                }
                before_less += is_less ? 1u : 0u;
                before_ties += is_tie ? 1u : 0u;
            }
        }
    }
}

// the ordered pairs as keys and indices (either output may be NULL)
constexpr uint32_t kTopkDecodeThreads = 256;
template<typename K>
__global__ __launch_bounds__(kTopkDecodeThreads) void topk_decode_kernel(const K* __restrict__ pair_codes, const uint32_t* __restrict__ pair_indices,
                                                                         uint32_t k, TopkCode<K> code, K* __restrict__ out_keys,
                                                                         uint32_t* __restrict__ out_indices)
{
    const uint32_t r = blockIdx.x * kTopkDecodeThreads + threadIdx.x;
    if (r >= k) return;
    if (out_keys) out_keys[r] = code.decode(pair_codes[r]);
    if (out_indices) out_indices[r] = pair_indices[r];
}

} // namespace glu_hip
