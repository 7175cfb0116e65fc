// topk_batch_kernels.hpp -- gfx950 kernels of BATCHED TOP-K (glu_top_k_run_batch_ptr / _batch_offsets_ptr): the k best keys of every
// segment of an array, each segment under the contract of glu_top_k_run_ptr with k_s = min(k, its length).  Not in the reference.
//
// Every class works on code words c = KeyCodec::encode(key), complemented for `largest`: "the k_s smallest unsigned words" is the
// only case.  The arithmetic of a select is topk_pick.hpp's (topk_crosses, topk_advance) and topk_batch_plan.hpp's (the same at the
// wave class's digit width).  Three classes, each a kernel that walks a LIST of segments with a grid sized to the device:
//   wave   topk_batch_wave_kernel    1 .. 512 keys: one WAVE per segment, four to the workgroup, no workgroup barrier.  A lane holds 8
//                                    consecutive keys in registers (lane order is index order); 8-bit rounds on a wave-private row of
//                                    256 counters in LDS; the ranks of the compaction are two wave scans of the lanes' flag counts.
//   block  topk_batch_block_kernel   up to a tile of 8 / 32 / 128 KiB of code words: one WORKGROUP per segment reads it ONCE into LDS
//                                    (whole 16-byte packs from the boundary at or below the segment, the ends masked), runs all 11-bit
//                                    rounds on a table of 2048 counters in LDS, then flags, ranks and writes in index order.
//   long   topk_batch_long_kernel    any length: one workgroup per segment streams the keys.  Round 1 counts over the segment; where the
//                                    threshold's bucket fits the candidate buffer in LDS one more read collects it and the remaining
//                                    rounds run in LDS, else every remaining round reads the segment again, filtered by the prefix
//                                    (decided in the kernel).  The compaction goes tile after tile with running carries.
// topk_batch_bin_kernel in front (device offsets only) appends every non-empty segment to the list of its class: THE ONLY ATOMICS ON
// DEVICE MEMORY, and the order of a list does not matter.  (The tables and the candidate buffer are LDS; only counts are taken from
// them, and integer counts commute.)  Everything a caller sees is written at ranks that follow from counts: same input, same bits.
// A segment is [offsets[s], offsets[s + 1]), and one whose end lies below its begin or beyond `total` is EMPTY to every kernel here
// (batch_offsets_segment).  Outputs are rows of stride k; out_indices are local to the segment.
#pragma once

#include "batch_lists.hpp"
#include "radix_sort_kernels.hpp"
#include "topk_batch_plan.hpp"

namespace glu_hip
{
// the key of a call as a code word and back (topk_kernels.hpp's TopkCode; that header defines the single call's kernels)
template<typename K>
struct TopkBatchCode
{
    uint32_t xf;      // KEY_XF_*
    uint32_t largest; // != 0: the code is complemented
    __device__ __forceinline__ K flip() const { return largest ? (K) ~(K) 0 : (K) 0; }
    __device__ __forceinline__ K encode(K key) const { return KeyCodec<K>(xf).encode(key) ^ flip(); }
    __device__ __forceinline__ K decode(K code) const { return KeyCodec<K>(xf).decode(code ^ flip()); }
};

// What a call passes to its class kernels.  K: the keys as unsigned words of their width.
template<typename K>
struct TopkBatchArgs
{
    const K* keys;
    const uint32_t* offsets;    // device, or NULL: equal partitions of `count` keys
    uint32_t count, total;
    const uint32_t* list;       // NULL: the segments 0 .. nsegs - 1 themselves; else list[0 .. min(*list_count, nsegs))
    const uint32_t* list_count;
    uint32_t nsegs;
    TopkBatchCode<K> code;
    uint32_t k;
    uint32_t pairs;             // != 0 (the sorted stage): out_keys receives CODE WORDS and the entries [k_s, k) of a row all-ones pads
    K* out_keys;                // rows of stride k; each may be NULL
    uint32_t* out_indices;
    K* out_kth;                 // one key per segment
};

template<typename K>
__device__ __forceinline__ void topk_batch_segment(const TopkBatchArgs<K>& a, uint32_t seg, uint32_t& begin, uint32_t& len)
{
    if (a.offsets) batch_offsets_segment(a.offsets, a.total, seg, begin, len);
    else
    {
        begin = seg * a.count; // (the host checked count x partitions against 2^32)
        len = a.count;
    }
}

template<typename K>
__device__ __forceinline__ uint32_t topk_batch_list_length(const TopkBatchArgs<K>& a)
{
    return a.list_count ? batch_list_length(*a.list_count, a.nsegs) : a.nsegs;
}

template<typename K>
__device__ __forceinline__ void topk_batch_emit(const TopkBatchArgs<K>& a, size_t row, uint32_t rank, K code, uint32_t index)
{
    if (a.out_keys) a.out_keys[row + rank] = a.pairs ? code : a.code.decode(code);
    if (a.out_indices) a.out_indices[row + rank] = index;
}

// the sorted stage: the entries [k_s, k) of a row become all-ones codes, which the stable sort keeps behind every real entry
template<typename K>
__device__ __forceinline__ void topk_batch_pad(const TopkBatchArgs<K>& a, size_t row, uint32_t k_s, uint32_t thread, uint32_t threads)
{
    if (!a.pairs) return;
    for (uint32_t j = k_s + thread; j < a.k; j += threads)
    {
        a.out_keys[row + j] = (K) ~(K) 0;
        a.out_indices[row + j] = j;
    }
}

// keeps the COMPILER from moving LDS accesses across the points where one lane of a wave reads what another wrote (the lanes run in
// lockstep and the LDS serves a wave's accesses in order)
__device__ __forceinline__ void topk_batch_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------------------
// Binning (device offsets): list c receives the segments of class c.  Empty segments are in no list.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_batch_bin_kernel(const uint32_t* __restrict__ offsets, uint32_t nsegs, uint32_t total,
                                                             BatchListsLayout layout, uint32_t* __restrict__ counts,
                                                             uint32_t* __restrict__ lists)
{
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * 256u; base < nsegs; base += gridDim.x * 256u)
    {
        const uint32_t seg = base + threadIdx.x;
        int cls = -1;
        if (seg < nsegs)
        {
            uint32_t begin, len;
            batch_offsets_segment(offsets, total, seg, begin, len);
            if (len >= 1u)
            {
                cls = BATCH_LIST_LONG;
#pragma unroll
                for (int c = BATCH_LIST_BLOCK; c >= 0; c--)
                    if (len <= layout.limit[c]) cls = c;
            }
        }
        batch_append<kTopkBatchLists>(cls, seg, lane, layout, counts, lists);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Wave per segment.
// ---------------------------------------------------------------------------------------------------------
template<typename K>
__global__ __launch_bounds__(kTopkBatchWaveWaves * 64) void topk_batch_wave_kernel(TopkBatchArgs<K> a)
{
    constexpr uint32_t KPT = kTopkBatchWaveKpt, W = kTopkBatchWaveDigitBits, BINS = 1u << W, ROUNDS = (uint32_t) sizeof(K) * 8u / W;
    static_assert(BINS == 4u * 64u && (sizeof(K) * 8u) % W == 0, "a lane scans four counters of the row; every round takes a whole digit");
    __shared__ __align__(16) uint32_t cnt[kTopkBatchWaveWaves][BINS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* const row = cnt[wave];
    uint4* const row4 = reinterpret_cast<uint4*>(row);
    const uint32_t n_list = topk_batch_list_length(a);
    const bool arrays = a.out_keys || a.out_indices;

    for (uint32_t li = blockIdx.x * kTopkBatchWaveWaves + wave; li < n_list; li += gridDim.x * kTopkBatchWaveWaves)
    {
        const uint32_t seg = a.list ? a.list[li] : li;
        uint32_t begin, len;
        topk_batch_segment(a, seg, begin, len);
        if (len == 0u || len > kTopkBatchWaveTile) continue; // (wave-uniform)
        const uint32_t k_s = a.k < len ? a.k : len;
        const K* const src = a.keys + begin;
        K c[KPT];
        uint32_t valid = 0;
#pragma unroll
        for (uint32_t i = 0; i < KPT; i++)
        {
            const uint32_t p = lane * KPT + i;
            const bool ok = p < len;
            c[i] = ok ? a.code.encode(src[p]) : (K) ~(K) 0;
            valid |= (ok ? 1u : 0u) << i;
        }
        TopkState s = topk_begin(len, k_s); // (wave-uniform)
        for (uint32_t r = 0; r < ROUNDS; r++)
        {
            const uint32_t shift = topk_shift_w(sizeof(K), W, r);
            const K prefix = (K) s.prefix, mask = (K) s.mask;
            row4[lane] = make_uint4(0u, 0u, 0u, 0u);
            topk_batch_wave_sync();
#pragma unroll
            for (uint32_t i = 0; i < KPT; i++)
                if (((valid >> i) & 1u) && (c[i] & mask) == prefix) atomicAdd(&row[topk_digit(c[i], shift, W)], 1u); // (LDS)
            topk_batch_wave_sync();
            const uint4 t = row4[lane];
            uint32_t all;
            uint32_t before = wave_exclusive_sum(t.x + t.y + t.z + t.w, lane, all);
            // the one counter of the row at which the cumulative count reaches `need`
            uint32_t d = 0, front = 0, in_it = 0;
            bool hit = false;
            const uint32_t four[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
            {
                if (topk_crosses(before, four[j], s.need))
                {
                    hit = true;
                    d = 4u * lane + j;
                    front = before;
                    in_it = four[j];
                }
                before += four[j];
            }
            const uint64_t m = __ballot(hit);
            const int from = m ? (int) __builtin_ctzll(m) : 0;
            d = (uint32_t) __shfl((int) d, from);
            front = (uint32_t) __shfl((int) front, from);
            in_it = (uint32_t) __shfl((int) in_it, from);
            topk_advance_w(s, sizeof(K), W, r, d, front, in_it);
            topk_batch_wave_sync(); // (the row is read before a lane clears it again)
        }
        const K threshold = (K) s.prefix;
        if (a.out_kth && lane == 0) a.out_kth[seg] = a.code.decode(threshold);
        if (!arrays) continue; // (wave-uniform)
        const size_t out_row = (size_t) seg * a.k;
        uint32_t less = 0, equal = 0;
#pragma unroll
        for (uint32_t i = 0; i < KPT; i++)
        {
            const bool ok = (valid >> i) & 1u;
            less |= (ok && c[i] < threshold ? 1u : 0u) << i;
            equal |= (ok && c[i] == threshold ? 1u : 0u) << i;
        }
        uint32_t all;
        uint32_t before_less = wave_exclusive_sum((uint32_t) __popc(less), lane, all);
        uint32_t before_ties = wave_exclusive_sum((uint32_t) __popc(equal), lane, all);
#pragma unroll
        for (uint32_t i = 0; i < KPT; i++)
        {
            const bool is_less = (less >> i) & 1u, is_tie = (equal >> i) & 1u;
            // the elements in front that are taken: every one below the threshold and the first `need` equal to it
            const uint32_t rank = before_less + (before_ties < s.need ? before_ties : s.need);
            if ((is_less || (is_tie && before_ties < s.need)) && rank < k_s) topk_batch_emit(a, out_row, rank, c[i], lane * KPT + i);
            before_less += is_less ? 1u : 0u;
            before_ties += is_tie ? 1u : 0u;
        }
        topk_batch_pad(a, out_row, k_s, lane, 64u);
    }
}

// ---------------------------------------------------------------------------------------------------------
// What the workgroup classes share: a round over a source of code words, the pick, the compaction over a source.
// ---------------------------------------------------------------------------------------------------------
template<int THREADS>
struct TopkBatchShared
{
    static constexpr int WAVES = THREADS / 64;
    uint32_t table[kTopkBins];
    uint32_t wave_sums[WAVES];
    uint32_t result[2][4];       // the pick of a round, by the round's parity: digit, words in front of it, words in it
    uint32_t wsum[2][WAVES][2];  // the compaction's wave totals (less, ties), by the tile's parity
    uint32_t fill;               // candidates held (the long class)
};

// The crossing digit of sh.table by the THREADS threads of a workgroup, thread t holding the counters [t * PER, (t + 1) * PER).
// Ends with a barrier.
template<int THREADS>
__device__ __forceinline__ void topk_batch_pick(TopkBatchShared<THREADS>& sh, uint32_t need, uint32_t* result)
{
    constexpr uint32_t PER = kTopkBins / THREADS;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++)
    {
        c[j] = sh.table[threadIdx.x * PER + j];
        sum += c[j];
    }
    uint32_t total;
    uint32_t before = wave_exclusive_sum(sum, lane, total);
    if (lane == 0) sh.wave_sums[wave] = total;
    __syncthreads();
    before += sum_of_preceding_waves(sh.wave_sums, TopkBatchShared<THREADS>::WAVES, wave, lane);
#pragma unroll
    for (uint32_t j = 0; j < PER; j++)
    {
        if (topk_crosses(before, c[j], need))
        {
            result[0] = threadIdx.x * PER + j;
            result[1] = before;
            result[2] = c[j];
        }
        before += c[j];
    }
    __syncthreads();
}

// Round `round` (11-bit digits) over the code words fetch(0 .. n) that match the prefix.  `s` is workgroup-uniform, in registers.
template<typename K, int THREADS, typename Fetch>
__device__ __forceinline__ void topk_batch_round(Fetch fetch, uint32_t n, TopkState& s, uint32_t round, TopkBatchShared<THREADS>& sh)
{
    const uint32_t shift = topk_shift(sizeof(K), round), bits = topk_bits(sizeof(K), round);
    const K prefix = (K) s.prefix, mask = (K) s.mask;
    uint32_t* const result = sh.result[round & 1u]; // (the other one than the round before: no barrier between its readers and this)
    for (uint32_t b = threadIdx.x; b < kTopkBins; b += THREADS) sh.table[b] = 0u;
    if (threadIdx.x == 0) result[0] = result[1] = result[2] = 0u;
    __syncthreads();
#pragma unroll 4
    for (uint64_t i = threadIdx.x; i < n; i += THREADS)
    {
        const K c = fetch((uint32_t) i);
        if ((c & mask) == prefix) atomicAdd(&sh.table[topk_digit(c, shift, bits)], 1u); // (LDS)
    }
    __syncthreads();
    topk_batch_pick<THREADS>(sh, s.need, result);
    topk_advance(s, sizeof(K), round, result[0], result[1], result[2]);
}

// Every code word of fetch(0 .. n) below `threshold` and the first `need` equal to it, to row `row` of the outputs at the rank
// less_before + min(ties_before, need): ascending indices, exactly k_s of them.  Tile after tile (a thread takes 4 consecutive
// words), one barrier a tile, the carries running in registers; ends at the tile behind which nothing is taken any more.
template<typename K, int THREADS, typename Fetch>
__device__ __forceinline__ void topk_batch_compact(Fetch fetch, uint32_t n, K threshold, uint32_t need, uint32_t k_s, const TopkBatchArgs<K>& a,
                                                   size_t row, TopkBatchShared<THREADS>& sh)
{
    constexpr uint32_t VPT = 4, TILE = THREADS * VPT;
    constexpr int WAVES = TopkBatchShared<THREADS>::WAVES;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry_less = 0, carry_ties = 0, phase = 0;
    for (uint64_t base = 0; base < n; base += TILE) // (workgroup-uniform)
    {
        if (carry_less + (carry_ties < need ? carry_ties : need) >= k_s) break; // (workgroup-uniform) all k_s are written
        const uint64_t i0 = base + threadIdx.x * VPT;
        K c[VPT];
        uint32_t less = 0, equal = 0;
#pragma unroll
        for (uint32_t e = 0; e < VPT; e++)
        {
            const bool ok = i0 + e < n;
            c[e] = ok ? fetch((uint32_t) (i0 + e)) : (K) 0;
            less |= (ok && c[e] < threshold ? 1u : 0u) << e;
            equal |= (ok && c[e] == threshold ? 1u : 0u) << e;
        }
        uint32_t wave_less, wave_ties;
        uint32_t before_less = wave_exclusive_sum((uint32_t) __popc(less), lane, wave_less);
        uint32_t before_ties = wave_exclusive_sum((uint32_t) __popc(equal), lane, wave_ties);
        uint32_t(*w)[2] = sh.wsum[phase++ & 1u]; // (the other rows than the tile before: one barrier a tile)
        if (lane == 0)
        {
            w[wave][0] = wave_less;
            w[wave][1] = wave_ties;
        }
        __syncthreads();
        uint32_t tile_less = 0, tile_ties = 0;
#pragma unroll
        for (int i = 0; i < WAVES; i++)
        {
            const uint32_t l = w[i][0], t = w[i][1];
            if (i < (int) wave)
            {
                before_less += l;
                before_ties += t;
            }
            tile_less += l;
            tile_ties += t;
        }
        before_less += carry_less;
        before_ties += carry_ties;
#pragma unroll
        for (uint32_t e = 0; e < VPT; e++)
        {
            const bool is_less = (less >> e) & 1u, is_tie = (equal >> e) & 1u;
            const uint32_t rank = before_less + (before_ties < need ? before_ties : need);
            if ((is_less || (is_tie && before_ties < need)) && rank < k_s) topk_batch_emit(a, row, rank, c[e], (uint32_t) (i0 + e));
            before_less += is_less ? 1u : 0u;
            before_ties += is_tie ? 1u : 0u;
        }
        carry_less += tile_less;
        carry_ties += tile_ties;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Workgroup per segment, the segment's code words in LDS (TILE of them at the most).  Dynamic LDS: the code words, then
// TopkBatchShared.
// ---------------------------------------------------------------------------------------------------------
template<typename K, int THREADS, int TILE>
constexpr size_t topk_batch_block_lds() { return (size_t) TILE * sizeof(K) + sizeof(TopkBatchShared<THREADS>); }

template<typename K, int THREADS, int TILE>
__global__ __launch_bounds__(THREADS) void topk_batch_block_kernel(TopkBatchArgs<K> a)
{
    extern __shared__ __align__(16) unsigned char topk_batch_lds[];
    K* const codes = reinterpret_cast<K*>(topk_batch_lds);
    TopkBatchShared<THREADS>& sh = *reinterpret_cast<TopkBatchShared<THREADS>*>(topk_batch_lds + (size_t) TILE * sizeof(K));
    constexpr uint32_t VEC = 16 / sizeof(K);
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    const uint32_t n_list = topk_batch_list_length(a);
    const bool arrays = a.out_keys || a.out_indices;

    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) // (workgroup-uniform)
    {
        const uint32_t seg = a.list ? a.list[li] : li;
        uint32_t begin, len;
        topk_batch_segment(a, seg, begin, len);
        if (len == 0u || len > (uint32_t) TILE) continue; // (workgroup-uniform)
        const uint32_t k_s = a.k < len ? a.k : len;
        // the segment, once: whole 16-byte packs from the boundary at or below it, what lies in front of it and behind it masked
        const K* const src = a.keys + begin;
        const uint32_t lead = (uint32_t) (reinterpret_cast<uintptr_t>(src) & 15u) / (uint32_t) sizeof(K);
        const u32x4_t* const packs = reinterpret_cast<const u32x4_t*>(src - lead);
        const uint32_t n_packs = (lead + len + VEC - 1u) / VEC;
        for (uint32_t p = threadIdx.x; p < n_packs; p += THREADS)
        {
            const u32x4_t raw = packs[p];
            K x[VEC];
            __builtin_memcpy(x, &raw, 16);
#pragma unroll
            for (uint32_t e = 0; e < VEC; e++)
            {
                const uint32_t at = p * VEC + e - lead; // (below `lead`: wraps beyond len)
                if (at < len) codes[at] = a.code.encode(x[e]);
            }
        }
        __syncthreads();
        const auto from_lds = [&](uint32_t i) { return codes[i]; };
        TopkState s = topk_begin(len, k_s); // (workgroup-uniform)
        for (uint32_t r = 0; r < topk_rounds(sizeof(K)); r++) topk_batch_round<K, THREADS>(from_lds, len, s, r, sh);
        const K threshold = (K) s.prefix;
        if (a.out_kth && threadIdx.x == 0) a.out_kth[seg] = a.code.decode(threshold);
        if (arrays)
        {
            const size_t row = (size_t) seg * a.k;
            topk_batch_compact<K, THREADS>(from_lds, len, threshold, s.need, k_s, a, row, sh);
            topk_batch_pad(a, row, k_s, threadIdx.x, THREADS);
        }
        __syncthreads(); // (the next segment overwrites the code words)
    }
}

// ---------------------------------------------------------------------------------------------------------
// Workgroup per segment of any length, streaming.
// ---------------------------------------------------------------------------------------------------------
template<typename K>
__global__ __launch_bounds__(kTopkBatchLongThreads) void topk_batch_long_kernel(TopkBatchArgs<K> a)
{
    constexpr int THREADS = (int) kTopkBatchLongThreads;
    constexpr uint32_t ROOM = kTopkBatchCandBytes / sizeof(K);
    __shared__ K cand[ROOM];
    __shared__ TopkBatchShared<THREADS> sh;
    const uint32_t n_list = topk_batch_list_length(a);
    const bool arrays = a.out_keys || a.out_indices;

    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) // (workgroup-uniform)
    {
        const uint32_t seg = a.list ? a.list[li] : li;
        uint32_t begin, len;
        topk_batch_segment(a, seg, begin, len);
        if (len == 0u) continue; // (workgroup-uniform)
        const uint32_t k_s = a.k < len ? a.k : len;
        const K* const src = a.keys + begin;
        const auto from_input = [&](uint32_t i) { return a.code.encode(src[i]); };
        TopkState s = topk_begin(len, k_s); // (workgroup-uniform)
        topk_batch_round<K, THREADS>(from_input, len, s, 0, sh);
        if (s.bucket <= ROOM) // (workgroup-uniform) the candidates: one more read, the remaining rounds in LDS
        {
            if (threadIdx.x == 0) sh.fill = 0u;
            __syncthreads();
            const K prefix = (K) s.prefix, mask = (K) s.mask;
#pragma unroll 4
            for (uint64_t i = threadIdx.x; i < len; i += THREADS)
            {
                const K c = from_input((uint32_t) i);
                if ((c & mask) == prefix)
                {
                    const uint32_t at = atomicAdd(&sh.fill, 1u); // (LDS; any order: only counts are taken from the candidates)
                    if (at < ROOM) cand[at] = c;
                }
            }
            __syncthreads();
            const uint32_t held = s.bucket;
            const auto from_cand = [&](uint32_t i) { return cand[i]; };
            for (uint32_t r = 1; r < topk_rounds(sizeof(K)); r++) topk_batch_round<K, THREADS>(from_cand, held, s, r, sh);
        }
        else
            for (uint32_t r = 1; r < topk_rounds(sizeof(K)); r++) topk_batch_round<K, THREADS>(from_input, len, s, r, sh);
        const K threshold = (K) s.prefix;
        if (a.out_kth && threadIdx.x == 0) a.out_kth[seg] = a.code.decode(threshold);
        if (arrays)
        {
            const size_t row = (size_t) seg * a.k;
            topk_batch_compact<K, THREADS>(from_input, len, threshold, s.need, k_s, a, row, sh);
            topk_batch_pad(a, row, k_s, threadIdx.x, THREADS);
        }
        __syncthreads(); // (the next segment's first round clears the table and the candidates)
    }
}

// ---------------------------------------------------------------------------------------------------------
// The sorted stage's last kernel: entry j < k_s of every ordered row of pairs, decoded into the outputs (either may be NULL).
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kTopkBatchDecodeThreads = 256;
template<typename K>
__global__ __launch_bounds__(kTopkBatchDecodeThreads) void topk_batch_decode_kernel(const K* __restrict__ pair_codes,
                                                                                   const uint32_t* __restrict__ pair_indices,
                                                                                   TopkBatchArgs<K> a, K* __restrict__ out_keys,
                                                                                   uint32_t* __restrict__ out_indices)
{
    const uint64_t entries = (uint64_t) a.nsegs * a.k; // (below 2^32: the host)
    for (uint64_t at = (uint64_t) blockIdx.x * kTopkBatchDecodeThreads + threadIdx.x; at < entries; at += (uint64_t) gridDim.x * kTopkBatchDecodeThreads)
    {
        const uint32_t seg = (uint32_t) (at / a.k), j = (uint32_t) (at - (uint64_t) seg * a.k);
        uint32_t begin, len;
        topk_batch_segment(a, seg, begin, len);
        if (j >= len) continue; // (j < k: below k_s)
        if (out_keys) out_keys[at] = a.code.decode(pair_codes[at]);
        if (out_indices) out_indices[at] = pair_indices[at];
    }
}

} // namespace glu_hip
