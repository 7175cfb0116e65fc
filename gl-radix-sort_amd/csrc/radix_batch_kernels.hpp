// radix_batch_kernels.hpp -- gfx950 kernels of the BATCHED radix sort (glu_radix_sort_run_batch_ptr / _batch_offsets_ptr): every
// segment of an array sorted independently, stable, ascending, in place.  Not in the reference, whose RadixSort sorts one array
// per call (glu/RadixSort.hpp:273-334) while its BlellochScan takes num_partitions (BlellochScan.hpp:130-139).
//
// Three size classes, each a kernel that walks a LIST of segment indices with a grid sized to the device:
//   wave   radix_batch_wave_kernel   2 .. 512 elements: one WAVE per segment, keys and values in registers (8 per lane), 8-bit
//                                    rounds of ballot ranking against a wave-private 256-counter row in LDS, wave-level scan of the
//                                    row, re-staging through a wave-private LDS slice.  No __syncthreads(): the waves of a workgroup
//                                    never wait for each other.
//   block  radix_batch_block_kernel  up to one LDS tile (1024 / 4096 / 16384 elements; 8-byte keys: 8192): one WORKGROUP per
//                                    segment, the body of radix_sort_single_block_kernel at a segment base with a run-time length.
//   long   radix_batch_long_kernel   any length: one workgroup per segment streams 8-bit counting passes (the reference's stable
//                                    counting pass, RadixSort.hpp:142-182, by one workgroup) between the caller's arrays and the
//                                    object's scratch arrays; an even number of passes, so the result lands in the caller's arrays.
// radix_batch_bin_kernel in front (device offsets only) writes the five lists.  The lists, their layout and the clamps are
// batch_lists.hpp's: a segment is [offsets[s], offsets[s + 1]), and one whose end lies below its begin or beyond `total` is EMPTY
// to every kernel here (batch_offsets_segment).
#pragma once

#include "batch_lists.hpp"
#include "radix_sort_kernels.hpp"

namespace glu_hip
{
constexpr int kBatchWaveKpt = 8;                                // elements per lane of the wave class
constexpr uint32_t kBatchWaveTile = kWave * kBatchWaveKpt;      // 512
constexpr int kBatchWaveWaves = 4;                              // waves (= segments in flight) per workgroup of the wave class
constexpr int kBatchLists = BATCH_LIST_LONG + 1;                // wave, block x 3 tile geometries, long: one-word entries, no chunks
constexpr int kBatchLongKpt = 4;                                // elements per thread and tile of the long class (1024 threads)

// Element range of segment `seg`.  offsets == NULL: equal partitions of `count` elements (the host checked count x partitions
// against 2^32).
__device__ __forceinline__ void batch_segment(const uint32_t* __restrict__ offsets, uint32_t count, uint32_t total, uint32_t seg,
                                              uint32_t& begin, uint32_t& len)
{
    if (offsets) batch_offsets_segment(offsets, total, seg, begin, len);
    else
    {
        begin = seg * count;
        len = count;
    }
}

// Stable rank of this lane's element among the elements of the wave that were ranked into `row` so far and share its digit `d`
// (8 bits): the wave's lanes with the same digit are found with one ballot per digit bit, the lanes below this one counted with
// v_mbcnt, the row's counter advanced by the size of the group (every lane of the group writes the same word).
__device__ __forceinline__ uint32_t batch_ballot_rank(uint32_t d, uint32_t* row)
{
    uint32_t* const cnt = row + d;
    const uint32_t prev = *cnt;
    uint32_t plo = ~0u, phi = ~0u;
#pragma unroll
    for (int bit = 0; bit < 8; bit++)
    {
        int32_t sel;
        asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(sel) : "v"(d), "n"(bit));
        const uint64_t m = __ballot(sel < 0);
        plo = __builtin_amdgcn_bitop3_b32(plo, (uint32_t) m, (uint32_t) sel, 0x90);
        phi = __builtin_amdgcn_bitop3_b32(phi, (uint32_t) (m >> 32), (uint32_t) sel, 0x90);
    }
    const uint32_t lower = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
    const uint32_t total = (uint32_t) __popc(plo) + (uint32_t) __popc(phi);
    uint32_t rank = prev + lower;
    asm volatile("" : "+v"(rank));
    *cnt = prev + total;
    return rank;
}

// The lanes of a wave run in lockstep and the LDS serves a wave's accesses in order; this only keeps the COMPILER from moving LDS
// accesses across the points where one lane reads what another lane wrote.
__device__ __forceinline__ void batch_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------------------
// Binning (device offsets): list c receives the indices of the segments of class c, its word of the count line their number
// (batch_append).  Segments of 0 or 1 elements are in no list.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void radix_batch_bin_kernel(const uint32_t* __restrict__ offsets, uint32_t nsegs, uint32_t total,
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
            if (len >= 2u)
            {
                cls = BATCH_LIST_LONG;
#pragma unroll
                for (int c = BATCH_LIST_BLOCK; c >= 0; c--)
                    if (len <= layout.limit[c]) cls = c;
            }
        }
        batch_append<kBatchLists>(cls, seg, lane, layout, counts, lists);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Wave per segment.
// ---------------------------------------------------------------------------------------------------------
template<typename KeyT, bool VALS>
struct BatchWaveSmem
{
    PairArray<KeyT, (int) kBatchWaveTile, VALS> stage[kBatchWaveWaves];
    alignas(16) uint32_t cnt[kBatchWaveWaves][256];
};

// list == NULL: the segments 0 .. nsegs - 1 themselves; else list[0 .. min(*list_count, nsegs)).  xf: KeyTransform of the keys.
template<typename KeyT, bool VALS>
__global__ __launch_bounds__(kBatchWaveWaves* kWave) void radix_batch_wave_kernel(KeyT* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                                  const uint32_t* __restrict__ offsets, uint32_t count,
                                                                                  uint32_t total, const uint32_t* __restrict__ list,
                                                                                  const uint32_t* __restrict__ list_count, uint32_t nsegs,
                                                                                  uint32_t xf)
{
    constexpr int KPT = kBatchWaveKpt;
    __shared__ BatchWaveSmem<KeyT, VALS> s;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto& stage = s.stage[wave];
    uint32_t* const row = s.cnt[wave];
    uint4* const row4 = reinterpret_cast<uint4*>(row);
    const KeyCodec<KeyT, true> codec(xf);
    const uint32_t n_list = list_count ? batch_list_length(*list_count, nsegs) : nsegs;

    for (uint32_t li = blockIdx.x * kBatchWaveWaves + wave; li < n_list; li += gridDim.x * kBatchWaveWaves)
    {
        const uint32_t seg = list ? list[li] : li;
        uint32_t begin, len;
        batch_segment(offsets, count, total, seg, begin, len);
        if (len < 2u || len > kBatchWaveTile) continue; // (wave-uniform)
        KeyT* const k = keys + begin;
        uint32_t* const v = VALS ? vals + begin : nullptr;
        const int groups = (int) ((len + 63u) >> 6); // groups of 64 elements that hold any: the others are skipped, not padded

        KeyT key[KPT];
        uint32_t val[KPT];
#pragma unroll
        for (int i = 0; i < KPT; i++)
        {
            const uint32_t p = i * kWave + lane;
            const bool ok = p < len;
            key[i] = ok ? codec.encode(k[p]) : (KeyT) ~(KeyT) 0; // pads: highest digit in every round, behind every element
            val[i] = (VALS && ok) ? v[p] : 0u;
        }

        for (uint32_t shift = 0; shift < sizeof(KeyT) * 8; shift += 8)
        {
            row4[lane] = make_uint4(0u, 0u, 0u, 0u);
            batch_wave_sync();
            uint32_t rank[KPT];
#pragma unroll
            for (int i = 0; i < KPT; i++)
                if (i < groups) rank[i] = batch_ballot_rank(digit_of<KeyT>(key[i], shift, 0xFFu), row);
            batch_wave_sync();
            {
                const uint4 c = row4[lane];
                uint32_t all;
                const uint32_t excl = wave_exclusive_sum(c.x + c.y + c.z + c.w, lane, all);
                row4[lane] = make_uint4(excl, excl + c.x, excl + c.x + c.y, excl + c.x + c.y + c.z);
            }
            batch_wave_sync();
#pragma unroll
            for (int i = 0; i < KPT; i++)
                if (i < groups) stage.put(row[digit_of<KeyT>(key[i], shift, 0xFFu)] + rank[i], key[i], val[i]);
            batch_wave_sync();
#pragma unroll
            for (int i = 0; i < KPT; i++)
                if (i < groups) stage.get(i * kWave + lane, key[i], val[i]);
            batch_wave_sync();
        }

#pragma unroll
        for (int i = 0; i < KPT; i++)
        {
            const uint32_t p = i * kWave + lane;
            if (p < len)
            {
                k[p] = codec.decode(key[i]);
                if (VALS) v[p] = val[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Workgroup per segment: radix_sort_single_block_kernel's rounds at a segment base (its own body: the existing kernel's code
// stays as it is).  Element p of the tile belongs to wave p / (64 x KPT), item (p / 64) % KPT, lane p % 64.
// ---------------------------------------------------------------------------------------------------------
template<typename KeyT, int THREADS, int KPT, bool VALS>
struct BatchBlockSmem
{
    static constexpr int WAVES = THREADS / kWave;
    static constexpr int TILE = THREADS * KPT;
    static constexpr int WCNT_STRIDE = 256 + wcnt_row_pad(WAVES);
    PairArray<KeyT, TILE, VALS> stage;
    uint32_t wcnt[WAVES][WCNT_STRIDE];
    uint32_t scan_tmp[WAVES];
};

template<typename KeyT, int THREADS, int KPT, bool VALS>
__global__ __launch_bounds__(THREADS) void radix_batch_block_kernel(KeyT* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                    const uint32_t* __restrict__ offsets, uint32_t count, uint32_t total,
                                                                    const uint32_t* __restrict__ list,
                                                                    const uint32_t* __restrict__ list_count, uint32_t nsegs, uint32_t xf)
{
    using Smem = BatchBlockSmem<KeyT, THREADS, KPT, VALS>;
    constexpr int WAVES = Smem::WAVES;
    constexpr int WAVE_TILE = kWave * KPT;
    constexpr int WQ = WAVES / 4;
    constexpr int SCAN_THREADS = 256 * WQ;
    constexpr int SCAN_WAVES = SCAN_THREADS / kWave;
    static_assert(WAVES % 4 == 0 && SCAN_THREADS <= THREADS, "offset scan geometry");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem& s = *reinterpret_cast<Smem*>(smem_raw);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wave_off = wave * WAVE_TILE + lane;
    uint32_t* const my_cnt = s.wcnt[wave];
    const KeyCodec<KeyT, true> codec(xf);
    const uint32_t n_list = list_count ? batch_list_length(*list_count, nsegs) : nsegs;

    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x)
    {
        const uint32_t seg = list ? list[li] : li;
        uint32_t begin, len;
        batch_segment(offsets, count, total, seg, begin, len);
        if (len < 2u || len > (uint32_t) Smem::TILE) continue; // (uniform over the workgroup)
        KeyT* const k = keys + begin;
        uint32_t* const v = VALS ? vals + begin : nullptr;
        // groups of 64 elements of this wave that hold any element (the others are skipped: a short segment in a large tile costs
        // the waves it reaches, not the tile)
        const uint32_t wave_first = wave * WAVE_TILE;
        const int groups = wave_first >= len ? 0 : (int) (((len - wave_first) + 63u) >> 6);

        KeyT key[KPT];
        uint32_t val[KPT];
#pragma unroll
        for (int i = 0; i < KPT; i++)
        {
            const uint32_t p = wave_off + i * kWave;
            const bool ok = p < len;
            key[i] = ok ? codec.encode(k[p]) : (KeyT) ~(KeyT) 0;
            val[i] = (VALS && ok) ? v[p] : 0u;
        }

        for (uint32_t shift = 0; shift < sizeof(KeyT) * 8; shift += 8)
        {
            for (int i = tid; i < WAVES * Smem::WCNT_STRIDE; i += THREADS) (&s.wcnt[0][0])[i] = 0;
            __syncthreads();

            uint32_t rank[KPT];
#pragma unroll
            for (int i = 0; i < KPT; i++)
                if (i < groups) rank[i] = batch_ballot_rank(digit_of<KeyT>(key[i], shift, 0xFFu), my_cnt);
            __syncthreads();

            {
                const uint32_t sd = tid / WQ, sw = (tid % WQ) * 4;
                uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
                if (tid < SCAN_THREADS)
                {
                    c0 = s.wcnt[sw + 0][sd];
                    c1 = s.wcnt[sw + 1][sd];
                    c2 = s.wcnt[sw + 2][sd];
                    c3 = s.wcnt[sw + 3][sd];
                }
                uint32_t excl = 0;
                if (wave < SCAN_WAVES)
                {
                    uint32_t wtotal;
                    excl = wave_exclusive_sum(c0 + c1 + c2 + c3, lane, wtotal);
                    if (lane == 0) s.scan_tmp[wave] = wtotal;
                }
                __syncthreads();
                excl += sum_of_preceding_waves(s.scan_tmp, SCAN_WAVES, wave < SCAN_WAVES ? wave : 0u, lane);
                if (tid < SCAN_THREADS)
                {
                    s.wcnt[sw + 0][sd] = excl;
                    s.wcnt[sw + 1][sd] = excl + c0;
                    s.wcnt[sw + 2][sd] = excl + c0 + c1;
                    s.wcnt[sw + 3][sd] = excl + c0 + c1 + c2;
                }
            }
            __syncthreads();

#pragma unroll
            for (int i = 0; i < KPT; i++)
                if (i < groups) s.stage.put(my_cnt[digit_of<KeyT>(key[i], shift, 0xFFu)] + rank[i], key[i], val[i]);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; i++)
                if (i < groups) s.stage.get(wave_off + i * kWave, key[i], val[i]);
            __syncthreads();
        }

#pragma unroll
        for (int i = 0; i < KPT; i++)
        {
            const uint32_t p = wave_off + i * kWave;
            if (p < len)
            {
                k[p] = codec.decode(key[i]);
                if (VALS) v[p] = val[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Longer segments: one workgroup per segment, 8-bit counting passes over all key bits between the caller's arrays and the scratch
// arrays (element i of the caller's arrays <-> element i of the scratch arrays).  Per pass: the segment's digit histogram
// (wave-private LDS counters), its exclusive scan (base[]), then tile after tile in order: ballot ranks inside every wave,
// the waves' counters turned into positions behind base[], a store per element, base[] advanced.  Tile order, wave order, item
// order and lane order are the element order, so every pass is stable.  A workgroup reads back only what it wrote itself.
// ---------------------------------------------------------------------------------------------------------
struct BatchLongSmem
{
    uint32_t wcnt[16][256];
    uint32_t base[256];
    uint32_t scan_tmp[4];
};

template<typename KeyT, bool VALS>
__global__ __launch_bounds__(1024) void radix_batch_long_kernel(KeyT* __restrict__ keys, uint32_t* __restrict__ vals,
                                                               KeyT* __restrict__ tmp_keys, uint32_t* __restrict__ tmp_vals,
                                                               const uint32_t* __restrict__ offsets, uint32_t total,
                                                               const uint32_t* __restrict__ list,
                                                               const uint32_t* __restrict__ list_count, uint32_t nsegs, uint32_t xf)
{
    constexpr int THREADS = 1024, WAVES = 16, KPT = kBatchLongKpt, WAVE_TILE = kWave * KPT, TILE = THREADS * KPT;
    constexpr uint32_t PASSES = sizeof(KeyT); // 4 or 8: even
    __shared__ BatchLongSmem s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* const my_cnt = s.wcnt[wave];
    const KeyCodec<KeyT, true> codec(xf);
    const uint32_t n_list = list_count ? batch_list_length(*list_count, nsegs) : nsegs;

    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x)
    {
        const uint32_t seg = list ? list[li] : li;
        uint32_t begin, len;
        batch_segment(offsets, 0u, total, seg, begin, len);
        if (len < 2u) continue; // (uniform over the workgroup)

        for (uint32_t pass = 0; pass < PASSES; pass++)
        {
            const bool first = pass == 0, last = pass == PASSES - 1;
            const KeyT* const src_k = ((pass & 1u) ? tmp_keys : keys) + begin;
            KeyT* const dst_k = ((pass & 1u) ? keys : tmp_keys) + begin;
            const uint32_t* const src_v = VALS ? ((pass & 1u) ? tmp_vals : vals) + begin : nullptr;
            uint32_t* const dst_v = VALS ? ((pass & 1u) ? vals : tmp_vals) + begin : nullptr;
            const uint32_t shift = pass * 8u;

            // histogram of the segment
            for (int i = tid; i < WAVES * 256; i += THREADS) (&s.wcnt[0][0])[i] = 0;
            __syncthreads();
            for (uint64_t p = tid; p < len; p += THREADS) // (64-bit: len may lie within a stride of 2^32)
            {
                KeyT key = src_k[p];
                if (first) key = codec.encode(key);
                atomicAdd(&my_cnt[digit_of<KeyT>(key, shift, 0xFFu)], 1u);
            }
            __syncthreads();
            {
                uint32_t sum = 0, excl = 0;
                if (tid < 256)
                {
#pragma unroll
                    for (int w = 0; w < WAVES; w++) sum += s.wcnt[w][tid];
                }
                if (wave < 4)
                {
                    uint32_t wtotal;
                    excl = wave_exclusive_sum(sum, lane, wtotal);
                    if (lane == 0) s.scan_tmp[wave] = wtotal;
                }
                __syncthreads();
                if (tid < 256)
                {
                    for (uint32_t w = 0; w < wave; w++) excl += s.scan_tmp[w];
                    s.base[tid] = excl;
                }
            }
            __syncthreads();

            for (uint64_t t0 = 0; t0 < len; t0 += TILE) // (64-bit element positions: a segment may end within a tile of 2^32)
            {
                for (int i = tid; i < WAVES * 256; i += THREADS) (&s.wcnt[0][0])[i] = 0;
                KeyT key[KPT];
                uint32_t val[KPT], rank[KPT];
                const uint64_t wave_first = t0 + wave * WAVE_TILE;
                const int groups = wave_first >= len ? 0 : (int) (((len - wave_first) + 63u) >> 6);
#pragma unroll
                for (int i = 0; i < KPT; i++)
                {
                    const uint64_t p = wave_first + i * kWave + lane;
                    const bool ok = p < len;
                    KeyT raw = ok ? src_k[p] : (KeyT) 0;
                    if (first) raw = codec.encode(raw);
                    key[i] = ok ? raw : (KeyT) ~(KeyT) 0; // pads rank behind every element of the last tile and are not stored
                    val[i] = (VALS && ok) ? src_v[p] : 0u;
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < KPT; i++)
                    if (i < groups) rank[i] = batch_ballot_rank(digit_of<KeyT>(key[i], shift, 0xFFu), my_cnt);
                __syncthreads();
                if (tid < 256)
                {
                    uint32_t running = s.base[tid];
#pragma unroll
                    for (int w = 0; w < WAVES; w++)
                    {
                        const uint32_t c = s.wcnt[w][tid];
                        s.wcnt[w][tid] = running;
                        running += c;
                    }
                    s.base[tid] = running;
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < KPT; i++)
                {
                    const uint64_t p = wave_first + i * kWave + lane;
                    if (i < groups && p < len)
                    {
                        const uint32_t at = my_cnt[digit_of<KeyT>(key[i], shift, 0xFFu)] + rank[i];
                        if (at < len) // (always, while nobody else writes the segment: the histogram counted these elements)
                        {
                            dst_k[at] = last ? codec.decode(key[i]) : key[i];
                            if (VALS) dst_v[at] = val[i];
                        }
                    }
                }
                __syncthreads();
            }
            // the next pass reads what this one stored (this workgroup's own stores, behind a workgroup barrier)
            __threadfence_block();
            __syncthreads();
        }
    }
}

} // namespace glu_hip
