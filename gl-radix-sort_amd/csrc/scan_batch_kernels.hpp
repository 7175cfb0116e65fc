// scan_batch_kernels.hpp -- gfx950 kernels of the BATCHED scan: every segment of an array scanned on its own.
// glu_scan_run_batch_offsets_ptr is the exclusive `+` scan in place (OP_SUM, !INCLUSIVE, IN_PLACE: the code it always was);
// glu_scan_run_batch_offsets_op_ptr takes any of Reduce's four operators, exclusive or inclusive, and may store to a second array
// (scan_ops_wave_kernel and scan_ops_block_kernel around the same bodies).  Not in the
// reference, whose BlellochScan takes equal power-of-two partitions and does an exclusive `+` scan only
// (glu/BlellochScan.hpp:130-139).
//
// Three size classes (scan_batch_plan is the one place that draws the lines, in BYTES of a segment):
//   short   scan_batch_wave_kernel     up to 2 KiB: a group of 4 / 16 / 64 lanes of a wave holds one segment in registers (up to
//                                      128 B, up to 512 B, more), lane j the elements [j * e, (j + 1) * e) with e = ceil(length /
//                                      lanes): in-lane sums, a scan over the group's lanes with shuffles, one store per element.
//                                      No LDS, no barrier.
//   medium  scan_batch_block_kernel    up to 64 KiB:  a workgroup scans one segment tile after tile (ScanCfg::CHUNK elements, the
//           (mode 0)                   tile of scan_chunks_kernel) with a running carry: 8 B of traffic per 4-byte element.
//   long    reduce_batch_chunk_kernel  the segment is cut into chunks of 32 KiB; the batched reduce's chunk kernel (Sum) writes
//           scan_batch_block_kernel    partials[slot] = sum of one chunk, a segment's slots side by side in chunk order; mode 1
//           (modes 1 and 2)            scans every long segment's run of partials in place (the same tile loop: a segment of 2^28
//                                      uint32 has 32768 partials, eight tiles); mode 2 scans every chunk with partials[slot] as
//                                      its carry-in.  12 B per 4-byte element, and one long segment fills the device.
// In front, the batched reduce's binning kernel (reduce_batch_bin_kernel, with no `out` array to write identities to) lists the
// segments by class: three short lists by group size, the medium list, the long list and the list of chunks.  The lists, their
// layout and the clamps are batch_lists.hpp's (BatchListsLayout, batch_offsets_segment, batch_list_length): a segment whose end
// lies below its begin or beyond `total` is EMPTY to every kernel, so nothing outside [0, total) is read or written.
//
// Operator and kind: OP is combined with the earlier operand on the left everywhere; positions that hold no element read as the
// operator's identity (scan_identity: 0, 1, +inf or the type's maximum, -inf or the type's lowest), which is also what an
// exclusive scan stores first.  INCLUSIVE stores exclusive OP x, so under Sum a first element -0.0 comes out as +0.0.  The chunk
// sums of the long class are exclusive-scanned whatever the kind is; the kind is applied where the elements are stored.
// Store side: loads follow `data`, stores go to the same positions of `out`.  Which element goes to which lane follows data's
// address alone; 16-byte stores are used where `out` shares data's address modulo 16 (always, in place), single elements
// otherwise, so the results are the same bits wherever `out` lies.
//
// Order of addition: inside a lane in ascending order, then lanes, waves, tiles and chunks in their order.  Which element goes to
// which lane depends on the segment's address (its 16-byte alignment), its length and its class, and on nothing else: no atomics
// on values, no look-back, nothing in arrival order.  List positions and chunk slots ARE handed out in arrival order; every item
// works on a range of its own, and the one range whose address follows from a slot -- a long segment's run of partials -- is laid
// out from its own first element, not from a 16-byte boundary (FROM_FIRST below).
#pragma once

#include <limits>
#include <type_traits>

#include "reduce_batch_kernels.hpp"

namespace glu_hip
{
constexpr uint32_t kSbGroup4Bytes = 128;       // up to here 4 lanes hold a segment (32 B per lane)
constexpr uint32_t kSbGroup16Bytes = 512;      // up to here 16 lanes (32 B per lane), beyond it the whole wave
constexpr uint32_t kSbWaveBytes = 2048;        // longest segment of the short class (32 B per lane)
constexpr uint32_t kSbBlockBytes = 64 * 1024;  // longest segment of the medium class
constexpr uint32_t kSbChunkBytes = 32 * 1024;  // chunk of the long class
constexpr int kSbThreads = 256;
constexpr int kSbWaves = kSbThreads / kW;
static_assert(kSbThreads == kRbThreads, "reduce_batch_chunk_kernel writes the chunk sums");

enum
{
    SB_MODE_SEGMENTS = 0, // the medium list: a segment of the caller's array per item
    SB_MODE_PARTIALS = 1, // the long list: a long segment's run of partials per item
    SB_MODE_CHUNKS = 2    // the chunk list: a chunk of a long segment per item, carry-in from its partial
};

// host only: class (0 = empty, 1 = short, 2 = medium, 3 = long) and workgroups one segment of `count` elements is spread over
inline void scan_batch_plan(uint64_t count, uint32_t elem_bytes, uint32_t& path, uint32_t& workgroups)
{
    workgroups = count ? 1u : 0u;
    if (count == 0) path = 0;
    else if (count <= kSbWaveBytes / elem_bytes) path = 1;
    else if (count <= kSbBlockBytes / elem_bytes) path = 2;
    else
    {
        path = 3;
        const uint64_t chunk = kSbChunkBytes / elem_bytes;
        const uint64_t n = (count + chunk - 1) / chunk;
        workgroups = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) n;
    }
}

// the identity element of OP (the batched reduce's identity_of, on the device)
template<int OP, typename S, int N>
__device__ __forceinline__ Elem<S, N> scan_identity()
{
    S v;
    if (OP == OP_SUM) v = (S) 0;
    else if (OP == OP_MUL) v = (S) 1;
    else if (std::is_floating_point<S>::value) v = OP == OP_MIN ? std::numeric_limits<S>::infinity() : -std::numeric_limits<S>::infinity();
    else v = OP == OP_MIN ? std::numeric_limits<S>::max() : std::numeric_limits<S>::lowest();
    Elem<S, N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.c[i] = v;
    return r;
}

// The one-segment form: the offsets {0, total} of the segment [0, total), written on the device so that the call copies nothing
// from the host.
static __global__ void scan_batch_whole_offsets_kernel(uint32_t* __restrict__ offsets, uint32_t total)
{
    if (threadIdx.x < 2) offsets[threadIdx.x] = threadIdx.x ? total : 0u;
}

// ---------------------------------------------------------------------------------------------------------
// Short segments: a group of 1 << lg lanes per segment, the segment in registers.
// ---------------------------------------------------------------------------------------------------------
// IN_PLACE: `out` is the only array, loads go through it too and `data` is not looked at; otherwise `data` is only read and may
// or may not be the same array.
template<int OP, bool INCLUSIVE, typename S, int N, bool IN_PLACE>
__device__ __forceinline__ void scan_batch_wave(const Elem<S, N>* data, Elem<S, N>* out, BatchListsArgs a)
{
    using T = Elem<S, N>;
    constexpr uint32_t EMAX = kSbWaveBytes / kW / (uint32_t) sizeof(T); // elements a lane can hold: 8 / 4 / 2 / 1
    static_assert(kSbGroup4Bytes <= 4 * EMAX * sizeof(T) && kSbGroup16Bytes <= 16 * EMAX * sizeof(T), "a group holds its longest segment");
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a third of the grid walks each short list
    const int sub = (int) (blockIdx.x % 3u);
    const uint32_t block = blockIdx.x / 3u, blocks = gridDim.x / 3u;
    const uint32_t lg = sub == BATCH_LIST_SHORT4 ? 2u : sub == BATCH_LIST_SHORT16 ? 4u : 6u;
    const uint32_t G = 1u << lg, per_wave = kW >> lg;
    const uint32_t n = batch_list_length(a.counts, a.layout, sub);
    const uint32_t* list = a.lists + a.layout.start[sub];
    const uint32_t j = lane & (G - 1u);

    for (uint64_t first = (uint64_t) (block * kSbWaves + wave) * per_wave; first < n; first += (uint64_t) blocks * kSbWaves * per_wave)
    {
        const uint64_t li = first + (lane >> lg);
        uint64_t begin = 0, len64 = 0;
        if (li < n) batch_lists_segment(a, list[li], begin, len64);
        uint32_t len = (uint32_t) len64;
        if (len > a.layout.limit[sub]) len = 0; // (only overlapping -- malformed -- lists can hold such an entry)
        const T* p = (IN_PLACE ? out : data) + begin;
        T* q = out + begin;
        const uint32_t per_lane = (len + G - 1u) >> lg; // <= EMAX
        const uint32_t i0 = j * per_lane;
        T x[EMAX];
#pragma unroll
        for (uint32_t k = 0; k < EMAX; k++) x[k] = (k < per_lane && i0 + k < len) ? p[i0 + k] : scan_identity<OP, S, N>();
        T incl = x[0];
#pragma unroll
        for (uint32_t k = 1; k < EMAX; k++) incl = combine<OP>(incl, x[k]);
#pragma unroll
        for (uint32_t off = 1; off < (uint32_t) kW; off <<= 1)
        {
            if (off >= G) continue; // wave-uniform
            T t = shfl_up_t(incl, (int) off);
            if (j >= off) incl = combine<OP>(t, incl);
        }
        T up = shfl_up_t(incl, 1);
        T acc = j == 0 ? scan_identity<OP, S, N>() : up;
#pragma unroll
        for (uint32_t k = 0; k < EMAX; k++)
        {
            if (INCLUSIVE) acc = combine<OP>(acc, x[k]);
            if (k < per_lane && i0 + k < len) q[i0 + k] = acc;
            if (!INCLUSIVE) acc = combine<OP>(acc, x[k]);
        }
    }
}

// the exclusive `+` scan in place (glu_scan_run_batch_offsets_ptr) / every operator and kind with a store pointer
template<typename S, int N>
__global__ __launch_bounds__(kSbThreads) void scan_batch_wave_kernel(Elem<S, N>* __restrict__ data, BatchListsArgs a)
{
    scan_batch_wave<OP_SUM, false, S, N, true>(data, data, a);
}
template<int OP, bool INCLUSIVE, typename S, int N>
__global__ __launch_bounds__(kSbThreads) void scan_ops_wave_kernel(const Elem<S, N>* data, Elem<S, N>* out, BatchListsArgs a)
{
    scan_batch_wave<OP, INCLUSIVE, S, N, false>(data, out, a);
}

// ---------------------------------------------------------------------------------------------------------
// Scan of one contiguous range by a workgroup, read at `p` and stored at the same positions of `q`, `carry` in front of it:
// tile after tile of ScanCfg::CHUNK elements, laid out inside a tile like a chunk of scan_chunks_kernel (group-major, then lane,
// then the elements of a 16-byte pack).  Tiles are counted from the 16-byte boundary at or below the range's first element, so every pack is aligned: whole
// packs take one 16-byte load, the packs that hold the range's first and last elements go element by element, and nothing
// outside the range is read or written.  Stores go the same way where q lies as p does modulo 16 (IN_PLACE: q == p, not looked
// at), element by element otherwise.  FROM_FIRST (the partials of a long segment, whose slot -- and with it the run's
// alignment -- depends on the order in which segments were binned): tiles are counted from the range's own first element
// instead, so that which element goes to which lane depends on the range's length alone; packs are then accessed 16 bytes at a
// time only if the range happens to be aligned, element by element otherwise, with the same result.  `phase` alternates the two rows of wsum so that one barrier per tile is enough
// (a row is written again two tiles later, behind the barrier of the tile in between).
// ---------------------------------------------------------------------------------------------------------
// (IN_PLACE: the one pointer of the range is a restrict pointer, as it was when the range had one pointer only)
template<typename T, bool IN_PLACE>
struct ScanBatchStore
{
    using ptr = T*;
};
template<typename T>
struct ScanBatchStore<T, true>
{
    using ptr = T* __restrict__;
};

template<int OP, bool INCLUSIVE, typename S, int N, bool FROM_FIRST, bool IN_PLACE>
__device__ __forceinline__ void scan_batch_range(const Elem<S, N>* p, typename ScanBatchStore<Elem<S, N>, IN_PLACE>::ptr q, uint32_t len,
                                                 Elem<S, N> carry, uint32_t tid, Elem<S, N> (*wsum)[kSbWaves], uint32_t& phase)
{
    using T = Elem<S, N>;
    using C = ScanCfg<T, 4, kSbThreads>;
    if (IN_PLACE) p = q;
    const uint32_t lane = tid & 63, wave = tid >> 6;
    if (len == 0) return; // (workgroup-uniform)
    const uint32_t mis = (C::VEC > 1 && !FROM_FIRST) ? (uint32_t) (((uintptr_t) p & 15u) / sizeof(T)) : 0u; // elements behind the boundary
    const bool packs = !FROM_FIRST || ((uintptr_t) p & 15u) == 0; // 16-byte accesses are possible
    const bool spacks = IN_PLACE ? packs : packs && (((uintptr_t) q - (uintptr_t) p) & 15u) == 0; // ... on the store side (workgroup-uniform)
    const uint32_t vlen = len + mis;
    T run = carry;
    for (uint32_t tile = 0; tile < vlen; tile += C::CHUNK) // (workgroup-uniform)
    {
        const uint32_t lo = tile == 0 ? mis : 0u;
        const uint32_t hi = vlen - tile < (uint32_t) C::CHUNK ? vlen - tile : (uint32_t) C::CHUNK;
        const T* base = p + ((int64_t) tile - (int64_t) mis); // element e of the tile; only elements in [lo, hi) are touched
        T* sbase = q + ((int64_t) tile - (int64_t) mis);
        T x[C::GROUPS][C::VEC];
#pragma unroll
        for (int g = 0; g < C::GROUPS; g++)
        {
            const uint32_t e0 = wave * C::WAVE_ELEMS + (g * kW + lane) * C::VEC;
            if (packs && e0 >= lo && e0 + C::VEC <= hi)
            {
                const Pack<T, C::VEC> pk = *reinterpret_cast<const Pack<T, C::VEC>*>(base + e0);
#pragma unroll
                for (int k = 0; k < C::VEC; k++) x[g][k] = pk.v[k];
            }
            else
            {
#pragma unroll
                for (int k = 0; k < C::VEC; k++) x[g][k] = (e0 + k >= lo && e0 + k < hi) ? base[e0 + k] : scan_identity<OP, S, N>();
            }
        }
        T gexcl[C::GROUPS], gtot[C::GROUPS];
#pragma unroll
        for (int g = 0; g < C::GROUPS; g++)
        {
            T incl = x[g][0];
#pragma unroll
            for (int k = 1; k < C::VEC; k++) incl = combine<OP>(incl, x[g][k]);
#pragma unroll
            for (int off = 1; off < kW; off <<= 1)
            {
                T t = shfl_up_t(incl, off);
                if (lane >= (uint32_t) off) incl = combine<OP>(t, incl);
            }
            gtot[g] = shfl_t(incl, kW - 1);
            T up = shfl_up_t(incl, 1);
            gexcl[g] = lane == 0 ? scan_identity<OP, S, N>() : up;
        }
        T wave_total = gtot[0];
#pragma unroll
        for (int g = 1; g < C::GROUPS; g++) wave_total = combine<OP>(wave_total, gtot[g]);
        T* row = wsum[phase & 1u];
        phase++;
        if (lane == 0) row[wave] = wave_total;
        __syncthreads();
        T mine = run;
#pragma unroll
        for (int w = 0; w < kSbWaves; w++)
        {
            if ((uint32_t) w == wave) mine = run;
            run = combine<OP>(run, row[w]);
        }
#pragma unroll
        for (int g = 0; g < C::GROUPS; g++)
        {
            T acc = combine<OP>(mine, gexcl[g]);
            Pack<T, C::VEC> pk;
#pragma unroll
            for (int k = 0; k < C::VEC; k++)
            {
                if (INCLUSIVE) acc = combine<OP>(acc, x[g][k]);
                pk.v[k] = acc;
                if (!INCLUSIVE) acc = combine<OP>(acc, x[g][k]);
            }
            const uint32_t e0 = wave * C::WAVE_ELEMS + (g * kW + lane) * C::VEC;
            if (spacks && e0 >= lo && e0 + C::VEC <= hi) *reinterpret_cast<Pack<T, C::VEC>*>(sbase + e0) = pk;
            else
            {
#pragma unroll
                for (int k = 0; k < C::VEC; k++)
                    if (e0 + k >= lo && e0 + k < hi) sbase[e0 + k] = pk.v[k];
            }
            mine = combine<OP>(mine, gtot[g]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// One workgroup per item of a list (see SB_MODE_*), the grid sized to the device.
// ---------------------------------------------------------------------------------------------------------
template<int OP, bool INCLUSIVE, typename S, int N, bool IN_PLACE>
__device__ __forceinline__ void scan_batch_block(const Elem<S, N>* data, Elem<S, N>* out, Elem<S, N>* __restrict__ partials, BatchListsArgs a,
                                                 int mode, Elem<S, N> (*wsum)[kSbWaves])
{
    using T = Elem<S, N>;
    const uint32_t tid = threadIdx.x;
    const int c = mode == SB_MODE_SEGMENTS ? BATCH_LIST_BLOCK : mode == SB_MODE_PARTIALS ? BATCH_LIST_LONG : BATCH_LIST_CHUNKS;
    const uint32_t n = batch_list_length(a.counts, a.layout, c);
    uint32_t phase = 0;
    for (uint32_t li = blockIdx.x; li < n; li += gridDim.x)
    {
        uint64_t begin, len;
        if (mode == SB_MODE_SEGMENTS)
        {
            batch_lists_segment(a, a.lists[a.layout.start[BATCH_LIST_BLOCK] + li], begin, len);
            scan_batch_range<OP, INCLUSIVE, S, N, false, IN_PLACE>(data + begin, out + begin, (uint32_t) len, scan_identity<OP, S, N>(), tid, wsum,
                                                                   phase);
            continue;
        }
        const uint2 entry = reinterpret_cast<const uint2*>(a.lists + a.layout.start[c])[li];
        batch_lists_segment(a, entry.x, begin, len);
        if (mode == SB_MODE_PARTIALS)
        {
            // entry.y = slot of the segment's first chunk (a listed segment's whole run lies inside the chunk list); the chunk
            // sums become the chunks' carry-ins: an exclusive scan in place, whatever the kind of the call
            const uint64_t nchunks = (len + a.layout.chunk - 1) / a.layout.chunk;
            uint64_t room = a.layout.capacity[BATCH_LIST_CHUNKS] > entry.y ? a.layout.capacity[BATCH_LIST_CHUNKS] - entry.y : 0;
            scan_batch_range<OP, false, S, N, true, true>(nullptr, partials + entry.y, (uint32_t) (nchunks < room ? nchunks : room),
                                                          scan_identity<OP, S, N>(), tid, wsum, phase);
        }
        else
        {
            // entry.y = chunk of the segment; li = its slot
            const uint64_t at = (uint64_t) entry.y * a.layout.chunk;
            if (at >= len) continue; // (workgroup-uniform)
            const uint64_t left = len - at;
            scan_batch_range<OP, INCLUSIVE, S, N, false, IN_PLACE>(data + begin + at, out + begin + at,
                                                                   left < a.layout.chunk ? (uint32_t) left : a.layout.chunk, partials[li], tid, wsum, phase);
        }
    }
}

// the exclusive `+` scan in place (glu_scan_run_batch_offsets_ptr) / every operator and kind with a store pointer
template<typename S, int N>
__global__ __launch_bounds__(kSbThreads) void scan_batch_block_kernel(Elem<S, N>* __restrict__ data, Elem<S, N>* __restrict__ partials,
                                                                       BatchListsArgs a, int mode)
{
    __shared__ Elem<S, N> wsum[2][kSbWaves];
    scan_batch_block<OP_SUM, false, S, N, true>(data, data, partials, a, mode, wsum);
}
template<int OP, bool INCLUSIVE, typename S, int N>
__global__ __launch_bounds__(kSbThreads) void scan_ops_block_kernel(const Elem<S, N>* data, Elem<S, N>* out, Elem<S, N>* __restrict__ partials,
                                                                     BatchListsArgs a, int mode)
{
    __shared__ Elem<S, N> wsum[2][kSbWaves];
    scan_batch_block<OP, INCLUSIVE, S, N, false>(data, out, partials, a, mode, wsum);
}

} // namespace glu_hip
