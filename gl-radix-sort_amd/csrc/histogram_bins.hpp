// histogram_bins.hpp -- the arithmetic of HISTOGRAM (histogram_kernels.hpp, glu_histogram.hip) in plain C++: the three rules that
// give a sample its bin (even bins over integers, exactly; even bins over floats, in double; sorted edges, by a branch-free upper
// bound), how the host folds lo, hi and bins into what the kernels evaluate, and the plan of a call.  The kernels include this
// header, and tests/test_histogram_bins.py includes it with a host compiler and holds every rule against numpy: what holds there
// holds on the device.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define GLU_HIST_FN __host__ __device__ __forceinline__
#else
#define GLU_HIST_FN inline // (a host compiler: the test program)
#endif

namespace glu_hip
{
constexpr uint32_t kHistNoBin = 0xFFFFFFFFu;      // the sample is not counted
constexpr uint32_t kHistLdsBins = 8192;           // the largest table kept in LDS; the largest number of uneven bins
constexpr uint32_t kHistMaxEvenBins = 1u << 24;   // the largest number of even bins
constexpr uint32_t kHistPacks = 4;                // 16-byte packs of samples per thread and tile: 64 bytes a lane in flight
constexpr uint64_t kHistMaxCount = 0xFFFFFFFFull; // count < 2^32

enum
{
    HIST_EVEN = 0,
    HIST_EDGES = 1
};
enum
{
    HIST_PATH_LDS = 0,
    HIST_PATH_GLOBAL = 1,
    HIST_PATH_BATCH = 2 // a batched call (the batched plan below); what glu_histogram_last reports for it
};

// ---- even bins over uint32 / int32: bin = floor((x - lo) / W), exactly ---------------------------------------------------------
// d = (uint32) x - (uint32) lo is x - lo for lo <= x (hi - lo <= 2^32 - 1 fits a word) and at least hi - lo + 1 for x < lo (it
// wraps past the top of the type), so lo <= x < hi is the one unsigned comparison d < span, signed or not.
// The division by the kernel-uniform W is a multiplication: with c = ceil(2^64 / W), c * W = 2^64 + e and 0 <= e < W, so
// c * d / 2^64 = d / W + (e / W) * d / 2^64, and the second term is below 2^-32 < 1 / W, the least distance of d / W from the
// next whole number: floor(c * d / 2^64) = floor(d / W) for EVERY d < 2^32, not nearly.  W = 1 has c = 2^64: it is told apart.
struct HistEvenInt
{
    uint32_t lo;    // the bits of lo
    uint32_t span;  // hi - lo = W * bins
    uint64_t magic; // ceil(2^64 / W); unused where W == 1
    uint32_t w_is_one;
};

// the top 64 bits of the 96-bit product c * d, its low word
GLU_HIST_FN uint32_t hist_div(uint32_t d, const HistEvenInt& r)
{
    const uint64_t low = (r.magic & 0xFFFFFFFFull) * d;
    const uint64_t high = (r.magic >> 32) * d + (low >> 32); // (2^32 - 1)^2 + 2^32 - 1 < 2^64
    return r.w_is_one ? d : (uint32_t) (high >> 32);
}

template<typename T>
GLU_HIST_FN uint32_t hist_even_int_bin(const HistEvenInt& r, T x)
{
    const uint32_t d = (uint32_t) x - r.lo;
    return d < r.span ? hist_div(d, r) : kHistNoBin;
}

// host: false where W = (hi - lo) / bins is not a whole number >= 1.  lo and hi as the type holds them, widened.
inline bool hist_make_even_int(int64_t lo, int64_t hi, uint32_t bins, HistEvenInt* out)
{
    if (hi <= lo || bins == 0) return false;
    const uint64_t span = (uint64_t) (hi - lo); // <= 2^32 - 1 for both 32-bit types
    if (span > 0xFFFFFFFFull || span % bins) return false;
    const uint64_t w = span / bins;
    out->lo = (uint32_t) lo;
    out->span = (uint32_t) span;
    out->w_is_one = w == 1 ? 1u : 0u;
    out->magic = w == 1 ? 0ull : 0xFFFFFFFFFFFFFFFFull / w + 1ull; // (w >= 2: floor((2^64 - 1) / w) + 1 = ceil(2^64 / w))
    return true;
}

// ---- even bins over float / double: one subtraction and one multiplication in IEEE double ---------------------------------------
// d = (double) x; a NaN fails the comparison and is dropped; bin = min((uint32) ((d - lo) * scale), bins - 1).  Nothing here can
// contract into an FMA, so numpy restates it bit for bit.
struct HistEvenFloat
{
    double lo, hi, scale;
    uint32_t last; // bins - 1
};

template<typename T>
GLU_HIST_FN uint32_t hist_even_float_bin(const HistEvenFloat& r, T x)
{
    const double d = (double) x;
    if (!(d >= r.lo && d < r.hi)) return kHistNoBin;
    const uint32_t b = (uint32_t) ((d - r.lo) * r.scale); // 0 <= the product <= bins * (1 + 2^-51): it fits
    return b < r.last ? b : r.last;
}

// host: false where lo, hi are not finite, lo >= hi, or hi - lo or the scale is not finite in double
inline bool hist_make_even_float(double lo, double hi, uint32_t bins, HistEvenFloat* out)
{
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || bins == 0) return false;
    const double width = hi - lo;
    if (!std::isfinite(width)) return false;
    const double scale = (double) bins / width;
    if (!std::isfinite(scale)) return false;
    out->lo = lo;
    out->hi = hi;
    out->scale = scale;
    out->last = bins - 1;
    return true;
}

// ---- sorted edges: bin = #{e in edges : e <= x} - 1 ---------------------------------------------------------------------------
// trips of the bound loop over `len` edges: the bound is one of 0 .. len  (search_steps of sorted search)
GLU_HIST_FN uint32_t hist_steps(uint32_t len) { return len ? 32u - (uint32_t) __builtin_clz(len) : 0u; }

// The upper bound of x among n_edges = bins + 1 >= 2 non-decreasing edges, built bit by bit from the top as sorted search's DIRECT
// path builds it: `steps` = hist_steps(n_edges) trips whatever the values hold, every probe clamped into [0, n_edges).  The
// comparison is the type's own: integers in their order, floats as IEEE values (-0.0 == +0.0; a NaN sample passes no edge and has
// bound 0).  edge_at(i) is called with i < n_edges only.  Returns the bin where 0 <= bin < bins, else kHistNoBin: edges that are not
// sorted or hold a NaN give some bound in 0 .. n_edges, hence a wrong bin or none, and never an index outside the table.
template<typename T, typename EdgeAt>
GLU_HIST_FN uint32_t hist_edges_bin(T x, uint32_t n_edges, uint32_t steps, EdgeAt edge_at)
{
    uint32_t pos = 0;
    for (uint32_t step = steps ? 1u << (steps - 1) : 0u; step; step >>= 1) // (kernel-uniform)
    {
        const uint32_t next = pos + step;
        const uint32_t probe = next < n_edges ? next : n_edges; // 1 <= probe <= n_edges
        const T e = edge_at(probe - 1u);
        pos = (next <= n_edges && e <= x) ? next : pos;
    }
    const uint32_t bin = pos - 1u; // (no edge passed: wraps to kHistNoBin)
    return bin < n_edges - 1u ? bin : kHistNoBin;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// Threads per workgroup, by what a workgroup keeps in LDS, so that every mode has 16 waves to the CU:
//   even        a table of 8192 counters, 32 KiB                           256 threads, 4 workgroups (5 would fit)
//   edges, 4 B  the table and 8193 edges, 64 KiB + 16 B: two to the CU     512 threads
//   edges, 8 B  the table and 8193 edges, 96 KiB + 16 B: one to the CU    1024 threads
constexpr uint32_t hist_threads(uint32_t key_bytes, int mode) { return mode == HIST_EVEN ? 256u : key_bytes == 4 ? 512u : 1024u; }
// Workgroups of the counting kernel at the most: the workgroups that are resident on 256 CUs at once (rows of the partial table).
constexpr uint32_t hist_groups_max(uint32_t key_bytes, int mode) { return mode == HIST_EVEN ? 1024u : key_bytes == 4 ? 512u : 256u; }
constexpr uint32_t hist_tile(uint32_t key_bytes, int mode) { return hist_threads(key_bytes, mode) * kHistPacks * (16u / key_bytes); }

struct HistPlan
{
    uint32_t path, threads, tile, tiles, groups, kernels;
    size_t scratch_bytes;
};

// LDS path (bins <= 8192): count, unless there is nothing to count; sum the columns, unless nothing is counted AND the call
// accumulates.  GLOBAL path: clear, unless the call accumulates; add, unless there is nothing to count.
inline HistPlan hist_plan(uint64_t count, uint32_t bins, uint32_t key_bytes, int mode, bool accumulate)
{
    HistPlan p;
    p.path = bins <= kHistLdsBins ? (uint32_t) HIST_PATH_LDS : (uint32_t) HIST_PATH_GLOBAL;
    p.threads = hist_threads(key_bytes, mode);
    p.tile = hist_tile(key_bytes, mode);
    p.tiles = (uint32_t) ((count + p.tile - 1) / p.tile);
    const uint32_t most = hist_groups_max(key_bytes, mode);
    p.groups = p.tiles < most ? p.tiles : most;
    if (p.path == HIST_PATH_LDS)
    {
        p.kernels = (count ? 1u : 0u) + (count || !accumulate ? 1u : 0u);
        p.scratch_bytes = (size_t) p.groups * bins * sizeof(uint32_t);
    }
    else
    {
        p.kernels = (accumulate ? 0u : 1u) + (count ? 1u : 0u);
        p.scratch_bytes = 0;
    }
    return p;
}

// ---- the batched plan (histogram_batch_kernels.hpp: every segment of an array counted into a row of its own) --------------------
// Three classes by the length of a segment, drawn here and nowhere else (glu_histogram_plan_batch reports them):
//   wave   up to wave_limit samples and bins <= 2048: a wave per segment with a table of its own, four to a workgroup (32 KiB).
//          8 KiB of samples.  With more bins the class is empty and its segments are the block class's.
//   block  up to block_limit = one chunk: a workgroup per segment, the table of the single call.
//   long   cut into chunks of max(512 KiB of samples, 64 samples per bin): a chunk's partial row of bins * 4 bytes is then at most
//          1/16 of a byte per sample of the chunk, and a batch has at most 2 * (total / chunk) chunks (hist_batch_slots): the
//          scratch of a prepared batch stays at or below total / 8 bytes.
// Each value was held against half and twice of the starting values (4 KiB, 256 KiB, one chunk) on the device, and 8 KiB and 512 KiB
// won (profiles/histogram_batch/constants.txt); against twice of THESE they were not held: provisional upwards.
// (A tuning build of glu_histogram.hip sets one of the three macros; the library is built without them.)
#ifndef GLU_HIST_BATCH_WAVE_BYTES
#define GLU_HIST_BATCH_WAVE_BYTES 8192
#endif
#ifndef GLU_HIST_BATCH_CHUNK_BYTES
#define GLU_HIST_BATCH_CHUNK_BYTES (1u << 19)
#endif
#ifndef GLU_HIST_BATCH_BLOCK_BYTES
#define GLU_HIST_BATCH_BLOCK_BYTES GLU_HIST_BATCH_CHUNK_BYTES
#endif
constexpr uint32_t kHistBatchWaveBytes = GLU_HIST_BATCH_WAVE_BYTES;   // longest segment of the wave class, in bytes of samples
constexpr uint32_t kHistBatchWaveBins = 2048;                         // most bins of the wave class: four tables of them are 32 KiB
constexpr uint32_t kHistBatchWaves = 4;                               // waves (segments at a time) of a workgroup of the wave class
constexpr uint32_t kHistBatchChunkBytes = GLU_HIST_BATCH_CHUNK_BYTES; // a chunk of the long class, in bytes of samples, at the least
constexpr uint32_t kHistBatchBlockBytes = GLU_HIST_BATCH_BLOCK_BYTES; // longest segment of the block class: one chunk
constexpr uint32_t kHistBatchChunkPerBin = 64;                        // ... and both in samples per bin, at the least

constexpr uint32_t hist_batch_wave_limit(uint32_t bins, uint32_t key_bytes) { return bins <= kHistBatchWaveBins ? kHistBatchWaveBytes / key_bytes : 0u; }
constexpr uint32_t hist_batch_at_least_per_bin(uint32_t samples, uint32_t bins)
{
    return samples > kHistBatchChunkPerBin * bins ? samples : kHistBatchChunkPerBin * bins;
}
constexpr uint32_t hist_batch_chunk(uint32_t bins, uint32_t key_bytes) { return hist_batch_at_least_per_bin(kHistBatchChunkBytes / key_bytes, bins); }
constexpr uint32_t hist_batch_block_limit(uint32_t bins, uint32_t key_bytes)
{
    return hist_batch_at_least_per_bin(kHistBatchBlockBytes / key_bytes, bins);
}

struct HistBatchPlan
{
    uint32_t path, workgroups, wave_limit, block_limit, chunk; // path: 0 = empty, 1 = wave, 2 = block, 3 = long
    size_t scratch_bytes_per_chunk;
};

// one segment of `count` samples (bins <= kHistLdsBins: the caller)
inline HistBatchPlan hist_batch_plan(uint64_t count, uint32_t bins, uint32_t key_bytes)
{
    HistBatchPlan p;
    p.wave_limit = hist_batch_wave_limit(bins, key_bytes);
    p.block_limit = hist_batch_block_limit(bins, key_bytes);
    p.chunk = hist_batch_chunk(bins, key_bytes);
    p.scratch_bytes_per_chunk = (size_t) bins * sizeof(uint32_t);
    p.path = count == 0 ? 0u : count <= p.wave_limit ? 1u : count <= p.block_limit ? 2u : 3u;
    p.workgroups = p.path == 3 ? (uint32_t) ((count + p.chunk - 1) / p.chunk) : p.path ? 1u : 0u;
    return p;
}

} // namespace glu_hip
