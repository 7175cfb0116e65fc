// glu_key_runs.hip -- key runs of libglu_hip.so (key_runs_kernels.hpp): glu_key_runs_create, glu_key_runs_destroy,
// glu_key_runs_prepare, glu_key_runs_run_ptr, glu_key_runs_plan.
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "glu_batch_host.hpp"
#include "glu_key_runs_object.hpp"
#include "key_runs_kernels.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
glu_status check_count(size_t count)
{
    return count < ((size_t) 1 << 32) ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "key runs take fewer than 2^32 keys (got %zu)", count);
}

glu_status check_key_bits(uint32_t key_bits)
{
    return key_bits == 32 || key_bits == 64 ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "key_bits must be 32 or 64 (got %u)", key_bits);
}

// The tile counts of `count` keys.  A base that is not 16-byte aligned moves the keys up to a pack's length into the first tile,
// which can add a tile behind the last: one more than the plan's.
glu_status reserve_tiles(glu_key_runs_s* r, size_t count, uint32_t key_bits)
{
    uint32_t tile, tiles, rounds;
    key_runs_plan(count, key_bits / 8, tile, tiles, rounds);
    return count ? r->tile_counts.reserve(((size_t) tiles + 1) * sizeof(uint32_t)) : GLU_OK;
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

struct Call
{
    glu_key_runs_s* runs;
    const void* keys;
    size_t count;
    uint32_t begin_bit, end_bit;
    void* unique_keys;
    uint32_t* offsets;
    size_t max_runs;
    uint32_t* num_runs;
    hipStream_t stream;
};

// Three kernels, whatever the keys hold: the heads of every tile counted, the counts scanned by one workgroup, the heads written
// with their ranks (and the offsets behind the last run filled).  The grids follow from `count`, `max_runs` and the alignment of
// `keys`, never from the data.
template<typename K>
glu_status run(const Call& c)
{
    using C = KeyRunsCfg<K>;
    KeyRunsArgs<K> a;
    a.lo = ((uintptr_t) c.keys & 15u) / sizeof(K);
    a.hi = a.lo + c.count;
    a.base = (const K*) c.keys - a.lo;
    const uint32_t width = c.end_bit - c.begin_bit;
    a.mask = width == 0 ? (K) 0 : (K) ((width >= 8 * sizeof(K) ? ~(K) 0 : (((K) 1 << width) - 1)) << c.begin_bit);
    a.tiles = c.count ? (uint32_t) ((a.hi + C::TILE - 1) / C::TILE) : 0u;
    uint32_t* tile_counts = (uint32_t*) c.runs->tile_counts.ptr;
    const uint32_t device_grid = cus() * 8u;
    hipLaunchKernelGGL((key_runs_count_kernel<K>), dim3(std::max(1u, std::min(a.tiles, device_grid))), dim3(kKrThreads), 0, c.stream, a,
                       tile_counts);
    HIP_TRY(hipGetLastError());
    GLU_TRY(launch_tile_count_scan(tile_counts, a.tiles, c.num_runs, c.stream));
    // (the fill: a workgroup per 4096 entries of offsets, if the tiles ask for fewer)
    const uint32_t fill_blocks = (uint32_t) std::min<uint64_t>((c.max_runs + 1 + 4095) / 4096, device_grid);
    hipLaunchKernelGGL((key_runs_write_kernel<K>), dim3(std::max(fill_blocks, std::min(a.tiles, device_grid))), dim3(kKrThreads), 0, c.stream,
                       a, (const uint32_t*) tile_counts, (const uint32_t*) c.num_runs, (K*) c.unique_keys, c.offsets, (uint32_t) c.max_runs);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}
} // namespace

glu_status glu_hip::host::launch_tile_count_scan(uint32_t* tile_counts, uint32_t tiles, uint32_t* total, hipStream_t stream)
{
    hipLaunchKernelGGL(key_runs_scan_kernel, dim3(1), dim3(kSbThreads), 0, stream, tile_counts, tiles, total);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

uint32_t glu_hip::host::tile_count_scan_rounds(uint32_t tiles) { return (tiles + kKrScanRound - 1) / kKrScanRound; }

extern "C" {

glu_status glu_key_runs_plan(size_t count, uint32_t key_bits, uint32_t* tile, uint32_t* tiles, uint32_t* scan_rounds)
{
    GLU_TRY(check_key_bits(key_bits));
    GLU_TRY(check_count(count));
    uint32_t t, n, r;
    key_runs_plan(count, key_bits / 8, t, n, r);
    if (tile) *tile = t;
    if (tiles) *tiles = n;
    if (scan_rounds) *scan_rounds = r;
    return GLU_OK;
}

glu_status glu_key_runs_create(glu_key_runs* out)
{
    GLU_TRY(enter());
    if (!out) return fail(GLU_ERROR_INVALID_ARGUMENT, "out is NULL");
    *out = new glu_key_runs_s();
    return GLU_OK;
}

glu_status glu_key_runs_destroy(glu_key_runs runs)
{
    GLU_TRY(enter());
    if (!runs) return GLU_OK;
    (void) hipDeviceSynchronize(); // (a caller stream may still run its kernels)
    runs->tile_counts.release();
    delete runs;
    return GLU_OK;
}

glu_status glu_key_runs_prepare(glu_key_runs runs, size_t count, uint32_t key_bits)
{
    GLU_TRY(enter());
    if (!runs) return fail(GLU_ERROR_INVALID_ARGUMENT, "runs is NULL");
    GLU_TRY(check_key_bits(key_bits));
    GLU_TRY(check_count(count));
    return reserve_tiles(runs, count, key_bits);
}

glu_status glu_key_runs_run_ptr(glu_key_runs runs, const void* keys, size_t count, uint32_t key_bits, uint32_t begin_bit,
                                uint32_t end_bit, void* unique_keys, uint32_t* offsets, size_t max_runs, uint32_t* num_runs, void* stream)
{
    GLU_TRY(enter());
    if (!runs) return fail(GLU_ERROR_INVALID_ARGUMENT, "runs is NULL");
    GLU_TRY(check_key_bits(key_bits));
    GLU_TRY(check_count(count));
    if (max_runs >= ((size_t) 1 << 32)) return fail(GLU_ERROR_INVALID_ARGUMENT, "max_runs must be below 2^32 (got %zu)", max_runs);
    if (begin_bit > end_bit || end_bit > key_bits)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid bit range [%u, %u) of %u-bit keys", begin_bit, end_bit, key_bits);
    if (count && !keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid key buffer");
    if (!offsets) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid offsets array");
    if (!num_runs) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid num_runs pointer");
    const size_t key_bytes = key_bits / 8;
    if ((uintptr_t) keys % key_bytes) return fail(GLU_ERROR_INVALID_ARGUMENT, "keys is not aligned to the key size");
    if ((uintptr_t) unique_keys % key_bytes) return fail(GLU_ERROR_INVALID_ARGUMENT, "unique_keys is not aligned to the key size");
    if ((uintptr_t) offsets % sizeof(uint32_t)) return fail(GLU_ERROR_INVALID_ARGUMENT, "the offsets array is not aligned to its element size");
    if ((uintptr_t) num_runs % sizeof(uint32_t)) return fail(GLU_ERROR_INVALID_ARGUMENT, "num_runs is not aligned to 4 bytes");
    if (overlaps(keys, count * key_bytes, offsets, (max_runs + 1) * sizeof(uint32_t)))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "the offsets array overlaps keys");
    if (unique_keys && overlaps(keys, count * key_bytes, unique_keys, max_runs * key_bytes))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "unique_keys overlaps keys");
    if (overlaps(keys, count * key_bytes, num_runs, sizeof(uint32_t))) return fail(GLU_ERROR_INVALID_ARGUMENT, "num_runs overlaps keys");
    GLU_TRY(reserve_tiles(runs, count, key_bits));
    const Call c{runs, keys, count, begin_bit, end_bit, unique_keys, offsets, max_runs, num_runs, pick_stream(stream)};
    return key_bits == 64 ? run<uint64_t>(c) : run<uint32_t>(c);
}

} // extern "C"
