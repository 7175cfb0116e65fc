// glu_key_runs.hip -- key runs of libglu_hip.so (key_runs_kernels.hpp): glu_key_runs_create, glu_key_runs_destroy,
// glu_key_runs_prepare, glu_key_runs_run_ptr, glu_key_runs_plan; and the launch of the count scan that key runs and select share
// (glu_tile_host.hpp).
// The library's other translation units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "glu_key_runs_object.hpp"
#include "key_runs_kernels.hpp"
#include "tile_count_scan_kernel.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
glu_status check_count(size_t count) { return check_tile_count(count, "key runs take fewer than 2^32 keys"); }

glu_status check_key_bits(uint32_t key_bits)
{
    return key_bits == 32 || key_bits == 64 ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "key_bits must be 32 or 64 (got %u)", key_bits);
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
    KeyRunsArgs<K> a;
    a.keys = tile_span<K, kKeyRunsPacks>(c.keys, c.count);
    const uint32_t width = c.end_bit - c.begin_bit;
    a.mask = width == 0 ? (K) 0 : (K) ((width >= 8 * sizeof(K) ? ~(K) 0 : (((K) 1 << width) - 1)) << c.begin_bit);
    const uint32_t tiles = a.keys.tiles;
    uint32_t* tile_counts = (uint32_t*) c.runs->tile_counts.ptr;
    hipLaunchKernelGGL((key_runs_count_kernel<K>), dim3(tile_grid(tiles)), dim3(kTileThreads), 0, c.stream, a, tile_counts);
    HIP_TRY(hipGetLastError());
    GLU_TRY(launch_tile_count_scan(tile_counts, tiles, c.num_runs, c.stream));
    // (the fill: a workgroup per 4096 entries of offsets, if the tiles ask for fewer)
    const uint32_t fill_blocks = tile_grid((uint32_t) ((c.max_runs + 1 + 4095) / 4096));
    hipLaunchKernelGGL((key_runs_write_kernel<K>), dim3(std::max(fill_blocks, tile_grid(tiles))), dim3(kTileThreads), 0, c.stream, a,
                       (const uint32_t*) tile_counts, (const uint32_t*) c.num_runs, (K*) c.unique_keys, c.offsets, (uint32_t) c.max_runs);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}
} // namespace

glu_status glu_hip::host::launch_tile_count_scan(uint32_t* tile_counts, uint32_t tiles, uint32_t* total, hipStream_t stream, uint32_t most)
{
    hipLaunchKernelGGL(key_runs_scan_kernel, dim3(1), dim3(kSbThreads), 0, stream, tile_counts, tiles, total, most);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

extern "C" {

glu_status glu_key_runs_plan(size_t count, uint32_t key_bits, uint32_t* tile, uint32_t* tiles, uint32_t* scan_rounds)
{
    GLU_TRY(check_key_bits(key_bits));
    GLU_TRY(check_count(count));
    const TilePlan p = tile_plan(count, key_bits / 8, kKeyRunsPacks);
    store(tile, p.tile);
    store(tiles, p.tiles);
    store(scan_rounds, p.scan_rounds);
    return GLU_OK;
}

glu_status glu_key_runs_create(glu_key_runs* out) { return create_object(out); }

glu_status glu_key_runs_destroy(glu_key_runs runs) { return destroy_object(runs); }

glu_status glu_key_runs_prepare(glu_key_runs runs, size_t count, uint32_t key_bits)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(runs, "runs"));
    GLU_TRY(check_key_bits(key_bits));
    GLU_TRY(check_count(count));
    return runs->tile_counts.reserve(count, key_bits / 8, kKeyRunsPacks);
}

glu_status glu_key_runs_run_ptr(glu_key_runs runs, const void* keys, size_t count, uint32_t key_bits, uint32_t begin_bit,
                                uint32_t end_bit, void* unique_keys, uint32_t* offsets, size_t max_runs, uint32_t* num_runs, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(runs, "runs"));
    GLU_TRY(check_key_bits(key_bits));
    GLU_TRY(check_count(count));
    GLU_TRY(check_below_2_32(max_runs, "max_runs"));
    if (begin_bit > end_bit || end_bit > key_bits)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid bit range [%u, %u) of %u-bit keys", begin_bit, end_bit, key_bits);
    if (count && !keys) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid key buffer");
    if (!offsets) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid offsets array");
    if (!num_runs) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid num_runs pointer");
    const size_t key_bytes = key_bits / 8;
    GLU_TRY(check_aligned(keys, key_bytes, "keys", "the key size"));
    GLU_TRY(check_aligned(unique_keys, key_bytes, "unique_keys", "the key size"));
    GLU_TRY(check_aligned(offsets, sizeof(uint32_t), "the offsets array", "its element size"));
    GLU_TRY(check_aligned_4(num_runs, "num_runs"));
    // (the outputs are not held against each other)
    GLU_TRY(check_disjoint({{offsets, (max_runs + 1) * sizeof(uint32_t), "the offsets array"}, {unique_keys, max_runs * key_bytes, "unique_keys"},
                            {num_runs, sizeof(uint32_t), "num_runs"}},
                           {{keys, count * key_bytes, "keys"}}));
    GLU_TRY(runs->tile_counts.reserve(count, key_bits / 8, kKeyRunsPacks));
    const Call c{runs, keys, count, begin_bit, end_bit, unique_keys, offsets, max_runs, num_runs, pick_stream(stream)};
    return key_bits == 64 ? run<uint64_t>(c) : run<uint32_t>(c);
}

} // extern "C"
