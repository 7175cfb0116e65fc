// glu_batch_host.hpp -- what the translation units of the batched operators (glu_sort_batch.hip, glu_reduce_batch.hip,
// glu_scan_batch.hip) share on the host side: the limits of a batch and their checks, the list image of a call with device offsets
// (batch_lists.hpp: a line of counts, then the lists), the grid of the short lists, and what a call leaves for *_read_batch.
#pragma once

#include <algorithm>

#include "batch_lists.hpp"
#include "glu_host.hpp"

namespace glu_hip
{
namespace host
{
constexpr size_t kBatchMaxSegments = (size_t) 1 << 24;
constexpr uint32_t kBatchCountWords = 64; // the list counts (kBatchCounts words) in front of the lists, on a line of their own
static_assert(kBatchCounts <= (int) kBatchCountWords, "the counts fit their line");
inline uint32_t cus() { return (uint32_t) g_dev.num_cus; }

inline glu_status check_batch_total(size_t total)
{
    return total < ((size_t) 1 << 32) ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "a batch must hold fewer than 2^32 elements (got %zu)", total);
}

inline glu_status check_batch_segments(size_t num_segments)
{
    return num_segments <= kBatchMaxSegments ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "num_segments %zu exceeds 2^24", num_segments);
}

inline glu_status check_batch_offsets(const uint32_t* offsets, size_t num_segments)
{
    if (num_segments && !offsets) return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid offsets array");
    return check_aligned(offsets, sizeof(uint32_t), "the offsets array", "its element size");
}

// the list image of a batch, reserved: the line of counts, then the lists of `layout`
inline glu_status reserve_batch_lists(Scratch& image, const BatchClasses& cls, size_t total, size_t num_segments, BatchListsLayout& layout)
{
    size_t words;
    layout = batch_lists_layout(cls, total, num_segments, words);
    return image.reserve((kBatchCountWords + words) * sizeof(uint32_t));
}

// The head of a call with device offsets: the image reserved, its counts cleared on `stream`; where the counts and the lists lie,
// and the grid of the binning kernel (256 segments per workgroup and round).
inline glu_status begin_batch_offsets(Scratch& image, const BatchClasses& cls, size_t total, size_t num_segments, hipStream_t stream,
                                      BatchListsLayout& layout, uint32_t*& counts, uint32_t*& lists, uint32_t& bin_grid)
{
    GLU_TRY(reserve_batch_lists(image, cls, total, num_segments, layout));
    counts = (uint32_t*) image.ptr;
    lists = counts + kBatchCountWords;
    HIP_TRY(hipMemsetAsync(counts, 0, kBatchCountWords * sizeof(uint32_t), stream));
    bin_grid = std::min<uint32_t>((uint32_t) ((num_segments + 255) / 256), cus() * 4u);
    return GLU_OK;
}

// Workgroups per short list of the kernels that walk BATCH_LIST_SHORT4 / 16 / 64 with a third of their grid each (the reduce's and
// the scan's wave kernels, `waves` waves per workgroup): a workgroup's waves hold 16 / 4 / 1 segments of the three lists at a time.
inline uint32_t short_lists_blocks(const BatchListsLayout& layout, uint32_t waves)
{
    uint32_t blocks = 1;
    for (int s = BATCH_LIST_SHORT4; s <= BATCH_LIST_SHORT64; s++)
    {
        const uint32_t per_block = waves * (s == BATCH_LIST_SHORT4 ? 16u : s == BATCH_LIST_SHORT16 ? 4u : 1u);
        blocks = std::max<uint32_t>(blocks, (uint32_t) (((uint64_t) layout.capacity[s] + per_block - 1) / per_block));
    }
    return std::min<uint32_t>(blocks, cus() * 8u);
}

// Segments per class (wave, workgroup, long) of an object's last batched call: the host's own numbers where it chose the class
// (equal partitions), else the counts the binning kernel left in the list image.
struct LastBatch
{
    uint32_t by_class[3] = {0, 0, 0};
    bool on_device = false;

    void reset() { *this = LastBatch(); }

    // the first `wave_lists` of the four bounded lists are the operator's wave class, the others its workgroup class
    glu_status read(const Scratch& image, int wave_lists, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments) const
    {
        uint32_t out[3] = {by_class[0], by_class[1], by_class[2]};
        if (on_device)
        {
            uint32_t counts[kBatchCounts];
            HIP_TRY(hipMemcpy(counts, image.ptr, sizeof(counts), hipMemcpyDeviceToHost));
            out[0] = out[1] = 0;
            for (int c = 0; c < BATCH_LIST_LONG; c++) out[c < wave_lists ? 0 : 1] += counts[c];
            out[2] = counts[kBatchCountLong];
        }
        store(wave_segments, out[0]);
        store(block_segments, out[1]);
        store(long_segments, out[2]);
        return GLU_OK;
    }
};
} // namespace host
} // namespace glu_hip
