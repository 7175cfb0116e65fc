// glu/Gather.hpp -- glu::Gather on MI355X (not in the reference): items fetched or placed by uint32 indices that live on the
// device.  The step behind every operator that ends in indices: the values of glu::RadixSort and glu::Merge, the out_indices of
// glu::TopK and glu::Select, the positions of glu::SortedSearch.  numpy's items[indices] and out[indices] = items.
#ifndef GLU_GATHER_HPP
#define GLU_GATHER_HPP

#include "hip_utils.hpp"

namespace glu
{
    /// Items are 4, 8, 16 or 32 bytes and are copied bit for bit; `items` and `out` are aligned to min(item_bytes, 16), the inputs
    /// are only read, and `out` overlaps none of them.  No index is trusted: an entry whose index is out of range is skipped and the
    /// entry of `out` it would have written is not touched.  The object owns no device memory: every call is allocation-free, can
    /// be captured, and is enqueued, not waited for (the gather section of glu_hip.h).
    class Gather
    {
    public:
        Gather() { GLU_CHECK_STATUS(glu_gather_create(&m_impl)); }

        Gather(const Gather&) = delete;
        Gather& operator=(const Gather&) = delete;

        ~Gather() { glu_gather_destroy(m_impl); }

        /// out[j] = items[indices[j]] for j < count, wherever indices[j] < item_count.
        void operator()(const void* device_items, size_t item_count, uint32_t item_bytes, const uint32_t* device_indices, size_t count,
                        void* device_out, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_gather_run_ptr(m_impl, device_items, item_count, item_bytes, device_indices, count, device_out, stream));
        }

        /// The same over buffers, from their starts.
        void operator()(const ShaderStorageBuffer& items, size_t item_count, uint32_t item_bytes, const ShaderStorageBuffer& indices,
                        size_t count, ShaderStorageBuffer& out)
        {
            (*this)((const void*) items.device_ptr(), item_count, item_bytes, (const uint32_t*) indices.device_ptr(), count,
                    (void*) out.device_ptr());
        }

        /// Rows of stride k of indices local to equal partitions of `count` items, what glu::TopK's batched call writes:
        /// out[s * k + j] = items[s * count + indices[s * k + j]] for j < min(k, count).
        void batch(const void* device_items, uint32_t item_bytes, size_t count, size_t num_partitions, const uint32_t* device_indices,
                   size_t k, void* device_out, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_gather_run_batch_ptr(m_impl, device_items, item_bytes, count, num_partitions, device_indices, k, device_out,
                                                      stream));
        }

        /// ... local to the segments [offsets[s], offsets[s + 1]) of num_segments + 1 uint32 on the device:
        /// out[s * k + j] = items[offsets[s] + indices[s * k + j]] for j < min(k, the segment's length).
        void batch_offsets(const void* device_items, uint32_t item_bytes, size_t total, const uint32_t* device_offsets, size_t num_segments,
                           const uint32_t* device_indices, size_t k, void* device_out, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_gather_run_batch_offsets_ptr(m_impl, device_items, item_bytes, total, device_offsets, num_segments,
                                                              device_indices, k, device_out, stream));
        }

        /// out[indices[j]] = items[j] for j < count, wherever indices[j] < out_count.  The indices are expected to be distinct.
        void scatter(const void* device_items, uint32_t item_bytes, const uint32_t* device_indices, size_t count, void* device_out,
                     size_t out_count, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_gather_scatter_ptr(m_impl, device_items, item_bytes, device_indices, count, device_out, out_count, stream));
        }

        /// What a call over `count` entries does (glu_gather_plan; host only, no device needed).
        struct Plan
        {
            uint32_t tile = 0, tiles = 0, kernels = 0;
        };
        [[nodiscard]] static Plan plan(size_t count, uint32_t item_bytes)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_gather_plan(count, item_bytes, &p.tile, &p.tiles, &p.kernels));
            return p;
        }

        /// What the last call enqueued: the tiles and the number of kernels.
        struct Last
        {
            uint32_t tiles = 0, kernels = 0;
        };
        [[nodiscard]] Last last() const
        {
            Last l;
            GLU_CHECK_STATUS(glu_gather_last(m_impl, &l.tiles, &l.kernels));
            return l;
        }

    private:
        glu_gather m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_GATHER_HPP
