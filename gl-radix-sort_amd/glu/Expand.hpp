// glu/Expand.hpp -- glu::Expand on MI355X (not in the reference): from the offsets of segments to the segment, the rank inside it and
// the segment's item for every element.  The inverse of glu::KeyRuns; numpy.repeat with the counts on the device.
#ifndef GLU_EXPAND_HPP
#define GLU_EXPAND_HPP

#include "hip_utils.hpp"

namespace glu
{
    /// `offsets`: num_segments + 1 non-decreasing uint32 on the device (what glu::KeyRuns writes and the batched operators read).
    /// For every j < total with offsets[0] <= j < offsets[num_segments], s = the last segment with offsets[s] <= j (empty segments
    /// are skipped): out_segments[j] = s, out_ranks[j] = j - offsets[s], out_items[j] = items[s].  Other positions are not
    /// touched.  Everything stays on the device; the work is enqueued, not waited for (glu_expand_run_ptr in glu_hip.h).
    class Expand
    {
    public:
        Expand() { GLU_CHECK_STATUS(glu_expand_create(&m_impl)); }

        Expand(const Expand&) = delete;
        Expand& operator=(const Expand&) = delete;

        ~Expand() { glu_expand_destroy(m_impl); }

        /// Scratch for calls of up to `total` elements and `num_segments` segments: they then allocate nothing and can be captured.
        void prepare(size_t total, size_t num_segments) { GLU_CHECK_STATUS(glu_expand_prepare(m_impl, total, num_segments)); }

        /// Every output may be nullptr; device_items and device_out_items are both nullptr or both set, item_bytes is 4, 8, 16 or
        /// 32.  The outputs hold `total` elements and overlap nothing.  The inputs are only read.
        void operator()(const uint32_t* device_offsets, size_t num_segments, size_t total, const void* device_items, uint32_t item_bytes,
                        void* device_out_items, uint32_t* device_out_segments, uint32_t* device_out_ranks, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_expand_run_ptr(m_impl, device_offsets, num_segments, total, device_items, item_bytes, device_out_items,
                                                device_out_segments, device_out_ranks, stream));
        }

        /// Segments and ranks in buffers, from their starts.
        void operator()(const ShaderStorageBuffer& offsets, size_t num_segments, size_t total, ShaderStorageBuffer& out_segments,
                        ShaderStorageBuffer& out_ranks)
        {
            (*this)((const uint32_t*) offsets.device_ptr(), num_segments, total, nullptr, 0, nullptr, (uint32_t*) out_segments.device_ptr(),
                    (uint32_t*) out_ranks.device_ptr());
        }

        /// out_segments[j] = the segment of element j.
        void segment_ids(const uint32_t* device_offsets, size_t num_segments, size_t total, uint32_t* device_out_segments,
                         void* stream = nullptr)
        {
            (*this)(device_offsets, num_segments, total, nullptr, 0, nullptr, device_out_segments, nullptr, stream);
        }

        /// out_ranks[j] = the index of element j inside its segment.
        void ranks(const uint32_t* device_offsets, size_t num_segments, size_t total, uint32_t* device_out_ranks, void* stream = nullptr)
        {
            (*this)(device_offsets, num_segments, total, nullptr, 0, nullptr, nullptr, device_out_ranks, stream);
        }

        /// out_items[j] = items[the segment of element j]: numpy.repeat, the broadcast of a per-segment result.
        void gather(const uint32_t* device_offsets, size_t num_segments, size_t total, const void* device_items, uint32_t item_bytes,
                    void* device_out_items, void* stream = nullptr)
        {
            (*this)(device_offsets, num_segments, total, device_items, item_bytes, device_out_items, nullptr, nullptr, stream);
        }

        /// What a call with these sizes does (glu_expand_plan; host only, no device needed).
        struct Plan
        {
            uint32_t tile = 0, tiles = 0, kernels = 0;
            size_t scratch_bytes = 0;
        };
        [[nodiscard]] static Plan plan(size_t total, size_t num_segments)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_expand_plan(total, num_segments, &p.tile, &p.tiles, &p.kernels, &p.scratch_bytes));
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
            GLU_CHECK_STATUS(glu_expand_last(m_impl, &l.tiles, &l.kernels));
            return l;
        }

    private:
        glu_expand m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_EXPAND_HPP
