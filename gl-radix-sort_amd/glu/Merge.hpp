// glu/Merge.hpp -- glu::Merge on MI355X (not in the reference): two sorted arrays of keys, with or without 4-byte values, into one
// sorted array, stable, in the order glu::RadixSort sorts.
#ifndef GLU_MERGE_HPP
#define GLU_MERGE_HPP

#include "hip_utils.hpp"

namespace glu
{
    /// out = the stable sort of the concatenation A || B by the sort's order of keys (floats by their bits: -0.0 < +0.0, NaNs
    /// beyond the infinities); both inputs sorted in that order.  Among equal keys A's elements come first and each side keeps
    /// its order.  Everything stays on the device; the work is enqueued, not waited for (glu_merge_run_ptr in glu_hip.h).
    class Merge
    {
    public:
        Merge() { GLU_CHECK_STATUS(glu_merge_create(&m_impl)); }

        Merge(const Merge&) = delete;
        Merge& operator=(const Merge&) = delete;

        ~Merge() { glu_merge_destroy(m_impl); }

        /// Scratch for calls of up to `total_count` = a_count + b_count keys: they then allocate nothing and can be captured.
        void prepare(size_t total_count, glu_key_type key_type = GLU_KEY_UINT32)
        {
            GLU_CHECK_STATUS(glu_merge_prepare(m_impl, total_count, key_type));
        }

        /// The value pointers are all nullptr (keys only) or all set; out_keys and out_vals hold a_count + b_count elements and
        /// overlap nothing.  The inputs are only read.
        void operator()(const void* device_a_keys, const uint32_t* device_a_vals, size_t a_count, const void* device_b_keys,
                        const uint32_t* device_b_vals, size_t b_count, void* device_out_keys, uint32_t* device_out_vals,
                        glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_merge_run_ptr(m_impl, device_a_keys, device_a_vals, a_count, device_b_keys, device_b_vals, b_count,
                                               device_out_keys, device_out_vals, key_type, stream));
        }

        /// uint32 keys and values in buffers, from their starts.
        void operator()(const ShaderStorageBuffer& a_keys, const ShaderStorageBuffer& a_vals, size_t a_count, const ShaderStorageBuffer& b_keys,
                        const ShaderStorageBuffer& b_vals, size_t b_count, ShaderStorageBuffer& out_keys, ShaderStorageBuffer& out_vals)
        {
            (*this)(a_keys.device_ptr(), (const uint32_t*) a_vals.device_ptr(), a_count, b_keys.device_ptr(),
                    (const uint32_t*) b_vals.device_ptr(), b_count, out_keys.device_ptr(), (uint32_t*) out_vals.device_ptr());
        }

        /// uint32 keys alone in buffers, from their starts.
        void operator()(const ShaderStorageBuffer& a_keys, size_t a_count, const ShaderStorageBuffer& b_keys, size_t b_count,
                        ShaderStorageBuffer& out_keys)
        {
            (*this)(a_keys.device_ptr(), nullptr, a_count, b_keys.device_ptr(), nullptr, b_count, out_keys.device_ptr(), nullptr);
        }

        /// Scratch for batched calls of up to `total_count` = a_total + b_total keys: they then allocate nothing and can be captured.
        void prepare_batch(size_t total_count, glu_key_type key_type = GLU_KEY_UINT32)
        {
            GLU_CHECK_STATUS(glu_merge_prepare_batch(m_impl, total_count, key_type));
        }

        /// The two sorted runs of every segment into one, all segments in one call: segment s is A[a_offsets[s], a_offsets[s + 1])
        /// and B[b_offsets[s], b_offsets[s + 1]) (device arrays of num_segments + 1 words), its output starts at the sum of the
        /// two offsets relative to their first; device_out_offsets (optional) receives those sums
        /// (glu_merge_run_batch_offsets_ptr in glu_hip.h).  One segment with offsets written on the device is the merge whose
        /// counts live on the device.
        void merge_batch_offsets(const void* device_a_keys, const uint32_t* device_a_vals, const uint32_t* device_a_offsets, size_t a_total,
                                 const void* device_b_keys, const uint32_t* device_b_vals, const uint32_t* device_b_offsets, size_t b_total,
                                 size_t num_segments, void* device_out_keys, uint32_t* device_out_vals, uint32_t* device_out_offsets = nullptr,
                                 glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_merge_run_batch_offsets_ptr(m_impl, device_a_keys, device_a_vals, device_a_offsets, a_total, device_b_keys,
                                                             device_b_vals, device_b_offsets, b_total, num_segments, device_out_keys,
                                                             device_out_vals, device_out_offsets, key_type, stream));
        }

        /// The same over equal partitions: a_len keys of A and b_len keys of B per segment (either may be 0).
        void merge_batch(const void* device_a_keys, const uint32_t* device_a_vals, size_t a_len, const void* device_b_keys,
                         const uint32_t* device_b_vals, size_t b_len, size_t num_segments, void* device_out_keys, uint32_t* device_out_vals,
                         uint32_t* device_out_offsets = nullptr, glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_merge_run_batch_ptr(m_impl, device_a_keys, device_a_vals, a_len, device_b_keys, device_b_vals, b_len,
                                                     num_segments, device_out_keys, device_out_vals, device_out_offsets, key_type, stream));
        }

        /// What a call with these counts does (glu_merge_plan; host only, no device needed).
        struct Plan
        {
            uint32_t tile = 0, tiles = 0, kernels = 0;
            size_t scratch_bytes = 0;
        };
        [[nodiscard]] static Plan plan(size_t a_count, size_t b_count, glu_key_type key_type = GLU_KEY_UINT32, bool with_vals = true)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_merge_plan(a_count, b_count, key_type, with_vals ? 1 : 0, &p.tile, &p.tiles, &p.kernels, &p.scratch_bytes));
            return p;
        }

        /// What a batched call of `total_count` = a_total + b_total keys in `num_segments` segments does (glu_merge_plan_batch).
        [[nodiscard]] static Plan plan_batch(size_t total_count, size_t num_segments, glu_key_type key_type = GLU_KEY_UINT32, bool with_vals = true)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_merge_plan_batch(total_count, num_segments, key_type, with_vals ? 1 : 0, &p.tile, &p.tiles, &p.kernels,
                                                  &p.scratch_bytes));
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
            GLU_CHECK_STATUS(glu_merge_last(m_impl, &l.tiles, &l.kernels));
            return l;
        }

    private:
        glu_merge m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_MERGE_HPP
