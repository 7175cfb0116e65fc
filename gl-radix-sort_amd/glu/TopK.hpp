// glu/TopK.hpp -- glu::TopK on MI355X (not in the reference): the k smallest or the k largest keys of an array and their indices, by a
// radix select, in the order glu::RadixSort sorts.
#ifndef GLU_TOPK_HPP
#define GLU_TOPK_HPP

#include "hip_utils.hpp"

namespace glu
{
    /// smallest: the first k elements of the stable ascending sort of (key, index); largest: the first k of the stable sort by
    /// descending key, equal keys still by ascending index (floats by their bits: -0.0 < +0.0, NaNs beyond the infinities).  With
    /// `sorted` the outputs come best first, without it in ascending order of the index.  The keys are only read; everything stays on
    /// the device; the work is enqueued, not waited for (glu_top_k_run_ptr in glu_hip.h).
    class TopK
    {
    public:
        TopK() { GLU_CHECK_STATUS(glu_top_k_create(&m_impl)); }

        TopK(const TopK&) = delete;
        TopK& operator=(const TopK&) = delete;

        ~TopK() { glu_top_k_destroy(m_impl); }

        /// Scratch for calls of up to `count` keys and k up to `max_k`: they then allocate nothing and can be captured.
        void prepare(size_t count, size_t max_k, glu_key_type key_type = GLU_KEY_UINT32)
        {
            GLU_CHECK_STATUS(glu_top_k_prepare(m_impl, count, max_k, key_type));
        }

        /// "PATH" (GLU_TOP_K_PATH_AUTO, _CANDIDATES, _FULL) and "CAND_CAPACITY" (0: the default of the count).
        void set_option(const char* name, long long value) { GLU_CHECK_STATUS(glu_top_k_set_option(m_impl, name, value)); }

        /// out_keys and out_indices hold k entries, out_kth one key; each may be nullptr, not all three.
        void smallest(const void* device_keys, size_t count, size_t k, void* device_out_keys, uint32_t* device_out_indices,
                      glu_key_type key_type = GLU_KEY_UINT32, bool sorted = true, void* device_out_kth = nullptr, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_ptr(m_impl, device_keys, key_type, count, k, 0, sorted ? 1 : 0, device_out_keys, device_out_indices,
                                               device_out_kth, stream));
        }
        void largest(const void* device_keys, size_t count, size_t k, void* device_out_keys, uint32_t* device_out_indices,
                     glu_key_type key_type = GLU_KEY_UINT32, bool sorted = true, void* device_out_kth = nullptr, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_ptr(m_impl, device_keys, key_type, count, k, 1, sorted ? 1 : 0, device_out_keys, device_out_indices,
                                               device_out_kth, stream));
        }
        /// The k-th smallest (largest) key alone, one key on the device: an order statistic, no compaction and no ordering.
        void kth(const void* device_keys, size_t count, size_t k, void* device_out_kth, glu_key_type key_type = GLU_KEY_UINT32,
                 bool from_largest = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_ptr(m_impl, device_keys, key_type, count, k, from_largest ? 1 : 0, 0, nullptr, nullptr, device_out_kth,
                                               stream));
        }

        /// uint32 keys in buffers, from their starts.
        void smallest(const ShaderStorageBuffer& keys, size_t count, size_t k, ShaderStorageBuffer& out_keys, ShaderStorageBuffer& out_indices,
                      bool sorted = true)
        {
            smallest(keys.device_ptr(), count, k, out_keys.device_ptr(), (uint32_t*) out_indices.device_ptr(), GLU_KEY_UINT32, sorted);
        }
        void largest(const ShaderStorageBuffer& keys, size_t count, size_t k, ShaderStorageBuffer& out_keys, ShaderStorageBuffer& out_indices,
                     bool sorted = true)
        {
            largest(keys.device_ptr(), count, k, out_keys.device_ptr(), (uint32_t*) out_indices.device_ptr(), GLU_KEY_UINT32, sorted);
        }
        void kth(const ShaderStorageBuffer& keys, size_t count, size_t k, ShaderStorageBuffer& out_kth, bool from_largest = false)
        {
            kth(keys.device_ptr(), count, k, out_kth.device_ptr(), GLU_KEY_UINT32, from_largest);
        }

        /// ---- batched: the k best keys of every segment in one call (glu_top_k_run_batch_ptr / _batch_offsets_ptr in glu_hip.h).
        /// Outputs are rows of stride k; indices are local to the segment; out_kth holds one key per segment.  Each output may be
        /// nullptr, not all three.  With offsets, a segment shorter than k fills only its first min(k, length) entries.
        void prepare_batch(size_t total, size_t num_segments, size_t max_k, glu_key_type key_type = GLU_KEY_UINT32)
        {
            GLU_CHECK_STATUS(glu_top_k_prepare_batch(m_impl, total, num_segments, max_k, key_type));
        }
        void smallest_batch(const void* device_keys, size_t count, size_t num_partitions, size_t k, void* device_out_keys,
                            uint32_t* device_out_indices, glu_key_type key_type = GLU_KEY_UINT32, bool sorted = true,
                            void* device_out_kth = nullptr, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_batch_ptr(m_impl, device_keys, key_type, count, num_partitions, k, 0, sorted ? 1 : 0, device_out_keys,
                                                     device_out_indices, device_out_kth, stream));
        }
        void largest_batch(const void* device_keys, size_t count, size_t num_partitions, size_t k, void* device_out_keys,
                           uint32_t* device_out_indices, glu_key_type key_type = GLU_KEY_UINT32, bool sorted = true,
                           void* device_out_kth = nullptr, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_batch_ptr(m_impl, device_keys, key_type, count, num_partitions, k, 1, sorted ? 1 : 0, device_out_keys,
                                                     device_out_indices, device_out_kth, stream));
        }
        void kth_batch(const void* device_keys, size_t count, size_t num_partitions, size_t k, void* device_out_kth,
                       glu_key_type key_type = GLU_KEY_UINT32, bool from_largest = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_batch_ptr(m_impl, device_keys, key_type, count, num_partitions, k, from_largest ? 1 : 0, 0, nullptr,
                                                     nullptr, device_out_kth, stream));
        }
        /// device_offsets: num_segments + 1 uint32 on the device, as glu::KeyRuns writes them.
        void smallest_batch_offsets(const void* device_keys, size_t total, const uint32_t* device_offsets, size_t num_segments, size_t k,
                                    void* device_out_keys, uint32_t* device_out_indices, glu_key_type key_type = GLU_KEY_UINT32,
                                    bool sorted = true, void* device_out_kth = nullptr, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_batch_offsets_ptr(m_impl, device_keys, key_type, total, device_offsets, num_segments, k, 0,
                                                             sorted ? 1 : 0, device_out_keys, device_out_indices, device_out_kth, stream));
        }
        void largest_batch_offsets(const void* device_keys, size_t total, const uint32_t* device_offsets, size_t num_segments, size_t k,
                                   void* device_out_keys, uint32_t* device_out_indices, glu_key_type key_type = GLU_KEY_UINT32,
                                   bool sorted = true, void* device_out_kth = nullptr, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_batch_offsets_ptr(m_impl, device_keys, key_type, total, device_offsets, num_segments, k, 1,
                                                             sorted ? 1 : 0, device_out_keys, device_out_indices, device_out_kth, stream));
        }
        void kth_batch_offsets(const void* device_keys, size_t total, const uint32_t* device_offsets, size_t num_segments, size_t k,
                               void* device_out_kth, glu_key_type key_type = GLU_KEY_UINT32, bool from_largest = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_top_k_run_batch_offsets_ptr(m_impl, device_keys, key_type, total, device_offsets, num_segments, k,
                                                             from_largest ? 1 : 0, 0, nullptr, nullptr, device_out_kth, stream));
        }
        /// uint32 keys in buffers, from their starts.
        void smallest_batch(const ShaderStorageBuffer& keys, size_t count, size_t num_partitions, size_t k, ShaderStorageBuffer& out_keys,
                            ShaderStorageBuffer& out_indices, bool sorted = true)
        {
            smallest_batch(keys.device_ptr(), count, num_partitions, k, out_keys.device_ptr(), (uint32_t*) out_indices.device_ptr(), GLU_KEY_UINT32,
                           sorted);
        }
        void largest_batch(const ShaderStorageBuffer& keys, size_t count, size_t num_partitions, size_t k, ShaderStorageBuffer& out_keys,
                           ShaderStorageBuffer& out_indices, bool sorted = true)
        {
            largest_batch(keys.device_ptr(), count, num_partitions, k, out_keys.device_ptr(), (uint32_t*) out_indices.device_ptr(), GLU_KEY_UINT32,
                          sorted);
        }
        void smallest_batch_offsets(const ShaderStorageBuffer& keys, size_t total, const ShaderStorageBuffer& offsets, size_t num_segments,
                                    size_t k, ShaderStorageBuffer& out_keys, ShaderStorageBuffer& out_indices, bool sorted = true)
        {
            smallest_batch_offsets(keys.device_ptr(), total, (const uint32_t*) offsets.device_ptr(), num_segments, k, out_keys.device_ptr(),
                                   (uint32_t*) out_indices.device_ptr(), GLU_KEY_UINT32, sorted);
        }
        void largest_batch_offsets(const ShaderStorageBuffer& keys, size_t total, const ShaderStorageBuffer& offsets, size_t num_segments,
                                   size_t k, ShaderStorageBuffer& out_keys, ShaderStorageBuffer& out_indices, bool sorted = true)
        {
            largest_batch_offsets(keys.device_ptr(), total, (const uint32_t*) offsets.device_ptr(), num_segments, k, out_keys.device_ptr(),
                                  (uint32_t*) out_indices.device_ptr(), GLU_KEY_UINT32, sorted);
        }
        /// The segments of the last batched call per class and the kernels it enqueued: synchronise first.
        struct LastBatch
        {
            uint32_t wave_segments = 0, block_segments = 0, long_segments = 0, kernels = 0;
        };
        [[nodiscard]] LastBatch read_batch() const
        {
            LastBatch l;
            GLU_CHECK_STATUS(glu_top_k_read_batch(m_impl, &l.wave_segments, &l.block_segments, &l.long_segments, &l.kernels));
            return l;
        }

        /// What a call with these sizes does (glu_top_k_plan; host only, no device needed).
        struct Plan
        {
            uint32_t rounds = 0, digit_shift[6] = {}, digit_bits[6] = {}, tile = 0, tiles = 0, capacity = 0, kernels = 0;
            size_t scratch_bytes = 0;
        };
        [[nodiscard]] static Plan plan(size_t count, size_t k, glu_key_type key_type = GLU_KEY_UINT32, bool sorted = true, bool with_arrays = true,
                                       int path = GLU_TOP_K_PATH_AUTO, size_t cand_capacity = 0)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_top_k_plan(count, k, key_type, sorted ? 1 : 0, with_arrays ? 1 : 0, path, cand_capacity, &p.rounds, p.digit_shift,
                                            p.digit_bits, &p.tile, &p.tiles, &p.capacity, &p.kernels, &p.scratch_bytes));
            return p;
        }

        /// What the last call did, read back from the device: synchronise first.
        struct Last
        {
            uint32_t path = 0, candidates = 0, ties = 0, kernels = 0;
        };
        [[nodiscard]] Last read_last() const
        {
            Last l;
            GLU_CHECK_STATUS(glu_top_k_read_last(m_impl, &l.path, &l.candidates, &l.ties, &l.kernels));
            return l;
        }

    private:
        glu_top_k m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_TOPK_HPP
