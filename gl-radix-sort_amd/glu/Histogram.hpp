// glu/Histogram.hpp -- glu::Histogram on MI355X (not in the reference): how many samples fall into each bin, over even bins or over
// sorted bin edges; numpy.histogram, torch.histc and torch.bincount on the device.
#ifndef GLU_HISTOGRAM_HPP
#define GLU_HISTOGRAM_HPP

#include <type_traits>

#include "hip_utils.hpp"

namespace glu
{
    /// out_counts[b] = the samples of bin b, uint32.  Everything stays on the device; the work is enqueued, not waited for
    /// (glu_histogram_run_even_ptr and glu_histogram_run_edges_ptr in glu_hip.h).  The same input gives the same bits every time.
    class Histogram
    {
    public:
        Histogram() { GLU_CHECK_STATUS(glu_histogram_create(&m_impl)); }

        Histogram(const Histogram&) = delete;
        Histogram& operator=(const Histogram&) = delete;

        ~Histogram() { glu_histogram_destroy(m_impl); }

        /// Scratch for calls of up to `count` samples and `bins` bins: they then allocate nothing and can be captured.
        void prepare(size_t count, size_t bins) { GLU_CHECK_STATUS(glu_histogram_prepare(m_impl, count, bins)); }

        /// `bins` even bins over [lo, hi); lo and hi are values of the sample's type (uint32_t, int32_t, float or double) on the
        /// host.  Integers: (hi - lo) / bins must be a whole number, and the bin is exact.  accumulate: add to out_counts.
        template<typename T>
        void even(const T* device_samples, size_t count, T lo, T hi, size_t bins, uint32_t* device_out_counts, bool accumulate = false,
                  void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_histogram_run_even_ptr(m_impl, device_samples, count, key_type_of<T>(), &lo, &hi, bins, device_out_counts,
                                                        accumulate ? 1 : 0, stream));
        }

        /// Bins between `bins + 1` non-decreasing device edges of the sample's type: bin b holds edges[b] <= x < edges[b + 1].
        template<typename T>
        void edges(const T* device_samples, size_t count, const T* device_edges, size_t bins, uint32_t* device_out_counts,
                   bool accumulate = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_histogram_run_edges_ptr(m_impl, device_samples, count, key_type_of<T>(), device_edges, bins,
                                                         device_out_counts, accumulate ? 1 : 0, stream));
        }

        /// out_counts[v] = the ids equal to v, v < bins (ids of `bins` and more are not counted).
        void bincount(const uint32_t* device_ids, size_t count, size_t bins, uint32_t* device_out_counts, bool accumulate = false,
                      void* stream = nullptr)
        {
            even<uint32_t>(device_ids, count, 0u, (uint32_t) bins, bins, device_out_counts, accumulate, stream);
        }

        /// uint32 ids in a buffer, from its start.
        void bincount(const ShaderStorageBuffer& ids, size_t count, size_t bins, ShaderStorageBuffer& out_counts, bool accumulate = false)
        {
            bincount((const uint32_t*) ids.device_ptr(), count, bins, (uint32_t*) out_counts.device_ptr(), accumulate);
        }

        /// Batched histogram (glu_histogram_run_batch_*_ptr in glu_hip.h): out_counts[s * bins + b] = the samples of segment s in
        /// bin b, by the rule of even() / edges(), every segment in one call.  Scratch for batches of up to `total` samples in up
        /// to `num_segments` segments over `bins` bins: they then allocate nothing and can be captured.
        void prepare_batch(size_t total, size_t num_segments, size_t bins)
        {
            GLU_CHECK_STATUS(glu_histogram_prepare_batch(m_impl, total, num_segments, bins));
        }

        /// `num_partitions` adjacent partitions of `count` samples, `bins` even bins over [lo, hi) for all of them.
        template<typename T>
        void even_batch(const T* device_samples, size_t count, size_t num_partitions, T lo, T hi, size_t bins, uint32_t* device_out_counts,
                        bool accumulate = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_histogram_run_batch_even_ptr(m_impl, device_samples, count, num_partitions, key_type_of<T>(), &lo, &hi, bins,
                                                              device_out_counts, accumulate ? 1 : 0, stream));
        }

        /// The segments [offsets[s], offsets[s + 1]) of `total` samples; `device_offsets`: num_segments + 1 uint32, only read.
        template<typename T>
        void even_batch_offsets(const T* device_samples, size_t total, const uint32_t* device_offsets, size_t num_segments, T lo, T hi,
                                size_t bins, uint32_t* device_out_counts, bool accumulate = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_histogram_run_batch_offsets_even_ptr(m_impl, device_samples, total, device_offsets, num_segments,
                                                                      key_type_of<T>(), &lo, &hi, bins, device_out_counts, accumulate ? 1 : 0,
                                                                      stream));
        }

        /// Partitions over the one array of `bins + 1` device edges.
        template<typename T>
        void edges_batch(const T* device_samples, size_t count, size_t num_partitions, const T* device_edges, size_t bins,
                         uint32_t* device_out_counts, bool accumulate = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_histogram_run_batch_edges_ptr(m_impl, device_samples, count, num_partitions, key_type_of<T>(), device_edges, bins,
                                                               device_out_counts, accumulate ? 1 : 0, stream));
        }

        /// Segments of device offsets over the one array of `bins + 1` device edges.
        template<typename T>
        void edges_batch_offsets(const T* device_samples, size_t total, const uint32_t* device_offsets, size_t num_segments,
                                 const T* device_edges, size_t bins, uint32_t* device_out_counts, bool accumulate = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_histogram_run_batch_offsets_edges_ptr(m_impl, device_samples, total, device_offsets, num_segments,
                                                                       key_type_of<T>(), device_edges, bins, device_out_counts,
                                                                       accumulate ? 1 : 0, stream));
        }

        /// out_counts[p * bins + v] = the ids of partition p equal to v, v < bins.
        void bincount_batch(const uint32_t* device_ids, size_t count, size_t num_partitions, size_t bins, uint32_t* device_out_counts,
                            bool accumulate = false, void* stream = nullptr)
        {
            even_batch<uint32_t>(device_ids, count, num_partitions, 0u, (uint32_t) bins, bins, device_out_counts, accumulate, stream);
        }

        /// ... of the segments of device offsets.
        void bincount_batch_offsets(const uint32_t* device_ids, size_t total, const uint32_t* device_offsets, size_t num_segments, size_t bins,
                                    uint32_t* device_out_counts, bool accumulate = false, void* stream = nullptr)
        {
            even_batch_offsets<uint32_t>(device_ids, total, device_offsets, num_segments, 0u, (uint32_t) bins, bins, device_out_counts, accumulate,
                                         stream);
        }

        /// What the last batched call did with its segments (glu_histogram_read_batch; synchronise its stream first).
        struct BatchClasses
        {
            uint32_t wave_segments = 0, block_segments = 0, long_segments = 0;
        };
        [[nodiscard]] BatchClasses read_batch() const
        {
            BatchClasses r;
            GLU_CHECK_STATUS(glu_histogram_read_batch(m_impl, &r.wave_segments, &r.block_segments, &r.long_segments));
            return r;
        }

        /// What a call with these counts does (glu_histogram_plan; host only, no device needed).
        struct Plan
        {
            uint32_t path = 0, threads = 0, tile = 0, groups = 0, kernels = 0;
            size_t scratch_bytes = 0;
        };
        [[nodiscard]] static Plan plan(size_t count, size_t bins, glu_key_type key_type = GLU_KEY_UINT32, int mode = GLU_HISTOGRAM_EVEN)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_histogram_plan(count, bins, key_type, mode, &p.path, &p.threads, &p.tile, &p.groups, &p.kernels, &p.scratch_bytes));
            return p;
        }

        /// What the last call enqueued: the path, the workgroups of the counting kernel and the number of kernels.
        struct Last
        {
            uint32_t path = 0, groups = 0, kernels = 0;
        };
        [[nodiscard]] Last last() const
        {
            Last l;
            GLU_CHECK_STATUS(glu_histogram_last(m_impl, &l.path, &l.groups, &l.kernels));
            return l;
        }

    private:
        template<typename T>
        static constexpr glu_key_type key_type_of()
        {
            static_assert(sizeof(T) == 4 || sizeof(T) == 8, "samples are 4 or 8 bytes wide");
            if constexpr (sizeof(T) == 4)
                return std::is_floating_point<T>::value ? GLU_KEY_FLOAT32 : std::is_signed<T>::value ? GLU_KEY_INT32 : GLU_KEY_UINT32;
            else
                return std::is_floating_point<T>::value ? GLU_KEY_FLOAT64 : std::is_signed<T>::value ? GLU_KEY_INT64 : GLU_KEY_UINT64;
        }

        glu_histogram m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_HISTOGRAM_HPP
