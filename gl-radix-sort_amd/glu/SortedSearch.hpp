// glu/SortedSearch.hpp -- glu::SortedSearch on MI355X (not in the reference): the lower and the upper bound of many needles in a
// sorted haystack -- numpy.searchsorted on the device, in the order glu::RadixSort sorts.
#ifndef GLU_SORTEDSEARCH_HPP
#define GLU_SORTEDSEARCH_HPP

#include "hip_utils.hpp"

namespace glu
{
    enum SearchPath
    {
        SearchPath_Auto = GLU_SEARCH_PATH_AUTO,
        SearchPath_Direct = GLU_SEARCH_PATH_DIRECT,
        SearchPath_Indexed = GLU_SEARCH_PATH_INDEXED,
        SearchPath_Batch = GLU_SEARCH_PATH_BATCH ///< what last() reports after a batched call; not a path to set
    };

    /// lower[j] = the keys of the haystack below needles[j], upper[j] = the keys not above it, in the sort's order (floats by
    /// their bits: -0.0 < +0.0, NaNs beyond the infinities).  Everything stays on the device; the work is enqueued, not waited for
    /// (glu_sorted_search_run_ptr in glu_hip.h).
    class SortedSearch
    {
    public:
        SortedSearch() { GLU_CHECK_STATUS(glu_sorted_search_create(&m_impl)); }

        SortedSearch(const SortedSearch&) = delete;
        SortedSearch& operator=(const SortedSearch&) = delete;

        ~SortedSearch() { glu_sorted_search_destroy(m_impl); }

        /// Scratch for the index of `hay_count` keys: calls then allocate nothing and can be captured into a graph.
        void prepare(size_t hay_count, glu_key_type key_type = GLU_KEY_UINT32)
        {
            GLU_CHECK_STATUS(glu_sorted_search_prepare(m_impl, hay_count, key_type));
        }

        /// Auto (the default) chooses from the two counts; Indexed on a haystack too short for an index still runs Direct.
        void set_path(SearchPath path) { GLU_CHECK_STATUS(glu_sorted_search_set_option(m_impl, "PATH", path)); }

        /// "PATH" or "TOP_ENTRIES" (glu_sorted_search_set_option).
        void set_option(const char* name, long long value) { GLU_CHECK_STATUS(glu_sorted_search_set_option(m_impl, name, value)); }

        /// Builds the index of a haystack that will be searched again and again (operator() with reuse_index = true).
        void index(const void* device_hay, size_t hay_count, glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_sorted_search_index_ptr(m_impl, device_hay, hay_count, key_type, stream));
        }

        /// device_lower and device_upper: needle_count words each, either may be nullptr.  reuse_index: the caller's promise that
        /// the haystack is the one index() (or the last indexed call) saw, unchanged.
        void operator()(const void* device_hay, size_t hay_count, const void* device_needles, size_t needle_count, glu_key_type key_type,
                        uint32_t* device_lower, uint32_t* device_upper, bool reuse_index = false, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_sorted_search_run_ptr(m_impl, device_hay, hay_count, device_needles, needle_count, key_type, device_lower,
                                                       device_upper, reuse_index ? 1 : 0, stream));
        }

        /// lower only: the first position at which a needle could be inserted (std::lower_bound)
        void lower_bound(const void* device_hay, size_t hay_count, const void* device_needles, size_t needle_count, glu_key_type key_type,
                         uint32_t* device_lower, void* stream = nullptr)
        {
            (*this)(device_hay, hay_count, device_needles, needle_count, key_type, device_lower, nullptr, false, stream);
        }

        /// upper only: the last position at which a needle could be inserted (std::upper_bound)
        void upper_bound(const void* device_hay, size_t hay_count, const void* device_needles, size_t needle_count, glu_key_type key_type,
                         uint32_t* device_upper, void* stream = nullptr)
        {
            (*this)(device_hay, hay_count, device_needles, needle_count, key_type, nullptr, device_upper, false, stream);
        }

        /// both: hay[lower[j] .. upper[j]) are the copies of needles[j] (std::equal_range); a needle is present iff upper > lower
        void equal_range(const void* device_hay, size_t hay_count, const void* device_needles, size_t needle_count, glu_key_type key_type,
                         uint32_t* device_lower, uint32_t* device_upper, void* stream = nullptr)
        {
            (*this)(device_hay, hay_count, device_needles, needle_count, key_type, device_lower, device_upper, false, stream);
        }

        /// Batched, equal partitions: row p of `needle_count` needles searched in row p of `hay_count` keys, num_partitions rows in
        /// one kernel.  Positions are local to the row (torch.searchsorted on 2-D tensors).  device_lower and device_upper:
        /// num_partitions * needle_count words each, either may be nullptr.  No scratch: capturable from the first call
        /// (glu_sorted_search_run_batch_ptr).
        void search_batch(const void* device_hay, size_t hay_count, const void* device_needles, size_t needle_count, size_t num_partitions,
                          glu_key_type key_type, uint32_t* device_lower, uint32_t* device_upper, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_sorted_search_run_batch_ptr(m_impl, device_hay, hay_count, device_needles, needle_count, num_partitions, key_type,
                                                             device_lower, device_upper, stream));
        }

        /// Batched, device offsets: the needles [needle_offsets[s], needle_offsets[s + 1]) searched in the haystack
        /// [hay_offsets[s], hay_offsets[s + 1]); both arrays hold num_segments + 1 device words, as glu::KeyRuns writes them.
        /// device_needle_offsets nullptr: equal rows of needle_total / num_segments needles.  Positions are local to the segment
        /// (glu_sorted_search_run_batch_offsets_ptr).
        void search_batch_offsets(const void* device_hay, size_t hay_total, const uint32_t* device_hay_offsets, const void* device_needles,
                                  size_t needle_total, const uint32_t* device_needle_offsets, size_t num_segments, glu_key_type key_type,
                                  uint32_t* device_lower, uint32_t* device_upper, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_sorted_search_run_batch_offsets_ptr(m_impl, device_hay, hay_total, device_hay_offsets, device_needles, needle_total,
                                                                     device_needle_offsets, num_segments, key_type, device_lower, device_upper,
                                                                     stream));
        }

        /// lower only, per row (torch.searchsorted(sorted, values, right=False))
        void lower_bound_batch(const void* device_hay, size_t hay_count, const void* device_needles, size_t needle_count, size_t num_partitions,
                               glu_key_type key_type, uint32_t* device_lower, void* stream = nullptr)
        {
            search_batch(device_hay, hay_count, device_needles, needle_count, num_partitions, key_type, device_lower, nullptr, stream);
        }

        /// upper only, per row (torch.searchsorted(sorted, values, right=True); the sample of a row's CDF)
        void upper_bound_batch(const void* device_hay, size_t hay_count, const void* device_needles, size_t needle_count, size_t num_partitions,
                               glu_key_type key_type, uint32_t* device_upper, void* stream = nullptr)
        {
            search_batch(device_hay, hay_count, device_needles, needle_count, num_partitions, key_type, nullptr, device_upper, stream);
        }

        /// The most keys of a tile's haystacks that the batched calls stage in LDS: 0 (never), 16 .. 32768 / key bytes, or
        /// GLU_SEARCH_BATCH_WINDOW_DEFAULT, the maximum of the call's key width.  It never changes a result.
        void set_batch_window(uint32_t keys) { GLU_CHECK_STATUS(glu_sorted_search_set_batch_window(m_impl, keys)); }

        /// What a batched call over `needle_total` needles does (glu_sorted_search_plan_batch; host only, no device needed).
        struct BatchPlan
        {
            uint32_t tile = 0, tiles = 0, window_keys = 0, kernels = 0;
        };
        [[nodiscard]] static BatchPlan plan_batch(size_t needle_total, glu_key_type key_type = GLU_KEY_UINT32,
                                                  uint32_t window_keys = GLU_SEARCH_BATCH_WINDOW_DEFAULT)
        {
            BatchPlan p;
            GLU_CHECK_STATUS(glu_sorted_search_plan_batch(needle_total, key_type, window_keys, &p.tile, &p.tiles, &p.window_keys, &p.kernels));
            return p;
        }

        /// What a call with these counts does on the Auto path (glu_sorted_search_plan; host only, no device needed).
        struct Plan
        {
            uint32_t path = 0, levels = 0, fanout = 0;
            size_t index_bytes = 0;
        };
        [[nodiscard]] static Plan plan(size_t hay_count, size_t needle_count, glu_key_type key_type = GLU_KEY_UINT32, uint32_t top_entries = 0)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_sorted_search_plan(hay_count, needle_count, key_type, top_entries, &p.path, &p.levels, &p.fanout, &p.index_bytes));
            return p;
        }

        /// What the last call enqueued: the path taken, the levels of the index used, the number of kernels.
        struct Last
        {
            uint32_t path = 0, levels = 0, kernels = 0;
        };
        [[nodiscard]] Last last() const
        {
            Last l;
            GLU_CHECK_STATUS(glu_sorted_search_last(m_impl, &l.path, &l.levels, &l.kernels));
            return l;
        }

    private:
        glu_sorted_search m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_SORTEDSEARCH_HPP
