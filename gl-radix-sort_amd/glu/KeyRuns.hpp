// glu/KeyRuns.hpp -- glu::KeyRuns on MI355X (not in the reference): the runs of equal keys of an array as an offsets array for
// the batched calls of glu::RadixSort, glu::Reduce and glu::BlellochScan.
#ifndef GLU_KEYRUNS_HPP
#define GLU_KEYRUNS_HPP

#include "hip_utils.hpp"

namespace glu
{
    /// The heads of the runs of equal keys (glu_key_runs_run_ptr in glu_hip.h): after a sort by key, the groups.  Everything stays
    /// on the device; the work is enqueued, not waited for.
    class KeyRuns
    {
    public:
        KeyRuns() { GLU_CHECK_STATUS(glu_key_runs_create(&m_impl)); }

        KeyRuns(const KeyRuns&) = delete;
        KeyRuns& operator=(const KeyRuns&) = delete;

        ~KeyRuns() { glu_key_runs_destroy(m_impl); }

        /// Scratch for up to `count` keys of `key_bits` (32 or 64) bits: calls then allocate nothing and can be captured into a graph.
        void prepare(size_t count, uint32_t key_bits = 32) { GLU_CHECK_STATUS(glu_key_runs_prepare(m_impl, count, key_bits)); }

        /// A head is an index i with i == 0 or keys[i] and keys[i - 1] differing in a bit of [begin_bit, end_bit); R = their number.
        /// device_offsets (max_runs + 1 uint32, all written): the heads in ascending order, then `count` in every entry from
        /// min(R, max_runs) on -- the offsets of max_runs segments for the batched calls.  device_unique_keys (max_runs keys, or
        /// nullptr): the whole key at every head.  *device_num_runs = R, also where R > max_runs (the last segment then holds the
        /// remaining runs merged).  The keys are only read.
        void operator()(const void* device_keys, size_t count, uint32_t key_bits, uint32_t begin_bit, uint32_t end_bit,
                        void* device_unique_keys, uint32_t* device_offsets, size_t max_runs, uint32_t* device_num_runs,
                        void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_key_runs_run_ptr(m_impl, device_keys, count, key_bits, begin_bit, end_bit, device_unique_keys,
                                                  device_offsets, max_runs, device_num_runs, stream));
        }

        /// What a call does with `count` keys (glu_key_runs_plan; host only, no device needed).
        struct Plan
        {
            uint32_t tile = 0, tiles = 0, scan_rounds = 0;
        };
        [[nodiscard]] static Plan plan(size_t count, uint32_t key_bits = 32)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_key_runs_plan(count, key_bits, &p.tile, &p.tiles, &p.scan_rounds));
            return p;
        }

    private:
        glu_key_runs m_impl = nullptr;
    };

    /// The arrays of one KeyRuns call, for the compositions Reduce::reduce_by_key and BlellochScan::scan_by_key: the keys with
    /// their bit range and the three outputs (KeyRuns::operator()).  All pointers are device pointers.
    struct KeyRunsArrays
    {
        const void* keys = nullptr;
        size_t count = 0;
        uint32_t key_bits = 32, begin_bit = 0, end_bit = 32;
        void* unique_keys = nullptr; ///< max_runs keys, or nullptr
        uint32_t* offsets = nullptr; ///< max_runs + 1 words, supplied by the caller
        size_t max_runs = 0;         ///< at most 2^24 in a composition (the limit of the batched calls)
        uint32_t* num_runs = nullptr;
    };
} // namespace glu

#endif // GLU_KEYRUNS_HPP
