// glu/BlellochScan.hpp -- glu::BlellochScan on MI355X (drop-in for reference glu/BlellochScan.hpp:80-191).
#ifndef GLU_BLELLOCHSCAN_HPP
#define GLU_BLELLOCHSCAN_HPP

#include "KeyRuns.hpp"
#include "data_types.hpp"
#include "hip_utils.hpp"

namespace glu
{
    /// Exclusive prefix sum (`+`, identity 0), in place, over `num_partitions` adjacent partitions of `count`
    /// elements each.  Keeps the reference's name although the device algorithm is a chunked
    /// reduce-then-scan rather than Blelloch's up/down sweep; results are identical for integer types.
    /// The batched forms below scan segments given by device offsets, and with an operator and a kind also inclusively, with
    /// Reduce's other operators, and into a second array.
    class BlellochScan
    {
    public:
        explicit BlellochScan(DataType data_type) :
            m_data_type(data_type)
        {
            GLU_CHECK_STATUS(glu_scan_create(static_cast<glu_data_type>(data_type), &m_impl));
        }

        BlellochScan(const BlellochScan&) = delete;
        BlellochScan& operator=(const BlellochScan&) = delete;

        ~BlellochScan() { glu_scan_destroy(m_impl); }

        /// @param buffer the buffer to scan
        /// @param count elements per partition (must be a power of 2, as in the reference)
        /// @param num_partitions number of adjacent partitions
        void operator()(GLuint buffer, size_t count, size_t num_partitions = 1)
        {
            GLU_CHECK_ARGUMENT(buffer, "Invalid buffer");
            GLU_CHECK_ARGUMENT(count > 0, "Count must be greater than zero");
            GLU_CHECK_ARGUMENT(is_power_of_2(count), "Count must be a power of 2");
            GLU_CHECK_ARGUMENT(num_partitions >= 1, "Num of partitions must be >= 1");
            GLU_CHECK_STATUS(glu_scan_run(m_impl, buffer, count, num_partitions));
        }

        /// Native form: raw device pointer + hipStream_t; any count > 0 is accepted.
        void operator()(void* device_data, size_t count, size_t num_partitions, void* stream)
        {
            GLU_CHECK_STATUS(glu_scan_run_ptr(m_impl, device_data, count, num_partitions, stream));
        }

        /// Batched scan (not in the reference; glu_scan_run_batch_offsets_ptr in glu_hip.h): elements [offsets[s], offsets[s + 1])
        /// of the array of `total` elements become their own exclusive scan, in place, for every s < num_segments, in one
        /// asynchronous launch sequence.  device_offsets is a DEVICE array of num_segments + 1 non-decreasing uint32 and is not
        /// read by the host; elements outside the segments are not touched.
        void scan_batch_offsets(void* device_data, size_t total, const uint32_t* device_offsets, size_t num_segments, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_scan_run_batch_offsets_ptr(m_impl, device_data, total, device_offsets, num_segments, stream));
        }
        /// The batched scan with any of Reduce's operators, exclusive or inclusive (glu_scan_run_batch_offsets_op_ptr in
        /// glu_hip.h): device_out receives the scan of every segment of device_data at the same positions and is not touched
        /// outside the segments; nullptr or device_data itself: in place.  Otherwise device_data is only read, and the two arrays
        /// of `total` elements must not overlap.  The identities of an exclusive scan are Reduce's: 0, 1, the type's largest
        /// value (+infinity) for Min, its lowest (-infinity) for Max.
        void scan_batch_offsets(const void* device_data, void* device_out, size_t total, const uint32_t* device_offsets, size_t num_segments,
                                glu_reduce_operator op, glu_scan_kind kind, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_scan_run_batch_offsets_op_ptr(m_impl, device_data, device_out, total, device_offsets, num_segments, op, kind, stream));
        }
        /// The scan of a whole array of `total` (< 2^32) elements as one segment, no offsets array needed: cumsum, cumprod,
        /// cummin and cummax.  Capturable after prepare_batch(total, 1).
        void inclusive_scan(const void* device_data, void* device_out, size_t total, glu_reduce_operator op, void* stream = nullptr)
        {
            scan_batch_offsets(device_data, device_out, total, nullptr, 1, op, GLU_SCAN_INCLUSIVE, stream);
        }
        void exclusive_scan(const void* device_data, void* device_out, size_t total, glu_reduce_operator op, void* stream = nullptr)
        {
            scan_batch_offsets(device_data, device_out, total, nullptr, 1, op, GLU_SCAN_EXCLUSIVE, stream);
        }
        /// Scan by key (KeyRuns.hpp): the runs of `k.keys` taken by `runs`, then the values of every run replaced by their own
        /// exclusive scan, in place -- the two calls, on the caller's stream, with nothing between them.  device_values: k.count
        /// elements of the data type.
        void scan_by_key(KeyRuns& runs, const KeyRunsArrays& k, void* device_values, void* stream = nullptr)
        {
            GLU_CHECK_ARGUMENT(k.max_runs <= ((size_t) 1 << 24), "scan_by_key: max_runs %zu exceeds 2^24", k.max_runs);
            runs(k.keys, k.count, k.key_bits, k.begin_bit, k.end_bit, k.unique_keys, k.offsets, k.max_runs, k.num_runs, stream);
            scan_batch_offsets(device_values, k.count, k.offsets, k.max_runs, stream);
        }
        /// Scan by key with an operator and a kind: a running maximum, minimum, sum or product per run of keys, stored to
        /// device_out (nullptr: in place, over device_values).
        void scan_by_key(KeyRuns& runs, const KeyRunsArrays& k, const void* device_values, glu_reduce_operator op, glu_scan_kind kind,
                         void* device_out = nullptr, void* stream = nullptr)
        {
            GLU_CHECK_ARGUMENT(k.max_runs <= ((size_t) 1 << 24), "scan_by_key: max_runs %zu exceeds 2^24", k.max_runs);
            runs(k.keys, k.count, k.key_bits, k.begin_bit, k.end_bit, k.unique_keys, k.offsets, k.max_runs, k.num_runs, stream);
            scan_batch_offsets(device_values, device_out, k.count, k.offsets, k.max_runs, op, kind, stream);
        }
        /// Scratch for batched scans of up to `total` elements in up to `num_segments` segments (they then allocate nothing and
        /// can be captured into a graph).
        void prepare_batch(size_t total, size_t num_segments) { GLU_CHECK_STATUS(glu_scan_prepare_batch(m_impl, total, num_segments)); }
        /// Segments each path of the last batched call took (glu_scan_read_batch; synchronise its stream first).
        struct BatchReport
        {
            uint32_t wave_segments = 0, block_segments = 0, long_segments = 0;
        };
        [[nodiscard]] BatchReport read_batch() const
        {
            BatchReport r;
            GLU_CHECK_STATUS(glu_scan_read_batch(m_impl, &r.wave_segments, &r.block_segments, &r.long_segments));
            return r;
        }

        [[nodiscard]] DataType data_type() const { return m_data_type; }

    private:
        const DataType m_data_type;
        glu_scan m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_BLELLOCHSCAN_HPP
