// glu/Reduce.hpp -- glu::Reduce on MI355X (drop-in for reference glu/Reduce.hpp:42-136).
#ifndef GLU_REDUCE_HPP
#define GLU_REDUCE_HPP

#include "KeyRuns.hpp"
#include "data_types.hpp"
#include "hip_utils.hpp"

namespace glu
{
    /// The operators that can be used for the reduction (reference glu/Reduce.hpp:42-48).
    enum ReduceOperator
    {
        ReduceOperator_Sum = GLU_REDUCE_SUM,
        ReduceOperator_Mul = GLU_REDUCE_MUL,
        ReduceOperator_Min = GLU_REDUCE_MIN,
        ReduceOperator_Max = GLU_REDUCE_MAX
    };

    /// In-place reduction: after `reduce(buffer, count)` element 0 of the buffer holds the (component-wise)
    /// sum / product / min / max of elements [0, count).  The work is enqueued, not waited for.
    class Reduce
    {
    public:
        explicit Reduce(DataType data_type, ReduceOperator operator_) :
            m_data_type(data_type),
            m_operator(operator_)
        {
            GLU_CHECK_STATUS(glu_reduce_create(static_cast<glu_data_type>(data_type),
                                               static_cast<glu_reduce_operator>(operator_), &m_impl));
        }

        Reduce(const Reduce&) = delete;
        Reduce& operator=(const Reduce&) = delete;

        ~Reduce() { glu_reduce_destroy(m_impl); }

        void operator()(GLuint buffer, size_t count)
        {
            GLU_CHECK_ARGUMENT(buffer, "Invalid buffer");
            GLU_CHECK_ARGUMENT(count > 0, "Count must be greater than zero");
            GLU_CHECK_STATUS(glu_reduce_run(m_impl, buffer, count));
        }

        /// Native form: raw device pointer + hipStream_t (nullptr = the library queue).
        void operator()(void* device_data, size_t count, void* stream)
        {
            GLU_CHECK_STATUS(glu_reduce_run_ptr(m_impl, device_data, count, stream));
        }

        /// Batched reduce (not in the reference; glu_reduce_run_batch_ptr in glu_hip.h): `num_partitions` adjacent partitions of
        /// `count` elements each -- the shape of BlellochScan::operator() -- device_out[p] = the reduction of partition p, in one
        /// asynchronous launch sequence.  Unlike operator() it only READS device_data; device_out (num_partitions elements of the
        /// data type) must not overlap it.  An empty partition yields the operator's identity.
        void reduce_batch(const void* device_data, void* device_out, size_t count, size_t num_partitions, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_reduce_run_batch_ptr(m_impl, device_data, device_out, count, num_partitions, stream));
        }
        /// The same for segments of any lengths: device_out[s] = the reduction of elements [offsets[s], offsets[s + 1]) of the
        /// array of `total` elements; device_offsets is a DEVICE array of num_segments + 1 non-decreasing uint32 and is not read
        /// by the host.
        void reduce_batch_offsets(const void* device_data, void* device_out, size_t total, const uint32_t* device_offsets,
                                  size_t num_segments, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_reduce_run_batch_offsets_ptr(m_impl, device_data, device_out, total, device_offsets, num_segments, stream));
        }
        /// Reduce by key (KeyRuns.hpp): the runs of `k.keys` taken by `runs`, then device_out[r] = the reduction of the values of
        /// run r, for r < k.max_runs (the operator's identity from the number of runs on) -- the two calls, on the caller's
        /// stream, with nothing between them.  device_values: k.count elements of the data type, only read.
        void reduce_by_key(KeyRuns& runs, const KeyRunsArrays& k, const void* device_values, void* device_out, void* stream = nullptr)
        {
            GLU_CHECK_ARGUMENT(k.max_runs <= ((size_t) 1 << 24), "reduce_by_key: max_runs %zu exceeds 2^24", k.max_runs);
            runs(k.keys, k.count, k.key_bits, k.begin_bit, k.end_bit, k.unique_keys, k.offsets, k.max_runs, k.num_runs, stream);
            reduce_batch_offsets(device_values, device_out, k.count, k.offsets, k.max_runs, stream);
        }
        /// Scratch for batched reduces of up to `total` elements in up to `num_segments` segments (they then allocate nothing and
        /// can be captured into a graph).
        void prepare_batch(size_t total, size_t num_segments) { GLU_CHECK_STATUS(glu_reduce_prepare_batch(m_impl, total, num_segments)); }
        /// Segments each path of the last batched call took (glu_reduce_read_batch; synchronise its stream first).
        struct BatchReport
        {
            uint32_t wave_segments = 0, block_segments = 0, long_segments = 0;
        };
        [[nodiscard]] BatchReport last_batch() const
        {
            BatchReport r;
            GLU_CHECK_STATUS(glu_reduce_read_batch(m_impl, &r.wave_segments, &r.block_segments, &r.long_segments));
            return r;
        }

        [[nodiscard]] DataType data_type() const { return m_data_type; }
        [[nodiscard]] ReduceOperator reduce_operator() const { return m_operator; }

    private:
        const DataType m_data_type;
        const ReduceOperator m_operator;
        glu_reduce m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_REDUCE_HPP
