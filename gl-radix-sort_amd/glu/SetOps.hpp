// glu/SetOps.hpp -- glu::SetOps on MI355X (not in the reference): union, intersection, difference and symmetric difference of two
// sorted arrays of keys, with or without 4-byte values, in the order glu::RadixSort sorts, with std::set_* multiset semantics.
#ifndef GLU_SET_OPS_HPP
#define GLU_SET_OPS_HPP

#include "hip_utils.hpp"

namespace glu
{
    /// Both inputs are sorted in the sort's order of keys (floats by their bits: -0.0 and +0.0 are different keys, a NaN equals only
    /// the NaN with the same bits).  A key m times in A and n times in B is max(m, n) / min(m, n) / max(m - n, 0) / |m - n| times in
    /// the union / intersection / difference / symmetric difference.  The kept elements keep merge's order (A first among equal
    /// keys); the intersection holds A's keys and values.  out[0 .. min(S, max_out)) is written and the number S of kept elements
    /// goes to *device_num_out (a uint32_t on the device) also when S > max_out.  With device_out_keys == nullptr or max_out == 0
    /// the call only counts.  Everything stays on the device; the work is enqueued, not waited for (glu_set_ops_run_ptr in glu_hip.h).
    class SetOps
    {
    public:
        SetOps() { GLU_CHECK_STATUS(glu_set_ops_create(&m_impl)); }

        SetOps(const SetOps&) = delete;
        SetOps& operator=(const SetOps&) = delete;

        ~SetOps() { glu_set_ops_destroy(m_impl); }

        /// Scratch for calls of up to `total_count` = a_count + b_count keys: they then allocate nothing and can be captured.
        void prepare(size_t total_count, glu_key_type key_type = GLU_KEY_UINT32)
        {
            GLU_CHECK_STATUS(glu_set_ops_prepare(m_impl, total_count, key_type));
        }

        /// Any of the four operations.  device_a_vals and device_out_vals are both nullptr (keys only) or both set; device_b_vals is
        /// needed only by a union or a symmetric difference with values.  The inputs are only read.
        void operator()(glu_set_op op, const void* device_a_keys, const uint32_t* device_a_vals, size_t a_count, const void* device_b_keys,
                        const uint32_t* device_b_vals, size_t b_count, void* device_out_keys, uint32_t* device_out_vals, size_t max_out,
                        uint32_t* device_num_out, glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_set_ops_run_ptr(m_impl, (int) op, device_a_keys, device_a_vals, a_count, device_b_keys, device_b_vals, b_count,
                                                 device_out_keys, device_out_vals, max_out, device_num_out, key_type, stream));
        }

        /// Every element of A, and the elements of B beyond A's copies of their key.
        void set_union(const void* device_a_keys, const uint32_t* device_a_vals, size_t a_count, const void* device_b_keys,
                       const uint32_t* device_b_vals, size_t b_count, void* device_out_keys, uint32_t* device_out_vals, size_t max_out,
                       uint32_t* device_num_out, glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            (*this)(GLU_SET_UNION, device_a_keys, device_a_vals, a_count, device_b_keys, device_b_vals, b_count, device_out_keys,
                    device_out_vals, max_out, device_num_out, key_type, stream);
        }

        /// The elements of A that have a copy of their own in B (A's keys and values; B's values are not read).
        void set_intersection(const void* device_a_keys, const uint32_t* device_a_vals, size_t a_count, const void* device_b_keys,
                              size_t b_count, void* device_out_keys, uint32_t* device_out_vals, size_t max_out, uint32_t* device_num_out,
                              glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            (*this)(GLU_SET_INTERSECTION, device_a_keys, device_a_vals, a_count, device_b_keys, nullptr, b_count, device_out_keys,
                    device_out_vals, max_out, device_num_out, key_type, stream);
        }

        /// The elements of A beyond B's copies of their key (B's values are not read).
        void set_difference(const void* device_a_keys, const uint32_t* device_a_vals, size_t a_count, const void* device_b_keys,
                            size_t b_count, void* device_out_keys, uint32_t* device_out_vals, size_t max_out, uint32_t* device_num_out,
                            glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            (*this)(GLU_SET_DIFFERENCE, device_a_keys, device_a_vals, a_count, device_b_keys, nullptr, b_count, device_out_keys,
                    device_out_vals, max_out, device_num_out, key_type, stream);
        }

        /// The elements of either side beyond the other side's copies of their key.
        void set_symmetric_difference(const void* device_a_keys, const uint32_t* device_a_vals, size_t a_count, const void* device_b_keys,
                                      const uint32_t* device_b_vals, size_t b_count, void* device_out_keys, uint32_t* device_out_vals,
                                      size_t max_out, uint32_t* device_num_out, glu_key_type key_type = GLU_KEY_UINT32,
                                      void* stream = nullptr)
        {
            (*this)(GLU_SET_SYMMETRIC_DIFFERENCE, device_a_keys, device_a_vals, a_count, device_b_keys, device_b_vals, b_count,
                    device_out_keys, device_out_vals, max_out, device_num_out, key_type, stream);
        }

        /// Scratch for batched calls of up to `total_count` = a_total + b_total keys in up to `num_segments` segments: they then
        /// allocate nothing and can be captured.
        void prepare_batch(size_t total_count, size_t num_segments = 1, glu_key_type key_type = GLU_KEY_UINT32)
        {
            GLU_CHECK_STATUS(glu_set_ops_prepare_batch(m_impl, total_count, num_segments, key_type));
        }

        /// Any of the four operations on every segment's two sorted runs in one call: segment s of the result is `op` of
        /// A[a_offsets[s], a_offsets[s + 1]) and B[b_offsets[s], b_offsets[s + 1]), the segments' results back to back from out[0].
        /// The offsets are DEVICE arrays of num_segments + 1 words; a_total and b_total are the arrays' lengths.  Keys never match
        /// across segments.  *device_num_out receives the total kept, also beyond max_out; device_out_offsets (optional) the
        /// num_segments + 1 offsets of the compacted segments, held to max_out (in a call that only counts: the running
        /// cardinalities, not held to it).  One segment whose offset words were written on the device is the set operation whose
        /// counts live on the device (glu_set_ops_run_batch_offsets_ptr in glu_hip.h).
        void set_op_batch_offsets(glu_set_op op, const void* device_a_keys, const uint32_t* device_a_vals, const uint32_t* device_a_offsets,
                                  size_t a_total, const void* device_b_keys, const uint32_t* device_b_vals, const uint32_t* device_b_offsets,
                                  size_t b_total, size_t num_segments, void* device_out_keys, uint32_t* device_out_vals, size_t max_out,
                                  uint32_t* device_num_out, uint32_t* device_out_offsets = nullptr, glu_key_type key_type = GLU_KEY_UINT32,
                                  void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_set_ops_run_batch_offsets_ptr(m_impl, (int) op, device_a_keys, device_a_vals, device_a_offsets, a_total,
                                                               device_b_keys, device_b_vals, device_b_offsets, b_total, num_segments,
                                                               device_out_keys, device_out_vals, max_out, device_out_offsets, device_num_out,
                                                               key_type, stream));
        }

        /// The same over equal partitions: segment s is A[s * a_len, (s + 1) * a_len) and B[s * b_len, (s + 1) * b_len); either
        /// length may be 0.
        void set_op_batch(glu_set_op op, const void* device_a_keys, const uint32_t* device_a_vals, size_t a_len, const void* device_b_keys,
                          const uint32_t* device_b_vals, size_t b_len, size_t num_segments, void* device_out_keys, uint32_t* device_out_vals,
                          size_t max_out, uint32_t* device_num_out, uint32_t* device_out_offsets = nullptr,
                          glu_key_type key_type = GLU_KEY_UINT32, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_set_ops_run_batch_ptr(m_impl, (int) op, device_a_keys, device_a_vals, a_len, device_b_keys, device_b_vals, b_len,
                                                       num_segments, device_out_keys, device_out_vals, max_out, device_out_offsets,
                                                       device_num_out, key_type, stream));
        }

        /// What a call with these counts does (glu_set_ops_plan; host only, no device needed).  with_arrays: the call writes its
        /// result (false: it only counts).
        struct Plan
        {
            uint32_t tile = 0, tiles = 0, kernels = 0;
            size_t scratch_bytes = 0;
        };
        [[nodiscard]] static Plan plan(size_t a_count, size_t b_count, glu_key_type key_type = GLU_KEY_UINT32, bool with_arrays = true)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_set_ops_plan(a_count, b_count, key_type, with_arrays ? 1 : 0, &p.tile, &p.tiles, &p.kernels, &p.scratch_bytes));
            return p;
        }

        /// What a batched call does (glu_set_ops_plan_batch; host only, no device needed).  with_arrays: the call writes its result;
        /// with_offsets: it writes out_offsets.
        [[nodiscard]] static Plan plan_batch(size_t a_total, size_t b_total, size_t num_segments, glu_key_type key_type = GLU_KEY_UINT32,
                                             bool with_arrays = true, bool with_offsets = true)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_set_ops_plan_batch(a_total, b_total, num_segments, key_type, with_arrays ? 1 : 0, with_offsets ? 1 : 0, &p.tile,
                                                    &p.tiles, &p.kernels, &p.scratch_bytes));
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
            GLU_CHECK_STATUS(glu_set_ops_last(m_impl, &l.tiles, &l.kernels));
            return l;
        }

    private:
        glu_set_ops m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_SET_OPS_HPP
