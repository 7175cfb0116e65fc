// glu/Select.hpp -- glu::Select on MI355X (not in the reference): stable stream compaction by a stencil and a comparison -- the
// indices of the elements whose stencil passes, and the items at them, side by side and in their order.
#ifndef GLU_SELECT_HPP
#define GLU_SELECT_HPP

#include "data_types.hpp"
#include "hip_utils.hpp"

namespace glu
{
    /// The element type of a stencil: the four scalar DataType's with their values, or a byte (a bool mask, byte flags).
    enum SelectStencil
    {
        SelectStencil_Float = GLU_DATA_TYPE_FLOAT,
        SelectStencil_Double = GLU_DATA_TYPE_DOUBLE,
        SelectStencil_Int = GLU_DATA_TYPE_INT,
        SelectStencil_Uint = GLU_DATA_TYPE_UINT,
        SelectStencil_Byte = GLU_SELECT_STENCIL_BYTE
    };

    enum SelectOperator
    {
        SelectOperator_Equal = GLU_SELECT_EQ,
        SelectOperator_NotEqual = GLU_SELECT_NE,
        SelectOperator_Less = GLU_SELECT_LT,
        SelectOperator_LessEqual = GLU_SELECT_LE,
        SelectOperator_Greater = GLU_SELECT_GT,
        SelectOperator_GreaterEqual = GLU_SELECT_GE
    };

    /// What out_indices of a batched call holds: the index in the array, or in the element's segment.
    enum SelectIndex
    {
        SelectIndex_Global = GLU_SELECT_INDEX_GLOBAL,
        SelectIndex_Local = GLU_SELECT_INDEX_LOCAL
    };

    /// The arrays of one Select call (glu_select_run_ptr in glu_hip.h).  All pointers are device pointers but `threshold`.
    struct SelectArrays
    {
        const void* stencil = nullptr;
        SelectStencil stencil_type = SelectStencil_Uint;
        SelectOperator op = SelectOperator_NotEqual;
        const void* threshold = nullptr; ///< HOST pointer to one value of the stencil's type; nullptr: zero
        size_t count = 0;
        const void* items = nullptr;     ///< count items of item_bytes bytes, or nullptr; may be the stencil itself
        uint32_t item_bytes = 4;         ///< 4, 8, 16 or 32 (Select::item_bytes(DataType))
        void* out_items = nullptr;       ///< max_out items, given iff items is
        uint32_t* out_indices = nullptr; ///< max_out words, or nullptr
        size_t max_out = 0;
        uint32_t* num_selected = nullptr;
    };

    /// Element i is selected iff stencil[i] OP threshold (IEEE comparison of floats and doubles: a NaN passes only NotEqual,
    /// -0.0 equals +0.0; Int signed, Uint and Byte unsigned).  Everything stays on the device; the work is enqueued, not waited for.
    class Select
    {
    public:
        Select() { GLU_CHECK_STATUS(glu_select_create(&m_impl)); }

        Select(const Select&) = delete;
        Select& operator=(const Select&) = delete;

        ~Select() { glu_select_destroy(m_impl); }

        /// Scratch for up to `count` elements of such a stencil: calls then allocate nothing and can be captured into a graph.
        void prepare(size_t count, SelectStencil stencil_type = SelectStencil_Uint)
        {
            GLU_CHECK_STATUS(glu_select_prepare(m_impl, count, stencil_type));
        }

        /// S = the number of selected elements, i_0 < i_1 < ... their indices.  out_indices[r] = i_r and out_items[r] =
        /// items[i_r] for r < min(S, max_out); entries behind that are not touched.  *num_selected = S, also where S > max_out.
        /// The stencil and the items are only read.
        void operator()(const SelectArrays& a, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_select_run_ptr(m_impl, a.stencil, a.stencil_type, a.op, a.threshold, a.count, a.items, a.item_bytes,
                                                a.out_items, a.out_indices, a.max_out, a.num_selected, stream));
        }

        void operator()(const void* device_stencil, SelectStencil stencil_type, SelectOperator op, const void* host_threshold,
                        size_t count, const void* device_items, uint32_t item_bytes, void* device_out_items,
                        uint32_t* device_out_indices, size_t max_out, uint32_t* device_num_selected, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_select_run_ptr(m_impl, device_stencil, stencil_type, op, host_threshold, count, device_items, item_bytes,
                                                device_out_items, device_out_indices, max_out, device_num_selected, stream));
        }

        /// Scratch for batches of up to `total` elements (about total / 8 bytes): the batched calls then allocate nothing.
        void prepare_batch(size_t total, size_t num_segments, SelectStencil stencil_type = SelectStencil_Uint)
        {
            GLU_CHECK_STATUS(glu_select_prepare_batch(m_impl, total, num_segments, stencil_type));
        }

        /// The select of `a` over a.count = count * num_partitions elements in segments of `count`: the same compaction, and
        /// out_offsets[s] = min(a.max_out, the selected elements in front of segment s) for s = 0 .. num_partitions (nullptr skips
        /// it) -- the offsets of the compacted segments, in the form every batched operator takes.  SelectIndex_Local writes the
        /// index inside the element's segment.  a.count is not looked at.
        void select_batch(const SelectArrays& a, size_t count, size_t num_partitions, uint32_t* out_offsets,
                          SelectIndex index_form = SelectIndex_Global, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_select_run_batch_ptr(m_impl, a.stencil, a.stencil_type, a.op, a.threshold, count, num_partitions, a.items,
                                                      a.item_bytes, a.out_items, a.out_indices, index_form, a.max_out, out_offsets,
                                                      a.num_selected, stream));
        }

        /// The same over the segments [offsets[s], offsets[s + 1]) of device offsets (num_segments + 1 words, what KeyRuns writes),
        /// a.count being the length of the arrays: only elements from offsets[0] to offsets[num_segments] can be selected.
        void select_batch_offsets(const SelectArrays& a, const uint32_t* offsets, size_t num_segments, uint32_t* out_offsets,
                                  SelectIndex index_form = SelectIndex_Global, void* stream = nullptr)
        {
            GLU_CHECK_STATUS(glu_select_run_batch_offsets_ptr(m_impl, a.stencil, a.stencil_type, a.op, a.threshold, a.count, offsets,
                                                              num_segments, a.items, a.item_bytes, a.out_items, a.out_indices, index_form,
                                                              a.max_out, out_offsets, a.num_selected, stream));
        }

        /// What a batched call does (glu_select_plan_batch; host only, no device needed).
        struct BatchPlan
        {
            uint32_t tile = 0, tiles = 0, scan_rounds = 0, kernels = 0;
            size_t scratch_bytes = 0;
        };
        [[nodiscard]] static BatchPlan plan_batch(size_t total, size_t num_segments, SelectStencil stencil_type = SelectStencil_Uint,
                                                  SelectIndex index_form = SelectIndex_Global)
        {
            BatchPlan p;
            GLU_CHECK_STATUS(glu_select_plan_batch(total, num_segments, stencil_type, index_form, &p.tile, &p.tiles, &p.scan_rounds, &p.kernels,
                                                   &p.scratch_bytes));
            return p;
        }

        /// Bytes of an item of `data_type` (4, 8, 16 or 32): what item_bytes takes for arrays of Vec4, DVec4 and the like.
        [[nodiscard]] static uint32_t item_bytes(DataType data_type) { return (uint32_t) data_type_size(data_type); }

        /// What a call does with `count` elements (glu_select_plan; host only, no device needed).
        struct Plan
        {
            uint32_t tile = 0, tiles = 0, scan_rounds = 0;
        };
        [[nodiscard]] static Plan plan(size_t count, SelectStencil stencil_type = SelectStencil_Uint)
        {
            Plan p;
            GLU_CHECK_STATUS(glu_select_plan(count, stencil_type, &p.tile, &p.tiles, &p.scan_rounds));
            return p;
        }

    private:
        glu_select m_impl = nullptr;
    };
} // namespace glu

#endif // GLU_SELECT_HPP
