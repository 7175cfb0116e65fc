// glu_reduce_object.hpp -- what the translation units behind glu::BlellochScan and glu::Reduce share on the host side: the Reduce
// object (glu_scan_reduce.hip owns its life, glu_reduce_batch.hip its batched calls) and the dispatch over the twelve data types.
#pragma once

#include "glu_batch_host.hpp"

struct glu_reduce_s
{
    glu_data_type type;
    glu_reduce_operator op;
    glu_hip::host::Scratch partials;
    // the batched reduce: the list counts and the segment lists of a call with device offsets; the per-chunk partials of long segments
    glu_hip::host::Scratch batch_lists;
    glu_hip::host::Scratch batch_partials;
    glu_hip::host::LastBatch last_batch; // segments per class of the last batched call (glu_reduce_read_batch)
    void release()
    {
        for (glu_hip::host::Scratch* s : {&partials, &batch_lists, &batch_partials}) s->release();
    }
};

namespace glu_hip
{
namespace host
{
inline size_t data_type_size(glu_data_type t)
{
    switch (t)
    {
    case GLU_DATA_TYPE_FLOAT: case GLU_DATA_TYPE_INT: case GLU_DATA_TYPE_UINT: return 4;
    case GLU_DATA_TYPE_DOUBLE: case GLU_DATA_TYPE_VEC2: case GLU_DATA_TYPE_UVEC2: case GLU_DATA_TYPE_IVEC2: return 8;
    case GLU_DATA_TYPE_VEC4: case GLU_DATA_TYPE_UVEC4: case GLU_DATA_TYPE_IVEC4: case GLU_DATA_TYPE_DVEC2: return 16;
    case GLU_DATA_TYPE_DVEC4: return 32;
    default: return 0;
    }
}

// calls f.template operator()<S, N>() for the scalar type / component count of `t`
template<typename F>
glu_status dispatch_type(glu_data_type t, F&& f)
{
    switch (t)
    {
    case GLU_DATA_TYPE_FLOAT: return f.template operator()<float, 1>();
    case GLU_DATA_TYPE_DOUBLE: return f.template operator()<double, 1>();
    case GLU_DATA_TYPE_INT: return f.template operator()<int32_t, 1>();
    case GLU_DATA_TYPE_UINT: return f.template operator()<uint32_t, 1>();
    case GLU_DATA_TYPE_VEC2: return f.template operator()<float, 2>();
    case GLU_DATA_TYPE_VEC4: return f.template operator()<float, 4>();
    case GLU_DATA_TYPE_DVEC2: return f.template operator()<double, 2>();
    case GLU_DATA_TYPE_DVEC4: return f.template operator()<double, 4>();
    case GLU_DATA_TYPE_UVEC2: return f.template operator()<uint32_t, 2>();
    case GLU_DATA_TYPE_UVEC4: return f.template operator()<uint32_t, 4>();
    case GLU_DATA_TYPE_IVEC2: return f.template operator()<int32_t, 2>();
    case GLU_DATA_TYPE_IVEC4: return f.template operator()<int32_t, 4>();
    default: return fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid data type: %d", (int) t);
    }
}
} // namespace host
} // namespace glu_hip
