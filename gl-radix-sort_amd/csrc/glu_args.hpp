// glu_args.hpp -- the argument rules of the entry points, each stated once: key types, the limits of a call, arrays that must not
// overlap, alignment, items, handles and out-parameters.  Plain C++ (no HIP header: tests/test_args_layer.py compiles it with a host
// compiler and its own fail()); glu_host.hpp includes it, so every translation unit has it.
// What a unit checks, and in which order, stays the unit's: the helpers only say how one check reads and what it answers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#define GLU_HIP_BUILD 1
#include "glu_hip.h"

namespace glu_hip
{
namespace host
{
glu_status fail(glu_status code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define GLU_TRY(expr)                                                                                                  \
    do                                                                                                                 \
    {                                                                                                                  \
        glu_status s_ = (expr);                                                                                        \
        if (s_ != GLU_OK) return s_;                                                                                   \
    } while (0)

// ---- key types: glu_key_type as an int (a caller may pass anything)
inline glu_status check_key_type(int key_type)
{
    return key_type >= (int) GLU_KEY_UINT32 && key_type <= (int) GLU_KEY_FLOAT64 ? GLU_OK
                                                                                 : fail(GLU_ERROR_INVALID_ARGUMENT, "Invalid key type: %d", key_type);
}
inline uint32_t key_bytes_of(int key_type) { return key_type >= (int) GLU_KEY_UINT64 ? 8u : 4u; }
// how the kernels turn a key into its unsigned sort order: the values of KEY_XF_NONE, _SIGNED and _FLOAT of radix_sort_kernels.hpp
// (every unit that hands one to a kernel holds them equal by static_assert)
constexpr uint32_t kKeyXfNone = 0, kKeyXfSigned = 1, kKeyXfFloat = 2;
inline uint32_t key_xf_of(int key_type)
{
    switch (key_type)
    {
    case GLU_KEY_INT32:
    case GLU_KEY_INT64: return kKeyXfSigned;
    case GLU_KEY_FLOAT32:
    case GLU_KEY_FLOAT64: return kKeyXfFloat;
    default: return kKeyXfNone;
    }
}

// ---- limits.  `what`: the operator's own sentence, e.g. "select takes a count below 2^32"
inline glu_status check_tile_count(size_t count, const char* what)
{
    return count < ((size_t) 1 << 32) ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "%s (got %zu)", what, count);
}
// max_out, max_runs: the room of an output array, a word on the device
inline glu_status check_below_2_32(size_t value, const char* name)
{
    return value < ((size_t) 1 << 32) ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "%s must be below 2^32 (got %zu)", name, value);
}

// ---- arrays.  Adjacent arrays do not overlap, and an array of no bytes overlaps nothing.
inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

struct Array
{
    const void* ptr; // NULL: not given, overlaps nothing
    size_t bytes;
    const char* name;
};
inline bool overlaps(const Array& a, const Array& b) { return a.ptr && b.ptr && overlaps(a.ptr, a.bytes, b.ptr, b.bytes); }

// Which pairs check_disjoint holds apart besides every output against every input, and when:
enum OutputPairs
{
    kOutputsMayOverlap,   // none (key runs, select, histogram, the batched reduce)
    kOutputsAfterInputs,  // after all of those, an output against the outputs before it: "<later> overlaps <earlier>" (merge, sorted search)
    kOutputsBeforeInputs, // an output against the outputs behind it, then against the inputs: "<earlier> overlaps <later>" (expand)
};

// The first pair that overlaps, outputs in their order and for each the inputs in theirs: "<output> overlaps <other>".
inline glu_status check_disjoint(std::initializer_list<Array> outputs, std::initializer_list<Array> inputs, OutputPairs pairs = kOutputsMayOverlap)
{
    const auto refuse = [](const Array& o, const Array& other) { return fail(GLU_ERROR_INVALID_ARGUMENT, "%s overlaps %s", o.name, other.name); };
    for (const Array* o = outputs.begin(); o != outputs.end(); o++)
    {
        if (pairs == kOutputsBeforeInputs)
            for (const Array* behind = o + 1; behind != outputs.end(); behind++)
                if (overlaps(*o, *behind)) return refuse(*o, *behind);
        for (const Array& i : inputs)
            if (overlaps(*o, i)) return refuse(*o, i);
    }
    if (pairs == kOutputsAfterInputs)
        for (const Array* o = outputs.begin(); o != outputs.end(); o++)
            for (const Array* before = outputs.begin(); before != o; before++)
                if (overlaps(*o, *before)) return refuse(*o, *before);
    return GLU_OK;
}

// ---- alignment: "<name> is not aligned to <to>"; `to` names the rule in the caller's words ("the key size", "4 bytes", ...).
// NULL is aligned to everything.
inline glu_status check_aligned(const void* ptr, size_t align, const char* name, const char* to)
{
    return (uintptr_t) ptr % align ? fail(GLU_ERROR_INVALID_ARGUMENT, "%s is not aligned to %s", name, to) : GLU_OK;
}
inline glu_status check_aligned_4(const void* ptr, const char* name) { return check_aligned(ptr, 4, name, "4 bytes"); }

// ---- items: what select and expand gather, 4 to 32 bytes each, moved in pieces of up to 16
inline glu_status check_item_bytes(uint32_t item_bytes)
{
    return item_bytes == 4 || item_bytes == 8 || item_bytes == 16 || item_bytes == 32
               ? GLU_OK
               : fail(GLU_ERROR_INVALID_ARGUMENT, "item_bytes must be 4, 8, 16 or 32 (got %u)", item_bytes);
}
inline uint32_t item_align(uint32_t item_bytes) { return item_bytes < 16 ? item_bytes : 16u; }
inline const char* bytes_text(uint32_t align) { return align == 4 ? "4 bytes" : align == 8 ? "8 bytes" : "16 bytes"; }
// items, then out_items, of a call that gathers (items != NULL; item_bytes has been checked)
inline glu_status check_items_aligned(const void* items, const void* out_items, uint32_t item_bytes, const char* to)
{
    if (!items) return GLU_OK;
    GLU_TRY(check_aligned(items, item_align(item_bytes), "items", to));
    return check_aligned(out_items, item_align(item_bytes), "out_items", to);
}

// ---- handles, other pointers a call needs, and out-parameters
inline glu_status check_not_null(const void* ptr, const char* name)
{
    return ptr ? GLU_OK : fail(GLU_ERROR_INVALID_ARGUMENT, "%s is NULL", name);
}
// several pointers under one sentence of the unit's own ("NULL argument", "NULL array", "Invalid key buffer"): the whole message
inline glu_status check_none_null(std::initializer_list<const void*> ptrs, const char* message)
{
    for (const void* ptr : ptrs)
        if (!ptr) return fail(GLU_ERROR_INVALID_ARGUMENT, "%s", message);
    return GLU_OK;
}
template<typename T, typename V>
inline void store(T* out, V value)
{
    if (out) *out = (T) value;
}

// ---- GLU_HIP_SCRATCH_FILL, the test switch of Scratch::reserve (glu_host.hpp): `text` is the variable as it stands.  Unset or
// empty: *byte = -1, nothing is filled.  A decimal or 0x integer 0 .. 255: that byte.  Anything else refuses the call that grows.
inline glu_status check_scratch_fill(const char* text, int* byte)
{
    *byte = -1;
    if (!text || !*text) return GLU_OK;
    long value = 0;
    int digits = 0;
    const bool hex = text[0] == '0' && (text[1] == 'x' || text[1] == 'X');
    for (const char* c = text + (hex ? 2 : 0); *c && value <= 255; c++, digits++)
    {
        const int d = *c >= '0' && *c <= '9' ? *c - '0' : hex && *c >= 'a' && *c <= 'f' ? *c - 'a' + 10 : hex && *c >= 'A' && *c <= 'F' ? *c - 'A' + 10 : -1;
        if (d < 0) return fail(GLU_ERROR_INVALID_ARGUMENT, "GLU_HIP_SCRATCH_FILL must be an integer 0 .. 255 (got \"%s\")", text);
        value = value * (hex ? 16 : 10) + d;
    }
    if (digits == 0 || value > 255) return fail(GLU_ERROR_INVALID_ARGUMENT, "GLU_HIP_SCRATCH_FILL must be an integer 0 .. 255 (got \"%s\")", text);
    *byte = (int) value;
    return GLU_OK;
}
} // namespace host
} // namespace glu_hip
