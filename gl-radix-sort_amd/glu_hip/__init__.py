"""ctypes binding of libglu_hip.so (include/glu_hip.h) -- used by the tests, bench.py and the
multi-GPU driver.  The C++17 headers in ../glu/ are the drop-in surface for the reference's users; this
module is the thinnest possible Python view of the same C ABI.

There is no CPU fallback: importing works anywhere (so that symbol/ABI tests run without a GPU), but every
compute call returns GLU_ERROR_NO_DEVICE without an MI355X and raises GluError.
"""
import ctypes
import os

import numpy as np

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("GLU_HIP_LIB_PATH") or os.path.join(_PKG_DIR, "lib", "libglu_hip.so")  # override: tuning builds

# glu/data_types.hpp:8-22 and glu/Reduce.hpp:42-48 (same numeric values)
DataType_Float, DataType_Double, DataType_Int, DataType_Uint, DataType_Vec2, DataType_Vec4, DataType_DVec2, \
    DataType_DVec4, DataType_UVec2, DataType_UVec4, DataType_IVec2, DataType_IVec4 = range(12)
ReduceOperator_Sum, ReduceOperator_Mul, ReduceOperator_Min, ReduceOperator_Max = range(4)
# glu_select_run_ptr: the stencil types (the four scalar data types with their values, and a byte) and the comparisons
SelectStencil_Float, SelectStencil_Double, SelectStencil_Int, SelectStencil_Uint, SelectStencil_Byte = 0, 1, 2, 3, 12
SelectOperator_EQ, SelectOperator_NE, SelectOperator_LT, SelectOperator_LE, SelectOperator_GT, SelectOperator_GE = range(6)
# glu_select_run_batch_ptr: what out_indices holds (the index in the array, or in the element's segment)
SelectIndex_Global, SelectIndex_Local = 0, 1
# glu_sorted_search_set_option("PATH", ...) and what glu_sorted_search_plan / glu_sorted_search_last report
SearchPath_Auto, SearchPath_Direct, SearchPath_Indexed = range(3)
SearchPath_Batch = 3  # what glu_sorted_search_last reports after a batched call (never an option)
SEARCH_BATCH_WINDOW_DEFAULT = 0xFFFFFFFF  # set_batch_window / plan_sorted_search_batch: the maximum of the call's key width
# glu_top_k_set_option("PATH", ...) and what glu_top_k_read_last reports
TopKPath_Auto, TopKPath_Candidates, TopKPath_Full = range(3)
KEY_TYPES = {"uint32": 0, "int32": 1, "float32": 2, "uint64": 3, "int64": 4, "float64": 5}  # glu_key_type by numpy dtype name

GLU_OK = 0
GLU_ERROR_INVALID_ARGUMENT = 1
GLU_ERROR_INVALID_STATE = 2
GLU_ERROR_OUT_OF_MEMORY = 3
GLU_ERROR_DEVICE = 4
GLU_ERROR_NO_DEVICE = 5

# every symbol include/glu_hip.h declares: (name, restype, argtypes)
_u32, _u64, _sz, _int, _vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
_P = ctypes.POINTER
SYMBOLS = [
    ("glu_last_error", ctypes.c_char_p, []),
    ("glu_version", ctypes.c_char_p, []),
    ("glu_scratch_filled_bytes", _int, [_P(_sz)]),
    ("glu_device_count", _int, [_P(_int)]),
    ("glu_set_device", _int, [_int]),
    ("glu_device_info", _int, [ctypes.c_char_p, _sz]),
    ("glu_device_synchronize", _int, []),
    ("glu_queue", _int, [_P(_vp)]),
    ("glu_buffer_create", _int, [_sz, _P(_u32)]),
    ("glu_buffer_create_with_data", _int, [_vp, _sz, _P(_u32)]),
    ("glu_buffer_wrap", _int, [_vp, _sz, _P(_u32)]),
    ("glu_buffer_destroy", _int, [_u32]),
    ("glu_buffer_size", _int, [_u32, _P(_sz)]),
    ("glu_buffer_device_ptr", _int, [_u32, _P(_vp)]),
    ("glu_buffer_write", _int, [_u32, _vp, _sz, _sz]),
    ("glu_buffer_read", _int, [_u32, _vp, _sz, _sz]),
    ("glu_buffer_fill_u32", _int, [_u32, _u32]),
    ("glu_buffer_copy", _int, [_u32, _u32, _sz, _sz, _sz]),
    ("glu_radix_sort_create", _int, [_P(_vp)]),
    ("glu_radix_sort_destroy", _int, [_vp]),
    ("glu_radix_sort_prepare", _int, [_vp, _sz]),
    ("glu_radix_sort_prepare_u64", _int, [_vp, _sz]),
    ("glu_radix_sort_prepare_ex", _int, [_vp, _sz, _sz, _int]),
    ("glu_radix_sort_run", _int, [_vp, _u32, _u32, _sz, _sz]),
    ("glu_radix_sort_run_ptr", _int, [_vp, _vp, _vp, _sz, _sz, _vp]),
    ("glu_radix_sort_run_u64", _int, [_vp, _u32, _u32, _sz, _sz]),
    ("glu_radix_sort_run_u64_ptr", _int, [_vp, _vp, _vp, _sz, _sz, _vp]),
    ("glu_radix_sort_run_keys", _int, [_vp, _u32, _sz, _sz]),
    ("glu_radix_sort_run_keys_ptr", _int, [_vp, _vp, _sz, _sz, _vp]),
    ("glu_radix_sort_run_keys_u64_ptr", _int, [_vp, _vp, _sz, _sz, _vp]),
    ("glu_radix_sort_run_typed_ptr", _int, [_vp, _vp, _vp, _sz, _int, _vp]),
    ("glu_radix_sort_run_bit_range_ptr", _int, [_vp, _vp, _vp, _sz, _u32, _u32, _u32, _vp]),
    ("glu_radix_sort_partition_ptr", _int, [_vp, _vp, _vp, _vp, _vp, _sz, _u32, _u32, _vp, _vp]),
    ("glu_radix_sort_run_segments_ptr", _int, [_vp, _vp, _vp, _vp, _vp, _sz, _P(_u64), _P(_u64), _P(_u32), _sz, _u32, _u32, _vp]),
    ("glu_radix_sort_plan_segments", _int, [_P(_u64), _P(_u64), _P(_u32), _sz, _u32, _u32, _P(_u32), _sz, _P(_u32), _P(_u32), _P(_u64), _P(_sz)]),
    ("glu_radix_sort_set_digit_bits", _int, [_vp, _u32]),
    ("glu_radix_sort_set_option", _int, [_vp, ctypes.c_char_p, ctypes.c_longlong]),
    ("glu_radix_sort_get_digit_bits", _int, [_vp, _P(_u32)]),
    ("glu_radix_sort_scratch_size", _int, [_vp, _P(_sz)]),
    ("glu_radix_sort_scratch_placement", _int, [_vp, _P(_u32), _P(ctypes.c_double), _P(ctypes.c_double)]),
    ("glu_radix_sort_set_profiling", _int, [_vp, _int]),
    ("glu_radix_sort_read_profile", _int, [_vp, _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(_u64)]),
    ("glu_radix_sort_read_plan", _int, [_vp, _P(_u32), _P(_u32), _P(_u32), _sz]),
    ("glu_radix_sort_read_profile_finish", _int, [_vp, _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(_u64),
                                                  _P(ctypes.c_double), _P(_u64)]),
    ("glu_radix_sort_plan_finish", _int, [_sz, _u32, _P(_u32), _P(_u32)]),
    ("glu_radix_sort_read_finish", _int, [_vp, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_radix_sort_read_handoff", _int, [_vp, _P(_u32)]),
    ("glu_radix_sort_read_long_runs", _int, [_vp, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_radix_sort_read_seg_finish", _int, [_vp, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_radix_sort_run_batch_ptr", _int, [_vp, _vp, _vp, _sz, _sz, _int, _vp]),
    ("glu_radix_sort_run_batch_offsets_ptr", _int, [_vp, _vp, _vp, _sz, _vp, _sz, _int, _vp]),
    ("glu_radix_sort_prepare_batch", _int, [_vp, _sz, _sz, _sz, _int]),
    ("glu_radix_sort_plan_batch", _int, [_sz, _u32, _int, _P(_u32), _P(_u32)]),
    ("glu_radix_sort_read_batch", _int, [_vp, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_scan_create", _int, [_int, _P(_vp)]),
    ("glu_scan_destroy", _int, [_vp]),
    ("glu_scan_prepare", _int, [_vp, _sz, _sz]),
    ("glu_scan_run", _int, [_vp, _u32, _sz, _sz]),
    ("glu_scan_run_ptr", _int, [_vp, _vp, _sz, _sz, _vp]),
    ("glu_scan_run_batch_offsets_ptr", _int, [_vp, _vp, _sz, _vp, _sz, _vp]),
    ("glu_scan_run_batch_offsets_op_ptr", _int, [_vp, _vp, _vp, _sz, _vp, _sz, _int, _int, _vp]),
    ("glu_scan_prepare_batch", _int, [_vp, _sz, _sz]),
    ("glu_scan_plan_batch", _int, [_sz, _u32, _P(_u32), _P(_u32)]),
    ("glu_scan_read_batch", _int, [_vp, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_reduce_create", _int, [_int, _int, _P(_vp)]),
    ("glu_reduce_destroy", _int, [_vp]),
    ("glu_reduce_run", _int, [_vp, _u32, _sz]),
    ("glu_reduce_run_ptr", _int, [_vp, _vp, _sz, _vp]),
    ("glu_reduce_run_batch_ptr", _int, [_vp, _vp, _vp, _sz, _sz, _vp]),
    ("glu_reduce_run_batch_offsets_ptr", _int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    ("glu_reduce_prepare_batch", _int, [_vp, _sz, _sz]),
    ("glu_reduce_plan_batch", _int, [_sz, _u32, _P(_u32), _P(_u32)]),
    ("glu_reduce_read_batch", _int, [_vp, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_key_runs_create", _int, [_P(_vp)]),
    ("glu_key_runs_destroy", _int, [_vp]),
    ("glu_key_runs_prepare", _int, [_vp, _sz, _u32]),
    ("glu_key_runs_run_ptr", _int, [_vp, _vp, _sz, _u32, _u32, _u32, _vp, _vp, _sz, _vp, _vp]),
    ("glu_key_runs_plan", _int, [_sz, _u32, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_select_create", _int, [_P(_vp)]),
    ("glu_select_destroy", _int, [_vp]),
    ("glu_select_prepare", _int, [_vp, _sz, _int]),
    ("glu_select_run_ptr", _int, [_vp, _vp, _int, _int, _vp, _sz, _vp, _u32, _vp, _vp, _sz, _vp, _vp]),
    ("glu_select_plan", _int, [_sz, _int, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_select_prepare_batch", _int, [_vp, _sz, _sz, _int]),
    ("glu_select_run_batch_ptr", _int, [_vp, _vp, _int, _int, _vp, _sz, _sz, _vp, _u32, _vp, _vp, _int, _sz, _vp, _vp, _vp]),
    ("glu_select_run_batch_offsets_ptr", _int, [_vp, _vp, _int, _int, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp, _int, _sz, _vp, _vp, _vp]),
    ("glu_select_plan_batch", _int, [_sz, _sz, _int, _int, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_sorted_search_create", _int, [_P(_vp)]),
    ("glu_sorted_search_destroy", _int, [_vp]),
    ("glu_sorted_search_prepare", _int, [_vp, _sz, _int]),
    ("glu_sorted_search_set_option", _int, [_vp, ctypes.c_char_p, ctypes.c_longlong]),
    ("glu_sorted_search_index_ptr", _int, [_vp, _vp, _sz, _int, _vp]),
    ("glu_sorted_search_run_ptr", _int, [_vp, _vp, _sz, _vp, _sz, _int, _vp, _vp, _int, _vp]),
    ("glu_sorted_search_plan", _int, [_sz, _sz, _int, _u32, _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_sorted_search_last", _int, [_vp, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_sorted_search_run_batch_ptr", _int, [_vp, _vp, _sz, _vp, _sz, _sz, _int, _vp, _vp, _vp]),
    ("glu_sorted_search_run_batch_offsets_ptr", _int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _vp, _vp, _vp]),
    ("glu_sorted_search_set_batch_window", _int, [_vp, _u32]),
    ("glu_sorted_search_plan_batch", _int, [_sz, _int, _u32, _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_merge_create", _int, [_P(_vp)]),
    ("glu_merge_destroy", _int, [_vp]),
    ("glu_merge_prepare", _int, [_vp, _sz, _int]),
    ("glu_merge_run_ptr", _int, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _int, _vp]),
    ("glu_merge_plan", _int, [_sz, _sz, _int, _int, _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_merge_last", _int, [_vp, _P(_u32), _P(_u32)]),
    ("glu_merge_prepare_batch", _int, [_vp, _sz, _int]),
    ("glu_merge_run_batch_offsets_ptr", _int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _int, _vp]),
    ("glu_merge_run_batch_ptr", _int, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _int, _vp]),
    ("glu_merge_plan_batch", _int, [_sz, _sz, _int, _int, _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_set_ops_create", _int, [_P(_vp)]),
    ("glu_set_ops_destroy", _int, [_vp]),
    ("glu_set_ops_prepare", _int, [_vp, _sz, _int]),
    ("glu_set_ops_run_ptr", _int, [_vp, _int, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _int, _vp]),
    ("glu_set_ops_plan", _int, [_sz, _sz, _int, _int, _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_set_ops_last", _int, [_vp, _P(_u32), _P(_u32)]),
    ("glu_set_ops_prepare_batch", _int, [_vp, _sz, _sz, _int]),
    ("glu_set_ops_run_batch_offsets_ptr", _int, [_vp, _int, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _int, _vp]),
    ("glu_set_ops_run_batch_ptr", _int, [_vp, _int, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _int, _vp]),
    ("glu_set_ops_plan_batch", _int, [_sz, _sz, _sz, _int, _int, _int, _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_histogram_create", _int, [_P(_vp)]),
    ("glu_histogram_destroy", _int, [_vp]),
    ("glu_histogram_prepare", _int, [_vp, _sz, _sz]),
    ("glu_histogram_run_even_ptr", _int, [_vp, _vp, _sz, _int, _vp, _vp, _sz, _vp, _int, _vp]),
    ("glu_histogram_run_edges_ptr", _int, [_vp, _vp, _sz, _int, _vp, _sz, _vp, _int, _vp]),
    ("glu_histogram_plan", _int, [_sz, _sz, _int, _int, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_histogram_last", _int, [_vp, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_histogram_run_batch_even_ptr", _int, [_vp, _vp, _sz, _sz, _int, _vp, _vp, _sz, _vp, _int, _vp]),
    ("glu_histogram_run_batch_offsets_even_ptr", _int, [_vp, _vp, _sz, _vp, _sz, _int, _vp, _vp, _sz, _vp, _int, _vp]),
    ("glu_histogram_run_batch_edges_ptr", _int, [_vp, _vp, _sz, _sz, _int, _vp, _sz, _vp, _int, _vp]),
    ("glu_histogram_run_batch_offsets_edges_ptr", _int, [_vp, _vp, _sz, _vp, _sz, _int, _vp, _sz, _vp, _int, _vp]),
    ("glu_histogram_prepare_batch", _int, [_vp, _sz, _sz, _sz]),
    ("glu_histogram_plan_batch", _int, [_sz, _sz, _int, _int, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_histogram_read_batch", _int, [_vp, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_expand_create", _int, [_P(_vp)]),
    ("glu_expand_destroy", _int, [_vp]),
    ("glu_expand_prepare", _int, [_vp, _sz, _sz]),
    ("glu_expand_run_ptr", _int, [_vp, _vp, _sz, _sz, _vp, _u32, _vp, _vp, _vp, _vp]),
    ("glu_expand_plan", _int, [_sz, _sz, _P(_u32), _P(_u32), _P(_u32), _P(_sz)]),
    ("glu_expand_last", _int, [_vp, _P(_u32), _P(_u32)]),
    ("glu_gather_create", _int, [_P(_vp)]),
    ("glu_gather_destroy", _int, [_vp]),
    ("glu_gather_run_ptr", _int, [_vp, _vp, _sz, _u32, _vp, _sz, _vp, _vp]),
    ("glu_gather_run_batch_ptr", _int, [_vp, _vp, _u32, _sz, _sz, _vp, _sz, _vp, _vp]),
    ("glu_gather_run_batch_offsets_ptr", _int, [_vp, _vp, _u32, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    ("glu_gather_scatter_ptr", _int, [_vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp]),
    ("glu_gather_plan", _int, [_sz, _u32, _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_gather_last", _int, [_vp, _P(_u32), _P(_u32)]),
    ("glu_top_k_create", _int, [_P(_vp)]),
    ("glu_top_k_destroy", _int, [_vp]),
    ("glu_top_k_prepare", _int, [_vp, _sz, _sz, _int]),
    ("glu_top_k_set_option", _int, [_vp, ctypes.c_char_p, ctypes.c_longlong]),
    ("glu_top_k_run_ptr", _int, [_vp, _vp, _int, _sz, _sz, _int, _int, _vp, _vp, _vp, _vp]),
    ("glu_top_k_read_last", _int, [_vp, _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_top_k_plan", _int, [_sz, _sz, _int, _int, _int, _int, _sz, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32),
                              _P(_sz)]),
    ("glu_top_k_run_batch_ptr", _int, [_vp, _vp, _int, _sz, _sz, _sz, _int, _int, _vp, _vp, _vp, _vp]),
    ("glu_top_k_run_batch_offsets_ptr", _int, [_vp, _vp, _int, _sz, _vp, _sz, _sz, _int, _int, _vp, _vp, _vp, _vp]),
    ("glu_top_k_prepare_batch", _int, [_vp, _sz, _sz, _sz, _int]),
    ("glu_top_k_plan_batch", _int, [_sz, _sz, _sz, _int, _int, _int, _int, _sz, _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_u32), _P(_sz),
                                    _P(_u32), _P(_sz)]),
    ("glu_top_k_read_batch", _int, [_vp, _P(_u32), _P(_u32), _P(_u32), _P(_u32)]),
    ("glu_dist_available", _int, []),
    ("glu_dist_unique_id", _int, [_vp, _sz]),
    ("glu_dist_create", _int, [_vp, _sz, _int, _int, _P(_vp)]),
    ("glu_dist_destroy", _int, [_vp]),
    ("glu_dist_world", _int, [_vp, _P(_int), _P(_int)]),
    ("glu_dist_partition_shift", _int, [_vp, _P(_u32)]),
    ("glu_dist_local_sorter", _int, [_vp, _P(_vp)]),
    ("glu_dist_prepare", _int, [_vp, _sz, _sz]),
    ("glu_dist_sort_begin", _int, [_vp, _vp, _vp, _sz, _vp, _P(_sz)]),
    ("glu_dist_sort_finish", _int, [_vp, _vp, _vp, _sz, _vp]),
    ("glu_dist_sort_ptr", _int, [_vp, _vp, _vp, _sz, _vp, _P(_vp), _P(_vp), _P(_sz)]),
    ("glu_dist_last_local_sort", _int, [_vp, _P(_u32)]),
    ("glu_dist_set_rounds", _int, [_vp, _int]),
    ("glu_dist_last_rounds", _int, [_vp, _P(_u32)]),
    ("glu_dist_set_reserved_cus", _int, [_vp, _int]),
    ("glu_dist_set_profiling", _int, [_vp, _int]),
    ("glu_dist_phase_times", _int, [_vp, _P(ctypes.c_double), _P(_u64)]),
    ("glu_dist_plan_buckets", _int, [_P(_u32), _int, _P(_int)]),
    ("glu_dist_plan_counts", _int, [_P(_u32), _int, _int, _P(_int), _P(_u64), _P(_u64)]),
    ("glu_dist_plan_groups", _int, [_P(_u32), _int, _P(_int), _int, _P(_int)]),
    ("glu_timer_begin", _int, [_P(_vp)]),
    ("glu_timer_end", _int, [_vp, _P(_u64)]),
]

_lib = None


class GluError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("glu_hip status %d: %s" % (status, message))
        self.status = status
        self.message = message


def lib():
    """Loads libglu_hip.so (built by __graft_entry__.build() / make -C gl-radix-sort_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status):
    if status != GLU_OK:
        raise GluError(status, lib().glu_last_error().decode())


def device_count():
    c = _int(0)
    check(lib().glu_device_count(ctypes.byref(c)))
    return c.value


def set_device(i):
    check(lib().glu_set_device(i))


def device_info():
    buf = ctypes.create_string_buffer(256)
    check(lib().glu_device_info(buf, 256))
    return buf.value.decode()


def synchronize():
    check(lib().glu_device_synchronize())


def queue():
    s = _vp()
    check(lib().glu_queue(ctypes.byref(s)))
    return s.value


class ShaderStorageBuffer:
    """Python mirror of glu::ShaderStorageBuffer (reference glu/gl_utils.hpp:146-246) over the C ABI."""

    def __init__(self, data=None, size=0):
        self._h = _u32(0)
        self._size = 0
        if data is not None:
            a = np.ascontiguousarray(data)
            if a.nbytes == 0:
                raise GluError(GLU_ERROR_INVALID_ARGUMENT, "empty data")
            check(lib().glu_buffer_create_with_data(a.ctypes.data_as(_vp), a.nbytes, ctypes.byref(self._h)))
            self._size = a.nbytes
        elif size > 0:
            self.resize(size)

    @classmethod
    def wrap(cls, device_ptr, size):
        b = cls()
        check(lib().glu_buffer_wrap(_vp(device_ptr), size, ctypes.byref(b._h)))
        b._size = size
        return b

    def handle(self):
        return self._h.value

    def size(self):
        return self._size

    def device_ptr(self):
        p = _vp()
        check(lib().glu_buffer_device_ptr(self._h, ctypes.byref(p)))
        return p.value

    def resize(self, size, keep_data=False):
        if size == self._size:
            return
        new = _u32(0)
        check(lib().glu_buffer_create(size, ctypes.byref(new)))
        if keep_data and self._h.value:
            check(lib().glu_buffer_copy(self._h, new, min(self._size, size), 0, 0))
        if self._h.value:
            check(lib().glu_buffer_destroy(self._h))
        self._h, self._size = new, size

    def clear(self, value=0):
        check(lib().glu_buffer_fill_u32(self._h, value))

    def write_data(self, data):
        a = np.ascontiguousarray(data)
        check(lib().glu_buffer_write(self._h, a.ctypes.data_as(_vp), a.nbytes, 0))

    def get_data(self, dtype):
        dt = np.dtype(dtype)
        if self._size % dt.itemsize:
            raise GluError(GLU_ERROR_INVALID_ARGUMENT, "Size %d isn't a multiple of %d" % (self._size, dt.itemsize))
        out = np.empty(self._size // dt.itemsize, dtype=dt)
        if self._size:
            check(lib().glu_buffer_read(self._h, out.ctypes.data_as(_vp), self._size, 0))
        return out

    def destroy(self):
        if self._h.value and _lib is not None:
            _lib.glu_buffer_destroy(self._h)
        self._h = _u32(0)
        self._size = 0

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def scratch_filled_bytes():
    """The bytes of operator scratch this process has filled under GLU_HIP_SCRATCH_FILL (glu_scratch_filled_bytes; host only): 0
    while the variable was never set.  A test of the switch reads it before and after to show that it was not vacuous."""
    a = _sz(0)
    check(lib().glu_scratch_filled_bytes(ctypes.byref(a)))
    return a.value


def plan_finish(count, key_bytes=4):
    """(first_capacity, last_capacity) of the in-LDS pass's tiles a whole-key sort of `count` elements enqueues by default; (0, 0):
    no attempt to end in LDS (glu_radix_sort_plan_finish; host only)."""
    a, b = _u32(0), _u32(0)
    check(lib().glu_radix_sort_plan_finish(count, key_bytes, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def plan_batch(count, key_bytes=4, with_vals=True):
    """(path, tile) of a batch of equal partitions of `count` elements (glu_radix_sort_plan_batch; host only): path 0 = nothing to
    do, 1 = a wave per partition, 2 = a workgroup per partition, 3 = longer than an LDS tile; tile in elements."""
    a, b = _u32(0), _u32(0)
    check(lib().glu_radix_sort_plan_batch(count, key_bytes, 1 if with_vals else 0, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def plan_reduce_batch(count, elem_bytes=4):
    """(path, workgroups) of a segment of `count` elements of `elem_bytes` bytes in a batched reduce (glu_reduce_plan_batch; host
    only): path 0 = empty, 1 = a wave or part of one per segment, 2 = a workgroup per segment, 3 = several workgroups per segment."""
    a, b = _u32(0), _u32(0)
    check(lib().glu_reduce_plan_batch(count, elem_bytes, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def plan_scan_batch(count, elem_bytes=4):
    """(path, workgroups) of a segment of `count` elements of `elem_bytes` bytes in a batched scan (glu_scan_plan_batch; host
    only): path 0 = empty, 1 = a wave or part of one per segment, 2 = a workgroup per segment, 3 = several workgroups per segment."""
    a, b = _u32(0), _u32(0)
    check(lib().glu_scan_plan_batch(count, elem_bytes, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def plan_key_runs(count, key_bits=32):
    """(tile, tiles, scan_rounds) of key runs over `count` keys of `key_bits` bits (glu_key_runs_plan; host only): keys per tile,
    tiles of keys that start on a 16-byte boundary, rounds of the scan of the tile counts."""
    a, b, c = _u32(0), _u32(0), _u32(0)
    check(lib().glu_key_runs_plan(count, key_bits, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def plan_select(count, stencil_type=SelectStencil_Uint):
    """(tile, tiles, scan_rounds) of a select over `count` elements of a stencil of `stencil_type` (glu_select_plan; host only):
    elements per tile, tiles of a stencil that starts on a 16-byte boundary, rounds of the scan of the tile counts."""
    a, b, c = _u32(0), _u32(0), _u32(0)
    check(lib().glu_select_plan(count, stencil_type, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def plan_select_batch(total, num_segments, stencil_type=SelectStencil_Uint, index_form=SelectIndex_Global):
    """(tile, tiles, scan_rounds, kernels, scratch_bytes) of a batched select over `total` elements in `num_segments` segments
    (glu_select_plan_batch; host only): tile and tiles as plan_select's, the rounds of the scan of tiles + 1 counts, the kernels of a
    call with all three outputs, the bytes prepare_batch reserves."""
    a, b, c, d, e = _u32(0), _u32(0), _u32(0), _u32(0), _sz(0)
    check(lib().glu_select_plan_batch(total, num_segments, stencil_type, index_form, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                      ctypes.byref(d), ctypes.byref(e)))
    return a.value, b.value, c.value, d.value, e.value


def plan_sorted_search(hay_count, needle_count, key_type="uint32", top_entries=0):
    """(path, levels, fanout, index_bytes) of a sorted search of `needle_count` needles in `hay_count` keys on the AUTO path
    (glu_sorted_search_plan; host only): SearchPath_Direct or SearchPath_Indexed, the levels L of the index (whatever the path), the
    keys to a 128-byte line, the bytes of the index.  top_entries 0: the default, what LDS holds."""
    a, b, c, d = _u32(), _u32(), _u32(), _sz()
    check(lib().glu_sorted_search_plan(hay_count, needle_count, KEY_TYPES[key_type], top_entries, ctypes.byref(a), ctypes.byref(b),
                                       ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


def plan_sorted_search_batch(needle_total, key_type="uint32", window_keys=SEARCH_BATCH_WINDOW_DEFAULT):
    """(tile, tiles, window_keys_used, kernels) of a batched sorted search of `needle_total` needles (glu_sorted_search_plan_batch;
    host only): needles per tile, tiles of needles that start on a 16-byte boundary, the window in keys (window_keys: 0, a value in
    the range of the key width or the default, its maximum), 1 kernel (0 for no needles)."""
    a, b, c, d = _u32(), _u32(), _u32(), _u32()
    check(lib().glu_sorted_search_plan_batch(needle_total, KEY_TYPES[key_type], window_keys, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                             ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


def plan_merge(a_count, b_count, key_type="uint32", with_vals=True):
    """(tile, tiles, kernels, scratch_bytes) of a merge of `a_count` and `b_count` keys (glu_merge_plan; host only): the outputs per
    workgroup, ceil((a_count + b_count) / tile), 2 kernels (0 for nothing), the bytes of the split table."""
    a, b, c, d = _u32(), _u32(), _u32(), _sz()
    check(lib().glu_merge_plan(a_count, b_count, KEY_TYPES[key_type], 1 if with_vals else 0, ctypes.byref(a), ctypes.byref(b),
                               ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


def plan_merge_batch(total_count, num_segments, key_type="uint32", with_vals=True):
    """(tile, tiles, kernels, scratch_bytes) of a batched merge of `total_count` = a_total + b_total keys in `num_segments` segments
    (glu_merge_plan_batch; host only): merge's tile, ceil(total_count / tile), 2 kernels (1 for no keys, 0 for no segments), the bytes
    of the boundary table."""
    a, b, c, d = _u32(), _u32(), _u32(), _sz()
    check(lib().glu_merge_plan_batch(total_count, num_segments, KEY_TYPES[key_type], 1 if with_vals else 0, ctypes.byref(a), ctypes.byref(b),
                                     ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


SetOp_Union, SetOp_Intersection, SetOp_Difference, SetOp_SymmetricDifference = 0, 1, 2, 3
SET_OPS = {"union": SetOp_Union, "intersection": SetOp_Intersection, "difference": SetOp_Difference,
           "symmetric_difference": SetOp_SymmetricDifference}


def plan_set_ops(a_count, b_count, key_type="uint32", with_arrays=True):
    """(tile, tiles, kernels, scratch_bytes) of a set operation on `a_count` and `b_count` keys (glu_set_ops_plan; host only): merge's
    tile, ceil((a_count + b_count) / tile), 4 kernels (3 for a call that only counts, 1 for nothing), the bytes of the bounds and the
    tile counts."""
    a, b, c, d = _u32(), _u32(), _u32(), _sz()
    check(lib().glu_set_ops_plan(a_count, b_count, KEY_TYPES[key_type], 1 if with_arrays else 0, ctypes.byref(a), ctypes.byref(b),
                                 ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


def plan_set_ops_batch(a_total, b_total, num_segments, key_type="uint32", with_arrays=True, with_offsets=True):
    """(tile, tiles, kernels, scratch_bytes) of a batched set operation on `a_total` and `b_total` keys in `num_segments` segments
    (glu_set_ops_plan_batch; host only): merge's tile, ceil((a_total + b_total) / tile), 3 kernels + 1 with out_offsets + 1 with
    arrays (1 + with_offsets for no keys, 1 for no segments), the bytes of the bounds, the tile counts and the threads' words."""
    a, b, c, d = _u32(), _u32(), _u32(), _sz()
    check(lib().glu_set_ops_plan_batch(a_total, b_total, num_segments, KEY_TYPES[key_type], 1 if with_arrays else 0,
                                       1 if with_offsets else 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


HistogramMode_Even, HistogramMode_Edges = 0, 1
HistogramPath_Lds, HistogramPath_Global = 0, 1
HISTOGRAM_MODES = {"even": HistogramMode_Even, "edges": HistogramMode_Edges}


def plan_histogram(count, bins, key_type="uint32", mode="even"):
    """(path, threads, tile, groups, kernels, scratch_bytes) of a histogram of `count` samples over `bins` bins (glu_histogram_plan;
    host only): HistogramPath_Lds where bins <= 8192 else HistogramPath_Global, the workgroup and the tile of the counting kernel,
    its workgroups min(ceil(count / tile), groups_max), the kernels of a call that does not accumulate, the bytes of the partial rows."""
    a, b, c, d, e, f = _u32(), _u32(), _u32(), _u32(), _u32(), _sz()
    check(lib().glu_histogram_plan(count, bins, KEY_TYPES[key_type], HISTOGRAM_MODES.get(mode, mode), ctypes.byref(a), ctypes.byref(b),
                                   ctypes.byref(c), ctypes.byref(d), ctypes.byref(e), ctypes.byref(f)))
    return a.value, b.value, c.value, d.value, e.value, f.value


HistogramPath_Batch = 2


def plan_histogram_batch(count, bins, key_type="uint32", mode="even"):
    """(path, workgroups, (wave_limit, block_limit), chunk, scratch_bytes_per_chunk) of one segment of `count` samples in a batched
    histogram over `bins` bins (glu_histogram_plan_batch; host only): path 0 = empty, 1 = a wave per segment, 2 = a workgroup per
    segment, 3 = cut into chunks (workgroups = their number); the limits of the wave class (0 where bins > 2048) and of the block
    class in samples, the samples of a chunk, and the bytes a chunk's partial row takes in the object's scratch."""
    a, b, d, e = _u32(), _u32(), _u32(), _sz()
    c = (_u32 * 2)()
    check(lib().glu_histogram_plan_batch(count, bins, KEY_TYPES[key_type], HISTOGRAM_MODES.get(mode, mode), ctypes.byref(a), ctypes.byref(b),
                                         c, ctypes.byref(d), ctypes.byref(e)))
    return a.value, b.value, (c[0], c[1]), d.value, e.value


def plan_expand(total, num_segments):
    """(tile, tiles, kernels, scratch_bytes) of an expand of `num_segments` segments over `total` elements (glu_expand_plan; host
    only): the merged items (offsets and outputs together) per workgroup, ceil((num_segments + 1 + total) / tile), 2 kernels and the
    bytes of the split table; with no element or no segment, 0 tiles, kernels and bytes."""
    a, b, c, d = _u32(), _u32(), _u32(), _sz()
    check(lib().glu_expand_plan(total, num_segments, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value


def plan_gather(count, item_bytes):
    """(tile, tiles, kernels) of a gather or a scatter of `count` entries of `item_bytes` (glu_gather_plan; host only): the entries
    per workgroup, ceil(count / tile) (a call on an array that starts inside a 16-byte pack can take one more), 1 kernel, or 0
    where count is 0."""
    a, b, c = _u32(), _u32(), _u32()
    check(lib().glu_gather_plan(count, item_bytes, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def plan_top_k(count, k, key_type="uint32", sorted=True, with_arrays=True, path=TopKPath_Auto, cand_capacity=0):
    """What a top-k of `k` of `count` keys does (glu_top_k_plan; host only): {"rounds", "digits": [(shift, bits) per round], "tile",
    "tiles" (glu_select_plan's for the key width), "capacity" (candidates kept), "kernels", "scratch_bytes"}."""
    rounds, tile, tiles, cap, kernels, scratch = _u32(), _u32(), _u32(), _u32(), _u32(), _sz()
    shift, bits = (_u32 * 6)(), (_u32 * 6)()
    check(lib().glu_top_k_plan(count, k, KEY_TYPES[key_type], 1 if sorted else 0, 1 if with_arrays else 0, path, cand_capacity,
                               ctypes.byref(rounds), shift, bits, ctypes.byref(tile), ctypes.byref(tiles), ctypes.byref(cap),
                               ctypes.byref(kernels), ctypes.byref(scratch)))
    return {"rounds": rounds.value, "digits": [(shift[r], bits[r]) for r in range(rounds.value)], "tile": tile.value, "tiles": tiles.value,
            "capacity": cap.value, "kernels": kernels.value, "scratch_bytes": scratch.value}


# glu_top_k_plan_batch's path
TopKBatch_None, TopKBatch_Wave, TopKBatch_Block, TopKBatch_Long, TopKBatch_Loop, TopKBatch_Binned = range(6)


def plan_top_k_batch(count, num_segments, k, key_type="uint32", offsets_form=False, sorted=True, with_arrays=True, loop_min=0):
    """What a batched top-k does (glu_top_k_plan_batch; host only).  count: keys per partition, or the batch's total with
    offsets_form.  {"path" (TopKBatch_*), "tile", "limits" (longest segment of the wave class and the three workgroup tiles),
    "wave_digit_bits", "cand_room", "loop_min", "kernels", "scratch_bytes"}: the single statement of the provisional class limits."""
    path, tile, bits, room, kernels, loop, scratch = _u32(), _u32(), _u32(), _u32(), _u32(), _sz(), _sz()
    limits = (_u32 * 4)()
    check(lib().glu_top_k_plan_batch(count, num_segments, k, KEY_TYPES[key_type], 1 if offsets_form else 0, 1 if sorted else 0,
                                     1 if with_arrays else 0, loop_min, ctypes.byref(path), ctypes.byref(tile), limits, ctypes.byref(bits),
                                     ctypes.byref(room), ctypes.byref(loop), ctypes.byref(kernels), ctypes.byref(scratch)))
    return {"path": path.value, "tile": tile.value, "limits": list(limits), "wave_digit_bits": bits.value, "cand_room": room.value,
            "loop_min": loop.value, "kernels": kernels.value, "scratch_bytes": scratch.value}


def _read_batch(fn, handle):
    a, b, c = _u32(0), _u32(0), _u32(0)
    check(fn(handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return {"wave": a.value, "block": b.value, "long": c.value}


class _Handle:
    """An object of the C ABI behind a handle: _CREATE(*arguments, &handle) makes it, _DESTROY(handle) ends it, once."""

    _CREATE = _DESTROY = None
    _borrowed = False  # the handle belongs to another object (Dist.sorter): never destroyed from here

    def _create(self, *arguments):
        self._h = _vp()
        check(getattr(lib(), self._CREATE)(*arguments, ctypes.byref(self._h)))

    def destroy(self):
        if self._h and _lib is not None and not self._borrowed:
            getattr(_lib, self._DESTROY)(self._h)
        self._h = _vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class RadixSort(_Handle):
    """glu::RadixSort (reference glu/RadixSort.hpp:186-354) over the C ABI."""

    _CREATE, _DESTROY = "glu_radix_sort_create", "glu_radix_sort_destroy"

    def __init__(self, digit_bits=None, options=None):
        """options: {name: integer} switches for tests / tuning (glu_radix_sort_set_option; names as in the environment, with or
        without the GLU_HIP_ prefix) -- set on THIS object, the process environment is not touched."""
        self._create()
        if digit_bits is not None:
            check(lib().glu_radix_sort_set_digit_bits(self._h, digit_bits))
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def set_option(self, name, value):
        check(lib().glu_radix_sort_set_option(self._h, str(name).encode(), int(value)))

    def set_digit_bits(self, bits):
        check(lib().glu_radix_sort_set_digit_bits(self._h, bits))

    @property
    def digit_bits(self):
        b = _u32(0)
        check(lib().glu_radix_sort_get_digit_bits(self._h, ctypes.byref(b)))
        return b.value

    def prepare_internal_buffers(self, count, key_bytes=4, with_vals=True):
        """Grow-only scratch for `count` elements (RadixSort.hpp:237-271); key_bytes 4 or 8, with_vals False for
        keys-only sorts.  After it the matching run call allocates nothing."""
        check(lib().glu_radix_sort_prepare_ex(self._h, count, key_bytes, 1 if with_vals else 0))

    def scratch_size(self):
        s = _sz(0)
        check(lib().glu_radix_sort_scratch_size(self._h, ctypes.byref(s)))
        return s.value

    def scratch_placement(self):
        """What the last prepare measured when it placed the large scratch arrays (glu_radix_sort_scratch_placement):
        {"candidates": n, "chosen_ms": t, "slowest_ms": t}; candidates == 0: no measurement was made."""
        n, a, b = _u32(0), ctypes.c_double(0), ctypes.c_double(0)
        check(lib().glu_radix_sort_scratch_placement(self._h, ctypes.byref(n), ctypes.byref(a), ctypes.byref(b)))
        return {"candidates": int(n.value), "chosen_ms": float(a.value), "slowest_ms": float(b.value)}

    def set_profiling(self, enable):
        """True: events at every kernel boundary of a pass; "light": only around the kernel that moves a pass's data (the scatter,
        the in-LDS pass) -- a few microseconds of queue time per event saved; False: off."""
        check(lib().glu_radix_sort_set_profiling(self._h, 2 if enable == "light" else (1 if enable else 0)))

    def read_profile(self):
        """{count_ms, scan_ms, scatter_ms, passes}: summed device time per kernel class since the last read."""
        c, s, x = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        n = _u64(0)
        f, fn = ctypes.c_double(0), _u64(0)
        check(lib().glu_radix_sort_read_profile_finish(self._h, ctypes.byref(c), ctypes.byref(s), ctypes.byref(x),
                                                       ctypes.byref(n), ctypes.byref(f), ctypes.byref(fn)))
        return {"count_ms": c.value, "scan_ms": s.value, "scatter_ms": x.value, "passes": n.value,
                "finish_ms": f.value, "finish_passes": fn.value}

    def read_plan(self, passes, roles=False):
        """(skipped[passes], counted_alone[passes]) -- with roles=True also pair_role[passes] -- of the last planned sort
        (>= 2^22 elements); synchronise first."""
        sk, ca, ro = (_u32 * passes)(), (_u32 * passes)(), (_u32 * passes)()
        check(lib().glu_radix_sort_read_plan(self._h, sk, ca, ro, passes))
        return (list(sk), list(ca), list(ro)) if roles else (list(sk), list(ca))

    def read_finish(self):
        """{attempted, accepted, longest_run, capacity} of the last sort: did it try to / did it end in LDS
        (glu_radix_sort_read_finish); synchronise first."""
        a, b, c, d, e = _u32(0), _u32(0), _u32(0), _u32(0), _u32(0)
        check(lib().glu_radix_sort_read_finish(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d),
                                               ctypes.byref(e)))
        return {"attempted": a.value, "accepted": b.value, "longest_run": c.value, "capacity": d.value, "top_bit": e.value}

    def read_handoff(self):
        """{narrow}: 1 if the last sort handed its in-LDS pass 2-byte keys in the object's side array (glu_radix_sort_read_handoff);
        synchronise first."""
        a = _u32(0)
        check(lib().glu_radix_sort_read_handoff(self._h, ctypes.byref(a)))
        return {"narrow": a.value}

    def read_long_runs(self):
        """{runs, sub_blocks, pairs}: what the last sort that ended in LDS gave to the segmented passes for runs longer than the tile
        (glu_radix_sort_read_long_runs); waits for the device."""
        a, b, c = _u32(0), _u32(0), _u32(0)
        check(lib().glu_radix_sort_read_long_runs(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"runs": a.value, "sub_blocks": b.value, "pairs": c.value}

    def read_seg_finish(self):
        """{attempted, accepted, longest_run, capacity, runs, tile, split} of the last SEGMENTED sort: did it try to / did it end
        in LDS (glu_radix_sort_read_seg_finish); waits for the device."""
        a, b, c, d, e, f, g = (_u32(0) for _ in range(7))
        check(lib().glu_radix_sort_read_seg_finish(self._h, *(ctypes.byref(x) for x in (a, b, c, d, e, f, g))))
        return {"attempted": a.value, "accepted": b.value, "longest_run": c.value, "capacity": d.value, "runs": e.value,
                "tile": f.value, "split": g.value}

    def __call__(self, key_buffer, val_buffer, count, num_steps=0, key_bytes=4):
        kb = key_buffer.handle() if isinstance(key_buffer, ShaderStorageBuffer) else key_buffer
        vb = val_buffer.handle() if isinstance(val_buffer, ShaderStorageBuffer) else val_buffer
        fn = lib().glu_radix_sort_run if key_bytes == 4 else lib().glu_radix_sort_run_u64
        check(fn(self._h, kb, vb, count, num_steps))

    def sort_keys(self, key_buffer, count, num_steps=0):
        """Keys-only sort of a uint32 buffer (no value buffer at all)."""
        kb = key_buffer.handle() if isinstance(key_buffer, ShaderStorageBuffer) else key_buffer
        check(lib().glu_radix_sort_run_keys(self._h, kb, count, num_steps))

    def sort_keys_ptr(self, keys_ptr, count, num_steps=0, stream=None, key_bytes=4):
        fn = lib().glu_radix_sort_run_keys_ptr if key_bytes == 4 else lib().glu_radix_sort_run_keys_u64_ptr
        check(fn(self._h, _vp(keys_ptr), count, num_steps, _vp(stream)))

    KEY_TYPES = {"uint32": 0, "int32": 1, "float32": 2, "uint64": 3, "int64": 4, "float64": 5}

    def sort_typed_ptr(self, keys_ptr, vals_ptr, count, key_type, stream=None):
        """key_type: a numpy dtype name in KEY_TYPES; vals_ptr may be None (keys only)."""
        check(lib().glu_radix_sort_run_typed_ptr(self._h, _vp(keys_ptr), _vp(vals_ptr), count, self.KEY_TYPES[key_type],
                                                 _vp(stream)))

    def sort_batch_ptr(self, keys_ptr, vals_ptr, count, num_partitions, key_type="uint32", stream=None):
        """Batched sort: num_partitions adjacent partitions of `count` elements, each sorted on its own, in place
        (glu_radix_sort_run_batch_ptr); vals_ptr may be None (keys only)."""
        check(lib().glu_radix_sort_run_batch_ptr(self._h, _vp(keys_ptr), _vp(vals_ptr), count, num_partitions,
                                                 self.KEY_TYPES[key_type], _vp(stream)))

    def sort_batch_offsets_ptr(self, keys_ptr, vals_ptr, total, offsets_ptr, num_segments, key_type="uint32", stream=None):
        """Batched sort of the segments [offsets[s], offsets[s + 1]) -- offsets_ptr: DEVICE array of num_segments + 1 uint32 --
        each on its own, in place (glu_radix_sort_run_batch_offsets_ptr); vals_ptr may be None (keys only)."""
        check(lib().glu_radix_sort_run_batch_offsets_ptr(self._h, _vp(keys_ptr), _vp(vals_ptr), total, _vp(offsets_ptr),
                                                         num_segments, self.KEY_TYPES[key_type], _vp(stream)))

    def prepare_batch(self, total, num_segments, key_bytes=4, with_vals=True):
        """Grow-only scratch for batched sorts of up to `total` elements in up to `num_segments` segments: after it the two
        calls above allocate nothing (glu_radix_sort_prepare_batch)."""
        check(lib().glu_radix_sort_prepare_batch(self._h, total, num_segments, key_bytes, 1 if with_vals else 0))

    def read_batch(self):
        """{wave, block, long}: segments each path of the last batched call took (glu_radix_sort_read_batch); synchronise first."""
        return _read_batch(lib().glu_radix_sort_read_batch, self._h)

    def sort_bit_range_ptr(self, keys_ptr, vals_ptr, count, begin_bit, end_bit, stream=None, key_bytes=4):
        """Stable sort by the key bits [begin_bit, end_bit) only; vals_ptr may be None (keys only)."""
        check(lib().glu_radix_sort_run_bit_range_ptr(self._h, _vp(keys_ptr), _vp(vals_ptr), count, key_bytes * 8, begin_bit,
                                                     end_bit, _vp(stream)))

    def run_ptr(self, keys_ptr, vals_ptr, count, num_steps=0, stream=None, key_bytes=4):
        fn = lib().glu_radix_sort_run_ptr if key_bytes == 4 else lib().glu_radix_sort_run_u64_ptr
        check(fn(self._h, _vp(keys_ptr), _vp(vals_ptr), count, num_steps, _vp(stream)))

    def run_segments_ptr(self, in_keys, in_vals, out_keys, out_vals, count, piece_begin, piece_len, piece_segment,
                         num_segments, key_bits, stream=None):
        """Segmented stable sort (glu_radix_sort_run_segments_ptr): the pieces [piece_begin[i], + piece_len[i]) of the
        input arrays, grouped into segments piece_segment[i], leave as segments in ascending order, each stably sorted by
        its low key_bits bits; the input arrays are clobbered."""
        pb = np.ascontiguousarray(piece_begin, dtype=np.uint64)
        pl = np.ascontiguousarray(piece_len, dtype=np.uint64)
        ps = np.ascontiguousarray(piece_segment, dtype=np.uint32)
        assert pb.shape == pl.shape == ps.shape and pb.ndim == 1
        check(lib().glu_radix_sort_run_segments_ptr(
            self._h, _vp(in_keys), _vp(in_vals), _vp(out_keys), _vp(out_vals), count,
            pb.ctypes.data_as(_P(_u64)), pl.ctypes.data_as(_P(_u64)), ps.ctypes.data_as(_P(_u32)), pb.shape[0],
            num_segments, key_bits, _vp(stream)))

    def partition_ptr(self, src_keys, src_vals, dst_keys, dst_vals, count, shift, bits, histogram_ptr=None,
                      stream=None):
        check(lib().glu_radix_sort_partition_ptr(self._h, _vp(src_keys), _vp(src_vals), _vp(dst_keys), _vp(dst_vals),
                                                 count, shift, bits, _vp(histogram_ptr), _vp(stream)))


class KeyRuns(_Handle):
    """glu::KeyRuns (not in the reference) over the C ABI: the runs of equal keys as offsets for the batched calls."""

    _CREATE, _DESTROY = "glu_key_runs_create", "glu_key_runs_destroy"

    MAX_COMPOSED_RUNS = 1 << 24  # the limit of the batched calls, which run_by_key_ptr of Reduce and BlellochScan go through

    def __init__(self):
        self._create()

    def prepare(self, count, key_bits=32):
        """Scratch for up to `count` keys: after it run_ptr allocates nothing (capturable) (glu_key_runs_prepare)."""
        check(lib().glu_key_runs_prepare(self._h, count, key_bits))

    def run_ptr(self, keys_ptr, count, offsets_ptr, max_runs, num_runs_ptr, unique_keys_ptr=None, key_bits=32, begin_bit=0,
                end_bit=None, stream=None):
        """offsets[0 .. max_runs] = the heads of the runs of keys equal in the bits [begin_bit, end_bit) (end_bit None: key_bits),
        then `count`; unique_keys[r] = the key at head r (None skips it); *num_runs = the number of runs, also beyond max_runs.
        All pointers are device pointers; the keys are only read (glu_key_runs_run_ptr)."""
        check(lib().glu_key_runs_run_ptr(self._h, _vp(keys_ptr), count, key_bits, begin_bit, key_bits if end_bit is None else end_bit,
                                         _vp(unique_keys_ptr), _vp(offsets_ptr), max_runs, _vp(num_runs_ptr), _vp(stream)))


class Select(_Handle):
    """glu::Select (not in the reference) over the C ABI: stable stream compaction by a stencil and a comparison."""

    _CREATE, _DESTROY = "glu_select_create", "glu_select_destroy"

    _THRESHOLD_TYPES = {SelectStencil_Float: ctypes.c_float, SelectStencil_Double: ctypes.c_double, SelectStencil_Int: ctypes.c_int32,
                        SelectStencil_Uint: ctypes.c_uint32, SelectStencil_Byte: ctypes.c_uint8}

    def __init__(self):
        self._create()

    def prepare(self, count, stencil_type=SelectStencil_Uint):
        """Scratch for up to `count` elements: after it run_ptr allocates nothing (capturable) (glu_select_prepare)."""
        check(lib().glu_select_prepare(self._h, count, stencil_type))

    def run_ptr(self, stencil_ptr, count, max_out, num_selected_ptr, out_indices_ptr=None, items_ptr=None, out_items_ptr=None,
                item_bytes=4, stencil_type=SelectStencil_Uint, op=SelectOperator_NE, threshold=None, stream=None):
        """Element i is selected iff stencil[i] `op` threshold (a Python number, packed into the stencil's type; None: zero).
        out_indices[r] = the index of the r-th selected element, out_items[r] = its item (either may be None), for r below
        min(selected, max_out); *num_selected = the number selected, also beyond max_out.  All pointers are device pointers; the
        stencil and the items are only read (glu_select_run_ptr)."""
        value = self._threshold(threshold, stencil_type)
        check(lib().glu_select_run_ptr(self._h, _vp(stencil_ptr), stencil_type, op, ctypes.byref(value) if value is not None else None, count,
                                       _vp(items_ptr), item_bytes, _vp(out_items_ptr), _vp(out_indices_ptr), max_out, _vp(num_selected_ptr),
                                       _vp(stream)))

    @classmethod
    def _threshold(cls, threshold, stencil_type):
        """`threshold` packed into the stencil's type (None: the call's NULL, zero)."""
        value = None
        if threshold is not None and stencil_type in cls._THRESHOLD_TYPES:
            ctype = cls._THRESHOLD_TYPES[stencil_type]
            if ctype not in (ctypes.c_float, ctypes.c_double):
                bits = 8 * ctypes.sizeof(ctype)
                lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if ctype is ctypes.c_int32 else (0, (1 << bits) - 1)
                if int(threshold) != threshold or not lo <= int(threshold) <= hi:
                    raise GluError(GLU_ERROR_INVALID_ARGUMENT, "threshold %r is no value of the stencil's type" % (threshold,))
                threshold = int(threshold)
            value = ctype(threshold)
        return value

    def prepare_batch(self, total, num_segments, stencil_type=SelectStencil_Uint):
        """Scratch for batches of up to `total` elements: after it the batched calls allocate nothing (capturable)
        (glu_select_prepare_batch)."""
        check(lib().glu_select_prepare_batch(self._h, total, num_segments, stencil_type))

    def run_batch_ptr(self, stencil_ptr, count, num_partitions, max_out, num_selected_ptr, out_indices_ptr=None, items_ptr=None,
                      out_items_ptr=None, item_bytes=4, out_offsets_ptr=None, index_form=SelectIndex_Global,
                      stencil_type=SelectStencil_Uint, op=SelectOperator_NE, threshold=None, stream=None):
        """run_ptr over `num_partitions` segments of `count` elements each: the same compaction, out_offsets[0 .. num_partitions] = the
        offsets of the compacted segments (clamped to max_out), and with SelectIndex_Local the indices inside the element's segment
        (glu_select_run_batch_ptr)."""
        value = self._threshold(threshold, stencil_type)
        check(lib().glu_select_run_batch_ptr(self._h, _vp(stencil_ptr), stencil_type, op, ctypes.byref(value) if value is not None else None,
                                             count, num_partitions, _vp(items_ptr), item_bytes, _vp(out_items_ptr), _vp(out_indices_ptr),
                                             index_form, max_out, _vp(out_offsets_ptr), _vp(num_selected_ptr), _vp(stream)))

    def run_batch_offsets_ptr(self, stencil_ptr, total, offsets_ptr, num_segments, max_out, num_selected_ptr, out_indices_ptr=None,
                              items_ptr=None, out_items_ptr=None, item_bytes=4, out_offsets_ptr=None, index_form=SelectIndex_Global,
                              stencil_type=SelectStencil_Uint, op=SelectOperator_NE, threshold=None, stream=None):
        """The same over the segments [offsets[s], offsets[s + 1]) of device offsets (num_segments + 1 words, what KeyRuns writes):
        only the elements from offsets[0] to offsets[num_segments] can be selected (glu_select_run_batch_offsets_ptr)."""
        value = self._threshold(threshold, stencil_type)
        check(lib().glu_select_run_batch_offsets_ptr(self._h, _vp(stencil_ptr), stencil_type, op,
                                                     ctypes.byref(value) if value is not None else None, total, _vp(offsets_ptr), num_segments,
                                                     _vp(items_ptr), item_bytes, _vp(out_items_ptr), _vp(out_indices_ptr), index_form, max_out,
                                                     _vp(out_offsets_ptr), _vp(num_selected_ptr), _vp(stream)))


class SortedSearch(_Handle):
    """glu::SortedSearch (not in the reference) over the C ABI: lower and upper bounds of many needles in a sorted haystack."""

    _CREATE, _DESTROY = "glu_sorted_search_create", "glu_sorted_search_destroy"

    NEEDLE_PACKS = 2  # 16-byte packs of needles per thread and tile (sorted_search_kernels.hpp: kSearchPacks)

    def __init__(self):
        self._create()

    @classmethod
    def needle_tile(cls, key_type="uint32"):
        """Needles per tile of the indexed search kernel: 256 threads x NEEDLE_PACKS packs of 16 bytes."""
        return 256 * cls.NEEDLE_PACKS * (16 // np.dtype(key_type).itemsize)

    def prepare(self, hay_count, key_type="uint32"):
        """Scratch for the index of `hay_count` keys at the TOP_ENTRIES set now: later calls allocate nothing (capturable)
        (glu_sorted_search_prepare)."""
        check(lib().glu_sorted_search_prepare(self._h, hay_count, KEY_TYPES[key_type]))

    def set_option(self, name, value):
        """"PATH": SearchPath_Auto, _Direct or _Indexed; "TOP_ENTRIES": the most entries of the index's top level
        (glu_sorted_search_set_option).  Anything else is refused."""
        check(lib().glu_sorted_search_set_option(self._h, name.encode(), value))

    def index_ptr(self, hay_ptr, hay_count, key_type="uint32", stream=None):
        """Builds the index of the haystack and remembers it for run_ptr(reuse_index=True) (glu_sorted_search_index_ptr)."""
        check(lib().glu_sorted_search_index_ptr(self._h, _vp(hay_ptr), hay_count, KEY_TYPES[key_type], _vp(stream)))

    def run_ptr(self, hay_ptr, hay_count, needles_ptr, needle_count, out_lower_ptr=None, out_upper_ptr=None, key_type="uint32",
                reuse_index=False, stream=None):
        """out_lower[j] = the keys of the haystack below needles[j], out_upper[j] = the keys not above it, in the sort's order;
        either may be None.  All pointers are device pointers; the haystack and the needles are only read
        (glu_sorted_search_run_ptr)."""
        check(lib().glu_sorted_search_run_ptr(self._h, _vp(hay_ptr), hay_count, _vp(needles_ptr), needle_count, KEY_TYPES[key_type],
                                              _vp(out_lower_ptr), _vp(out_upper_ptr), 1 if reuse_index else 0, _vp(stream)))

    def run_batch_ptr(self, hay_ptr, hay_count, needles_ptr, needle_count, num_partitions, out_lower_ptr=None, out_upper_ptr=None,
                      key_type="uint32", stream=None):
        """Row p of `needle_count` needles searched in row p of `hay_count` keys, for num_partitions rows in one kernel; the
        positions are local to the row, as torch.searchsorted gives them (glu_sorted_search_run_batch_ptr)."""
        check(lib().glu_sorted_search_run_batch_ptr(self._h, _vp(hay_ptr), hay_count, _vp(needles_ptr), needle_count, num_partitions,
                                                    KEY_TYPES[key_type], _vp(out_lower_ptr), _vp(out_upper_ptr), _vp(stream)))

    def run_batch_offsets_ptr(self, hay_ptr, hay_total, hay_offsets_ptr, needles_ptr, needle_total, needle_offsets_ptr, num_segments,
                              out_lower_ptr=None, out_upper_ptr=None, key_type="uint32", stream=None):
        """The needles of segment s searched in the haystack of segment s, both from device offsets of num_segments + 1 uint32
        (needle_offsets_ptr None: equal rows of needle_total / num_segments needles); positions local to the segment
        (glu_sorted_search_run_batch_offsets_ptr)."""
        check(lib().glu_sorted_search_run_batch_offsets_ptr(self._h, _vp(hay_ptr), hay_total, _vp(hay_offsets_ptr), _vp(needles_ptr),
                                                            needle_total, _vp(needle_offsets_ptr), num_segments, KEY_TYPES[key_type],
                                                            _vp(out_lower_ptr), _vp(out_upper_ptr), _vp(stream)))

    def set_batch_window(self, keys):
        """The most keys of a tile's haystacks that the batched calls stage in LDS: 0 (never), 16 .. 32768 / key bytes, or
        SEARCH_BATCH_WINDOW_DEFAULT (glu_sorted_search_set_batch_window)."""
        check(lib().glu_sorted_search_set_batch_window(self._h, keys))

    def last(self):
        """(path, levels, kernels) of what the last index_ptr, run_ptr or batched call enqueued (glu_sorted_search_last; no device
        read)."""
        a, b, c = _u32(), _u32(), _u32()
        check(lib().glu_sorted_search_last(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value


class Merge(_Handle):
    """glu::Merge (not in the reference) over the C ABI: two sorted arrays of keys, with or without uint32 values, into one, stable."""

    _CREATE, _DESTROY = "glu_merge_create", "glu_merge_destroy"

    def __init__(self):
        self._create()

    def prepare(self, total_count, key_type="uint32"):
        """Scratch for calls of up to `total_count` = a_count + b_count keys: they allocate nothing (capturable) (glu_merge_prepare)."""
        check(lib().glu_merge_prepare(self._h, total_count, KEY_TYPES[key_type]))

    def run_ptr(self, a_keys_ptr, a_vals_ptr, a_count, b_keys_ptr, b_vals_ptr, b_count, out_keys_ptr, out_vals_ptr, key_type="uint32",
                stream=None):
        """out = the stable sort of A || B by the sort's order of keys, A first among equal keys; both inputs sorted in that order and
        only read.  All pointers are device pointers; the three value pointers are all None or all set (glu_merge_run_ptr)."""
        check(lib().glu_merge_run_ptr(self._h, _vp(a_keys_ptr), _vp(a_vals_ptr), a_count, _vp(b_keys_ptr), _vp(b_vals_ptr), b_count,
                                      _vp(out_keys_ptr), _vp(out_vals_ptr), KEY_TYPES[key_type], _vp(stream)))

    def prepare_batch(self, total_count, key_type="uint32"):
        """Scratch for batched calls of up to `total_count` = a_total + b_total keys: they allocate nothing (capturable)
        (glu_merge_prepare_batch)."""
        check(lib().glu_merge_prepare_batch(self._h, total_count, KEY_TYPES[key_type]))

    def run_batch_offsets_ptr(self, a_keys_ptr, a_vals_ptr, a_offsets_ptr, a_total, b_keys_ptr, b_vals_ptr, b_offsets_ptr, b_total,
                              num_segments, out_keys_ptr, out_vals_ptr, out_offsets_ptr=None, key_type="uint32", stream=None):
        """Segment s of the output = the merge of A[a_offsets[s], a_offsets[s + 1]) and B[b_offsets[s], b_offsets[s + 1]), the
        segments back to back; the offsets are device arrays of num_segments + 1 uint32 words, a_total and b_total the arrays'
        lengths.  out_offsets (optional) receives the num_segments + 1 output offsets (glu_merge_run_batch_offsets_ptr)."""
        check(lib().glu_merge_run_batch_offsets_ptr(self._h, _vp(a_keys_ptr), _vp(a_vals_ptr), _vp(a_offsets_ptr), a_total, _vp(b_keys_ptr),
                                                    _vp(b_vals_ptr), _vp(b_offsets_ptr), b_total, num_segments, _vp(out_keys_ptr),
                                                    _vp(out_vals_ptr), _vp(out_offsets_ptr), KEY_TYPES[key_type], _vp(stream)))

    def run_batch_ptr(self, a_keys_ptr, a_vals_ptr, a_len, b_keys_ptr, b_vals_ptr, b_len, num_segments, out_keys_ptr, out_vals_ptr,
                      out_offsets_ptr=None, key_type="uint32", stream=None):
        """The same over equal partitions: segment s is A[s * a_len, (s + 1) * a_len) and B[s * b_len, (s + 1) * b_len)
        (glu_merge_run_batch_ptr)."""
        check(lib().glu_merge_run_batch_ptr(self._h, _vp(a_keys_ptr), _vp(a_vals_ptr), a_len, _vp(b_keys_ptr), _vp(b_vals_ptr), b_len,
                                            num_segments, _vp(out_keys_ptr), _vp(out_vals_ptr), _vp(out_offsets_ptr), KEY_TYPES[key_type],
                                            _vp(stream)))

    def last(self):
        """(tiles, kernels) of what the last run_ptr or batched call enqueued (glu_merge_last; no device read)."""
        a, b = _u32(), _u32()
        check(lib().glu_merge_last(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class SetOps(_Handle):
    """glu::SetOps (not in the reference) over the C ABI: union, intersection, difference and symmetric difference of two sorted
    arrays of keys, with or without uint32 values, with std::set_* multiset semantics; the result and its length on the device."""

    _CREATE, _DESTROY = "glu_set_ops_create", "glu_set_ops_destroy"

    def __init__(self):
        self._create()

    def prepare(self, total_count, key_type="uint32"):
        """Scratch for calls of up to `total_count` = a_count + b_count keys: they allocate nothing (capturable) (glu_set_ops_prepare)."""
        check(lib().glu_set_ops_prepare(self._h, total_count, KEY_TYPES[key_type]))

    def run_ptr(self, op, a_keys_ptr, a_vals_ptr, a_count, b_keys_ptr, b_vals_ptr, b_count, out_keys_ptr, out_vals_ptr, max_out,
                num_out_ptr, key_type="uint32", stream=None):
        """`op`: "union", "intersection", "difference" or "symmetric_difference" (or a SetOp_* constant).  The kept elements in merge's
        order go to out[0 .. min(S, max_out)), their number S to *num_out (a uint32 on the device), also when S > max_out.  With
        out_keys_ptr None or max_out 0 the call only counts.  Both inputs sorted in the sort's order and only read; all pointers are
        device pointers (glu_set_ops_run_ptr)."""
        check(lib().glu_set_ops_run_ptr(self._h, SET_OPS.get(op, op), _vp(a_keys_ptr), _vp(a_vals_ptr), a_count, _vp(b_keys_ptr),
                                        _vp(b_vals_ptr), b_count, _vp(out_keys_ptr), _vp(out_vals_ptr), max_out, _vp(num_out_ptr),
                                        KEY_TYPES[key_type], _vp(stream)))

    def prepare_batch(self, total_count, num_segments=1, key_type="uint32"):
        """Scratch for batched calls of up to `total_count` = a_total + b_total keys: they allocate nothing (capturable)
        (glu_set_ops_prepare_batch)."""
        check(lib().glu_set_ops_prepare_batch(self._h, total_count, num_segments, KEY_TYPES[key_type]))

    def run_batch_offsets_ptr(self, op, a_keys_ptr, a_vals_ptr, a_offsets_ptr, a_total, b_keys_ptr, b_vals_ptr, b_offsets_ptr, b_total,
                              num_segments, out_keys_ptr, out_vals_ptr, max_out, num_out_ptr, out_offsets_ptr=None, key_type="uint32",
                              stream=None):
        """Segment s of the result = `op` of A[a_offsets[s], a_offsets[s + 1]) and B[b_offsets[s], b_offsets[s + 1]), the segments'
        results back to back; the offsets are device arrays of num_segments + 1 uint32 words, a_total and b_total the arrays' lengths.
        *num_out receives the total kept; out_offsets (optional) the num_segments + 1 offsets of the compacted segments, held to
        max_out (not in a call that only counts) (glu_set_ops_run_batch_offsets_ptr)."""
        check(lib().glu_set_ops_run_batch_offsets_ptr(self._h, SET_OPS.get(op, op), _vp(a_keys_ptr), _vp(a_vals_ptr), _vp(a_offsets_ptr),
                                                      a_total, _vp(b_keys_ptr), _vp(b_vals_ptr), _vp(b_offsets_ptr), b_total, num_segments,
                                                      _vp(out_keys_ptr), _vp(out_vals_ptr), max_out, _vp(out_offsets_ptr), _vp(num_out_ptr),
                                                      KEY_TYPES[key_type], _vp(stream)))

    def run_batch_ptr(self, op, a_keys_ptr, a_vals_ptr, a_len, b_keys_ptr, b_vals_ptr, b_len, num_segments, out_keys_ptr, out_vals_ptr,
                      max_out, num_out_ptr, out_offsets_ptr=None, key_type="uint32", stream=None):
        """The same over equal partitions: segment s is A[s * a_len, (s + 1) * a_len) and B[s * b_len, (s + 1) * b_len)
        (glu_set_ops_run_batch_ptr)."""
        check(lib().glu_set_ops_run_batch_ptr(self._h, SET_OPS.get(op, op), _vp(a_keys_ptr), _vp(a_vals_ptr), a_len, _vp(b_keys_ptr),
                                              _vp(b_vals_ptr), b_len, num_segments, _vp(out_keys_ptr), _vp(out_vals_ptr), max_out,
                                              _vp(out_offsets_ptr), _vp(num_out_ptr), KEY_TYPES[key_type], _vp(stream)))

    def last(self):
        """(tiles, kernels) of what the last run_ptr or batched call enqueued (glu_set_ops_last; no device read)."""
        a, b = _u32(), _u32()
        check(lib().glu_set_ops_last(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


_HISTOGRAM_BOUNDS = {"uint32": ctypes.c_uint32, "int32": ctypes.c_int32, "float32": ctypes.c_float, "float64": ctypes.c_double,
                     "uint64": ctypes.c_uint64, "int64": ctypes.c_int64}


class Histogram(_Handle):
    """glu::Histogram (not in the reference) over the C ABI: uint32 counts of the samples per bin, over even bins or sorted edges."""

    _CREATE, _DESTROY = "glu_histogram_create", "glu_histogram_destroy"

    def __init__(self):
        self._create()

    def prepare(self, count, bins):
        """Scratch for calls of up to `count` samples and `bins` bins: they allocate nothing (capturable) (glu_histogram_prepare)."""
        check(lib().glu_histogram_prepare(self._h, count, bins))

    def run_even_ptr(self, samples_ptr, count, lo, hi, bins, out_counts_ptr, key_type="uint32", accumulate=False, stream=None):
        """`bins` even bins over [lo, hi).  lo and hi are Python numbers: integers that the sample's type holds (others are refused),
        floats rounded to the sample's type (for float32 samples lo = 0.1 means np.float32(0.1), which the kernels widen to double).
        Integers: (hi - lo) / bins a whole number, the bin exact; floats: min(uint32((double(x) - lo) * (bins / (hi - lo))),
        bins - 1).  lo = 0, hi = bins over uint32 is bincount.  Pointers are device pointers (glu_histogram_run_even_ptr)."""
        lo_v, hi_v = self._bounds(lo, hi, key_type)
        check(lib().glu_histogram_run_even_ptr(self._h, _vp(samples_ptr), count, KEY_TYPES[key_type], ctypes.byref(lo_v), ctypes.byref(hi_v),
                                               bins, _vp(out_counts_ptr), 1 if accumulate else 0, _vp(stream)))

    @staticmethod
    def _bounds(lo, hi, key_type):
        """lo and hi as one value each of the sample's type, for the host pointers of the even-bins calls."""
        c = _HISTOGRAM_BOUNDS[key_type]
        try:
            lo_v, hi_v = c(lo), c(hi)
        except TypeError:  # (a fraction for an integer type)
            raise GluError(GLU_ERROR_INVALID_ARGUMENT, "lo or hi is not a value of %s: %r, %r" % (key_type, lo, hi))
        # (a float32 bound is rounded to float32, as numpy rounds a Python float it stores in a float32 array; an integer bound that
        # the type does not hold is refused, not wrapped)
        if key_type in ("uint32", "int32", "uint64", "int64") and (lo_v.value != lo or hi_v.value != hi):
            raise GluError(GLU_ERROR_INVALID_ARGUMENT, "lo or hi is not a value of %s: %r, %r" % (key_type, lo, hi))
        return lo_v, hi_v

    def run_edges_ptr(self, samples_ptr, count, edges_ptr, bins, out_counts_ptr, key_type="uint32", accumulate=False, stream=None):
        """Bins between the bins + 1 non-decreasing DEVICE edges of the sample's type: bin b counts edges[b] <= x < edges[b + 1], floats
        as IEEE values (NaN samples dropped) (glu_histogram_run_edges_ptr)."""
        check(lib().glu_histogram_run_edges_ptr(self._h, _vp(samples_ptr), count, KEY_TYPES[key_type], _vp(edges_ptr), bins,
                                                _vp(out_counts_ptr), 1 if accumulate else 0, _vp(stream)))

    def last(self):
        """(path, groups, kernels) of what the last run enqueued (glu_histogram_last; no device read)."""
        a, b, c = _u32(), _u32(), _u32()
        check(lib().glu_histogram_last(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def prepare_batch(self, total, num_segments, bins):
        """Scratch for batched calls of up to `total` samples in up to `num_segments` segments over `bins` bins: they allocate nothing
        (capturable) (glu_histogram_prepare_batch)."""
        check(lib().glu_histogram_prepare_batch(self._h, total, num_segments, bins))

    def run_batch_even_ptr(self, samples_ptr, count, num_partitions, lo, hi, bins, out_counts_ptr, key_type="uint32", accumulate=False,
                           stream=None):
        """out_counts[p * bins + b] = the samples of partition p, [p * count, (p + 1) * count), in even bin b over [lo, hi): run_even_ptr's
        rule for every partition, in one call (glu_histogram_run_batch_even_ptr)."""
        lo_v, hi_v = self._bounds(lo, hi, key_type)
        check(lib().glu_histogram_run_batch_even_ptr(self._h, _vp(samples_ptr), count, num_partitions, KEY_TYPES[key_type], ctypes.byref(lo_v),
                                                     ctypes.byref(hi_v), bins, _vp(out_counts_ptr), 1 if accumulate else 0, _vp(stream)))

    def run_batch_offsets_even_ptr(self, samples_ptr, total, offsets_ptr, num_segments, lo, hi, bins, out_counts_ptr, key_type="uint32",
                                   accumulate=False, stream=None):
        """The same for the segments [offsets[s], offsets[s + 1]) of `total` samples; `offsets` is a device array of num_segments + 1
        uint32, only read (glu_histogram_run_batch_offsets_even_ptr)."""
        lo_v, hi_v = self._bounds(lo, hi, key_type)
        check(lib().glu_histogram_run_batch_offsets_even_ptr(self._h, _vp(samples_ptr), total, _vp(offsets_ptr), num_segments, KEY_TYPES[key_type],
                                                             ctypes.byref(lo_v), ctypes.byref(hi_v), bins, _vp(out_counts_ptr),
                                                             1 if accumulate else 0, _vp(stream)))

    def run_batch_edges_ptr(self, samples_ptr, count, num_partitions, edges_ptr, bins, out_counts_ptr, key_type="uint32", accumulate=False,
                            stream=None):
        """Every partition of `count` samples over the one device array of bins + 1 edges (glu_histogram_run_batch_edges_ptr)."""
        check(lib().glu_histogram_run_batch_edges_ptr(self._h, _vp(samples_ptr), count, num_partitions, KEY_TYPES[key_type], _vp(edges_ptr), bins,
                                                      _vp(out_counts_ptr), 1 if accumulate else 0, _vp(stream)))

    def run_batch_offsets_edges_ptr(self, samples_ptr, total, offsets_ptr, num_segments, edges_ptr, bins, out_counts_ptr, key_type="uint32",
                                    accumulate=False, stream=None):
        """Every segment of device offsets over the one device array of bins + 1 edges (glu_histogram_run_batch_offsets_edges_ptr)."""
        check(lib().glu_histogram_run_batch_offsets_edges_ptr(self._h, _vp(samples_ptr), total, _vp(offsets_ptr), num_segments,
                                                              KEY_TYPES[key_type], _vp(edges_ptr), bins, _vp(out_counts_ptr),
                                                              1 if accumulate else 0, _vp(stream)))

    def read_batch(self):
        """{wave, block, long}: segments each class of the last batched call took (glu_histogram_read_batch); synchronise first."""
        return _read_batch(lib().glu_histogram_read_batch, self._h)


class Expand(_Handle):
    """glu::Expand (not in the reference) over the C ABI: for every element the segment that holds it, its rank inside the segment
    and the segment's item, from the offsets of the batched family.  The inverse of KeyRuns; numpy.repeat on the device."""

    _CREATE, _DESTROY = "glu_expand_create", "glu_expand_destroy"

    def __init__(self):
        self._create()

    def prepare(self, total, num_segments):
        """Scratch for calls of up to `total` elements and `num_segments` segments: they allocate nothing (capturable)
        (glu_expand_prepare)."""
        check(lib().glu_expand_prepare(self._h, total, num_segments))

    def run_ptr(self, offsets_ptr, num_segments, total, out_segments_ptr=None, out_ranks_ptr=None, items_ptr=None, out_items_ptr=None,
                item_bytes=4, stream=None):
        """With s(j) = numpy.searchsorted(offsets, j, "right") - 1 for j < total, wherever 0 <= s(j) < num_segments:
        out_segments[j] = s(j), out_ranks[j] = j - offsets[s(j)], out_items[j] = items[s(j)] (item_bytes 4, 8, 16 or 32); other
        positions are not touched.  Every output is optional.  All pointers are device pointers (glu_expand_run_ptr)."""
        check(lib().glu_expand_run_ptr(self._h, _vp(offsets_ptr), num_segments, total, _vp(items_ptr), item_bytes, _vp(out_items_ptr),
                                       _vp(out_segments_ptr), _vp(out_ranks_ptr), _vp(stream)))

    def last(self):
        """(tiles, kernels) of what the last run_ptr enqueued (glu_expand_last; no device read)."""
        a, b = _u32(), _u32()
        check(lib().glu_expand_last(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class Gather(_Handle):
    """glu::Gather (not in the reference) over the C ABI: items of 4, 8, 16 or 32 bytes fetched or placed by uint32 indices on the
    device.  No index is trusted: an entry whose index is out of range is skipped and its place in `out` is not touched.  The object
    owns no device memory; every call is allocation-free.  All pointers are device pointers."""

    _CREATE, _DESTROY = "glu_gather_create", "glu_gather_destroy"

    def __init__(self):
        self._create()

    def run_ptr(self, items_ptr, item_count, item_bytes, indices_ptr, count, out_ptr, stream=None):
        """out[j] = items[indices[j]] for j < count wherever indices[j] < item_count (glu_gather_run_ptr)."""
        check(lib().glu_gather_run_ptr(self._h, _vp(items_ptr), item_count, item_bytes, _vp(indices_ptr), count, _vp(out_ptr), _vp(stream)))

    def run_batch_ptr(self, items_ptr, item_bytes, count, num_partitions, indices_ptr, k, out_ptr, stream=None):
        """Rows of stride k of indices local to equal partitions of `count` items, what TopK.run_batch_ptr writes:
        out[s * k + j] = items[s * count + indices[s * k + j]] for j < min(k, count) (glu_gather_run_batch_ptr)."""
        check(lib().glu_gather_run_batch_ptr(self._h, _vp(items_ptr), item_bytes, count, num_partitions, _vp(indices_ptr), k, _vp(out_ptr),
                                             _vp(stream)))

    def run_batch_offsets_ptr(self, items_ptr, item_bytes, total, offsets_ptr, num_segments, indices_ptr, k, out_ptr, stream=None):
        """... local to the segments [offsets[s], offsets[s + 1]) of a device array of num_segments + 1 uint32; the entries
        j >= min(k, length) of a row are not touched (glu_gather_run_batch_offsets_ptr)."""
        check(lib().glu_gather_run_batch_offsets_ptr(self._h, _vp(items_ptr), item_bytes, total, _vp(offsets_ptr), num_segments,
                                                     _vp(indices_ptr), k, _vp(out_ptr), _vp(stream)))

    def scatter_ptr(self, items_ptr, item_bytes, indices_ptr, count, out_ptr, out_count, stream=None):
        """out[indices[j]] = items[j] for j < count wherever indices[j] < out_count; the indices are expected to be distinct
        (glu_gather_scatter_ptr)."""
        check(lib().glu_gather_scatter_ptr(self._h, _vp(items_ptr), item_bytes, _vp(indices_ptr), count, _vp(out_ptr), out_count,
                                           _vp(stream)))

    def last(self):
        """(tiles, kernels) of what the last call enqueued (glu_gather_last; no device read)."""
        a, b = _u32(), _u32()
        check(lib().glu_gather_last(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class TopK(_Handle):
    """glu::TopK (not in the reference) over the C ABI: the k smallest or largest keys and their indices by a radix select, in the
    sort's order (floats by their bits), equal keys by ascending index."""

    _CREATE, _DESTROY = "glu_top_k_create", "glu_top_k_destroy"

    def __init__(self, options=None):
        """options: {"PATH": TopKPath_*, "CAND_CAPACITY": n, "BATCH_LOOP_MIN": n} (glu_top_k_set_option)."""
        self._create()
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def set_option(self, name, value):
        check(lib().glu_top_k_set_option(self._h, str(name).encode(), int(value)))

    def prepare(self, count, max_k, key_type="uint32"):
        """Scratch for calls of up to `count` keys and k up to `max_k` under the options set now: they allocate nothing (capturable)
        (glu_top_k_prepare)."""
        check(lib().glu_top_k_prepare(self._h, count, max_k, KEY_TYPES[key_type]))

    def run_ptr(self, keys_ptr, count, k, out_keys_ptr=None, out_indices_ptr=None, out_kth_ptr=None, key_type="uint32", largest=False,
                sorted=True, stream=None):
        """The k smallest (largest) of `count` keys: out_keys[0 .. k) bit for bit, out_indices[0 .. k) uint32, *out_kth the k-th best
        key; each may be None, not all.  sorted: best first, else ascending indices.  All pointers are device pointers; the keys are
        only read (glu_top_k_run_ptr)."""
        check(lib().glu_top_k_run_ptr(self._h, _vp(keys_ptr), KEY_TYPES[key_type], count, k, 1 if largest else 0, 1 if sorted else 0,
                                      _vp(out_keys_ptr), _vp(out_indices_ptr), _vp(out_kth_ptr), _vp(stream)))

    def read_last(self):
        """{path, candidates, ties, kernels} of the last run_ptr, read back from the device (glu_top_k_read_last); synchronise first."""
        a, b, c, d = _u32(), _u32(), _u32(), _u32()
        check(lib().glu_top_k_read_last(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return {"path": a.value, "candidates": b.value, "ties": c.value, "kernels": d.value}

    def prepare_batch(self, total, num_segments, max_k, key_type="uint32"):
        """Scratch for batched calls of up to `total` keys in up to `num_segments` segments and k up to `max_k` under the options set
        now: they allocate nothing (capturable) (glu_top_k_prepare_batch)."""
        check(lib().glu_top_k_prepare_batch(self._h, total, num_segments, max_k, KEY_TYPES[key_type]))

    def run_batch_ptr(self, keys_ptr, count, num_partitions, k, out_keys_ptr=None, out_indices_ptr=None, out_kth_ptr=None, key_type="uint32",
                      largest=False, sorted=True, stream=None):
        """The k best keys of each of `num_partitions` partitions of `count` keys: rows of stride k of out_keys (bit for bit) and
        out_indices (uint32, local to the partition), out_kth[s] the k-th best of partition s; each may be None, not all
        (glu_top_k_run_batch_ptr)."""
        check(lib().glu_top_k_run_batch_ptr(self._h, _vp(keys_ptr), KEY_TYPES[key_type], count, num_partitions, k, 1 if largest else 0,
                                            1 if sorted else 0, _vp(out_keys_ptr), _vp(out_indices_ptr), _vp(out_kth_ptr), _vp(stream)))

    def run_batch_offsets_ptr(self, keys_ptr, total, offsets_ptr, num_segments, k, out_keys_ptr=None, out_indices_ptr=None, out_kth_ptr=None,
                              key_type="uint32", largest=False, sorted=True, stream=None):
        """... of the segments [offsets[s], offsets[s + 1]) of a device array of num_segments + 1 uint32, k_s = min(k, length) per
        segment; the entries j >= k_s of a row and the out_kth of an empty segment are not touched
        (glu_top_k_run_batch_offsets_ptr)."""
        check(lib().glu_top_k_run_batch_offsets_ptr(self._h, _vp(keys_ptr), KEY_TYPES[key_type], total, _vp(offsets_ptr), num_segments, k,
                                                    1 if largest else 0, 1 if sorted else 0, _vp(out_keys_ptr), _vp(out_indices_ptr),
                                                    _vp(out_kth_ptr), _vp(stream)))

    def read_batch(self):
        """{wave, block, long, kernels} of the last batched call: its segments per class and the kernels it enqueued
        (glu_top_k_read_batch); synchronise first."""
        a, b, c, d = _u32(0), _u32(0), _u32(0), _u32(0)
        check(lib().glu_top_k_read_batch(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return {"wave": a.value, "block": b.value, "long": c.value, "kernels": d.value}


def _check_composed_runs(max_runs):
    if max_runs > KeyRuns.MAX_COMPOSED_RUNS:
        raise GluError(GLU_ERROR_INVALID_ARGUMENT, "max_runs %d exceeds 2^24" % max_runs)


class BlellochScan(_Handle):
    """glu::BlellochScan (reference glu/BlellochScan.hpp:80-191) over the C ABI."""

    _CREATE, _DESTROY = "glu_scan_create", "glu_scan_destroy"

    def __init__(self, data_type):
        self._create(data_type)

    def __call__(self, buffer, count, num_partitions=1):
        b = buffer.handle() if isinstance(buffer, ShaderStorageBuffer) else buffer
        check(lib().glu_scan_run(self._h, b, count, num_partitions))

    def prepare(self, count, num_partitions=1):
        """Scratch for scans of `count` x `num_partitions` elements: after it a scan allocates nothing (capturable)."""
        check(lib().glu_scan_prepare(self._h, count, num_partitions))

    def run_ptr(self, data_ptr, count, num_partitions=1, stream=None):
        check(lib().glu_scan_run_ptr(self._h, _vp(data_ptr), count, num_partitions, _vp(stream)))

    OPS = {"sum": 0, "mul": 1, "min": 2, "max": 3}  # glu_reduce_operator

    def run_batch_offsets_ptr(self, data_ptr, total, offsets_ptr, num_segments, stream=None, out_ptr=None, op="sum", inclusive=False):
        """Elements [offsets[s], offsets[s+1]) become their own exclusive scan, in place, for every segment (offsets: num_segments
        + 1 uint32 on the DEVICE) (glu_scan_run_batch_offsets_ptr).  With `out_ptr`, an `op` ("sum", "mul", "min", "max" or a
        glu_reduce_operator) or `inclusive`: that scan, stored to `out_ptr` where one is given, `data_ptr` then only read
        (glu_scan_run_batch_offsets_op_ptr)."""
        if out_ptr is None and op in ("sum", 0) and not inclusive:
            check(lib().glu_scan_run_batch_offsets_ptr(self._h, _vp(data_ptr), total, _vp(offsets_ptr), num_segments, _vp(stream)))
            return
        check(lib().glu_scan_run_batch_offsets_op_ptr(self._h, _vp(data_ptr), _vp(out_ptr), total, _vp(offsets_ptr), num_segments,
                                                      self.OPS.get(op, op), int(bool(inclusive)), _vp(stream)))

    def run_whole_ptr(self, data_ptr, total, stream=None, out_ptr=None, op="sum", inclusive=False):
        """The scan of the whole array [0, total) as one segment, no offsets array needed: cumsum, cumprod, cummin, cummax
        (glu_scan_run_batch_offsets_op_ptr with offsets == NULL)."""
        check(lib().glu_scan_run_batch_offsets_op_ptr(self._h, _vp(data_ptr), _vp(out_ptr), total, None, 1, self.OPS.get(op, op),
                                                      int(bool(inclusive)), _vp(stream)))

    def run_by_key_ptr(self, runs, keys_ptr, values_ptr, count, offsets_ptr, max_runs, num_runs_ptr, unique_keys_ptr=None,
                       key_bits=32, begin_bit=0, end_bit=None, stream=None, out_ptr=None, op="sum", inclusive=False):
        """Scan by key: runs.run_ptr on the keys, then the values of every run become their own exclusive scan, in place -- the
        two calls on one stream (glu::BlellochScan::scan_by_key).  max_runs <= 2^24.  out_ptr, op, inclusive: as in
        run_batch_offsets_ptr."""
        _check_composed_runs(max_runs)
        runs.run_ptr(keys_ptr, count, offsets_ptr, max_runs, num_runs_ptr, unique_keys_ptr, key_bits, begin_bit, end_bit, stream)
        self.run_batch_offsets_ptr(values_ptr, count, offsets_ptr, max_runs, stream, out_ptr=out_ptr, op=op, inclusive=inclusive)

    def prepare_batch(self, total, num_segments):
        """Grow-only scratch for batched scans of up to `total` elements in up to `num_segments` segments: after it the call
        above allocates nothing (glu_scan_prepare_batch)."""
        check(lib().glu_scan_prepare_batch(self._h, total, num_segments))

    def read_batch(self):
        """{wave, block, long}: segments each path of the last batched call took (glu_scan_read_batch); synchronise first."""
        return _read_batch(lib().glu_scan_read_batch, self._h)


class Reduce(_Handle):
    """glu::Reduce (reference glu/Reduce.hpp:51-136) over the C ABI."""

    _CREATE, _DESTROY = "glu_reduce_create", "glu_reduce_destroy"

    def __init__(self, data_type, operator_):
        self._create(data_type, operator_)

    def __call__(self, buffer, count):
        b = buffer.handle() if isinstance(buffer, ShaderStorageBuffer) else buffer
        check(lib().glu_reduce_run(self._h, b, count))

    def run_ptr(self, data_ptr, count, stream=None):
        check(lib().glu_reduce_run_ptr(self._h, _vp(data_ptr), count, _vp(stream)))

    def run_batch_ptr(self, data_ptr, out_ptr, count, num_partitions, stream=None):
        """out[p] = the reduction of partition p of `num_partitions` adjacent partitions of `count` elements; data is only read
        (glu_reduce_run_batch_ptr)."""
        check(lib().glu_reduce_run_batch_ptr(self._h, _vp(data_ptr), _vp(out_ptr), count, num_partitions, _vp(stream)))

    def run_batch_offsets_ptr(self, data_ptr, out_ptr, total, offsets_ptr, num_segments, stream=None):
        """out[s] = the reduction of elements [offsets[s], offsets[s+1]) (offsets: num_segments + 1 uint32 on the DEVICE); data is
        only read (glu_reduce_run_batch_offsets_ptr)."""
        check(lib().glu_reduce_run_batch_offsets_ptr(self._h, _vp(data_ptr), _vp(out_ptr), total, _vp(offsets_ptr), num_segments,
                                                     _vp(stream)))

    def run_by_key_ptr(self, runs, keys_ptr, values_ptr, out_ptr, count, offsets_ptr, max_runs, num_runs_ptr, unique_keys_ptr=None,
                       key_bits=32, begin_bit=0, end_bit=None, stream=None):
        """Reduce by key: runs.run_ptr on the keys, then out[r] = the reduction of the values of run r for r < max_runs (the
        identity from the number of runs on) -- the two calls on one stream (glu::Reduce::reduce_by_key).  max_runs <= 2^24."""
        _check_composed_runs(max_runs)
        runs.run_ptr(keys_ptr, count, offsets_ptr, max_runs, num_runs_ptr, unique_keys_ptr, key_bits, begin_bit, end_bit, stream)
        self.run_batch_offsets_ptr(values_ptr, out_ptr, count, offsets_ptr, max_runs, stream)

    def prepare_batch(self, total, num_segments):
        """Grow-only scratch for batched reduces of up to `total` elements in up to `num_segments` segments: after it the two
        calls above allocate nothing (glu_reduce_prepare_batch)."""
        check(lib().glu_reduce_prepare_batch(self._h, total, num_segments))

    def read_batch(self):
        """{wave, block, long}: segments each path of the last batched call took (glu_reduce_read_batch); synchronise first."""
        return _read_batch(lib().glu_reduce_read_batch, self._h)


def measure_elapsed_time(callback):
    """glu::measure_gl_elapsed_time (reference glu/gl_utils.hpp:249-265): nanoseconds of device time."""
    t = _vp()
    check(lib().glu_timer_begin(ctypes.byref(t)))
    callback()
    ns = _u64(0)
    check(lib().glu_timer_end(t, ctypes.byref(ns)))
    return ns.value


DIST_UNIQUE_ID_BYTES = 128
DIST_BUCKETS = 256


def plan_segments(piece_begin, piece_len, piece_segment, num_segments, num_workgroups):
    """glu_radix_sort_plan_segments (host only): -> (sub_blocks [n][2], workgroup_first, segment_first, segment_start)."""
    pb = np.ascontiguousarray(piece_begin, dtype=np.uint64)
    pl = np.ascontiguousarray(piece_len, dtype=np.uint64)
    ps = np.ascontiguousarray(piece_segment, dtype=np.uint32)
    cap = pb.shape[0] + num_workgroups
    subs = np.zeros((cap, 2), dtype=np.uint32)
    wg = np.zeros(num_workgroups + 1, dtype=np.uint32)
    sf = np.zeros(num_segments + 1, dtype=np.uint32)
    ss = np.zeros(num_segments + 1, dtype=np.uint64)
    n = _sz(0)
    check(lib().glu_radix_sort_plan_segments(pb.ctypes.data_as(_P(_u64)), pl.ctypes.data_as(_P(_u64)), ps.ctypes.data_as(_P(_u32)),
                                             pb.shape[0], num_segments, num_workgroups, subs.ctypes.data_as(_P(_u32)), cap,
                                             wg.ctypes.data_as(_P(_u32)), sf.ctypes.data_as(_P(_u32)), ss.ctypes.data_as(_P(_u64)),
                                             ctypes.byref(n)))
    return subs[:n.value], wg, sf, ss


def dist_available():
    """glu_dist_available: raises GluError unless this process can load RCCL with the entry points glu_dist_* needs."""
    check(lib().glu_dist_available())


def dist_unique_id():
    """Rank 0: the RCCL unique id (bytes) to hand to every rank's Dist(...)."""
    buf = ctypes.create_string_buffer(DIST_UNIQUE_ID_BYTES)
    check(lib().glu_dist_unique_id(buf, DIST_UNIQUE_ID_BYTES))
    return buf.raw


def dist_plan(all_hist, world_size, rank):
    """The C ABI's plan (host only): (bucket_owner[256], send_counts[world], recv_counts[world]) as Python lists."""
    flat = [int(x) for row in all_hist for x in row]
    assert len(flat) == world_size * DIST_BUCKETS
    h = (_u32 * len(flat))(*flat)
    owner = (_int * DIST_BUCKETS)()
    check(lib().glu_dist_plan_buckets(h, world_size, owner))
    send, recv = (_u64 * world_size)(), (_u64 * world_size)()
    check(lib().glu_dist_plan_counts(h, world_size, rank, owner, send, recv))
    return list(owner), list(send), list(recv)


def dist_plan_groups(all_hist, world_size, owner, rounds):
    """glu_dist_plan_groups (host only): [world][rounds + 1] bucket boundaries of every rank's groups."""
    flat = [int(x) for row in all_hist for x in row]
    h = (_u32 * len(flat))(*flat)
    own = (_int * DIST_BUCKETS)(*[int(x) for x in owner])
    cut = (_int * (world_size * (rounds + 1)))()
    check(lib().glu_dist_plan_groups(h, world_size, own, rounds, cut))
    return [list(cut[q * (rounds + 1):(q + 1) * (rounds + 1)]) for q in range(world_size)]


class Dist(_Handle):
    """glu_dist over the C ABI: the sharded sort of one rank (RCCL communicator + local sorter inside the library)."""

    _CREATE, _DESTROY = "glu_dist_create", "glu_dist_destroy"

    def __init__(self, unique_id, world_size, rank):
        self._create(unique_id, len(unique_id), world_size, rank)
        self.world_size, self.rank = world_size, rank

    def prepare(self, local_count, recv_capacity=0):
        check(lib().glu_dist_prepare(self._h, local_count, recv_capacity))

    @property
    def sorter(self):
        """The local RadixSort inside the object (borrowed: profiling / digit width, never destroyed from here)."""
        h = _vp()
        check(lib().glu_dist_local_sorter(self._h, ctypes.byref(h)))
        s = RadixSort.__new__(RadixSort)
        s._h = h
        s._borrowed = True
        return s

    def sort_begin(self, keys_ptr, vals_ptr, local_count, stream=None):
        n = _sz(0)
        check(lib().glu_dist_sort_begin(self._h, _vp(keys_ptr), _vp(vals_ptr), local_count, _vp(stream), ctypes.byref(n)))
        return n.value

    def sort_finish(self, recv_keys_ptr, recv_vals_ptr, capacity, stream=None):
        check(lib().glu_dist_sort_finish(self._h, _vp(recv_keys_ptr), _vp(recv_vals_ptr), capacity, _vp(stream)))

    def sort_ptr(self, keys_ptr, vals_ptr, local_count, stream=None):
        """-> (device pointer of the shard's keys, of its values, count); the arrays belong to the object."""
        k, v, n = _vp(), _vp(), _sz(0)
        check(lib().glu_dist_sort_ptr(self._h, _vp(keys_ptr), _vp(vals_ptr), local_count, _vp(stream), ctypes.byref(k),
                                      ctypes.byref(v), ctypes.byref(n)))
        return k.value or 0, v.value or 0, n.value

    def partition_shift(self):
        sh = _u32(0)
        check(lib().glu_dist_partition_shift(self._h, ctypes.byref(sh)))
        return sh.value

    def last_local_sort(self):
        """'segmented' (three passes over the low 24 bits per bucket) or 'ordinary' (all 32 bits): the last sort's local sort."""
        v = _u32(0)
        check(lib().glu_dist_last_local_sort(self._h, ctypes.byref(v)))
        return "segmented" if v.value else "ordinary"

    def set_rounds(self, rounds):
        """Rounds of the exchange (glu_dist_set_rounds; the same value on every rank)."""
        check(lib().glu_dist_set_rounds(self._h, int(rounds)))

    def last_rounds(self):
        """In how many rounds the last sort's exchange was posted (glu_dist_last_rounds)."""
        v = _u32(0)
        check(lib().glu_dist_last_rounds(self._h, ctypes.byref(v)))
        return int(v.value)

    def set_reserved_cus(self, cus):
        check(lib().glu_dist_set_reserved_cus(self._h, cus))

    def set_profiling(self, enable):
        check(lib().glu_dist_set_profiling(self._h, 1 if enable else 0))

    def phase_times(self):
        ms = (ctypes.c_double * 4)()
        n = _u64(0)
        check(lib().glu_dist_phase_times(self._h, ms, ctypes.byref(n)))
        names = ("partition", "histogram_exchange_and_plan", "all_to_all", "local_sort")
        return {"sorts": int(n.value), **{k: float(ms[i]) for i, k in enumerate(names)}}
