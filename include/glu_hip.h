/*
 * glu_hip.h -- C ABI of libglu_hip.so: MI355X (gfx950) radix sort / exclusive scan / reduce.
 *
 * This is the drop-in boundary for the hot path of loryruta/gl-radix-sort (reference @ v2).  The reference
 * has no FFI layer: its operators are header-only C++ classes (namespace glu) that record OpenGL compute
 * dispatches against GLuint buffer names.  The functions below are what those classes need from the device
 * side; the C++17 headers in gl-radix-sort_amd/glu/ re-create the reference's classes on top of them, and any
 * other host language binds the same symbols (INTEGRATION.md shows the bindings).
 *
 * Conventions
 *   - every function returns glu_status (0 = GLU_OK); nothing here prints or calls exit() -- the
 *     print-and-exit(1) convention of glu/errors.hpp:8-18 lives in the C++ headers above this ABI;
 *   - glu_last_error() returns a thread-local message for the last non-zero status;
 *   - buffers are named by 32-bit handles exactly like GLuint buffer names: 0 is "no buffer"
 *     (checked the way glu/RadixSort.hpp:275-276 checks it);
 *   - all handle-based calls enqueue on one in-order queue per process (a HIP stream owned by the
 *     library, the analogue of the thread's GL command queue) and return without waiting for the GPU,
 *     like the reference's operator() (glu/RadixSort.hpp:273-334 never blocks).  glu_buffer_read() and
 *     glu_device_synchronize() wait.  *_ptr entry points take raw device pointers plus a caller stream
 *     (a hipStream_t passed as void*; NULL = the library queue -- to target HIP's null stream pass the
 *     hipStreamLegacy / hipStreamPerThread handle, not 0);
 *   - no function allocates device memory inside a sort/scan/reduce call once the matching
 *     *_prepare() has been called with a count at least as large (glu/RadixSort.hpp:237-271:
 *     grow-only scratch).
 *   - not thread-safe per handle; distinct handles may be used from distinct host threads (every entry point makes the
 *     library's device the calling thread's current HIP device; per-kernel one-time setup is guarded).  The
 *     *_ptr entry points accept NULL arrays when count == 0 (an empty shard).
 */
#ifndef GLU_HIP_H
#define GLU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(GLU_HIP_BUILD)
#define GLU_API __attribute__((visibility("default")))
#else
#define GLU_API
#endif

typedef int glu_status;
enum
{
    GLU_OK = 0,
    GLU_ERROR_INVALID_ARGUMENT = 1, /* what GLU_CHECK_ARGUMENT rejects in the reference */
    GLU_ERROR_INVALID_STATE = 2,    /* what GLU_CHECK_STATE rejects */
    GLU_ERROR_OUT_OF_MEMORY = 3,
    GLU_ERROR_DEVICE = 4,           /* a HIP runtime call failed; message has the hipError string */
    GLU_ERROR_NO_DEVICE = 5         /* no gfx950 GPU visible: there is NO CPU fallback */
};

/* glu/data_types.hpp:8-22 -- same numeric values */
typedef enum glu_data_type
{
    GLU_DATA_TYPE_FLOAT = 0,
    GLU_DATA_TYPE_DOUBLE,
    GLU_DATA_TYPE_INT,
    GLU_DATA_TYPE_UINT,
    GLU_DATA_TYPE_VEC2,
    GLU_DATA_TYPE_VEC4,
    GLU_DATA_TYPE_DVEC2,
    GLU_DATA_TYPE_DVEC4,
    GLU_DATA_TYPE_UVEC2,
    GLU_DATA_TYPE_UVEC4,
    GLU_DATA_TYPE_IVEC2,
    GLU_DATA_TYPE_IVEC4,
    GLU_DATA_TYPE_COUNT_
} glu_data_type;

/* glu/Reduce.hpp:42-48 -- same numeric values */
typedef enum glu_reduce_operator
{
    GLU_REDUCE_SUM = 0,
    GLU_REDUCE_MUL,
    GLU_REDUCE_MIN,
    GLU_REDUCE_MAX,
    GLU_REDUCE_COUNT_
} glu_reduce_operator;

typedef unsigned int glu_buffer; /* replaces GLuint buffer names (glu/gl_utils.hpp:149) */
typedef struct glu_radix_sort_s* glu_radix_sort;
typedef struct glu_scan_s* glu_scan;
typedef struct glu_reduce_s* glu_reduce;
typedef struct glu_key_runs_s* glu_key_runs;
typedef struct glu_select_s* glu_select;
typedef struct glu_timer_s* glu_timer;
typedef struct glu_dist_s* glu_dist;

/* ---- library / device ---------------------------------------------------------------------------- */

/* Thread-local text for the last failing call on this thread ("" if none). */
GLU_API const char* glu_last_error(void);
/* "glu_hip <version> gfx950" */
GLU_API const char* glu_version(void);
/* Number of visible HIP devices (0 is not an error here). */
GLU_API glu_status glu_device_count(int* count);
/* Select the device the library queue lives on (default: the current HIP device, normally 0).  Must be
 * called before the first buffer / operator is created; one device per process (one process per GPU). */
GLU_API glu_status glu_set_device(int device);
/* Human readable device line: name, gcnArchName, CU count, memory. */
GLU_API glu_status glu_device_info(char* out, size_t out_size);
/* Block until everything enqueued on the library queue has finished (the glFinish analogue). */
GLU_API glu_status glu_device_synchronize(void);
/* The library queue as a hipStream_t (void*), for callers that want to enqueue their own work in order. */
GLU_API glu_status glu_queue(void** stream);

/* Host only, no device.  A test switch: with GLU_HIP_SCRATCH_FILL set to an integer 0 .. 255 (read whenever an operator object's
 * scratch grows, never inside a call that does not grow), every new scratch allocation is filled with that byte before the call
 * goes on, so that a test can hold the results apart from what fresh device memory happens to contain.  Any other value is an
 * invalid-argument error of the call that grows.  *bytes: the bytes filled so far by this process (0 while the variable was never
 * set), by which such a test shows that it did fill something. */
GLU_API glu_status glu_scratch_filled_bytes(size_t* bytes);

/* ---- buffers: replaces glu::ShaderStorageBuffer's GL calls (glu/gl_utils.hpp:146-246) ------------- */

/* glCreateBuffers + glBufferStorage(size, NULL)      (gl_utils.hpp:203-205).  size may be 0. */
GLU_API glu_status glu_buffer_create(size_t size, glu_buffer* out);
/* glBufferStorage(size, data)                          (gl_utils.hpp:165-167) */
GLU_API glu_status glu_buffer_create_with_data(const void* data, size_t size, glu_buffer* out);
/* Name an existing device allocation (e.g. a torch tensor's data_ptr()); not owned, never freed. */
GLU_API glu_status glu_buffer_wrap(void* device_ptr, size_t size, glu_buffer* out);
/* glDeleteBuffers                                      (gl_utils.hpp:186-187).  0 is ignored. */
GLU_API glu_status glu_buffer_destroy(glu_buffer buffer);
GLU_API glu_status glu_buffer_size(glu_buffer buffer, size_t* size);
GLU_API glu_status glu_buffer_device_ptr(glu_buffer buffer, void** device_ptr);
/* glBufferSubData(offset, size, data)                  (gl_utils.hpp:221-227) */
GLU_API glu_status glu_buffer_write(glu_buffer buffer, const void* data, size_t size, size_t offset);
/* glGetBufferSubData(offset, size, data); waits        (gl_utils.hpp:229-238) */
GLU_API glu_status glu_buffer_read(glu_buffer buffer, void* data, size_t size, size_t offset);
/* glClearBufferData(GL_R32UI, value): whole buffer     (gl_utils.hpp:215-219) */
GLU_API glu_status glu_buffer_fill_u32(glu_buffer buffer, uint32_t value);
/* glCopyBufferSubData                                  (gl_utils.hpp:13-22) */
GLU_API glu_status glu_buffer_copy(glu_buffer src, glu_buffer dst, size_t size, size_t src_offset, size_t dst_offset);

/* ---- radix sort: replaces glu::RadixSort (glu/RadixSort.hpp:186-354) ------------------------------ */

/* RadixSort::RadixSort()                               (RadixSort.hpp:205-233) */
GLU_API glu_status glu_radix_sort_create(glu_radix_sort* out);
GLU_API glu_status glu_radix_sort_destroy(glu_radix_sort sort);
/* RadixSort::prepare_internal_buffers(count)           (RadixSort.hpp:237-271): grow-only scratch for
 * `count` pairs with 32-bit keys.
 * Cost: for less than 512 MiB of keys, the allocations.  From there on (2^27 32-bit keys) prepare also PLACES the key and
 * value scratch by measurement (glu_radix_sort_scratch_placement below): 0.13-1 s of host time, usually 0.3 s, up to 48
 * calibration sorts on the library queue behind a hipDeviceSynchronize, and transiently about 2 x (4 arrays of the prepared
 * size + 7.5 GiB of spacers) of device memory.  When hipMemGetInfo reports less free memory than that the search is skipped
 * (GLU_VERBOSE says so) and the arrays are two plain hipMallocs: everything works, large sorts run 5-8 % slower on some
 * placements.  Only the glu_radix_sort_prepare* / glu_dist_prepare calls do this: a sort on an object that was not prepared
 * for its size grows the scratch with plain allocations (hipFree + hipMalloc: a device-wide synchronisation, not
 * capturable) and never measures. */
GLU_API glu_status glu_radix_sort_prepare(glu_radix_sort sort, size_t count);
/* Same for 64-bit keys (BASELINE.json config 5). */
GLU_API glu_status glu_radix_sort_prepare_u64(glu_radix_sort sort, size_t count);
/* The general form (RadixSort.hpp:237-271 knows one key type only): scratch for `count` elements of `key_bytes`-byte
 * keys (4 or 8), with or without a value array.  After it, the matching run entry point (run / run_u64 / run_keys* /
 * run_typed / run_bit_range with that key width) allocates nothing for counts up to `count`.  A run of a wider key type
 * than prepared for still works but grows the scratch inside the call (hipFree + hipMalloc: a device-wide
 * synchronisation, and not capturable into a graph). */
GLU_API glu_status glu_radix_sort_prepare_ex(glu_radix_sort sort, size_t count, size_t key_bytes, int with_vals);
/* RadixSort::operator()(key_buffer, val_buffer, count, num_steps)   (RadixSort.hpp:273-334).
 * Stable ascending sort of `count` (uint32 key, uint32 val) pairs by the low 4*num_steps key bits
 * (num_steps == 0 or > 8: all 32 bits).  count <= 1 returns immediately (:278).  count must be < 2^32.
 * Deliberate deviation: the result is always left in key_buffer / val_buffer; the
 * reference leaves it in its private scratch buffers when num_steps is odd.
 * Every sort entry point below behaves the same way: the call only enqueues work (no host synchronisation, no allocation
 * once prepared: it can be captured into a HIP graph); up to 16384 pairs it is one kernel launch; from 2^22 elements up a
 * counting pass whose digit is the same in every key is skipped on the device (same result, less work). */
GLU_API glu_status glu_radix_sort_run(glu_radix_sort sort, glu_buffer key_buffer, glu_buffer val_buffer, size_t count,
                                      size_t num_steps);
/* Raw-pointer form of the same call; `stream` is a hipStream_t or NULL. */
GLU_API glu_status glu_radix_sort_run_ptr(glu_radix_sort sort, uint32_t* keys, uint32_t* vals, size_t count,
                                          size_t num_steps, void* stream);
/* 64-bit keys + 32-bit payload, num_steps 4-bit digits (0 or > 16: all 64 bits). */
GLU_API glu_status glu_radix_sort_run_u64(glu_radix_sort sort, glu_buffer key_buffer, glu_buffer val_buffer,
                                          size_t count, size_t num_steps);
GLU_API glu_status glu_radix_sort_run_u64_ptr(glu_radix_sort sort, uint64_t* keys, uint32_t* vals, size_t count,
                                              size_t num_steps, void* stream);
/* Keys-only sorts (not in the reference, whose value buffer is mandatory -- README.md:88-89 tells users to allocate a
 * dummy one): same ordering of the keys, no value traffic (12 instead of 20 bytes per key and pass). */
GLU_API glu_status glu_radix_sort_run_keys(glu_radix_sort sort, glu_buffer key_buffer, size_t count, size_t num_steps);
GLU_API glu_status glu_radix_sort_run_keys_ptr(glu_radix_sort sort, uint32_t* keys, size_t count, size_t num_steps,
                                               void* stream);
GLU_API glu_status glu_radix_sort_run_keys_u64_ptr(glu_radix_sort sort, uint64_t* keys, size_t count, size_t num_steps,
                                                   void* stream);
/* Typed keys (not in the reference: uint32 only).  Signed integers and IEEE floats are sorted in their natural order
 * (floats as a total order: -0 < +0, NaNs beyond the infinities of their sign) by encoding the key on the first pass's
 * loads and decoding on the last pass's stores -- no extra pass over memory.  vals may be NULL (keys only). */
typedef enum glu_key_type
{
    GLU_KEY_UINT32 = 0,
    GLU_KEY_INT32,
    GLU_KEY_FLOAT32,
    GLU_KEY_UINT64,
    GLU_KEY_INT64,
    GLU_KEY_FLOAT64
} glu_key_type;
GLU_API glu_status glu_radix_sort_run_typed_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t count,
                                                glu_key_type key_type, void* stream);
/* Stable sort by the key bits [begin_bit, end_bit) only (not in the reference, whose num_steps always starts at bit 0,
 * RadixSort.hpp:303,331-332): keys that are known to fit 24 bits sort in 3 passes instead of 4, a sort by the high bits
 * alone leaves the low-bit order untouched.  key_bits is 32 or 64 (unsigned keys), vals may be NULL (keys only), the
 * result is in the caller's arrays for every pass count; begin_bit == end_bit is a no-op. */
GLU_API glu_status glu_radix_sort_run_bit_range_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t count,
                                                    uint32_t key_bits, uint32_t begin_bit, uint32_t end_bit, void* stream);
/* One stable counting pass on the digit (key >> shift) & ((1 << bits) - 1), 1 <= bits <= 8, from src to dst
 * (distinct buffers).  This is the partition step of the multi-GPU sort (top-8-bit buckets).  If
 * digit_histogram != NULL it receives the 1 << bits digit totals (device memory, uint32). */
GLU_API glu_status glu_radix_sort_partition_ptr(glu_radix_sort sort, const uint32_t* src_keys, const uint32_t* src_vals,
                                                uint32_t* dst_keys, uint32_t* dst_vals, size_t count, uint32_t shift,
                                                uint32_t bits, uint32_t* digit_histogram, void* stream);
/* Segmented stable sort (not in the reference; it is the local sort of the sharded sort below, where a rank's shard
 * arrives as one message per source rank, each grouped by top-byte bucket): the input arrays hold `num_pieces` pieces,
 * piece i = elements [piece_begin[i], piece_begin[i] + piece_len[i]) of in_keys / in_vals, together exactly `count`
 * elements and no element twice (the pieces tile [0, count): GLU_ERROR_INVALID_ARGUMENT otherwise); piece i belongs to
 * segment piece_segment[i] < num_segments <= 2^24.  Segment g = its pieces laid end to end in the
 * order they are listed.  The output arrays receive the segments in ascending order of g, each stably sorted by the low
 * `key_bits` key bits (0, 8, 16, 24 or 32; 0 = only the regrouping).  Each pass is the reference's stable counting pass
 * (RadixSort.hpp:142-182) applied per segment, all segments in one launch sequence of the sort's own kernels; the first
 * pass reads the pieces where they lie, so the regrouping costs no pass of its own.  in != out; the input arrays are used
 * as scratch (their contents are lost).  Enqueues on `stream` (the piece arrays are read before the call returns); after
 * glu_radix_sort_prepare(sort, count) it allocates nothing on the device.  Not capturable into a graph (the sub-block
 * descriptors of a call are staged through pinned buffers that later calls reuse): GLU_ERROR_INVALID_STATE under capture. */
GLU_API glu_status glu_radix_sort_run_segments_ptr(glu_radix_sort sort, uint32_t* in_keys, uint32_t* in_vals,
                                                   uint32_t* out_keys, uint32_t* out_vals, size_t count,
                                                   const uint64_t* piece_begin, const uint64_t* piece_len,
                                                   const uint32_t* piece_segment, size_t num_pieces, uint32_t num_segments,
                                                   uint32_t key_bits, void* stream);
/* The host half of glu_radix_sort_run_segments_ptr as a pure function (no device needed: unit-testable): how a segmented pass
 * over these pieces is cut into sub-blocks for `num_workgroups` workgroups.  A sub-block is the part of one piece that falls
 * into one workgroup's equal share of the elements; sub-blocks are numbered segment-major, in the order of each segment's
 * elements.  sub_blocks: [*num_sub_blocks][2] = (begin, end) element range in the input arrays (room for sub_block_capacity
 * pairs; at most num_pieces + num_workgroups are needed); workgroup_first: [num_workgroups + 1], workgroup w runs the
 * sub-blocks [workgroup_first[w], workgroup_first[w + 1]); segment_first: [num_segments + 1] first sub-block of every
 * segment; segment_start: [num_segments + 1] where every segment starts in the output.  Any output array may be NULL. */
GLU_API glu_status glu_radix_sort_plan_segments(const uint64_t* piece_begin, const uint64_t* piece_len,
                                                const uint32_t* piece_segment, size_t num_pieces, uint32_t num_segments,
                                                uint32_t num_workgroups, uint32_t* sub_blocks, size_t sub_block_capacity,
                                                uint32_t* workgroup_first, uint32_t* segment_first, uint64_t* segment_start,
                                                size_t* num_sub_blocks);
/* Digit width (bits per counting pass) the sort uses internally: 4 (the reference's pass structure: 8 passes
 * for 32-bit keys) or 8 (4 passes).  The sorted result is identical; see DESIGN.md. */
GLU_API glu_status glu_radix_sort_set_digit_bits(glu_radix_sort sort, uint32_t bits);
GLU_API glu_status glu_radix_sort_get_digit_bits(glu_radix_sort sort, uint32_t* bits);
/* Switches of a sort object for tests, tuning and A/B runs (nothing the reference has: its only knob is num_steps,
 * RadixSort.hpp:273): `name` is one of the options listed in gl-radix-sort_amd/csrc/glu_hip.hip (kSortOptions: SORT_LDS_FINISH,
 * SORT_FINISH_MIN, SORT_PAIR_MIN, SORT_FORK, SORT_NO_LINES, ...), case-insensitive, with or without the prefix GLU_HIP_.  Takes effect from the
 * object's next prepare / sort.  The process environment (GLU_HIP_<NAME>=value) supplies DEFAULTS, read when an object is
 * created; a program never needs to touch it.  GLU_ERROR_INVALID_ARGUMENT for an unknown name. */
GLU_API glu_status glu_radix_sort_set_option(glu_radix_sort sort, const char* name, long long value);
/* Where the two large scratch arrays lie to each other decides between discrete speeds of every pass on this memory system,
 * so glu_radix_sort_prepare* places key + value scratch of 512 MiB of keys or more BY MEASUREMENT: the value array is
 * allocated behind spacers of 0, 0.5 .. 7.5 GiB (8 to 16 candidates; the search ends when one of them is 7 % faster
 * than the slowest seen, or after a second), each candidate sorts pseudo-random pairs of the prepared count
 * three times on the library queue, the fastest pair of arrays is kept, everything else is freed again (0.13-1 s, usually 0.3 s, once,
 * inside an explicit prepare call only -- no sort, no glu_dist_sort_* call measures or makes transient allocations;
 * GLU_HIP_SCRATCH_TUNE=0 takes the first allocation as the reference's prepare_internal_buffers does,
 * RadixSort.hpp:237-271).  This reports what the last such measurement saw: the number of candidates (0 = none was made:
 * switched off, too little free memory, arrays below 512 MiB, or the scratch was grown by a sort and not by prepare), the
 * calibration sort time of the chosen and of the slowest one. */
GLU_API glu_status glu_radix_sort_scratch_placement(glu_radix_sort sort, uint32_t* candidates, double* chosen_ms, double* slowest_ms);
/* Bytes of scratch currently owned by the sort object (keys + vals + tables). */
GLU_API glu_status glu_radix_sort_scratch_size(glu_radix_sort sort, size_t* bytes);
/* Per-kernel device timing (the measure_gl_elapsed_time idea, glu/gl_utils.hpp:249-265, at kernel granularity):
 * while enabled, every counting pass records HIP events on its stream around the count, scan and scatter
 * kernels.  glu_radix_sort_read_profile waits for the recorded work, returns the summed device milliseconds
 * per kernel class and the number of passes since the previous read, and resets the accumulation. */
/* enable = 2 ("light"): only the two events around the kernel that moves the data of a pass that is expected to run are
 * recorded (the scatter kernel of a counting pass, the in-LDS pass); count_ms / scan_ms then read 0.  An event between two
 * kernels costs the queue a few microseconds: the 28 of a large sort that ends in LDS were 4 % of its time. */
GLU_API glu_status glu_radix_sort_set_profiling(glu_radix_sort sort, int enable);
GLU_API glu_status glu_radix_sort_read_profile(glu_radix_sort sort, double* count_ms, double* scan_ms,
                                               double* scatter_ms, uint64_t* passes);
/* The same with the in-LDS pass of sorts that ended in LDS (glu_radix_sort_read_finish below): finish_ms = its summed
 * device milliseconds, finish_passes = how many ran.  Such a sort enqueues two sequences of passes of which one returns at
 * once; both calls book the passes that did the work (which sequence that was is read from the last sort and assumed for
 * every sort since the previous read): the two top-bit passes when the sort ended in LDS, else the ordinary passes plus the
 * count kernel the refused attempt cost. */
GLU_API glu_status glu_radix_sort_read_profile_finish(glu_radix_sort sort, double* count_ms, double* scan_ms,
                                                      double* scatter_ms, uint64_t* passes, double* finish_ms,
                                                      uint64_t* finish_passes);
/* Diagnostics of the last sort of >= 2^22 elements on this object, whose passes are planned on the device (the caller has
 * synchronised the sort's stream): for pass p < passes, skipped[p] != 0 if the pass was an identity (every key had the same
 * digit value: its scatter did not run) -- 1 if its count kernel found that out, 2 if it was known before counting (the
 * first pass of a sort of unsigned keys notes which key bits vary at all; a later pass on bits that do not vary reads
 * nothing); pair_role[p] = 1 / 2 if the pass was the first / second of a pair of passes that
 * share one read of the keys (large sorts with 8-bit digits: the first pass's count kernel also builds a two-digit
 * histogram, the second pass takes its count table from it), 0 if it stood alone; counted_alone[p] = 1 if a second pass
 * of a pair counted for itself after all (skewed digit values, a 16-bit counter overflow).  Any array may be NULL;
 * passes <= 32. */
GLU_API glu_status glu_radix_sort_read_plan(glu_radix_sort sort, uint32_t* skipped, uint32_t* counted_alone,
                                            uint32_t* pair_role, size_t passes);
/* Host only (no device needed): the tiles of the in-LDS pass a whole-key sort of `count` elements of 4- or 8-byte keys
 * enqueues by default -- first_capacity: the tile that suits uniformly drawn keys, last_capacity: the largest one enqueued
 * behind it; both 0: such a sort makes no attempt (too small, or its runs would outgrow the largest tile). */
GLU_API glu_status glu_radix_sort_plan_finish(size_t count, uint32_t key_bytes, uint32_t* first_capacity,
                                              uint32_t* last_capacity);
/* A sort that ends in LDS (replaces six of the reference's eight 4-bit steps, glu/RadixSort.hpp:289-333, by one pass).  A sort of
 * whole 32-bit or 64-bit keys (any key type) of 7 * 2^22 (keys only: 2^25; 64-bit keys: 3 * 2^21) .. about 2^29 elements with 8-bit digits first tries a
 * shorter way to the same result: two counting passes on 16 TOP key bits, after which the array is 65536 runs of keys that share
 * those bits, and one pass in which a workgroup per run orders the run by the remaining low bits inside LDS, in place -- 52.25
 * instead of 72.5 bytes of memory traffic per pair with 32-bit keys, 80.25 instead of 225 with 64-bit keys (which rank key bits
 * [32, 48) and repair ties exactly).  The device decides from exact run lengths before anything is moved: the in-LDS pass is
 * enqueued in the tile geometry that suits uniformly drawn keys of this count (1536 / 2560 / 4608 / 9216 pairs) and in the next
 * larger ones, and the device runs the smallest that holds the runs (`capacity`); runs longer than the tile go to segmented
 * passes (glu_radix_sort_read_long_runs below) or -- 64-bit, typed and keys-only sorts; keys crowded into few runs -- send the sort
 * to the ordinary passes, at the cost of one extra read of the keys (every sort asks: its cost does not depend on what the
 * object sorted before).  The launch sequence is the same either way (the kernels of the sequence not taken return at once), so the
 * sort stays asynchronous and capturable.
 * This reports, for the last sort on the object (the caller has synchronised its stream): attempted = 1 if both sequences were
 * enqueued, accepted = 1 if the sort ended in LDS, longest_run = the longest run counted (0xFFFFFFFF: not counted), capacity =
 * the tile the device chose (refused: the largest one enqueued).  glu_radix_sort_read_plan describes the ordinary passes (all
 * "skipped without counting" when accepted = 1).
 * top_bit: the runs were the values of key bits [top_bit - 16, top_bit).  Untyped keys: the device chooses it from a sample of
 * the keys -- the highest bit that varies in the sample + 1, at least 16 (64-bit keys: moved up to 40 or 48 where a digit would
 * straddle the key words) -- so keys below 2^28 make 65536 runs of bits [12, 28) on an object's FIRST sort; the exact bits
 * collected by the first count kernel check the sample: a missed bit refuses the attempt and becomes the floor of the next
 * sort's sample.  Typed keys (and GLU_HIP_SORT_DEVICE_TOP=0): the whole key's top 16 bits / the round-4 guess from the object's
 * previous attempt.
 * GLU_HIP_SORT_LDS_FINISH=0 in the environment of glu_radix_sort_create switches the attempt off.  Any pointer may be NULL. */
GLU_API glu_status glu_radix_sort_read_finish(glu_radix_sort sort, uint32_t* attempted, uint32_t* accepted,
                                              uint32_t* longest_run, uint32_t* capacity, uint32_t* top_bit);
/* The narrow hand-off of a sort that ends in LDS (untyped 32-bit keys with values).  Behind the two counting passes a pair's position
 * says what its top key bits are, so the second of them hands the in-LDS pass only the low 16 bits of every key, in a side array of
 * n x 2 bytes in the object's scratch (reserved by glu_radix_sort_prepare, or by the first sort, for counts at which the attempt is
 * made): 48.25 instead of 52.25 bytes of memory traffic per pair.  The device decides (before anything moves) for it when the sort
 * ends in LDS, no run is longer than the tile and the in-LDS pass orders the runs by its bucket round; every other sort hands over
 * whole keys in the key array, as before.  narrow = 1: the last sort on the object took the narrow hand-off (the caller has
 * synchronised its stream).  GLU_HIP_SORT_NARROW_HANDOFF=0 (environment of glu_radix_sort_create, or glu_radix_sort_set_option BEFORE
 * the object's scratch is prepared: it decides the side array's allocation) switches it off. */
GLU_API glu_status glu_radix_sort_read_handoff(glu_radix_sort sort, uint32_t* narrow);
/* Runs LONGER than the tile of the in-LDS pass (round 5; 4-byte untyped keys with values): they no longer send the whole sort back
 * to the ordinary passes -- the device lists them as segments, two segmented counting passes (the reference's pass per segment,
 * glu/RadixSort.hpp:142-182) order just their elements by the low 16 key bits, and the in-LDS pass takes every other run.  The
 * tile is the smallest enqueued one that leaves at most 8192 runs and an eighth of the pairs to those passes (failing that the
 * largest, if it leaves at most half); keys crowded into few runs are still refused.  runs / sub_blocks / pairs: what the last
 * sort gave to the segmented passes (all 0: nothing, or the sort did not end in LDS).  GLU_HIP_SORT_LONG_RUNS=0 in the environment
 * of glu_radix_sort_create restores the round-4 rule (one run longer than the largest enqueued tile refuses the sort). */
GLU_API glu_status glu_radix_sort_read_long_runs(glu_radix_sort sort, uint32_t* runs, uint32_t* sub_blocks, uint32_t* pairs);
/* The same question for the last SEGMENTED sort of the object (glu_radix_sort_run_segments_ptr; the local sort of glu_dist_*):
 * a segmented sort by 16 key bits or more first tries ONE counting pass on the top digit of those bits (into the object's scratch
 * arrays) and one pass that orders every run (segment, top digit) by the remaining bits inside LDS on its way into the output --
 * the reference's pass, glu/RadixSort.hpp:289-333, once instead of three times for 24 bits.  `tile`: pairs a workgroup orders at
 * a time; `split`: workgroups a run is split over (by ranges of the remaining key bits: runs of the sharded sort at eight ranks are
 * four tiles long); runs that come out longer than tile x split are walked in pieces.  attempted: both sequences were enqueued;
 * accepted: the device found no run longer than `capacity` (32 tiles per workgroup) and ended the sort in LDS -- otherwise the
 * ordinary segmented passes ran; runs = segments x 256.
 * GLU_HIP_SEG_LDS_FINISH=0 in the environment of glu_radix_sort_create switches the attempt off.  Waits for the device. */
GLU_API glu_status glu_radix_sort_read_seg_finish(glu_radix_sort sort, uint32_t* attempted, uint32_t* accepted,
                                                  uint32_t* longest_run, uint32_t* capacity, uint32_t* runs, uint32_t* tile,
                                                  uint32_t* split);

/* ---- batched radix sort (not in the reference, whose RadixSort sorts one array per call while its BlellochScan takes
 * num_partitions, glu/BlellochScan.hpp:130-139): a stable ascending sort of EVERY SEGMENT of an array independently, in place,
 * in one asynchronous launch sequence, for all six glu_key_type's, with a uint32 value array or without (vals == NULL: keys only).
 *   - Result per segment = the stable sort glu_radix_sort_run_typed_ptr gives for that slice alone (the same natural order of
 *     signed and float keys: -0 < +0, NaNs beyond the infinities of their sign); values follow their keys.
 *   - Elements outside [offsets[0], offsets[num_segments]) are not touched.  Empty segments and segments of one element are legal.
 *     total, and count * num_partitions, must be < 2^32; num_segments (num_partitions) <= 2^24.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check: NULL keys with a non-zero size, an array that is not aligned to its
 *     element size, an unknown key type, count * num_partitions beyond the limit.  `offsets` lives on the DEVICE and is not read by
 *     the host: the kernels treat a segment whose end is below its begin, or beyond `total`, as empty, and so never reach outside
 *     [0, total); which elements move is then unspecified.  Offsets must be non-decreasing for the result above.
 *   - The call only enqueues on `stream`: no host synchronisation, no read-back of `offsets`, no side stream (a captured graph is a
 *     linear chain), and no device allocation once glu_radix_sort_prepare_batch covered the sizes (else grow-only allocation inside
 *     the call, as in every other entry point: not capturable).
 *   - Three size classes.  Up to 512 elements a WAVE sorts the segment (registers + a wave-private LDS slice, no workgroup barrier:
 *     the waves of a workgroup work on different segments); up to the single-block limit (16384 elements with 4-byte keys, 8192
 *     with 8-byte keys) a WORKGROUP sorts it inside LDS, in a tile of 1024, 4096 or 16384 (8192) elements; both read and write
 *     every element once.  LONGER segments: with device offsets one workgroup per segment streams 8-bit counting passes between the
 *     caller's arrays and the object's scratch arrays (correct for any length, one CU per segment: meant for the few long segments
 *     of a mixed batch); equal partitions longer than a tile are sorted one after the other by the ordinary sort, each large
 *     enough to fill the device.  With device offsets a binning kernel lists the segments of every class first and every class
 *     kernel walks its list with a grid sized to the device: seven launches whatever the segments look like. */

/* num_partitions adjacent partitions of `count` elements each (the shape of glu_scan_run_ptr) */
GLU_API glu_status glu_radix_sort_run_batch_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t count,
                                                size_t num_partitions, glu_key_type key_type, void* stream);
/* segment s = elements [offsets[s], offsets[s+1]); offsets: DEVICE array of num_segments + 1 uint32, non-decreasing */
GLU_API glu_status glu_radix_sort_run_batch_offsets_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t total,
                                                        const uint32_t* offsets, size_t num_segments,
                                                        glu_key_type key_type, void* stream);
/* Grow-only scratch so that the two calls above allocate nothing (and can be captured) for batches of up to `total` elements of
 * `key_bytes`-byte keys (4 or 8) in up to `num_segments` segments: the segment lists (at most 4 bytes per segment and class that
 * fits `total`) and, for the long class and for equal partitions beyond a tile, key (+ value) scratch of `total` elements
 * (glu_radix_sort_prepare_ex, with what it says about placing large arrays). */
GLU_API glu_status glu_radix_sort_prepare_batch(glu_radix_sort sort, size_t total, size_t num_segments, size_t key_bytes,
                                                int with_vals);
/* Host only, no device (unit-testable, like glu_radix_sort_plan_finish): which path an equal-length batch takes and the tile
 * it uses: path 0 = nothing to do (count <= 1), 1 = wave per segment, 2 = workgroup per segment, 3 = longer than an LDS tile
 * (tile: the largest one); tile in elements.  Either pointer may be NULL. */
GLU_API glu_status glu_radix_sort_plan_batch(size_t count, uint32_t key_bytes, int with_vals, uint32_t* path, uint32_t* tile);
/* Diagnostics of the last batched call on the object (the caller has synchronised its stream): how many segments each path took
 * (segments of 0 or 1 elements take none).  Any pointer may be NULL. */
GLU_API glu_status glu_radix_sort_read_batch(glu_radix_sort sort, uint32_t* wave_segments, uint32_t* block_segments,
                                             uint32_t* long_segments);

/* ---- exclusive scan: replaces glu::BlellochScan (glu/BlellochScan.hpp:80-191) ---------------------- */

/* BlellochScan::BlellochScan(data_type)                (BlellochScan.hpp:91-121) */
GLU_API glu_status glu_scan_create(glu_data_type data_type, glu_scan* out);
GLU_API glu_status glu_scan_destroy(glu_scan scan);
/* Optional: pre-size the internal block-sum scratch for count * num_partitions elements. */
GLU_API glu_status glu_scan_prepare(glu_scan scan, size_t count, size_t num_partitions);
/* BlellochScan::operator()(buffer, count, num_partitions)   (BlellochScan.hpp:130-139): in-place exclusive
 * `+` scan (identity 0) of num_partitions adjacent partitions of `count` elements each.  The reference's
 * argument checks are kept (:132-135): buffer != 0, count > 0, count a power of two, num_partitions >= 1. */
GLU_API glu_status glu_scan_run(glu_scan scan, glu_buffer buffer, size_t count, size_t num_partitions);
/* Raw-pointer form; additionally accepts any count > 0 (no power-of-two requirement).  From 2^23 4-byte elements up a
 * single-pass chained scan runs (not under stream capture, where the three-launch form is used): its order of additions
 * follows the arrival order of the chunks, so float sums are not bitwise reproducible from run to run there (integer
 * results are exact either way); GLU_HIP_SCAN_CHAINED=0 selects the reproducible form. */
GLU_API glu_status glu_scan_run_ptr(glu_scan scan, void* data, size_t count, size_t num_partitions, void* stream);

/* ---- batched scan (not in the reference, whose BlellochScan takes equal power-of-two partitions): EVERY SEGMENT of an array
 * replaced by its own exclusive `+` scan (identity 0), in place, in one asynchronous launch sequence, for all twelve
 * glu_data_type's.  Segment s is [offsets[s], offsets[s+1]), in elements of the object's data type.  Equal partitions have no
 * entry point of their own here: glu_scan_run_ptr is that entry point.
 *   - Result: element i of segment s receives the sum of elements [offsets[s], i) of the segment's ORIGINAL contents,
 *     component-wise for vector types.  The first element of a non-empty segment becomes 0.  Integer types are exact modulo 2^32.
 *     A float result is a sum of exactly those elements, in an order fixed by the geometry alone: the segment's address modulo
 *     16, its length and its class.  The same call (same pointers, same shape, same contents) gives the same bits every time: no
 *     atomics on values and no look-back in ticket or arrival order on this path (unlike the chained form of glu_scan_run_ptr).
 *   - Elements outside [offsets[0], offsets[num_segments]) are not touched.  Empty segments are legal anywhere.
 *     num_segments == 0: nothing is done, GLU_OK, NULL arrays are accepted.
 *   - Limits (those of the batched sort and the batched reduce): total < 2^32, num_segments <= 2^24, `data` aligned to its
 *     element size, 16 bytes at most, `offsets` 4-byte aligned.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check: NULL scan; NULL data with a non-zero total; NULL or misaligned
 *     offsets; misaligned data; the limits above.
 *   - `offsets` lives on the DEVICE and is never read by the host.  A segment whose end lies below its begin or beyond `total` is
 *     empty to every kernel, and no kernel reads or writes outside [0, total) of `data` whatever the offsets hold: list lengths
 *     and chunk slots are clamped to the lists' capacity, the chunk slots come from a 64-bit counter that cannot wrap (the
 *     batched reduce's lists and clamps).  Which elements of [0, total) change under malformed or overlapping offsets is
 *     unspecified, as in the batched sort.
 *   - The call only enqueues on `stream`: no host synchronisation, no read-back of `offsets`, no side stream, and no device
 *     allocation once glu_scan_prepare_batch covered the sizes (else grow-only allocation inside the call, as in every other
 *     entry point: not capturable).  The number of enqueued operations depends on `total` and `num_segments` as passed by the
 *     host, never on the data: the list counts are cleared, a binning kernel lists the segments by class, then one kernel scans
 *     the short segments, one the medium ones and three the long ones (at most seven enqueued operations; a class that no
 *     segment of a batch of `total` elements can belong to is skipped).
 *   - Three classes by the BYTES of a segment (glu_scan_plan_batch).  Up to 2 KiB a group of 4, 16 or 64 lanes of a wave holds
 *     the segment in registers (up to 128 bytes, up to 512 bytes, more): no barrier, no LDS.  Up to 64 KiB a workgroup scans it
 *     tile after tile with a running carry, with 16-byte accesses from its first 16-byte-aligned element: every element is read
 *     once and written once.  Longer segments are cut into chunks of 32 KiB: a workgroup per chunk writes the chunk's sum to the
 *     object's scratch, a second kernel scans each segment's sums in chunk order, a third scans every chunk with its sum of the
 *     chunks before it as carry-in, so one long segment occupies the whole device (three passes over memory instead of two). */

/* data[offsets[s] .. offsets[s+1]) = its own exclusive + scan, in place, for every s < num_segments;
 * offsets: DEVICE array of num_segments + 1 uint32, non-decreasing, in elements of the object's data type */
GLU_API glu_status glu_scan_run_batch_offsets_ptr(glu_scan scan, void* data, size_t total, const uint32_t* offsets,
                                                  size_t num_segments, void* stream);

/* The batched scan with any of Reduce's four operators, exclusive or inclusive, in place or into a second array: cumsum, cumprod,
 * cummin and cummax per segment.  The object is the one glu_scan_create makes; its scratch does not depend on the operator, so
 * `op` and `kind` are arguments of the call and may change from call to call.  For every segment [b, e) = [offsets[s],
 * offsets[s+1]) and every i in it, with x the ORIGINAL contents of `data`:
 *   - GLU_SCAN_EXCLUSIVE: out[i] = x[b] OP ... OP x[i-1], and out[b] = the identity of OP: 0 for Sum, 1 for Mul, +infinity (floats)
 *     or the type's maximum (integers) for Min, -infinity or the type's lowest value for Max (the values the batched reduce gives
 *     an empty segment).
 *   - GLU_SCAN_INCLUSIVE: out[i] = exclusive[i] OP x[i].  Under Sum a first element -0.0 therefore comes out as +0.0 (0 + -0.0).
 *   - Vector types are scanned per component.  Integers wrap modulo 2^32 as they do in Reduce.  The earlier operand is always on
 *     the left.  Float Min / Max are `a < b ? a : b` and `a > b ? a : b` (Reduce's), which do not commute on NaN: results at and
 *     behind a NaN in a segment are unspecified, and which of two zeros of different sign comes out is, too.
 *   - out == NULL or out == data: in place.  Otherwise `data` is only read and `out` receives the results at the same positions;
 *     positions of `out` outside the segments are not touched.  `out` is aligned like `data` (to the element size, 16 bytes at
 *     most) and need not share data's address modulo 16: which element goes to which lane follows data's address alone, 16-byte
 *     stores are used only where they are aligned on out's side, and the results are the same bits wherever `out` lies.  Ranges
 *     of `total` elements that overlap without being identical: GLU_ERROR_INVALID_ARGUMENT.
 *   - offsets == NULL with num_segments == 1: the one segment [0, total), the scan of a whole array.  The two offset words are
 *     written into a scratch of the object by a small kernel that takes `total` as an argument: no host-to-device copy, the call
 *     stays capturable (glu_scan_prepare_batch reserves that scratch too).  total < 2^32 here as well.  NULL offsets with more
 *     than one segment: GLU_ERROR_INVALID_ARGUMENT.
 *   - An `op` outside glu_reduce_operator or a `kind` outside glu_scan_kind: GLU_ERROR_INVALID_ARGUMENT.
 *   - Everything else is the contract of glu_scan_run_batch_offsets_ptr above: the limits, device offsets the host never reads,
 *     malformed segments empty to every kernel, enqueue only, the same classes (glu_scan_plan_batch, glu_scan_read_batch), no
 *     atomics on values, no look-back, the same bits every time; a segment's result depends on its data, its length, data's
 *     address modulo 16 and its class only.  The chunk partials of the long class are combined with `op` and scanned exclusively
 *     whatever `kind` is.  op = GLU_REDUCE_SUM, kind = GLU_SCAN_EXCLUSIVE, in place is glu_scan_run_batch_offsets_ptr itself. */
typedef enum glu_scan_kind
{
    GLU_SCAN_EXCLUSIVE = 0,
    GLU_SCAN_INCLUSIVE = 1
} glu_scan_kind;
GLU_API glu_status glu_scan_run_batch_offsets_op_ptr(glu_scan scan, const void* data, void* out, size_t total,
                                                     const uint32_t* offsets, size_t num_segments, glu_reduce_operator op,
                                                     glu_scan_kind kind, void* stream);
/* Grow-only scratch so that the call above allocates nothing (and can be captured) for batches of up to `total` (< 2^32) elements
 * in up to `num_segments` (<= 2^24) segments: the segment lists (4 bytes per segment and class that fits `total`, 16 bytes per
 * 32 KiB chunk), one partial per chunk of the long class, and the two offset words of the one-segment form. */
GLU_API glu_status glu_scan_prepare_batch(glu_scan scan, size_t total, size_t num_segments);
/* Host only, no device (unit-testable, like glu_reduce_plan_batch): the class of a segment of `count` elements of `elem_bytes`
 * (4, 8, 16 or 32) bytes: path 0 = nothing to do, 1 = a wave (or part of a wave) per segment, 2 = a workgroup per segment,
 * 3 = several workgroups per segment; workgroups = how many one such segment is spread over (0 for an empty one), as in
 * glu_reduce_plan_batch.  Either pointer may be NULL. */
GLU_API glu_status glu_scan_plan_batch(size_t count, uint32_t elem_bytes, uint32_t* path, uint32_t* workgroups);
/* Diagnostics of the last batched call on the object (the caller has synchronised its stream): how many segments each path took
 * (empty ones take none).  Any pointer may be NULL. */
GLU_API glu_status glu_scan_read_batch(glu_scan scan, uint32_t* wave_segments, uint32_t* block_segments,
                                       uint32_t* long_segments);

/* ---- reduce: replaces glu::Reduce (glu/Reduce.hpp:51-136) ----------------------------------------- */

/* Reduce::Reduce(data_type, operator)                  (Reduce.hpp:62-107) */
GLU_API glu_status glu_reduce_create(glu_data_type data_type, glu_reduce_operator op, glu_reduce* out);
GLU_API glu_status glu_reduce_destroy(glu_reduce reduce);
/* Reduce::operator()(buffer, count)                    (Reduce.hpp:111-135): data[0] = op over data[0..count),
 * component-wise for vector types.  Elements other than data[0] are left untouched (the reference clobbers
 * some of them; only data[0] is contract).  Checks kept (:113-114): buffer != 0, count > 0. */
GLU_API glu_status glu_reduce_run(glu_reduce reduce, glu_buffer buffer, size_t count);
GLU_API glu_status glu_reduce_run_ptr(glu_reduce reduce, void* data, size_t count, void* stream);

/* ---- batched reduce (not in the reference, whose Reduce folds one array per call): out[s] = op over EVERY SEGMENT of an array,
 * each on its own, in one asynchronous launch sequence, for all twelve glu_data_type's and four glu_reduce_operator's.
 *   - `data` is READ ONLY: nothing is written to it.  This differs from glu_reduce_run_ptr, which works in place and leaves its
 *     result in data[0].  `out` receives one element of the object's data type per segment (vector types: component-wise) and
 *     must not overlap `data`; elements of `out` beyond the segments are not touched.  Both arrays must be aligned to the
 *     element size, 16 bytes at most (the rule of glu_reduce_run_ptr).
 *   - An EMPTY segment (count == 0, or equal offsets) yields the operator's identity: Sum 0, Mul 1, Min the largest value of the
 *     scalar type (floats: +inf), Max its lowest value (floats: -inf).  num_partitions == 0 / num_segments == 0: nothing is done,
 *     GLU_OK, NULL arrays are accepted.
 *   - Equal partitions are indexed with 64 bits: count * num_partitions may exceed 2^32 (as in glu_scan_run_ptr and
 *     glu_reduce_run_ptr); num_partitions must be < 2^31.  With device offsets total must be < 2^32 and num_segments <= 2^24
 *     (the limits of the batched sort).
 *   - `offsets` lives on the DEVICE and is never read by the host.  A segment whose end lies below its begin or beyond `total` is
 *     empty to every kernel (its out element gets the identity), so nothing outside [0, total) of `data` is read whatever the
 *     offsets hold, and every other segment still gets its result as long as those segments together hold no more than `total`
 *     elements -- what non-decreasing offsets guarantee and what the segment lists are sized for.  Of segments that overlap each
 *     other beyond that, those that found no room in the lists get NO result: their out elements keep what they held (which
 *     ones depends on arrival order); a result that is written is always the whole segment's.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check: NULL reduce; NULL data or out with a non-zero size; NULL or
 *     misaligned offsets; a misaligned array; out overlapping data; the limits above.
 *   - Reproducible: the same call (same pointers, same shape, same contents) gives the same bits every time.  The order of
 *     combination follows from the geometry alone -- a segment's address modulo 16, its length and its class -- with no atomics on
 *     values and nothing combined in arrival order.  NaNs and the sign of a zero under Min / Max are unspecified, as in
 *     glu_reduce_run_ptr.
 *   - The call only enqueues on `stream`: no host synchronisation, no read-back of `offsets`, no side stream, and no device
 *     allocation once glu_reduce_prepare_batch covered the sizes (else grow-only allocation inside the call, as in every other
 *     entry point: not capturable).  The number of launches depends on the sizes passed by the host, never on the data: with
 *     device offsets the list counts are cleared, a binning kernel writes the identity of empty segments and lists the others by
 *     class, then one kernel folds the short segments, one the medium ones and two the long ones (at most six enqueued
 *     operations); equal partitions take the one or two kernels of their class.
 *   - Three classes by the BYTES of a segment (glu_reduce_plan_batch).  Up to 4 KiB a group of 4, 16 or 64 lanes of a wave folds
 *     the segment (up to 16, up to 64, more elements): no barrier, no LDS.  Up to 256 KiB a workgroup folds it with 16-byte loads
 *     from its first 16-byte-aligned element.  Longer segments are cut into chunks of 256 KiB: a workgroup per chunk writes a
 *     partial result to the object's scratch, a second kernel folds each segment's partials in chunk order, so one long segment
 *     occupies the whole device. */

/* out[p] = op over data[p*count .. (p+1)*count), p < num_partitions (the shape of glu_scan_run_ptr) */
GLU_API glu_status glu_reduce_run_batch_ptr(glu_reduce reduce, const void* data, void* out, size_t count,
                                            size_t num_partitions, void* stream);
/* out[s] = op over data[offsets[s] .. offsets[s+1]); offsets: DEVICE array of num_segments + 1 uint32, non-decreasing */
GLU_API glu_status glu_reduce_run_batch_offsets_ptr(glu_reduce reduce, const void* data, void* out, size_t total,
                                                    const uint32_t* offsets, size_t num_segments, void* stream);
/* Grow-only scratch so that the two calls above allocate nothing (and can be captured) for batches of up to `total` (< 2^32)
 * elements in up to `num_segments` (<= 2^24) segments: the segment lists (4 bytes per segment and class that fits `total`, 16
 * bytes per 256 KiB chunk) and one partial result per chunk of the long class. */
GLU_API glu_status glu_reduce_prepare_batch(glu_reduce reduce, size_t total, size_t num_segments);
/* Host only, no device (unit-testable, like glu_radix_sort_plan_batch): the class of a segment of `count` elements of
 * `elem_bytes` (4, 8, 16 or 32) bytes: path 0 = empty, 1 = a wave (or part of a wave) per segment, 2 = a workgroup per segment,
 * 3 = several workgroups per segment; workgroups = how many one such segment is spread over (0 for an empty one).  Either
 * pointer may be NULL. */
GLU_API glu_status glu_reduce_plan_batch(size_t count, uint32_t elem_bytes, uint32_t* path, uint32_t* workgroups);
/* Diagnostics of the last batched call on the object (the caller has synchronised its stream): how many segments each path took
 * (empty ones take none).  Any pointer may be NULL. */
GLU_API glu_status glu_reduce_read_batch(glu_reduce reduce, uint32_t* wave_segments, uint32_t* block_segments,
                                         uint32_t* long_segments);

/* ---- key runs (not in the reference): the runs of equal keys of an array -- of SORTED keys: the groups -- as an offsets array
 * in exactly the form the three batched calls above take, so that what follows a sort by key needs no trip to the host:
 * reduce-by-key is glu_key_runs_run_ptr + glu_reduce_run_batch_offsets_ptr on the values, scan-by-key is glu_key_runs_run_ptr +
 * glu_scan_run_batch_offsets_ptr, a sort by a second key inside every group is glu_key_runs_run_ptr +
 * glu_radix_sort_run_batch_offsets_ptr.  Those compositions are two calls on one stream and have no entry point of their own
 * (glu::Reduce::reduce_by_key and glu::BlellochScan::scan_by_key make them).
 *   - A HEAD is an index i with i == 0 or ((keys[i] ^ keys[i-1]) & mask) != 0, where mask covers the key bits
 *     [begin_bit, end_bit).  R = the number of heads, h_0 < h_1 < ... their indices.  Equality is on BITS, the equivalence of the
 *     sort's total order for all six glu_key_type's: -0.0 and +0.0 are different keys, NaNs with different payloads are
 *     different keys; hence `key_bits` (32 or 64, as in glu_radix_sort_run_bit_range_ptr) and no key type.
 *     begin_bit == end_bit: no bit tells keys apart, one run if count > 0.  The keys need not be sorted: unsorted keys simply
 *     have more runs (the call is a run-length encoder).
 *   - offsets (max_runs + 1 entries, EVERY one written): offsets[r] = h_r for r < min(R, max_runs), offsets[r] = count for
 *     min(R, max_runs) <= r <= max_runs.  The array is non-decreasing, starts at 0 when count > 0 and ends at count: legal
 *     offsets of max_runs segments for the batched calls, the segments behind the last run empty.  If R > max_runs the last
 *     segment holds the remaining runs merged.
 *   - unique_keys (optional, NULL skips it): unique_keys[r] = keys[h_r] for r < min(R, max_runs), the WHOLE key, not its masked
 *     bits.  Entries behind that are not touched.
 *   - *num_runs = R, the true number even where it exceeds max_runs: how a caller detects overflow (after synchronising, or on
 *     the device).
 *   - `keys` is READ ONLY.  count == 0: R = 0, every offset 0, NULL keys accepted.
 *   - Limits: count < 2^32; max_runs < 2^32; keys and unique_keys aligned to the key size, offsets and num_runs to 4 bytes.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check: NULL runs; NULL keys with count > 0; NULL offsets or num_runs;
 *     misalignment; key_bits other than 32 or 64; begin_bit > end_bit or end_bit > key_bits; the limits above; offsets,
 *     unique_keys or num_runs overlapping keys.
 *   - The call only enqueues on `stream`: no host synchronisation, no side stream, no read-back, and no device allocation once
 *     glu_key_runs_prepare covered the count (else grow-only allocation inside the call: not capturable).  Always three
 *     kernels, whose grids follow from count, max_runs and the address of keys, never from the data: the heads of every tile of
 *     keys counted (glu_key_runs_plan: 256 threads x four 16-byte packs), the counts scanned by one workgroup with the tile loop
 *     of the batched scan, the heads written at their ranks and the rest of offsets filled.  The keys are read twice; no
 *     workgroup waits for another (no look-back, nothing in arrival order), so a captured call replays on any keys. */
GLU_API glu_status glu_key_runs_create(glu_key_runs* out);
GLU_API glu_status glu_key_runs_destroy(glu_key_runs runs);
/* Grow-only scratch so that the call below allocates nothing (and can be captured) for up to `count` (< 2^32) keys of `key_bits`
 * (32 or 64) bits: 4 bytes per tile of keys. */
GLU_API glu_status glu_key_runs_prepare(glu_key_runs runs, size_t count, uint32_t key_bits);
/* offsets[0 .. max_runs], unique_keys[0 .. min(R, max_runs)) and *num_runs as above; all four arrays on the DEVICE */
GLU_API glu_status glu_key_runs_run_ptr(glu_key_runs runs, const void* keys, size_t count, uint32_t key_bits,
                                        uint32_t begin_bit, uint32_t end_bit, void* unique_keys, uint32_t* offsets,
                                        size_t max_runs, uint32_t* num_runs, void* stream);
/* Host only, no device (unit-testable, like glu_scan_plan_batch): tile = keys per tile, tiles = ceil(count / tile), the tiles of
 * `count` keys that start on a 16-byte boundary (tiles are counted from the boundary at or below `keys`: keys that start behind
 * one can take one tile more), scan_rounds = the rounds the one workgroup that scans the tile counts makes (4096 counts each).
 * Any pointer may be NULL. */
GLU_API glu_status glu_key_runs_plan(size_t count, uint32_t key_bits, uint32_t* tile, uint32_t* tiles, uint32_t* scan_rounds);

/* ---- select (not in the reference): stable stream compaction by a stencil and a comparison.  Element i of `count` is SELECTED
 * iff stencil[i] OP threshold holds; the indices of the selected elements and the items at them are written side by side, in
 * ascending order of i, and their number is reported.  Keeping the values above a threshold, dropping zeros, keeping the groups
 * whose batched reduce passed a test: all on the device, on the caller's stream.
 *   - `stencil` is a device array of one of five element types: the four scalar glu_data_type's FLOAT, DOUBLE, INT, UINT (0 .. 3),
 *     or GLU_SELECT_STENCIL_BYTE (12), an unsigned byte -- what a bool mask or an array of byte flags is.
 *   - OP is one of GLU_SELECT_EQ, NE, LT, LE, GT, GE (0 .. 5).
 *   - `threshold` is a HOST pointer to one value of the stencil's type.  It is read during the call and passed by value to the
 *     kernels, so that the call stays capturable (a captured call replays with the threshold it was captured with).  NULL means
 *     zero: the classic "flags" form is UINT or BYTE, GLU_SELECT_NE, NULL.
 *   - FLOAT and DOUBLE compare as IEEE VALUES: a NaN, in the stencil or as the threshold, satisfies only NE, and -0.0 == +0.0.
 *     This is deliberately NOT the bit order of the sort (glu_radix_sort_run_typed_ptr puts -0.0 in front of +0.0 and orders the
 *     NaNs by their payloads) nor the bit equality of key runs: a comparison with a threshold means what it means in C.
 *     INT compares signed, UINT and BYTE compare unsigned.
 *   - S = the number of selected elements, i_0 < i_1 < ... their indices: the selection is STABLE.
 *   - out_indices (uint32, optional, NULL skips it): out_indices[r] = i_r for r < min(S, max_out).
 *   - out_items (optional; `items` and `out_items` are both NULL or both given): out_items[r] = items[i_r] for
 *     r < min(S, max_out), copied bit for bit.  item_bytes is 4, 8, 16 or 32 -- the sizes of all twelve glu_data_type's -- and is
 *     not looked at where items is NULL.  `items` may be the stencil array itself: select-if on the values.
 *   - *num_selected = S, the true number even where it exceeds max_out: how a caller detects overflow (after synchronising, or
 *     on the device).
 *   - THE OVERFLOW RULE: at most max_out entries are written; entries of the two output arrays at or behind min(S, max_out) are
 *     NOT TOUCHED, and nothing outside the arrays is read or written.  `stencil` and `items` are READ ONLY.
 *   - count == 0: S = 0, NULL stencil accepted.  With both outputs NULL (or max_out == 0) the call only counts.
 *   - Limits: count < 2^32; max_out < 2^32; stencil aligned to its element size, items and out_items to min(item_bytes, 16),
 *     out_indices and num_selected to 4 bytes.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument: NULL select; NULL
 *     stencil with count > 0; NULL num_selected; only one of items and out_items; a stencil_type, op or item_bytes outside the
 *     lists above; misalignment; the limits above; out_items, out_indices or num_selected overlapping stencil or items (the first
 *     min(count, max_out) entries of an output array are what can be written; arrays that merely touch are fine).  A refused call
 *     writes nothing.
 *   - The call only enqueues on `stream`: no host synchronisation, no side stream, no read-back, and no device allocation once
 *     glu_select_prepare covered the count (else grow-only allocation inside the call: not capturable).  Three kernels, whose
 *     grids follow from count and the address of stencil, never from the data: the selected elements of every tile counted
 *     (glu_select_plan), the counts scanned by one workgroup (the scan of key runs), the selected elements written at their
 *     ranks.  The stencil is read twice; no workgroup waits for another (no look-back, no atomics, nothing in arrival order), so
 *     a captured call replays on any contents. */
#define GLU_SELECT_STENCIL_BYTE 12 /* a stencil of unsigned bytes; the other stencil types are GLU_DATA_TYPE_FLOAT .. _UINT */
typedef enum glu_select_op
{
    GLU_SELECT_EQ = 0,
    GLU_SELECT_NE,
    GLU_SELECT_LT,
    GLU_SELECT_LE,
    GLU_SELECT_GT,
    GLU_SELECT_GE,
    GLU_SELECT_OP_COUNT_
} glu_select_op;
GLU_API glu_status glu_select_create(glu_select* out);
GLU_API glu_status glu_select_destroy(glu_select select);
/* Grow-only scratch so that the call below allocates nothing (and can be captured) for up to `count` (< 2^32) elements of a
 * stencil of `stencil_type`: 4 bytes per tile of the stencil. */
GLU_API glu_status glu_select_prepare(glu_select select, size_t count, int stencil_type);
/* out_indices[0 .. min(S, max_out)), out_items[0 .. min(S, max_out)) and *num_selected as above; stencil, items and the three
 * outputs on the DEVICE, threshold on the HOST */
GLU_API glu_status glu_select_run_ptr(glu_select select, const void* stencil, int stencil_type, int op, const void* threshold,
                                      size_t count, const void* items, uint32_t item_bytes, void* out_items,
                                      uint32_t* out_indices, size_t max_out, uint32_t* num_selected, void* stream);
/* Host only, no device (unit-testable, like glu_key_runs_plan and with its meaning): tile = stencil elements per tile (a whole
 * number of 16-byte packs), tiles = ceil(count / tile), the tiles of `count` elements that start on a 16-byte boundary (tiles are
 * counted from the boundary at or below `stencil`: a stencil that starts behind one can take one tile more), scan_rounds = the
 * rounds the one workgroup that scans the tile counts makes (4096 counts each).  Any pointer may be NULL. */
GLU_API glu_status glu_select_plan(size_t count, int stencil_type, uint32_t* tile, uint32_t* tiles, uint32_t* scan_rounds);

/* ---- batched select (not in the reference): the select above over the segments of the batched family, in one launch sequence.
 * It compacts the selected elements exactly as glu_select_run_ptr does, writes the OFFSETS OF THE COMPACTED SEGMENTS in the form
 * every batched operator takes, and can write indices local to the segment: filtering ragged data while keeping the groups --
 * the samples of each group above a threshold, each row's non-zeros -- with the rows of a batched reduce, histogram or top-k made
 * before the filter still lining up, because an emptied segment stays an empty segment.
 *   - The segments are equal partitions (`count` elements each, `num_partitions` of them: total = count * num_partitions,
 *     b_s = s * count), or device `offsets` (uint32, num_segments + 1 entries, what glu_key_runs_run_ptr writes):
 *     b_s = min(offsets[s], total) for s = 0 .. num_segments.  THE CONTRACT IS TOTAL: it defines a result for malformed offsets.
 *   - Element i is SELECTED iff b_0 <= i < b_num_segments and stencil[i] OP threshold.  Elements outside that range are never
 *     selected (expand's rule).  The stencil types, the six comparisons, the host threshold passed by value, the item widths and
 *     the alignment rules are those of glu_select_run_ptr.
 *   - S = the number selected, i_0 < i_1 < ... their indices.  out_items[r] = items[i_r] for r < min(S, max_out); entries at or
 *     behind that are not touched.  *num_selected = S, the true number: overflow shows as *num_selected > max_out.
 *   - out_indices, index_form GLU_SELECT_INDEX_GLOBAL: out_indices[r] = i_r.  GLU_SELECT_INDEX_LOCAL: out_indices[r] = i_r - b_s
 *     with s the last segment whose b_s <= i_r (numpy.searchsorted(offsets, i, "right") - 1, what expand and the batched top-k
 *     mean by a segment's element).
 *   - out_offsets[s] = min(max_out, the number of selected i < b_s) for EVERY s = 0 .. num_segments.  With non-decreasing offsets
 *     out_offsets[0] = 0 and segment s of the compacted arrays is [out_offsets[s], out_offsets[s + 1]).  The offsets are clamped
 *     to max_out: they always describe what was written, and a following batched call stays in bounds.
 *   - Offsets that decrease or lie beyond total: the definitions above still hold for out_offsets, the items, the GLOBAL indices
 *     and *num_selected; LOCAL indices are then unspecified; nothing outside the arrays is read or written in any case.
 *   - Each of the three outputs is optional: out_offsets may be NULL, out_indices may be NULL, items and out_items are both NULL
 *     or both given.  With only out_offsets the call counts per segment.  num_segments == 0 writes *num_selected = 0 and nothing
 *     else.
 *   - Limits: total < 2^32; num_segments <= 2^24; max_out < 2^32; offsets and out_offsets aligned to 4 bytes.
 *   - GLU_ERROR_INVALID_ARGUMENT, with a message that names the argument and nothing written, for everything the single call
 *     refuses; NULL or misaligned offsets; a misaligned out_offsets; an index_form outside 0 .. 1; out_offsets overlapping an
 *     input or another output; offsets overlapping an output.
 *   - The call only enqueues on `stream`: no host synchronisation, no read-back, no atomics, no look-back, nothing in arrival
 *     order, and no device allocation once glu_select_prepare_batch covered the sizes.  At most four kernels, whose grids follow
 *     from total, num_segments and the address of the stencil, never from the data: the single call's count, which also stores one
 *     flag bit per element and the wave sums of every tile; the count scan; one thread per boundary, which reads a scanned count,
 *     a wave sum and one wave's flag words (two or three cache lines per boundary whatever the data hold: 2^24 empty segments at
 *     one position are 2^24 threads, not one workgroup's loop); the single call's write, which takes its flags from the stored
 *     bits -- the batched call reads the stencil ONCE.  A captured call replays on other contents and on other offsets of the
 *     same shape.  THE SAME INPUT GIVES THE SAME BITS EVERY TIME. */
typedef enum glu_select_index
{
    GLU_SELECT_INDEX_GLOBAL = 0,
    GLU_SELECT_INDEX_LOCAL = 1
} glu_select_index;
/* Grow-only scratch so that the two calls below allocate nothing (and can be captured) for up to `total` (< 2^32) elements of a
 * stencil of `stencil_type`, at any number of segments: per tile of the stencil (one more than glu_select_plan's tiles) 4 bytes
 * of count, 16 bytes of wave sums and tile / 8 bytes of flags -- about total / 8 bytes, the figure glu_select_plan_batch
 * returns.  It is separate from the single call's scratch. */
GLU_API glu_status glu_select_prepare_batch(glu_select select, size_t total, size_t num_segments, int stencil_type);
/* equal partitions; everything but threshold on the DEVICE */
GLU_API glu_status glu_select_run_batch_ptr(glu_select select, const void* stencil, int stencil_type, int op, const void* threshold,
                                            size_t count, size_t num_partitions, const void* items, uint32_t item_bytes,
                                            void* out_items, uint32_t* out_indices, int index_form, size_t max_out,
                                            uint32_t* out_offsets, uint32_t* num_selected, void* stream);
/* device offsets */
GLU_API glu_status glu_select_run_batch_offsets_ptr(glu_select select, const void* stencil, int stencil_type, int op,
                                                    const void* threshold, size_t total, const uint32_t* offsets, size_t num_segments,
                                                    const void* items, uint32_t item_bytes, void* out_items, uint32_t* out_indices,
                                                    int index_form, size_t max_out, uint32_t* out_offsets, uint32_t* num_selected,
                                                    void* stream);
/* Host only, pure, no device: tile and tiles as glu_select_plan's for `total` elements; scan_rounds = the rounds of the count scan
 * over tiles + 1 counts (the last one becomes the total); kernels = those of a call with all three outputs (4; the offsets and the
 * write kernel drop out with their outputs, and the form changes none; 0 where total or num_segments is 0: the call only clears);
 * scratch_bytes = what glu_select_prepare_batch reserves (0 where total is 0).  Any pointer may be NULL. */
GLU_API glu_status glu_select_plan_batch(size_t total, size_t num_segments, int stencil_type, int index_form, uint32_t* tile,
                                         uint32_t* tiles, uint32_t* scan_rounds, uint32_t* kernels, size_t* scratch_bytes);

/* ---- sorted search (not in the reference): the lower and the upper bound of many needles in a sorted haystack, what
 * numpy.searchsorted is, on the device and on the caller's stream.  A join against the unique keys of key runs, a membership
 * test, the bin index of every sample over arbitrary sorted bin edges (the COUNTS per bin are glu_histogram_run_edges_ptr), the
 * rank of a value in a sorted array.
 *   - `hay`: hay_count keys of one of the six glu_key_type's, sorted in the order glu_radix_sort_run_typed_ptr produces.  For
 *     floats that is the TOTAL ORDER ON BITS: -0.0 < +0.0, and the NaNs lie beyond the infinities of their sign, ordered by
 *     their payloads.  This is deliberately the SORT'S order and NOT the IEEE comparison of select (glu_select_run_ptr): a
 *     position in a sorted array means what the sort made of it.  `needles`: needle_count keys of the same type, in any order.
 *   - With enc the encoding the sort gives a key (unsigned, in the sort's order):
 *       out_lower[j] = the number of i with enc(hay[i]) <  enc(needles[j])
 *       out_upper[j] = the number of i with enc(hay[i]) <= enc(needles[j])
 *     Both are device uint32_t[needle_count]; either may be NULL, not both; every entry is written.  A needle is in the
 *     haystack iff upper > lower, and hay[lower .. upper) are its copies.  `hay` and `needles` are READ ONLY.
 *   - hay_count == 0: every output is 0 and NULL hay is accepted.  needle_count == 0: nothing is enqueued beyond what the index
 *     needs.
 *   - Limits: hay_count < 2^32 and needle_count < 2^32; hay and needles aligned to the key size, the outputs to 4 bytes.
 *   - A `hay` that is NOT SORTED gives unspecified positions in [0, hay_count] and never a read outside the arrays: every probe
 *     index is clamped to the range it searches.
 *   - TWO PATHS, chosen on the host from the counts and an option, never from the data:
 *       DIRECT   a branch-free binary search of the haystack in global memory, ceil(log2(hay_count + 1)) probes for every
 *                needle (a trip count that is the same for the whole kernel), one needle per lane.  One kernel.  Few needles, short
 *                haystacks.
 *       INDEXED  an index of F-ary samples of the haystack, F = 128 / sizeof(key) keys to the 128-byte line (32 or 16): level k
 *                holds len_k = floor(hay_count / F^k) encoded keys, level_k[t] = enc(hay[(t + 1) * F^k - 1]), up to the first
 *                level L with len_L <= TOP_ENTRIES, which the search kernel keeps in LDS.  A needle is searched in LDS and then
 *                in ONE line per level, L lines in all, the haystack's among them.  The index holds fewer than
 *                hay_count / (F - 1) keys and lives in the object's grow-only scratch, every level from a 128-byte boundary;
 *                building it is one kernel that reads one key of every line of the haystack.  L == 0 (hay_count <= TOP_ENTRIES) has no
 *                index: the call is DIRECT.
 *     GLU_SEARCH_PATH_AUTO (the default) takes INDEXED iff L >= 1 and needle_count * 128 >= hay_count.  A call that builds the
 *     index enqueues two kernels, every other call one.
 *   - glu_sorted_search_index_ptr builds the index of a haystack and remembers (hay, hay_count, key_type, TOP_ENTRIES).
 *     glu_sorted_search_run_ptr on the INDEXED path without reuse_index builds it again and remembers it too.  reuse_index != 0
 *     is the caller's PROMISE that the haystack has not changed since: the call takes INDEXED whatever the needle count and
 *     enqueues only the search kernel; GLU_ERROR_INVALID_STATE if no index was built or if one of the four remembered values
 *     differs from the call's.
 *   - glu_sorted_search_set_option: "PATH" = GLU_SEARCH_PATH_AUTO, _DIRECT or _INDEXED (INDEXED with L == 0 still runs DIRECT);
 *     "TOP_ENTRIES" = the most entries of the top level, from F up to what LDS holds (8192 4-byte or 4096 8-byte keys, the
 *     default; a call refuses a value outside the range of its own key width).  Any other name, or a value out of range, is
 *     GLU_ERROR_INVALID_ARGUMENT.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument: NULL search; NULL hay
 *     with hay_count > 0; NULL needles with needle_count > 0; both outputs NULL; misalignment; a bad key type; the limits above;
 *     an output overlapping hay, needles or the other output (arrays that merely touch are fine).  A refused call writes nothing.
 *   - The calls only enqueue on `stream`: no host synchronisation, no side stream, no read-back, no atomics, nothing that waits
 *     for another workgroup, and no device allocation once glu_sorted_search_prepare covered the haystack (else grow-only
 *     allocation inside the call: not capturable; scratch that grows forgets the remembered index).  The kernels and their grids
 *     follow from the counts and the addresses, so a captured call replays on any contents.
 *   - OUT OF SCOPE: a haystack length that lives on the device (the idiom for the unique keys of key runs: pre-fill
 *     unique_keys[0 .. max_runs) with the type's largest key and search all max_runs entries); a special
 *     path for sorted needles (neighbouring lanes already share their lines).  A search per segment, every segment's needles in
 *     its own haystack, is glu_sorted_search_run_batch_ptr / glu_sorted_search_run_batch_offsets_ptr below. */
typedef struct glu_sorted_search_s* glu_sorted_search;
enum
{
    GLU_SEARCH_PATH_AUTO = 0,
    GLU_SEARCH_PATH_DIRECT = 1,
    GLU_SEARCH_PATH_INDEXED = 2,
    GLU_SEARCH_PATH_BATCH = 3 /* reported by glu_sorted_search_last after a batched call; not a value of the PATH option */
};
GLU_API glu_status glu_sorted_search_create(glu_sorted_search* out);
GLU_API glu_status glu_sorted_search_destroy(glu_sorted_search search);
/* Grow-only scratch for the index of `hay_count` (< 2^32) keys of `key_type` at the TOP_ENTRIES set now, so that the calls below
 * allocate nothing (and can be captured). */
GLU_API glu_status glu_sorted_search_prepare(glu_sorted_search search, size_t hay_count, glu_key_type key_type);
GLU_API glu_status glu_sorted_search_set_option(glu_sorted_search search, const char* name, long long value);
GLU_API glu_status glu_sorted_search_index_ptr(glu_sorted_search search, const void* hay, size_t hay_count, glu_key_type key_type,
                                               void* stream);
GLU_API glu_status glu_sorted_search_run_ptr(glu_sorted_search search, const void* hay, size_t hay_count, const void* needles,
                                             size_t needle_count, glu_key_type key_type, uint32_t* out_lower, uint32_t* out_upper,
                                             int reuse_index, void* stream);
/* Host only, no device: what a call with these counts does under GLU_SEARCH_PATH_AUTO.  top_entries 0: the default.  path =
 * GLU_SEARCH_PATH_DIRECT or _INDEXED; levels = L of the level rule above, whatever the path; fanout = F; index_bytes = the
 * scratch of the L levels, sum over k = 1 .. L of len_k * sizeof(key) rounded up to 128 (what prepare reserves).  Any pointer
 * may be NULL. */
GLU_API glu_status glu_sorted_search_plan(size_t hay_count, size_t needle_count, glu_key_type key_type, uint32_t top_entries,
                                          uint32_t* path, uint32_t* levels, uint32_t* fanout, size_t* index_bytes);
/* What the host enqueued in the object's last index_ptr or run_ptr (no device read): the path taken, the levels of the index
 * used (0 on the DIRECT path), the number of kernels. */
GLU_API glu_status glu_sorted_search_last(glu_sorted_search search, uint32_t* path, uint32_t* levels, uint32_t* kernels);

/* ---- batched sorted search (not in the reference): every segment's needles in that segment's own haystack, one kernel for the
 * whole batch, on the same glu_sorted_search object.  torch.searchsorted with a batched sorted sequence (sorted[B, N],
 * values[B, M]); the upper bound of M uniform numbers per row in that row's CDF (inverse-CDF sampling over the batched scan); the
 * positions of one side's keys within the matching group of the other after sort -> key runs on both sides, and the rank of a
 * value within its group.  enc, the six key types and the order are those of glu_sorted_search_run_ptr: the sort's total order on
 * bits, not select's IEEE comparison.
 *   - EQUAL PARTITIONS (glu_sorted_search_run_batch_ptr; the shape of glu_reduce_run_batch_ptr): row p of the haystack is
 *     hay[p * hay_count .. (p + 1) * hay_count), its needles are needles[p * needle_count .. (p + 1) * needle_count).
 *     hay_count * num_partitions < 2^32 and needle_count * num_partitions < 2^32.
 *   - DEVICE OFFSETS (glu_sorted_search_run_batch_offsets_ptr): hay_offsets and needle_offsets are device arrays of
 *     num_segments + 1 uint32, non-decreasing, as key runs writes them; the host never reads them.  Segment s has the haystack
 *     [hay_offsets[s], hay_offsets[s + 1]) and the needles [needle_offsets[s], needle_offsets[s + 1]).  num_segments <= 2^24,
 *     hay_total < 2^32, needle_total < 2^32.  needle_offsets == NULL: equal needle rows of needle_total / num_segments (it must
 *     divide, else GLU_ERROR_INVALID_ARGUMENT): ragged CDFs with M samples each.
 *   - For segment s with haystack [hb, he) and needles [nb, ne), and every j in [nb, ne):
 *       out_lower[j] = the number of i in [hb, he) with enc(hay[i]) <  enc(needles[j])
 *       out_upper[j] = the number of i in [hb, he) with enc(hay[i]) <= enc(needles[j])
 *     The positions are LOCAL to the segment, in [0, he - hb]: what torch.searchsorted gives per row, what batched top-k writes
 *     and what the batched gather takes; a caller who wants global positions adds hay_offsets[s] (glu_expand_run_ptr hands it to
 *     every needle).  Either output may be NULL, not both.  Every entry of a covered needle is written; needles in front of
 *     needle_offsets[0] or at or behind needle_offsets[num_segments] are not touched (expand's rule).  A segment whose haystack is
 *     empty gives 0 for all its needles.
 *   - num_partitions == 0, num_segments == 0 or no needles: nothing is enqueued, GLU_OK, NULL arrays accepted.
 *   - MALFORMED OFFSETS (decreasing, beyond the total): a segment that ends below its begin or beyond the total is empty, on
 *     either side.  The result is unspecified positions or untouched entries; no access outside the five arrays happens.  A
 *     haystack that is not sorted gives unspecified positions in [0, he - hb].
 *   - GLU_ERROR_INVALID_ARGUMENT, each with a message that names the argument: NULL search; NULL hay or needles with a non-zero
 *     size; NULL hay_offsets; both outputs NULL; misalignment (hay and needles to the key size, the outputs and the offsets to 4
 *     bytes); a bad key type; the limits above; an output overlapping hay, needles, either offsets array or the other output; a
 *     window outside the range of the call's key width.  A refused call writes nothing.
 *   - ONE KERNEL per call, none where there are no needles.  It is load-balanced over the needles: a workgroup takes tiles of 2048
 *     4-byte or 1024 8-byte consecutive needles, finds the tile's first and last segment and each needle's own segment by bounds over
 *     needle_offsets (equal rows: a multiplication), and searches every needle in its own haystack with a trip count that follows
 *     the longest haystack among the wave's needles.  One segment with all the needles fills the device; segments without needles
 *     cost nothing.
 *   - THE WINDOW: the haystacks of the consecutive segments of a tile are one range of `hay`; where it holds at most `window` keys
 *     the workgroup copies it into LDS once and every probe of the tile goes there, otherwise the probes go to global memory.
 *     glu_sorted_search_set_batch_window: keys = 0 (never stage), 16 <= keys <= 32768 / key bytes, or
 *     GLU_SEARCH_BATCH_WINDOW_DEFAULT: the maximum of the call's key width, 8192 or 4096 keys (DESIGN.md 4.21 on what was and
 *     what was not measured).  A call checks the value against its own key width.  The window never changes a result.
 *   - No scratch and no prepare: the calls allocate nothing, only enqueue on `stream` and are capturable from the first call on a
 *     fresh object.  No atomics, no host synchronisation, nothing that waits for another workgroup; the grid follows from the
 *     needle count and the needle pointer's alignment, so a captured call replays on any contents (offsets included) and gives the
 *     same bits every time.  The calls do not touch the object's index scratch or its remembered index: a reuse_index call after a
 *     batched call still works.
 *   - glu_sorted_search_last after a batched call: path = GLU_SEARCH_PATH_BATCH, levels = 0, kernels = 0 or 1.
 *   - OUT OF SCOPE: an index per segment (a few very long rows are served by the loop of single INDEXED calls, which is ahead of
 *     probing global memory there); a per-segment key type; 64-bit positions. */
#define GLU_SEARCH_BATCH_WINDOW_DEFAULT 0xFFFFFFFFu
GLU_API glu_status glu_sorted_search_run_batch_ptr(glu_sorted_search search, const void* hay, size_t hay_count, const void* needles,
                                                   size_t needle_count, size_t num_partitions, glu_key_type key_type,
                                                   uint32_t* out_lower, uint32_t* out_upper, void* stream);
GLU_API glu_status glu_sorted_search_run_batch_offsets_ptr(glu_sorted_search search, const void* hay, size_t hay_total,
                                                           const uint32_t* hay_offsets, const void* needles, size_t needle_total,
                                                           const uint32_t* needle_offsets, size_t num_segments, glu_key_type key_type,
                                                           uint32_t* out_lower, uint32_t* out_upper, void* stream);
GLU_API glu_status glu_sorted_search_set_batch_window(glu_sorted_search search, uint32_t keys);
/* Host only, no device, pure: tile = needles per tile (2048 or 1024), tiles = ceil(needle_total / tile), the tiles of needle_total
 * needles that start on a 16-byte boundary (a needle array that starts behind one can take one tile more), window_keys_used = the
 * window in keys (window_keys: 0, a value in the range of the key width, or GLU_SEARCH_BATCH_WINDOW_DEFAULT), kernels = 0 or 1.
 * Any pointer may be NULL. */
GLU_API glu_status glu_sorted_search_plan_batch(size_t needle_total, glu_key_type key_type, uint32_t window_keys, uint32_t* tile,
                                                uint32_t* tiles, uint32_t* window_keys_used, uint32_t* kernels);

/* ---- merge (not in the reference): two sorted arrays of keys, with or without 4-byte values, into one sorted array, stable, on
 * the device and on the caller's stream.  The update of a sorted table by a sorted batch, and the step between the batched or the
 * sharded sorts and one sorted array (a merge tree is repeated calls).  It moves every pair once: 16 bytes a pair for 4-byte keys
 * with values, 24 for 8-byte keys.
 *   - out = the STABLE SORT OF THE CONCATENATION A || B BY enc(key), enc being the encoding the sort gives a key: the order
 *     glu_radix_sort_run_typed_ptr produces and glu_sorted_search_run_ptr assumes (floats by their bits: -0.0 < +0.0, the NaNs
 *     beyond the infinities, ordered by payload).  Both inputs must be sorted in that order.  Among equal keys every element of A
 *     comes before every element of B, and each side keeps its own order:
 *       A[i] lands at i + the number of j with enc(B[j]) <  enc(A[i])      (sorted search's lower bound)
 *       B[j] lands at j + the number of i with enc(A[i]) <= enc(B[j])      (its upper bound)
 *     Keys are copied bit for bit; values are uint32_t like the sort's and follow their keys.
 *   - All six glu_key_type's.  a_count + b_count <= 2^32 - 1.
 *   - a_vals, b_vals and out_vals are all NULL (keys only) or all non-NULL.  A side of count 0 is not looked at: its pointers may be
 *     NULL.
 *   - The inputs are READ ONLY.  out_keys and out_vals must not overlap any input range or each other (arrays that merely touch are
 *     fine).  Every array may start at any multiple of its element size.
 *   - Two kernels when a_count + b_count > 0, none otherwise: merge path.  The first finds, for every tile boundary of the output,
 *     how many of the outputs in front of it come from A (a binary search over both inputs, (tiles + 1) words of the object's
 *     scratch); the second merges one tile per workgroup in LDS and writes it with contiguous lanes.  No atomics, no look-back, no
 *     side stream, no host synchronisation, and no device allocation once glu_merge_prepare covered the total (else grow-only
 *     allocation inside the call: not capturable).  The kernels and their grids follow from the counts and the addresses, so a
 *     captured call (one stream, no parallel branches) replays on any contents.
 *   - An input that is NOT SORTED gives unspecified output CONTENTS; the call still writes exactly out[0 .. a_count + b_count) and
 *     never reads or writes outside the six arrays (every probe of the searches is clamped, every tile's ranges are clamped).
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument: NULL merge; a NULL key
 *     pointer of a side with elements; a mix of NULL and non-NULL value pointers; misalignment; a bad key type; the limit above; an
 *     output overlapping an input or the other output.  A refused call writes nothing.
 *   - OUT OF SCOPE: more than two inputs (a merge tree is repeated calls); an in-place merge; values wider than 4 bytes (merge
 *     an iota as the values, and fetch the wide values through the merged iota with glu_gather_run_ptr, the gather by an
 *     arbitrary permutation; it takes one source array, so A's and B's values are copied into one array first).  (A segmented
 *     merge, and a merge whose counts live on the device: the batched calls below.  Set operations on two sorted arrays:
 *     glu_set_ops_run_ptr below.) */
typedef struct glu_merge_s* glu_merge;
/* Not in the reference. */
GLU_API glu_status glu_merge_create(glu_merge* out);
/* Not in the reference. */
GLU_API glu_status glu_merge_destroy(glu_merge merge);
/* Not in the reference.  Grow-only scratch (the split table) for calls with a_count + b_count <= total_count keys of `key_type`,
 * with or without values: after it a call allocates nothing (and can be captured). */
GLU_API glu_status glu_merge_prepare(glu_merge merge, size_t total_count, glu_key_type key_type);
/* Not in the reference.  The contract above.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_merge_run_ptr(glu_merge merge, const void* a_keys, const uint32_t* a_vals, size_t a_count, const void* b_keys,
                                     const uint32_t* b_vals, size_t b_count, void* out_keys, uint32_t* out_vals, glu_key_type key_type,
                                     void* stream);
/* Not in the reference.  Host only, no device, pure: tile = outputs per workgroup (256 threads x 11 for 4-byte keys, x 7 for
 * 8-byte keys, with and without values), tiles = ceil((a_count + b_count) / tile), kernels = 2 (0 if there is nothing to merge),
 * scratch_bytes = (tiles + 1) * 4 (0 if there is nothing to merge): what prepare reserves.  Any pointer may be NULL. */
GLU_API glu_status glu_merge_plan(size_t a_count, size_t b_count, glu_key_type key_type, int with_vals, uint32_t* tile, uint32_t* tiles,
                                  uint32_t* kernels, size_t* scratch_bytes);
/* Not in the reference.  What the host enqueued in the object's last run_ptr or batched call (no device read): the tiles and the
 * kernels. */
GLU_API glu_status glu_merge_last(glu_merge merge, uint32_t* tiles, uint32_t* kernels);

/* ---- batched merge (not in the reference): the two sorted runs of every segment into one, all segments in one call.
 *   - a_offsets and b_offsets are DEVICE arrays of num_segments + 1 uint32_t words; the host never reads them.  Segment s of A is
 *     A[a_offsets[s], a_offsets[s + 1]), of B likewise.  a_total and b_total are the host-known lengths of the arrays (they may be
 *     larger than the last offsets): they bound every access and size the grids.  With oa[s] = a_offsets[s] - a_offsets[0] and
 *     ob[s] likewise, the output of segment s is out[oa[s] + ob[s] .. oa[s + 1] + ob[s + 1]) and holds what glu_merge_run_ptr
 *     writes for that segment's two runs: the output is the stable sort of all elements by (segment, enc(key), side), A first.
 *     All six glu_key_type's; values uint32_t, all three value pointers given or all NULL; keys copied bit for bit.
 *   - Entries of out_keys / out_vals at and behind oa[S] + ob[S] are not touched.  out_offsets is optional: when given, all its
 *     num_segments + 1 entries oa[s] + ob[s] are written -- the form every batched call takes, so the merged rows go straight
 *     into a batched top-k, reduce or a further batched merge.  A segment empty on one side or on both is legal, anywhere and
 *     in any number.  num_segments == 0 merges nothing and writes out_offsets[0] = 0.
 *   - num_segments == 1 with offsets {0, n_a} and {0, n_b} written by the device is the merge whose COUNTS LIVE ON THE DEVICE
 *     (the num_out of select, the set operations, key runs, top-k): no host read, capturable.
 *   - a_total + b_total <= 2^32 - 1; num_segments <= 2^24.  Every array at any multiple of its element size.  The outputs
 *     (out_keys and out_vals over a_total + b_total elements, out_offsets) overlap no input, no offsets array and not each other.
 *   - NOT TRUSTED: inputs that are not sorted inside a segment, offsets that decrease or exceed their total give unspecified
 *     CONTENTS.  Nothing outside [0, a_total), [0, b_total), out[0, a_total + b_total) and the num_segments + 1 offset words is
 *     read or written, no output is written twice, and every out_offsets entry written is at most a_total + b_total (every offset
 *     is pinned into its side before use; tests/test_merge_batch_path.py walks the arithmetic on the host).
 *   - One merge path over all of A and B in the order (segment, enc(key)): a partition kernel (one thread per tile boundary:
 *     the boundary's segment by a bound over the offsets, then the split inside that segment; it also writes out_offsets) and a
 *     tile kernel (one workgroup per tile of the single call's size; a tile inside one segment runs the single merge's body, a
 *     tile over several segments merges by (segment, key) with a segment word beside every staged key).  Balanced over the
 *     outputs: one long segment fills the device, empty segments cost no tile anything.  No atomics, no look-back, no host
 *     synchronisation; the same call gives the same bits; after glu_merge_prepare_batch no allocation, and one captured call
 *     replays on other keys AND other offsets of the same capacity (the grids follow from a_total, b_total, num_segments).
 *   - GLU_ERROR_INVALID_ARGUMENT as for the single call, and for num_segments > 2^24 or a NULL offsets array.
 *   - OUT OF SCOPE: pairs of adjacent segments of one array; more than two inputs; values wider than 4 bytes; a key type per
 *     segment; 64-bit offsets; an in-place merge.  (Batched set operations: glu_set_ops_run_batch_offsets_ptr below.) */
/* Not in the reference.  Grow-only scratch for batched calls with a_total + b_total <= total_count keys of `key_type`. */
GLU_API glu_status glu_merge_prepare_batch(glu_merge merge, size_t total_count, glu_key_type key_type);
/* Not in the reference.  The contract above.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_merge_run_batch_offsets_ptr(glu_merge merge, const void* a_keys, const uint32_t* a_vals, const uint32_t* a_offsets,
                                                   size_t a_total, const void* b_keys, const uint32_t* b_vals, const uint32_t* b_offsets,
                                                   size_t b_total, size_t num_segments, void* out_keys, uint32_t* out_vals,
                                                   uint32_t* out_offsets, glu_key_type key_type, void* stream);
/* Not in the reference.  Equal partitions: a_offsets[s] = s * a_len, b_offsets[s] = s * b_len (a_total = num_segments * a_len,
 * b_total likewise); either length may be 0. */
GLU_API glu_status glu_merge_run_batch_ptr(glu_merge merge, const void* a_keys, const uint32_t* a_vals, size_t a_len, const void* b_keys,
                                           const uint32_t* b_vals, size_t b_len, size_t num_segments, void* out_keys, uint32_t* out_vals,
                                           uint32_t* out_offsets, glu_key_type key_type, void* stream);
/* Not in the reference.  Host only, no device, pure: tile as glu_merge_plan, tiles = ceil(total_count / tile) with total_count =
 * a_total + b_total, kernels = 2 (1 where total_count is 0: the partition kernel writes out_offsets; 0 where num_segments is 0),
 * scratch_bytes = (tiles + 1) * 8: what prepare_batch reserves.  Any pointer may be NULL. */
GLU_API glu_status glu_merge_plan_batch(size_t total_count, size_t num_segments, glu_key_type key_type, int with_vals, uint32_t* tile,
                                        uint32_t* tiles, uint32_t* kernels, size_t* scratch_bytes);

/* ---- set operations (not in the reference): union, intersection, difference and symmetric difference of two sorted arrays of
 * keys, with or without 4-byte values, on the device and on the caller's stream: std::set_union / set_intersection /
 * set_difference / set_symmetric_difference, with their multiset semantics.  The result and its length stay on the device.
 *   - ORDER AND EQUALITY are those of enc(key), enc being the encoding the sort gives a key (merge's order above).  Two keys are
 *     equal iff their bits are: -0.0 and +0.0 are different keys, a NaN equals only the NaN with the same bits (the family's choice
 *     for sort, merge, sorted search and top-k; not select's IEEE comparison).  Both inputs must be sorted in that order.
 *   - For A[i] with key k: its rank among A's copies of k is rA(i) = i - lower_bound(A, k); B holds mB(k) = upper_bound(B, k) -
 *     lower_bound(B, k) copies; A[i] is MATCHED iff rA(i) < mB(k).  B[j] is matched iff rB(j) < mA(k), the same the other way round.
 *       GLU_SET_UNION                 every element of A, and the unmatched elements of B
 *       GLU_SET_INTERSECTION          the matched elements of A (A's keys and values, never B's)
 *       GLU_SET_DIFFERENCE            the unmatched elements of A
 *       GLU_SET_SYMMETRIC_DIFFERENCE  the unmatched elements of A and the unmatched elements of B
 *     A key m times in A and n times in B is max(m, n) / min(m, n) / max(m - n, 0) / |m - n| times in the output.  The output is the
 *     kept elements in MERGE'S ORDER: A first among equal keys, each side in its own order.  Keys are copied bit for bit; values are
 *     uint32_t and follow their keys.
 *   - All six glu_key_type's.  a_count + b_count <= 2^32 - 1; max_out < 2^32.
 *   - *num_out (uint32_t, on the device, required) always receives the number S of kept elements, also when S > max_out, and 0 when
 *     both counts are 0.  out_keys[0 .. min(S, max_out)) and out_vals[0 .. min(S, max_out)) are written; entries behind them are not
 *     touched (select's rule).  With out_keys NULL or max_out 0 the call ONLY COUNTS; out_vals must then be NULL too.
 *   - VALUES: a_vals and out_vals are both NULL (keys only) or both non-NULL when a_count > 0.  b_vals is required exactly where
 *     elements of B can be written: union or symmetric difference, with values, b_count > 0; intersection and difference ignore it
 *     (it may be NULL).  A side of count 0 is not looked at: its pointers may be NULL.
 *   - The inputs are READ ONLY.  With bound = the most outputs the operation can have -- a_count + b_count for union and symmetric
 *     difference, a_count for difference, min(a_count, b_count) for intersection -- the first min(bound, max_out) entries of
 *     out_keys and out_vals, and num_out, must not overlap any input range or each other (arrays that merely touch are fine).
 *     Every array may start at any multiple of its element size.
 *   - Four kernels when a_count + b_count > 0 (three when the call only counts), on merge's tiles: the bounds of every tile
 *     boundary (merge's split, and where the copies of the first key behind it start in A and in B; 12 bytes a boundary of the
 *     object's scratch), the kept elements of every tile counted in LDS, the counts scanned by one workgroup (which writes
 *     *num_out), the kept elements of every tile written at their ranks by contiguous lanes.  With both counts 0 the scan alone
 *     runs and writes 0.  No atomics, no look-back, no side stream, no host synchronisation, nothing in arrival order: the same
 *     call gives the same bits every time.  No device allocation once glu_set_ops_prepare covered the total (else grow-only
 *     allocation inside the call: not capturable).  The kernels and their grids follow from the counts and the addresses, never
 *     from the data, so a captured call (one stream, no parallel branches) replays on any contents.
 *   - An input that is NOT SORTED gives unspecified output contents and an unspecified *num_out <= bound; the call still never reads
 *     or writes outside the arrays and writes nothing at or behind out[min(bound, max_out)].
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument: NULL set_ops; a NULL key
 *     pointer of a side with elements; NULL num_out; a_vals without out_vals or the reverse; a required b_vals missing; out_vals in
 *     a call that only counts; an op or a key type outside its list; misalignment; the limits above; an output overlapping an
 *     input, another output or num_out.  A refused call writes nothing.
 *   - OUT OF SCOPE: more than two inputs; set semantics that drop duplicates within one input (run glu_key_runs_run_ptr first: its
 *     unique keys are a set); values wider than 4 bytes (carry an iota and gather, as for merge); the indices of the partners in B.
 *     (Counts that live on the device: the batched call below with num_segments == 1.) */
typedef enum
{
    GLU_SET_UNION = 0,
    GLU_SET_INTERSECTION = 1,
    GLU_SET_DIFFERENCE = 2,
    GLU_SET_SYMMETRIC_DIFFERENCE = 3,
    GLU_SET_OP_COUNT_
} glu_set_op;
typedef struct glu_set_ops_s* glu_set_ops;
/* Not in the reference. */
GLU_API glu_status glu_set_ops_create(glu_set_ops* out);
/* Not in the reference. */
GLU_API glu_status glu_set_ops_destroy(glu_set_ops set_ops);
/* Not in the reference.  Grow-only scratch (the bounds and the tile counts) for calls with a_count + b_count <= total_count keys of
 * `key_type`: after it a call allocates nothing (and can be captured). */
GLU_API glu_status glu_set_ops_prepare(glu_set_ops set_ops, size_t total_count, glu_key_type key_type);
/* Not in the reference.  The contract above; `op` is a glu_set_op.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_set_ops_run_ptr(glu_set_ops set_ops, int op, const void* a_keys, const uint32_t* a_vals, size_t a_count,
                                       const void* b_keys, const uint32_t* b_vals, size_t b_count, void* out_keys, uint32_t* out_vals,
                                       size_t max_out, uint32_t* num_out, glu_key_type key_type, void* stream);
/* Not in the reference.  Host only, no device, pure: tile = merge's (256 threads x 11 for 4-byte keys, x 7 for 8-byte keys), tiles =
 * ceil((a_count + b_count) / tile), kernels = 4 with_arrays (out_keys given and max_out > 0), 3 for a call that only counts, 1 (the
 * scan, which writes *num_out = 0) if both counts are 0; scratch_bytes = (tiles + 1) * 12 + tiles * 4 (0 if both counts are 0): what
 * prepare reserves.  Any pointer may be NULL. */
GLU_API glu_status glu_set_ops_plan(size_t a_count, size_t b_count, glu_key_type key_type, int with_arrays, uint32_t* tile,
                                    uint32_t* tiles, uint32_t* kernels, size_t* scratch_bytes);
/* Not in the reference.  What the host enqueued in the object's last run_ptr or batched call (no device read): the tiles and the
 * kernels. */
GLU_API glu_status glu_set_ops_last(glu_set_ops set_ops, uint32_t* tiles, uint32_t* kernels);

/* ---- batched set operations (not in the reference): the set operation of the two sorted runs of every segment, all segments in
 * one call.  The contract is the batched merge's for the segments and the single set operation's for the result.
 *   - SEGMENTS.  a_offsets and b_offsets are DEVICE arrays of num_segments + 1 uint32_t words; the host never reads them.  Segment s
 *     of A is A[a_offsets[s], a_offsets[s + 1]), of B likewise.  a_total and b_total are the host-known lengths of the arrays (they
 *     may be larger than the last offsets): they bound every access and size every grid.  Every offset is pinned into its side
 *     before use, exactly as the batched merge pins it.  num_segments <= 2^24; a_total + b_total <= 2^32 - 1; max_out < 2^32.
 *   - RESULT.  Segment s of the result is what glu_set_ops_run_ptr(op, A_s, B_s) writes: the same multiset semantics, all six
 *     glu_key_type's, equality on bits, A first among equal keys, the intersection holding A's keys and values.  The segments'
 *     results lie back to back from out[0], in segment order.  Keys NEVER MATCH ACROSS SEGMENTS: a key that ends A_s and begins
 *     B_{s + 1} is two different elements.  b_vals is read only for the union and the symmetric difference (with values, b_total
 *     > 0: required there, ignored otherwise); a_vals and out_vals are both NULL or both non-NULL when a_total > 0.
 *   - *num_out (uint32_t, on the device, required) receives the true total S of kept elements, also beyond max_out.
 *     out[0 .. min(S, max_out)) is written; nothing behind it is touched.  out_keys NULL or max_out 0 ONLY COUNTS; out_vals must
 *     then be NULL.
 *   - out_offsets is optional.  When given, all its num_segments + 1 entries are written: entry s = min(max_out, the kept elements
 *     of the segments < s) -- the batched select's clamp: the entries describe what was written, and the next batched call over
 *     them stays in bounds.  An emptied segment stays an empty segment.  In a call that ONLY COUNTS the entries are NOT clamped by
 *     max_out (there is no array to stay inside): they are the running sums of the per-segment cardinalities, held to the bound
 *     below alone.
 *   - num_segments == 0 writes *num_out = 0 and out_offsets[0] = 0.  num_segments == 1 with both pairs of offset words written on
 *     the device ({0, n_a} and {0, n_b}, n_a being the num_out of an earlier call) is the set operation whose COUNTS LIVE ON THE
 *     DEVICE: a chain of set operations without a host read.
 *   - BOUND.  bound = the most outputs of the operation over the host-known totals: a_total + b_total for union and symmetric
 *     difference, a_total for difference, min(a_total, b_total) for intersection.  The first min(bound, max_out) entries of out_keys
 *     and out_vals, the num_segments + 1 entries of out_offsets and num_out must overlap no input, no offsets array and not each
 *     other.  Every array at any multiple of its element size.  The inputs and the offsets are READ ONLY.
 *   - Five kernels at most, on the caller's stream alone: the bounds of every tile boundary (the batched merge's segment and split,
 *     and where the first key's copies start inside that segment: 16 bytes a boundary), the kept elements of every tile decided and
 *     counted in LDS (each thread leaves one word: its decisions as bits and its rank in the tile), the counts scanned (*num_out),
 *     one thread per out_offsets entry (where given), and the kept elements of every tile written at their ranks (where something
 *     can be written; it takes the count kernel's decisions and does not decide twice).  No atomics, no side stream, no host
 *     synchronisation, nothing in arrival order: the same bits every time.  After glu_set_ops_prepare_batch no allocation, and one
 *     captured call (one stream, no parallel branches) replays on other keys AND other offsets of the same capacity.
 *   - NOT TRUSTED: runs that are not sorted, offsets that decrease or exceed their totals give unspecified CONTENTS; still *num_out
 *     <= bound, every out_offsets entry <= min(bound, max_out) (<= bound in a call that only counts), never an access outside the
 *     arrays and never a write at or behind out[min(bound, max_out)] (tests/test_set_ops_batch_path.py walks the arithmetic on the
 *     host).
 *   - GLU_ERROR_INVALID_ARGUMENT as for glu_set_ops_run_ptr and the batched merge, each with a message that names the argument:
 *     NULL set_ops; a NULL key pointer of a side with elements; NULL num_out; a_vals without out_vals or the reverse; a required
 *     b_vals missing; out_vals in a call that only counts; an op or a key type outside its list; misalignment; the limits above;
 *     num_segments > 2^24; a NULL offsets array; an output overlapping an input, an offsets array or another output.  A refused
 *     call writes nothing.
 *   - OUT OF SCOPE: more than two inputs; values wider than 4 bytes; a key type or an operation per segment; 64-bit offsets; the
 *     indices of the partners in B. */
/* Not in the reference.  Grow-only scratch for batched calls with a_total + b_total <= total_count keys of `key_type` in up to
 * num_segments segments, with or without arrays and out_offsets: after it a batched call allocates nothing. */
GLU_API glu_status glu_set_ops_prepare_batch(glu_set_ops set_ops, size_t total_count, size_t num_segments, glu_key_type key_type);
/* Not in the reference.  The contract above; `op` is a glu_set_op.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_set_ops_run_batch_offsets_ptr(glu_set_ops set_ops, int op, const void* a_keys, const uint32_t* a_vals,
                                                     const uint32_t* a_offsets, size_t a_total, const void* b_keys, const uint32_t* b_vals,
                                                     const uint32_t* b_offsets, size_t b_total, size_t num_segments, void* out_keys,
                                                     uint32_t* out_vals, size_t max_out, uint32_t* out_offsets, uint32_t* num_out,
                                                     glu_key_type key_type, void* stream);
/* Not in the reference.  Equal partitions: a_offsets[s] = s * a_len, b_offsets[s] = s * b_len (a_total = num_segments * a_len,
 * b_total likewise); either length may be 0. */
GLU_API glu_status glu_set_ops_run_batch_ptr(glu_set_ops set_ops, int op, const void* a_keys, const uint32_t* a_vals, size_t a_len,
                                             const void* b_keys, const uint32_t* b_vals, size_t b_len, size_t num_segments, void* out_keys,
                                             uint32_t* out_vals, size_t max_out, uint32_t* out_offsets, uint32_t* num_out,
                                             glu_key_type key_type, void* stream);
/* Not in the reference.  Host only, no device, pure: tile as glu_set_ops_plan, tiles = ceil((a_total + b_total) / tile); kernels = 3
 * (bounds, count, scan) + 1 with_offsets (out_offsets given) + 1 with_arrays (out_keys given and max_out > 0); with no keys
 * 1 + with_offsets (the scan writes *num_out = 0, the offsets kernel its zeros); with no segments 1 (the scan).  scratch_bytes =
 * (tiles + 1) * 16 + tiles * 4, and tiles * 1024 more (one word per thread and tile: the count kernel's decisions, read by the
 * offsets and the write kernel) unless the call only counts without out_offsets; 0 with no keys.  What prepare_batch reserves is
 * the plan with arrays and offsets.  Any pointer may be NULL. */
GLU_API glu_status glu_set_ops_plan_batch(size_t a_total, size_t b_total, size_t num_segments, glu_key_type key_type, int with_arrays,
                                          int with_offsets, uint32_t* tile, uint32_t* tiles, uint32_t* kernels, size_t* scratch_bytes);

/* ---- histogram (not in the reference): how many samples fall into each bin, over even bins (numpy.histogram with a range,
 * torch.histc, torch.bincount) or over sorted bin edges (numpy.histogram with edges), on the device and on the caller's stream.
 * One read of the samples, 4 or 8 bytes a sample; nothing per sample is written.
 *   - TYPES.  Samples are the six glu_key_type's.  Counts are uint32_t out_counts[bins] on the device; every entry is written.
 *   - ARGUMENTS.  count < 2^32.  `samples` is READ ONLY and aligned to its element size; out_counts is aligned to 4 bytes.
 *     accumulate != 0 adds the call's counts to what out_counts holds, modulo 2^32; with accumulate == 0 the call overwrites and the
 *     prior contents do not matter.  count == 0 is legal with NULL samples: all zeros, or nothing touched under accumulate.
 *   - EVEN BINS, glu_histogram_run_even_ptr.  `lo` and `hi` are HOST pointers to one value each of the sample's type, read during
 *     the call and passed to the kernels by value (as select passes its threshold), so the call stays capturable.  A sample counts
 *     iff lo <= x < hi.  1 <= bins <= 2^24.
 *       UINT32, INT32: W = ((int64) hi - lo) / bins must be a whole number >= 1, else the call is an invalid argument (uneven or
 *         fractional widths: pass edges).  bin = floor((x - lo) / W) EXACTLY, for every x in range: the kernels multiply by
 *         ceil(2^64 / W) and keep the top 64 bits of the 96-bit product, which is the quotient for every 32-bit dividend
 *         (histogram_bins.hpp has the proof), not a reciprocal that can be one off beside a multiple of W.  lo = 0, hi = bins is
 *         bincount.
 *       FLOAT32, FLOAT64: lo and hi finite, lo < hi, hi - lo and bins / (hi - lo) finite in double.  With d = (double) x, a NaN is
 *         dropped and d must satisfy lo <= d < hi; bin = min((uint32) ((d - lo) * scale), bins - 1) with
 *         scale = (double) bins / ((double) hi - (double) lo) computed once on the host: one subtraction and one multiplication in
 *         IEEE double, nothing that could contract into an FMA, no fast-math, so numpy restates it bit for bit.
 *       UINT64, INT64: an invalid argument here (their even bins are not exact in double): pass edges.
 *   - SORTED EDGES, glu_histogram_run_edges_ptr.  `edges` is a DEVICE array of bins + 1 values of the sample's type,
 *     non-decreasing.  1 <= bins <= 8192.  bin = (the number of e in edges with e <= x) - 1; the sample counts iff
 *     0 <= bin < bins, that is iff edges[0] <= x < edges[bins].  Floats compare as IEEE VALUES, as in select and in numpy:
 *     -0.0 == +0.0, and a NaN sample fails every comparison and is dropped.  This is deliberately NOT the order on bits of the sort
 *     and of sorted search (glu_sorted_search_run_ptr): a bin is a range of values, not a position in a sorted array.  Repeated
 *     edges make empty bins.  Edges that hold a NaN or are not non-decreasing give unspecified counts and never an access outside
 *     the arrays: the search is clamped and the bin is checked against `bins` before it is used.  More than 8192 uneven bins are
 *     OUT OF SCOPE; the way round: sort the samples, search the edges in them (glu_sorted_search_run_ptr), difference the bounds.
 *   - TWO PATHS, chosen from `bins`, never from the data (glu_histogram_plan states them).
 *       GLU_HISTOGRAM_PATH_LDS, bins <= 8192, both modes: kernel 1 runs groups = min(tiles, groups_max) workgroups, each with a
 *         table of `bins` counters in LDS (edges mode: and the edges beside it), walks its tiles adding with LDS atomics, and stores
 *         its table as row g of partial[groups][bins] in the object's scratch; kernel 2 sums the columns:
 *         out[b] = (accumulate ? out[b] : 0) + the sum over g of partial[g][b].  Kernel 2 always runs unless count == 0 and
 *         accumulate; with count == 0 it runs over zero rows, which writes the zeros.  No global atomics, no clearing pass.
 *       GLU_HISTOGRAM_PATH_GLOBAL, bins > 8192, even bins only: one kernel clears out_counts (skipped under accumulate), one adds
 *         with device-scope atomics straight into out_counts.  No scratch.
 *     Skew: a wave whose counted samples of a tile all fall into one bin issues ONE add of their number, and holds that add back
 *     while its following tiles fall into the same bin (one add per wave and call for input that is one value); a thread adds each
 *     run of equal bins among its own samples once.  On the LDS path skew costs nothing.  On the GLOBAL path hot bins that meet in
 *     neither rule serialise on their addresses (DESIGN.md 4.15 has the figures): skewed data wants at most 8192 bins.
 *   - The calls only enqueue on `stream`: no host synchronisation, no side stream, no read-back, and no device allocation once
 *     glu_histogram_prepare covered the counts (else grow-only allocation inside the call: not capturable).  Grids follow from the
 *     counts and the addresses, never from the data: a captured call (one stream, no parallel branches) replays on any contents,
 *     of the samples and of the device edges.
 *   - Counts are integers, so the atomics do not make a result depend on the order of arrival: THE SAME INPUT GIVES THE SAME BITS
 *     EVERY TIME.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument, and nothing written:
 *     a NULL object; NULL samples with count > 0; NULL out_counts, lo, hi or edges; misalignment; a bad key type; the limits and
 *     rules above; out_counts overlapping the samples or the edges (arrays that merely touch are fine).
 *   - OUT OF SCOPE: weights, several channels, 2-D, 64-bit counts, a right-closed last bin. */
typedef struct glu_histogram_s* glu_histogram;
enum
{
    GLU_HISTOGRAM_EVEN = 0,
    GLU_HISTOGRAM_EDGES = 1
};
enum
{
    GLU_HISTOGRAM_PATH_LDS = 0,
    GLU_HISTOGRAM_PATH_GLOBAL = 1,
    GLU_HISTOGRAM_PATH_BATCH = 2 /* a batched call (below) */
};
/* Not in the reference. */
GLU_API glu_status glu_histogram_create(glu_histogram* out);
/* Not in the reference. */
GLU_API glu_status glu_histogram_destroy(glu_histogram histogram);
/* Not in the reference.  Grow-only scratch (the partial rows) for calls with up to `count` samples and `bins` bins, of any key type
 * and either mode: after it such a call allocates nothing (and can be captured). */
GLU_API glu_status glu_histogram_prepare(glu_histogram histogram, size_t count, size_t bins);
/* Not in the reference.  The contract above, even bins.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_histogram_run_even_ptr(glu_histogram histogram, const void* samples, size_t count, glu_key_type key_type,
                                              const void* lo, const void* hi, size_t bins, uint32_t* out_counts, int accumulate, void* stream);
/* Not in the reference.  The contract above, sorted edges.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_histogram_run_edges_ptr(glu_histogram histogram, const void* samples, size_t count, glu_key_type key_type,
                                               const void* edges, size_t bins, uint32_t* out_counts, int accumulate, void* stream);
/* Not in the reference.  Host only, no device, pure.  mode = GLU_HISTOGRAM_EVEN or _EDGES.  path = _PATH_LDS where bins <= 8192,
 * else _PATH_GLOBAL.  threads = the workgroup of the counting kernel: 256 for even bins, 512 for edges of 4-byte and 1024 for edges
 * of 8-byte samples (16 waves to the CU beside 32, 64 and 96 KiB of LDS).  tile = threads x 4 packs of 16 bytes, in samples;
 * groups = min(ceil(count / tile), groups_max), groups_max = 1024, 512, 256 in the same order; kernels = what a call with
 * accumulate == 0 enqueues: 2, or 1 where count == 0 (under accumulate: one fewer on the GLOBAL path and where count == 0);
 * scratch_bytes = groups * bins * 4 on the LDS path, 0 on the GLOBAL path.  Any pointer may be NULL. */
GLU_API glu_status glu_histogram_plan(size_t count, size_t bins, glu_key_type key_type, int mode, uint32_t* path, uint32_t* threads,
                                      uint32_t* tile, uint32_t* groups, uint32_t* kernels, size_t* scratch_bytes);
/* Not in the reference.  What the host enqueued in the object's last run (no device read): the path, the workgroups of the counting
 * kernel and the number of kernels. */
GLU_API glu_status glu_histogram_last(glu_histogram histogram, uint32_t* path, uint32_t* groups, uint32_t* kernels);

/* ---- batched histogram (not in the reference): the counts of every segment of an array in one call, on the existing object.
 * out_counts[s * bins + b] = the samples of segment s that fall into bin b; a sample gets its bin by EXACTLY the rule of the single
 * call above.  Per-group distributions after sort -> key runs, a per-row bincount, the per-node feature histograms of tree learners.
 *   - EVEN BINS (glu_histogram_run_batch_even_ptr, _batch_offsets_even_ptr): the same lo, hi and bins for all segments; the types and
 *     argument rules of glu_histogram_run_even_ptr, integers exact and floats in double.  EDGES (_batch_edges_ptr,
 *     _batch_offsets_edges_ptr): ONE device array of bins + 1 edges shared by all segments, all six key types, compared as IEEE values.
 *   - SEGMENTS.  Equal partitions: segment s is [s * count, (s + 1) * count).  Device offsets: [offsets[s], offsets[s + 1]);
 *     `offsets` is a DEVICE array of num_segments + 1 uint32, non-decreasing, as glu_key_runs_run_ptr writes it; the host never reads
 *     it.  A segment that ends below its begin or beyond `total` is empty to every kernel.
 *   - LIMITS.  1 <= bins <= 8192 in both modes (every table is kept in LDS; there is no batched GLOBAL path).  The total
 *     (count * num_partitions, or `total`) is below 2^32; num_segments <= 2^24.  Rows are indexed with 64 bits.
 *   - EVERY entry of the num_segments * bins counts is written; an empty segment gives a row of zeros.  accumulate != 0 adds the
 *     call's counts modulo 2^32, and the row of an empty segment is then not touched.  num_segments == 0 does nothing.  NULL arrays
 *     are accepted where nothing would be read or written (samples of an empty batch, everything where num_segments == 0).
 *   - `samples`, `edges` and `offsets` are only read; nothing outside out_counts[0 .. num_segments * bins) is written.
 *   - MALFORMED OFFSETS (decreasing, overlapping beyond `total`, out of range): the call stays in bounds: it reads nothing outside
 *     [0, total) of the samples and writes nothing outside out_counts; the contents of out_counts are then unspecified.  As in the
 *     batched reduce: the segments that found no room in the lists (overlapping segments can ask for more list entries or chunks than
 *     an array of `total` samples has) get no result; the rows of the others are right.
 *   - THREE CLASSES by the length of a segment (glu_histogram_plan_batch states the limits).  Up to wave_limit samples and
 *     bins <= 2048: a wave per segment with a table of its own in LDS, four waves to the workgroup.  Up to block_limit: a workgroup
 *     per segment with the table (and the staged edges) of the single call.  Longer: the segment is cut into chunks, a workgroup per
 *     (segment, chunk) writes its table as a row of partials in the object's scratch, and a sum kernel adds every long segment's rows:
 *     out = (accumulate ? out : 0) + their sum.  No global atomics on counts anywhere; skew costs nothing.
 *   - LAUNCHES.  Device offsets: a memset of the list counts, a binning kernel (a lane per segment; it also zeroes the rows of the
 *     empty segments) and at most four more kernels, whatever the data hold.  Equal partitions: the host picks the class: one or two
 *     kernels, or only the zeroing where count == 0 (nothing at all under accumulate).
 *   - The call only enqueues on `stream`: no host synchronisation, no read-back, no side stream, and no device allocation once
 *     glu_histogram_prepare_batch covered the sizes (else grow-only allocation inside the call: not capturable).  Grids follow from
 *     the counts the host passes, never from the data: a captured call replays on other samples, offsets of the same shape and edges.
 *     THE SAME INPUT GIVES THE SAME BITS EVERY TIME.
 *   - GLU_ERROR_INVALID_ARGUMENT with a message that names the argument, and nothing written, for what the single call refuses and
 *     for: bins > 8192; num_segments > 2^24; a total of 2^32 or more; out_counts overlapping the samples, the edges or the offsets;
 *     64-bit integer samples with even bins; a NULL or misaligned offsets array.
 *   - glu_histogram_last then reports GLU_HISTOGRAM_PATH_BATCH, groups 0 and the number of kernels enqueued.
 *   - OUT OF SCOPE: per-segment lo, hi or edges; more than 8192 bins per segment; weights and 64-bit counts. */
/* Not in the reference.  The contract above, even bins over equal partitions.  Enqueues on `stream` (NULL: the library's queue). */
GLU_API glu_status glu_histogram_run_batch_even_ptr(glu_histogram histogram, const void* samples, size_t count, size_t num_partitions,
                                                    glu_key_type key_type, const void* lo, const void* hi, size_t bins, uint32_t* out_counts,
                                                    int accumulate, void* stream);
/* Not in the reference.  The contract above, even bins over device offsets. */
GLU_API glu_status glu_histogram_run_batch_offsets_even_ptr(glu_histogram histogram, const void* samples, size_t total, const uint32_t* offsets,
                                                            size_t num_segments, glu_key_type key_type, const void* lo, const void* hi, size_t bins,
                                                            uint32_t* out_counts, int accumulate, void* stream);
/* Not in the reference.  The contract above, sorted edges over equal partitions. */
GLU_API glu_status glu_histogram_run_batch_edges_ptr(glu_histogram histogram, const void* samples, size_t count, size_t num_partitions,
                                                     glu_key_type key_type, const void* edges, size_t bins, uint32_t* out_counts, int accumulate,
                                                     void* stream);
/* Not in the reference.  The contract above, sorted edges over device offsets. */
GLU_API glu_status glu_histogram_run_batch_offsets_edges_ptr(glu_histogram histogram, const void* samples, size_t total, const uint32_t* offsets,
                                                             size_t num_segments, glu_key_type key_type, const void* edges, size_t bins,
                                                             uint32_t* out_counts, int accumulate, void* stream);
/* Not in the reference.  Grow-only scratch (the segment lists and the partial rows of the long segments) for batched calls of up to
 * `total` samples in up to `num_segments` segments over `bins` bins, of any key type, mode and form: after it such a call allocates
 * nothing (and can be captured).  The partial rows take at most total / 8 bytes. */
GLU_API glu_status glu_histogram_prepare_batch(glu_histogram histogram, size_t total, size_t num_segments, size_t bins);
/* Not in the reference.  Host only, no device, pure: what one segment of `count` samples does in a batched call.  path = 0 (empty),
 * 1 (wave class), 2 (block class) or 3 (long class); workgroups = 0, 1, 1 or the chunks of the segment; class_limits[0] = wave_limit
 * = 8 KiB of samples, or 0 where bins > 2048; class_limits[1] = block_limit = chunk; chunk = max(512 KiB of samples, 64 samples per
 * bin); scratch_bytes_per_chunk = bins * 4.  Any pointer may be NULL. */
GLU_API glu_status glu_histogram_plan_batch(size_t count, size_t bins, glu_key_type key_type, int mode, uint32_t* path, uint32_t* workgroups,
                                            uint32_t* class_limits, uint32_t* chunk, size_t* scratch_bytes_per_chunk);
/* Not in the reference.  Segments per class of the object's last batched call: the host's own numbers for equal partitions, else the
 * counts the binning kernel left on the device (synchronise the call's stream first; this call reads them back). */
GLU_API glu_status glu_histogram_read_batch(glu_histogram histogram, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments);

/* ---- expand (not in the reference): from the offsets of segments back to the elements: for every element the segment that holds
 * it, its rank inside that segment and the segment's item, on the device and on the caller's stream.  The inverse of key runs
 * (glu_key_runs_run_ptr is a run-length encoder, this is the decoder), numpy.repeat / torch.repeat_interleave with device-resident
 * counts, the broadcast of a per-segment result (a sum of glu_reduce_run_batch_offsets_ptr) onto the segment's elements, and the
 * (needle, match) pairs of a join from glu_sorted_search_run_ptr's ranges.  It reads the offsets once and writes 4 bytes (an item:
 * item_bytes) per element and requested output.
 *   - `offsets` is the batched family's array: num_segments + 1 uint32_t on the device, non-decreasing, never read by the host.
 *     `total` is the host-known length of the output arrays (what `count` is to the batched calls).
 *   - For every j in [0, total): c(j) = the number of r in [0, num_segments] with offsets[r] <= j.  j is COVERED iff
 *     1 <= c(j) <= num_segments, that is iff offsets[0] <= j < offsets[num_segments]; then s(j) = c(j) - 1, which is
 *     numpy.searchsorted(offsets, j, side="right") - 1.  Empty segments, anywhere and in any number, are skipped by this rule.
 *       out_segments[j] = s(j)
 *       out_ranks[j]    = j - offsets[s(j)]
 *       out_items[j]    = items[s(j)], copied bit for bit; item_bytes is 4, 8, 16 or 32 (select's sizes), `items` holds
 *                         num_segments of them
 *     Each output is optional (NULL skips it); items and out_items are both NULL or both given (item_bytes is ignored without).
 *   - POSITIONS THAT ARE NOT COVERED ARE NOT TOUCHED (the batched family's rule).  Nothing at or behind `total` is written even
 *     where offsets[num_segments] > total: the positions below total are written, the rest is dropped, and the caller finds the
 *     true total in offsets[num_segments] (there is no count output).
 *   - The counts form has no entry point: write the counts to counts[0 .. num_segments), any value behind them, and run
 *     glu_scan_run_batch_offsets_ptr in place over the num_segments + 1 words as ONE segment; the exclusive sums are the offsets.
 *   - Offsets that decrease or go beyond `total` give unspecified CONTENTS of [0, total) of the outputs, and never a write outside
 *     [0, total) of the three outputs nor a read outside offsets[0 .. num_segments] and items[0 .. num_segments): every tile's
 *     ranges are clamped, and the segment index of a gather is tested against num_segments, not trusted.
 *   - total == 0 or num_segments == 0: nothing is enqueued, GLU_OK, and no array is looked at (all may be NULL).  With all three
 *     outputs NULL nothing is enqueued either.
 *   - num_segments <= 2^24, total < 2^32, total + num_segments + 1 <= 2^32 - 1.  offsets, out_segments and out_ranks are aligned to
 *     4 bytes, items and out_items to min(item_bytes, 16).  `offsets` and `items` are READ ONLY; no output may overlap them or
 *     another output (arrays that merely touch are fine).
 *   - Two kernels: a load-balancing search, which is merge path between the offsets and the positions 0 .. total - 1 with the
 *     offsets first on ties.  The first finds, for every tile boundary of that MERGED sequence of num_segments + 1 + total items,
 *     how many offsets lie in front of it ((tiles + 1) words of the object's scratch); the second takes one tile per workgroup:
 *     its offsets go to LDS, each marks the position it equals, a max-scan of the marks gives every position its segment, and the
 *     outputs leave in whole 16-byte packs by contiguous lanes.  A tile holds at most `tile` offsets AND outputs together, so
 *     millions of empty segments become tiles that write nothing, not one workgroup's loop.  No atomics, no look-back, no side
 *     stream, no host synchronisation, no read-back, and no device allocation once glu_expand_prepare covered the sizes (else
 *     grow-only allocation inside the call: not capturable).  The kernels and their grids follow from total, num_segments and the
 *     addresses, never from the data: a captured call (one stream, no parallel branches) replays on any offsets.  THE SAME INPUT
 *     GIVES THE SAME BITS EVERY TIME.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument: a NULL object; NULL
 *     offsets with work to do; only one of items and out_items; a bad item_bytes; misalignment; the limits above; an output
 *     overlapping offsets, items or another output.  A refused call writes nothing.
 *   - OUT OF SCOPE: a counts-form entry point (the recipe above); items wider than 32 bytes; a gather by an arbitrary permutation (that is
 *     glu_gather_run_ptr);
 *     64-bit offsets.  (A segmented select that rewrites offsets is glu_select_run_batch_offsets_ptr.) */
typedef struct glu_expand_s* glu_expand;
/* Not in the reference. */
GLU_API glu_status glu_expand_create(glu_expand* out);
/* Not in the reference. */
GLU_API glu_status glu_expand_destroy(glu_expand expand);
/* Not in the reference.  Grow-only scratch (the split table) for calls of up to `total` elements and `num_segments` segments: after
 * it such a call allocates nothing (and can be captured). */
GLU_API glu_status glu_expand_prepare(glu_expand expand, size_t total, size_t num_segments);
/* Not in the reference.  The contract above.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_expand_run_ptr(glu_expand expand, const uint32_t* offsets, size_t num_segments, size_t total, const void* items,
                                      uint32_t item_bytes, void* out_items, uint32_t* out_segments, uint32_t* out_ranks, void* stream);
/* Not in the reference.  Host only, no device, pure: tile = merged items (offsets and outputs together) per workgroup, 256 threads
 * x 11; tiles = ceil((num_segments + 1 + total) / tile); kernels = 2; scratch_bytes = (tiles + 1) * 4: what prepare reserves.
 * With total == 0 or num_segments == 0 there is nothing to do: tiles, kernels and scratch_bytes are 0.  Any pointer may be NULL. */
GLU_API glu_status glu_expand_plan(size_t total, size_t num_segments, uint32_t* tile, uint32_t* tiles, uint32_t* kernels,
                                   size_t* scratch_bytes);
/* Not in the reference.  What the host enqueued in the object's last run_ptr (no device read): the tiles and the kernels (0 and 0
 * where the call had nothing to do). */
GLU_API glu_status glu_expand_last(glu_expand expand, uint32_t* tiles, uint32_t* kernels);

/* ---- gather and scatter (not in the reference): items fetched or placed by uint32 indices that live on the device, on the
 * caller's stream.  The last step behind every operator that ends in indices: the sort's and merge's uint32 values (sort an iota
 * beside the keys, then fetch records of any width through it), the out_indices of top-k, batched top-k and select, the positions
 * of sorted search.  numpy's items[indices] and out[indices] = items.  Per entry it reads 4 bytes of index, moves item_bytes once
 * in and once out, and nothing else.
 *   - COMMON TO ALL CALLS.  item_bytes is 4, 8, 16 or 32 (select's and expand's sizes); items are copied bit for bit.  `items` and
 *     `out` are aligned to min(item_bytes, 16), `indices` and `offsets` to 4 bytes.  The inputs are READ ONLY; `out` must not
 *     overlap any of them (arrays that merely touch are fine).  NO INDEX IS TRUSTED: an entry whose index fails the call's test is
 *     skipped, the entry of `out` it would have written is NOT TOUCHED, and nothing outside the arrays as the host values state
 *     them is read or written.
 *   - glu_gather_run_ptr: for j < count, if indices[j] < item_count then out[j] = items[indices[j]].  Duplicate indices are fine
 *     (a broadcast).  count < 2^32, item_count <= 2^32; byte offsets are 64 bits wide (item_count * item_bytes reaches 128 GiB).
 *   - THE BATCHED FORMS read rows of stride k of indices LOCAL to a segment, exactly what glu_top_k_run_batch_ptr and
 *     glu_top_k_run_batch_offsets_ptr write, and the segments are theirs: partition s of `count` items each (total = count *
 *     num_partitions), or [offsets[s], offsets[s + 1]) of a device array the host never reads; a segment that ends below its begin
 *     or beyond `total` is empty.  With len_s the segment's length and k_s = min(k, len_s): for j < k_s, if indices[s * k + j] <
 *     len_s then out[s * k + j] = items[begin_s + indices[s * k + j]].  Every other entry of `out` is not touched: the entries
 *     j >= k_s of a row (batched top-k's own rule) and those whose index is not below len_s.  total < 2^32, num_segments <= 2^24,
 *     num_segments * k < 2^32.
 *   - glu_gather_scatter_ptr: for j < count, if indices[j] < out_count then out[indices[j]] = items[j]; entries of `out` that no
 *     index names are not touched.  The indices are expected to be distinct.  WHERE TWO ARE EQUAL that entry holds one of their
 *     items, and for 32-byte items possibly a mix of their 16-byte halves: the one place where the result is not determined.
 *     count < 2^32, out_count <= 2^32.
 *   - count == 0 enqueues nothing; so do k == 0 or no segment in the batched forms, an empty table (item_count, out_count or total
 *     of 0: no entry can move) and then no array is looked at (all may be NULL).
 *   - One kernel per call, in one stream, with one workgroup of 256 per tile.  The STREAMING SIDE (`out` of a gather, `items` of a
 *     scatter) moves in whole 16-byte packs by contiguous lanes whatever its alignment; a 32-byte item is two packs in two
 *     neighbouring lanes; only a pack that holds an end of the array or a skipped entry goes element by element.  A lane issues all
 *     of its index loads, then all of its item loads, then stores.  Indices and the streaming side bypass the caches' retention, so
 *     that the caches hold the table.  The row of a batched entry is an exact quotient by multiplication.  No scratch, hence no
 *     prepare: every call is allocation-free and capturable from the first.  No atomics, no LDS, no look-back, no side stream, no
 *     host synchronisation, no read-back.  The grid follows from the host values and the addresses, never from the data: a captured
 *     call replays on any contents.  THE SAME INPUT GIVES THE SAME BITS EVERY TIME (a scatter: with distinct indices).
 *   - What bounds it is the memory system's answer to scattered accesses of item_bytes: a random 4-byte read moves a whole cache
 *     line for 4 useful bytes unless the table stays in a cache.  profiles/gather/README.md has the measurements.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument: a NULL object; a NULL
 *     array with work to do; a bad item_bytes; misalignment; the limits above; `out` overlapping an input.  A refused call writes
 *     nothing.
 *   - OUT OF SCOPE: items wider than 32 bytes; 64-bit indices; a scatter that reduces colliding items; two source arrays in one
 *     call (merge's iota over A || B); bucketing the indices by source address before the gather. */
typedef struct glu_gather_s* glu_gather;
/* Not in the reference. */
GLU_API glu_status glu_gather_create(glu_gather* out);
/* Not in the reference. */
GLU_API glu_status glu_gather_destroy(glu_gather gather);
/* Not in the reference.  out[j] = items[indices[j]]: the contract above.  Enqueues on `stream` (NULL: the library's queue) and
 * returns. */
GLU_API glu_status glu_gather_run_ptr(glu_gather gather, const void* items, size_t item_count, uint32_t item_bytes,
                                      const uint32_t* indices, size_t count, void* out, void* stream);
/* Not in the reference.  Rows of stride k over equal partitions of `count` items. */
GLU_API glu_status glu_gather_run_batch_ptr(glu_gather gather, const void* items, uint32_t item_bytes, size_t count,
                                            size_t num_partitions, const uint32_t* indices, size_t k, void* out, void* stream);
/* Not in the reference.  Rows of stride k over the segments of device offsets. */
GLU_API glu_status glu_gather_run_batch_offsets_ptr(glu_gather gather, const void* items, uint32_t item_bytes, size_t total,
                                                    const uint32_t* offsets, size_t num_segments, const uint32_t* indices,
                                                    size_t k, void* out, void* stream);
/* Not in the reference.  out[indices[j]] = items[j]: the contract above. */
GLU_API glu_status glu_gather_scatter_ptr(glu_gather gather, const void* items, uint32_t item_bytes, const uint32_t* indices,
                                          size_t count, void* out, size_t out_count, void* stream);
/* Not in the reference.  Host only, no device, pure: tile = entries per workgroup (256 threads x 4 packs of 16 bytes: 4096, 2048,
 * 1024 and 512 items of 4, 8, 16 and 32 bytes; the 4 is PROVISIONAL: profiles/gather/tile_sizes.txt finds 2, 4 and 8 alike), tiles =
 * ceil(count / tile), the tiles of `count` entries from an aligned base (a call on an array that starts inside a pack can take one
 * more), kernels = 1, or 0 where count == 0.  Any pointer may be NULL. */
GLU_API glu_status glu_gather_plan(size_t count, uint32_t item_bytes, uint32_t* tile, uint32_t* tiles, uint32_t* kernels);
/* Not in the reference.  What the host enqueued in the object's last call (no device read): the tiles and the kernels (0 and 0
 * where the call had nothing to do). */
GLU_API glu_status glu_gather_last(glu_gather gather, uint32_t* tiles, uint32_t* kernels);

/* ---- top-k (not in the reference): the k smallest or the k largest of `count` keys and their indices, by a radix select, on the
 * device and on the caller's stream.  Nearest neighbours, beam search, a threshold at a quantile, the heaviest groups after a
 * batched reduce.  The keys are only READ (four times where they are spread out); nothing of size `count` is written.
 *   - `keys`: count keys of one of the six glu_key_type's, on the device, READ ONLY, in any order.  k, largest (0 = smallest) and
 *     sorted are host values.
 *   - THE ORDER IS THE SORT'S: the total order on bits that glu_radix_sort_run_typed_ptr produces.  -0.0 < +0.0, and the NaNs lie
 *     beyond the infinities of their sign, ordered by their payloads.  This is the choice of sorted search and merge, and
 *     deliberately NOT the IEEE comparison of select (glu_select_run_ptr): the result is a prefix of a sort, not a comparison
 *     with a value.
 *   - WHAT IS CHOSEN.  smallest: the first k elements of the stable ascending sort of (key, index).  largest: the first k elements
 *     of the stable sort by DESCENDING key, equal keys still by ASCENDING index.  One answer for every input: among equal keys
 *     at the threshold the lowest indices win.  With code() the sort's key code (complemented for largest), in numpy:
 *     numpy.argsort(code(keys), kind="stable")[:k].
 *   - OUTPUT ORDER.  sorted != 0: in that order, best first.  sorted == 0: the same k elements in ascending order of their index,
 *     as select writes them; the final ordering is skipped.
 *   - OUTPUTS, each optional.  out_keys: the keys, bit for bit.  out_indices: their uint32 indices.  out_kth: ONE key on the
 *     device, the k-th best, which is the threshold (a median, a quantile).  Exactly k entries of each given array are written
 *     and nothing behind them.  With both arrays NULL and out_kth given the call is an order statistic and enqueues no compaction
 *     and no ordering.  All three NULL is refused.
 *   - Limits: count < 2^32 (the tile layer's); k <= count; k == 0 writes nothing, out_kth neither; count == 0 requires k == 0 and
 *     accepts NULL keys.  keys, out_keys and out_kth are aligned to the key size, out_indices to 4 bytes.
 *   - GLU_ERROR_INVALID_ARGUMENT for what the host can check, each with a message that names the argument: a NULL object; NULL keys
 *     with count > 0; a bad key type; the limits above; misalignment; all outputs NULL; an output overlapping keys or another
 *     output (arrays that merely touch are fine).  A refused call writes nothing.
 *   - HOW.  The key code turns every case into "the k smallest unsigned words".  Digits are taken from the top, 11 bits each
 *     (11 + 11 + 10 for 4-byte keys, 5 x 11 + 9 for 8-byte keys); a small record on the device holds the prefix fixed so far, how
 *     many words are still needed among those that match it, and how many lie in front.  Round 1 counts the top digit of every
 *     key (tables in LDS, one row per workgroup, the columns summed, one workgroup picks the digit at which the cumulative count
 *     reaches k).  Then, decided ON THE DEVICE: GLU_TOP_K_PATH_CANDIDATES where the bucket of that digit holds at most
 *     CAND_CAPACITY keys (default max(2^16, ceil(count / 512)); uniform keys fill count / 2048): one more read appends the
 *     matching code words to the object's scratch and one workgroup runs the remaining rounds over them; else GLU_TOP_K_PATH_FULL:
 *     every remaining round reads the input again, filtered by the prefix (all keys equal, few distinct values).  Both chains are
 *     always enqueued; the kernels of the one not taken return at once.  The compaction counts per tile the keys below the
 *     threshold and the keys equal to it, scans both (the count scan of key runs and select) and writes every key below and the
 *     first `ties` equal ones at their ranks: ascending indices, exactly k.  sorted != 0: (code word, index) pairs go to scratch,
 *     the object's own glu_radix_sort orders them (unsigned, stable), a small kernel decodes them into the outputs.
 *   - THE ONE ATOMIC on device memory is the append of the candidates: a workgroup holds its candidates in LDS and adds their number
 *     to one word whenever it holds more than a tile's worth, and at its end.  Their order is arbitrary and does not matter: only
 *     counts are taken from them, and integer counts commute.  THE SAME INPUT GIVES THE SAME BITS EVERY TIME.
 *   - The call only enqueues on `stream`: no host synchronisation, no side stream, no read-back, and no device allocation once
 *     glu_top_k_prepare covered (count, max_k, key_type) under the options set (else grow-only allocation inside the call: not
 *     capturable).  The launch sequence follows from count, k, the key type, sorted, which outputs are given, the address of keys
 *     and the options, never from the data: a captured call (one stream, no parallel branches) replays on any contents. */
typedef struct glu_top_k_s* glu_top_k;
enum
{
    GLU_TOP_K_PATH_AUTO = 0,   /* an option only: the device decides */
    GLU_TOP_K_PATH_CANDIDATES, /* as AUTO (a bucket that does not fit still falls back to FULL on the device, and is reported so) */
    GLU_TOP_K_PATH_FULL        /* the candidate chain is not enqueued */
};
/* Not in the reference. */
GLU_API glu_status glu_top_k_create(glu_top_k* out);
/* Not in the reference. */
GLU_API glu_status glu_top_k_destroy(glu_top_k top_k);
/* Not in the reference.  Grow-only scratch (glu_top_k_plan's scratch_bytes, and the object's sort prepared for max_k pairs) for calls
 * of up to `count` keys of the width of `key_type` and k up to max_k, under the options set now: after it such a call allocates
 * nothing (and can be captured). */
GLU_API glu_status glu_top_k_prepare(glu_top_k top_k, size_t count, size_t max_k, glu_key_type key_type);
/* Not in the reference.  "PATH": GLU_TOP_K_PATH_AUTO, _CANDIDATES or _FULL.  "CAND_CAPACITY": the candidates the object keeps, 1 ..
 * 2^30, or 0 for the default of the count.  "BATCH_LOOP_MIN": equal partitions of a batched call of at least this many keys go
 * through the single call one by one, 0 .. 2^32 - 1, 0 for the default (2^22: the crossover measured at 64 rows, provisional otherwise).  They exist so that tests
 * reach every path at small sizes.  Anything else is refused. */
GLU_API glu_status glu_top_k_set_option(glu_top_k top_k, const char* name, long long value);
/* Not in the reference.  The contract above.  Enqueues on `stream` (NULL: the library's queue) and returns. */
GLU_API glu_status glu_top_k_run_ptr(glu_top_k top_k, const void* keys, glu_key_type key_type, size_t count, size_t k, int largest,
                                     int sorted, void* out_keys, uint32_t* out_indices, void* out_kth, void* stream);
/* Not in the reference.  For a caller who has synchronised the stream, like glu_radix_sort_read_finish, and the only function of the
 * operator that reads back: what the object's last run_ptr did.  path = GLU_TOP_K_PATH_CANDIDATES or _FULL, as the device chose after
 * round 1; candidates = the code words collected (0 on FULL); ties = the keys equal to the threshold that were taken (1 .. k);
 * kernels = the kernels enqueued, the internal sort counted as one.  All 0 where the call had k == 0.  Any pointer may be NULL. */
GLU_API glu_status glu_top_k_read_last(glu_top_k top_k, uint32_t* path, uint32_t* candidates, uint32_t* ties, uint32_t* kernels);
/* Not in the reference.  Host only, no device, pure.  For a call of `count` keys and `k` with the arrays given or not (with_arrays:
 * out_keys or out_indices), under PATH = path and CAND_CAPACITY = cand_capacity (0: the default): rounds = 3 or 6; digit_shift[r],
 * digit_bits[r] for r < rounds (room for 6): round r takes the bits [shift, shift + bits) of the code word; tile, tiles = those of
 * glu_select_plan for a stencil of the key's width; capacity = the candidates kept; kernels = 3 for round 1, + 2 for the candidate
 * chain (not under _PATH_FULL), + 3 for every remaining round over the input, + 4 for the compaction (with_arrays), + 2 for the
 * ordering (with_arrays and sorted); 0 where count or k is 0.  scratch_bytes = what glu_top_k_prepare(count, k, key_type) reserves
 * besides the internal sort: the state and the column sums, min(tiles, 1024) rows of 2048 counters, capacity code words, two counts
 * per tile (and one tile more), k pairs.  Any pointer may be NULL. */
GLU_API glu_status glu_top_k_plan(size_t count, size_t k, glu_key_type key_type, int sorted, int with_arrays, int path,
                                  size_t cand_capacity, uint32_t* rounds, uint32_t* digit_shift, uint32_t* digit_bits, uint32_t* tile,
                                  uint32_t* tiles, uint32_t* capacity, uint32_t* kernels, size_t* scratch_bytes);

/* ---- batched top-k: the k best keys of every segment in one call -----------------------------------------
 * Not in the reference.  The segments are equal partitions of `count` keys (glu_top_k_run_batch_ptr) or [offsets[s], offsets[s + 1])
 * of a DEVICE array of num_segments + 1 uint32 that the host never reads (glu_top_k_run_batch_offsets_ptr, as glu_key_runs writes
 * it); a segment that ends below its begin or beyond `total` is empty to every kernel.  `keys` are only read; all six key types.
 *   - WHAT IS CHOSEN.  The contract of glu_top_k_run_ptr applied to each segment with k_s = min(k, its length): with code() the
 *     sort's key code (complemented for largest), numpy.argsort(code(segment), kind="stable")[:k_s].  sorted != 0: best first, else
 *     in ascending order of the index.
 *   - OUTPUTS, each optional, rows of stride k.  out_keys[s * k + j]: the keys, bit for bit.  out_indices[s * k + j]: uint32 indices
 *     LOCAL to the segment (relative to offsets[s]), as torch.topk along a dimension gives.  out_kth[s]: the k_s-th best key of
 *     segment s.  The entries j >= k_s of a row and the out_kth of an empty segment are not touched.  All three NULL is refused.
 *     k == 0 or num_segments == 0 writes nothing.
 *   - Limits: total < 2^32; num_segments <= 2^24; num_segments * k < 2^32; equal partitions: k <= count.  keys, out_keys and out_kth
 *     are aligned to the key size, out_indices and offsets to 4 bytes; no output overlaps keys, offsets or another output.
 *     GLU_ERROR_INVALID_ARGUMENT with a message that names the argument; a refused call writes nothing.
 *   - HOW.  Three classes of segments by length (glu_top_k_plan_batch states the limits; ALL OF THEM ARE PROVISIONAL, no class
 *     limit is placed by a measurement yet): up to 512 keys a WAVE per segment holds them in registers and selects with 8-bit digits on a wave-private row
 *     of counters in LDS; up to 8 / 32 / 128 KiB of keys a WORKGROUP reads the segment once into LDS and runs every 11-bit round
 *     there; a longer segment is streamed by one workgroup (round 1 over the segment; then the threshold's bucket is collected into
 *     LDS where it fits, cand_room keys, else every round reads the segment again).  Equal partitions: the host picks the one class
 *     kernel (path GLU_TOP_K_BATCH_WAVE / _BLOCK / _LONG); partitions of at least BATCH_LOOP_MIN keys (glu_top_k_set_option; 0: the
 *     default) go through glu_top_k_run_ptr one after the other (GLU_TOP_K_BATCH_LOOP), each filling the device by itself.  Device
 *     offsets (GLU_TOP_K_BATCH_BINNED): a binning kernel appends every non-empty segment to the list of its class, one kernel per
 *     class walks its list.  sorted with arrays: the class kernels write (code word, local index) rows to scratch, padded behind
 *     k_s with all-ones codes, the object's own sort orders all rows with ONE glu_radix_sort_run_batch_ptr (stable: ties stay by
 *     ascending index, pads behind real entries), a decode kernel writes j < k_s of every row.  WHERE k EXCEEDS THE BATCHED SORT'S
 *     SINGLE-BLOCK LIMIT (glu_radix_sort_plan_batch: path 3) THAT SORT IS ONE ORDINARY SORT PER ROW, and `kernels` counts one per row.
 *   - The call only enqueues on `stream`: no host synchronisation, no read-back, no side stream; after glu_top_k_prepare_batch no
 *     allocation (capturable as a linear chain).  The launch sequence follows from host values only.  The same input gives the
 *     same bits every time: the only atomics on device memory are the list appends of the binning kernel, and the order of a list
 *     does not matter. */
enum
{
    GLU_TOP_K_BATCH_NONE = 0, /* nothing is enqueued: no key, no segment or k == 0 */
    GLU_TOP_K_BATCH_WAVE,     /* equal partitions on the wave class's kernel */
    GLU_TOP_K_BATCH_BLOCK,    /* ... on a workgroup tile's kernel */
    GLU_TOP_K_BATCH_LONG,     /* ... on the streaming kernel */
    GLU_TOP_K_BATCH_LOOP,     /* ... of at least BATCH_LOOP_MIN keys: the single call, partition after partition */
    GLU_TOP_K_BATCH_BINNED    /* device offsets: binning, then one kernel per class */
};
/* Not in the reference.  Equal partitions: segment s is partition s of `count` keys. */
GLU_API glu_status glu_top_k_run_batch_ptr(glu_top_k top_k, const void* keys, glu_key_type key_type, size_t count, size_t num_partitions,
                                           size_t k, int largest, int sorted, void* out_keys, uint32_t* out_indices, void* out_kth,
                                           void* stream);
/* Not in the reference.  Device offsets. */
GLU_API glu_status glu_top_k_run_batch_offsets_ptr(glu_top_k top_k, const void* keys, glu_key_type key_type, size_t total,
                                                   const uint32_t* offsets, size_t num_segments, size_t k, int largest, int sorted,
                                                   void* out_keys, uint32_t* out_indices, void* out_kth, void* stream);
/* Not in the reference.  Grow-only scratch for batched calls of up to `total` keys of the width of `key_type` in up to num_segments
 * segments with k up to max_k, under the options set now (the list image, the rows of pairs and the object's sort for them, the
 * single call's scratch where equal partitions of total / num_segments keys take the loop), and the LDS opt-in of the workgroup
 * kernels: after it such a call allocates nothing. */
GLU_API glu_status glu_top_k_prepare_batch(glu_top_k top_k, size_t total, size_t num_segments, size_t max_k, glu_key_type key_type);
/* Not in the reference.  Host only, no device, pure: the single statement of the unmeasured choices.  offsets_form == 0: `count` keys
 * per partition; else `count` is the batch's total.  loop_min: BATCH_LOOP_MIN, 0 for the default.  path = GLU_TOP_K_BATCH_*; tile =
 * the class limit the equal partitions run under (0: none); class_limits[0 .. 4) = the longest segment of the wave class and of the
 * three workgroup tiles for this key width (8-byte keys: half the 4-byte ones, the wave class excepted); wave_digit_bits = the wave
 * class's digit width; cand_room = keys of the long class's candidate buffer; loop_min_used = the threshold in force; kernels = what
 * the call enqueues (1 class kernel, or per partition the single call's under LOOP, or the binning kernel and one kernel per list
 * that can hold a segment; + the sort, counted as one or as one per row, and the decode kernel where sorted with arrays; 0 where
 * nothing is enqueued); scratch_bytes = the list image and the rows of pairs (LOOP: the single call's).  Any pointer may be NULL. */
GLU_API glu_status glu_top_k_plan_batch(size_t count, size_t num_segments, size_t k, glu_key_type key_type, int offsets_form, int sorted,
                                        int with_arrays, size_t loop_min, uint32_t* path, uint32_t* tile, uint32_t* class_limits,
                                        uint32_t* wave_digit_bits, uint32_t* cand_room, size_t* loop_min_used, uint32_t* kernels,
                                        size_t* scratch_bytes);
/* Not in the reference.  For a caller who has synchronised the stream: the segments of the object's last batched call per class (device
 * offsets: the counts the binning kernel left; equal partitions: the host's own; LOOP counts its partitions as long) and the kernels
 * it enqueued (the plan's).  Any pointer may be NULL. */
GLU_API glu_status glu_top_k_read_batch(glu_top_k top_k, uint32_t* wave_segments, uint32_t* block_segments, uint32_t* long_segments,
                                        uint32_t* kernels);

/* ---- sharded sort over the GPUs of one node ---------------------------------------------------------
 * The reference is single-device (one GL context, no communication code: SURVEY.md section 2 row C1); this is the
 * sharded form of glu::RadixSort::operator() (glu/RadixSort.hpp:273-334) that BASELINE.json configs[3] asks for.
 * One process per GPU, rank r holds slice r of the array.  A sort = stable partition of the slice by the top 8 key
 * bits -> ncclAllGather of the R x 256 bucket histograms -> identical contiguous bucket -> rank plan on every rank (a
 * bucket is never split) -> ONE grouped RCCL exchange of keys and values (receive segments in source-rank order) ->
 * local stable sort.  The ranks' outputs concatenated in rank order equal the single-device stable sort; shard sizes
 * follow the data.  If all keys of all ranks share the top byte (24-bit keys ...), the partition falls back to the next lower
 * byte, so that small-range keys still spread over the ranks; one hot bucket still bounds the balance.  RCCL is loaded with dlopen at first use (GLU_HIP_RCCL_LIB overrides the name).
 * Every rank must issue the same sequence of glu_dist calls (they contain collectives).
 * Errors are collective: when one rank finds its arguments, sizes or allocations wrong in glu_dist_sort_begin /
 * glu_dist_sort_finish / glu_dist_sort_ptr, EVERY rank returns a non-zero status from that call (the failing rank its own,
 * the others the same code with a message naming the rank) before anything is sent or received, and the object can be used
 * for the next sort; no rank is left waiting in a collective.  A rank that must give up between begin and finish (it
 * cannot allocate its receive arrays) still calls glu_dist_sort_finish, with capacity 0.  A failing RCCL or HIP call
 * after the ranks have agreed is not recoverable (it is reported by the rank that sees it; destroy the object). */

#define GLU_DIST_UNIQUE_ID_BYTES 128
/* Can this process load RCCL (GLU_HIP_RCCL_LIB, librccl.so.1, ...) with the nine entry points the sharded sort needs?
 * dlopen + dlsym only -- no device call and none of ncclGetUniqueId's side effects (a bootstrap listener socket and
 * thread per call): what a rank other than 0 asks before the ranks agree to use glu_dist_*. */
GLU_API glu_status glu_dist_available(void);
/* Rank 0: ncclGetUniqueId; the caller carries the bytes to the other ranks (MPI, torch.distributed, a file ...). */
GLU_API glu_status glu_dist_unique_id(void* id_out, size_t id_bytes);
/* ncclCommInitRank on the library's device (glu_set_device) + a local glu_radix_sort; collective over all ranks. */
GLU_API glu_status glu_dist_create(const void* unique_id, size_t id_bytes, int world_size, int rank, glu_dist* out);
GLU_API glu_status glu_dist_destroy(glu_dist dist);
GLU_API glu_status glu_dist_world(glu_dist dist, int* world_size, int* rank);
/* The bit position of the key byte the last sort on `dist` was partitioned on (24 unless the fallback ran). */
GLU_API glu_status glu_dist_partition_shift(glu_dist dist, uint32_t* shift);
/* The local glu_radix_sort that `dist` partitions and sorts with (owned by `dist`, do not destroy): for
 * glu_radix_sort_set_digit_bits / set_profiling / read_profile. */
GLU_API glu_status glu_dist_local_sorter(glu_dist dist, glu_radix_sort* out);
/* Grow-only buffers for slices of `local_count` pairs and (for glu_dist_sort_ptr) shards of `recv_capacity` pairs: after
 * it a sort whose slice / shard fit allocates nothing (the analogue of RadixSort::prepare_internal_buffers, :237-271).
 * Like glu_radix_sort_prepare it PLACES large arrays by measurement -- the local sorter's scratch, and against it the
 * send-side pair (the partitioned slice) and the receive-side pair of glu_dist_sort_ptr, three searches of 0.13-1 s each from
 * 2^27 pairs up (skipped when memory is short or GLU_HIP_SCRATCH_TUNE=0): every scatter pass of a rank's sort except the
 * first one's source, the caller's slice, then runs between pairs of arrays that were chosen, not drawn (2.33 -> 2.19 ms of
 * compute per 2^27 pairs in an alternating same-box comparison with the search switched off).  Receive arrays that a caller
 * hands to glu_dist_sort_finish are the caller's and are not placed. */
GLU_API glu_status glu_dist_prepare(glu_dist dist, size_t local_count, size_t recv_capacity);
/* First half of a sort: partition + histogram exchange + plan.  The partition is enqueued on `stream`; the call returns
 * when the host has the plan (it waits for the histogram exchange, which runs on a side stream beside the partition's
 * scatter kernel, not for the partition).  *recv_count = pairs this rank will receive. */
GLU_API glu_status glu_dist_sort_begin(glu_dist dist, const uint32_t* keys, const uint32_t* vals, size_t local_count,
                                       void* stream, size_t* recv_count);
/* Second half: the grouped exchange into the caller's arrays (capacity >= the count glu_dist_sort_begin returned) and the
 * local sort, enqueued on `stream` (no host synchronisation). */
GLU_API glu_status glu_dist_sort_finish(glu_dist dist, uint32_t* recv_keys, uint32_t* recv_vals, size_t capacity, void* stream);
/* Both halves with receive arrays owned by `dist` (grown if the shard does not fit).  LIFETIME of *out_keys / *out_vals: they
 * point into arrays `dist` owns and are valid until the NEXT glu_dist_sort_ptr call on `dist` returns -- that call may overwrite
 * them (same arrays) or outgrow them (the outgrown arrays stay allocated for exactly one more call, so a result that is still
 * being read while the next sort is enqueued does not dangle; the call after that frees them).  Copy out what must live longer;
 * glu_hip.dist.DistributedRadixSort.sort() returns tensors that alias these arrays under the same rule. */
GLU_API glu_status glu_dist_sort_ptr(glu_dist dist, const uint32_t* keys, const uint32_t* vals, size_t local_count,
                                     void* stream, uint32_t** out_keys, uint32_t** out_vals, size_t* out_count);
/* 1 if the local sort of the last sort on `dist` was the SEGMENTED sort of the low 24 bits per bucket (the shard arrives as one
 * message per source rank, each grouped by bucket; glu_radix_sort_run_segments_ptr: one segmented counting pass + an in-LDS pass
 * when the runs (bucket, next byte) fit an LDS tile -- up to four ranks x 2^27 pairs --, else three segmented passes;
 * glu_radix_sort_read_seg_finish on glu_dist_local_sorter tells which), 0 if it was the ordinary sort of all 32 bits (small
 * shards, shards made of very many tiny pieces, a partition on a lower byte). */
GLU_API glu_status glu_dist_last_local_sort(glu_dist dist, uint32_t* segmented);
/* The exchange in ROUNDS.  With more than one rank and large shards (2^24 pairs per rank and more; GLU_HIP_DIST_ROUNDS_MIN)
 * every rank's buckets are cut into `rounds` groups of about equal size (1 .. 8; default 3 from four ranks up, 1 below: at two
 * ranks half of the data never leaves and the one link to the peer bounds the exchange far above the sort; GLU_HIP_DIST_ROUNDS), round j
 * carries group j of every rank on a side stream, and the local sort of group j runs on the sort's stream behind round j
 * only: the later groups travel while the earlier ones are sorted, so ONE sort takes about partition + one round +
 * max(the other rounds, the sorts) instead of partition + exchange + sort.  The price is compute: a group is sorted by its
 * own three passes, and four sorts of a quarter cost about a third more than one sort of the whole (measured without a
 * fabric: 2.70 -> 3.2 ms per 2^27 pairs at 4 rounds).  A caller that keeps several sorts in flight on several objects, where
 * the exchange of one hides under the local sort of another anyway, sets 1 = one grouped exchange, then the local sort.
 * Every rank must use the same value (the rounds are part of the message sequence).  glu_dist_last_rounds: what the last
 * sort used. */
GLU_API glu_status glu_dist_set_rounds(glu_dist dist, int rounds);
GLU_API glu_status glu_dist_last_rounds(glu_dist dist, uint32_t* rounds);
/* CUs that the sort kernels of `dist` leave free (for RCCL kernels of another sort in flight; the partition pass always
 * leaves 8, one per XCD, for the histogram all-gather that runs beside its scatter kernel). */
GLU_API glu_status glu_dist_set_reserved_cus(glu_dist dist, int cus);
/* Device time per phase, averaged over the sorts since the last call (after glu_dist_set_profiling(dist, 1)):
 * ms4 = {partition, histogram exchange + plan (side stream), exchange, local sort}. */
GLU_API glu_status glu_dist_set_profiling(glu_dist dist, int enable);
GLU_API glu_status glu_dist_phase_times(glu_dist dist, double* ms4, uint64_t* sorts);
/* The plan as pure host functions (no device, no RCCL needed: unit-testable with simulated ranks).
 * all_hist: [world_size][256] bucket histograms; bucket_owner: [256] rank of every bucket (contiguous, monotone, balanced
 * on the boundary nearest to r * N / R); send_counts / recv_counts: [world_size] for `rank`. */
GLU_API glu_status glu_dist_plan_buckets(const uint32_t* all_hist, int world_size, int* bucket_owner);
GLU_API glu_status glu_dist_plan_counts(const uint32_t* all_hist, int world_size, int rank, const int* bucket_owner,
                                        uint64_t* send_counts, uint64_t* recv_counts);
/* The groups of the exchange in rounds (glu_dist_set_rounds): group_cut: [world_size][rounds + 1], group j of rank q =
 * the buckets [group_cut[q][j], group_cut[q][j + 1]) -- contiguous, in order, together exactly q's buckets, cut on the bucket
 * boundaries nearest to j / rounds of what q receives (a bucket is never split; groups may be empty). */
GLU_API glu_status glu_dist_plan_groups(const uint32_t* all_hist, int world_size, const int* bucket_owner, int rounds,
                                        int* group_cut);

/* ---- timing: replaces glu::measure_gl_elapsed_time (glu/gl_utils.hpp:249-265) ---------------------- */

/* glGenQueries + glBeginQuery(GL_TIME_ELAPSED) on the library queue. */
GLU_API glu_status glu_timer_begin(glu_timer* out);
/* glEndQuery + glGetQueryObjectui64v(GL_QUERY_RESULT): waits, returns nanoseconds, frees the timer. */
GLU_API glu_status glu_timer_end(glu_timer timer, uint64_t* elapsed_ns);

#ifdef __cplusplus
}
#endif

#endif /* GLU_HIP_H */
