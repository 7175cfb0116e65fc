// glu_hip.hip -- RadixSort's whole-key driver of libglu_hip.so: sort_prepare, the sort in one workgroup, sort_bits, the options of a
// sort object and the glu_radix_sort_* entry points of include/glu_hip.h that are not about segments or placement (gfx950 only, no
// CPU fallback).  What the sort's other translation units call here, and what this one calls in them: glu_sort_driver.hpp; all the
// library's units: glu_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <strings.h>
#include <vector>

#include "glu_host.hpp"
#include "glu_sort_driver.hpp"
#include "glu_sort_launch.hpp"
#include "radix_sort_kernels.hpp"
#include "radix_pair_passes.hpp"
#include "radix_lds_plan.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

// ------------------------------------------------------------------------------------------------------------
// radix sort
// ------------------------------------------------------------------------------------------------------------
// (may_place: glu_sort_driver.hpp)
glu_status glu_hip::host::sort_prepare(glu_radix_sort_s* s, size_t count, size_t key_size, bool with_vals, bool may_place)
{
    if (count <= 1) return GLU_OK;
    // large key + value scratch that has to be (re)allocated anyway: where the two arrays lie to each other decides between
    // discrete speeds of every pass, so a few placements are tried and the fastest is kept
    const bool grows = s->keys.size < count * key_size || (with_vals && s->vals.size < count * sizeof(uint32_t));
    if (grows && !s->tuning) // the arrays the last placement search chose (if any) are about to be replaced
        s->tuned_candidates = 0, s->tuned_ms = s->tuned_worst_ms = 0.0, s->tuned_spacer_mib = 0;
    // The narrow hand-off's side array of 2-byte keys: for the sorts that can take it -- 4-byte keys with values, of a size at which the
    // attempt to end in LDS is made (the same conditions as the attempt's tables below and in sort_bits).  In front of the placement
    // search, whose trial sorts then run as the object's sorts will.
    static_assert(256u * finish_geometry_capacity(kFinishGeometries) < kPlanMinCount, "PassPlan::narrow: a planned sort whose runs all fit a tile has both of its top-bit scatters move data");
    if (key_size == 4 && with_vals && s->narrow_handoff && s->lds_finish && s->pairs && !s->no_plan && !s->no_lines && !s->force_small &&
        count >= kPlanMinCount && count >= (s->finish_min ? s->finish_min : finish_min_count(key_size)) && finish_geometry_for(count) != 0)
        GLU_TRY(s->narrow_keys.reserve(count * sizeof(uint16_t)));
    if (may_place && with_vals && s->tune_scratch && !s->tuning && count * key_size >= kTuneMinKeyBytes && grows)
        GLU_TRY(tune_scratch_placement(s, count, key_size));
    GLU_TRY(s->keys.reserve(count * key_size));
    if (with_vals) GLU_TRY(s->vals.reserve(count * sizeof(uint32_t)));
    uint64_t cap = (uint64_t) g_dev.num_cus * kMaxBlocksPerCu;
    GLU_TRY(s->table.reserve((kMaxRadix * cap + kMaxRadix) * sizeof(uint32_t)));
    if (s->plan.size < sizeof(PassPlan))
    {
        GLU_TRY(s->plan.reserve(sizeof(PassPlan)));
        HIP_TRY(hipMemset(s->plan.ptr, 0, sizeof(PassPlan))); // never read uninitialised (glu_radix_sort_read_plan)
        HIP_TRY(hipDeviceSynchronize());                       // (the sort's stream does not wait for the null stream)
    }
    const size_t pair_from = std::min<size_t>(s->pair_min ? s->pair_min : kPairMinKeyBytes / key_size,
                                              s->lds_finish ? (s->finish_min ? s->finish_min : finish_min_count(key_size)) : (size_t) -1);
    if (count >= kPlanMinCount && count >= pair_from && s->pairs && !s->no_plan &&
        !s->no_lines && !s->force_small)
    {
        const size_t nb = (size_t) g_dev.num_cus;
        GLU_TRY(s->pair_t2.reserve((size_t) kPairRadix * nb * kPairRowWords * sizeof(uint32_t)));
        GLU_TRY(s->pair_table.reserve(((size_t) kPairRadix * nb + kPairRadix) * sizeof(uint32_t)));
        GLU_TRY(s->pair_ranges.reserve(nb * sizeof(uint2)));
        GLU_TRY(s->pair_sub.reserve((size_t) kPair4Radix * nb * kPairSub * sizeof(uint32_t)));
        if (s->lds_finish)
        {
            GLU_TRY(s->finish_lengths.reserve((size_t) kFinishRuns * sizeof(uint32_t)));
            GLU_TRY(s->finish_starts.reserve(((size_t) kFinishRuns + 1) * sizeof(uint32_t)));
            GLU_TRY(s->finish_crowded.reserve(crowded_list_words(kFinishRuns) * sizeof(uint32_t)));
            GLU_TRY(s->finish_outcomes.reserve(512 * sizeof(uint32_t))); // (per attempt of a window: outcome and tile; the hand-off)
            GLU_TRY(s->pair_wide.reserve((size_t) nb * kPairWideStride * sizeof(uint32_t)));
            {
                // runs longer than the in-LDS pass's tile are sorted by segmented passes (radix_finish_long_runs_kernel)
                const uint32_t shares = (uint32_t) g_dev.num_cus * kLongRunsSharesPerWg;
                GLU_TRY(s->long_image.reserve((size_t) LongRunsLayout(shares).words * sizeof(uint32_t)));
                GLU_TRY(s->long_hdr.reserve(64));
                GLU_TRY(s->long_bits.reserve(2 * ((size_t) kLongRunsMax + shares) * sizeof(uint64_t)));
                GLU_TRY(s->table.reserve(((size_t) kLongRunsMax + shares) * 256 * sizeof(uint32_t)));
            }
            if (!s->finish_hint)
            {
                HIP_TRY(hipHostMalloc((void**) &s->finish_hint, 64));
                memset(s->finish_hint, 0, 64);
            }
        }
    }
    return GLU_OK;
}

namespace
{
// n <= one tile: the whole sort in a single workgroup / single launch (always 8-bit digits: the result does not
// depend on the digit width)
template<typename KeyT, int THREADS, int KPT, bool XF>
glu_status launch_single_block_xf(KeyT* keys, uint32_t* vals, size_t count, uint32_t first_bit, uint32_t end_bit,
                                  hipStream_t stream, uint32_t xform)
{
    using Smem = SingleBlockSmem<KeyT, 8, THREADS, KPT>;
    auto kern = radix_sort_single_block_kernel<KeyT, 8, THREADS, KPT, XF>;
    static std::once_flag lds_opt_in;
    static hipError_t lds_opt_in_result = hipSuccess;
    std::call_once(lds_opt_in, [&] {
        lds_opt_in_result = hipFuncSetAttribute((const void*) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) sizeof(Smem));
    });
    HIP_TRY(lds_opt_in_result);
    hipLaunchKernelGGL(kern, dim3(1), dim3(THREADS), sizeof(Smem), stream, keys, vals, (uint32_t) count, first_bit, end_bit, xform);
    HIP_TRY(hipGetLastError());
    return GLU_OK;
}

template<typename KeyT, int THREADS, int KPT>
glu_status launch_single_block(KeyT* keys, uint32_t* vals, size_t count, uint32_t first_bit, uint32_t end_bit,
                               hipStream_t stream, uint32_t xform)
{
    if (xform) return launch_single_block_xf<KeyT, THREADS, KPT, true>(keys, vals, count, first_bit, end_bit, stream, xform);
    return launch_single_block_xf<KeyT, THREADS, KPT, false>(keys, vals, count, first_bit, end_bit, stream, 0);
}

template<typename KeyT>
constexpr size_t single_block_limit() { return sizeof(KeyT) == 4 ? 1024 * 16 : 1024 * 8; } // 144 KB / 112 KB of LDS

template<typename KeyT>
glu_status sort_single_block(KeyT* keys, uint32_t* vals, size_t count, uint32_t first_bit, uint32_t end_bit,
                             hipStream_t stream, uint32_t xform)
{
    if (count <= 1024) return launch_single_block<KeyT, 256, 4>(keys, vals, count, first_bit, end_bit, stream, xform);
    // 1024 threads even for small tiles: the passes are latency chains inside one CU, 16 waves shorten every link
    // (2048 pairs: 14 -> 11 us, 4096: 20 -> 15 us, 8192: 30 -> 23 us against 256 threads x 16 / 1024 x 12)
    if (count <= 2048) return launch_single_block<KeyT, 1024, 2>(keys, vals, count, first_bit, end_bit, stream, xform);
    if (count <= 4096) return launch_single_block<KeyT, 1024, 4>(keys, vals, count, first_bit, end_bit, stream, xform);
    if (count <= 8192) return launch_single_block<KeyT, 1024, 8>(keys, vals, count, first_bit, end_bit, stream, xform);
    if constexpr (sizeof(KeyT) == 4)
    {
        if (count <= 1024 * 12) return launch_single_block<KeyT, 1024, 12>(keys, vals, count, first_bit, end_bit, stream, xform);
        return launch_single_block<KeyT, 1024, 16>(keys, vals, count, first_bit, end_bit, stream, xform);
    }
    else
        return launch_single_block<KeyT, 1024, 8>(keys, vals, count, first_bit, end_bit, stream, xform);
}
} // namespace

// vals == nullptr: keys-only sort (no value traffic, no value scratch)
template<typename KeyT>
glu_status glu_hip::host::sort_bits(glu_radix_sort_s* s, KeyT* keys, uint32_t* vals, size_t count, uint32_t first_bit, uint32_t end_bit,
                                    hipStream_t stream, uint32_t key_xf)
{
    // 1. checks, and the whole sort in one workgroup
    if (count <= 1 || first_bit >= end_bit) return GLU_OK; // RadixSort.hpp:278-279
    if (count > 0xFFFF0000ull) return fail(GLU_ERROR_INVALID_ARGUMENT, "count %zu does not fit 32-bit indexing", count);
    if (((uintptr_t) keys % sizeof(KeyT)) != 0 || (vals && ((uintptr_t) vals % sizeof(uint32_t)) != 0))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "key/value arrays must be aligned to their element size");
    GLU_TRY(sort_prepare(s, count, sizeof(KeyT), vals != nullptr)); // RadixSort.hpp:281 (no-op when prepared)
    s->last_planned = false; // (what glu_radix_sort_read_plan / read_finish report is about THIS sort: step 4)
    s->last_finish_attempted = false;
    s->last_finish_long_ok = false;
    s->last_narrow_offered = false;

    if (count <= single_block_limit<KeyT>() && !s->no_single_block)
    {
        s->mark(stream); // profiling: booked as one "scatter" launch (count / scan intervals are empty)
        s->mark(stream);
        s->mark(stream, true);
        GLU_TRY(sort_single_block<KeyT>(keys, vals, count, first_bit, end_bit, stream, key_xf | (key_xf << 2)));
        s->mark(stream, true);
        return GLU_OK;
    }

    KeyT* kbuf[2] = {keys, (KeyT*) s->keys.ptr};
    uint32_t* vbuf[2] = {vals, vals ? (uint32_t*) s->vals.ptr : nullptr};
    s->cur_kind = 0;
    s->cur_behind = false; // (a call that failed half-way must not leave the next one's profile marks switched off)
    s->cur_seq = 0;
    // large sorts: device-side pass plan (constant-digit passes are skipped, the arrays' roles follow on the device)
    const bool planned = count >= kPlanMinCount && !s->no_plan;
    const bool pair_tables = planned && s->pairs && s->pair_t2.ptr;
    const bool pairs_ok = pair_tables && count >= (s->pair_min ? s->pair_min : kPairMinKeyBytes / sizeof(KeyT));
    const bool lines8 = lines_applicable<KeyT, 8>(s, kbuf[0], vbuf[0], kbuf[1], vbuf[1], count);
    const bool lines4 = lines_applicable<KeyT, 4>(s, kbuf[0], vbuf[0], kbuf[1], vbuf[1], count);

    // 2. the attempt.  Whole keys, 8-bit digits (one pass per key byte), line passes, from finish_min_count elements: the sort first
    // tries to end in LDS (radix_lds_finish.hpp) -- the two top-bit passes and the in-LDS pass are enqueued in front of the ordinary
    // passes, and the device runs one of the two sequences.
    uint32_t finish_kpt = 0; // (the geometry that suits uniform keys; 0: no attempt)
    if (pair_tables && s->lds_finish && s->finish_starts.ptr && first_bit == 0 && end_bit == 8 * sizeof(KeyT) && s->digit_bits == 8 &&
        count >= (s->finish_min ? s->finish_min : finish_min_count(sizeof(KeyT))) && lines8)
        finish_kpt = finish_geometry_for(count);
    // The runs' key bits are chosen on the device from a sample of the keys (untyped keys: radix_sample_top_kernel).
    // GLU_HIP_SORT_DEVICE_TOP=0: the host guesses from the object's last attempt (sort_call_plan.hpp: finish_attempts has both rules).
    const bool device_top = finish_kpt && s->device_top && key_xf == KEY_XF_NONE && !s->no_bit_shortcut;
    if (finish_kpt)
    {
        uint32_t hint[5] = {};
        if (s->finish_hint) // (word 0 was stored last: what is read behind it belongs to that attempt or a later one)
        {
            hint[0] = __atomic_load_n(s->finish_hint, __ATOMIC_ACQUIRE);
            hint[3] = __atomic_load_n(s->finish_hint + 3, __ATOMIC_ACQUIRE);
            hint[1] = s->finish_hint[1], hint[2] = s->finish_hint[2], hint[4] = s->finish_hint[4];
        }
        if (!finish_attempts(s->feedback, s->finish_hint ? hint : nullptr, device_top, sizeof(KeyT), end_bit)) finish_kpt = 0;
    }
    if (finish_kpt) s->cur_seq = s->feedback.finish_seq;
    // (typed keys and sorts that do not collect which bits vary: the whole key's top bits)
    const uint32_t finish_top_bit = finish_kpt && !device_top && key_xf == KEY_XF_NONE && !s->no_bit_shortcut && s->feedback.finish_top
                                        ? std::min<uint32_t>(s->feedback.finish_top, end_bit)
                                        : end_bit;
    // runs longer than the tile: segmented passes over just them (4-byte untyped keys with values, all 16 low bits inside two digits)
    // (every key type since round 6; the passes cover 16 low bits of 4-byte keys, 48 of 8-byte keys)
    const bool finish_long_ok = finish_kpt && s->long_runs && s->long_image.ptr && finish_top_bit >= 16 &&
                                finish_top_bit - 16u <= (sizeof(KeyT) == 4 ? 16u : 48u);
    // the narrow hand-off (PassPlan::narrow): untyped 4-byte keys with values, on an object whose prepare reserved the side array
    uint16_t* const narrow_keys = finish_kpt && sizeof(KeyT) == 4 && vals && key_xf == KEY_XF_NONE && s->narrow_handoff &&
                                          s->narrow_keys.size >= count * sizeof(uint16_t)
                                      ? (uint16_t*) s->narrow_keys.ptr
                                      : nullptr;
    const uint32_t finish_last = std::min<uint32_t>(finish_kpt + 2, kFinishGeometries); // the larger tiles enqueued behind it
    // the one that gets a workgroup per run: what this object's last sort took if that is among them, else the uniform-keys one
    const uint32_t finish_expected =
        s->feedback.finish_last_geo >= finish_kpt && s->feedback.finish_last_geo <= finish_last ? s->feedback.finish_last_geo : finish_kpt;

    // 3. the passes (sort_call_plan.hpp)
    static_assert(kSortCallMaxPasses == (uint32_t) kPlanMaxPasses, "a call's pass list is as long as the device-side plan");
    SortPassList list;
    if (!sort_call_passes(list, sizeof(KeyT), first_bit, end_bit, s->digit_bits, key_xf, finish_kpt != 0, finish_top_bit, pairs_ok, lines8, lines4))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "too many passes");
    const SortPass* const passes = list.passes;
    const uint32_t num_passes = list.num;

    // 4. what the read_* entry points report about this sort
    s->last_planned = planned;
    s->last_finish_attempted = finish_kpt != 0;
    s->last_finish_long_ok = finish_long_ok;
    s->last_narrow_offered = narrow_keys != nullptr && passes[1].pair_role == 2;
    s->last_device_top = finish_kpt && device_top;
    s->last_finish_top = finish_kpt ? finish_top_bit : 0u;
    s->last_finish_capacity = finish_kpt ? finish_geometry_capacity(finish_last) : 0u;
    if (planned)
        for (uint32_t i = 0; i < kSortCallMaxPasses; i++) s->last_pair_roles[i] = i < num_passes ? (uint32_t) passes[i].pair_role : 0u;

    // 5. enqueue
    if (planned)
    {
        // per sort: no follower counts for itself yet, nothing is known about the key bits
        PassPlan* plan = (PassPlan*) s->plan.ptr;
        static_assert(offsetof(PassPlan, narrow) + sizeof(plan->narrow) <= sizeof(PassPlan) && offsetof(PassPlan, narrow) + 64 > sizeof(PassPlan),
                      "narrow is the last member of the zeroed tail of the plan");
        static_assert(offsetof(PassPlan, pair_fallback) % 64 == 0 && sizeof(PassPlan) % 64 == 0, "one aligned fill");
        HIP_TRY(hipMemsetAsync(plan->pair_fallback, 0, sizeof(PassPlan) - offsetof(PassPlan, pair_fallback), stream));
        if (finish_kpt && device_top)
        {
            hipLaunchKernelGGL((radix_sample_top_kernel<KeyT>), dim3(kSampleTopBlocks), dim3(256), 0, stream, (const KeyT*) kbuf[0], (uint32_t) count, end_bit,
                               std::min<uint32_t>(s->feedback.top_floor, end_bit), plan);
            HIP_TRY(hipGetLastError());
        }
    }
    // (see glu_radix_sort_s::side)
    // Four cross-stream dependencies cost 0.1 ms that only long kernels hide: a sort whose attempt is refused and whose
    // ordinary passes skip (2^28 all-zero keys, the reference's benchmark input: 0.22 ms on one queue, 0.35 forked) is
    // better off on one queue -- so an object whose last known attempt was refused does not fork (the first sort of an object does).
    const bool fork = planned && finish_kpt && s->fork_behind && !s->feedback.finish_last_refused && s->ensure_side();
    // Once the side stream has forked (behind the plan kernel of pass 0: launch_pass_lines) it joins the caller's queue on every way
    // out of this function: no kernel stays in flight on a stream the caller cannot wait for, no capture ends with an unjoined fork.
    // The destructor is the way out of a failure and ignores what the two calls return.
    struct SideJoin
    {
        glu_radix_sort_s* s;
        hipStream_t stream;
        hipError_t join()
        {
            s->side_forked = false;
            const hipError_t e = hipEventRecord(s->ev_join, s->side);
            return e != hipSuccess ? e : hipStreamWaitEvent(stream, s->ev_join, 0);
        }
        ~SideJoin() { if (s->side_forked) (void) join(); }
    } side_join{s, stream};
    int cur = 0; // (sorts without a plan: which pair of arrays holds the data)
    uint32_t pass = 0;
    for (; pass < num_passes; pass++)
    {
        const uint32_t shift = passes[pass].shift, bits = passes[pass].bits, xform = passes[pass].xform;
        if (planned)
        {
            PlanArgs pa;
            pa.plan = (PassPlan*) s->plan.ptr;
            pa.pass = pass;
            pa.may_skip = xform == 0; // encode / decode passes run whatever the data looks like
            // the first pass's count kernel notes which key bits vary at all (untyped keys: what is sorted is the raw
            // bit pattern); a later pass whose digit cannot vary then knows that it is an identity before it counts
            if (key_xf == KEY_XF_NONE && !s->no_bit_shortcut) pa.flags = pass == 0 ? kPlanCollectBits : (pa.may_skip ? kPlanShortcut : 0u);
            pa.pair_role = passes[pass].pair_role;
            if (pa.pair_role == 1)
            {
                pa.shift2 = passes[pass + 1].shift;
                pa.bits2 = passes[pass + 1].bits;
            }
            s->cur_kind = finish_kpt && pass < 2 ? 1 : 0;
            pa.behind_attempt = finish_kpt && pass >= 2;
            s->cur_behind = pa.behind_attempt; // (light profiling: no events around the sequence that is expected to return at once)
            if (finish_kpt && pass == 0)
            {
                pa.finish_geo_first = finish_kpt;
                pa.finish_geo_last = finish_last;
                pa.finish_first_ordinary = 2;
                pa.finish_num_ordinary = num_passes - 2;
                pa.finish_seq = s->feedback.finish_seq;
                pa.finish_top_bit = finish_top_bit;
                pa.finish_key_bits = end_bit;
                pa.finish_long_ok = finish_long_ok;
                pa.fork_side = fork;
            }
            pa.unitsum_side = fork && pass == 1 && pa.pair_role == 2 && bits == 8;
            if (finish_kpt && pass < 2 && s->last_narrow_offered) pa.narrow_keys = narrow_keys;
            GLU_TRY(dispatch_pass<KeyT>(s, kbuf[0], vbuf[0], kbuf[1], vbuf[1], count, shift, bits, nullptr,
                                        fork && pa.behind_attempt ? s->side : stream, xform, pa));
            if (finish_kpt && pass == 1)
            {
                if (fork) HIP_TRY(hipEventRecord(s->ev_fork2, stream)); // (the data is where the in-LDS pass and the long-run passes find it)
                // the in-LDS pass, in place on whichever pair of arrays holds the data now (returns at once if the
                // device chose the ordinary passes, which follow)
                s->cur_kind = 2;
                s->cur_behind = false;
                s->mark(stream);
                s->mark(stream);
                const FinishMarks finish_marks{[](void* object, hipStream_t st) { ((glu_radix_sort_s*) object)->mark(st, true); }, s};
                // (keys-only sorts: vbuf[] holds null pointers)
                const auto finish = vals ? (key_xf != KEY_XF_NONE ? launch_finish<KeyT, true, true> : launch_finish<KeyT, true, false>)
                                         : (key_xf != KEY_XF_NONE ? launch_finish<KeyT, false, true> : launch_finish<KeyT, false, false>);
                GLU_TRY(finish(kbuf[0], vbuf[0], kbuf[1], vbuf[1], (const uint32_t*) s->finish_starts.ptr, finish_kpt, finish_last, finish_expected,
                               finish_top_bit - 16u, pa.plan, 2u, key_xf, stream, s->finish_rank_bits, (uint32_t*) s->finish_crowded.ptr, finish_marks,
                               s->last_narrow_offered ? (const uint16_t*) narrow_keys : (const uint16_t*) nullptr));
                if (finish_long_ok && !fork)
                    GLU_TRY(launch_long_run_passes_any<KeyT>(s, kbuf[0], vbuf[0], kbuf[1], vbuf[1], count, key_xf, stream));
            }
        }
        else
        {
            GLU_TRY(dispatch_pass<KeyT>(s, kbuf[cur], vbuf[cur], kbuf[cur ^ 1], vbuf[cur ^ 1], count, shift, bits, nullptr,
                                        stream, xform));
            cur ^= 1;
        }
    }
    s->cur_behind = false;
    if (fork)
    {
        // the side stream: (behind the ordinary passes) the segmented passes over long runs, beside the in-LDS pass; then it joins
        HIP_TRY(hipStreamWaitEvent(s->side, s->ev_fork2, 0));
        if (finish_long_ok) GLU_TRY(launch_long_run_passes_any<KeyT>(s, kbuf[0], vbuf[0], kbuf[1], vbuf[1], count, key_xf, s->side));
        HIP_TRY(side_join.join());
    }
    if (planned)
    {
        // the data is home unless an odd number of passes ran: decided and, if need be, copied on the device
        const dim3 grid((uint32_t) std::min<size_t>((count + 255) / 256, (size_t) g_dev.num_cus * 16));
        const auto finalize = vals ? radix_finalize_kernel<KeyT, true> : radix_finalize_kernel<KeyT, false>;
        hipLaunchKernelGGL(finalize, grid, dim3(256), 0, stream, kbuf[0], vbuf[0], (const KeyT*) kbuf[1], (const uint32_t*) vbuf[1],
                           (uint32_t) count, (const PassPlan*) s->plan.ptr, pass, finish_kpt ? 2u : 0u);
        HIP_TRY(hipGetLastError());
        return GLU_OK;
    }
    if (cur == 1)
    {
        // odd number of passes: the reference would leave the result in its private scratch (documented
        // deviation in glu_hip.h) -- bring it home
        HIP_TRY(hipMemcpyAsync(keys, kbuf[1], count * sizeof(KeyT), hipMemcpyDeviceToDevice, stream));
        if (vals) HIP_TRY(hipMemcpyAsync(vals, vbuf[1], count * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    }
    return GLU_OK;
}

// the reference's interface: num_steps 4-bit steps from bit 0 (0 or more than the key holds = the whole key,
// RadixSort.hpp:289,332)
template<typename KeyT>
glu_status glu_hip::host::sort_run(glu_radix_sort_s* s, KeyT* keys, uint32_t* vals, size_t count, size_t num_steps, hipStream_t stream,
                                   uint32_t key_xf)
{
    constexpr size_t kMaxSteps = sizeof(KeyT) * 2; // 4-bit steps: 8 for 32-bit keys
    const size_t steps = (num_steps == 0 || num_steps > kMaxSteps) ? kMaxSteps : num_steps;
    return sort_bits<KeyT>(s, keys, vals, count, 0u, (uint32_t) steps * 4, stream, key_xf);
}
// (the two key widths, for every unit that sorts: glu_sort_driver.hpp declares them extern)
template glu_status glu_hip::host::sort_bits<uint32_t>(glu_radix_sort_s*, uint32_t*, uint32_t*, size_t, uint32_t, uint32_t, hipStream_t, uint32_t);
template glu_status glu_hip::host::sort_bits<uint64_t>(glu_radix_sort_s*, uint64_t*, uint32_t*, size_t, uint32_t, uint32_t, hipStream_t, uint32_t);
template glu_status glu_hip::host::sort_run<uint32_t>(glu_radix_sort_s*, uint32_t*, uint32_t*, size_t, size_t, hipStream_t, uint32_t);
template glu_status glu_hip::host::sort_run<uint64_t>(glu_radix_sort_s*, uint64_t*, uint32_t*, size_t, size_t, hipStream_t, uint32_t);

// The switches of a sort object (tests, tuning, A/B runs): one table for glu_radix_sort_set_option and for the environment
// defaults glu_radix_sort_create reads (GLU_HIP_<NAME>).  Every field is documented where glu_radix_sort_s declares it.
namespace
{
struct SortOption
{
    const char* name;
    void (*set)(glu_radix_sort_s*, long long);
};
#define GLU_OPT(NAME, ...) {NAME, [](glu_radix_sort_s* s, long long v) { (void) v; __VA_ARGS__; }}
const SortOption kSortOptions[] = {
    GLU_OPT("DIGIT_BITS", if (v == 4 || v == 8) s->digit_bits = (uint32_t) v),
    GLU_OPT("SORT_BLOCKS", if (v > 0) s->max_blocks = (uint32_t) v),
    GLU_OPT("SORT_SMALL", s->force_small = v != 0),
    GLU_OPT("SORT_NO_SINGLE_BLOCK", s->no_single_block = v != 0),
    GLU_OPT("SORT_NO_FUSED_SCAN", s->no_fused_scan = v != 0),
    GLU_OPT("SORT_NO_PLAN", s->no_plan = v != 0),
    GLU_OPT("SORT_NO_LINES", s->no_lines = v != 0),
    GLU_OPT("SCRATCH_TUNE", s->tune_scratch = v != 0),
    GLU_OPT("SORT_PAIRS", s->pairs = v != 0),
    GLU_OPT("SORT_EQUAL_SHARES", s->equal_shares = v != 0),
    GLU_OPT("SORT_NO_BIT_SHORTCUT", s->no_bit_shortcut = v != 0),
    GLU_OPT("SORT_PAIR_MIN", s->pair_min = (size_t) v),
    GLU_OPT("SORT_LDS_FINISH", s->lds_finish = v != 0),
    GLU_OPT("SEG_LDS_FINISH", s->seg_finish = v != 0),
    GLU_OPT("SORT_LONG_RUNS", s->long_runs = v != 0),
    GLU_OPT("SORT_NARROW_HANDOFF", s->narrow_handoff = v != 0), // (decides an allocation: takes effect with the next prepare)
    GLU_OPT("SORT_DEVICE_TOP", s->device_top = v != 0),
    GLU_OPT("SORT_FORK", s->fork_behind = v != 0),
    GLU_OPT("SEG_SPLIT_MAX", s->seg_split_max = (uint32_t) std::min<long long>(std::max<long long>(v, 0), 3)),
    GLU_OPT("FINISH_RANK_BITS", if (v >= 8) s->finish_rank_bits = (uint32_t) v),
    GLU_OPT("SEG_SPLIT_MIN", s->seg_split_min = (uint32_t) std::min<long long>(std::max<long long>(v, 0), 3)),
    GLU_OPT("SEG_MAX_GEO", s->seg_max_geo = (uint32_t) std::min<long long>(std::max<long long>(v, 1), 5)),
    GLU_OPT("SEG_SPLIT_GEO", s->seg_split_geo = (uint32_t) std::min<long long>(std::max<long long>(v, 1), 4)),
    GLU_OPT("SORT_FINISH_MIN", s->finish_min = (size_t) v),
    GLU_OPT("SORT_FINISH_BACKOFF", s->feedback.finish_backoff = (uint32_t) std::max<long long>(0, v)),
    GLU_OPT("SORT_PAIR_UNIT_DIV", if (v >= 0) s->pair_unit_div = (uint32_t) v), // 0: no limit
    GLU_OPT("SORT_NT_STORES", s->nt_stores = v != 0),
    GLU_OPT("SORT_NT_MIN_BYTES", s->nt_min_bytes = (size_t) v),
    GLU_OPT("SORT_LARGE_MIN", s->large_min = (size_t) v),
};
#undef GLU_OPT

static_assert(kKeyXfNone == KEY_XF_NONE && kKeyXfSigned == KEY_XF_SIGNED && kKeyXfFloat == KEY_XF_FLOAT, "key_xf_of() speaks the kernels' KEY_XF_*");

// ---- what the entry points below share (which checks each makes, and in which order: the record of tests/test_gpu_refusals.py)

// The sort of whole keys of a key type (checked by the caller): the sort of its key width with its order transform.
glu_status sort_typed(glu_radix_sort_s* s, void* keys, uint32_t* vals, size_t count, int key_type, hipStream_t stream)
{
    const uint32_t xf = key_xf_of(key_type);
    return key_bytes_of(key_type) == 8 ? sort_run<uint64_t>(s, (uint64_t*) keys, vals, count, 0, stream, xf)
                                       : sort_run<uint32_t>(s, (uint32_t*) keys, vals, count, 0, stream, xf);
}

// glu_radix_sort_prepare, _prepare_u64 and _prepare_ex: the explicit prepare, which may place the scratch arrays by measurement
glu_status prepare_entry(glu_radix_sort sort, size_t count, size_t key_bytes, bool with_vals)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (key_bytes != 4 && key_bytes != 8) return fail(GLU_ERROR_INVALID_ARGUMENT, "key_bytes must be 4 or 8 (got %zu)", key_bytes);
    return sort_prepare(sort, count, key_bytes, with_vals, true);
}

// The sorts of whole keys in the caller's arrays.  WITH_VALS: the entry point takes values, and requires them.
template<typename KeyT, bool WITH_VALS>
glu_status run_ptr_entry(glu_radix_sort sort, KeyT* keys, uint32_t* vals, size_t count, size_t num_steps, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (count == 0) return GLU_OK; // an empty shard: nothing to sort, NULL arrays are fine (torch gives data_ptr() == 0)
    GLU_TRY(check_none_null({keys}, "Invalid key buffer"));
    if (WITH_VALS) GLU_TRY(check_none_null({vals}, "Invalid value buffer"));
    return sort_run<KeyT>(sort, keys, vals, count, num_steps, pick_stream(stream));
}

// The same in buffers of the registry, on the library's queue (RadixSort.hpp:275-276)
template<typename KeyT, bool WITH_VALS>
glu_status run_buffers_entry(glu_radix_sort sort, glu_buffer key_buffer, glu_buffer val_buffer, size_t count, size_t num_steps)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    Buffer k, v;
    GLU_TRY(lookup(key_buffer, k, "key buffer"));
    if (WITH_VALS) GLU_TRY(lookup(val_buffer, v, "value buffer"));
    if (count > 1 && (k.size / sizeof(KeyT) < count || (WITH_VALS && v.size / sizeof(uint32_t) < count)))
        return fail(GLU_ERROR_INVALID_ARGUMENT, "count %zu exceeds the %s buffer size", count, WITH_VALS ? "key/value" : "key");
    return sort_run<KeyT>(sort, (KeyT*) k.ptr, (uint32_t*) v.ptr, count, num_steps, g_dev.queue);
}

// Did the last sort on the object try to end in LDS?  (No plan yet: nothing was tried.)
bool last_sort_tried(const glu_radix_sort_s* s) { return s->plan.ptr && s->last_planned && s->last_finish_attempted; }

// The device's PassPlan of the last sort where it `ran_with` one, else zeros
glu_status read_device_plan(const glu_radix_sort_s* s, bool ran_with, PassPlan& host)
{
    memset(&host, 0, sizeof(host));
    if (ran_with) HIP_TRY(hipMemcpy(&host, s->plan.ptr, sizeof(host), hipMemcpyDeviceToHost));
    return GLU_OK;
}
} // namespace

// The ordinary typed sort as a linear chain on `stream`.  The sort's only fork is the side stream of a sort that tries to end in LDS
// (sort_bits: `fork`, switched by glu_radix_sort_s::fork_behind); whatever else is ever moved off the caller's queue has to ask
// fork_behind too, or this function's promise breaks.
glu_status glu_hip::host::sort_typed_one_queue(glu_radix_sort_s* s, void* keys, uint32_t* vals, size_t count, glu_key_type key_type,
                                               hipStream_t stream)
{
    const bool fork = s->fork_behind;
    s->fork_behind = false;
    const glu_status status = sort_typed(s, keys, vals, count, key_type, stream);
    s->fork_behind = fork;
    return status;
}

extern "C" {

glu_status glu_radix_sort_create(glu_radix_sort* out)
{
    // the process environment as DEFAULTS for new objects (GLU_HIP_<OPTION>=value, read here, when an object is created);
    // programs and tests set options on the object: glu_radix_sort_set_option
    return create_object(out, [](glu_radix_sort_s& s) {
        for (const SortOption& o : kSortOptions)
        {
            char name[96];
            snprintf(name, sizeof(name), "GLU_HIP_%s", o.name);
            if (const char* e = glu_env(name)) o.set(&s, atoll(e));
        }
        return GLU_OK;
    });
}

// the object may last have been used on a caller's stream (the *_ptr entry points): destroy_object drains the device, not only the
// library queue, before everything the object owns goes away (RAII of the reference: RadixSort.hpp:194-200, gl_utils.hpp:184-188)
glu_status glu_radix_sort_destroy(glu_radix_sort sort) { return destroy_object(sort); }

glu_status glu_radix_sort_prepare(glu_radix_sort sort, size_t count) { return prepare_entry(sort, count, sizeof(uint32_t), true); }

glu_status glu_radix_sort_prepare_ex(glu_radix_sort sort, size_t count, size_t key_bytes, int with_vals) { return prepare_entry(sort, count, key_bytes, with_vals != 0); }

glu_status glu_radix_sort_prepare_u64(glu_radix_sort sort, size_t count) { return prepare_entry(sort, count, sizeof(uint64_t), true); }

glu_status glu_radix_sort_run_ptr(glu_radix_sort sort, uint32_t* keys, uint32_t* vals, size_t count, size_t num_steps, void* stream)
{
    return run_ptr_entry<uint32_t, true>(sort, keys, vals, count, num_steps, stream);
}

glu_status glu_radix_sort_run_u64_ptr(glu_radix_sort sort, uint64_t* keys, uint32_t* vals, size_t count, size_t num_steps, void* stream)
{
    return run_ptr_entry<uint64_t, true>(sort, keys, vals, count, num_steps, stream);
}

glu_status glu_radix_sort_run_keys_ptr(glu_radix_sort sort, uint32_t* keys, size_t count, size_t num_steps, void* stream)
{
    return run_ptr_entry<uint32_t, false>(sort, keys, nullptr, count, num_steps, stream);
}

glu_status glu_radix_sort_run_keys_u64_ptr(glu_radix_sort sort, uint64_t* keys, size_t count, size_t num_steps, void* stream)
{
    return run_ptr_entry<uint64_t, false>(sort, keys, nullptr, count, num_steps, stream);
}

glu_status glu_radix_sort_run(glu_radix_sort sort, glu_buffer key_buffer, glu_buffer val_buffer, size_t count, size_t num_steps)
{
    return run_buffers_entry<uint32_t, true>(sort, key_buffer, val_buffer, count, num_steps);
}

glu_status glu_radix_sort_run_u64(glu_radix_sort sort, glu_buffer key_buffer, glu_buffer val_buffer, size_t count, size_t num_steps)
{
    return run_buffers_entry<uint64_t, true>(sort, key_buffer, val_buffer, count, num_steps);
}

glu_status glu_radix_sort_run_keys(glu_radix_sort sort, glu_buffer key_buffer, size_t count, size_t num_steps)
{
    return run_buffers_entry<uint32_t, false>(sort, key_buffer, 0, count, num_steps);
}

glu_status glu_radix_sort_run_typed_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t count, glu_key_type key_type, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    GLU_TRY(check_key_type(key_type));
    if (count == 0) return GLU_OK;
    GLU_TRY(check_none_null({keys}, "Invalid key buffer"));
    return sort_typed(sort, keys, vals, count, key_type, pick_stream(stream));
}

glu_status glu_radix_sort_run_bit_range_ptr(glu_radix_sort sort, void* keys, uint32_t* vals, size_t count, uint32_t key_bits,
                                            uint32_t begin_bit, uint32_t end_bit, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (key_bits != 32 && key_bits != 64) return fail(GLU_ERROR_INVALID_ARGUMENT, "key_bits must be 32 or 64 (got %u)", key_bits);
    if (begin_bit > end_bit || end_bit > key_bits)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "bad bit range [%u, %u) for %u-bit keys", begin_bit, end_bit, key_bits);
    if (count == 0) return GLU_OK;
    GLU_TRY(check_none_null({keys}, "Invalid key buffer"));
    hipStream_t st = pick_stream(stream);
    if (key_bits == 32) return sort_bits<uint32_t>(sort, (uint32_t*) keys, vals, count, begin_bit, end_bit, st);
    return sort_bits<uint64_t>(sort, (uint64_t*) keys, vals, count, begin_bit, end_bit, st);
}

glu_status glu_radix_sort_partition_ptr(glu_radix_sort sort, const uint32_t* src_keys, const uint32_t* src_vals,
                                        uint32_t* dst_keys, uint32_t* dst_vals, size_t count, uint32_t shift,
                                        uint32_t bits, uint32_t* digit_histogram, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (count > 0)
    {
        GLU_TRY(check_none_null({src_keys, src_vals, dst_keys, dst_vals}, "NULL array"));
        if (src_keys == dst_keys || src_vals == dst_vals)
            return fail(GLU_ERROR_INVALID_ARGUMENT, "partition needs distinct source and destination");
    }
    if (bits < 1 || bits > 8 || shift + bits > 32) return fail(GLU_ERROR_INVALID_ARGUMENT, "bad digit: shift %u bits %u", shift, bits);
    if (count > 0xFFFF0000ull) return fail(GLU_ERROR_INVALID_ARGUMENT, "count %zu does not fit 32-bit indexing", count);
    hipStream_t st = pick_stream(stream);
    if (count == 0)
    {
        if (digit_histogram) HIP_TRY(hipMemsetAsync(digit_histogram, 0, ((size_t) 1 << bits) * 4, st));
        return GLU_OK;
    }
    // table only (no key/val scratch needed)
    uint64_t cap = (uint64_t) g_dev.num_cus * kMaxBlocksPerCu;
    GLU_TRY(sort->table.reserve((kMaxRadix * cap + kMaxRadix) * sizeof(uint32_t)));
    return dispatch_pass<uint32_t>(sort, src_keys, src_vals, dst_keys, dst_vals, count, shift, bits, digit_histogram, st);
}

glu_status glu_radix_sort_set_digit_bits(glu_radix_sort sort, uint32_t bits)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (bits != 4 && bits != 8) return fail(GLU_ERROR_INVALID_ARGUMENT, "digit bits must be 4 or 8 (got %u)", bits);
    sort->digit_bits = bits;
    return GLU_OK;
}

glu_status glu_radix_sort_set_option(glu_radix_sort sort, const char* name, long long value)
{
    GLU_TRY(enter());
    GLU_TRY(check_none_null({sort, name}, "sort / name is NULL"));
    if (strncasecmp(name, "GLU_HIP_", 8) == 0) name += 8; // (the environment's spelling is accepted)
    for (const SortOption& o : kSortOptions)
        if (strcasecmp(name, o.name) == 0)
        {
            o.set(sort, value);
            return GLU_OK;
        }
    return fail(GLU_ERROR_INVALID_ARGUMENT, "no such option: %s", name);
}

glu_status glu_radix_sort_get_digit_bits(glu_radix_sort sort, uint32_t* bits)
{
    GLU_TRY(enter());
    GLU_TRY(check_none_null({sort, bits}, "NULL argument"));
    store(bits, sort->digit_bits);
    return GLU_OK;
}

glu_status glu_radix_sort_set_profiling(glu_radix_sort sort, int enable)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    sort->profiling = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    if (!enable) sort->clear_marks();
    return GLU_OK;
}

glu_status glu_radix_sort_read_plan(glu_radix_sort sort, uint32_t* skipped, uint32_t* counted_alone, uint32_t* pair_role, size_t passes)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (passes > (size_t) kPlanMaxPasses) return fail(GLU_ERROR_INVALID_ARGUMENT, "at most %d passes", kPlanMaxPasses);
    if (!sort->plan.ptr) return fail(GLU_ERROR_INVALID_STATE, "no sort has run on this object");
    // a sort below 2^22 elements runs without a device-side plan: every pass ran, none was paired
    PassPlan host;
    GLU_TRY(read_device_plan(sort, sort->last_planned, host));
    // a sort that tried to end in LDS has its two top-bit passes in front of the ordinary ones, which are what this call
    // reports (glu_radix_sort_read_finish tells which of the two sequences ran)
    const size_t first = last_sort_tried(sort) ? 2 : 0;
    for (size_t p = 0; p < passes; p++)
    {
        const bool have = first + p < (size_t) kPlanMaxPasses;
        if (skipped) skipped[p] = have ? host.skip[first + p] : 0u;
        if (counted_alone) counted_alone[p] = have ? host.pair_fallback[first + p] : 0u;
        if (pair_role) pair_role[p] = sort->last_planned && have ? sort->last_pair_roles[first + p] : 0u;
    }
    return GLU_OK;
}

glu_status glu_radix_sort_plan_finish(size_t count, uint32_t key_bytes, uint32_t* first_capacity, uint32_t* last_capacity)
{
    // host only (no device needed): which tiles of the in-LDS pass a whole-key sort of `count` elements would enqueue by default
    if (key_bytes != 4 && key_bytes != 8) return fail(GLU_ERROR_INVALID_ARGUMENT, "key_bytes must be 4 or 8 (got %u)", key_bytes);
    uint32_t first = 0, last = 0;
    if (count >= finish_min_count(key_bytes) && count >= kPlanMinCount && count <= 0xFFFF0000ull)
    {
        first = finish_geometry_for(count);
        last = first ? std::min<uint32_t>(first + 2, kFinishGeometries) : 0u;
    }
    store(first_capacity, finish_geometry_capacity(first));
    store(last_capacity, finish_geometry_capacity(last));
    return GLU_OK;
}

glu_status glu_radix_sort_read_long_runs(glu_radix_sort sort, uint32_t* runs, uint32_t* sub_blocks, uint32_t* pairs)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    uint32_t hdr[3] = {0, 0, 0};
    if (last_sort_tried(sort) && sort->last_finish_long_ok && sort->long_hdr.ptr)
        HIP_TRY(hipMemcpy(hdr, sort->long_hdr.ptr, sizeof(hdr), hipMemcpyDeviceToHost));
    store(runs, hdr[0]);
    store(sub_blocks, hdr[1]);
    store(pairs, hdr[2]);
    return GLU_OK;
}

glu_status glu_radix_sort_read_finish(glu_radix_sort sort, uint32_t* attempted, uint32_t* accepted, uint32_t* longest_run,
                                      uint32_t* capacity, uint32_t* top_bit)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    const bool tried = last_sort_tried(sort);
    PassPlan host;
    GLU_TRY(read_device_plan(sort, tried, host));
    store(attempted, tried ? 1u : 0u);
    store(accepted, tried && host.finish ? 1u : 0u);
    store(longest_run, tried ? host.finish_longest : 0u);
    if (tried && sort->last_device_top && host.top_bit) sort->last_finish_top = host.top_bit; // (chosen on the device)
    // the tile the device chose; refused: the largest one that was enqueued
    store(capacity, !tried ? 0u : host.finish ? finish_geometry_capacity(host.finish) : sort->last_finish_capacity);
    store(top_bit, tried ? sort->last_finish_top : 0u);
    return GLU_OK;
}

// Which hand-off between the second top-bit scatter and the in-LDS pass the last sort took: narrow = 1: 2-byte keys in the object's
// side array (PassPlan::narrow); 0: whole keys in the key array, or the sort did not end in LDS.
glu_status glu_radix_sort_read_handoff(glu_radix_sort sort, uint32_t* narrow)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    const bool offered = last_sort_tried(sort) && sort->last_narrow_offered;
    PassPlan host;
    GLU_TRY(read_device_plan(sort, offered, host));
    store(narrow, offered && host.finish && host.narrow ? 1u : 0u);
    return GLU_OK;
}

// Sums the recorded intervals.  Sorts that tried to end in LDS (radix_lds_finish.hpp) enqueue two sequences of passes, one of
// which returns at once; which one is read from the plan of the LAST sort and assumed for every sort since the previous
// read.  Booked are the passes that did the work: accepted -- the two top-bit passes (count / scan / scatter) and the in-LDS
// pass (finish_ms); refused -- the ordinary passes, plus the count interval of the first top-bit pass (the price of asking).
glu_status glu_radix_sort_read_profile_finish(glu_radix_sort sort, double* count_ms, double* scan_ms, double* scatter_ms,
                                              uint64_t* passes, double* finish_ms, uint64_t* finish_passes)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    double acc[3] = {0, 0, 0}, fin = 0;
    uint64_t live = 0, fin_n = 0;
    const size_t n = sort->slots.size() / 4;
    if (sort->events_used > 0) HIP_TRY(hipEventSynchronize(sort->events[sort->events_used - 1]));
    PassPlan host;
    GLU_TRY(read_device_plan(sort, last_sort_tried(sort), host));
    const bool last_accepted = host.finish != 0;
    // the outcome of every attempt of the window, by attempt number (a window of more than 256 sorts: the older ones by the last)
    // (words 256 .. 511: attempt number << 1 | the sort took the narrow hand-off)
    std::vector<uint32_t> ring(512, 0u);
    const bool have_ring = sort->finish_outcomes.ptr != nullptr;
    if (have_ring) HIP_TRY(hipMemcpy(ring.data(), sort->finish_outcomes.ptr, 512 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool seg_tried = false;
    uint32_t seg_longest = 0;
    GLU_TRY(read_seg_gate(sort, seg_tried, seg_longest));
    const bool seg_accepted = seg_tried && seg_longest <= sort->last_seg_finish_capacity;
    for (size_t p = 0; p < n; p++)
    {
        float ms[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; k++) // (light profiling: an interval without both of its events reads as zero)
            if (sort->slots[p * 4 + k] && sort->slots[p * 4 + k + 1])
                HIP_TRY(hipEventElapsedTime(&ms[k], sort->slots[p * 4 + k], sort->slots[p * 4 + k + 1]));
        const uint8_t kind = p < sort->pass_kinds.size() ? sort->pass_kinds[p] : 0;
        const uint32_t seq = p < sort->pass_seqs.size() ? sort->pass_seqs[p] : 0u;
        // (this pass's sort: accepted?  ring entry = attempt number << 3 | tile geometry)
        bool accepted = last_accepted;
        if (seq && have_ring && (ring[seq & 255u] >> 3) == seq) accepted = (ring[seq & 255u] & 7u) != 0u;
        const bool attempted = seq != 0 || sort->last_finish_attempted;
        // (light profiling records no events around the sequence the host expects not to run: such a pass is not a live pass with
        // zero time, whatever the device then decided)
        const bool timed = sort->slots[p * 4 + 2] && sort->slots[p * 4 + 3];
        // (the second top-bit scatter in two forms: the interval of the form that moved the data, by this sort's hand-off)
        if (timed && p < sort->between_forms.size() && sort->between_forms[p])
        {
            bool narrow = host.narrow != 0u;
            if (seq && have_ring && (ring[256u + (seq & 255u)] >> 1) == seq) narrow = (ring[256u + (seq & 255u)] & 1u) != 0u;
            if (narrow)
                HIP_TRY(hipEventElapsedTime(&ms[2], sort->between_forms[p], sort->slots[p * 4 + 3]));
            else
                HIP_TRY(hipEventElapsedTime(&ms[2], sort->slots[p * 4 + 2], sort->between_forms[p]));
        }
        if (kind == 2)
        {
            if (accepted || seg_accepted) fin += ms[2], fin_n++;
            continue;
        }
        if (kind == 3 && !seg_accepted)
        {
            acc[0] += ms[0], acc[1] += ms[1]; // its count and scan ran before the device said no
            continue;
        }
        if (kind == 4 && seg_accepted) continue; // the sequence not taken
        if (kind == 1 && !accepted)
        {
            acc[0] += ms[0]; // the leader's count kernel ran before the device said no
            continue;
        }
        if (kind == 0 && accepted && attempted) continue; // the sequence not taken
        if (!timed && sort->profiling == 2) continue;
        for (int k = 0; k < 3; k++) acc[k] += ms[k];
        live++;
    }
    sort->clear_marks();
    store(count_ms, acc[0]);
    store(scan_ms, acc[1]);
    store(scatter_ms, acc[2]);
    store(passes, live);
    store(finish_ms, fin);
    store(finish_passes, fin_n);
    return GLU_OK;
}

glu_status glu_radix_sort_read_profile(glu_radix_sort sort, double* count_ms, double* scan_ms, double* scatter_ms, uint64_t* passes)
{
    return glu_radix_sort_read_profile_finish(sort, count_ms, scan_ms, scatter_ms, passes, nullptr, nullptr);
}

// (the one entry point that does not ask for the device: it reads host fields only)
glu_status glu_radix_sort_scratch_placement(glu_radix_sort sort, uint32_t* candidates, double* chosen_ms, double* slowest_ms)
{
    GLU_TRY(check_not_null(sort, "sort"));
    store(candidates, sort->tuned_candidates);
    store(chosen_ms, sort->tuned_ms);
    store(slowest_ms, sort->tuned_worst_ms);
    return GLU_OK;
}

glu_status glu_radix_sort_scratch_size(glu_radix_sort sort, size_t* bytes)
{
    GLU_TRY(enter());
    GLU_TRY(check_none_null({sort, bytes}, "NULL argument"));
    size_t sum = 0;
    sort->for_each_scratch([&](const Scratch& sc) { sum += sc.size; });
    store(bytes, sum);
    return GLU_OK;
}

} // extern "C"
