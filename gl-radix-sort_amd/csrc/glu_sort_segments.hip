// glu_sort_segments.hip -- the segmented passes of libglu_hip.so (radix_seg_passes.hpp and the SEG = true line scatter): the passes
// over the long runs of a whole-key sort that ends in LDS, and the segmented sort -- glu_radix_sort_run_segments_ptr,
// glu_radix_sort_plan_segments, glu_radix_sort_read_seg_finish.  Its host arithmetic is seg_plan.hpp, plain C++.  Both launchers
// live here because they share kernel instantiations, which one translation unit must emit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "glu_host.hpp"
#include "glu_sort_driver.hpp"
#include "glu_sort_launch.hpp"
#include "radix_sort_kernels.hpp"
#include "radix_scatter_lines.hpp"
#include "radix_seg_passes.hpp"
#include "radix_lds_plan.hpp"

using namespace glu_hip;
using namespace glu_hip::host;

namespace
{
// The segmented passes over the LONG runs of a whole-key sort that ends in LDS (radix_finish_long_runs_kernel built their
// descriptors; hdr[0] = 0: there are none, or the sort was refused -- every kernel returns at once): key bits [0, 8) from the
// arrays that hold the data (PassPlan::flip[2], known on the device) into the other pair, bits [8, 16) back -- 4-byte keys.
// Round 6: 8-byte keys (six passes: up to 48 bits are left below the runs' bits), keys-only sorts, typed keys (the last pass
// decodes on store what the first top-bit pass encoded on load: the in-LDS pass, which does that for the other runs, leaves these alone).
template<typename KeyT, bool VALS, bool XF>
glu_status launch_long_run_passes(glu_radix_sort_s* s, KeyT* a_k, uint32_t* a_v, KeyT* b_k, uint32_t* b_v, size_t count, uint32_t key_xf,
                                  hipStream_t stream)
{
    using G = typename std::conditional<sizeof(KeyT) == 4 && VALS, SegLinesGeometry, LinesGeometry<KeyT, 8, VALS>>::type;
    constexpr int RADIX = 256;
    constexpr int RS = (G::KPT + 2) / 3;
    constexpr uint32_t kPasses = sizeof(KeyT) == 4 ? 2u : 6u; // (an even number: the runs come home)
    using Smem = LineSmem<KeyT, 8, G::THREADS, G::KPT, VALS>;
    auto scatter = radix_scatter_lines_kernel<KeyT, 8, G::THREADS, G::KPT, XF, VALS, 0, false, RS, true, true, 0, true>;
    static std::once_flag lds_opt_in;
    static hipError_t lds_opt_in_result = hipSuccess;
    std::call_once(lds_opt_in, [&] {
        lds_opt_in_result = hipFuncSetAttribute((const void*) scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int) sizeof(Smem));
    });
    HIP_TRY(lds_opt_in_result);
    // (kLongRunsSharesPerWg shares per workgroup, dealt round-robin: what is left of the long runs once those of one key value have
    // been emptied is spread over the chip)
    const uint32_t nwg = usable_cus(s), shares = nwg * kLongRunsSharesPerWg;
    const LongRunsLayout lay(shares);
    const uint32_t* image = (const uint32_t*) s->long_image.ptr;
    const uint32_t* hdr = (const uint32_t*) s->long_hdr.ptr;
    uint32_t* table = (uint32_t*) s->table.ptr;
    const PassPlan* plan = (const PassPlan*) s->plan.ptr;
    // (the first pass's count kernel also notes OR / AND of every sub-block's keys, its scan kernel empties the segments whose keys
    // agree on all the ordered bits: a long run of one key value -- every long run of a duplicate-heavy input -- stays where it is)
    KeyT* const sub_or = (KeyT*) s->long_bits.ptr;
    KeyT* const sub_and = sub_or + (kLongRunsMax + shares);
    for (uint32_t p = 0; p < kPasses; p++)
    {
        // (not typed keys: their long runs have to pass through the last pass, which decodes them)
        if (p == 0 && !XF)
        {
            hipLaunchKernelGGL((radix_seg_count_kernel<KeyT, 8, 1024, true>), dim3(nwg), dim3(1024), 0, stream, (const KeyT*) a_k, (const uint2*) image,
                               image + lay.off_first, table, 0u, 255u, hdr, 0u, kSegGateIfNot, (const KeyT*) b_k, plan, 2u, 0u, sub_or, sub_and, hdr + 3);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((radix_seg_scan_kernel<RADIX, KeyT>), dim3(512), dim3(RADIX), 0, stream, table, image + lay.off_list,
                               image + lay.off_start, hdr, 0u, kSegGateIfNot, hdr, (uint2*) const_cast<uint32_t*>(image), (const KeyT*) sub_or,
                               (const KeyT*) sub_and, plan, (uint32_t) (8 * sizeof(KeyT) - 16));
            HIP_TRY(hipGetLastError());
        }
        else
        {
            hipLaunchKernelGGL((radix_seg_count_kernel<KeyT, 8, 1024>), dim3(nwg), dim3(1024), 0, stream, (const KeyT*) a_k, (const uint2*) image,
                               image + lay.off_first, table, p * 8u, 255u, hdr, 0u, kSegGateIfNot, (const KeyT*) b_k, plan, 2u, p, (KeyT*) nullptr, (KeyT*) nullptr, hdr + 3);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((radix_seg_scan_kernel<RADIX>), dim3(512), dim3(RADIX), 0, stream, table, image + lay.off_list,
                               image + lay.off_start, hdr, 0u, kSegGateIfNot, hdr); // (workgroups loop over the device-counted segments)
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(scatter, dim3(nwg), dim3(G::THREADS), sizeof(Smem), stream, (const KeyT*) a_k, (const uint32_t*) a_v, b_k, b_v,
                           (const uint32_t*) table, (const uint32_t*) nullptr, (uint32_t) count, p * 8u, 255u, 0u, (unsigned long long*) nullptr,
                           XF && p + 1 == kPasses ? key_xf << 2 : 0u, const_cast<PassPlan*>(plan), 2u, (const uint2*) image, p,
                           image + lay.off_first, hdr, 0u, kSegGateIfNot, hdr + 3, (uint16_t*) nullptr);
        HIP_TRY(hipGetLastError());
    }
    return GLU_OK;
}

constexpr uint64_t kSegFinishMaxRuns = 1u << 18; // a segmented sort tries to end in LDS with up to this many runs (1024 segments)

// One segmented pass on the 8-bit digit at `shift`: count per sub-block, scan per segment, line scatter over sub-blocks.
// gate_mode (radix_seg_passes.hpp): kSegGateIfNot = a pass of the ordinary sequence enqueued behind an attempt to end in LDS;
// kSegGateIfFits + runs_end != 0 = the first pass of such an attempt: its count and scan kernels always run, the runs kernel
// behind them writes the run starts and the longest run (the gate), the scatter runs if that fits `gate_cap`.
glu_status launch_seg_pass(glu_radix_sort_s* s, const uint32_t* src_k, const uint32_t* src_v, uint32_t* dst_k, uint32_t* dst_v,
                           size_t count, uint32_t shift, const uint32_t* image, const SegImage& img, hipStream_t stream,
                           uint32_t gate_mode = kSegGateNone, uint32_t gate_cap = 0, uint32_t runs_end = 0)
{
    const uint32_t* gate = gate_mode != kSegGateNone ? (const uint32_t*) s->seg_gate.ptr : nullptr;
    const bool attempt = gate_mode == kSegGateIfFits;
    const uint32_t gm_count = attempt ? kSegGateNone : gate_mode; // (the attempt's count and scan make the decision)
    using G = SegLinesGeometry;
    constexpr int RADIX = 256;
    constexpr int RS = (G::KPT + 2) / 3;
    using Smem = LineSmem<uint32_t, 8, G::THREADS, G::KPT, true>;
    auto scatter_nt = radix_scatter_lines_kernel<uint32_t, 8, G::THREADS, G::KPT, false, true, 0, false, RS, true, true, 0, true>;
    auto scatter_plain = radix_scatter_lines_kernel<uint32_t, 8, G::THREADS, G::KPT, false, true, 0, false, RS, true, false, 0, true>;
    static std::once_flag lds_opt_in;
    static hipError_t lds_opt_in_result = hipSuccess;
    std::call_once(lds_opt_in, [&] {
        lds_opt_in_result = hipFuncSetAttribute((const void*) scatter_nt, hipFuncAttributeMaxDynamicSharedMemorySize, (int) sizeof(Smem));
        if (lds_opt_in_result == hipSuccess)
            lds_opt_in_result = hipFuncSetAttribute((const void*) scatter_plain, hipFuncAttributeMaxDynamicSharedMemorySize, (int) sizeof(Smem));
    });
    HIP_TRY(lds_opt_in_result);
    uint32_t* table = (uint32_t*) s->table.ptr;
    const uint2* subs = (const uint2*) image;
    s->mark(stream);
    hipLaunchKernelGGL((radix_seg_count_kernel<uint32_t, 8, 1024>), dim3(img.nwg), dim3(1024), 0, stream, src_k, subs, image + img.off_first, table,
                       shift, 255u, gate, gate_cap, gm_count, (const uint32_t*) nullptr, (const PassPlan*) nullptr, 0u, 0u);
    HIP_TRY(hipGetLastError());
    s->mark(stream);
    hipLaunchKernelGGL((radix_seg_scan_kernel<RADIX>), dim3(img.nseg), dim3(RADIX), 0, stream, table, image + img.off_list,
                       image + img.off_start, gate, gate_cap, gm_count, (const uint32_t*) nullptr);
    HIP_TRY(hipGetLastError());
    if (attempt)
    {
        hipLaunchKernelGGL((radix_seg_runs_kernel<RADIX>), dim3(1), dim3(1024), 0, stream, (const uint32_t*) table, image + img.off_list,
                           image + img.off_start, img.nseg, runs_end, (uint32_t*) s->finish_starts.ptr, (uint32_t*) s->seg_gate.ptr);
        HIP_TRY(hipGetLastError());
    }
    s->mark(stream, true);
    hipLaunchKernelGGL(s->nt_stores ? scatter_nt : scatter_plain, dim3(img.nwg), dim3(G::THREADS), sizeof(Smem), stream, src_k, src_v,
                       dst_k, dst_v, (const uint32_t*) table, (const uint32_t*) nullptr, (uint32_t) count, shift, 255u, 0u,
                       (unsigned long long*) nullptr, 0u, (PassPlan*) nullptr, 0u, subs, 0u, image + img.off_first, gate, gate_cap, gate_mode, (const uint32_t*) nullptr,
                       (uint16_t*) nullptr);
    HIP_TRY(hipGetLastError());
    s->mark(stream, true);
    return GLU_OK;
}

// The piece arrays of a segmented call as SegPieces, and the elements they hold together.  Piece by piece: it names a segment below
// num_segments and, where the call has a count (glu_radix_sort_run_segments_ptr; the plan has none: nullptr), lies inside [0, *count).
glu_status read_pieces(const uint64_t* piece_begin, const uint64_t* piece_len, const uint32_t* piece_segment, size_t num_pieces,
                       uint32_t num_segments, const size_t* count, std::vector<SegPiece>& pieces, uint64_t& total)
{
    pieces.resize(num_pieces);
    total = 0;
    for (size_t i = 0; i < num_pieces; i++)
    {
        if (piece_segment[i] >= num_segments) return fail(GLU_ERROR_INVALID_ARGUMENT, "piece %zu names segment %u of %u", i, piece_segment[i], num_segments);
        if (count && (piece_begin[i] > *count || piece_len[i] > *count - piece_begin[i]))
            return fail(GLU_ERROR_INVALID_ARGUMENT, "piece %zu [%llu, +%llu) exceeds count %zu", i, (unsigned long long) piece_begin[i],
                        (unsigned long long) piece_len[i], *count);
        pieces[i] = SegPiece{piece_begin[i], piece_len[i], piece_segment[i]};
        total += piece_len[i];
    }
    return GLU_OK;
}
} // namespace

template<typename KeyT>
glu_status glu_hip::host::launch_long_run_passes_any(glu_radix_sort_s* s, KeyT* a_k, uint32_t* a_v, KeyT* b_k, uint32_t* b_v, size_t count,
                                                     uint32_t key_xf, hipStream_t stream)
{
    if (a_v) return key_xf != KEY_XF_NONE ? launch_long_run_passes<KeyT, true, true>(s, a_k, a_v, b_k, b_v, count, key_xf, stream)
                                          : launch_long_run_passes<KeyT, true, false>(s, a_k, a_v, b_k, b_v, count, key_xf, stream);
    return key_xf != KEY_XF_NONE ? launch_long_run_passes<KeyT, false, true>(s, a_k, nullptr, b_k, nullptr, count, key_xf, stream)
                                 : launch_long_run_passes<KeyT, false, false>(s, a_k, nullptr, b_k, nullptr, count, key_xf, stream);
}
template glu_status glu_hip::host::launch_long_run_passes_any<uint32_t>(glu_radix_sort_s*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, size_t,
                                                                        uint32_t, hipStream_t);
template glu_status glu_hip::host::launch_long_run_passes_any<uint64_t>(glu_radix_sort_s*, uint64_t*, uint32_t*, uint64_t*, uint32_t*, size_t,
                                                                        uint32_t, hipStream_t);

// ------------------------------------------------------------------------------------------------------------
// segmented sort (radix_seg_passes.hpp): glu_radix_sort_run_segments_ptr
// ------------------------------------------------------------------------------------------------------------
void glu_hip::host::seg_make_plan(glu_radix_sort_s* s, std::vector<SegPiece>&& pieces, uint32_t nseg, size_t count, uint32_t bits,
                                  bool aligned, SegPlan& plan, uint64_t origin)
{
    plan.pieces = std::move(pieces);
    plan.nseg = nseg;
    plan.count = count;
    plan.bits = bits;
    plan.passes = bits / 8;
    seg_order_pieces(plan.pieces, nseg, origin, plan.seg_start);
    plan.by_copies = count < kSegMinCount || !aligned || plan.passes == 0;
    if (plan.by_copies) return;
    // descriptors of the first pass (the caller's pieces) and of the later ones (whole segments of the pass before)
    const uint32_t nwg = usable_cus(s);
    seg_build_image(plan.pieces.data(), plan.pieces.size(), nseg, plan.seg_start.data(), count, nwg, plan.first);
    if (plan.passes > 1)
    {
        std::vector<SegPiece> whole(nseg);
        for (uint32_t g = 0; g < nseg; g++) whole[g] = SegPiece{plan.seg_start[g], plan.seg_start[g + 1] - plan.seg_start[g], g};
        seg_build_image(whole.data(), whole.size(), nseg, plan.seg_start.data(), count, nwg, plan.later);
    }
}

// (here, not in seg_plan.hpp: it asks the in-LDS pass's tile geometries)
bool glu_hip::host::seg_finish_choice_for(const glu_radix_sort_s* s, uint32_t passes, uint32_t bits, uint64_t nruns, uint64_t largest,
                                          uint32_t& geo, uint32_t& split_log2)
{
    geo = 0, split_log2 = 0;
    if (!(s->seg_finish && s->lds_finish && passes >= 2 && bits == passes * 8 && nruns <= kSegFinishMaxRuns)) return false;
    split_log2 = std::min(s->seg_split_min, s->seg_split_max);
    for (; split_log2 <= s->seg_split_max && !geo; split_log2++)
    {
        geo = finish_geometry_for((size_t) (largest >> split_log2), 256u, std::min(s->seg_max_geo, kSegFinishGeometries));
        if (split_log2 > 0 && geo > s->seg_split_geo) geo = 0; // (split runs take the tiles that share a CU four at a time)
    }
    if (!geo) return false;
    split_log2--;
    return true;
}
bool glu_hip::host::seg_finish_choice(const glu_radix_sort_s* s, const SegPlan& plan, uint32_t& geo, uint32_t& split_log2)
{
    uint64_t largest = 0;
    for (uint32_t g = 0; g < plan.nseg; g++) largest = std::max<uint64_t>(largest, plan.seg_start[g + 1] - plan.seg_start[g]);
    return seg_finish_choice_for(s, plan.passes, plan.bits, (uint64_t) plan.nseg * 256u, largest, geo, split_log2);
}

glu_status glu_hip::host::seg_run_plan(glu_radix_sort_s* s, const SegPlan& plan, uint32_t* in_k, uint32_t* in_v, uint32_t* out_k,
                                       uint32_t* out_v, hipStream_t stream)
{
    const size_t count = plan.count;
    const uint32_t passes = plan.passes, nseg = plan.nseg;
    s->cur_kind = 0, s->cur_behind = false, s->cur_seq = 0; // (whatever an earlier call that failed half-way left)
    // (the scratch arrays are indexed like `out`: a plan with an origin -- a group of a sharded sort's rounds -- reaches further)
    GLU_TRY(sort_prepare(s, (plan.seg_start.empty() ? 0 : (size_t) plan.seg_start[0]) + count, sizeof(uint32_t), true));
    if (plan.by_copies)
    {
        // small (or unaligned, or nothing to sort by): lay the segments out with copies, then one sort per segment
        uint64_t at = plan.seg_start.empty() ? 0 : plan.seg_start[0];
        for (const SegPiece& pc : plan.pieces)
        {
            if (pc.len == 0) continue;
            HIP_TRY(hipMemcpyAsync(out_k + at, in_k + pc.begin, pc.len * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(out_v + at, in_v + pc.begin, pc.len * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
            at += pc.len;
        }
        if (passes)
            for (uint32_t g = 0; g < nseg; g++)
            {
                const uint64_t len = plan.seg_start[g + 1] - plan.seg_start[g];
                if (len > 1)
                    GLU_TRY(sort_bits<uint32_t>(s, out_k + plan.seg_start[g], out_v + plan.seg_start[g], (size_t) len, 0u, plan.bits, stream));
            }
        return GLU_OK;
    }
    uint32_t* tmp_k = (uint32_t*) s->keys.ptr;
    uint32_t* tmp_v = (uint32_t*) s->vals.ptr;
    const SegImage &first = plan.first, &later = plan.later;
    const size_t bytes = (first.words.size() + later.words.size()) * sizeof(uint32_t);
    GLU_TRY(s->seg_desc.reserve(std::max<size_t>(bytes, 1 << 16)));
    GLU_TRY(s->table.reserve((size_t) std::max(first.nsb, later.nsb) * 256 * sizeof(uint32_t)));
    glu_radix_sort_s::SegStage& st = s->seg_stage[s->seg_stage_next++ % 16];
    if (st.in_flight) HIP_TRY(hipEventSynchronize(st.copied)); // (sixteen calls ago: long done)
    if (st.size < bytes)
    {
        if (st.host) HIP_TRY(hipHostFree(st.host));
        st.host = nullptr;
        st.size = 0;
        HIP_TRY(hipHostMalloc(&st.host, std::max<size_t>(bytes, 1 << 16)));
        st.size = std::max<size_t>(bytes, 1 << 16);
    }
    if (!st.copied) HIP_TRY(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    memcpy(st.host, first.words.data(), first.words.size() * sizeof(uint32_t));
    if (!later.words.empty())
        memcpy((uint32_t*) st.host + first.words.size(), later.words.data(), later.words.size() * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(s->seg_desc.ptr, st.host, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(st.copied, stream));
    st.in_flight = true;
    const uint32_t* image_first = (const uint32_t*) s->seg_desc.ptr;
    const uint32_t* image_later = image_first + first.words.size();

    // A segmented sort that ENDS IN LDS (radix_seg_passes.hpp, radix_lds_finish.hpp): ONE counting pass, on the top digit of the
    // bits to sort by, straight from the caller's pieces into the sort's own scratch arrays -- after it the array is nseg x 256
    // runs (segment, top digit) whose starts are in the pass's scanned table -- and one pass that orders every run by the
    // remaining low bits inside LDS on its way into `out`: 20 + 16 B per pair instead of passes x 20.  The tile and, for long
    // runs, the number of workgroups a run is split over follow from the run length uniformly drawn keys would give (mean + 6
    // sigma); runs that come out longer are walked in pieces by radix_finish_ranges_kernel.  The device decides by the longest
    // run (the gate) before the pass's scatter moves anything: beyond 32 tiles per workgroup the ordinary passes, enqueued
    // behind, run instead (they return at once otherwise).  Needs the scratch arrays to be a third pair (in != scratch != out).
    uint32_t gate_mode = kSegGateNone, gate_cap = 0;
    const uint64_t nruns = (uint64_t) nseg * 256u;
    s->last_seg_finish_attempted = false;
    const bool third_pair = tmp_k != in_k && tmp_k != out_k && tmp_v != in_v && tmp_v != out_v;
    {
        uint32_t geo = 0, split_log2 = 0;
        if (third_pair && seg_finish_choice(s, plan, geo, split_log2))
        {
            GLU_TRY(s->finish_starts.reserve(((size_t) std::max<uint64_t>(nruns, kFinishRuns) + 1) * sizeof(uint32_t)));
            GLU_TRY(s->seg_gate.reserve(64));
            gate_cap = (uint32_t) std::min<uint64_t>(0xFFFFFFFFull, (uint64_t) finish_geometry_capacity(geo) * 32u << split_log2);
            const uint32_t end = (uint32_t) (plan.seg_start[0] + count);
            s->cur_kind = 3;
            GLU_TRY(launch_seg_pass(s, in_k, in_v, tmp_k, tmp_v, count, plan.bits - 8, image_first, first, stream, kSegGateIfFits, gate_cap, end));
            s->cur_kind = 2;
            s->mark(stream);
            s->mark(stream);
            s->mark(stream, true);
            GLU_TRY(launch_seg_finish(tmp_k, tmp_v, out_k, out_v, (const uint32_t*) s->finish_starts.ptr, (uint32_t) nruns, geo, split_log2,
                                      plan.bits - 8, (const uint32_t*) s->seg_gate.ptr, gate_cap, s->finish_rank_bits, stream));
            s->mark(stream, true);
            s->cur_kind = 0;
            gate_mode = kSegGateIfNot;
            s->last_seg_finish_attempted = true;
            s->last_seg_finish_capacity = gate_cap;
            s->last_seg_finish_runs = (uint32_t) nruns;
            s->last_seg_finish_tile = finish_geometry_capacity(geo);
            s->last_seg_finish_split = 1u << split_log2;
        }
    }

    // the arrays of every pass (seg_plan.hpp: seg_pass_arrays)
    uint32_t* const keys_of[] = {in_k, out_k, tmp_k};
    uint32_t* const vals_of[] = {in_v, out_v, tmp_v};
    for (uint32_t p = 0; p < passes; p++)
    {
        const SegPassArrays arrays = seg_pass_arrays(passes, p);
        s->cur_kind = gate_mode == kSegGateIfNot ? 4 : 0;
        s->cur_behind = gate_mode == kSegGateIfNot;
        GLU_TRY(launch_seg_pass(s, keys_of[(int) arrays.src], vals_of[(int) arrays.src], keys_of[(int) arrays.dst], vals_of[(int) arrays.dst], count,
                                p * 8, p == 0 ? image_first : image_later, p == 0 ? first : later, stream, gate_mode, gate_cap));
    }
    s->cur_kind = 0;
    s->cur_behind = false;
    return GLU_OK;
}

glu_status glu_hip::host::read_seg_gate(const glu_radix_sort_s* s, bool& tried, uint32_t& longest)
{
    tried = s->last_seg_finish_attempted && s->seg_gate.ptr;
    longest = 0;
    if (tried) HIP_TRY(hipMemcpy(&longest, s->seg_gate.ptr, sizeof(longest), hipMemcpyDeviceToHost));
    return GLU_OK;
}

extern "C" {

glu_status glu_radix_sort_run_segments_ptr(glu_radix_sort sort, uint32_t* in_keys, uint32_t* in_vals, uint32_t* out_keys,
                                           uint32_t* out_vals, size_t count, const uint64_t* piece_begin,
                                           const uint64_t* piece_len, const uint32_t* piece_segment, size_t num_pieces,
                                           uint32_t num_segments, uint32_t key_bits, void* stream)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    if (key_bits > 32 || key_bits % 8 != 0) return fail(GLU_ERROR_INVALID_ARGUMENT, "key_bits must be 0, 8, 16, 24 or 32 (got %u)", key_bits);
    if (count > 0xFFFF0000ull) return fail(GLU_ERROR_INVALID_ARGUMENT, "count %zu does not fit 32-bit indexing", count);
    if (num_pieces > 0) GLU_TRY(check_none_null({piece_begin, piece_len, piece_segment}, "NULL piece array"));
    if (num_segments == 0 && num_pieces > 0) return fail(GLU_ERROR_INVALID_ARGUMENT, "pieces but no segments");
    if (num_segments > kSegMaxSegments) return fail(GLU_ERROR_INVALID_ARGUMENT, "num_segments %u exceeds %u", num_segments, kSegMaxSegments);
    std::vector<SegPiece> pieces;
    uint64_t total = 0;
    GLU_TRY(read_pieces(piece_begin, piece_len, piece_segment, num_pieces, num_segments, &count, pieces, total));
    if (total != count) return fail(GLU_ERROR_INVALID_ARGUMENT, "the pieces hold %llu elements, count is %zu", (unsigned long long) total, count);
    if (count == 0) return GLU_OK;
    if (const SegTiling tiling = seg_pieces_tile(pieces); !tiling.tiles)
        return fail(GLU_ERROR_INVALID_ARGUMENT, "the pieces do not tile the input: element %llu is in %s piece",
                    (unsigned long long) tiling.element, tiling.twice ? "more than one" : "no");
    GLU_TRY(check_none_null({in_keys, in_vals, out_keys, out_vals}, "NULL array"));
    if (in_keys == out_keys || in_vals == out_vals) return fail(GLU_ERROR_INVALID_ARGUMENT, "the segmented sort needs distinct input and output arrays");
    // the sub-block descriptors of a call travel through a ring of pinned staging buffers that later calls overwrite, and a
    // prepared sorter may wait for a staging buffer's previous copy: a captured graph would replay neither correctly
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    (void) hipStreamIsCapturing(pick_stream(stream), &capturing);
    if (capturing != hipStreamCaptureStatusNone)
        return fail(GLU_ERROR_INVALID_STATE, "glu_radix_sort_run_segments_ptr cannot be captured into a graph (its descriptors are staged per call)");
    const bool aligned = (((uintptr_t) in_keys | (uintptr_t) in_vals | (uintptr_t) out_keys | (uintptr_t) out_vals) & 15u) == 0;
    SegPlan plan;
    seg_make_plan(sort, std::move(pieces), num_segments, count, key_bits, aligned, plan);
    return seg_run_plan(sort, plan, in_keys, in_vals, out_keys, out_vals, pick_stream(stream));
}

glu_status glu_radix_sort_plan_segments(const uint64_t* piece_begin, const uint64_t* piece_len, const uint32_t* piece_segment,
                                        size_t num_pieces, uint32_t num_segments, uint32_t num_workgroups, uint32_t* sub_blocks,
                                        size_t sub_block_capacity, uint32_t* workgroup_first, uint32_t* segment_first,
                                        uint64_t* segment_start, size_t* num_sub_blocks)
{
    // host only (no device needed): the cut of a segmented pass into sub-blocks, for inspection and tests
    if (num_pieces > 0) GLU_TRY(check_none_null({piece_begin, piece_len, piece_segment}, "NULL piece array"));
    if (num_workgroups == 0 || !num_sub_blocks) return fail(GLU_ERROR_INVALID_ARGUMENT, "bad arguments");
    if (num_segments > kSegMaxSegments) return fail(GLU_ERROR_INVALID_ARGUMENT, "num_segments %u exceeds %u", num_segments, kSegMaxSegments);
    if (num_workgroups > (1u << 20)) return fail(GLU_ERROR_INVALID_ARGUMENT, "num_workgroups %u exceeds %u", num_workgroups, 1u << 20);
    std::vector<SegPiece> pieces;
    uint64_t total = 0;
    GLU_TRY(read_pieces(piece_begin, piece_len, piece_segment, num_pieces, num_segments, nullptr, pieces, total));
    if (total > 0xFFFF0000ull) return fail(GLU_ERROR_INVALID_ARGUMENT, "the pieces hold %llu elements: more than 32-bit indexing", (unsigned long long) total);
    std::vector<uint64_t> start;
    seg_order_pieces(pieces, num_segments, 0, start);
    SegImage img;
    seg_build_image(pieces.data(), pieces.size(), num_segments, start.data(), total, num_workgroups, img);
    *num_sub_blocks = img.nsb;
    if (img.nsb > sub_block_capacity) return fail(GLU_ERROR_INVALID_ARGUMENT, "%u sub-blocks, room for %zu", img.nsb, sub_block_capacity);
    if (sub_blocks) memcpy(sub_blocks, img.words.data(), (size_t) img.nsb * 2 * sizeof(uint32_t));
    if (workgroup_first) memcpy(workgroup_first, img.words.data() + img.off_first, ((size_t) num_workgroups + 1) * sizeof(uint32_t));
    if (segment_first) memcpy(segment_first, img.words.data() + img.off_list, ((size_t) num_segments + 1) * sizeof(uint32_t));
    if (segment_start)
        for (uint32_t g = 0; g <= num_segments; g++) segment_start[g] = start[g];
    return GLU_OK;
}

glu_status glu_radix_sort_read_seg_finish(glu_radix_sort sort, uint32_t* attempted, uint32_t* accepted, uint32_t* longest_run,
                                          uint32_t* capacity, uint32_t* runs, uint32_t* tile, uint32_t* split)
{
    GLU_TRY(enter());
    GLU_TRY(check_not_null(sort, "sort"));
    bool tried;
    uint32_t longest;
    GLU_TRY(read_seg_gate(sort, tried, longest));
    store(attempted, tried ? 1u : 0u);
    store(accepted, tried && longest <= sort->last_seg_finish_capacity ? 1u : 0u);
    store(longest_run, longest);
    store(capacity, tried ? sort->last_seg_finish_capacity : 0u);
    store(runs, tried ? sort->last_seg_finish_runs : 0u);
    store(tile, tried ? sort->last_seg_finish_tile : 0u);
    store(split, tried ? sort->last_seg_finish_split : 0u);
    return GLU_OK;
}

} // extern "C"
