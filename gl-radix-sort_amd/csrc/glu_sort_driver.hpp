// glu_sort_driver.hpp -- what the translation units of the sort call in one another: the whole-key driver (glu_hip.hip), the
// placement search (glu_sort_placement.hip), the segmented sort (glu_sort_segments.hip), the batched sort (glu_sort_batch.hip) and the
// sharded sort (glu_dist.hip).  Declarations only: every template below is defined and explicitly instantiated in the unit named
// beside it, so its kernels are emitted once.  (A header of its own, not more of glu_sort_object.hpp: that one is the object and the
// launch geometries, which the pass launchers need too; this one is the units' calls, which they do not.)
#pragma once
#include <vector>

#include "glu_sort_object.hpp"
#include "seg_plan.hpp"

namespace glu_hip
{
namespace host
{
// ---- glu_hip.hip: the whole-key driver

// The scratch of a sort of `count` elements, grown if need be.
// may_place: only the explicit prepare entry points (glu_radix_sort_prepare*, glu_dist_prepare) pass true.  The lazy call at
// the head of every sort, of a segmented sort and of glu_dist_sort_finish takes the plain allocation: a sort call, a
// collective or a stream capture never measures, never runs calibration sorts and never makes transient allocations.
glu_status sort_prepare(glu_radix_sort_s* s, size_t count, size_t key_size, bool with_vals = true, bool may_place = false);

// The stable sort of key bits [first_bit, end_bit).  vals == nullptr: keys-only sort (no value traffic, no value scratch)
template<typename KeyT>
glu_status sort_bits(glu_radix_sort_s* s, KeyT* keys, uint32_t* vals, size_t count, uint32_t first_bit, uint32_t end_bit,
                     hipStream_t stream, uint32_t key_xf = KEY_XF_NONE);
extern template glu_status sort_bits<uint32_t>(glu_radix_sort_s*, uint32_t*, uint32_t*, size_t, uint32_t, uint32_t, hipStream_t, uint32_t);
extern template glu_status sort_bits<uint64_t>(glu_radix_sort_s*, uint64_t*, uint32_t*, size_t, uint32_t, uint32_t, hipStream_t, uint32_t);

// the reference's interface: num_steps 4-bit steps from bit 0 (0 or more than the key holds = the whole key,
// RadixSort.hpp:289,332)
template<typename KeyT>
glu_status sort_run(glu_radix_sort_s* s, KeyT* keys, uint32_t* vals, size_t count, size_t num_steps, hipStream_t stream,
                    uint32_t key_xf = KEY_XF_NONE);
extern template glu_status sort_run<uint32_t>(glu_radix_sort_s*, uint32_t*, uint32_t*, size_t, size_t, hipStream_t, uint32_t);
extern template glu_status sort_run<uint64_t>(glu_radix_sort_s*, uint64_t*, uint32_t*, size_t, size_t, hipStream_t, uint32_t);

// glu_radix_sort_run_typed_ptr's sort with every launch on `stream` itself: no part of the launch sequence may go to the object's side
// stream (glu_hip.hip, beside the one place that forks).  The batched sort loops it over partitions longer than an LDS tile.
glu_status sort_typed_one_queue(glu_radix_sort_s* s, void* keys, uint32_t* vals, size_t count, glu_key_type key_type, hipStream_t stream);

// ---- glu_sort_placement.hip: large scratch arrays placed by measurement

constexpr size_t kTuneMinKeyBytes = (size_t) 512 << 20; // scratch arrays from this size up are placed by measurement
// The object's own key and value scratch for `count` elements (sort_prepare with may_place; nothing chosen: its plain allocation follows).
glu_status tune_scratch_placement(glu_radix_sort_s* s, size_t count, size_t key_size);
// A pair of arrays of `count` 4-byte elements each for the caller's side of a sort, against the scratch of `s` in place.
glu_status place_pair_by_measurement(glu_radix_sort_s* s, size_t count, Scratch& keys, Scratch& vals);

// ---- glu_sort_segments.hip: the segmented passes and the segmented sort

constexpr size_t kSegMinCount = 1 << 16;       // below: gather + one sort per segment (the line kernel wants whole tiles to prefetch)
constexpr uint32_t kSegMaxSegments = 1u << 24; // (one workgroup per segment in the scan kernel, host vectors of this length)

// Host half of a segmented sort: the pieces sorted by segment (stably: the caller's order of a segment's pieces is the
// order of its elements), where every segment starts in the output, and the descriptor images of the passes.  Nothing is
// enqueued, so a caller (glu_dist) can look at `max_subs_per_wg` -- a workgroup pays about two tiles' time per sub-block,
// whatever its size -- and decide for another way before anything runs.
struct SegPlan
{
    std::vector<SegPiece> pieces;
    std::vector<uint64_t> seg_start; // [nseg + 1]
    uint32_t nseg = 0, passes = 0, bits = 0;
    size_t count = 0;
    bool by_copies = false; // small or unaligned inputs: gather with copies + one ordinary sort per segment
    SegImage first, later;
    uint32_t max_subs_per_wg() const { return std::max(first.max_subs_per_wg, later.max_subs_per_wg); }
};

// `origin`: where the first segment starts in the output (and in the arrays of the intermediate passes): the segments of a
// plan occupy [origin, origin + count) there, so several plans can share one set of (aligned) arrays -- the groups of a
// sharded sort's exchange in rounds, glu_dist.hip.
void seg_make_plan(glu_radix_sort_s* s, std::vector<SegPiece>&& pieces, uint32_t nseg, size_t count, uint32_t bits, bool aligned,
                   SegPlan& plan, uint64_t origin = 0);

// Will a segmented sort by this plan try to end in LDS (given a third pair of arrays to land its counting pass in)?  The tile and,
// for long runs, the number of workgroups a run is split over follow from the run length uniformly drawn keys would give in the
// LARGEST segment (segments may be of any sizes, empty ones included, and the host knows them).  Also asked by glu_dist, which
// allocates the landing pair of the exchange only for sorts that will use it.
bool seg_finish_choice_for(const glu_radix_sort_s* s, uint32_t passes, uint32_t bits, uint64_t nruns, uint64_t largest, uint32_t& geo,
                           uint32_t& split_log2);
bool seg_finish_choice(const glu_radix_sort_s* s, const SegPlan& plan, uint32_t& geo, uint32_t& split_log2);

// Device half: enqueues the passes of `plan` on `stream`.
glu_status seg_run_plan(glu_radix_sort_s* s, const SegPlan& plan, uint32_t* in_k, uint32_t* in_v, uint32_t* out_k, uint32_t* out_v,
                        hipStream_t stream);

// Did the last segmented sort try to end in LDS, and if so the longest run its first pass found (a device word)
glu_status read_seg_gate(const glu_radix_sort_s* s, bool& tried, uint32_t& longest);

// The segmented passes over the LONG runs of a whole-key sort that ends in LDS, a_* -> b_* and home again (sort_bits enqueues them
// beside or behind the in-LDS pass).  a_v == nullptr: a keys-only sort.
template<typename KeyT>
glu_status launch_long_run_passes_any(glu_radix_sort_s* s, KeyT* a_k, uint32_t* a_v, KeyT* b_k, uint32_t* b_v, size_t count, uint32_t key_xf,
                                      hipStream_t stream);
extern template glu_status launch_long_run_passes_any<uint32_t>(glu_radix_sort_s*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, size_t, uint32_t,
                                                                hipStream_t);
extern template glu_status launch_long_run_passes_any<uint64_t>(glu_radix_sort_s*, uint64_t*, uint32_t*, uint64_t*, uint32_t*, size_t, uint32_t,
                                                                hipStream_t);
} // namespace host
} // namespace glu_hip
