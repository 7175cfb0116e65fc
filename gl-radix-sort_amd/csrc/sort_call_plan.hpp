// sort_call_plan.hpp -- what one sort call decides on the host before it enqueues anything (glu_hip.hip: sort_bits): the list of its
// passes, and whether it tries to end in LDS given what the object's earlier attempts came to.  Plain C++: no HIP, no sort object
// (tests/test_sort_call_plan.py walks both functions on the CPU).
#pragma once
#include <algorithm>
#include <cstdint>

namespace glu_hip
{
constexpr uint32_t kSortCallMaxPasses = 32; // (kPlanMaxPasses of radix_sort_kernels.hpp: glu_hip.hip holds the two together)

struct SortPass
{
    uint32_t shift, bits, xform;
    int pair_role; // 0: the pass counts for itself, 1: leader, 2: follower (radix_pair_passes.hpp)
};
struct SortPassList
{
    SortPass passes[kSortCallMaxPasses];
    uint32_t num = 0;
};

// The passes of a sort of key bits [first_bit, end_bit): digit positions, key transforms (typed keys, key_xf != 0: encode on the
// first pass's loads, decode -- key_xf << 2 -- on the last pass's stores), and which passes share one count kernel.
// `attempt`: the sort first tries to end in LDS (radix_lds_finish.hpp) -- the two top-bit passes below `finish_top_bit` are enqueued
// in front of the ordinary passes, and the device runs one of the two sequences.  lines8 / lines4: a pass of 8-bit / 4-bit digits
// over this call's arrays runs the line kernel.  false: more passes than a plan holds.
inline bool sort_call_passes(SortPassList& list, uint32_t key_bytes, uint32_t first_bit, uint32_t end_bit, uint32_t digit_bits,
                             uint32_t key_xf, bool attempt, uint32_t finish_top_bit, bool pairs_ok, bool lines8, bool lines4)
{
    SortPass* const passes = list.passes;
    uint32_t num_passes = 0;
    if (attempt)
    {
        passes[0] = SortPass{finish_top_bit - 16u, 8u, key_xf, 0}; // (typed keys: encoded on load here, decoded on store by the in-LDS pass)
        passes[1] = SortPass{finish_top_bit - 8u, 8u, 0u, 0};
        num_passes = 2;
    }
    for (uint32_t shift = first_bit; shift < end_bit;)
    {
        uint32_t bits = std::min<uint32_t>(digit_bits, end_bit - shift);
        if (key_bytes == 8 && shift < 32 && shift + bits > 32) bits = 32 - shift; // a digit stays inside one key word
        const uint32_t xform = (shift == first_bit ? key_xf : 0u) | (shift + bits >= end_bit ? key_xf << 2 : 0u);
        if (num_passes == kSortCallMaxPasses) return false;
        passes[num_passes++] = SortPass{shift, bits, xform, 0};
        shift += bits;
    }
    list.num = num_passes;
    // A leader is a pass of the line kernel that does not encode keys on load; its follower is the pass after it, of the
    // line kernel of the same digit width (wider than 4 bits: the 8-bit kernels, else the 4-bit ones).
    if (pairs_ok || attempt)
        for (uint32_t i = 0; i + 1 < num_passes;)
        {
            const bool wide = passes[i].bits > 4;
            // (below the size from which ordinary passes pair, only the two top-bit passes of an attempt to end in LDS do)
            // (a leader does not encode keys on load -- except the first top-bit pass of an attempt, whose 8-bit pair-count
            // kernel has the encoding instantiation)
            if ((pairs_ok || (attempt && i == 0)) && wide == (passes[i + 1].bits > 4) && (wide ? lines8 : lines4) &&
                ((passes[i].xform & 3u) == 0 || (attempt && i == 0)))
            {
                passes[i].pair_role = 1;
                passes[i + 1].pair_role = 2;
                i += 2;
            }
            else
                i += 1;
        }
    return true;
}

// What a sort object remembers of its attempts to end in LDS.  A refused attempt costs one read of the keys; the plan kernel notes
// each attempt's outcome in five pinned host words (radix_finish_plan_kernel):
//   0: attempt number << 3 | tile geometry, 0 = refused -- stored last;  1, 2: which key bits varied, valid for the attempt number in
//   word 3;  4: the top bit the attempt used.
struct FinishFeedback
{
    uint32_t finish_seq = 0, finish_seq_acted_on = 0; // the number of the last attempt, and of the last one whose outcome was acted on
    uint32_t finish_wait = 0;         // sort calls that still sit out (finish_backoff)
    uint32_t finish_last_geo = 0;     // the tile geometry the device chose for the last sort whose outcome is known (0: none yet)
    bool finish_last_refused = false; // the last attempt whose outcome is known was refused (see glu_radix_sort_s::side)
    // The runs of a sort that ends in LDS are the values of the 16 key bits below `top`: the whole key's top 16 by default,
    // the top 16 of the bits that VARIED in this object's last attempt once that is known (keys below 2^28 make 4096 runs of the
    // whole key's top bits and 65536 of bits [12, 28)).  A guess: the plan kernel refuses if a bit from `top` up varies after all.
    uint32_t top_floor = 0;      // device_top: the exact top bit of an attempt whose sample missed a varying bit (handed to the next sample)
    uint32_t finish_top = 0;     // the host's guess (GLU_HIP_SORT_DEVICE_TOP=0); 0: the key's width
    uint32_t finish_backoff = 0; // GLU_HIP_SORT_FINISH_BACKOFF=N (0, the default: every sort attempts)
};

// One sort call that could attempt: takes in the last attempt's outcome if it has arrived (`hint`: the call's snapshot of the five
// words; nullptr: there are none) and says whether this call attempts -- then it takes the next attempt number.  No
// synchronisation: an outcome that is not there yet counts as unknown.  device_top: the runs' key bits are chosen on the device from
// a sample of the keys, and the host only remembers, as a floor for the next sample, the exact top bit of an attempt that was
// refused because its sample had missed a varying bit; else the host guesses the top bit from the object's last attempt (round 4).
inline bool finish_attempts(FinishFeedback& f, const uint32_t* hint, bool device_top, uint32_t key_bytes, uint32_t end_bit)
{
    const uint32_t seen = hint && f.finish_seq ? hint[0] : 0u;
    if (hint && f.finish_wait == 0 && f.finish_seq && (seen >> 3) == f.finish_seq) // the last attempt's outcome has arrived
    {
        const bool refused = (seen & 7u) == 0u;
        if (!refused) f.finish_last_geo = seen & 7u; // the tile it took
        f.finish_last_refused = refused;
        if (f.finish_seq != f.finish_seq_acted_on) // (acted on once)
        {
            f.finish_seq_acted_on = f.finish_seq;
            const bool bits_known = hint[3] == f.finish_seq;
            const uint64_t varying = (uint64_t) hint[1] | ((uint64_t) hint[2] << 32);
            bool assumption_changed = false; // (then what the last attempt was told says nothing about the next)
            if (device_top)
            {
                if (bits_known)
                {
                    const uint32_t exact = varying ? 64u - (uint32_t) __builtin_clzll(varying) : 0u, used = hint[4];
                    assumption_changed = refused && exact > used;
                    if (assumption_changed)
                        f.top_floor = exact; // the sample missed a bit that varies: the next one starts from here
                    else if (exact < f.top_floor)
                        f.top_floor = 0;     // (other keys now)
                }
            }
            else
            {
                const uint32_t was = f.finish_top ? f.finish_top : end_bit;
                uint32_t top = was;
                if (bits_known)
                {
                    // which key bits varied: the runs of the next attempt are the values of the top 16 of those
                    top = varying ? 64u - (uint32_t) __builtin_clzll(varying) : 16u;
                    top = std::min<uint32_t>(std::max<uint32_t>(top, 16u), end_bit);
                    if (key_bytes == 8 && top > 32 && top < 48 && top != 40) top = top < 40 ? 40 : 48; // a digit stays inside one key word
                }
                assumption_changed = top != was;
                if (assumption_changed) f.finish_top = top;
            }
            // refused for its runs, under the same assumption: do not ask again for a while
            if (refused && !assumption_changed && f.finish_backoff) f.finish_wait = f.finish_backoff;
        }
    }
    if (hint && f.finish_wait)
    {
        f.finish_wait--;
        return false;
    }
    f.finish_seq = f.finish_seq >= 0x0FFFFFFFu ? 1u : f.finish_seq + 1;
    return true;
}
} // namespace glu_hip
