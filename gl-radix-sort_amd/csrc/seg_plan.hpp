// seg_plan.hpp -- the host arithmetic of the segmented sort (glu_sort_segments.hip): the pieces of a call ordered by segment and where
// every segment starts, whether the pieces tile the input, the sub-block descriptors of a pass, and which arrays each pass reads and
// writes.  Plain C++: no HIP, no sort object (tests/test_seg_plan.py walks every function on the CPU).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace glu_hip
{
struct SegPiece
{
    uint64_t begin, len;
    uint32_t seg;
};

// Device image of one segmented pass's descriptors (uint32 words): subs[nsb] as (begin, end) pairs, wg_first[nwg + 1],
// seg_list[nseg + 1], seg_start[nseg].
struct SegImage
{
    std::vector<uint32_t> words;
    uint32_t nsb = 0, nwg = 0, nseg = 0, max_subs_per_wg = 0;
    size_t off_first = 0, off_list = 0, off_start = 0;
};

// The pieces stably ordered by segment (the caller's order of a segment's pieces is the order of its elements), and where every
// segment starts when the first one starts at `origin`: seg_start[nseg + 1], the last entry the end of the last segment.
inline void seg_order_pieces(std::vector<SegPiece>& pieces, uint32_t nseg, uint64_t origin, std::vector<uint64_t>& seg_start)
{
    std::stable_sort(pieces.begin(), pieces.end(), [](const SegPiece& a, const SegPiece& b) { return a.seg < b.seg; });
    seg_start.assign((size_t) nseg + 1, 0);
    for (const SegPiece& pc : pieces) seg_start[pc.seg + 1] += pc.len;
    seg_start[0] = origin;
    for (uint32_t g = 0; g < nseg; g++) seg_start[g + 1] += seg_start[g];
}

// Do the pieces tile the input?  They hold as many elements together as the input has, so it is enough that none overlaps another:
// `tiles`, or the first element that lies in no piece (`twice` false) or in more than one (`twice` true).
struct SegTiling
{
    bool tiles = true;
    uint64_t element = 0;
    bool twice = false;
};
inline SegTiling seg_pieces_tile(const std::vector<SegPiece>& pieces)
{
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    spans.reserve(pieces.size());
    for (const SegPiece& pc : pieces)
        if (pc.len) spans.emplace_back(pc.begin, pc.len);
    std::sort(spans.begin(), spans.end());
    uint64_t end = 0;
    for (const auto& sp : spans)
    {
        if (sp.first != end) return SegTiling{false, std::min(sp.first, end), sp.first < end};
        end = sp.first + sp.second;
    }
    return SegTiling();
}

// Cuts the pieces (sorted by segment, in the stable order of each segment's elements) into sub-blocks: workgroup w of
// `nwg` takes the elements [w * share, (w + 1) * share) of the pieces laid end to end, a sub-block is the part of one
// piece inside one workgroup's share.  Pure host function of its arguments.
inline void seg_build_image(const SegPiece* pieces, size_t npieces, uint32_t nseg, const uint64_t* seg_start, uint64_t total,
                            uint32_t nwg, SegImage& img)
{
    img.nwg = nwg;
    img.nseg = nseg;
    const uint64_t share = std::max<uint64_t>(1, (total + nwg - 1) / nwg);
    std::vector<uint32_t> subs, first((size_t) nwg + 1, 0), list((size_t) nseg + 1, 0);
    subs.reserve(2 * (npieces + nwg));
    uint64_t pos = 0; // position in the pieces laid end to end
    uint32_t seg_seen = 0;
    for (size_t p = 0; p < npieces; p++)
    {
        const SegPiece& pc = pieces[p];
        if (pc.len == 0) continue;
        while (seg_seen <= pc.seg) list[seg_seen++] = (uint32_t) (subs.size() / 2); // segments [.., pc.seg] start here
        uint64_t done = 0;
        while (done < pc.len)
        {
            const uint64_t w = (pos + done) / share;
            const uint64_t room = (w + 1) * share - (pos + done);
            const uint64_t take = std::min<uint64_t>(room, pc.len - done);
            subs.push_back((uint32_t) (pc.begin + done));
            subs.push_back((uint32_t) (pc.begin + done + take));
            first[std::min<uint64_t>(w, nwg - 1) + 1]++; // (counts; turned into offsets below)
            done += take;
        }
        pos += pc.len;
    }
    img.nsb = (uint32_t) (subs.size() / 2);
    while (seg_seen <= nseg) list[seg_seen++] = img.nsb;
    img.max_subs_per_wg = 0;
    for (uint32_t w = 0; w < nwg; w++)
    {
        img.max_subs_per_wg = std::max(img.max_subs_per_wg, first[w + 1]);
        first[w + 1] += first[w];
    }
    img.words.clear();
    img.words.insert(img.words.end(), subs.begin(), subs.end());
    img.off_first = img.words.size();
    img.words.insert(img.words.end(), first.begin(), first.end());
    img.off_list = img.words.size();
    img.words.insert(img.words.end(), list.begin(), list.end());
    img.off_start = img.words.size();
    for (uint32_t g = 0; g < nseg; g++) img.words.push_back((uint32_t) seg_start[g]);
    if (img.words.size() % 2) img.words.push_back(0); // the next image's (begin, end) pairs stay 8-byte aligned
}

// The arrays of pass p of `passes`: the last one writes `out`; with an odd number of passes they alternate in -> out -> in -> out,
// with an even number the sort's own scratch stands in for `out` until the last pass (in -> tmp -> in -> tmp -> out).
enum class SegArray
{
    In,
    Out,
    Scratch
};
struct SegPassArrays
{
    SegArray src, dst;
};
inline SegPassArrays seg_pass_arrays(uint32_t passes, uint32_t p)
{
    const SegArray other = (passes & 1u) ? SegArray::Out : SegArray::Scratch; // what `in` alternates with
    const bool from_in = (p & 1u) == 0;
    return SegPassArrays{from_in ? SegArray::In : other, p + 1 == passes ? SegArray::Out : (from_in ? other : SegArray::In)};
}
} // namespace glu_hip
