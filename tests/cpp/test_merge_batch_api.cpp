// C++ API test of glu::Merge's batched calls: ragged segments of uint32 pairs from device offsets (empty sides, offsets that do not
// start at 0, arrays longer than the last offset) and equal partitions of keys alone, each against std::stable_sort per segment
// (A's elements in front of B's, so the stable sort takes A first on ties); out_offsets exact, nothing written behind the last output.
#include <algorithm>
#include <random>
#include <vector>

#include "glu/Merge.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
// the stable sort of segment s of A followed by segment s of B, segment after segment
void expected(const std::vector<uint32_t>& a, const std::vector<uint32_t>& av, const std::vector<uint32_t>& ao, const std::vector<uint32_t>& b,
              const std::vector<uint32_t>& bv, const std::vector<uint32_t>& bo, std::vector<uint32_t>& keys, std::vector<uint32_t>& vals,
              std::vector<uint32_t>& offsets)
{
    keys.clear(), vals.clear(), offsets.clear();
    for (size_t s = 0; s + 1 < ao.size(); s++)
    {
        offsets.push_back((uint32_t) keys.size());
        std::vector<std::pair<uint32_t, uint32_t>> seg;
        for (uint32_t i = ao[s]; i < ao[s + 1]; i++) seg.push_back({a[i], av[i]});
        for (uint32_t j = bo[s]; j < bo[s + 1]; j++) seg.push_back({b[j], bv[j]});
        std::stable_sort(seg.begin(), seg.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        for (const auto& p : seg) keys.push_back(p.first), vals.push_back(p.second);
    }
    offsets.push_back((uint32_t) keys.size());
}

// sorted runs per segment, later segments holding smaller keys
void fill(std::mt19937& rng, const std::vector<uint32_t>& off, std::vector<uint32_t>& keys)
{
    const size_t segments = off.size() - 1;
    for (uint32_t& k : keys) k = rng();
    for (size_t s = 0; s < segments; s++)
    {
        for (uint32_t i = off[s]; i < off[s + 1]; i++) keys[i] = (uint32_t) (segments - s) * 1000u + rng() % 50u;
        std::sort(keys.begin() + off[s], keys.begin() + off[s + 1]);
    }
}
} // namespace

TEST_CASE("Merge-batch-of-ragged-segments-against-std-stable-sort")
{
    std::mt19937 rng(1);
    const size_t segments = 300;
    std::vector<uint32_t> ao(segments + 1), bo(segments + 1);
    ao[0] = 5, bo[0] = 2;
    for (size_t s = 0; s < segments; s++)
    {
        const uint32_t la = s == 17 ? 9000u : rng() % 4 ? rng() % 40 : 0u, lb = s == 200 ? 7000u : rng() % 3 ? rng() % 60 : 0u;
        ao[s + 1] = ao[s] + la, bo[s + 1] = bo[s] + lb;
    }
    const size_t a_total = ao.back() + 11, b_total = bo.back() + 3, room = a_total + b_total;
    std::vector<uint32_t> a(a_total), b(b_total), av(a_total), bv(b_total);
    fill(rng, ao, a);
    fill(rng, bo, b);
    for (size_t i = 0; i < a_total; i++) av[i] = (uint32_t) i;
    for (size_t j = 0; j < b_total; j++) bv[j] = (uint32_t) j | 0x80000000u;
    std::vector<uint32_t> want_keys, want_vals, want_offsets;
    expected(a, av, ao, b, bv, bo, want_keys, want_vals, want_offsets);
    const size_t total = want_keys.size();
    want_keys.resize(room, 0xA5A5A5A5u);
    want_vals.resize(room, 0xA5A5A5A5u);

    ShaderStorageBuffer ak(a), avb(av), aob(ao), bk(b), bvb(bv), bob(bo), ok(room * 4), ov(room * 4), oo((segments + 1) * 4);
    const Merge::Plan plan = Merge::plan_batch(room, segments);
    CHECK(plan.tile == Merge::plan(1, 1).tile);
    CHECK(plan.tiles == (room + plan.tile - 1) / plan.tile);
    CHECK(plan.kernels == 2);
    CHECK(plan.scratch_bytes == (plan.tiles + 1) * 8);
    CHECK(total > 4 * plan.tile);
    Merge merge;
    merge.prepare_batch(room);
    ok.clear(0xA5A5A5A5u);
    ov.clear(0xA5A5A5A5u);
    merge.merge_batch_offsets(ak.device_ptr(), (const uint32_t*) avb.device_ptr(), (const uint32_t*) aob.device_ptr(), a_total, bk.device_ptr(),
                              (const uint32_t*) bvb.device_ptr(), (const uint32_t*) bob.device_ptr(), b_total, segments, ok.device_ptr(),
                              (uint32_t*) ov.device_ptr(), (uint32_t*) oo.device_ptr());
    CHECK(ok.get_data<uint32_t>() == want_keys);
    CHECK(ov.get_data<uint32_t>() == want_vals);
    CHECK(oo.get_data<uint32_t>() == want_offsets);
    CHECK(merge.last().tiles == plan.tiles && merge.last().kernels == 2);
    // keys alone, no out_offsets
    ok.clear(0xA5A5A5A5u);
    ov.clear(0xA5A5A5A5u);
    merge.merge_batch_offsets(ak.device_ptr(), nullptr, (const uint32_t*) aob.device_ptr(), a_total, bk.device_ptr(), nullptr,
                              (const uint32_t*) bob.device_ptr(), b_total, segments, ok.device_ptr(), nullptr);
    CHECK(ok.get_data<uint32_t>() == want_keys);
    CHECK(ov.get_data<uint32_t>() == std::vector<uint32_t>(room, 0xA5A5A5A5u));
    CHECK(ak.get_data<uint32_t>() == a);
    CHECK(bk.get_data<uint32_t>() == b);
    CHECK(aob.get_data<uint32_t>() == ao);
    CHECK(bob.get_data<uint32_t>() == bo);
}

TEST_CASE("Merge-batch-of-equal-partitions-against-std-stable-sort")
{
    std::mt19937 rng(2);
    const size_t lens[4][3] = {{7, 9, 1000}, {3, 0, 50}, {0, 5, 50}, {4096, 4096, 3}};
    Merge merge;
    for (const auto& c : lens)
    {
        const size_t a_len = c[0], b_len = c[1], segments = c[2], room = (a_len + b_len) * segments;
        std::vector<uint32_t> ao(segments + 1), bo(segments + 1);
        for (size_t s = 0; s <= segments; s++) ao[s] = (uint32_t) (s * a_len), bo[s] = (uint32_t) (s * b_len);
        std::vector<uint32_t> a(a_len * segments), b(b_len * segments), av(a.size()), bv(b.size());
        fill(rng, ao, a);
        fill(rng, bo, b);
        for (size_t i = 0; i < a.size(); i++) av[i] = (uint32_t) i;
        for (size_t j = 0; j < b.size(); j++) bv[j] = (uint32_t) j | 0x80000000u;
        std::vector<uint32_t> want_keys, want_vals, want_offsets;
        expected(a, av, ao, b, bv, bo, want_keys, want_vals, want_offsets);
        // (a buffer of no bytes is not made: the empty side gets a word it never reads)
        ShaderStorageBuffer ak(a.empty() ? std::vector<uint32_t>(1) : a), avb(a.empty() ? std::vector<uint32_t>(1) : av);
        ShaderStorageBuffer bk(b.empty() ? std::vector<uint32_t>(1) : b), bvb(b.empty() ? std::vector<uint32_t>(1) : bv);
        ShaderStorageBuffer ok(room * 4), ov(room * 4), oo((segments + 1) * 4);
        merge.merge_batch(ak.device_ptr(), (const uint32_t*) avb.device_ptr(), a_len, bk.device_ptr(), (const uint32_t*) bvb.device_ptr(), b_len,
                          segments, ok.device_ptr(), (uint32_t*) ov.device_ptr(), (uint32_t*) oo.device_ptr());
        CHECK(ok.get_data<uint32_t>() == want_keys);
        CHECK(ov.get_data<uint32_t>() == want_vals);
        CHECK(oo.get_data<uint32_t>() == want_offsets);
        CHECK(merge.last().tiles == Merge::plan_batch(room, segments).tiles);
    }
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
