// C++ API test of glu::SetOps' batched calls: ragged segments of uint32 pairs from device offsets (empty sides, offsets that do not
// start at 0, arrays longer than the last offset, every segment over the same small key range) and equal partitions of keys alone,
// once per operation, each against std::set_union / set_intersection / set_difference / set_symmetric_difference per segment (on
// pairs compared by their keys alone: the algorithms keep A's elements where both sides match); out_offsets and *num_out exact,
// nothing written behind the last output.
#include <algorithm>
#include <iterator>
#include <random>
#include <vector>

#include "glu/SetOps.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
typedef std::pair<uint32_t, uint32_t> Pair;

// std::set_* of segment s of A and segment s of B, segment after segment
void expected(glu_set_op op, const std::vector<uint32_t>& a, const std::vector<uint32_t>& av, const std::vector<uint32_t>& ao,
              const std::vector<uint32_t>& b, const std::vector<uint32_t>& bv, const std::vector<uint32_t>& bo, std::vector<uint32_t>& keys,
              std::vector<uint32_t>& vals, std::vector<uint32_t>& offsets)
{
    keys.clear(), vals.clear(), offsets.clear();
    const auto by_key = [](const Pair& x, const Pair& y) { return x.first < y.first; };
    for (size_t s = 0; s + 1 < ao.size(); s++)
    {
        offsets.push_back((uint32_t) keys.size());
        std::vector<Pair> sa, sb, out;
        for (uint32_t i = ao[s]; i < ao[s + 1]; i++) sa.push_back({a[i], av[i]});
        for (uint32_t j = bo[s]; j < bo[s + 1]; j++) sb.push_back({b[j], bv[j]});
        if (op == GLU_SET_UNION) std::set_union(sa.begin(), sa.end(), sb.begin(), sb.end(), std::back_inserter(out), by_key);
        if (op == GLU_SET_INTERSECTION) std::set_intersection(sa.begin(), sa.end(), sb.begin(), sb.end(), std::back_inserter(out), by_key);
        if (op == GLU_SET_DIFFERENCE) std::set_difference(sa.begin(), sa.end(), sb.begin(), sb.end(), std::back_inserter(out), by_key);
        if (op == GLU_SET_SYMMETRIC_DIFFERENCE)
            std::set_symmetric_difference(sa.begin(), sa.end(), sb.begin(), sb.end(), std::back_inserter(out), by_key);
        for (const Pair& p : out) keys.push_back(p.first), vals.push_back(p.second);
    }
    offsets.push_back((uint32_t) keys.size());
}

// sorted runs per segment, every segment over the same 50 keys
void fill(std::mt19937& rng, const std::vector<uint32_t>& off, std::vector<uint32_t>& keys)
{
    for (uint32_t& k : keys) k = rng();
    for (size_t s = 0; s + 1 < off.size(); s++)
    {
        for (uint32_t i = off[s]; i < off[s + 1]; i++) keys[i] = rng() % (off[s + 1] - off[s] > 1000 ? 5000u : 50u);
        std::sort(keys.begin() + off[s], keys.begin() + off[s + 1]);
    }
}

const glu_set_op kOps[4] = {GLU_SET_UNION, GLU_SET_INTERSECTION, GLU_SET_DIFFERENCE, GLU_SET_SYMMETRIC_DIFFERENCE};
} // namespace

TEST_CASE("SetOps-batch-of-ragged-segments-against-std-set-algorithms")
{
    std::mt19937 rng(1);
    const size_t segments = 300;
    std::vector<uint32_t> ao(segments + 1), bo(segments + 1);
    ao[0] = 5, bo[0] = 2;
    for (size_t s = 0; s < segments; s++)
    {
        const uint32_t la = s == 17 ? 5000u : rng() % 4 ? rng() % 40 : 0u, lb = s == 17 ? 4000u : rng() % 3 ? rng() % 60 : 0u;
        ao[s + 1] = ao[s] + la, bo[s + 1] = bo[s] + lb;
    }
    const size_t a_total = ao.back() + 11, b_total = bo.back() + 3, room = a_total + b_total;
    std::vector<uint32_t> a(a_total), b(b_total), av(a_total), bv(b_total);
    fill(rng, ao, a);
    fill(rng, bo, b);
    for (size_t i = 0; i < a_total; i++) av[i] = (uint32_t) i;
    for (size_t j = 0; j < b_total; j++) bv[j] = (uint32_t) j | 0x80000000u;
    ShaderStorageBuffer ak(a), avb(av), aob(ao), bk(b), bvb(bv), bob(bo), ok(room * 4), ov(room * 4), oo((segments + 1) * 4), no(4);
    const SetOps::Plan plan = SetOps::plan_batch(a_total, b_total, segments);
    CHECK(plan.tile == SetOps::plan(1, 1).tile);
    CHECK(plan.tiles == (room + plan.tile - 1) / plan.tile);
    CHECK(plan.kernels == 5);
    CHECK(plan.scratch_bytes == (size_t) (plan.tiles + 1) * 16 + (size_t) plan.tiles * 4 + (size_t) plan.tiles * 1024);
    CHECK(SetOps::plan_batch(a_total, b_total, segments, GLU_KEY_UINT32, false, false).scratch_bytes == (size_t) (plan.tiles + 1) * 16 + (size_t) plan.tiles * 4);
    CHECK(plan.tiles > 4);
    SetOps sets;
    sets.prepare_batch(room, segments);
    for (const glu_set_op op : kOps)
    {
        std::vector<uint32_t> want_keys, want_vals, want_offsets;
        expected(op, a, av, ao, b, bv, bo, want_keys, want_vals, want_offsets);
        const uint32_t total = (uint32_t) want_keys.size();
        CHECK(total > 0 && total < room);
        want_keys.resize(room, 0xA5A5A5A5u);
        want_vals.resize(room, 0xA5A5A5A5u);
        ok.clear(0xA5A5A5A5u);
        ov.clear(0xA5A5A5A5u);
        const bool b_too = op == GLU_SET_UNION || op == GLU_SET_SYMMETRIC_DIFFERENCE; // (b_vals is read only by these two)
        sets.set_op_batch_offsets(op, ak.device_ptr(), (const uint32_t*) avb.device_ptr(), (const uint32_t*) aob.device_ptr(), a_total,
                                  bk.device_ptr(), b_too ? (const uint32_t*) bvb.device_ptr() : nullptr, (const uint32_t*) bob.device_ptr(), b_total,
                                  segments, ok.device_ptr(), (uint32_t*) ov.device_ptr(), room, (uint32_t*) no.device_ptr(),
                                  (uint32_t*) oo.device_ptr());
        CHECK(ok.get_data<uint32_t>() == want_keys);
        CHECK(ov.get_data<uint32_t>() == want_vals);
        CHECK(oo.get_data<uint32_t>() == want_offsets);
        CHECK(no.get_data<uint32_t>() == std::vector<uint32_t>(1, total));
        CHECK(sets.last().tiles == plan.tiles && sets.last().kernels == 5);
        // only counting: the cardinalities of every segment, no array written
        ok.clear(0xA5A5A5A5u);
        sets.set_op_batch_offsets(op, ak.device_ptr(), nullptr, (const uint32_t*) aob.device_ptr(), a_total, bk.device_ptr(), nullptr,
                                  (const uint32_t*) bob.device_ptr(), b_total, segments, nullptr, nullptr, 0, (uint32_t*) no.device_ptr(),
                                  (uint32_t*) oo.device_ptr());
        CHECK(oo.get_data<uint32_t>() == want_offsets);
        CHECK(no.get_data<uint32_t>() == std::vector<uint32_t>(1, total));
        CHECK(ok.get_data<uint32_t>() == std::vector<uint32_t>(room, 0xA5A5A5A5u));
        CHECK(sets.last().kernels == 4);
    }
    CHECK(ak.get_data<uint32_t>() == a);
    CHECK(bk.get_data<uint32_t>() == b);
    CHECK(aob.get_data<uint32_t>() == ao);
    CHECK(bob.get_data<uint32_t>() == bo);
}

TEST_CASE("SetOps-batch-of-equal-partitions-against-std-set-algorithms")
{
    std::mt19937 rng(2);
    const size_t lens[4][3] = {{7, 9, 1000}, {3, 0, 50}, {0, 5, 50}, {4096, 4096, 3}};
    SetOps sets;
    for (const auto& c : lens)
    {
        const size_t a_len = c[0], b_len = c[1], segments = c[2], room = (a_len + b_len) * segments;
        std::vector<uint32_t> ao(segments + 1), bo(segments + 1);
        for (size_t s = 0; s <= segments; s++) ao[s] = (uint32_t) (s * a_len), bo[s] = (uint32_t) (s * b_len);
        std::vector<uint32_t> a(a_len * segments), b(b_len * segments), av(a.size()), bv(b.size());
        fill(rng, ao, a);
        fill(rng, bo, b);
        // (a buffer of no bytes is not made: the empty side gets a word it never reads)
        ShaderStorageBuffer ak(a.empty() ? std::vector<uint32_t>(1) : a), bk(b.empty() ? std::vector<uint32_t>(1) : b);
        ShaderStorageBuffer ok(room * 4), oo((segments + 1) * 4), no(4);
        for (const glu_set_op op : kOps)
        {
            std::vector<uint32_t> want_keys, want_vals, want_offsets;
            expected(op, a, av, ao, b, bv, bo, want_keys, want_vals, want_offsets);
            const uint32_t total = (uint32_t) want_keys.size();
            want_keys.resize(room, 0xA5A5A5A5u);
            ok.clear(0xA5A5A5A5u);
            sets.set_op_batch(op, ak.device_ptr(), nullptr, a_len, bk.device_ptr(), nullptr, b_len, segments, ok.device_ptr(), nullptr, room,
                              (uint32_t*) no.device_ptr(), (uint32_t*) oo.device_ptr());
            CHECK(ok.get_data<uint32_t>() == want_keys);
            CHECK(oo.get_data<uint32_t>() == want_offsets);
            CHECK(no.get_data<uint32_t>() == std::vector<uint32_t>(1, total));
            CHECK(sets.last().tiles == SetOps::plan_batch(a.size(), b.size(), segments).tiles);
        }
    }
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
