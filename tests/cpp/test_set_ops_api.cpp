// C++ API test of glu::SetOps: uint32 pairs with duplicates on both sides against std::set_union / set_intersection /
// set_difference / set_symmetric_difference on (key, value) pairs compared by key alone (the standard's multiset semantics: the
// elements of the first range on ties, each range in its own order), keys alone, a call that only counts, a short max_out, and two
// arrays that glu::RadixSort sorted as floats (both zeros and NaNs among them).
#include <algorithm>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "glu/RadixSort.hpp"
#include "glu/SetOps.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
using Pair = std::pair<uint32_t, uint32_t>;
const auto by_key = [](const Pair& x, const Pair& y) { return x.first < y.first; };

std::vector<Pair> expected(glu_set_op op, const std::vector<Pair>& a, const std::vector<Pair>& b)
{
    std::vector<Pair> out;
    switch (op)
    {
    case GLU_SET_UNION: std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out), by_key); break;
    case GLU_SET_INTERSECTION: std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out), by_key); break;
    case GLU_SET_DIFFERENCE: std::set_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out), by_key); break;
    default: std::set_symmetric_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out), by_key); break;
    }
    // (std::set_union emits the extra copies of B behind ALL of A's copies of a key, as merge's order does)
    return out;
}
} // namespace

TEST_CASE("SetOps-pairs-and-keys-alone-against-the-std-set-algorithms")
{
    std::mt19937 rng(1);
    const size_t a_count = 100003, b_count = 5000, total = a_count + b_count;
    std::vector<uint32_t> a(a_count), b(b_count), av(a_count), bv(b_count);
    for (uint32_t& k : a) k = rng() % 30000; // (duplicates on both sides and across them)
    for (uint32_t& k : b) k = rng() % 30010;
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    for (size_t i = 0; i < a_count; i++) av[i] = (uint32_t) i;
    for (size_t j = 0; j < b_count; j++) bv[j] = (uint32_t) j | 0x80000000u;
    std::vector<Pair> pa(a_count), pb(b_count);
    for (size_t i = 0; i < a_count; i++) pa[i] = {a[i], av[i]};
    for (size_t j = 0; j < b_count; j++) pb[j] = {b[j], bv[j]};

    ShaderStorageBuffer ak(a), avb(av), bk(b), bvb(bv), ok(total * 4), ov(total * 4), num(4);
    const SetOps::Plan plan = SetOps::plan(a_count, b_count);
    CHECK(plan.tile == 256 * 11);
    CHECK(plan.tiles == (total + plan.tile - 1) / plan.tile);
    CHECK(plan.kernels == 4);
    CHECK(plan.scratch_bytes == (plan.tiles + 1) * 12 + plan.tiles * 4);
    CHECK(SetOps::plan(a_count, b_count, GLU_KEY_UINT32, false).kernels == 3);
    CHECK(SetOps::plan(0, 0).kernels == 1 && SetOps::plan(0, 0).scratch_bytes == 0);
    SetOps ops;
    ops.prepare(total);
    const uint32_t* avp = (const uint32_t*) avb.device_ptr();
    const uint32_t* bvp = (const uint32_t*) bvb.device_ptr();
    uint32_t* ovp = (uint32_t*) ov.device_ptr();
    uint32_t* nump = (uint32_t*) num.device_ptr();
    for (int op = 0; op < GLU_SET_OP_COUNT_; op++)
    {
        const std::vector<Pair> want = expected((glu_set_op) op, pa, pb);
        const size_t S = want.size();
        std::vector<uint32_t> want_keys(total, 0xA5A5A5A5u), want_vals(total, 0xA5A5A5A5u);
        for (size_t i = 0; i < S; i++) want_keys[i] = want[i].first, want_vals[i] = want[i].second;
        ok.clear(0xA5A5A5A5u);
        ov.clear(0xA5A5A5A5u);
        switch (op)
        {
        case GLU_SET_UNION: ops.set_union(ak.device_ptr(), avp, a_count, bk.device_ptr(), bvp, b_count, ok.device_ptr(), ovp, total, nump); break;
        case GLU_SET_INTERSECTION: ops.set_intersection(ak.device_ptr(), avp, a_count, bk.device_ptr(), b_count, ok.device_ptr(), ovp, total, nump); break;
        case GLU_SET_DIFFERENCE: ops.set_difference(ak.device_ptr(), avp, a_count, bk.device_ptr(), b_count, ok.device_ptr(), ovp, total, nump); break;
        default:
            ops.set_symmetric_difference(ak.device_ptr(), avp, a_count, bk.device_ptr(), bvp, b_count, ok.device_ptr(), ovp, total, nump);
            break;
        }
        CHECK(num.get_data<uint32_t>()[0] == S);
        CHECK(ok.get_data<uint32_t>() == want_keys); // (the entries behind S are untouched)
        CHECK(ov.get_data<uint32_t>() == want_vals);
        CHECK(ops.last().tiles == plan.tiles && ops.last().kernels == 4);
        // keys alone, room for half of them: S all the same
        const size_t room = S / 2;
        std::fill(want_keys.begin() + room, want_keys.end(), 0xA5A5A5A5u);
        ok.clear(0xA5A5A5A5u);
        ov.clear(0xA5A5A5A5u);
        num.clear(0xA5A5A5A5u);
        ops((glu_set_op) op, ak.device_ptr(), nullptr, a_count, bk.device_ptr(), nullptr, b_count, ok.device_ptr(), nullptr, room, nump);
        CHECK(num.get_data<uint32_t>()[0] == S);
        CHECK(ok.get_data<uint32_t>() == want_keys);
        CHECK(ov.get_data<uint32_t>() == std::vector<uint32_t>(total, 0xA5A5A5A5u));
        // a call that only counts
        num.clear(0xA5A5A5A5u);
        ops((glu_set_op) op, ak.device_ptr(), nullptr, a_count, bk.device_ptr(), nullptr, b_count, nullptr, nullptr, 0, nump);
        CHECK(num.get_data<uint32_t>()[0] == S);
        CHECK(ops.last().tiles == plan.tiles && ops.last().kernels == 3);
        CHECK(ok.get_data<uint32_t>() == want_keys);
    }
    ops(GLU_SET_UNION, nullptr, nullptr, 0, nullptr, nullptr, 0, ok.device_ptr(), nullptr, total, nump); // nothing to look at
    CHECK(num.get_data<uint32_t>()[0] == 0);
    CHECK(ops.last().tiles == 0 && ops.last().kernels == 1);
    CHECK(ak.get_data<uint32_t>() == a);
    CHECK(bk.get_data<uint32_t>() == b);
    CHECK(avb.get_data<uint32_t>() == av);
    CHECK(bvb.get_data<uint32_t>() == bv);
}

TEST_CASE("SetOps-on-floats-the-sort-sorted-compare-keys-by-their-bits")
{
    std::mt19937 rng(2);
    const size_t n = 40000;
    std::vector<float> a(n), b(n);
    for (float& f : a) f = (float) ((int) (rng() % 4001) - 2000) / 16.0f;
    for (float& f : b) f = (float) ((int) (rng() % 4001) - 2000) / 8.0f;
    a[0] = -0.0f, a[1] = -0.0f, a[2] = std::numeric_limits<float>::quiet_NaN(), a[3] = std::numeric_limits<float>::infinity();
    b[0] = 0.0f, b[1] = -0.0f, b[2] = -std::numeric_limits<float>::quiet_NaN(), b[3] = std::numeric_limits<float>::infinity();
    ShaderStorageBuffer ak(a), bk(b), ok(2 * n * 4), num(4);
    RadixSort sort;
    sort.sort_typed((float*) ak.device_ptr(), (uint32_t*) nullptr, n);
    sort.sort_typed((float*) bk.device_ptr(), (uint32_t*) nullptr, n);
    // the sort's order as unsigned keys
    const auto enc = [](uint32_t k) { return (k & 0x80000000u) ? ~k : k | 0x80000000u; };
    std::vector<uint32_t> ea = ak.get_data<uint32_t>(), eb = bk.get_data<uint32_t>();
    for (uint32_t& k : ea) k = enc(k);
    for (uint32_t& k : eb) k = enc(k);
    CHECK(std::is_sorted(ea.begin(), ea.end()) && std::is_sorted(eb.begin(), eb.end()));
    SetOps ops;
    for (int op = 0; op < GLU_SET_OP_COUNT_; op++)
    {
        std::vector<uint32_t> want;
        switch (op)
        {
        case GLU_SET_UNION: std::set_union(ea.begin(), ea.end(), eb.begin(), eb.end(), std::back_inserter(want)); break;
        case GLU_SET_INTERSECTION: std::set_intersection(ea.begin(), ea.end(), eb.begin(), eb.end(), std::back_inserter(want)); break;
        case GLU_SET_DIFFERENCE: std::set_difference(ea.begin(), ea.end(), eb.begin(), eb.end(), std::back_inserter(want)); break;
        default: std::set_symmetric_difference(ea.begin(), ea.end(), eb.begin(), eb.end(), std::back_inserter(want)); break;
        }
        ops((glu_set_op) op, ak.device_ptr(), nullptr, n, bk.device_ptr(), nullptr, n, ok.device_ptr(), nullptr, 2 * n,
            (uint32_t*) num.device_ptr(), GLU_KEY_FLOAT32);
        const size_t S = num.get_data<uint32_t>()[0];
        CHECK(S == want.size());
        std::vector<uint32_t> got = ok.get_data<uint32_t>();
        got.resize(S);
        for (uint32_t& k : got) k = enc(k);
        CHECK(got == want);
    }
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
