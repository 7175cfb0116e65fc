// C++ API test of glu::Merge: uint32 pairs with duplicates on both sides against std::merge (stable, the first range in front on
// ties), keys alone, and two halves that glu::RadixSort sorted as floats (both zeros, an infinity and a NaN among them) merged into
// what the sort makes of the whole.
#include <algorithm>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "glu/Merge.hpp"
#include "glu/RadixSort.hpp"
#include "util/mini_test.hpp"

using namespace glu;

TEST_CASE("Merge-pairs-and-keys-alone-against-std-merge")
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
    // (key, value) pairs compared by key alone: std::merge is stable and takes the first range on ties
    std::vector<std::pair<uint32_t, uint32_t>> pa(a_count), pb(b_count), want(total);
    for (size_t i = 0; i < a_count; i++) pa[i] = {a[i], av[i]};
    for (size_t j = 0; j < b_count; j++) pb[j] = {b[j], bv[j]};
    std::merge(pa.begin(), pa.end(), pb.begin(), pb.end(), want.begin(), [](const auto& x, const auto& y) { return x.first < y.first; });
    std::vector<uint32_t> want_keys(total), want_vals(total);
    for (size_t i = 0; i < total; i++) want_keys[i] = want[i].first, want_vals[i] = want[i].second;

    ShaderStorageBuffer ak(a), avb(av), bk(b), bvb(bv), ok(total * 4), ov(total * 4);
    const Merge::Plan plan = Merge::plan(a_count, b_count);
    CHECK(plan.tile == 256 * 11);
    CHECK(plan.tiles == (total + plan.tile - 1) / plan.tile);
    CHECK(plan.kernels == 2);
    CHECK(plan.scratch_bytes == (plan.tiles + 1) * 4);
    Merge merge;
    merge.prepare(total);
    ok.clear(0xA5A5A5A5u);
    ov.clear(0xA5A5A5A5u);
    merge(ak, avb, a_count, bk, bvb, b_count, ok, ov);
    CHECK(ok.get_data<uint32_t>() == want_keys);
    CHECK(ov.get_data<uint32_t>() == want_vals);
    CHECK(merge.last().tiles == plan.tiles && merge.last().kernels == 2);
    ok.clear(0xA5A5A5A5u);
    ov.clear(0xA5A5A5A5u);
    merge(ak, a_count, bk, b_count, ok); // keys alone
    CHECK(ok.get_data<uint32_t>() == want_keys);
    CHECK(ov.get_data<uint32_t>() == std::vector<uint32_t>(total, 0xA5A5A5A5u));
    merge(ak.device_ptr(), nullptr, 0, bk.device_ptr(), nullptr, 0, ok.device_ptr(), nullptr); // nothing to merge
    CHECK(merge.last().tiles == 0 && merge.last().kernels == 0);
    CHECK(ok.get_data<uint32_t>() == want_keys);
    CHECK(ak.get_data<uint32_t>() == a);
    CHECK(bk.get_data<uint32_t>() == b);
    CHECK(avb.get_data<uint32_t>() == av);
    CHECK(bvb.get_data<uint32_t>() == bv);
}

TEST_CASE("Merge-of-two-sorted-halves-of-floats-is-the-sort-of-the-whole")
{
    std::mt19937 rng(2);
    const size_t half = 40000, total = 2 * half;
    std::vector<float> keys(total);
    for (float& f : keys) f = (float) ((int) (rng() % 4001) - 2000) / 16.0f;
    keys[0] = -0.0f;
    keys[1] = 0.0f;
    keys[2] = std::numeric_limits<float>::infinity();
    keys[3] = std::numeric_limits<float>::quiet_NaN();
    keys[half] = 0.0f;
    keys[half + 1] = -0.0f;
    keys[half + 2] = -std::numeric_limits<float>::infinity();
    keys[half + 3] = -std::numeric_limits<float>::quiet_NaN();
    std::vector<uint32_t> vals(total);
    for (size_t i = 0; i < total; i++) vals[i] = (uint32_t) i;
    ShaderStorageBuffer whole_k(keys), whole_v(vals), parts_k(keys), parts_v(vals), out_k(total * 4), out_v(total * 4);
    RadixSort sort;
    sort.sort_typed((float*) whole_k.device_ptr(), (uint32_t*) whole_v.device_ptr(), total);
    float* pk = (float*) parts_k.device_ptr();
    uint32_t* pv = (uint32_t*) parts_v.device_ptr();
    sort.sort_typed(pk, pv, half);
    sort.sort_typed(pk + half, pv + half, half);
    Merge merge;
    merge(pk, pv, half, pk + half, pv + half, half, out_k.device_ptr(), (uint32_t*) out_v.device_ptr(), GLU_KEY_FLOAT32);
    // bit for bit: the values of the first half are below those of the second, so the stable sort and the merge agree on ties
    CHECK(out_k.get_data<uint32_t>() == whole_k.get_data<uint32_t>());
    CHECK(out_v.get_data<uint32_t>() == whole_v.get_data<uint32_t>());
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
