// C++ API test of glu::Gather: records fetched through the values of a sort against a serial restatement, indices out of range left
// untouched, the scatter back, and the batched forms on rows of local indices over equal partitions and device offsets.
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "glu/Gather.hpp"
#include "glu/RadixSort.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
constexpr uint32_t kPoison = 0xA5A5A5A5u;
constexpr uint64_t kPoison64 = ((uint64_t) kPoison << 32) | kPoison;
} // namespace

TEST_CASE("Gather-records-through-the-values-of-a-sort-and-scatter-them-back")
{
    std::mt19937 rng(1);
    const size_t n = 100003;
    std::vector<uint32_t> keys(n), iota(n);
    std::vector<uint64_t> records(n);
    for (uint32_t& k : keys) k = rng() % 5000u;
    for (uint64_t& r : records) r = (((uint64_t) rng() << 32) | rng()) & ~(1ull << 63);
    std::iota(iota.begin(), iota.end(), 0u);
    std::vector<uint32_t> order = iota;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });

    ShaderStorageBuffer kb(keys), vb(iota), rb(records), out(n * 8), back(n * 8);
    RadixSort sort;
    sort(kb.handle(), vb.handle(), n);
    CHECK(vb.get_data<uint32_t>() == order);

    const Gather::Plan plan = Gather::plan(n, 8);
    CHECK(plan.tile == 256 * 4 * 2);
    CHECK(plan.tiles == (n + plan.tile - 1) / plan.tile);
    CHECK(plan.kernels == 1);
    Gather gather;
    out.clear(kPoison);
    gather(rb, n, 8, vb, n, out);
    std::vector<uint64_t> want(n);
    for (size_t j = 0; j < n; j++) want[j] = records[order[j]];
    CHECK(out.get_data<uint64_t>() == want);
    CHECK(gather.last().tiles == plan.tiles && gather.last().kernels == 1);

    back.clear(kPoison);
    gather.scatter(out.device_ptr(), 8, (const uint32_t*) vb.device_ptr(), n, back.device_ptr(), n);
    CHECK(back.get_data<uint64_t>() == records);
    CHECK(rb.get_data<uint64_t>() == records);

    // indices that are out of range leave their entry untouched
    std::vector<uint32_t> idx(5000);
    for (size_t j = 0; j < idx.size(); j++) idx[j] = j % 3 == 1 ? (uint32_t) n + (uint32_t) (j % 7) * 0x20000000u : rng() % (uint32_t) n;
    ShaderStorageBuffer xb(idx), some(idx.size() * 8);
    some.clear(kPoison);
    gather(rb.device_ptr(), n, 8, (const uint32_t*) xb.device_ptr(), idx.size(), some.device_ptr());
    std::vector<uint64_t> want_some(idx.size(), kPoison64);
    for (size_t j = 0; j < idx.size(); j++)
        if (idx[j] < n) want_some[j] = records[idx[j]];
    CHECK(some.get_data<uint64_t>() == want_some);

    gather(rb.device_ptr(), n, 8, (const uint32_t*) xb.device_ptr(), 0, some.device_ptr()); // nothing to do
    CHECK(gather.last().tiles == 0 && gather.last().kernels == 0);
    CHECK(some.get_data<uint64_t>() == want_some);
}

TEST_CASE("Gather-batched-rows-of-local-indices")
{
    std::mt19937 rng(2);
    const size_t count = 1000, parts = 37, k = 17, total = count * parts;
    std::vector<uint64_t> items(total);
    for (uint64_t& r : items) r = (((uint64_t) rng() << 32) | rng()) & ~(1ull << 63);
    std::vector<uint32_t> idx(parts * k);
    for (uint32_t& i : idx) i = rng() % (uint32_t) (count + 20); // a few not below the segment's length
    ShaderStorageBuffer ib(items), xb(idx), out(parts * k * 8);
    Gather gather;
    out.clear(kPoison);
    gather.batch(ib.device_ptr(), 8, count, parts, (const uint32_t*) xb.device_ptr(), k, out.device_ptr());
    std::vector<uint64_t> want(parts * k, kPoison64);
    for (size_t s = 0; s < parts; s++)
        for (size_t j = 0; j < k; j++)
            if (idx[s * k + j] < count) want[s * k + j] = items[s * count + idx[s * k + j]];
    CHECK(out.get_data<uint64_t>() == want);

    // device offsets: an empty segment, one shorter than k, the rest of uneven lengths
    std::vector<uint32_t> offsets(parts + 1);
    offsets[0] = 5;
    for (size_t s = 0; s < parts; s++) offsets[s + 1] = offsets[s] + (s == 3 ? 0u : s == 4 ? 9u : 300u + rng() % 600u);
    REQUIRE(offsets[parts] <= total);
    ShaderStorageBuffer fb(offsets);
    out.clear(kPoison);
    gather.batch_offsets(ib.device_ptr(), 8, total, (const uint32_t*) fb.device_ptr(), parts, (const uint32_t*) xb.device_ptr(), k,
                         out.device_ptr());
    std::fill(want.begin(), want.end(), kPoison64);
    for (size_t s = 0; s < parts; s++)
    {
        const size_t len = offsets[s + 1] - offsets[s];
        for (size_t j = 0; j < std::min(k, len); j++)
            if (idx[s * k + j] < len) want[s * k + j] = items[offsets[s] + idx[s * k + j]];
    }
    CHECK(out.get_data<uint64_t>() == want);
    CHECK(ib.get_data<uint64_t>() == items);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
