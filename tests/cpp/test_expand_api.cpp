// C++ API test of glu::Expand: segments, ranks and 8-byte items of offsets with empty segments and a partial cover against a serial
// restatement, the three named forms, and the round trip with glu::KeyRuns (run-length encode, then decode).
#include <algorithm>
#include <random>
#include <vector>

#include "glu/Expand.hpp"
#include "glu/KeyRuns.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
constexpr uint32_t kPoison = 0xA5A5A5A5u;
}

TEST_CASE("Expand-segments-ranks-and-items-against-a-serial-restatement")
{
    std::mt19937 rng(1);
    const size_t n = 5000, total = 100003;
    // offsets[0] = 7 > 0 and offsets[n] < total: head and tail stay untouched; a third of the segments are empty
    std::vector<uint32_t> offsets(n + 1);
    offsets[0] = 7;
    for (size_t s = 0; s < n; s++) offsets[s + 1] = offsets[s] + (rng() % 3 == 0 ? 0u : rng() % 38u);
    REQUIRE(offsets[n] < total);
    std::vector<uint64_t> items(n);
    for (uint64_t& v : items) v = ((uint64_t) rng() << 32) | rng();
    std::vector<uint32_t> want_seg(total, kPoison), want_rank(total, kPoison);
    std::vector<uint64_t> want_items(total, ((uint64_t) kPoison << 32) | kPoison);
    for (size_t s = 0; s < n; s++)
        for (uint32_t j = offsets[s]; j < offsets[s + 1]; j++) want_seg[j] = (uint32_t) s, want_rank[j] = j - offsets[s], want_items[j] = items[s];

    ShaderStorageBuffer ob(offsets), ib(items), seg(total * 4), rank(total * 4), out(total * 8);
    const Expand::Plan plan = Expand::plan(total, n);
    CHECK(plan.tile == 256 * 11);
    CHECK(plan.tiles == (total + n + 1 + plan.tile - 1) / plan.tile);
    CHECK(plan.kernels == 2);
    CHECK(plan.scratch_bytes == (plan.tiles + 1) * 4);
    Expand expand;
    expand.prepare(total, n);
    seg.clear(kPoison);
    rank.clear(kPoison);
    out.clear(kPoison);
    expand((const uint32_t*) ob.device_ptr(), n, total, ib.device_ptr(), 8, out.device_ptr(), (uint32_t*) seg.device_ptr(),
           (uint32_t*) rank.device_ptr());
    CHECK(seg.get_data<uint32_t>() == want_seg);
    CHECK(rank.get_data<uint32_t>() == want_rank);
    CHECK(out.get_data<uint64_t>() == want_items);
    CHECK(expand.last().tiles == plan.tiles && expand.last().kernels == 2);

    // the named forms and the buffer form, each writing only what it names
    seg.clear(kPoison);
    rank.clear(kPoison);
    out.clear(kPoison);
    expand.segment_ids((const uint32_t*) ob.device_ptr(), n, total, (uint32_t*) seg.device_ptr());
    CHECK(seg.get_data<uint32_t>() == want_seg);
    CHECK(rank.get_data<uint32_t>() == std::vector<uint32_t>(total, kPoison));
    seg.clear(kPoison);
    expand.ranks((const uint32_t*) ob.device_ptr(), n, total, (uint32_t*) rank.device_ptr());
    CHECK(rank.get_data<uint32_t>() == want_rank);
    CHECK(seg.get_data<uint32_t>() == std::vector<uint32_t>(total, kPoison));
    rank.clear(kPoison);
    expand.gather((const uint32_t*) ob.device_ptr(), n, total, ib.device_ptr(), 8, out.device_ptr());
    CHECK(out.get_data<uint64_t>() == want_items);
    CHECK(rank.get_data<uint32_t>() == std::vector<uint32_t>(total, kPoison));
    expand(ob, n, total, seg, rank);
    CHECK(seg.get_data<uint32_t>() == want_seg);
    CHECK(rank.get_data<uint32_t>() == want_rank);
    expand((const uint32_t*) ob.device_ptr(), 0, total, nullptr, 0, nullptr, (uint32_t*) seg.device_ptr(), nullptr); // no segment
    CHECK(expand.last().tiles == 0 && expand.last().kernels == 0);
    CHECK(seg.get_data<uint32_t>() == want_seg);
    CHECK(ob.get_data<uint32_t>() == offsets);
    CHECK(ib.get_data<uint64_t>() == items);
}

TEST_CASE("Expand-decodes-what-KeyRuns-encodes")
{
    std::mt19937 rng(2);
    const size_t count = 70001, max_runs = 4096;
    std::vector<uint32_t> keys(count);
    for (uint32_t& k : keys) k = (rng() % 900) * 7919u;
    std::sort(keys.begin(), keys.end());
    ShaderStorageBuffer kb(keys), unique(max_runs * 4), offsets((max_runs + 1) * 4), num_runs(4), decoded(count * 4);
    KeyRuns runs;
    runs(kb.device_ptr(), count, 32, 0, 32, unique.device_ptr(), (uint32_t*) offsets.device_ptr(), max_runs, (uint32_t*) num_runs.device_ptr());
    // max_runs is far above the number of runs: the tail of the offsets holds `count`, trailing empty segments that expand skips
    decoded.clear(kPoison);
    Expand expand;
    expand.gather((const uint32_t*) offsets.device_ptr(), max_runs, count, unique.device_ptr(), 4, decoded.device_ptr());
    CHECK(num_runs.get_data<uint32_t>()[0] <= 900u);
    CHECK(decoded.get_data<uint32_t>() == keys);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
