// C++ API test of glu::TopK's batched calls: the k smallest (sorted) of equal partitions and the k largest (unsorted) of segments
// given by device offsets, of uint32 keys with duplicates, against std::stable_sort of (key, index) per segment; local indices, rows
// of stride k, entries behind min(k, length) untouched; the k-th keys alone; what the object reports of the last batched call.
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "glu/TopK.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
constexpr uint32_t kPoison = 0xA5A5A5A5u;

// the first min(k, len) local indices of the stable sort of keys[begin, begin + len)
std::vector<uint32_t> head(const std::vector<uint32_t>& keys, size_t begin, size_t len, size_t k, bool largest)
{
    std::vector<uint32_t> order(len);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return largest ? keys[begin + a] > keys[begin + b] : keys[begin + a] < keys[begin + b]; });
    order.resize(std::min(k, len));
    return order;
}
} // namespace

TEST_CASE("TopK-smallest-batch-of-equal-partitions-sorted")
{
    std::mt19937 rng(3);
    const size_t count = 3000, parts = 37, k = 50;
    std::vector<uint32_t> keys(count * parts);
    for (uint32_t& v : keys) v = (rng() % 900u) * 7919u;
    ShaderStorageBuffer kb(keys), ok((parts * k + 8) * 4), oi((parts * k + 8) * 4), kth(parts * 4);
    TopK topk;
    topk.prepare_batch(count * parts, parts, k);
    ok.clear(kPoison);
    oi.clear(kPoison);
    topk.smallest_batch(kb, count, parts, k, ok, oi);
    const std::vector<uint32_t> got_i = oi.get_data<uint32_t>(), got_k = ok.get_data<uint32_t>();
    topk.kth_batch(kb.device_ptr(), count, parts, k, kth.device_ptr());
    const std::vector<uint32_t> got_t = kth.get_data<uint32_t>();
    for (size_t p = 0; p < parts; p++)
    {
        const std::vector<uint32_t> want = head(keys, p * count, count, k, false);
        for (size_t r = 0; r < k; r++) CHECK(got_i[p * k + r] == want[r] && got_k[p * k + r] == keys[p * count + want[r]]);
        CHECK(got_t[p] == keys[p * count + want[k - 1]]);
    }
    for (size_t r = parts * k; r < parts * k + 8; r++) CHECK(got_i[r] == kPoison && got_k[r] == kPoison);
    const TopK::LastBatch last = topk.read_batch();
    CHECK(last.wave_segments + last.block_segments + last.long_segments == parts && last.kernels == 1);
    CHECK(kb.get_data<uint32_t>() == keys);
}

TEST_CASE("TopK-largest-batch-of-device-offsets-unsorted")
{
    std::mt19937 rng(4);
    const std::vector<uint32_t> lengths = {0, 1, 7, 600, 0, 5000, 40000, 3, 70000, 512};
    std::vector<uint32_t> offsets = {1};
    for (uint32_t n : lengths) offsets.push_back(offsets.back() + n);
    const size_t total = offsets.back() + 2, segments = lengths.size(), k = 9;
    std::vector<uint32_t> keys(total);
    for (uint32_t& v : keys) v = (rng() % 5000u) * 104729u;
    ShaderStorageBuffer kb(keys), ob(offsets), ok(segments * k * 4), oi(segments * k * 4);
    TopK topk;
    ok.clear(kPoison);
    oi.clear(kPoison);
    topk.largest_batch_offsets(kb, total, ob, segments, k, ok, oi, false);
    const std::vector<uint32_t> got_i = oi.get_data<uint32_t>(), got_k = ok.get_data<uint32_t>();
    for (size_t s = 0; s < segments; s++)
    {
        std::vector<uint32_t> want = head(keys, offsets[s], lengths[s], k, true);
        std::sort(want.begin(), want.end());
        for (size_t r = 0; r < want.size(); r++) CHECK(got_i[s * k + r] == want[r] && got_k[s * k + r] == keys[offsets[s] + want[r]]);
        for (size_t r = want.size(); r < k; r++) CHECK(got_i[s * k + r] == kPoison && got_k[s * k + r] == kPoison);
    }
    const TopK::LastBatch last = topk.read_batch();
    CHECK(last.wave_segments + last.block_segments + last.long_segments == 8 && last.wave_segments >= 4 && last.long_segments >= 1);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
