// C++ API test of the batched sort of glu::RadixSort (sort_batch / sort_batch_offsets): every segment of an array sorted on its
// own, stable, in place -- checked against std::stable_sort of every slice.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "glu/RadixSort.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
    template<typename KeyT>
    std::vector<KeyT> random_keys(size_t n, uint32_t seed)
    {
        std::mt19937_64 rng(seed);
        std::vector<KeyT> keys(n);
        for (KeyT& k : keys)
        {
            const uint64_t r = rng();
            if constexpr (std::is_floating_point_v<KeyT>) k = (KeyT) ((double) (int64_t) (r >> 40) - 8388608.0) / (KeyT) 64;
            else k = (KeyT) ((r & 7) == 0 ? (r >> 8) & 0xFF : r >> 8); // every eighth key from a small range: ties
        }
        return keys;
    }

    /// sorts on the device, returns true if every segment equals std::stable_sort of its slice and nothing else moved
    template<typename KeyT>
    bool run_case(const std::vector<uint32_t>& offsets, size_t total, bool with_vals, size_t equal_count, uint32_t seed,
                  RadixSort::BatchReport* report = nullptr)
    {
        std::vector<KeyT> keys = random_keys<KeyT>(total, seed);
        std::vector<uint32_t> vals(total);
        std::iota(vals.begin(), vals.end(), 0u);
        ShaderStorageBuffer key_buffer(keys.data(), total * sizeof(KeyT));
        ShaderStorageBuffer val_buffer(vals);
        ShaderStorageBuffer offset_buffer(offsets);
        const size_t num_segments = offsets.size() - 1;

        RadixSort radix_sort;
        radix_sort.prepare_internal_buffers_batch(total, num_segments, sizeof(KeyT), with_vals);
        uint32_t* device_vals = with_vals ? (uint32_t*) val_buffer.device_ptr() : nullptr;
        if (equal_count)
            radix_sort.sort_batch<KeyT>((KeyT*) key_buffer.device_ptr(), device_vals, equal_count, num_segments);
        else
            radix_sort.sort_batch_offsets<KeyT>((KeyT*) key_buffer.device_ptr(), device_vals, total,
                                                (const uint32_t*) offset_buffer.device_ptr(), num_segments);
        std::vector<KeyT> got_keys = key_buffer.get_data<KeyT>();
        std::vector<uint32_t> got_vals = val_buffer.get_data<uint32_t>();
        if (report) *report = radix_sort.last_batch();

        std::vector<uint32_t> order(total);
        std::iota(order.begin(), order.end(), 0u);
        for (size_t s = 0; s < num_segments; s++)
            std::stable_sort(order.begin() + offsets[s], order.begin() + offsets[s + 1],
                             [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        for (size_t i = 0; i < total; i++)
        {
            if (std::memcmp(&got_keys[i], &keys[order[i]], sizeof(KeyT)) != 0) return false;
            if (with_vals && got_vals[i] != order[i]) return false;
            if (!with_vals && got_vals[i] != i) return false;
        }
        return true;
    }

    std::vector<uint32_t> mixed_offsets(uint32_t seed, uint32_t head, size_t& total)
    {
        std::mt19937 rng(seed);
        std::vector<uint32_t> lengths = {0, 1, 2, 64, 65, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385, 50000, 0, 1};
        for (int i = 0; i < 400; i++) lengths.push_back(rng() % 100);
        for (int i = 0; i < 40; i++) lengths.push_back(rng() % 3000);
        std::shuffle(lengths.begin(), lengths.end(), rng);
        std::vector<uint32_t> offsets = {head};
        for (uint32_t len : lengths) offsets.push_back(offsets.back() + len);
        total = offsets.back() + 321; // elements behind the last segment
        return offsets;
    }
} // namespace

TEST_CASE("RadixSort-batch-equal-partitions")
{
    for (size_t count : {1u, 2u, 64u, 500u, 513u, 4096u, 16384u, 20000u})
    {
        const size_t parts = count < 5000 ? 37 : 3;
        std::vector<uint32_t> offsets(parts + 1);
        for (size_t s = 0; s <= parts; s++) offsets[s] = (uint32_t) (s * count);
        RadixSort::BatchReport report;
        CHECK(run_case<uint32_t>(offsets, count * parts, true, count, (uint32_t) count, &report));
        CHECK(report.wave_segments + report.block_segments + report.long_segments == (count > 1 ? parts : 0));
    }
}

TEST_CASE("RadixSort-batch-offsets-every-key-type")
{
    size_t total = 0;
    const std::vector<uint32_t> offsets = mixed_offsets(7, 100, total);
    RadixSort::BatchReport report;
    CHECK(run_case<uint32_t>(offsets, total, true, 0, 1, &report));
    CHECK(report.wave_segments > 0);
    CHECK(report.block_segments > 0);
    CHECK(report.long_segments > 0);
    CHECK(run_case<int32_t>(offsets, total, true, 0, 2));
    CHECK(run_case<float>(offsets, total, false, 0, 3));
    CHECK(run_case<uint64_t>(offsets, total, true, 0, 4));
    CHECK(run_case<int64_t>(offsets, total, false, 0, 5));
    CHECK(run_case<double>(offsets, total, true, 0, 6));
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
