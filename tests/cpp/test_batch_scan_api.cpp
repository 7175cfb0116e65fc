// C++ API test of the batched scan of glu::BlellochScan (scan_batch_offsets): every segment of an array replaced by its own
// exclusive sum, in place, the rest of the array left alone -- checked against a plain loop over every slice.
#include <algorithm>
#include <cstring>
#include <random>
#include <vector>

#include "glu/BlellochScan.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
    template<typename S>
    S add(S a, S b)
    {
        if constexpr (std::is_same_v<S, int32_t>) return (int32_t) ((uint32_t) a + (uint32_t) b);
        else return a + b;
    }

    /// values whose sums are exact in every order: multiples of 1/8 of small magnitude (segments here hold at most 200000 elements
    /// of magnitude up to 40/8: 200000 * 40 < 2^24); integers: any word
    template<typename S>
    std::vector<S> inputs(size_t scalars, uint32_t seed)
    {
        std::mt19937 rng(seed);
        std::vector<S> data(scalars);
        for (S& v : data)
        {
            const uint32_t r = rng();
            if constexpr (std::is_floating_point_v<S>) v = (S) ((int) (r % 81u) - 40) * (S) 0.125;
            else v = (S) r;
        }
        return data;
    }

    /// scans on the device, returns true if every segment is the exclusive sum of its slice and everything else is untouched
    template<typename S>
    bool run_case(DataType data_type, int components, const std::vector<uint32_t>& offsets, size_t total, uint32_t seed,
                  BlellochScan::BatchReport* report = nullptr)
    {
        const size_t num_segments = offsets.size() - 1;
        const std::vector<S> data = inputs<S>(total * components, seed);
        ShaderStorageBuffer data_buffer(data);
        ShaderStorageBuffer offset_buffer(offsets);

        BlellochScan scan(data_type);
        scan.prepare_batch(total, num_segments);
        scan.scan_batch_offsets(data_buffer.device_ptr(), total, (const uint32_t*) offset_buffer.device_ptr(), num_segments);
        const std::vector<S> got = data_buffer.get_data<S>();
        if (report) *report = scan.read_batch();

        std::vector<S> want = data;
        for (size_t s = 0; s < num_segments; s++)
            for (int c = 0; c < components; c++)
            {
                S acc = (S) 0;
                for (size_t i = offsets[s]; i < offsets[s + 1]; i++)
                {
                    want[i * components + c] = acc;
                    acc = add(acc, data[i * components + c]);
                }
            }
        return std::memcmp(got.data(), want.data(), want.size() * sizeof(S)) == 0;
    }

    std::vector<uint32_t> mixed_offsets(uint32_t seed, uint32_t head, size_t& total)
    {
        std::mt19937 rng(seed);
        std::vector<uint32_t> lengths = {0, 1, 2, 16, 17, 64, 65, 128, 129, 1024, 1025, 8192, 8193, 16384, 16385, 65536, 65537, 200000, 0, 1};
        for (int i = 0; i < 400; i++) lengths.push_back(rng() % 100);
        for (int i = 0; i < 40; i++) lengths.push_back(rng() % 3000);
        std::shuffle(lengths.begin(), lengths.end(), rng);
        std::vector<uint32_t> offsets = {head};
        for (uint32_t len : lengths) offsets.push_back(offsets.back() + len);
        total = offsets.back() + 321; // elements behind the last segment
        return offsets;
    }
} // namespace

TEST_CASE("Scan-batch-offsets-types")
{
    size_t total = 0;
    const std::vector<uint32_t> offsets = mixed_offsets(7, 100, total);
    BlellochScan::BatchReport report;
    CHECK(run_case<uint32_t>(DataType_Uint, 1, offsets, total, 1, &report));
    CHECK(report.wave_segments > 0);
    CHECK(report.block_segments > 0);
    CHECK(report.long_segments > 0);
    CHECK(run_case<int32_t>(DataType_Int, 1, offsets, total, 2));
    CHECK(run_case<float>(DataType_Float, 1, offsets, total, 3));
    CHECK(run_case<float>(DataType_Vec2, 2, offsets, total, 4));
    CHECK(run_case<double>(DataType_Double, 1, offsets, total, 5));
    CHECK(run_case<int32_t>(DataType_IVec4, 4, offsets, total, 6));
    CHECK(run_case<double>(DataType_DVec4, 4, offsets, total, 7));
}

TEST_CASE("Scan-batch-no-segments-and-empty-segments")
{
    std::vector<uint32_t> data(100, 5u);
    ShaderStorageBuffer data_buffer(data);
    const std::vector<uint32_t> offsets = {10, 10, 10, 20, 20};
    ShaderStorageBuffer offset_buffer(offsets);
    BlellochScan scan(DataType_Uint);
    scan.scan_batch_offsets(nullptr, 100, nullptr, 0);
    scan.scan_batch_offsets(data_buffer.device_ptr(), 100, (const uint32_t*) offset_buffer.device_ptr(), 4);
    const std::vector<uint32_t> got = data_buffer.get_data<uint32_t>();
    for (size_t i = 0; i < 100; i++) CHECK(got[i] == (i >= 10 && i < 20 ? 5u * (uint32_t) (i - 10) : 5u));
    const BlellochScan::BatchReport report = scan.read_batch();
    CHECK(report.wave_segments == 1);
    CHECK(report.block_segments + report.long_segments == 0);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
