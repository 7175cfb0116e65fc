// C++ API test of the batched reduce of glu::Reduce (reduce_batch / reduce_batch_offsets): every segment of an array folded on its
// own into out[segment], the input left alone -- checked against a plain loop over every slice.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "glu/Reduce.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
    template<typename S>
    S identity_of(ReduceOperator op)
    {
        if (op == ReduceOperator_Sum) return (S) 0;
        if (op == ReduceOperator_Mul) return (S) 1;
        if (std::is_floating_point_v<S>)
            return op == ReduceOperator_Min ? std::numeric_limits<S>::infinity() : -std::numeric_limits<S>::infinity();
        return op == ReduceOperator_Min ? std::numeric_limits<S>::max() : std::numeric_limits<S>::lowest();
    }

    template<typename S>
    S combine(ReduceOperator op, S a, S b)
    {
        if constexpr (std::is_same_v<S, int32_t>)
        {
            if (op == ReduceOperator_Sum) return (int32_t) ((uint32_t) a + (uint32_t) b);
            if (op == ReduceOperator_Mul) return (int32_t) ((uint32_t) a * (uint32_t) b);
        }
        if (op == ReduceOperator_Sum) return a + b;
        if (op == ReduceOperator_Mul) return a * b;
        return op == ReduceOperator_Min ? std::min(a, b) : std::max(a, b);
    }

    /// values whose sums are exact in every order (multiples of 1/8 of small magnitude); products: mostly ones
    template<typename S>
    std::vector<S> inputs(size_t scalars, ReduceOperator op, uint32_t seed)
    {
        std::mt19937 rng(seed);
        std::vector<S> data(scalars);
        for (S& v : data)
        {
            const uint32_t r = rng();
            if (op == ReduceOperator_Mul) v = (r % 4096u) == 0 ? (S) 2 : (S) 1;
            else if constexpr (std::is_floating_point_v<S>) v = (S) ((int) (r % 8000u) - 4000) * (S) 0.125;
            else v = (S) r;
        }
        return data;
    }

    /// reduces on the device (equal_count != 0: equal partitions), returns true if every out[s] is the fold of its slice, the
    /// elements of out behind the segments and the whole input are untouched
    template<typename S>
    bool run_case(DataType data_type, int components, ReduceOperator op, const std::vector<uint32_t>& offsets, size_t total,
                  size_t equal_count, uint32_t seed, Reduce::BatchReport* report = nullptr)
    {
        const size_t num_segments = offsets.size() - 1;
        const std::vector<S> data = inputs<S>(total * components, op, seed);
        const S guard = (S) 77;
        std::vector<S> out((num_segments + 3) * components, guard);
        const std::vector<S> uploaded = data.empty() ? std::vector<S>(1, guard) : data; // (a buffer cannot be made from no data)
        ShaderStorageBuffer data_buffer(uploaded);
        ShaderStorageBuffer out_buffer(out);
        ShaderStorageBuffer offset_buffer(offsets);

        Reduce reduce(data_type, op);
        reduce.prepare_batch(total, num_segments);
        if (equal_count)
            reduce.reduce_batch(data_buffer.device_ptr(), out_buffer.device_ptr(), equal_count, num_segments);
        else
            reduce.reduce_batch_offsets(data_buffer.device_ptr(), out_buffer.device_ptr(), total, (const uint32_t*) offset_buffer.device_ptr(),
                                        num_segments);
        const std::vector<S> got = out_buffer.get_data<S>();
        const std::vector<S> data_after = data_buffer.get_data<S>();
        if (report) *report = reduce.last_batch();

        if (std::memcmp(data_after.data(), uploaded.data(), uploaded.size() * sizeof(S)) != 0) return false;
        for (size_t s = 0; s < num_segments; s++)
            for (int c = 0; c < components; c++)
            {
                S want = identity_of<S>(op);
                for (size_t i = offsets[s]; i < offsets[s + 1]; i++) want = i == offsets[s] ? data[i * components + c] : combine(op, want, data[i * components + c]);
                if (std::memcmp(&got[s * components + c], &want, sizeof(S)) != 0) return false;
            }
        for (size_t i = num_segments * components; i < got.size(); i++)
            if (got[i] != guard) return false;
        return true;
    }

    std::vector<uint32_t> mixed_offsets(uint32_t seed, uint32_t head, size_t& total)
    {
        std::mt19937 rng(seed);
        std::vector<uint32_t> lengths = {0, 1, 2, 16, 17, 64, 65, 128, 129, 1024, 1025, 8192, 8193, 65536, 65537, 200000, 0, 1};
        for (int i = 0; i < 400; i++) lengths.push_back(rng() % 100);
        for (int i = 0; i < 40; i++) lengths.push_back(rng() % 3000);
        std::shuffle(lengths.begin(), lengths.end(), rng);
        std::vector<uint32_t> offsets = {head};
        for (uint32_t len : lengths) offsets.push_back(offsets.back() + len);
        total = offsets.back() + 321; // elements behind the last segment
        return offsets;
    }
} // namespace

TEST_CASE("Reduce-batch-equal-partitions")
{
    for (size_t count : {0u, 1u, 4u, 32u, 100u, 1024u, 1025u, 65536u, 65537u, 300000u})
    {
        const size_t parts = count < 5000 ? 37 : 3;
        std::vector<uint32_t> offsets(parts + 1);
        for (size_t s = 0; s <= parts; s++) offsets[s] = (uint32_t) (s * count);
        Reduce::BatchReport report;
        CHECK(run_case<uint32_t>(DataType_Uint, 1, ReduceOperator_Sum, offsets, count * parts, count, (uint32_t) count, &report));
        CHECK(report.wave_segments + report.block_segments + report.long_segments == (count ? parts : 0));
        if (count == 0) // (equal_count == 0 selects the offsets form above: the equal-partition form of empty partitions, by hand)
        {
            std::vector<float> out(parts + 1, 5.0f);
            ShaderStorageBuffer out_buffer(out);
            Reduce reduce(DataType_Float, ReduceOperator_Min);
            reduce.reduce_batch(nullptr, out_buffer.device_ptr(), 0, parts);
            out = out_buffer.get_data<float>();
            for (size_t s = 0; s < parts; s++) CHECK(out[s] == std::numeric_limits<float>::infinity());
            CHECK(out[parts] == 5.0f);
        }
    }
}

TEST_CASE("Reduce-batch-offsets-types-and-operators")
{
    size_t total = 0;
    const std::vector<uint32_t> offsets = mixed_offsets(7, 100, total);
    Reduce::BatchReport report;
    CHECK(run_case<uint32_t>(DataType_Uint, 1, ReduceOperator_Sum, offsets, total, 0, 1, &report));
    CHECK(report.wave_segments > 0);
    CHECK(report.block_segments > 0);
    CHECK(report.long_segments > 0);
    CHECK(run_case<int32_t>(DataType_Int, 1, ReduceOperator_Max, offsets, total, 0, 2));
    CHECK(run_case<float>(DataType_Float, 1, ReduceOperator_Min, offsets, total, 0, 3));
    CHECK(run_case<float>(DataType_Vec2, 2, ReduceOperator_Sum, offsets, total, 0, 4));
    CHECK(run_case<double>(DataType_Double, 1, ReduceOperator_Mul, offsets, total, 0, 5));
    CHECK(run_case<int32_t>(DataType_IVec4, 4, ReduceOperator_Min, offsets, total, 0, 6));
    CHECK(run_case<double>(DataType_DVec4, 4, ReduceOperator_Sum, offsets, total, 0, 7));
}

/// Four equal partitions that hold the same long float segment of three chunks, every chunk +0.0 but for one element, so that the
/// three partials are exactly 2^24, 1 and -2^24: (2^24 + 1) - 2^24 is 0 and (2^24 - 2^24) + 1 is 1.  The partitions' runs of
/// partials start at slots 0, 3, 6 and 9 -- every residue modulo the four floats of a 16-byte pack -- and a result may depend on
/// the segment's alignment, length and data only: the four must be the same bits.
TEST_CASE("Reduce-batch-equal-partitions-of-identical-floats-that-round")
{
    auto workgroups_of = [](size_t count) {
        uint32_t path = 0, workgroups = 0;
        GLU_CHECK_STATUS(glu_reduce_plan_batch(count, (uint32_t) sizeof(float), &path, &workgroups));
        return path == 3 ? workgroups : 0u;
    };
    size_t chunk = 1; // elements of a long segment's chunk (= the longest segment of one workgroup)
    while (workgroups_of(2 * chunk) == 0) chunk *= 2;
    const size_t parts = 4, count = 3 * chunk - 8;
    CHECK(workgroups_of(chunk) == 0);
    CHECK(workgroups_of(chunk + 1) == 2);
    CHECK(workgroups_of(count) == 3);

    std::vector<float> data(count * parts, 0.0f);
    for (size_t p = 0; p < parts; p++)
    {
        data[p * count + 12345] = 16777216.0f;
        data[p * count + chunk + 777] = 1.0f;
        data[p * count + 2 * chunk + 4321] = -16777216.0f;
    }
    std::vector<float> out(parts + 1, 77.0f);
    ShaderStorageBuffer data_buffer(data);
    ShaderStorageBuffer out_buffer(out);
    Reduce reduce(DataType_Float, ReduceOperator_Sum);
    reduce.reduce_batch(data_buffer.device_ptr(), out_buffer.device_ptr(), count, parts);
    out = out_buffer.get_data<float>();
    CHECK(reduce.last_batch().long_segments == parts);
    for (size_t p = 0; p < parts; p++)
    {
        if (std::memcmp(&out[p], &out[0], sizeof(float)) != 0) printf("partition %zu: %g, partition 0: %g\n", p, out[p], out[0]);
        CHECK(std::memcmp(&out[p], &out[0], sizeof(float)) == 0);
        CHECK(out[p] == 0.0f || out[p] == 1.0f);
    }
    CHECK(out[parts] == 77.0f);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
