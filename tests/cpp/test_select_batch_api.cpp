// C++ API test of glu::Select's batched calls: ragged segments with empty ones and a partial cover under a float stencil, with local
// indices, items and the offsets of the compacted segments; equal partitions under a byte mask with a capacity below the number
// selected -- checked against a plain loop over the stencil.
#include <algorithm>
#include <cstring>
#include <random>
#include <vector>

#include "glu/Select.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
constexpr uint32_t kPoison = 0xA5A5A5A5u;

// the contract, restated: the selected elements of [b_0, b_n), their segment-local indices and the clamped ranks of the boundaries
struct Expected
{
    std::vector<uint32_t> global, local, offsets;
};
template<typename Pred>
Expected expected(size_t total, const std::vector<uint32_t>& bounds, size_t max_out, Pred selected)
{
    Expected e;
    std::vector<uint32_t> rank(total + 1, 0);
    size_t s = 0;
    for (size_t i = 0; i < total; i++)
    {
        const bool in = i >= bounds.front() && i < bounds.back() && selected(i);
        rank[i + 1] = rank[i] + (in ? 1u : 0u);
        if (!in) continue;
        while (s + 1 < bounds.size() && bounds[s + 1] <= i) s++;
        e.global.push_back((uint32_t) i);
        e.local.push_back((uint32_t) i - bounds[s]);
    }
    for (uint32_t b : bounds) e.offsets.push_back((uint32_t) std::min<size_t>(max_out, rank[b]));
    return e;
}
} // namespace

TEST_CASE("Batched-select-over-ragged-segments-with-local-indices")
{
    std::mt19937 rng(3);
    const Select::BatchPlan one = Select::plan_batch(1, 1, SelectStencil_Float);
    const size_t total = 3 * one.tile + 17;
    std::vector<float> values(total);
    for (float& v : values) v = (float) (rng() % 2001) / 1000.0f - 1.0f;
    // segments: a partial cover from 5, empty ones, one across a tile edge, the last ends 9 in front of the end
    std::vector<uint32_t> bounds = {5, 5, 70, 70, 70, one.tile - 1, one.tile + 1, 2 * one.tile, (uint32_t) total - 9};
    const size_t segments = bounds.size() - 1, max_out = total;
    const float threshold = 0.5f;
    const Expected want = expected(total, bounds, max_out, [&](size_t i) { return values[i] > threshold; });
    const Select::BatchPlan plan = Select::plan_batch(total, segments, SelectStencil_Float, SelectIndex_Local);
    CHECK(plan.tile == Select::plan(total, SelectStencil_Float).tile && plan.tiles == Select::plan(total, SelectStencil_Float).tiles);
    CHECK(plan.kernels == 4 && plan.scan_rounds == 1 && plan.scratch_bytes >= total / 8 && plan.scratch_bytes <= total / 4 + 1024);
    CHECK(Select::plan_batch(0, segments).scratch_bytes == 0);

    ShaderStorageBuffer value_buffer(values), bound_buffer(bounds), item_buffer(max_out * 4), index_buffer(max_out * 4),
        offset_buffer((segments + 1) * 4), num_buffer(4);
    item_buffer.clear(kPoison);
    index_buffer.clear(kPoison);
    offset_buffer.clear(kPoison);
    Select select;
    select.prepare_batch(total, segments, SelectStencil_Float);
    SelectArrays a;
    a.stencil = value_buffer.device_ptr();
    a.stencil_type = SelectStencil_Float;
    a.op = SelectOperator_Greater;
    a.threshold = &threshold;
    a.count = total;
    a.items = value_buffer.device_ptr();
    a.item_bytes = 4;
    a.out_items = item_buffer.device_ptr();
    a.out_indices = (uint32_t*) index_buffer.device_ptr();
    a.max_out = max_out;
    a.num_selected = (uint32_t*) num_buffer.device_ptr();
    select.select_batch_offsets(a, (const uint32_t*) bound_buffer.device_ptr(), segments, (uint32_t*) offset_buffer.device_ptr(),
                                SelectIndex_Local);
    CHECK(num_buffer.get_data<uint32_t>()[0] == want.global.size());
    CHECK(want.global.size() > total / 8);
    CHECK(offset_buffer.get_data<uint32_t>() == want.offsets);
    std::vector<uint32_t> indices = index_buffer.get_data<uint32_t>();
    const std::vector<uint32_t> items = item_buffer.get_data<uint32_t>();
    bool same = true;
    for (size_t r = 0; r < max_out; r++)
    {
        uint32_t bits = kPoison;
        if (r < want.global.size()) memcpy(&bits, &values[want.global[r]], 4);
        same = same && indices[r] == (r < want.local.size() ? want.local[r] : kPoison) && items[r] == bits;
    }
    CHECK(same);
    // the same call in global form, indices only
    a.items = nullptr;
    a.out_items = nullptr;
    select.select_batch_offsets(a, (const uint32_t*) bound_buffer.device_ptr(), segments, nullptr);
    indices = index_buffer.get_data<uint32_t>();
    same = true;
    for (size_t r = 0; r < max_out; r++) same = same && indices[r] == (r < want.global.size() ? want.global[r] : kPoison);
    CHECK(same);
    CHECK(value_buffer.get_data<float>() == values);
    CHECK(bound_buffer.get_data<uint32_t>() == bounds);
}

TEST_CASE("Batched-select-over-equal-partitions-by-a-byte-mask-with-overflow")
{
    std::mt19937 rng(4);
    const size_t count = 255, partitions = 40, total = count * partitions;
    std::vector<uint8_t> mask(total);
    for (uint8_t& m : mask) m = rng() % 3 == 0 ? (uint8_t) (1 + rng() % 255) : 0;
    std::fill(mask.begin() + 3 * count, mask.begin() + 5 * count, (uint8_t) 0); // two partitions lose everything
    std::vector<uint32_t> bounds(partitions + 1);
    for (size_t s = 0; s <= partitions; s++) bounds[s] = (uint32_t) (s * count);
    const size_t selected = (size_t) std::count_if(mask.begin(), mask.end(), [](uint8_t m) { return m != 0; });
    const size_t max_out = selected / 2;
    const Expected want = expected(total, bounds, max_out, [&](size_t i) { return mask[i] != 0; });
    ShaderStorageBuffer mask_buffer(mask), index_buffer((max_out + 1) * 4), offset_buffer((partitions + 1) * 4), num_buffer(4);
    index_buffer.clear(kPoison);
    offset_buffer.clear(kPoison);
    Select select;
    SelectArrays a;
    a.stencil = mask_buffer.device_ptr();
    a.stencil_type = SelectStencil_Byte;
    a.out_indices = (uint32_t*) index_buffer.device_ptr();
    a.max_out = max_out;
    a.num_selected = (uint32_t*) num_buffer.device_ptr();
    select.select_batch(a, count, partitions, (uint32_t*) offset_buffer.device_ptr(), SelectIndex_Local);
    CHECK(num_buffer.get_data<uint32_t>()[0] == selected); // the true number, beyond max_out
    const std::vector<uint32_t> offsets = offset_buffer.get_data<uint32_t>();
    CHECK(offsets == want.offsets);
    CHECK(offsets[3] == offsets[4] && offsets[4] == offsets[5]); // an emptied segment stays an empty segment
    CHECK(offsets[partitions] == max_out);                        // clamped: the offsets describe what was written
    const std::vector<uint32_t> indices = index_buffer.get_data<uint32_t>();
    bool same = indices[max_out] == kPoison;
    for (size_t r = 0; r < max_out; r++) same = same && indices[r] == want.local[r];
    CHECK(same);
    CHECK(mask_buffer.get_data<uint8_t>() == mask);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
