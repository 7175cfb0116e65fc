// C++ API test of glu::Select: values above a threshold with their indices, a byte mask over 16-byte items, and a capacity below
// the number selected -- checked against a plain loop over the stencil.
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "glu/Select.hpp"
#include "util/mini_test.hpp"

using namespace glu;

TEST_CASE("Select-if-on-float-values-with-indices")
{
    std::mt19937 rng(1);
    const size_t count = 3 * Select::plan(1, SelectStencil_Float).tile + 77;
    std::vector<float> values(count);
    for (size_t i = 0; i < count; i++) values[i] = (float) (rng() % 2001) / 1000.0f - 1.0f;
    values[5] = std::numeric_limits<float>::quiet_NaN();
    values[6] = -0.0f;
    const float threshold = 0.25f;
    std::vector<uint32_t> want_indices;
    std::vector<float> want_items;
    for (size_t i = 0; i < count; i++)
        if (values[i] > threshold)
        {
            want_indices.push_back((uint32_t) i);
            want_items.push_back(values[i]);
        }
    const size_t max_out = count;
    ShaderStorageBuffer value_buffer(values), item_buffer(max_out * sizeof(float)), index_buffer(max_out * sizeof(uint32_t)),
        num_buffer(sizeof(uint32_t));
    item_buffer.clear(0xA5A5A5A5u);
    index_buffer.clear(0xA5A5A5A5u);
    Select select;
    const Select::Plan plan = Select::plan(count, SelectStencil_Float);
    CHECK(plan.tile > 0);
    CHECK(plan.tiles == (count + plan.tile - 1) / plan.tile);
    CHECK(plan.scan_rounds == 1);
    select.prepare(count, SelectStencil_Float);
    select(value_buffer.device_ptr(), SelectStencil_Float, SelectOperator_Greater, &threshold, count, value_buffer.device_ptr(),
           Select::item_bytes(DataType_Float), item_buffer.device_ptr(), (uint32_t*) index_buffer.device_ptr(), max_out,
           (uint32_t*) num_buffer.device_ptr());
    const std::vector<uint32_t> indices = index_buffer.get_data<uint32_t>();
    const std::vector<uint32_t> items = item_buffer.get_data<uint32_t>();
    CHECK(num_buffer.get_data<uint32_t>()[0] == want_indices.size());
    CHECK(want_indices.size() > count / 4 && want_indices.size() < count / 2);
    bool same = true;
    for (size_t r = 0; r < max_out; r++)
    {
        uint32_t bits = 0xA5A5A5A5u;
        if (r < want_items.size()) memcpy(&bits, &want_items[r], 4);
        same = same && indices[r] == (r < want_indices.size() ? want_indices[r] : 0xA5A5A5A5u) && items[r] == bits;
    }
    CHECK(same);
    // a NaN passes NotEqual only, and -0.0 equals +0.0: with the threshold +0.0, Equal selects element 6 and not element 5
    const float zero = 0.0f;
    select(value_buffer.device_ptr(), SelectStencil_Float, SelectOperator_Equal, &zero, 16, nullptr, 0, nullptr,
           (uint32_t*) index_buffer.device_ptr(), 16, (uint32_t*) num_buffer.device_ptr());
    const uint32_t zeros = num_buffer.get_data<uint32_t>()[0];
    const std::vector<uint32_t> zero_indices = index_buffer.get_data<uint32_t>();
    bool six = false, five = false;
    for (uint32_t r = 0; r < zeros; r++)
    {
        six = six || zero_indices[r] == 6;
        five = five || zero_indices[r] == 5;
    }
    CHECK(six && !five);
}

TEST_CASE("Select-by-a-byte-mask-with-wide-items-and-overflow")
{
    std::mt19937 rng(2);
    const size_t count = 2 * Select::plan(1, SelectStencil_Byte).tile + 13;
    std::vector<uint8_t> mask(count);
    std::vector<uint32_t> items(4 * count); // (uvec4 items)
    for (size_t i = 0; i < count; i++) mask[i] = rng() % 3 == 0 ? (uint8_t) (1 + rng() % 255) : 0;
    for (uint32_t& v : items) v = rng();
    std::vector<uint32_t> want;
    for (size_t i = 0; i < count; i++)
        if (mask[i]) want.push_back((uint32_t) i);
    const size_t max_out = want.size() / 2; // fewer than are selected
    ShaderStorageBuffer mask_buffer(mask), item_buffer(items), out_buffer((max_out + 1) * 16), num_buffer(sizeof(uint32_t));
    out_buffer.clear(0xA5A5A5A5u);
    Select select;
    SelectArrays a;
    a.stencil = mask_buffer.device_ptr();
    a.stencil_type = SelectStencil_Byte;
    a.count = count;
    a.items = item_buffer.device_ptr();
    a.item_bytes = Select::item_bytes(DataType_UVec4);
    a.out_items = out_buffer.device_ptr();
    a.max_out = max_out;
    a.num_selected = (uint32_t*) num_buffer.device_ptr();
    CHECK(a.item_bytes == 16);
    CHECK(Select::item_bytes(DataType_DVec4) == 32);
    select(a); // (NotEqual against a null threshold: the flags form)
    const std::vector<uint32_t> out = out_buffer.get_data<uint32_t>();
    CHECK(num_buffer.get_data<uint32_t>()[0] == want.size()); // the true number, beyond max_out
    bool same = true;
    for (size_t r = 0; r < max_out; r++)
        for (size_t w = 0; w < 4; w++) same = same && out[4 * r + w] == items[4 * (size_t) want[r] + w];
    for (size_t w = 0; w < 4; w++) same = same && out[4 * max_out + w] == 0xA5A5A5A5u; // (the entry behind max_out: not touched)
    CHECK(same);
    CHECK(mask_buffer.get_data<uint8_t>() == mask);
    CHECK(item_buffer.get_data<uint32_t>() == items);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
