// C++ API test of glu::KeyRuns and of the two compositions over it, glu::Reduce::reduce_by_key and glu::BlellochScan::scan_by_key:
// sorted keys with runs of many lengths -- checked against a plain loop over the keys.
#include <algorithm>
#include <random>
#include <vector>

#include "glu/BlellochScan.hpp"
#include "glu/KeyRuns.hpp"
#include "glu/Reduce.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
    /// non-decreasing keys: runs of 1 .. 3000 equal keys, a few of them longer than a tile
    template<typename K>
    std::vector<K> sorted_keys(size_t runs, uint32_t seed)
    {
        std::mt19937 rng(seed);
        std::vector<K> keys;
        K key = 5;
        for (size_t r = 0; r < runs; r++)
        {
            const size_t len = r % 97 == 0 ? 5000 + rng() % 4000 : r % 7 == 0 ? 1 + rng() % 3000 : 1 + rng() % 4;
            keys.insert(keys.end(), len, key);
            key += (K) (1 + rng() % 1000);
        }
        return keys;
    }

    std::vector<uint32_t> heads_of(const std::vector<uint32_t>& keys)
    {
        std::vector<uint32_t> heads;
        for (size_t i = 0; i < keys.size(); i++)
            if (i == 0 || keys[i] != keys[i - 1]) heads.push_back((uint32_t) i);
        return heads;
    }
} // namespace

TEST_CASE("KeyRuns-offsets-unique-keys-and-count")
{
    const std::vector<uint64_t> keys = sorted_keys<uint64_t>(700, 1);
    const size_t count = keys.size(), max_runs = 1000;
    std::vector<uint32_t> heads;
    for (size_t i = 0; i < count; i++)
        if (i == 0 || keys[i] != keys[i - 1]) heads.push_back((uint32_t) i);
    ShaderStorageBuffer key_buffer(keys), unique_buffer(max_runs * sizeof(uint64_t)), offset_buffer((max_runs + 1) * sizeof(uint32_t)),
        num_buffer(sizeof(uint32_t));
    unique_buffer.clear(0xA5A5A5A5u);
    KeyRuns runs;
    const KeyRuns::Plan plan = KeyRuns::plan(count, 64);
    CHECK(plan.tile > 0);
    CHECK(plan.tiles == (count + plan.tile - 1) / plan.tile);
    runs.prepare(count, 64);
    runs(key_buffer.device_ptr(), count, 64, 0, 64, unique_buffer.device_ptr(), (uint32_t*) offset_buffer.device_ptr(), max_runs,
         (uint32_t*) num_buffer.device_ptr());
    const std::vector<uint32_t> offsets = offset_buffer.get_data<uint32_t>();
    const std::vector<uint64_t> unique = unique_buffer.get_data<uint64_t>();
    CHECK(num_buffer.get_data<uint32_t>()[0] == heads.size());
    CHECK(heads.size() == 700);
    bool same = true;
    for (size_t r = 0; r <= max_runs; r++) same = same && offsets[r] == (r < heads.size() ? heads[r] : (uint32_t) count);
    for (size_t r = 0; r < max_runs; r++) same = same && unique[r] == (r < heads.size() ? keys[heads[r]] : 0xA5A5A5A5A5A5A5A5ull);
    CHECK(same);
    CHECK(key_buffer.get_data<uint64_t>() == keys);
}

TEST_CASE("Reduce-by-key")
{
    const std::vector<uint32_t> keys = sorted_keys<uint32_t>(900, 2);
    const size_t count = keys.size(), max_runs = 1024;
    const std::vector<uint32_t> heads = heads_of(keys);
    std::mt19937 rng(3);
    std::vector<uint32_t> values(count);
    for (uint32_t& v : values) v = rng();
    ShaderStorageBuffer key_buffer(keys), value_buffer(values), out_buffer(max_runs * sizeof(uint32_t)),
        unique_buffer(max_runs * sizeof(uint32_t)), offset_buffer((max_runs + 1) * sizeof(uint32_t)), num_buffer(sizeof(uint32_t));
    KeyRuns runs;
    Reduce reduce(DataType_Uint, ReduceOperator_Sum);
    KeyRunsArrays k;
    k.keys = key_buffer.device_ptr();
    k.count = count;
    k.unique_keys = unique_buffer.device_ptr();
    k.offsets = (uint32_t*) offset_buffer.device_ptr();
    k.max_runs = max_runs;
    k.num_runs = (uint32_t*) num_buffer.device_ptr();
    reduce.reduce_by_key(runs, k, value_buffer.device_ptr(), out_buffer.device_ptr());
    const std::vector<uint32_t> out = out_buffer.get_data<uint32_t>();
    CHECK(num_buffer.get_data<uint32_t>()[0] == heads.size());
    bool same = true;
    for (size_t r = 0; r < max_runs; r++)
    {
        uint32_t want = 0;
        if (r < heads.size())
            for (size_t i = heads[r]; i < (r + 1 < heads.size() ? heads[r + 1] : count); i++) want += values[i];
        same = same && out[r] == want;
    }
    CHECK(same);
    CHECK(value_buffer.get_data<uint32_t>() == values);
}

TEST_CASE("Scan-by-key")
{
    const std::vector<uint32_t> keys = sorted_keys<uint32_t>(900, 4);
    const size_t count = keys.size(), max_runs = 900;
    std::mt19937 rng(5);
    std::vector<uint32_t> values(count);
    for (uint32_t& v : values) v = rng();
    ShaderStorageBuffer key_buffer(keys), value_buffer(values), offset_buffer((max_runs + 1) * sizeof(uint32_t)), num_buffer(sizeof(uint32_t));
    KeyRuns runs;
    BlellochScan scan(DataType_Uint);
    KeyRunsArrays k;
    k.keys = key_buffer.device_ptr();
    k.count = count;
    k.offsets = (uint32_t*) offset_buffer.device_ptr();
    k.max_runs = max_runs;
    k.num_runs = (uint32_t*) num_buffer.device_ptr();
    scan.scan_by_key(runs, k, value_buffer.device_ptr());
    const std::vector<uint32_t> got = value_buffer.get_data<uint32_t>();
    std::vector<uint32_t> want(count);
    uint32_t acc = 0;
    for (size_t i = 0; i < count; i++)
    {
        if (i == 0 || keys[i] != keys[i - 1]) acc = 0;
        want[i] = acc;
        acc += values[i];
    }
    CHECK(got == want);
    CHECK(num_buffer.get_data<uint32_t>()[0] == 900);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
