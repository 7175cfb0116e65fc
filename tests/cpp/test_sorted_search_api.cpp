// C++ API test of glu::SortedSearch: equal ranges of uint32 needles on both paths and with a reused index, and lower bounds of
// float needles in a haystack that glu::RadixSort sorted (both zeros, an infinity and a NaN among them) -- checked against
// std::lower_bound and std::upper_bound on the host.
#include <algorithm>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "glu/RadixSort.hpp"
#include "glu/SortedSearch.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
// the sort's order of floats, as unsigned keys
uint32_t float_key(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
} // namespace

TEST_CASE("SortedSearch-equal-range-on-both-paths-and-with-a-reused-index")
{
    std::mt19937 rng(1);
    const size_t hay_count = 100003, needle_count = 5000;
    std::vector<uint32_t> hay(hay_count), needles(needle_count);
    for (uint32_t& k : hay) k = rng() % 30000; // (duplicates)
    std::sort(hay.begin(), hay.end());
    for (uint32_t& k : needles) k = rng() % 30010;
    needles[0] = 0;
    needles[1] = 0xFFFFFFFFu;
    std::vector<uint32_t> want_lower(needle_count), want_upper(needle_count);
    for (size_t j = 0; j < needle_count; j++)
    {
        want_lower[j] = (uint32_t) (std::lower_bound(hay.begin(), hay.end(), needles[j]) - hay.begin());
        want_upper[j] = (uint32_t) (std::upper_bound(hay.begin(), hay.end(), needles[j]) - hay.begin());
    }
    ShaderStorageBuffer hay_buffer(hay), needle_buffer(needles), lower_buffer(needle_count * 4), upper_buffer(needle_count * 4);
    uint32_t* lower = (uint32_t*) lower_buffer.device_ptr();
    uint32_t* upper = (uint32_t*) upper_buffer.device_ptr();
    SortedSearch search;
    const SortedSearch::Plan plan = SortedSearch::plan(hay_count, needle_count);
    CHECK(plan.fanout == 32);
    CHECK(plan.levels == 1); // 100003 / 32 = 3125 entries fit LDS
    CHECK(plan.path == SearchPath_Indexed);
    CHECK(plan.index_bytes == (3125 * 4 + 127) / 128 * 128);
    search.prepare(hay_count);
    for (SearchPath path : {SearchPath_Direct, SearchPath_Indexed, SearchPath_Auto})
    {
        lower_buffer.clear(0xA5A5A5A5u);
        upper_buffer.clear(0xA5A5A5A5u);
        search.set_path(path);
        search.equal_range(hay_buffer.device_ptr(), hay_count, needle_buffer.device_ptr(), needle_count, GLU_KEY_UINT32, lower, upper);
        CHECK(lower_buffer.get_data<uint32_t>() == want_lower);
        CHECK(upper_buffer.get_data<uint32_t>() == want_upper);
        const SortedSearch::Last last = search.last();
        CHECK(last.path == (path == SearchPath_Direct ? SearchPath_Direct : SearchPath_Indexed));
        CHECK(last.kernels == (path == SearchPath_Direct ? 1u : 2u));
        CHECK(last.levels == (path == SearchPath_Direct ? 0u : 1u));
    }
    // the index once, then searches that enqueue one kernel each
    search.set_path(SearchPath_Auto);
    search.index(hay_buffer.device_ptr(), hay_count);
    CHECK(search.last().kernels == 1);
    upper_buffer.clear(0xA5A5A5A5u);
    search(hay_buffer.device_ptr(), hay_count, needle_buffer.device_ptr(), 7, GLU_KEY_UINT32, nullptr, upper, true);
    CHECK(search.last().kernels == 1 && search.last().path == SearchPath_Indexed);
    std::vector<uint32_t> got = upper_buffer.get_data<uint32_t>();
    bool same = true;
    for (size_t j = 0; j < needle_count; j++) same = same && got[j] == (j < 7 ? want_upper[j] : 0xA5A5A5A5u);
    CHECK(same);
    CHECK(hay_buffer.get_data<uint32_t>() == hay);
    CHECK(needle_buffer.get_data<uint32_t>() == needles);
}

TEST_CASE("SortedSearch-lower-bound-of-floats-in-the-sorts-order")
{
    std::mt19937 rng(2);
    const size_t hay_count = 40000, needle_count = 3000;
    std::vector<float> hay(hay_count), needles(needle_count);
    for (float& f : hay) f = (float) ((int) (rng() % 4001) - 2000) / 16.0f;
    hay[0] = -0.0f;
    hay[1] = 0.0f;
    hay[2] = std::numeric_limits<float>::infinity();
    hay[3] = std::numeric_limits<float>::quiet_NaN();
    hay[4] = -std::numeric_limits<float>::infinity();
    for (float& f : needles) f = (float) ((int) (rng() % 4101) - 2050) / 16.0f;
    needles[0] = -0.0f;
    needles[1] = 0.0f;
    needles[2] = std::numeric_limits<float>::quiet_NaN();
    needles[3] = std::numeric_limits<float>::infinity();
    ShaderStorageBuffer hay_buffer(hay), needle_buffer(needles), lower_buffer(needle_count * 4);
    RadixSort sort;
    sort.sort_typed((float*) hay_buffer.device_ptr(), nullptr, hay_count);
    std::vector<uint32_t> keys(hay_count);
    for (size_t i = 0; i < hay_count; i++) keys[i] = float_key(hay[i]);
    std::sort(keys.begin(), keys.end());
    SortedSearch search;
    for (SearchPath path : {SearchPath_Direct, SearchPath_Indexed})
    {
        lower_buffer.clear(0xA5A5A5A5u);
        search.set_path(path);
        search.lower_bound(hay_buffer.device_ptr(), hay_count, needle_buffer.device_ptr(), needle_count, GLU_KEY_FLOAT32,
                           (uint32_t*) lower_buffer.device_ptr());
        const std::vector<uint32_t> got = lower_buffer.get_data<uint32_t>();
        bool same = true;
        for (size_t j = 0; j < needle_count; j++)
            same = same && got[j] == (uint32_t) (std::lower_bound(keys.begin(), keys.end(), float_key(needles[j])) - keys.begin());
        CHECK(same);
        CHECK(got[1] == got[0] + 1); // one -0.0 in front of +0.0
    }
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
