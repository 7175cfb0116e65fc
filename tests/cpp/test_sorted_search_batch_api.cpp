// C++ API test of glu::SortedSearch's batched calls: equal partitions whose rows hold the same key range (a probe that leaks into
// a neighbouring row changes the answer), at the default window and with the window off; ragged segments from device offsets on both
// sides, with empty haystacks, segments without needles and uncovered needles in front and behind; equal needle rows over ragged
// haystacks -- checked against std::lower_bound and std::upper_bound per segment on the host.
#include <algorithm>
#include <random>
#include <vector>

#include "glu/SortedSearch.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
constexpr uint32_t kPoison = 0xA5A5A5A5u;

// the bounds of needles[nb, ne) in hay[hb, he), local to the segment
void expect(const std::vector<uint32_t>& hay, size_t hb, size_t he, const std::vector<uint32_t>& needles, size_t nb, size_t ne,
            std::vector<uint32_t>& lower, std::vector<uint32_t>& upper)
{
    for (size_t j = nb; j < ne; j++)
    {
        lower[j] = (uint32_t) (std::lower_bound(hay.begin() + hb, hay.begin() + he, needles[j]) - (hay.begin() + hb));
        upper[j] = (uint32_t) (std::upper_bound(hay.begin() + hb, hay.begin() + he, needles[j]) - (hay.begin() + hb));
    }
}
} // namespace

TEST_CASE("SortedSearch-batch-equal-partitions-with-and-without-the-window")
{
    std::mt19937 rng(5);
    const size_t rows = 37, hay_count = 128, needle_count = 100;
    std::vector<uint32_t> hay(rows * hay_count), needles(rows * needle_count);
    for (uint32_t& k : hay) k = rng() % 300;
    for (size_t p = 0; p < rows; p++) std::sort(hay.begin() + p * hay_count, hay.begin() + (p + 1) * hay_count);
    for (uint32_t& k : needles) k = rng() % 302;
    std::vector<uint32_t> want_lower(needles.size()), want_upper(needles.size());
    for (size_t p = 0; p < rows; p++)
        expect(hay, p * hay_count, (p + 1) * hay_count, needles, p * needle_count, (p + 1) * needle_count, want_lower, want_upper);
    ShaderStorageBuffer hay_buffer(hay), needle_buffer(needles), lower_buffer(needles.size() * 4), upper_buffer(needles.size() * 4);
    uint32_t* lower = (uint32_t*) lower_buffer.device_ptr();
    uint32_t* upper = (uint32_t*) upper_buffer.device_ptr();
    const SortedSearch::BatchPlan plan = SortedSearch::plan_batch(needles.size());
    CHECK(plan.tile == 2048 && plan.tiles == 2 && plan.window_keys == 8192 && plan.kernels == 1);
    CHECK(SortedSearch::plan_batch(needles.size(), GLU_KEY_UINT64).window_keys == 4096);
    CHECK(SortedSearch::plan_batch(0).kernels == 0);
    SortedSearch search; // (no prepare: the batched calls keep no scratch)
    for (uint32_t window : {GLU_SEARCH_BATCH_WINDOW_DEFAULT, 0u, 256u})
    {
        lower_buffer.clear(kPoison);
        upper_buffer.clear(kPoison);
        search.set_batch_window(window);
        search.search_batch(hay_buffer.device_ptr(), hay_count, needle_buffer.device_ptr(), needle_count, rows, GLU_KEY_UINT32, lower, upper);
        CHECK(lower_buffer.get_data<uint32_t>() == want_lower);
        CHECK(upper_buffer.get_data<uint32_t>() == want_upper);
        const SortedSearch::Last last = search.last();
        CHECK(last.path == SearchPath_Batch && last.levels == 0 && last.kernels == 1);
    }
    lower_buffer.clear(kPoison);
    upper_buffer.clear(kPoison);
    search.lower_bound_batch(hay_buffer.device_ptr(), hay_count, needle_buffer.device_ptr(), needle_count, rows, GLU_KEY_UINT32, lower);
    search.upper_bound_batch(hay_buffer.device_ptr(), hay_count, needle_buffer.device_ptr(), needle_count, rows, GLU_KEY_UINT32, upper);
    CHECK(lower_buffer.get_data<uint32_t>() == want_lower);
    CHECK(upper_buffer.get_data<uint32_t>() == want_upper);
    search.search_batch(nullptr, hay_count, nullptr, needle_count, 0, GLU_KEY_UINT32, nullptr, nullptr); // no rows: nothing is looked at
    CHECK(search.last().kernels == 0 && search.last().path == SearchPath_Batch);
    CHECK(hay_buffer.get_data<uint32_t>() == hay);
    CHECK(needle_buffer.get_data<uint32_t>() == needles);
}

TEST_CASE("SortedSearch-batch-ragged-segments-from-device-offsets")
{
    std::mt19937 rng(6);
    const size_t segments = 200;
    const uint32_t lengths[] = {0, 1, 2, 63, 64, 65, 700};
    std::vector<uint32_t> hay_offsets(segments + 1, 0), needle_offsets(segments + 1, 0);
    needle_offsets[0] = 3; // three needles in front belong to no segment
    for (size_t s = 0; s < segments; s++)
    {
        hay_offsets[s + 1] = hay_offsets[s] + lengths[rng() % 7];
        needle_offsets[s + 1] = needle_offsets[s] + (s >= 50 && s < 120 ? 0u : lengths[rng() % 7]);
    }
    const size_t hay_total = hay_offsets[segments], needle_total = needle_offsets[segments] + 5; // and five behind
    std::vector<uint32_t> hay(hay_total), needles(needle_total);
    for (uint32_t& k : hay) k = rng() % 90;
    for (size_t s = 0; s < segments; s++) std::sort(hay.begin() + hay_offsets[s], hay.begin() + hay_offsets[s + 1]);
    for (uint32_t& k : needles) k = rng() % 92;
    std::vector<uint32_t> want_lower(needle_total, kPoison), want_upper(needle_total, kPoison);
    for (size_t s = 0; s < segments; s++)
        expect(hay, hay_offsets[s], hay_offsets[s + 1], needles, needle_offsets[s], needle_offsets[s + 1], want_lower, want_upper);
    ShaderStorageBuffer hay_buffer(hay), needle_buffer(needles), ho_buffer(hay_offsets), no_buffer(needle_offsets);
    ShaderStorageBuffer lower_buffer(needle_total * 4), upper_buffer(needle_total * 4);
    SortedSearch search;
    for (uint32_t window : {GLU_SEARCH_BATCH_WINDOW_DEFAULT, 0u, 64u})
    {
        lower_buffer.clear(kPoison);
        upper_buffer.clear(kPoison);
        search.set_batch_window(window);
        search.search_batch_offsets(hay_buffer.device_ptr(), hay_total, (const uint32_t*) ho_buffer.device_ptr(), needle_buffer.device_ptr(),
                                    needle_total, (const uint32_t*) no_buffer.device_ptr(), segments, GLU_KEY_UINT32,
                                    (uint32_t*) lower_buffer.device_ptr(), (uint32_t*) upper_buffer.device_ptr());
        CHECK(lower_buffer.get_data<uint32_t>() == want_lower);
        CHECK(upper_buffer.get_data<uint32_t>() == want_upper);
        CHECK(search.last().path == SearchPath_Batch && search.last().kernels == 1);
    }
    // equal needle rows over the ragged haystacks: 7 samples per segment
    const size_t row = 7;
    std::vector<uint32_t> samples(segments * row);
    for (uint32_t& k : samples) k = rng() % 92;
    std::vector<uint32_t> row_lower(samples.size()), row_upper(samples.size());
    for (size_t s = 0; s < segments; s++) expect(hay, hay_offsets[s], hay_offsets[s + 1], samples, s * row, (s + 1) * row, row_lower, row_upper);
    ShaderStorageBuffer sample_buffer(samples), row_upper_buffer(samples.size() * 4);
    row_upper_buffer.clear(kPoison);
    search.set_batch_window(GLU_SEARCH_BATCH_WINDOW_DEFAULT);
    search.search_batch_offsets(hay_buffer.device_ptr(), hay_total, (const uint32_t*) ho_buffer.device_ptr(), sample_buffer.device_ptr(),
                                samples.size(), nullptr, segments, GLU_KEY_UINT32, nullptr, (uint32_t*) row_upper_buffer.device_ptr());
    CHECK(row_upper_buffer.get_data<uint32_t>() == row_upper);
    // (the class ends the program on a refusal, so the refusal is asked of the C ABI: the needle count does not divide)
    glu_sorted_search raw = nullptr;
    CHECK(glu_sorted_search_create(&raw) == GLU_OK);
    CHECK(glu_sorted_search_run_batch_offsets_ptr(raw, hay_buffer.device_ptr(), hay_total, (const uint32_t*) ho_buffer.device_ptr(),
                                                  sample_buffer.device_ptr(), samples.size() - 1, nullptr, segments, GLU_KEY_UINT32, nullptr,
                                                  (uint32_t*) row_upper_buffer.device_ptr(), nullptr) == GLU_ERROR_INVALID_ARGUMENT);
    CHECK(glu_sorted_search_destroy(raw) == GLU_OK);
    CHECK(row_upper_buffer.get_data<uint32_t>() == row_upper); // a refused call writes nothing
    CHECK(hay_buffer.get_data<uint32_t>() == hay);
    CHECK(ho_buffer.get_data<uint32_t>() == hay_offsets);
    CHECK(no_buffer.get_data<uint32_t>() == needle_offsets);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
