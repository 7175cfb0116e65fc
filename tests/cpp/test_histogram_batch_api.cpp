// C++ API test of the batched glu::Histogram: bincount_batch over equal partitions and bincount_batch_offsets over ragged segments
// (empty ones among them, every class of length) against a loop on the host, accumulate, even bins of floats and edges per segment.
#include <random>
#include <string>
#include <vector>

#include "glu/Histogram.hpp"
#include "util/mini_test.hpp"

using namespace glu;

// rows of the segments of `offsets` by bin_of(sample) (a bin, or `bins` and more: not counted)
template<typename T, typename BinOf>
static std::vector<uint32_t> rows_of(const std::vector<T>& x, const std::vector<uint32_t>& offsets, size_t bins, BinOf bin_of)
{
    std::vector<uint32_t> want((offsets.size() - 1) * bins, 0);
    for (size_t s = 0; s + 1 < offsets.size(); s++)
        for (uint32_t i = offsets[s]; i < offsets[s + 1]; i++)
        {
            const size_t b = bin_of(x[i]);
            if (b < bins) want[s * bins + b]++;
        }
    return want;
}

TEST_CASE("Histogram-batch-bincount-over-partitions-and-offsets")
{
    std::mt19937 rng(3);
    const size_t bins = 100;
    // every class of length: empty, a wave's, a workgroup's, cut into chunks
    const std::vector<uint32_t> lens = {0, 5, 2048, 0, 2049, 131072, 131073, 300000, 0, 3};
    std::vector<uint32_t> offsets(1, 0);
    for (uint32_t n : lens) offsets.push_back(offsets.back() + n);
    const size_t total = offsets.back(), segments = lens.size();
    std::vector<uint32_t> ids(total);
    for (uint32_t& x : ids) x = rng() % 130; // (ids of 100 and more are not counted)
    const auto id = [](uint32_t x) { return (size_t) x; };
    ShaderStorageBuffer in(ids), offs(offsets), out(segments * bins * 4);
    Histogram hist;
    hist.prepare_batch(total, segments, bins);
    out.clear(0xA5A5A5A5u);
    hist.bincount_batch_offsets((const uint32_t*) in.device_ptr(), total, (const uint32_t*) offs.device_ptr(), segments, bins,
                                (uint32_t*) out.device_ptr());
    const std::vector<uint32_t> want = rows_of(ids, offsets, bins, id);
    CHECK(out.get_data<uint32_t>() == want);
    CHECK(hist.last().path == GLU_HISTOGRAM_PATH_BATCH && hist.last().groups == 0 && hist.last().kernels == 5);
    const Histogram::BatchClasses classes = hist.read_batch();
    CHECK(classes.wave_segments == 3 && classes.block_segments == 2 && classes.long_segments == 2);
    hist.bincount_batch_offsets((const uint32_t*) in.device_ptr(), total, (const uint32_t*) offs.device_ptr(), segments, bins,
                                (uint32_t*) out.device_ptr(), true); // twice the counts
    std::vector<uint32_t> twice(want);
    for (uint32_t& c : twice) c *= 2;
    CHECK(out.get_data<uint32_t>() == twice);
    // equal partitions of 1000 ids: the first 37000 of the same array
    std::vector<uint32_t> rows(38);
    for (size_t p = 0; p < rows.size(); p++) rows[p] = (uint32_t) (p * 1000);
    ShaderStorageBuffer out_rows(37 * bins * 4);
    out_rows.clear(0xA5A5A5A5u);
    hist.bincount_batch((const uint32_t*) in.device_ptr(), 1000, 37, bins, (uint32_t*) out_rows.device_ptr());
    CHECK(out_rows.get_data<uint32_t>() == rows_of(ids, rows, bins, id));
    CHECK(hist.last().path == GLU_HISTOGRAM_PATH_BATCH && hist.last().kernels == 1);
    CHECK(hist.read_batch().wave_segments == 37);
    CHECK(in.get_data<uint32_t>() == ids);
    CHECK(offs.get_data<uint32_t>() == offsets);
    // more than 8192 bins are refused (the class prints and exits on an error: asked through the C ABI), and nothing is written
    glu_histogram raw = nullptr;
    CHECK(glu_histogram_create(&raw) == GLU_OK);
    const uint32_t lo = 0, hi = 8193;
    out_rows.clear(0xA5A5A5A5u);
    CHECK(glu_histogram_run_batch_even_ptr(raw, in.device_ptr(), 10, 1, GLU_KEY_UINT32, &lo, &hi, 8193, (uint32_t*) out_rows.device_ptr(), 0,
                                           nullptr) == GLU_ERROR_INVALID_ARGUMENT);
    CHECK(std::string(glu_last_error()).find("bins must be 1 .. 8192") != std::string::npos);
    CHECK(out_rows.get_data<uint32_t>() == std::vector<uint32_t>(37 * bins, 0xA5A5A5A5u));
    CHECK(glu_histogram_destroy(raw) == GLU_OK);
}

TEST_CASE("Histogram-batch-even-floats-and-edges-per-segment")
{
    std::mt19937 rng(4);
    const size_t bins = 49, count = 3000, parts = 21;
    std::vector<float> x(count * parts);
    for (float& f : x) f = (float) (rng() % 100000) / 80000.0f - 0.125f;
    std::vector<uint32_t> rows(parts + 1);
    for (size_t p = 0; p <= parts; p++) rows[p] = (uint32_t) (p * count);
    const double scale = (double) bins / (1.0 - 0.0);
    ShaderStorageBuffer in(x), offs(rows), out(parts * bins * 4);
    Histogram hist;
    out.clear(0xA5A5A5A5u);
    hist.even_batch((const float*) in.device_ptr(), count, parts, 0.0f, 1.0f, bins, (uint32_t*) out.device_ptr());
    const std::vector<uint32_t> want = rows_of(x, rows, bins, [&](float f) {
        const double d = (double) f;
        if (!(d >= 0.0 && d < 1.0)) return bins;
        const size_t b = (size_t) ((d - 0.0) * scale);
        return b < bins - 1 ? b : bins - 1;
    });
    CHECK(out.get_data<uint32_t>() == want);
    out.clear(0xA5A5A5A5u);
    hist.even_batch_offsets((const float*) in.device_ptr(), x.size(), (const uint32_t*) offs.device_ptr(), parts, 0.0f, 1.0f, bins,
                            (uint32_t*) out.device_ptr());
    CHECK(out.get_data<uint32_t>() == want);
    // edges: 0, 0.1, 0.1 (an empty bin), 0.5, 0.9
    const std::vector<float> e = {0.0f, 0.1f, 0.1f, 0.5f, 0.9f};
    ShaderStorageBuffer edges(e), out_e(parts * 4 * 4);
    const std::vector<uint32_t> want_e = rows_of(x, rows, 4, [&](float f) {
        size_t passed = 0;
        for (float edge : e) passed += edge <= f ? 1 : 0;
        return passed ? passed - 1 : (size_t) 4;
    });
    out_e.clear(0xA5A5A5A5u);
    hist.edges_batch((const float*) in.device_ptr(), count, parts, (const float*) edges.device_ptr(), 4, (uint32_t*) out_e.device_ptr());
    CHECK(out_e.get_data<uint32_t>() == want_e);
    out_e.clear(0xA5A5A5A5u);
    hist.edges_batch_offsets((const float*) in.device_ptr(), x.size(), (const uint32_t*) offs.device_ptr(), parts,
                             (const float*) edges.device_ptr(), 4, (uint32_t*) out_e.device_ptr());
    CHECK(out_e.get_data<uint32_t>() == want_e);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
