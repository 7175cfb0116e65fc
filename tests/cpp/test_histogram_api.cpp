// C++ API test of glu::Histogram: bincount and even bins of uint32 ids against a loop on the host, accumulate, even bins of floats
// with both zeros, an infinity and a NaN, and equi-depth bins: glu::RadixSort sorts a copy of the samples, every k-th key becomes an
// edge of a device array, and every bin must hold its k samples.
#include <cmath>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "glu/Histogram.hpp"
#include "glu/RadixSort.hpp"
#include "util/mini_test.hpp"

using namespace glu;

TEST_CASE("Histogram-bincount-even-and-accumulate-against-the-host")
{
    std::mt19937 rng(1);
    const size_t count = 100003, bins = 100;
    std::vector<uint32_t> ids(count);
    for (uint32_t& x : ids) x = rng() % 130; // (ids of 100 and more are not counted)
    std::vector<uint32_t> want(bins, 0), want_wide(10, 0);
    for (uint32_t x : ids)
    {
        if (x < bins) want[x]++;
        if (x >= 20 && x < 120) want_wide[(x - 20) / 10]++;
    }
    ShaderStorageBuffer in(ids), out(bins * 4), out_wide(10 * 4);
    const Histogram::Plan plan = Histogram::plan(count, bins);
    CHECK(plan.path == GLU_HISTOGRAM_PATH_LDS);
    CHECK(plan.threads == 256 && plan.tile == 4096);
    CHECK(plan.groups == (count + plan.tile - 1) / plan.tile);
    CHECK(plan.kernels == 2);
    CHECK(plan.scratch_bytes == (size_t) plan.groups * bins * 4);
    CHECK(Histogram::plan(count, 8193).path == GLU_HISTOGRAM_PATH_GLOBAL);
    CHECK(Histogram::plan(count, 8192, GLU_KEY_FLOAT64, GLU_HISTOGRAM_EDGES).threads == 1024);
    Histogram hist;
    hist.prepare(count, bins);
    out.clear(0xA5A5A5A5u);
    hist.bincount(in, count, bins, out);
    CHECK(out.get_data<uint32_t>() == want);
    CHECK(hist.last().path == plan.path && hist.last().groups == plan.groups && hist.last().kernels == 2);
    hist.bincount(in, count, bins, out, true); // twice the counts
    std::vector<uint32_t> twice(want);
    for (uint32_t& c : twice) c *= 2;
    CHECK(out.get_data<uint32_t>() == twice);
    out_wide.clear(0xA5A5A5A5u);
    hist.even((const uint32_t*) in.device_ptr(), count, 20u, 120u, 10, (uint32_t*) out_wide.device_ptr());
    CHECK(out_wide.get_data<uint32_t>() == want_wide);
    hist.bincount(in, 0, bins, out); // nothing to count: zeros
    CHECK(out.get_data<uint32_t>() == std::vector<uint32_t>(bins, 0));
    CHECK(hist.last().groups == 0 && hist.last().kernels == 1);
    CHECK(in.get_data<uint32_t>() == ids);
    // W = 10 / 3 is refused (the class prints and exits on an error: asked through the C ABI), and nothing is written
    glu_histogram raw = nullptr;
    CHECK(glu_histogram_create(&raw) == GLU_OK);
    const uint32_t lo = 0, hi = 10;
    out_wide.clear(0xA5A5A5A5u);
    CHECK(glu_histogram_run_even_ptr(raw, in.device_ptr(), count, GLU_KEY_UINT32, &lo, &hi, 3, (uint32_t*) out_wide.device_ptr(), 0, nullptr) ==
          GLU_ERROR_INVALID_ARGUMENT);
    CHECK(std::string(glu_last_error()).find("glu_histogram_run_edges_ptr") != std::string::npos);
    CHECK(out_wide.get_data<uint32_t>() == std::vector<uint32_t>(10, 0xA5A5A5A5u));
    CHECK(glu_histogram_destroy(raw) == GLU_OK);
}

TEST_CASE("Histogram-even-bins-of-floats-drop-NaN-and-infinities")
{
    std::mt19937 rng(2);
    const size_t count = 50000, bins = 49;
    std::vector<float> x(count);
    for (float& f : x) f = (float) (rng() % 100000) / 80000.0f - 0.125f;
    x[0] = -0.0f;
    x[1] = 0.0f;
    x[2] = std::numeric_limits<float>::infinity();
    x[3] = std::numeric_limits<float>::quiet_NaN();
    x[4] = std::nextafter(1.0f, 0.0f);
    x[5] = 1.0f;
    const double scale = (double) bins / (1.0 - 0.0);
    std::vector<uint32_t> want(bins, 0);
    for (float f : x)
    {
        const double d = (double) f;
        if (!(d >= 0.0 && d < 1.0)) continue;
        const uint32_t b = (uint32_t) ((d - 0.0) * scale);
        want[b < bins - 1 ? b : bins - 1]++;
    }
    ShaderStorageBuffer in(x), out(bins * 4);
    out.clear(0xA5A5A5A5u);
    Histogram hist;
    hist.even((const float*) in.device_ptr(), count, 0.0f, 1.0f, bins, (uint32_t*) out.device_ptr());
    CHECK(out.get_data<uint32_t>() == want);
}

TEST_CASE("Histogram-equi-depth-bins-from-device-edges")
{
    const size_t bins = 64, depth = 1000, count = bins * depth;
    std::vector<uint32_t> x(count), iota(count);
    for (size_t i = 0; i < count; i++) x[i] = (uint32_t) i * 2654435761u, iota[i] = (uint32_t) i; // (a bijection: all different)
    ShaderStorageBuffer samples(x), sorted(x), vals(iota), edges((bins + 1) * 4), out(bins * 4);
    RadixSort sort;
    sort((uint32_t*) sorted.device_ptr(), (uint32_t*) vals.device_ptr(), count, 0, nullptr);
    // every depth-th key of the sorted copy is an edge; the last edge is the largest key: that one sample is nobody's
    const std::vector<uint32_t> s = sorted.get_data<uint32_t>();
    std::vector<uint32_t> e(bins + 1);
    for (size_t b = 0; b < bins; b++) e[b] = s[b * depth];
    e[bins] = s[count - 1];
    edges.write_data(e.data(), e.size() * 4);
    Histogram hist;
    out.clear(0xA5A5A5A5u);
    hist.edges((const uint32_t*) samples.device_ptr(), count, (const uint32_t*) edges.device_ptr(), bins, (uint32_t*) out.device_ptr());
    std::vector<uint32_t> want(bins, (uint32_t) depth);
    want[bins - 1] = (uint32_t) depth - 1;
    CHECK(out.get_data<uint32_t>() == want);
    CHECK(hist.last().path == GLU_HISTOGRAM_PATH_LDS && hist.last().kernels == 2);
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
