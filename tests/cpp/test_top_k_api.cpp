// C++ API test of glu::TopK: the k smallest (sorted) and the k largest (unsorted) of uint32 keys with duplicates and of floats with
// both zeros, against std::stable_sort of (code, index); the k-th key alone; the plan and what the device reports of the last call.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "glu/TopK.hpp"
#include "util/mini_test.hpp"

using namespace glu;

namespace
{
constexpr uint32_t kPoison = 0xA5A5A5A5u;

// the sort's code of a float's bits: negative values flip every bit, the others the sign bit
uint32_t float_code(uint32_t bits) { return bits & 0x80000000u ? ~bits : bits ^ 0x80000000u; }

// the first k indices of the stable sort by code (complemented for largest)
std::vector<uint32_t> head(const std::vector<uint32_t>& code, size_t k, bool largest)
{
    std::vector<uint32_t> order(code.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return largest ? code[a] > code[b] : code[a] < code[b]; });
    order.resize(k);
    return order;
}
} // namespace

TEST_CASE("TopK-smallest-sorted-and-largest-unsorted-of-uint32-keys-with-duplicates")
{
    std::mt19937 rng(1);
    const size_t n = 100003, k = 1000;
    std::vector<uint32_t> keys(n);
    for (uint32_t& v : keys) v = (rng() % 40000u) * 7919u;
    ShaderStorageBuffer kb(keys), ok((k + 8) * 4), oi((k + 8) * 4), kth(4);
    TopK topk;
    topk.prepare(n, k);
    const TopK::Plan plan = TopK::plan(n, k);
    CHECK(plan.rounds == 3 && plan.tile == 4096 && plan.tiles == (n + 4095) / 4096 && plan.capacity == 65536);

    std::vector<uint32_t> want = head(keys, k, false);
    ok.clear(kPoison);
    oi.clear(kPoison);
    topk.smallest(kb.device_ptr(), n, k, ok.device_ptr(), (uint32_t*) oi.device_ptr(), GLU_KEY_UINT32, true, kth.device_ptr());
    std::vector<uint32_t> got_i = oi.get_data<uint32_t>(), got_k = ok.get_data<uint32_t>();
    for (size_t r = 0; r < k; r++) CHECK(got_i[r] == want[r] && got_k[r] == keys[want[r]]);
    for (size_t r = k; r < k + 8; r++) CHECK(got_i[r] == kPoison && got_k[r] == kPoison);
    CHECK(kth.get_data<uint32_t>()[0] == keys[want[k - 1]]);
    const TopK::Last last = topk.read_last();
    CHECK(last.path == GLU_TOP_K_PATH_CANDIDATES && last.kernels == plan.kernels && last.ties >= 1);

    want = head(keys, k, true);
    std::sort(want.begin(), want.end());
    ok.clear(kPoison);
    oi.clear(kPoison);
    topk.largest(kb, n, k, ok, oi, false);
    got_i = oi.get_data<uint32_t>(), got_k = ok.get_data<uint32_t>();
    for (size_t r = 0; r < k; r++) CHECK(got_i[r] == want[r] && got_k[r] == keys[want[r]]);
    for (size_t r = k; r < k + 8; r++) CHECK(got_i[r] == kPoison && got_k[r] == kPoison);
    CHECK(kb.get_data<uint32_t>() == keys);
}

TEST_CASE("TopK-floats-in-the-sorts-order-and-the-kth-key-alone")
{
    std::mt19937 rng(2);
    const size_t n = 20001, k = 300;
    std::vector<float> keys(n);
    for (float& v : keys) v = (float) ((int) (rng() % 2001u) - 1000) * 0.5f;
    for (size_t i = 0; i < n; i += 97) keys[i] = i % 2 ? -0.0f : 0.0f;
    std::vector<uint32_t> code(n);
    for (size_t i = 0; i < n; i++)
    {
        uint32_t bits;
        std::memcpy(&bits, &keys[i], 4);
        code[i] = float_code(bits);
    }
    ShaderStorageBuffer kb(keys), ok(k * 4), oi(k * 4), kth(4);
    TopK topk;
    for (bool largest : {false, true})
    {
        const std::vector<uint32_t> want = head(code, k, largest);
        if (largest) topk.largest(kb.device_ptr(), n, k, ok.device_ptr(), (uint32_t*) oi.device_ptr(), GLU_KEY_FLOAT32);
        else topk.smallest(kb.device_ptr(), n, k, ok.device_ptr(), (uint32_t*) oi.device_ptr(), GLU_KEY_FLOAT32);
        CHECK(oi.get_data<uint32_t>() == want);
        const std::vector<float> got = ok.get_data<float>();
        for (size_t r = 0; r < k; r++) CHECK(std::memcmp(&got[r], &keys[want[r]], 4) == 0);
        kth.clear(kPoison);
        topk.kth(kb.device_ptr(), n, k, kth.device_ptr(), GLU_KEY_FLOAT32, largest);
        const float t = kth.get_data<float>()[0];
        CHECK(std::memcmp(&t, &keys[want[k - 1]], 4) == 0);
        CHECK(topk.read_last().kernels == TopK::plan(n, k, GLU_KEY_FLOAT32, false, false).kernels);
    }
}

int main(int argc, char** argv) { return mini_test::run(argc, argv); }
