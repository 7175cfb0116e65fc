// test_bucket_order.cpp -- the ordering step of the in-LDS pass (gl-radix-sort_amd/csrc/bucket_order.hpp) on the host: a stand-alone
// program, no library and no GPU.
//   g++ -std=c++17 -O1 -g -I gl-radix-sort_amd/csrc -o test_bucket_order tests/cpp/test_bucket_order.cpp
//   (tests/test_bucket_order.py builds and runs it plain and with -fsanitize=address,undefined)
// What it checks, for 4-byte and 8-byte words:
//   * the networks: for every length 2 .. 8 every 0-1 input (the 0-1 principle: a network of exchanges that orders every input of
//     zeros and ones orders every input), and every permutation of distinct words for lengths 2 .. 4 and 8;
//   * the insertion: lengths 9 .. 24 on seeded random words;
//   * that no step writes outside its bucket (guard words before and behind it keep their values);
//   * the mask walk over one thread's buckets: tables with no bucket of two words or more, one, every bucket, only the last -- and
//     mixed ones --, the stage compared with std::sort per bucket.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "bucket_order.hpp"

using namespace glu_hip;

static long failures = 0, checks = 0;
#define EXPECT(cond, ...)                                                                                                                \
    do                                                                                                                                   \
    {                                                                                                                                    \
        checks++;                                                                                                                        \
        if (!(cond))                                                                                                                     \
        {                                                                                                                                \
            if (failures++ < 20) printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond), printf(__VA_ARGS__), printf("\n");             \
        }                                                                                                                                \
    } while (0)

// the step for a bucket of m words, as the walk chooses it
template<typename WordT>
static void order_bucket(WordT* p, uint32_t m)
{
    if (m <= 4u)
        bucket_order4(p, m);
    else if (m <= 8u)
        bucket_order8(p, m);
    else
        bucket_order_insertion(p, m);
}

// `in` (m words) between guards: eight words in front, eight behind, which are words of neighbouring buckets in the kernel -- the
// step may read them, and must leave them as they are.  fn(p, m) orders it.
template<typename WordT, typename Fn>
static void check_one(const std::vector<WordT>& in, Fn fn, const char* what)
{
    const uint32_t m = (uint32_t) in.size();
    std::vector<WordT> stage(m + 16);
    for (uint32_t i = 0; i < 8; i++) stage[i] = (WordT) (1000 + i), stage[8 + m + i] = (WordT) (2000 + i); // (smaller and larger than the words: no accident hides a use)
    std::copy(in.begin(), in.end(), stage.begin() + 8);
    fn(stage.data() + 8, m);
    std::vector<WordT> want(in);
    std::sort(want.begin(), want.end());
    bool same = std::equal(want.begin(), want.end(), stage.begin() + 8), guards = true;
    for (uint32_t i = 0; i < 8; i++) guards = guards && stage[i] == (WordT) (1000 + i) && stage[8 + m + i] == (WordT) (2000 + i);
    EXPECT(same, "%s, %u words", what, m);
    EXPECT(guards, "%s, %u words: a word outside the bucket was written", what, m);
}

template<typename WordT>
static void networks()
{
    auto net = [](WordT* p, uint32_t m) { order_bucket(p, m); };
    // a bucket of five words or more first meets the 4-word network on its first four words (the walk's first loop), then its own
    auto as_walked = [](WordT* p, uint32_t m) {
        bucket_order4(p, m < 4u ? m : 4u);
        if (m > 4u) order_bucket(p, m);
    };
    for (uint32_t m = 2; m <= 8; m++)
    {
        // every 0-1 input.  (The kernel's words are unique; equal words still have to come out ordered for the principle to apply.)
        for (uint32_t bits = 0; bits < (1u << m); bits++)
        {
            std::vector<WordT> in(m);
            for (uint32_t i = 0; i < m; i++) in[i] = (WordT) ((bits >> i) & 1u);
            check_one(in, net, "0-1 input");
            check_one(in, as_walked, "0-1 input as walked");
        }
        if (m > 4 && m < 8) continue;
        // every permutation of distinct words: large ones, in the top bits of the word type too
        std::vector<uint32_t> perm(m);
        std::iota(perm.begin(), perm.end(), 0u);
        do
        {
            std::vector<WordT> in(m);
            for (uint32_t i = 0; i < m; i++) in[i] = (WordT) (((WordT) (perm[i] + 1u) << (8 * sizeof(WordT) - 5)) | (WordT) (7u - perm[i]));
            check_one(in, net, "permutation");
            if (m == 8) check_one(in, as_walked, "permutation as walked");
        } while (std::next_permutation(perm.begin(), perm.end()));
    }
}

template<typename WordT>
static void insertion(uint32_t seed)
{
    std::mt19937_64 rng(seed);
    for (uint32_t m = 9; m <= kBucketMaxLen; m++)
        for (int rep = 0; rep < 200; rep++)
        {
            std::vector<WordT> in(m);
            for (uint32_t i = 0; i < m; i++) in[i] = (WordT) ((rng() << 6) | i) & (WordT) ~((WordT) 1 << (8 * sizeof(WordT) - 1)); // unique, below the pad
            if (rep == 0) std::sort(in.begin(), in.end());
            if (rep == 1) std::sort(in.begin(), in.end()), std::reverse(in.begin(), in.end());
            check_one(in, [](WordT* p, uint32_t n) { bucket_order_insertion(p, n); }, "insertion");
            check_one(in, [](WordT* p, uint32_t n) { bucket_order4(p, 4u), order_bucket(p, n); }, "insertion as walked");
        }
}

// One workgroup's table as the kernel lays it out: THREADS threads, thread t owns buckets j * THREADS + t; `lengths` per bucket;
// the buckets lie one behind the other in the stage from position f4 on, and the stage has the kernel's room behind them.
template<int BPT, typename WordT>
static void walk_table(const std::vector<uint32_t>& lengths, uint32_t threads, uint32_t f4, std::mt19937_64& rng, const char* what)
{
    const uint32_t nb = (uint32_t) lengths.size();
    std::vector<uint32_t> table(nb);
    uint32_t total = f4;
    for (uint32_t b = 0; b < nb; b++) table[b] = total | (lengths[b] << 16), total += lengths[b];
    const WordT GUARD = (WordT) 0x5A5A5A5A;
    std::vector<WordT> stage(total + 12, GUARD), want;
    // unique words, ascending from bucket to bucket, shuffled inside each bucket
    WordT next = 1;
    for (uint32_t b = 0; b < nb; b++)
    {
        WordT* p = stage.data() + (table[b] & 0xFFFFu);
        for (uint32_t i = 0; i < lengths[b]; i++) p[i] = next, next += (WordT) (1 + rng() % 1000);
        std::shuffle(p, p + lengths[b], rng);
    }
    want = stage;
    for (uint32_t b = 0; b < nb; b++) std::sort(want.begin() + (table[b] & 0xFFFFu), want.begin() + (table[b] & 0xFFFFu) + lengths[b]);
    long reads = 0;
    for (uint32_t t = 0; t < threads; t++)
        bucket_order_walk<BPT>(stage.data(), [&](int j) {
            reads++;
            EXPECT(j >= 0 && j < BPT, "%s: entry %d asked for", what, j);
            return table[(uint32_t) (j < 0 || j >= BPT ? 0 : j) * threads + t];
        });
    EXPECT(stage == want, "%s (BPT %d, %u threads, f4 %u)", what, BPT, threads, f4);
    (void) reads;
}

template<int BPT, typename WordT>
static void walks(uint32_t seed)
{
    std::mt19937_64 rng(seed);
    const uint32_t threads = 8, nb = BPT * threads;
    for (uint32_t f4 = 0; f4 < 4; f4++)
    {
        walk_table<BPT, WordT>(std::vector<uint32_t>(nb, 0u), threads, f4, rng, "no bucket at all");
        walk_table<BPT, WordT>(std::vector<uint32_t>(nb, 1u), threads, f4, rng, "no bucket of two or more");
        for (uint32_t m : {2u, 3u, 4u, 5u, 8u, 9u, kBucketMaxLen})
        {
            walk_table<BPT, WordT>(std::vector<uint32_t>(nb, m), threads, f4, rng, "every bucket");
            for (uint32_t rest : {0u, 1u})
            {
                std::vector<uint32_t> one(nb, rest), last(nb, rest), first(nb, rest), lane(nb, rest);
                one[nb / 2 + 3] = m;                                       // one bucket, of one thread
                for (uint32_t t = 0; t < threads; t++) last[(BPT - 1) * threads + t] = m, first[t] = m; // only the last / first of every thread
                for (uint32_t j = 0; j < (uint32_t) BPT; j++) lane[j * threads + 5] = m; // one thread's full worklist beside empty ones
                last[nb - 1] = m; // (the very last bucket: what it reads behind itself is the stage's spare room)
                walk_table<BPT, WordT>(one, threads, f4, rng, "one bucket");
                walk_table<BPT, WordT>(last, threads, f4, rng, "only the last bucket of a thread");
                walk_table<BPT, WordT>(first, threads, f4, rng, "only the first bucket of a thread");
                walk_table<BPT, WordT>(lane, threads, f4, rng, "one thread's buckets");
            }
        }
        // mixed lengths: Poisson-like (what uniformly drawn keys give), and fuller ones
        for (int rep = 0; rep < 50; rep++)
        {
            std::vector<uint32_t> mixed(nb);
            std::poisson_distribution<uint32_t> d(rep < 25 ? 1.0 : 3.5);
            for (auto& m : mixed) m = std::min<uint32_t>(d(rng), kBucketMaxLen);
            if (rep % 5 == 0) mixed[rng() % nb] = kBucketMaxLen, mixed[rng() % nb] = 9;
            walk_table<BPT, WordT>(mixed, threads, f4, rng, "mixed lengths");
        }
    }
}

int main()
{
    networks<uint32_t>();
    networks<uint64_t>();
    insertion<uint32_t>(1);
    insertion<uint64_t>(2);
    walks<16, uint32_t>(3); // BPT of the 256 x 18 tile
    walks<4, uint32_t>(4);  // 256 x 6
    walks<8, uint64_t>(5);  // 64-bit keys, 512 x 9
    walks<32, uint32_t>(6); // (every bit of the mask)
    walks<1, uint64_t>(7);
    printf("bucket_order: %ld checks, %ld failed\n", checks, failures);
    return failures ? 1 : 0;
}
