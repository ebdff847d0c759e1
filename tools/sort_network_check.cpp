// Checks the compare-exchange networks of fedfr_amd/csrc/robust_net.h (the sort inside robust_trimmed_mean_kernel) on the host with the 0-1
// principle: a network sorts every input iff it sorts every sequence of zeros and ones.  K = 1 .. 16: all 2^K sequences; K = 17 .. 32: 2^18
// pseudo-random ones.  Prints one line per K (exchange count) and exits non-zero on the first network that fails.
//   c++ -O2 -std=c++17 -I fedfr_amd/csrc tools/sort_network_check.cpp -o sort_network_check && ./sort_network_check
#include <cstdint>
#include <cstdio>
#include "robust_net.h"

template <int K>
static long check() {
  constexpr RobustNet<K> net = robust_make_net<K>();
  static_assert(net.n <= K * 8, "exchange table too small");
  const bool all = K <= 16;
  const uint64_t count = all ? (1ull << K) : (1ull << 18), mask = (1ull << K) - 1;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  long bad = 0;
  for (uint64_t t = 0; t < count; ++t) {
    uint64_t x = t;
    if (!all) {
      rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;      // xorshift64
      x = rng & mask;
    }
    uint64_t v = x;
    for (int e = 0; e < net.n; ++e) {
      const int a = net.a[e], b = net.b[e];
      if (((v >> a) & 1) > ((v >> b) & 1)) v ^= (1ull << a) | (1ull << b);
    }
    const int ones = __builtin_popcountll(x);
    const uint64_t want = ones ? (((1ull << ones) - 1) << (K - ones)) : 0;      // ascending: the ones at the top
    bad += v != want;
  }
  std::printf("K=%d exchanges=%d %s=%llu bad=%ld\n", K, net.n, all ? "exhaustive" : "random", (unsigned long long)count, bad);
  return bad;
}
template <int K>
struct All {
  static long run() { return All<K - 1>::run() + check<K>(); }
};
template <>
struct All<0> {
  static long run() { return 0; }
};
int main() { return All<32>::run() ? 1 : 0; }
