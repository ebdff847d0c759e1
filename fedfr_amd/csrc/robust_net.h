// The compare-exchange networks of robust_trimmed_mean_kernel (robust.hip), as a compile-time table.  Plain C++ (no HIP), so that
// tools/sort_network_check.cpp can include it and check every network on the host with the 0-1 principle.
#pragma once

template <int K>
struct RobustNet {
  int n;
  unsigned char a[K * 8], b[K * 8];      // (K = 32: 191 exchanges)
};
// Batcher's merge exchange (Knuth 5.2.2 M) for arbitrary K
template <int K>
constexpr RobustNet<K> robust_make_net() {
  RobustNet<K> r{};
  for (int p = 1; p < K; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j <= K - 1 - k; j += 2 * k)
        for (int i = 0; i <= (k - 1 < K - j - k - 1 ? k - 1 : K - j - k - 1); ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            r.a[r.n] = (unsigned char)(i + j);
            r.b[r.n] = (unsigned char)(i + j + k);
            ++r.n;
          }
  return r;
}
