// LDS top-K candidate buffer of a 256-thread workgroup (ident.hip, ident64.hip): a header and CAP doubles that the caller places (static or
// dynamic LDS).  Values above the running K-th bound are appended; when the buffer fills, a descending bitonic sort cuts it back to K.  What
// remains after the last cut is the exact top-K multiset (ties included) of everything offered, whatever order it was offered in.  CAP is a
// power of two above K, so a cut always leaves room.
#pragma once
#include "common.h"

struct CandHdr {
  double thr;                         // a value <= thr cannot enter the top-K (K values >= thr are held)
  unsigned long long negs;            // the caller's count of negatives (kept here so the workgroup can sum it with one LDS atomic)
  int n;                              // candidates written (may run past CAP while a chunk overflows)
  int pad;
};

__device__ __forceinline__ void cand_init(CandHdr& h) {
  if (threadIdx.x == 0) {
    h.n = 0;
    h.thr = -INFINITY;
    h.negs = 0ull;
  }
}

// Sort v[0, n) descending (padded with -inf to a power of two >= 64), keep min(n, K) of it and raise thr to the K-th value.  Called by
// the whole workgroup after a barrier that follows the last write to the buffer.
template <int CAP>
__device__ void cand_cut(CandHdr& h, double* v, int K) {
  const int tid = threadIdx.x;
  const int n = min(h.n, CAP);
  int n2 = 64;
  while (n2 < n) n2 <<= 1;
  for (int i = n + tid; i < n2; i += 256) v[i] = -INFINITY;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (n2 >> 1); i += 256) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
        const double a = v[lo], b = v[hi];
        if ((lo & k) == 0 ? a < b : a > b) {
          v[lo] = b;
          v[hi] = a;
        }
      }
      __syncthreads();
    }
  if (tid == 0) {
    const int m = min(n, K);
    h.n = m;
    if (m == K) h.thr = v[K - 1];
  }
  __syncthreads();
}

// Offer this thread's values x[i] (bit i of pend set) to the buffer; every thread of the workgroup calls it (it holds barriers).  Values
// that find the buffer full stay pending across a cut.
template <int CAP, int NV>
__device__ __forceinline__ void cand_offer(CandHdr& h, double* v, const double (&x)[NV], unsigned pend, int K) {
  for (;;) {
    const double thr = h.thr;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if ((pend >> i) & 1u) {
        if (x[i] > thr) {
          const int s = atomicAdd(&h.n, 1);
          if (s < CAP) {
            v[s] = x[i];
            pend &= ~(1u << i);
          }
        } else {
          pend &= ~(1u << i);
        }
      }
    if (!__syncthreads_or(pend != 0u)) return;
    cand_cut<CAP>(h, v, K);
  }
}
