// The row-slab mapping of the streaming kernels over [M][C] 16-bit tensors (bn_rowslab.hip): one thread owns 8 consecutive channels (16-byte
// vector load/store), C/8 threads cover a row, 256/(C/8) rows per pass, a workgroup walks one slab of rows.
#pragma once
#include "common.h"

constexpr int EW_THREADS = 256;

// streaming 16-B load of data this pass is the last reader of for a long while: non-temporal, which keeps L2 / MALL for the data the next
// kernel needs (same-box A/B: 21.05 -> 20.91 ms/step)
__device__ __forceinline__ uint4 ew_ld16(const bf16_t* p) {
  typedef __attribute__((ext_vector_type(4))) unsigned u4v;
  const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}
// 8 per-channel fp32 values from c0 on (a null vector reads as dflt)
__device__ __forceinline__ void load8f(const float* p, int c0, float* v, float dflt) {
  if (p) {
    const float4 a = *reinterpret_cast<const float4*>(p + c0), b = *reinterpret_cast<const float4*>(p + c0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = dflt;
  }
}

// A thread's place in the mapping, and (set_slab) its workgroup's slab [mbeg, mend).  The block -> slab mapping goes through xcd_remap, i.e. XCD x
// streams rows [x M/8, (x+1) M/8) = the images whose conv tiles ran on XCD x (the conv kernels use the same remap), so a tensor is read from the L2
// its producer left it in and the next conv finds its input image in its own L2.  Partial rows are indexed by the logical slab id `bid`.
// Two steps: a kernel issues its per-channel loads (which need c0) between them.  With the slab arithmetic (xcd_remap's scalar divisions) in
// front of those loads, bn_apply_kernel<false, false> took 27.85 us instead of 27.42 in the step (profiles/ew_split_ab_v1.txt, first build).
struct RowSlab {
  int tpr, rpp;       // threads per row, rows per pass
  int cl, rl;         // this thread's column group and row within a pass
  int c0;             // its first channel
  bool active;        // rl < rpp (C/8 not a divisor of 256 leaves idle threads)
  int bid, mbeg, mend;
  __device__ __forceinline__ explicit RowSlab(int C) {
    tpr = C >> 3;
    rpp = EW_THREADS / tpr;
    cl = threadIdx.x % tpr;
    rl = threadIdx.x / tpr;
    active = rl < rpp;
    c0 = cl * 8;
  }
  __device__ __forceinline__ void set_slab(int M, int slab) {
    bid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    mbeg = bid * slab;
    mend = min(M, mbeg + slab);
  }
  __device__ __forceinline__ int first_row() const { return active ? mbeg + rl : mend; }      // an idle thread walks no row
};
