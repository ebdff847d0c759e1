// Narrow secure aggregation on the flat parameter buffer: a client uploads 8- or 16-bit codes of its ROTATED update, packed 4 or 2 to a
// 32-bit word, under the pairwise and self masks of secagg.h; everything between the encoder and the decoder is arithmetic in Z / 2^b on
// the fields of those words.  The format is stated in include/fedfr_hip.h ("NARROW WORDS") and restated in numpy in
// tests/secagg_narrow_cases.py; the kernels are held to that restatement bit for bit:
//   rht_fill_kernel                         dst = 2^-6 H (D src), or D (2^-6 H src): the rotation alone
//   secagg_mask_narrow_kernel<BITS>         y = pack(encode(2^-6 H D (xi - x))) (+) the k streams, one pass: x and xi read once, y written once
//   secagg_aggregate_narrow_kernel<BITS,KU> S = (first ? 0 : acc) (+) KU uploads (+) the k streams; last ? out = (x +) rescale D 2^-6 H (S 2^-f) : acc = S
// ONE WORKGROUP, ONE ROTATION BLOCK.  256 lanes hold the 4096 elements of a block, 16 each, and the 12 butterfly levels run as three
// phases of four levels in registers: lane t holds elements 16 t + j (levels 1 .. 8), then (t / 16) 256 + 16 j + t % 16 (levels 16 .. 128),
// then 256 j + t (levels 256 .. 2048), with one pass through LDS between two phases.  A lane always writes the LDS words it read last, so
// one barrier per exchange is enough.  The level ORDER is that of the format, so the bits do not depend on this decomposition.
// THE GENERATOR.  A rotation block is 1024 (b = 8) or 2048 (b = 16) packed words: 64 or 128 ChaCha20 blocks per stream, fewer than the
// lanes.  The 256 lanes split into 4 or 2 PARTS; part p generates streams p, p + PARTS, ... for every ChaCha20 block of the rotation block
// and sums them field-wise in registers; the parts meet in LDS, where every lane adds the partial sums of its own 4 or 8 words.  With
// PARTS or more streams no lane idles in the generator.
// LDS: the rotation buffer (4096 floats, padded to 5376: rht_idx), the partial mask sums (4096 words) and the 128 sign words: 38.5 KB.
#include "secagg_narrow.h"
#include "multi_state.h"
#include <cmath>

// ---- the rotation, written once ---------------------------------------------------------------------------------------------------------
// element e of the block lives at word rht_idx(e): 4 words of padding behind every 16 elements and 16 more behind every 256, so that the
// 16-byte accesses of 16 neighbouring lanes (64 B apart) and the 4-byte accesses of the middle phase (lanes 256 elements apart) spread over
// the banks.  Every multiple of 4 stays a multiple of 4: ds_read_b128 / ds_write_b128 stay aligned.
constexpr int RHT_LDS_WORDS = RHT_BLOCK + 4 * (RHT_BLOCK / 16) + 16 * (RHT_BLOCK / 256);      // 5376
__device__ __forceinline__ int rht_idx(int e) { return e + 4 * (e >> 4) + 16 * (e >> 8); }
__device__ __forceinline__ int rht_elem_b(int t, int j) { return ((t >> 4) << 8) | (j << 4) | (t & 15); }      // the middle phase
__device__ __forceinline__ int rht_elem_c(int t, int j) { return (j << 8) | t; }                                // the last phase

typedef float f4 __attribute__((ext_vector_type(4)));
// lane t's elements 16 t + j, as four 16-byte accesses
__device__ __forceinline__ void rht_store_a(float* rot, const float (&v)[RHT_EPT], int t) {
#pragma unroll
  for (int h = 0; h < 4; ++h) *reinterpret_cast<f4*>(rot + rht_idx(16 * t + 4 * h)) = f4{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
}
__device__ __forceinline__ void rht_load_a(const float* rot, float (&v)[RHT_EPT], int t) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const f4 q = *reinterpret_cast<const f4*>(rot + rht_idx(16 * t + 4 * h));
    v[4 * h] = q.x; v[4 * h + 1] = q.y; v[4 * h + 2] = q.z; v[4 * h + 3] = q.w;
  }
}
// four levels on the register index: (a, b) -> (a + b, a - b), one fp32 operation each
__device__ __forceinline__ void rht_levels4(float (&v)[RHT_EPT]) {
#pragma unroll
  for (int m = 1; m < RHT_EPT; m <<= 1) {
#pragma unroll
    for (int j = 0; j < RHT_EPT; ++j) {
      if (j & m) continue;
      const float a = v[j], b = v[j | m];
      v[j] = __fadd_rn(a, b);
      v[j | m] = __fsub_rn(a, b);
    }
  }
}
// v: elements 16 t + j of the block on entry, elements 256 j + t of 2^-6 H (the block) on return.  The caller's last access to `rot` by
// any lane lies behind a barrier, or is this lane's own access to the words of elements 16 t + j.
__device__ __forceinline__ void rht_rotate(float* rot, float (&v)[RHT_EPT], int t) {
  rht_levels4(v);                                   // h = 1, 2, 4, 8
  rht_store_a(rot, v, t);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RHT_EPT; ++j) v[j] = rot[rht_idx(rht_elem_b(t, j))];
  rht_levels4(v);                                   // h = 16 .. 128
#pragma unroll
  for (int j = 0; j < RHT_EPT; ++j) rot[rht_idx(rht_elem_b(t, j))] = v[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RHT_EPT; ++j) v[j] = rot[rht_idx(rht_elem_c(t, j))];
  rht_levels4(v);                                   // h = 256 .. 2048
#pragma unroll
  for (int j = 0; j < RHT_EPT; ++j) v[j] = __fmul_rn(v[j], 0x1p-6f);
}
// the 128 sign words of rotation block rb: words 128 rb .. 128 rb + 127 of the stream = Philox blocks 32 rb .. 32 rb + 31, one per lane
__device__ __forceinline__ void rht_sign_words(unsigned* sgn, const DpStream& s, size_t rb, int t) {
  if (t < RHT_BLOCK / 128) reinterpret_cast<uint4*>(sgn)[t] = dp_words(s, (unsigned long long)rb * (RHT_BLOCK / 128) + t);
}
__device__ __forceinline__ float rht_flip(float v, unsigned bit) { return __uint_as_float(__float_as_uint(v) ^ (bit << 31)); }
__device__ __forceinline__ void rht_sign_a(const unsigned* sgn, float (&v)[RHT_EPT], int t) {      // elements 16 t + j
  const unsigned bits = sgn[t >> 1] >> (16 * (t & 1));
#pragma unroll
  for (int j = 0; j < RHT_EPT; ++j) v[j] = rht_flip(v[j], (bits >> j) & 1u);
}
__device__ __forceinline__ void rht_sign_c(const unsigned* sgn, float (&v)[RHT_EPT], int t) {      // elements 256 j + t
#pragma unroll
  for (int j = 0; j < RHT_EPT; ++j) v[j] = rht_flip(v[j], (sgn[8 * j + (t >> 5)] >> (t & 31)) & 1u);
}
// rot <- elements of block rb of (b ? a - b : a), read in the memory layout (lane t: 16-byte slots 256 h + t); 0 behind n
__device__ __forceinline__ void rht_stage_in(float* rot, const float* __restrict__ a, const float* __restrict__ b, size_t rb, size_t n, int t) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int le = 4 * (256 * h + t);
    const size_t e = rb * RHT_BLOCK + le;
    f4 u = f4{0.f, 0.f, 0.f, 0.f};
    if (e + 4 <= n) {
      u = ld_once<4>(a, e / 4);
      if (b) {
        const f4 w = ld_once<4>(b, e / 4);
        u = f4{__fsub_rn(u.x, w.x), __fsub_rn(u.y, w.y), __fsub_rn(u.z, w.z), __fsub_rn(u.w, w.w)};
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (e + c < n) u[c] = b ? __fsub_rn(a[e + c], b[e + c]) : a[e + c];
    }
    *reinterpret_cast<f4*>(rot + rht_idx(le)) = u;
  }
}

// A stream's key as the loop body sees it: opaque to the optimiser, so that the 20 round keys of Philox (k + r W) are formed where they are
// used, by scalar additions, instead of being hoisted out of the rotation-block loop into 20 SGPRs per stream that then spill
__device__ __forceinline__ DpStream dp_stream_here(DpStream s) {
  asm volatile("" : "+s"(s.k0), "+s"(s.k1));
  return s;
}

// ---- the generator's split -------------------------------------------------------------------------------------------------------------
// msk[p][16 c + i] = sum over the streams s = p, p + PARTS, ... < k of sign_s (word i of ChaCha20 block block0 + c), field-wise, for the
// parts p < min(k, PARTS).  A part is one or two whole waves: its stream index is wave-uniform (keys and nonces stay in SGPRs).
template <int BITS>
__device__ __forceinline__ void narrow_mask_parts(unsigned* msk, const MaskStreams& ms, int k, unsigned block0, int t) {
  using F = Fields<BITS>;
  const int part = __builtin_amdgcn_readfirstlane(t / F::CHACHA_BLOCKS), cb = t % F::CHACHA_BLOCKS;
  if (part >= k) return;
  unsigned m[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = 0u;
#pragma unroll 1
  for (int s = part; s < k; s += F::PARTS) {
    unsigned w[16];
    chacha_block(ms.key[s], block0 + (unsigned)cb, ms.nonce[s][0], ms.nonce[s][1], ms.nonce[s][2], w);
    if (ms.sign[s] > 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] = F::add(m[i], w[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] = F::sub(m[i], w[i]);
    }
  }
#pragma unroll
  for (int h = 0; h < 4; ++h)
    reinterpret_cast<uvec4*>(msk + part * F::WORDS + 16 * cb)[h] = uvec4{m[4 * h], m[4 * h + 1], m[4 * h + 2], m[4 * h + 3]};
}
// w (+)= the partial sums of the lane's own words (behind the barrier that follows narrow_mask_parts)
template <int BITS>
__device__ __forceinline__ void narrow_add_parts(const unsigned* msk, int k, unsigned (&w)[Fields<BITS>::WORDS_PER_LANE], int t) {
  using F = Fields<BITS>;
  const int parts = k < F::PARTS ? k : F::PARTS;
  for (int p = 0; p < parts; ++p) {
#pragma unroll
    for (int h = 0; h < F::WORDS_PER_LANE / 4; ++h) {
      const uvec4 m = reinterpret_cast<const uvec4*>(msk + p * F::WORDS + F::WORDS_PER_LANE * t)[h];
      w[4 * h] = F::add(w[4 * h], m.x); w[4 * h + 1] = F::add(w[4 * h + 1], m.y);
      w[4 * h + 2] = F::add(w[4 * h + 2], m.z); w[4 * h + 3] = F::add(w[4 * h + 3], m.w);
    }
  }
}

// ---- the encoder -----------------------------------------------------------------------------------------------------------------------
// t = v coef;  fl = floor(t);  q = clamp(fl + [r 2^-24 < t - fl], -limit, limit) with r the top 24 bits of the draw; a t that is NaN or
// infinite gives 0.  t - fl is ONE fp32 subtraction, not an exact difference: for a tiny negative t (fl = -1) it rounds to 1.0f and q is
// 0 whatever the draw, a bias below 2^-24 of a code, and the restatement makes the same subtraction.  fl is brought inside +-(limit + 1)
// first (every such integer is a float), so the sum fl + [..] and its conversion to int lose nothing.
__device__ __forceinline__ int narrow_encode(float v, float coef, unsigned draw, int limit, int& saturated, int& nonfinite) {
  const float t = __fmul_rn(v, coef);
  const bool finite = __builtin_fabsf(t) < __builtin_inff();
  const float fl = __builtin_floorf(t);
  const float frac = __fsub_rn(t, fl);
  const float u = __fmul_rn((float)(draw >> 8), 0x1p-24f);
  const float lim1 = (float)(limit + 1);
  const float fc = __builtin_fminf(__builtin_fmaxf(finite ? fl : 0.f, -lim1), lim1);
  int q = (int)__fadd_rn(fc, u < frac ? 1.f : 0.f);
  q = min(max(q, -limit), limit);
  q = finite ? q : 0;
  saturated += (finite && (q == limit || q == -limit)) ? 1 : 0;
  nonfinite += finite ? 0 : 1;
  return q;
}

// ---- the kernels -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RHT_THREADS) void rht_fill_kernel(float* __restrict__ dst, const float* __restrict__ src, NarrowArgs a, int inverse) {
  __shared__ __attribute__((aligned(16))) float rot[RHT_LDS_WORDS];
  __shared__ __attribute__((aligned(16))) unsigned sgn[RHT_BLOCK / 32];
  const int t = threadIdx.x;
  const size_t nblk = rht_padded(a.n) / RHT_BLOCK;
  for (size_t rb = blockIdx.x; rb < nblk; rb += gridDim.x) {
    __syncthreads();                                // the last iteration's reads of rot and sgn
    rht_sign_words(sgn, dp_stream_here(a.signs), rb, t);
    rht_stage_in(rot, src, nullptr, rb, a.n, t);
    __syncthreads();
    float v[RHT_EPT];
    rht_load_a(rot, v, t);
    if (!inverse) rht_sign_a(sgn, v, t);
    rht_rotate(rot, v, t);
    if (inverse) rht_sign_c(sgn, v, t);
#pragma unroll
    for (int j = 0; j < RHT_EPT; ++j) dst[rb * RHT_BLOCK + rht_elem_c(t, j)] = v[j];
  }
}

template <int BITS>
__global__ __launch_bounds__(RHT_THREADS) void secagg_mask_narrow_kernel(unsigned* __restrict__ y, const float* __restrict__ x, const float* __restrict__ xi,
                                                                         float coef, int limit, MaskStreams ms, NarrowArgs a, int* __restrict__ counters) {
  using F = Fields<BITS>;
  __shared__ __attribute__((aligned(16))) float rot[RHT_LDS_WORDS];
  __shared__ __attribute__((aligned(16))) unsigned msk[F::PARTS * F::WORDS];
  __shared__ __attribute__((aligned(16))) unsigned sgn[RHT_BLOCK / 32];
  const int t = threadIdx.x;
  const size_t nblk = rht_padded(a.n) / RHT_BLOCK;
  int saturated = 0, nonfinite = 0;
  for (size_t rb = blockIdx.x; rb < nblk; rb += gridDim.x) {
    __syncthreads();                                // the last iteration's reads of rot, msk and sgn
    rht_sign_words(sgn, dp_stream_here(a.signs), rb, t);
    rht_stage_in(rot, xi, x, rb, a.n, t);           // u = xi - x
    narrow_mask_parts<BITS>(msk, ms, a.k, a.counter0 + (unsigned)(rb * F::CHACHA_BLOCKS), t);
    __syncthreads();
    float v[RHT_EPT];
    rht_load_a(rot, v, t);
    rht_sign_a(sgn, v, t);                          // D u
    rht_rotate(rot, v, t);                          // 2^-6 H D u, elements 256 j + t
#pragma unroll
    for (int j = 0; j < RHT_EPT; ++j) rot[rht_idx(rht_elem_c(t, j))] = v[j];
    __syncthreads();
    rht_load_a(rot, v, t);                          // elements 16 t + j: the lane's packed words
    int q[RHT_EPT];
    const DpStream draws = dp_stream_here(a.draws);
#pragma unroll
    for (int h = 0; h < 4; ++h) {                   // element e draws word e of the private stream: Philox block e / 4
      const uint4 r = dp_words(draws, (unsigned long long)rb * (RHT_BLOCK / 4) + 4 * t + h);
      q[4 * h] = narrow_encode(v[4 * h], coef, r.x, limit, saturated, nonfinite);
      q[4 * h + 1] = narrow_encode(v[4 * h + 1], coef, r.y, limit, saturated, nonfinite);
      q[4 * h + 2] = narrow_encode(v[4 * h + 2], coef, r.z, limit, saturated, nonfinite);
      q[4 * h + 3] = narrow_encode(v[4 * h + 3], coef, r.w, limit, saturated, nonfinite);
    }
    unsigned w[F::WORDS_PER_LANE];
    F::pack(q, w);
    narrow_add_parts<BITS>(msk, a.k, w, t);
    uvec4* yv = reinterpret_cast<uvec4*>(y + rb * F::WORDS + F::WORDS_PER_LANE * t);
#pragma unroll
    for (int h = 0; h < F::WORDS_PER_LANE / 4; ++h) yv[h] = uvec4{w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
  }
  if (counters) {                                   // one atomic per wave and counter (integer sums: one result whatever the order)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      saturated += __shfl_xor(saturated, o, 64);
      nonfinite += __shfl_xor(nonfinite, o, 64);
    }
    if ((t & 63) == 0) {
      if (saturated) atomicAdd(counters, saturated);
      if (nonfinite) atomicAdd(counters + 1, nonfinite);
    }
  }
}

// out may be x: element e of both is touched by one lane, read before write; acc is read when !first, written when !last
template <int BITS, int KU>
__global__ __launch_bounds__(RHT_THREADS) void secagg_aggregate_narrow_kernel(float* out, const float* x, unsigned* acc, BytePtrs<SECAGG_MAX_UPLOADS> ys,
                                                                              MaskStreams ms, NarrowArgs a, float scale, float rescale, int first,
                                                                              int last) {
  using F = Fields<BITS>;
  __shared__ __attribute__((aligned(16))) float rot[RHT_LDS_WORDS];
  __shared__ __attribute__((aligned(16))) unsigned msk[F::PARTS * F::WORDS];
  __shared__ __attribute__((aligned(16))) unsigned sgn[RHT_BLOCK / 32];
  const int t = threadIdx.x;
  const size_t nblk = rht_padded(a.n) / RHT_BLOCK;
  for (size_t rb = blockIdx.x; rb < nblk; rb += gridDim.x) {
    __syncthreads();                                // the last iteration's reads of rot, msk and sgn
    if (last) rht_sign_words(sgn, dp_stream_here(a.signs), rb, t);
    narrow_mask_parts<BITS>(msk, ms, a.k, a.counter0 + (unsigned)(rb * F::CHACHA_BLOCKS), t);
    const size_t v0 = (rb * F::WORDS + F::WORDS_PER_LANE * t) / 4;      // the lane's first 16-byte slot
    unsigned s[F::WORDS_PER_LANE];
#pragma unroll
    for (int i = 0; i < F::WORDS_PER_LANE; ++i) s[i] = 0u;
    if (!first) {
#pragma unroll
      for (int h = 0; h < F::WORDS_PER_LANE / 4; ++h) {
        const uvec4 w = reinterpret_cast<const uvec4*>(acc)[v0 + h];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[4 * h + c] = w[c];
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int h = 0; h < F::WORDS_PER_LANE / 4; ++h) {
        const uvec4 w = ld_once_u4(reinterpret_cast<const unsigned*>(ys.src[u]), v0 + h);
#pragma unroll
        for (int c = 0; c < 4; ++c) s[4 * h + c] = F::add(s[4 * h + c], w[c]);
      }
    }
    __syncthreads();
    narrow_add_parts<BITS>(msk, a.k, s, t);
    if (!last) {                                    // (uniform: every lane of the grid takes the same side)
#pragma unroll
      for (int h = 0; h < F::WORDS_PER_LANE / 4; ++h) reinterpret_cast<uvec4*>(acc)[v0 + h] = uvec4{s[4 * h], s[4 * h + 1], s[4 * h + 2], s[4 * h + 3]};
      continue;
    }
    float v[RHT_EPT];
#pragma unroll
    for (int j = 0; j < RHT_EPT; ++j) v[j] = __fmul_rn((float)F::field(s[j / F::PER_WORD], j % F::PER_WORD), scale);      // S 2^-f: exact
    rht_rotate(rot, v, t);                          // 2^-6 H s, elements 256 j + t
    rht_sign_c(sgn, v, t);
#pragma unroll
    for (int j = 0; j < RHT_EPT; ++j) {
      const size_t e = rb * RHT_BLOCK + rht_elem_c(t, j);
      if (e >= a.n) continue;
      const float d = __fmul_rn(v[j], rescale);
      out[e] = x ? __fadd_rn(x[e], d) : d;
    }
  }
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------
static inline int narrow_grid(size_t n) {
  const size_t nblk = rht_padded(n) / RHT_BLOCK;
  return (int)(nblk > 2048 ? 2048 : nblk);
}
static inline int narrow_bits_ok(const char* who, int bits) {
  FEDFR_REQUIRE(bits == 8 || bits == 16, "%s: bits must be 8 or 16 (bits=%d)", who, bits);
  return FEDFR_OK;
}

int secagg_rht_fill(float* dst, const float* src, size_t n, unsigned long long rotation_seed, unsigned long long round, int inverse, hipStream_t st) {
  FEDFR_REQUIRE(dst && src, "rht_fill: null pointer (dst=%p src=%p)", (void*)dst, (const void*)src);
  FEDFR_REQUIRE(dst != src, "rht_fill: dst and src must be distinct (%p)", (void*)dst);
  FEDFR_REQUIRE((((uintptr_t)dst | (uintptr_t)src) & 15) == 0, "rht_fill: dst (%p) and src (%p) must be 16-byte aligned", (void*)dst, (const void*)src);
  if (n == 0) return FEDFR_OK;
  NarrowArgs a{};
  a.signs = dp_stream(rotation_seed, round, RHT_SIGN_SID, 0);
  a.n = n;
  hipLaunchKernelGGL(rht_fill_kernel, dim3(narrow_grid(n)), dim3(RHT_THREADS), 0, st, dst, src, a, inverse ? 1 : 0);
  FEDFR_LAUNCH_CHECK("rht_fill");
  return FEDFR_OK;
}

int secagg_mask_narrow(unsigned* y, const float* x, const float* xi, float coef, int participants, int bits, unsigned long long rotation_seed,
                       unsigned long long private_seed, unsigned long long round, const unsigned* keys, const unsigned* nonces, const int* signs,
                       int k, unsigned counter0, size_t n, int* counters, hipStream_t st) {
  FEDFR_REQUIRE(y && x && xi, "secagg_mask_narrow: null pointer (y=%p x=%p xi=%p)", (void*)y, (const void*)x, (const void*)xi);
  FEDFR_TRY(narrow_bits_ok("secagg_mask_narrow", bits));
  const int top = (1 << (bits - 1)) - 1;
  FEDFR_REQUIRE(participants >= 1 && participants <= top, "secagg_mask_narrow: 1 to %d participants at %d bits, so that the code limit %d / K is >= 1 (K=%d)",
                top, bits, top, participants);
  MaskStreams ms{};
  FEDFR_TRY(mask_streams_fill(ms, "secagg_mask_narrow", keys, nonces, signs, k));
  FEDFR_REQUIRE((((uintptr_t)y | (uintptr_t)x | (uintptr_t)xi) & 15) == 0, "secagg_mask_narrow: y (%p), x (%p) and xi (%p) must be 16-byte aligned",
                (void*)y, (const void*)x, (const void*)xi);
  FEDFR_REQUIRE(((uintptr_t)counters & 3) == 0, "secagg_mask_narrow: counters (%p) must be 4-byte aligned", (void*)counters);
  if (n == 0) return FEDFR_OK;
  FEDFR_TRY(counter_fits("secagg_mask_narrow", rht_padded(n) / (32 / bits), counter0));
  NarrowArgs a{};
  a.signs = dp_stream(rotation_seed, round, RHT_SIGN_SID, 0);
  a.draws = dp_stream(private_seed, round, RHT_ROUND_SID, 0);
  a.counter0 = counter0;
  a.k = k;
  a.n = n;
  const int limit = top / participants;
  if (bits == 8)
    hipLaunchKernelGGL(secagg_mask_narrow_kernel<8>, dim3(narrow_grid(n)), dim3(RHT_THREADS), 0, st, y, x, xi, coef, limit, ms, a, counters);
  else
    hipLaunchKernelGGL(secagg_mask_narrow_kernel<16>, dim3(narrow_grid(n)), dim3(RHT_THREADS), 0, st, y, x, xi, coef, limit, ms, a, counters);
  FEDFR_LAUNCH_CHECK("secagg_mask_narrow");
  return FEDFR_OK;
}

int secagg_aggregate_narrow(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, int bits, unsigned long long rotation_seed,
                            unsigned long long round, const unsigned* keys, const unsigned* nonces, const int* signs, int k, unsigned counter0,
                            int frac_bits, float rescale, size_t n, int first, int last, hipStream_t st) {
  FEDFR_REQUIRE(ku >= 0 && ku <= SECAGG_MAX_UPLOADS, "secagg_aggregate_narrow: 0 to %d uploads per call (ku=%d)", SECAGG_MAX_UPLOADS, ku);
  FEDFR_TRY(narrow_bits_ok("secagg_aggregate_narrow", bits));
  MaskStreams ms{};
  FEDFR_TRY(mask_streams_fill(ms, "secagg_aggregate_narrow", keys, nonces, signs, k));
  FEDFR_REQUIRE(k + ku > 0, "secagg_aggregate_narrow: nothing to add (ku=%d, k=%d)", ku, k);
  FEDFR_REQUIRE(ku == 0 || ys, "secagg_aggregate_narrow: null pointer (ys=%p) with ku=%d", (const void*)ys, ku);
  FEDFR_REQUIRE(frac_bits >= 0 && frac_bits <= 30, "secagg_aggregate_narrow: frac_bits must be 0 to 30 (frac_bits=%d)", frac_bits);
  FEDFR_REQUIRE(std::isfinite(rescale), "secagg_aggregate_narrow: rescale must be finite (rescale=%g)", (double)rescale);
  first = first ? 1 : 0;
  last = last ? 1 : 0;
  FEDFR_REQUIRE((first && last) || acc, "secagg_aggregate_narrow: a chained pass (first=%d last=%d) needs acc", first, last);
  FEDFR_REQUIRE(!last || out, "secagg_aggregate_narrow: the last pass (last=%d) needs out", last);
  BytePtrs<SECAGG_MAX_UPLOADS> yp{};
  uintptr_t al = (uintptr_t)out | (uintptr_t)x | (uintptr_t)acc;      // (null: no bits)
  FEDFR_TRY(byte_ptrs_fill(yp, reinterpret_cast<const void* const*>(ys), ku, "secagg_aggregate_narrow", "upload", al));
  FEDFR_REQUIRE((al & 15) == 0, "secagg_aggregate_narrow: out (%p), x (%p), acc (%p) and the uploads must be 16-byte aligned", (void*)out,
                (const void*)x, (void*)acc);
  if (n == 0) return FEDFR_OK;
  FEDFR_TRY(counter_fits("secagg_aggregate_narrow", rht_padded(n) / (32 / bits), counter0));
  NarrowArgs a{};
  a.signs = dp_stream(rotation_seed, round, RHT_SIGN_SID, 0);
  a.counter0 = counter0;
  a.k = k;
  a.n = n;
  const float scale = std::ldexp(1.0f, -frac_bits);
  dispatch_int<0, SECAGG_MAX_UPLOADS>(ku, [&](auto kc) {
    constexpr int KU = decltype(kc)::value;
    if (bits == 8)
      hipLaunchKernelGGL((secagg_aggregate_narrow_kernel<8, KU>), dim3(narrow_grid(n)), dim3(RHT_THREADS), 0, st, out, last ? x : nullptr, acc, yp, ms, a,
                         scale, rescale, first, last);
    else
      hipLaunchKernelGGL((secagg_aggregate_narrow_kernel<16, KU>), dim3(narrow_grid(n)), dim3(RHT_THREADS), 0, st, out, last ? x : nullptr, acc, yp, ms, a,
                         scale, rescale, first, last);
  });
  FEDFR_LAUNCH_CHECK("secagg_aggregate_narrow");
  return FEDFR_OK;
}
