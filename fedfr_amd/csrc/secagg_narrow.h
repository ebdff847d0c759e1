// Narrow secure aggregation (see secagg_narrow.hip): masked uploads of 8- or 16-bit codes packed into 32-bit words and summed FIELD-WISE in
// Z / 2^b, after a block-diagonal randomised Hadamard rotation and stochastic rounding (Kairouz, Liu, Steinke, "The Distributed Discrete
// Gaussian Mechanism for Federated Learning with Secure Aggregation", ICML 2021, sections 4 and 5: flatten, round, sum modulo).  The format is
// stated in include/fedfr_hip.h, "NARROW WORDS", and restated in numpy in tests/secagg_narrow_cases.py.  Here: the constants, the field-wise
// arithmetic, the rotation, the generator's split and the encoder, each written ONCE for the kernels of secagg_narrow.hip and for the pass
// of ddp_narrow.hip (the same words under distributed DP), and the host entry points.  The generators are those of secagg.h (ChaCha20 mask
// streams) and dp.h (Philox: the public signs and the private rounding draws); neither is written again.
#pragma once
#include "common.h"
#include "dp.h"
#include "multi_state.h"
#include "secagg.h"

constexpr int RHT_BLOCK = 4096;                       // B: elements of one rotation block = one workgroup iteration
constexpr int RHT_THREADS = 256;                      // lanes of a workgroup: RHT_EPT elements each
constexpr int RHT_EPT = RHT_BLOCK / RHT_THREADS;      // 16
constexpr unsigned RHT_SIGN_SID = 0x52485444u;        // "RHTD": the Philox stream id of the public signs D
constexpr unsigned RHT_ROUND_SID = 0x53525244u;       // "SRRD": the Philox stream id of a client's private rounding draws
static_assert(RHT_EPT == 16 && RHT_BLOCK == 1 << 12, "three phases of four butterfly levels in registers");

__host__ __device__ static inline size_t rht_padded(size_t n) { return (n + RHT_BLOCK - 1) / RHT_BLOCK * RHT_BLOCK; }

// ---- field-wise arithmetic mod 2^BITS on the 32 / BITS fields of a word: no carry or borrow crosses a field ----------------------------
template <int BITS>
struct Fields {
  static_assert(BITS == 8 || BITS == 16, "8- or 16-bit fields");
  static constexpr unsigned HI = BITS == 8 ? 0x80808080u : 0x80008000u;      // the top bit of every field
  static constexpr int PER_WORD = 32 / BITS;                                 // F
  static constexpr int WORDS_PER_LANE = RHT_EPT / PER_WORD;                  // packed words of a lane's 16 elements: 4 or 8
  static constexpr int WORDS = RHT_BLOCK / PER_WORD;                         // packed words of a rotation block: 1024 or 2048
  static constexpr int CHACHA_BLOCKS = WORDS / 16;                           // ChaCha20 blocks per stream and rotation block: 64 or 128
  static constexpr int PARTS = RHT_THREADS / CHACHA_BLOCKS;                  // groups of lanes that share the streams of a launch: 4 or 2
  // the low BITS - 1 bits are added (or subtracted under a planted top bit) without leaving their field; the top bits are a xor
  __host__ __device__ static inline unsigned add(unsigned a, unsigned b) { return ((a & ~HI) + (b & ~HI)) ^ ((a ^ b) & HI); }
  __host__ __device__ static inline unsigned sub(unsigned a, unsigned b) { return ((a | HI) - (b & ~HI)) ^ ((a ^ ~b) & HI); }
  // field i of w as a signed number
  __host__ __device__ static inline int field(unsigned w, int i) { return (int)(w << (32 - BITS * (i + 1))) >> (32 - BITS); }
  // 16 codes -> the lane's packed words: element j is field j % F of word j / F, little end first
  __device__ static inline void pack(const int (&q)[RHT_EPT], unsigned (&w)[WORDS_PER_LANE]) {
#pragma unroll
    for (int i = 0; i < WORDS_PER_LANE; ++i) {
      w[i] = 0u;
#pragma unroll
      for (int c = 0; c < PER_WORD; ++c) w[i] |= ((unsigned)q[PER_WORD * i + c] & ((1u << BITS) - 1u)) << (BITS * c);
    }
  }
};

// what every kernel of the family is told about the public rotation and the mask streams: uniform, by value
struct NarrowArgs {
  DpStream signs;            // the public Rademacher signs D: (rotation seed, round, RHT_SIGN_SID)
  DpStream draws;            // the client's private rounding draws: (private seed, round, RHT_ROUND_SID); unused by the aggregate
  unsigned counter0;         // the ChaCha20 block of packed word 0
  int k;                     // mask streams of this launch
  size_t n;                  // elements (the last rotation block is padded with zeros)
};

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
// the lane's 16 codes of elements 16 t + j of rotation block rb: element e draws word e of the private stream, Philox block e / 4
__device__ __forceinline__ void narrow_encode_lane(const float (&v)[RHT_EPT], int (&q)[RHT_EPT], const DpStream& draws, size_t rb, int t, float coef,
                                                   int limit, int& saturated, int& nonfinite) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const uint4 r = dp_words(draws, (unsigned long long)rb * (RHT_BLOCK / 4) + 4 * t + h);
    q[4 * h] = narrow_encode(v[4 * h], coef, r.x, limit, saturated, nonfinite);
    q[4 * h + 1] = narrow_encode(v[4 * h + 1], coef, r.y, limit, saturated, nonfinite);
    q[4 * h + 2] = narrow_encode(v[4 * h + 2], coef, r.z, limit, saturated, nonfinite);
    q[4 * h + 3] = narrow_encode(v[4 * h + 3], coef, r.w, limit, saturated, nonfinite);
  }
}
// the lane's packed words of rotation block rb, as 16-byte stores
template <int BITS>
__device__ __forceinline__ void narrow_store_lane(unsigned* __restrict__ y, size_t rb, int t, const unsigned (&w)[Fields<BITS>::WORDS_PER_LANE]) {
  using F = Fields<BITS>;
  uvec4* yv = reinterpret_cast<uvec4*>(y + rb * F::WORDS + F::WORDS_PER_LANE * t);
#pragma unroll
  for (int h = 0; h < F::WORDS_PER_LANE / 4; ++h) yv[h] = uvec4{w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------
static inline int narrow_grid(size_t n) {      // one workgroup per rotation block, 2048 at the most
  const size_t nblk = rht_padded(n) / RHT_BLOCK;
  return (int)(nblk > 2048 ? 2048 : nblk);
}

int secagg_rht_fill(float* dst, const float* src, size_t n, unsigned long long rotation_seed, unsigned long long round, int inverse,
                    hipStream_t st);
int secagg_mask_narrow(unsigned* y, const float* x, const float* xi, float coef, int participants, int bits, unsigned long long rotation_seed,
                       unsigned long long private_seed, unsigned long long round, const unsigned* keys, const unsigned* nonces, const int* signs,
                       int k, unsigned counter0, size_t n, int* counters, hipStream_t st);
int secagg_aggregate_narrow(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, int bits,
                            unsigned long long rotation_seed, unsigned long long round, const unsigned* keys, const unsigned* nonces,
                            const int* signs, int k, unsigned counter0, int frac_bits, float rescale, size_t n, int first, int last,
                            hipStream_t st);
