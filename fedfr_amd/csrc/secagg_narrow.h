// Narrow secure aggregation (see secagg_narrow.hip): masked uploads of 8- or 16-bit codes packed into 32-bit words and summed FIELD-WISE in
// Z / 2^b, after a block-diagonal randomised Hadamard rotation and stochastic rounding (Kairouz, Liu, Steinke, "The Distributed Discrete
// Gaussian Mechanism for Federated Learning with Secure Aggregation", ICML 2021, sections 4 and 5: flatten, round, sum modulo).  The format is
// stated in include/fedfr_hip.h, "NARROW WORDS", and restated in numpy in tests/secagg_narrow_cases.py.  Here: the constants, the field-wise
// arithmetic, the rotation and the encoder, each written ONCE for the three kernels, and the host entry points.  The generators are those of
// secagg.h (ChaCha20 mask streams) and dp.h (Philox: the public signs and the private rounding draws); neither is written again.
#pragma once
#include "common.h"
#include "dp.h"
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

int secagg_rht_fill(float* dst, const float* src, size_t n, unsigned long long rotation_seed, unsigned long long round, int inverse,
                    hipStream_t st);
int secagg_mask_narrow(unsigned* y, const float* x, const float* xi, float coef, int participants, int bits, unsigned long long rotation_seed,
                       unsigned long long private_seed, unsigned long long round, const unsigned* keys, const unsigned* nonces, const int* signs,
                       int k, unsigned counter0, size_t n, int* counters, hipStream_t st);
int secagg_aggregate_narrow(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, int bits,
                            unsigned long long rotation_seed, unsigned long long round, const unsigned* keys, const unsigned* nonces,
                            const int* signs, int k, unsigned counter0, int frac_bits, float rescale, size_t n, int first, int last,
                            hipStream_t st);
