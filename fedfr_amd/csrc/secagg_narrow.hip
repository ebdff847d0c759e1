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
// The rotation, the generator's split and the encoder are in secagg_narrow.h: ddp_narrow.hip builds its pass from the same pieces.
#include "secagg_narrow.h"
#include <cmath>

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
    narrow_encode_lane(v, q, dp_stream_here(a.draws), rb, t, coef, limit, saturated, nonfinite);
    unsigned w[F::WORDS_PER_LANE];
    F::pack(q, w);
    narrow_add_parts<BITS>(msk, a.k, w, t);
    narrow_store_lane<BITS>(y, rb, t, w);
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
