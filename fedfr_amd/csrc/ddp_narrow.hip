// Distributed differential privacy on 16-bit narrow words: the two halves of the distributed discrete Gaussian mechanism (Kairouz, Liu,
// Steinke, ICML 2021) in ONE pass.  A client clips its update, rotates it, rounds it stochastically to integer codes, adds its own share of
// discrete Gaussian noise mod 2^16, packs two fields to a word and masks them field-wise.  The format is stated in include/fedfr_hip.h
// ("NARROW WORDS UNDER DISTRIBUTED DP") and restated in numpy in tests/ddp_narrow_cases.py.  Nothing is written here a second time:
//   the rotation, the generator's split, the encoder, the field arithmetic      secagg_narrow.h (the pass is secagg_mask_narrow_kernel<16>'s)
//   the sampler, its queue and the noise stream                                 ddp.h
//   ddp_mask_narrow_kernel     y = pack(encode(2^-6 H D (xi - x) clip_coef 2^f) + noise) (+) the k streams; x and xi read once, y written
//                              once; the exact integer sum of the squared codes of all n_pad elements, taken before the noise
// ONE WORKGROUP, ONE ROTATION BLOCK, as there.  The noise of lane t's elements 16 t + j (positions 4096 rb + 16 t + j of the padded ROTATED
// vector: the padding coordinates carry a part of the update after the rotation, so they carry noise too) is drawn by THE QUEUE of ddp.h
// into the wave's strip of 1024 words.  LDS: the strips ALIAS the rotation buffer (4 x 1024 of its 5376 words), behind the barrier that
// follows every lane's last read of it, so the pass keeps the 38.5 KB and the occupancy of the narrow pass.  Like ddp_mask_kernel the pass
// is bound by the two fp64 transcendentals of an attempt, 1.31 attempts per element, not by memory.
#include "ddp.h"
#include "secagg_narrow.h"
#include <cmath>

static_assert(RHT_THREADS / 64 * RHT_EPT * 64 <= RHT_LDS_WORDS, "the four noise strips fit the rotation buffer they alias");

__global__ __launch_bounds__(RHT_THREADS) void ddp_mask_narrow_kernel(unsigned* __restrict__ y, const float* __restrict__ x, const float* __restrict__ xi,
                                                                      const float* __restrict__ clip_coef, float scale, int limit, DpStream ns, DGauss g,
                                                                      MaskStreams ms, NarrowArgs a, int* __restrict__ counters,
                                                                      unsigned long long* __restrict__ sqnorm) {
  using F = Fields<16>;
  __shared__ __attribute__((aligned(16))) float rot[RHT_LDS_WORDS];
  __shared__ __attribute__((aligned(16))) unsigned msk[F::PARTS * F::WORDS];
  __shared__ __attribute__((aligned(16))) unsigned sgn[RHT_BLOCK / 32];
  __shared__ unsigned long long red[RHT_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  unsigned* nz = reinterpret_cast<unsigned*>(rot) + wv * (RHT_EPT * 64);      // the wave's noise strip: value i of a lane at nz[i * 64 + lane]
  const size_t nblk = rht_padded(a.n) / RHT_BLOCK;
  const float coef = __fmul_rn(clip_coef[0], scale);      // min(1, C / ||xi - x||) 2^f: a power-of-two scaling, exact
  int saturated = 0, nonfinite = 0, exhausted = 0;
  unsigned long long sq = 0ull;
  for (size_t rb = blockIdx.x; rb < nblk; rb += gridDim.x) {
    __syncthreads();                                // the last iteration's reads of rot (the strips), msk and sgn
    rht_sign_words(sgn, dp_stream_here(a.signs), rb, t);
    rht_stage_in(rot, xi, x, rb, a.n, t);           // u = xi - x
    narrow_mask_parts<16>(msk, ms, a.k, a.counter0 + (unsigned)(rb * F::CHACHA_BLOCKS), t);
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
    __syncthreads();                                // every lane has read rot for the last time: the strips may take its place
    const size_t e0 = rb * RHT_BLOCK + (size_t)RHT_EPT * t;
    exhausted += dgauss_queue(nz, lane, RHT_EPT, ns, g, [&](int i) { return e0 + i; });
#pragma unroll
    for (int j = 0; j < RHT_EPT; ++j) {
      sq += (unsigned long long)((long long)q[j] * q[j]);
      q[j] += (int)nz[j * 64 + lane];               // mod 2^16 once packed: pack keeps the low 16 bits
    }
    unsigned w[F::WORDS_PER_LANE];
    F::pack(q, w);
    narrow_add_parts<16>(msk, a.k, w, t);
    narrow_store_lane<16>(y, rb, t, w);
  }
  // integer sums: one result whatever the order.  Lanes by shuffles; the counters then take one atomic per wave, the squared norm goes
  // through LDS and takes ONE 64-bit atomic add per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    saturated += __shfl_xor(saturated, o, 64);
    nonfinite += __shfl_xor(nonfinite, o, 64);
    exhausted += __shfl_xor(exhausted, o, 64);
    sq += __shfl_xor(sq, o, 64);
  }
  if (lane == 0) {
    red[wv] = sq;
    if (counters) {
      if (saturated) atomicAdd(counters, saturated);
      if (nonfinite) atomicAdd(counters + 1, nonfinite);
      if (exhausted) atomicAdd(counters + 2, exhausted);
    }
  }
  __syncthreads();
  if (t == 0 && sqnorm) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int w = 0; w < RHT_THREADS / 64; ++w) s += red[w];
    if (s) atomicAdd(sqnorm, s);
  }
}

int ddp_secagg_mask_narrow_dp(unsigned* y, const float* x, const float* xi, const float* clip_coef, int frac_bits, int limit, int bits,
                              unsigned long long rotation_seed, unsigned long long private_seed, unsigned long long round,
                              unsigned long long noise_seed, unsigned long long noise_round, unsigned long long noise_offset, double sigma,
                              const unsigned* keys, const unsigned* nonces, const int* signs, int k, unsigned counter0, size_t n, int* counters,
                              unsigned long long* sqnorm, hipStream_t st) {
  const char* who = "secagg_mask_narrow_dp";
  FEDFR_REQUIRE(y && x && xi && clip_coef, "%s: null pointer (y=%p x=%p xi=%p clip_coef=%p)", who, (void*)y, (const void*)x, (const void*)xi,
                (const void*)clip_coef);
  FEDFR_REQUIRE(bits == 16, "%s: bits must be 16: the sampler's smallest sigma leaves no room for codes in 8-bit fields, and 32-bit words "
                "are fedfr_secagg_mask_dp (bits=%d)", who, bits);
  FEDFR_REQUIRE(frac_bits >= 8 && frac_bits <= 30, "%s: frac_bits must be 8 to 30 (frac_bits=%d)", who, frac_bits);
  FEDFR_REQUIRE(limit >= 1 && limit <= 32767, "%s: code_limit must be 1 to 32767 (code_limit=%d)", who, limit);
  FEDFR_REQUIRE(n <= (size_t)-1 - RHT_BLOCK, "%s: n = %zu cannot be padded to whole rotation blocks", who, n);
  FEDFR_TRY(dgauss_args(who, sigma, rht_padded(n), noise_offset));
  MaskStreams ms{};
  FEDFR_TRY(mask_streams_fill(ms, who, keys, nonces, signs, k));
  FEDFR_REQUIRE((((uintptr_t)y | (uintptr_t)x | (uintptr_t)xi) & 15) == 0, "%s: y (%p), x (%p) and xi (%p) must be 16-byte aligned", who, (void*)y,
                (const void*)x, (const void*)xi);
  FEDFR_REQUIRE(((uintptr_t)clip_coef & 3) == 0 && ((uintptr_t)counters & 3) == 0 && ((uintptr_t)sqnorm & 7) == 0,
                "%s: clip_coef (%p) and counters (%p) must be 4-byte, sqnorm (%p) 8-byte aligned", who, (const void*)clip_coef, (void*)counters,
                (void*)sqnorm);
  if (n == 0) return FEDFR_OK;
  FEDFR_TRY(counter_fits(who, rht_padded(n) / Fields<16>::PER_WORD, counter0));
  NarrowArgs a{};
  a.signs = dp_stream(rotation_seed, round, RHT_SIGN_SID, 0);
  a.draws = dp_stream(private_seed, round, RHT_ROUND_SID, 0);
  a.counter0 = counter0;
  a.k = k;
  a.n = n;
  hipLaunchKernelGGL(ddp_mask_narrow_kernel, dim3(narrow_grid(n)), dim3(RHT_THREADS), 0, st, y, x, xi, clip_coef, std::ldexp(1.0f, frac_bits), limit,
                     dgauss_stream(noise_seed, noise_round, DDP_NOISE_STREAM, noise_offset), dgauss_params(sigma), ms, a, counters, sqnorm);
  FEDFR_LAUNCH_CHECK("secagg_mask_narrow_dp");
  return FEDFR_OK;
}
