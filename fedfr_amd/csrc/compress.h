// compressed client uploads: 8 / 4-bit codes of x_i - x (+ the client's residual) with one shared power-of-two scale byte per 32
// elements, and the weighted aggregate of up to 8 such uploads (see compress.hip; the format: include/fedfr_hip.h)
#pragma once
#include "common.h"

size_t delta_code_bytes(int bits, size_t n);
size_t delta_scale_bytes(size_t n);
int delta_quantize(const float* x, const float* xi, float* resid, void* codes, unsigned char* scales, int bits, size_t n, int* nonfinite_blocks,
                   hipStream_t st);
int delta_aggregate(float* dst, const float* base, const void* const* codes, const unsigned char* const* scales, const float* ws, int k, int bits,
                    size_t n, int accumulate, hipStream_t st);
// the clip of compressed uploads: squared norms of <= 8 uploads as the server will apply them, straight from the codes and the scale bytes,
// and the clipped weights (the workspace rule is shared with sparse.hip's sparse_sqnorm: m = n there, the largest keep here)
size_t upload_sqnorm_ws_bytes(int k, size_t m);
int delta_sqnorm(const void* const* codes, const unsigned char* const* scales, const float* ws, int k, int bits, size_t n, float clip, double* sq,
                 float* coef, void* workspace, size_t ws_bytes, hipStream_t st);
// delta_aggregate with the weights read from DEVICE memory and, on the last pass, noise_std z of the stream of dp.h added before `base`
int delta_aggregate_dp(float* dst, const float* base, const void* const* codes, const unsigned char* const* scales, const float* coef, int k, int bits,
                       size_t n, int accumulate, int last, float noise_std, unsigned long long seed, unsigned long long round, unsigned stream_id,
                       unsigned long long offset, hipStream_t st);
