// top-k sparsified client uploads: the `keep` largest-magnitude entries of x_i - x (+ the client's residual) as sorted (index, value) pairs,
// found by an exact radix select on the device, and the weighted aggregate of up to 8 such uploads (see sparse.hip; the format:
// include/fedfr_hip.h)
#pragma once
#include "common.h"

size_t topk_workspace_bytes(size_t n, int feedback);
int topk_sparsify(const float* x, const float* xi, float* resid, size_t n, size_t keep, unsigned* idx, float* val, int* nonfinite, void* ws,
                  hipStream_t st);
int sparse_aggregate(float* dst, const float* base, const unsigned* const* idx, const float* const* val, const size_t* keeps, const float* ws, int k,
                     size_t n, int accumulate, hipStream_t st);
// the clip of top-k uploads: squared norms of <= 8 uploads (sum of val^2), the count of entries that break the format (index out of range or
// not ascending: the scattered vector has that norm only without them), and the clipped weights
int sparse_sqnorm(const unsigned* const* idx, const float* const* val, const size_t* keeps, const float* ws, int k, size_t n, float clip, double* sq,
                  float* coef, int* violations, void* workspace, size_t ws_bytes, hipStream_t st);
// sparse_aggregate with the weights read from DEVICE memory and, on the last pass, noise_std z of the stream of dp.h added to EVERY element
int sparse_aggregate_dp(float* dst, const float* base, const unsigned* const* idx, const float* const* val, const size_t* keeps, const float* coef,
                        int k, size_t n, int accumulate, int last, float noise_std, unsigned long long seed, unsigned long long round,
                        unsigned stream_id, unsigned long long offset, hipStream_t st);
