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
