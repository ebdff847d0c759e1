// reweighted aggregation over flat fp32 client states: the fused step-and-distances pass and the weights kernel of the geometric median
// (RFA) and of centred clipping (see reweight.hip)
#pragma once
#include "common.h"

size_t reweight_ws_bytes(int k, size_t n);
int reweight_step(float* dst, const float* z, const float* const* xs, const float* beta, int k, size_t n, void* workspace, size_t ws_bytes,
                  hipStream_t st);
int reweight_weights(int rule, const double* alpha, double param, int slot, int iters, int k, size_t n, const void* workspace, size_t ws_bytes,
                     double* hist_d, float* hist_beta, double* info, hipStream_t st);
