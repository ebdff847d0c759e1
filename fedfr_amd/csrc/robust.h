// robust aggregation over flat fp32 client states: coordinate-wise trimmed mean / median, pairwise squared distances and the
// Krum / Multi-Krum selection (see robust.hip)
#pragma once
#include "common.h"

int robust_trimmed_mean(float* dst, const float* const* srcs, int k, int trim, size_t n, hipStream_t st);
size_t robust_pairdist_ws_bytes(int k, size_t n);
int robust_pairdist(const float* const* xs, int k, size_t n, double* dist, void* workspace, size_t ws_bytes, hipStream_t st);
int robust_krum_select(const double* dist, int k, int f, int m, double* score, int* selected, hipStream_t st);
