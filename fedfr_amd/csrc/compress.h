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
