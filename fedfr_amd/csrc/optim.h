// flat-buffer optimiser / aggregation / PartialFC sampling kernels (see optim.hip)
#pragma once
#include "common.h"

int optim_sgd(float* p, float* g, float* buf, bf16_t* shadow, size_t n, float lr, float mu, float wd, int first,
              hipStream_t st, float gscale = 1.f, unsigned* overflow = nullptr,    // gscale != 1: g holds gradient / gscale; it is multiplied in the kernel and stored back
              const float* anchor = nullptr, float prox = 0.f, const float* corr = nullptr);      // DRIFT TERMS (fedfr_hip.h): d += prox (p - anchor); d += corr
// SCAFFOLD's end-of-round pass: cn = fma(inv_mass, x - y, -corr); dc = cn - c_i; c_i = cn (corr null: +0.0)
int optim_scaffold_control(float* ci, float* dc, const float* x, const float* y, const float* corr, float inv_mass, size_t n, hipStream_t st);
int optim_fedavg_axpy(float* dst, const float* src, float w, size_t n, int accumulate, hipStream_t st);
int optim_fedavg_multi(float* dst, const float* const* srcs, const float* ws, int k, size_t n, int accumulate, hipStream_t st);
size_t optim_fedopt_sqnorm_ws_bytes(int k, size_t n);
int optim_fedopt_sqnorm(const float* x, const float* const* xs, const float* ws, int k, size_t n, float clip, double* sq, float* coef,
                        void* workspace, size_t ws_bytes, hipStream_t st);
// the last step of every squared-norm pass (fedopt_sqnorm_final_kernel, launched here and nowhere else): sq_i = the `grid` fp64 partials of row
// i of `part` in ascending order, coef_i = ws[i] min(1, clip / sqrt(sq_i)) in fp64, rounded once.  The callers (optim_fedopt_sqnorm,
// compress.hip: delta_sqnorm, sparse.hip: sparse_sqnorm) have checked the arguments
int optim_fedopt_sqnorm_final(const double* part, int grid, int k, const float* ws, float clip, double* sq, float* coef, hipStream_t st);
int optim_fedopt_multi(int kind, float* x_out, const float* x, const float* const* xs, const float* coef, int k, size_t n, float* m, float* v,
                       float* scratch, int first, int last, float lr, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                       float tau, hipStream_t st);
int optim_fedavg_i64(float* acc, const long long* src, float w, int n, int accumulate, long long* out_trunc, hipStream_t st);
int optim_pfc_rand(float* perm, int n, unsigned long long seed, unsigned long long step, hipStream_t st);
int optim_pfc_localize(long long* label, int n, long long class_start, int num_local, float* perm, hipStream_t st);
int optim_pfc_topk(const float* perm, int n, int k, long long* index, int* npos_out, hipStream_t st);
int optim_pfc_positive(const float* perm, int n, long long* index, int* count, hipStream_t st);
int optim_pfc_remap(long long* label, int n, const long long* index, int k, hipStream_t st);
int optim_rows(float* dst, const float* src, const long long* index, int k, int D, int scatter, int nrows, hipStream_t st);
