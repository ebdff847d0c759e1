// fp32 head kernels (see head.hip).
#pragma once
#include "common.h"

int head_normalize_rows(const float* x, float* xn, float* inv, int R, int D, float eps, hipStream_t st);
int head_normalize_rows_bwd(const float* xn, const float* inv, const float* dxn, float* dx, int R, int D, float beta,
                            hipStream_t st);
int head_sgemm(const float* A, const float* B, float* C, int M, int N, int K, long long sam, long long sak,
               long long sbk, long long sbn, int ldc, float alpha, float beta, const float* bias, hipStream_t st);
int head_normalize_rows_bwd_slabs(const float* xn, const float* inv, const float* dxn, int nslab, long long slab_stride, float* dx, int R, int D,
                                  float beta, hipStream_t st);
int head_sgemm_splitk(const float* A, const float* B, float* C, int M, int N, int K, long long sam, long long sak, long long sbk, long long sbn,
                      int ldc, float alpha, int splits, long long slab_stride, hipStream_t st);
int head_softmax_ce_fused(float* z, const long long* label, int R, int C, int ldz, float s, float m, int arc, float inv_batch, float* prob_t,
                          int nslab, long long slab_stride, float* nll_t, hipStream_t st);
// same, products accumulated in fp64 (fp32 validation path of the backbone)
int head_sgemm_f64acc(const float* A, const float* B, float* C, int M, int N, int K, long long sam, long long sak, long long sbk, long long sbn,
                      int ldc, float alpha, float beta, const float* bias, hipStream_t st);
int head_margin_rowmax(float* z, const long long* label, int R, int C, int ldz, float s, float m, int arc, float* row_max,
                       float* dmul, float* z_t, hipStream_t st);
int head_exp_rowsum(float* z, int R, int C, int ldz, const float* row_max, float* row_sum, hipStream_t st);
int head_softmax_grad(float* z, const long long* label, int R, int C, int ldz, const float* row_sum, const float* dmul, float s,
                      float inv_batch, float* prob_t, const float* row_max, const float* z_t, float* nll_t, hipStream_t st);
int head_margin_bwd(const float* dlogits, const long long* label, const float* dmul, float s, int R, int C, float* dcos,
                    hipStream_t st);
int head_nll_mean(const float* prob_t, int R, float floor_, float* loss, hipStream_t st);
int head_exp_rowsum_target(float* z, const long long* label, int R, int C, int ldz, const float* row_max, float* sums2, hipStream_t st);
int head_nll_mean_ratio(const float* num, const float* den, int R, float floor_, float* loss, hipStream_t st);
int head_bce_logits(const float* cosv, const long long* label, const float* bias, int B, int C, float m, float r, float t,
                    float* z, unsigned char* gt, float* dzdcos, hipStream_t st);
int head_bce_loss(const float* z, const unsigned char* gt, const float* dzdcos, int B, int C, float r, float lam, float loss_scale,
                  float* dz, float* dcos, float* row_loss, hipStream_t st);
int head_colsum_f32(const float* x, int R, int C, float* out, hipStream_t st);
int head_sum_scale(const float* x, int n, float scale, float* out, hipStream_t st);
int head_contrastive(const float* x, const float* g, const float* l, int B, int D, float temperature, float* row_loss, float* dx,
                     hipStream_t st);
int head_sgemm_colflag(const float* A, const float* B, int M, int N, int K, long long sam, long long sak, long long sbk,
                       long long sbn, float alpha, float thr, unsigned char* flags, hipStream_t st);
int head_class_accumulate(const float* x, const long long* label, int B, int D, int C, float* sums, float* counts, hipStream_t st);
// the ROC histogram slot of a pair score s (reference roc_cuda.py:14-30): bin = int((s + 1) * 1000), truncation as int() there, clamped to
// [0, 2000] (the reference would write out of bounds instead); slot 2 * bin counts same-label pairs, 2 * bin + 1 different-label pairs
constexpr int ROC_NBIN = 4002;
__device__ __forceinline__ int roc_slot(double s, bool same) {
  int bin = (int)((s + 1.0) * 1000.0);
  bin = bin < 0 ? 0 : (bin > 2000 ? 2000 : bin);
  return 2 * bin + (same ? 0 : 1);
}
int head_roc_histogram(const float* feat, const long long* label, int N, int D, int T, unsigned long long* hist, hipStream_t st);
// grouped pair histogram (roc_groups.hip): G disjoint target sets in one pass over the unordered pairs; tile_group is HOST memory
int head_roc_histogram_groups(const float* feat, const long long* label, int N, int D, const int* row_index, const int* tile_group,
                              int n_tiles, int G, int* tile_group_dev, unsigned long long* hist, hipStream_t st);
// 1:N identification (ident.hip): positive score per query + exact top-K negatives per column segment
size_t ident_workspace_bytes(int Q, int S, int K);
int ident_topk(const float* query, const long long* qid, int Q, const float* gallery, const long long* gid, int G, int D,
               const long long* seg, int S, int K, double* pos, double* neg_topk, long long* neg_count, void* ws, size_t ws_bytes,
               hipStream_t st);
// IJB-C job 1:N (ident64.hip): fp64 features, one gallery, K up to 4096, positive score + ranks per query
size_t ident_rank_workspace_bytes(int Q, int G, int K);
int ident_rank_topk(const double* query, int Q, const double* gallery, int G, int D, const long long* mask, int K, double* pos,
                    double* neg_topk, long long* neg_count, int* rank_gt, int* rank_eq, void* ws, size_t ws_bytes, int* status,
                    hipStream_t st);
// IJB-C template evaluation (ijbc.hip): template pooling, pair scores fused with the ROC counts at the genuine scores
size_t ijbc_template_pool_workspace_bytes(int N, int norm_images);
int ijbc_template_pool(const float* feats, int N, int D, int flip, const float* face, int norm_images, const int* t_off, int T,
                       const int* m_off, int M, const int* img, int NI, int mode, float* raw, double* out, void* ws, size_t ws_bytes,
                       int* status, hipStream_t st);
size_t ijbc_roc_workspace_bytes(long long P, int G);
int ijbc_pair_scores_roc(const double* feats, int T, int D, const int* lut, long long lut_n, const long long* p1, const long long* p2,
                         long long P, double* score, const long long* label, const double* gv, int G, unsigned long long* counts, void* ws,
                         size_t ws_bytes, int* status, hipStream_t st);
int ijbc_roc_counts(const double* score, const long long* label, long long P, const double* gv, int G, unsigned long long* counts, void* ws,
                    size_t ws_bytes, int* status, hipStream_t st);
// spread-out regulariser of the class centres (spreadout.hip): loss and d(loss)/d(Fn) in one pass, the N x N matrix never written
size_t spreadout_workspace_bytes(int N, int D);
int spreadout_grad(const float* fn, int N, int D, float margin, int mean, float* dfn, float* loss, long long* active, void* ws, size_t ws_bytes,
                   hipStream_t st);
// k-fold 1:1 verification (verif.hip): normalise, pair distances, per-fold threshold histograms and the norm sum in one pass
size_t verif_workspace_bytes(int P, int nfolds);
int verif_fold_counts(const void* emb0, const void* emb1, int fp64_input, int normalize, const unsigned char* issame, int P, int D,
                      int nfolds, const double* thr_a, int Ta, const double* thr_b, int Tb, unsigned long long* counts_a,
                      unsigned long long* counts_b, double* dist, double* norm_sum, int* status, void* ws, size_t ws_bytes, hipStream_t st);
// BottleBlock converter (bottle.hip): four-branch bottleneck MLP with a residual, forward in 2 launches, backward in 2; params / grads are HOST
// arrays of 18 device pointers: br1..br4 x (first weight, first bias, second weight, second bias), then concat_fc weight and bias
size_t bottle_workspace_bytes(int B, int D);
int bottle_forward(const float* x, const float* const* params, int B, int D, float* h1, float* h2, float* y, hipStream_t st);
int bottle_backward(const float* x, const float* const* params, const float* h1, const float* h2, const float* dy, int B, int D, float* dx,
                    float* const* grads, void* ws, size_t ws_bytes, hipStream_t st);
// fused head of train_with_public_data (branch.hip): BCE in one pass, the embedding gradient of all branches in one pass, the whole head as one call
size_t branch_bce_workspace_bytes(int B, int C);
int branch_bce_fused(const float* cosv, const long long* label, const float* bias, int B, int C, float m, float r, float t, float lam,
                     float loss_scale, float* row_loss, float* dcos, float* dbias, void* ws, size_t ws_bytes, hipStream_t st);
int branch_dfeats(const float* xn, const float* inv, const float* dxn, int nslab, long long slab_stride, const float* dbce, const float* dcon,
                  float mu, float* dfeats, int B, int D, hipStream_t st);
size_t branch_workspace_bytes(int B, int D, int C, int n_class, int conv, int detach, int contrastive);
int branch_head(const float* feats, const long long* labels, int B, int D, const float* fc, int C, int arc, float s, float m, int conv,
                const float* const* conv_params, const float* bce_w, const float* bce_b, int n_class, float bce_m, float bce_r, float bce_t,
                float bce_lam, float bce_scale, const float* gfeats, const float* lfeats, float temperature, float mu, int detach, float* losses,
                float* dfeats, float* dfc, float* const* conv_grads, float* dbce_w, float* dbce_b, void* ws, size_t ws_bytes, hipStream_t st);
