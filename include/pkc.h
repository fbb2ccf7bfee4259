/* pkc.h — C ABI of libpkc.so, the MI355X-native (gfx950) hot path of pytorch-kaldi-CGS run_nn().
 *
 * Every entry point replaces an implicit PyTorch-eager op sequence of the reference (file:line
 * cited per function, paths relative to the reference repo).  Conventions:
 *   - plain pointers + sizes, no torch types; all device pointers are caller-owned HBM buffers,
 *     the library never allocates device memory on a hot call;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream;
 *   - return 0 (PKC_OK) or a negative status; pkc_last_error() gives a thread-local message;
 *   - thread-safe across streams (no global mutable state besides the error string).
 * Layouts: row-major matrices, fp32 in HBM ("parity" precision); PKC_PREC_BF16 computes the
 * matmuls on bf16 MFMA with fp32 accumulation ("performance" precision).
 */
#ifndef PKC_H_
#define PKC_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point is added or a struct changes (tests/test_abi_layout.py asserts it):
 * 1: rounds 1-3; 2: pkc_logsoftmax_bwd, and the structs as they stand after round 3 (which appended
 * pkc_dense_bwd_args.dz_scratch without a bump); 3: pkc_opt_seg (direct PKC_OP_OPTIM);
 * 4: PKC_PREC_BF16X3; 5: pkc_rnn_args.step_bf16 and its bf16 operand copies;
 * 6: pkc_bn_bwd_epi, pkc_gemm_bnbwd_ok, pkc_dense_bwd_pre;
 * 7: pkc_src_digest, pkc_gemm_grouped_tile, pkc_rnn_args.persist_* (persistent liGRU time loops);
 * 8: pkc_rnn_args.qh_exact (exact quantised-h step products).
 * pkc_combine_args and its three entry points joined under 9 without a bump: no existing struct or
 * entry point changed (tests/test_model_ops_cpu.py checks the new struct's layout).  pkc_rnn_std_args
 * and pkc_rnn_std_fwd / _bwd joined the same way (tests/test_cudnn_cpu.py checks its layout), and so
 * did pkc_sru_args with pkc_sru_fwd / _bwd / _mask_x / _dx (tests/test_sru_cpu.py) and
 * pkc_lstmp_args with pkc_lstmp_fwd / _bwd (tests/test_lstmp_cpu.py). */
#define PKC_ABI_VERSION 9

enum { PKC_OK = 0, PKC_ERR_ARG = -1, PKC_ERR_HIP = -2, PKC_ERR_IO = -3, PKC_ERR_UNSUPPORTED = -4 };
/* FP32: exact fp32 MFMA (parity); BF16: fp32 operands rounded to bf16 for the MFMA;
 * BF16IN: operands stored as bf16 in HBM (A and B point at bf16 arrays), fp32 accumulation;
 * BF16X3: compensated bf16 — fp32 operands split at staging into a bf16 head and a bf16 tail
 * (a = hi + lo, lo = bf16(a - hi)) and multiplied as hi*hi + hi*lo + lo*hi on the bf16 MFMA with
 * fp32 accumulation: products to ~2^-16 relative (the dropped lo*lo term), i.e. fp32-class
 * results at 3/16 of the exact-fp32 MFMA cost.  Every tile body takes it (64x64 and 128x128,
 * pkc_gemm, pkc_gemm_grouped, pkc_gemm_colstats). */
enum { PKC_PREC_FP32 = 0, PKC_PREC_BF16 = 1, PKC_PREC_BF16IN = 2, PKC_PREC_BF16X3 = 3 };
/* neural_networks.py:54-78 act_fun */
enum { PKC_ACT_LINEAR = 0, PKC_ACT_RELU = 1, PKC_ACT_TANH = 2, PKC_ACT_SIGMOID = 3,
       PKC_ACT_HTANH = 4, PKC_ACT_LEAKY = 5, PKC_ACT_ELU = 6 };
enum { PKC_NORM_NONE = 0, PKC_NORM_BN_TRAIN = 1, PKC_NORM_BN_EVAL = 2 };
enum { PKC_OPT_SGD = 0, PKC_OPT_RMSPROP = 1, PKC_OPT_ADAM = 2 };

int pkc_abi_version(void);
const char* pkc_last_error(void);
/* SHA-256 (hex) of the csrc/ + include/ sources this library was linked from (generated at build
 * time; pkc._lib refuses a library whose digest differs from its tree's). */
const char* pkc_src_digest(void);

/* ---------------------------------------------------------------------------------------------
 * Matmul (replaces the cuBLAS GEMMs behind nn.Linear / F.linear in the reference:
 * neural_networks.py:306-317 (MLP wx), 951-954 (LSTM W), 1554-1555 (liGRU W) and their autograd
 * backward).  Computes, for split z = 0..splits-1 over the K range [z*Kc, (z+1)*Kc):
 *     C[z*slab_stride + m*ldc + n] = sum_k A(m,k) * B(n,k)
 * with A(m,k) = a_kcontig ? A[m*lda+k] : A[k*lda+m] and B(n,k) = b_kcontig ? B[n*ldb+k] : B[k*ldb+n].
 * forward  Y = X W^T      : a_kcontig=1, b_kcontig=1
 * backward dX = dY W      : a_kcontig=1, b_kcontig=0
 * backward dW = dY^T X    : a_kcontig=0, b_kcontig=0
 * Split-K partial slabs are summed by the consumer kernels (dense_fwd/dense_bwd/nll) in a fixed
 * order, so results are deterministic.  splits<=0 picks a split count for the shape.
 * Leading dimensions (elements): lda, ldb in [1, 2^31), ldc in [N, 2^26) — the kernels keep row
 * offsets in 32 bits (PKC_ERR_ARG otherwise; pkc_gemm_grouped checks the same per problem).
 * ------------------------------------------------------------------------------------------- */
int pkc_gemm(int prec, int a_kcontig, int b_kcontig, int M, int N, int K,
             const void* A, int64_t lda, const void* B, int64_t ldb,
             float* C, int64_t ldc, int splits, int64_t slab_stride, void* stream);
int pkc_gemm_pick_splits(int M, int N, int K);
/* Up to 8 independent operations in one launch — the launch boundary (~1.5-1.9 us on MI355X)
 * dominates a 128-row batch's matmuls, so a layer's dW and dX, two heads' logits, or the heads'
 * dW/dX together with their bias gradients and the loss reduction share one kernel.
 *   PKC_OP_GEMM  : exactly pkc_gemm(prec, a_kcontig, b_kcontig, M, N, K, A, lda, B, ldb, C, ldc,
 *                  splits, slab_stride)
 *   PKC_OP_COLSUM: C[n] = sum_m A[m*N + n]  (M rows, N columns, fp32)
 *   PKC_OP_SLABSUM: C[i] = sum_{s<M} A[s*slab_stride + i], i < N, summed in slab order (fp32): the
 *                  partial slabs of a split-K matmul (e.g. a large-batch dW) into one result
 *   PKC_OP_LOSS  : pkc_loss_finalize(nheads = M, row_loss = A, weights = B, rows = N,
 *                  row_err = X1, out = C, acc = X2, advance_ctr = X3)
 *   PKC_OP_OPTIM : pkc_optim_step(tensors_dev = A, chunk_map_dev = B, nchunks = M) — the update of
 *                  a layer whose gradients are complete rides in a later launch of the backward.
 *                  Direct form (X1 != NULL): X1 is a HOST array of N pkc_opt_seg (read during the
 *                  call) listing the op's work items as runs of chunks of single tensors, M = the
 *                  sum of their nchunks.  Their pointers travel in the kernel arguments, so a work
 *                  item's loads start without the map -> descriptor round trips; the
 *                  hyper-parameters (lr, step, ...) are still read from tensors_dev[tensor], so a
 *                  captured graph sees set_lr / step updates.  When a launch's direct segments would
 *                  exceed PKC_OPT_SEGS_MAX the op falls back to the map (B then required).
 *   PKC_OP_GATHER: pkc_batch_gather(feats = A, ld_feats = lda, F = N, labels = B, nlab = ldb,
 *                  B = M rows, n_batches = slab_stride, step_ctr = X1, x_out = C, lab_out = X2,
 *                  advance = 0, x_bf16 = X3) — the next batch's gather sharing a launch with the
 *                  previous step's last weight update (neither reads what the other writes)
 * Block-sparse GEMM (static HCGS masks multiplied into W, HCGS.py:24-28 /
 * neural_networks.py:258, 858-861): with ktiles != NULL (and splits == 1) the 64-column output
 * tile j reads only the 32-deep k-tiles ktiles[j * (kmax + 1) + 1 .. + count], count =
 * ktiles[j * (kmax + 1)]: the k-tiles whose B rows (64 of them) hold a nonzero.  Exact: every
 * skipped product is a zero weight, so the sums are those of the dense matmul. */
enum { PKC_OP_GEMM = 0, PKC_OP_COLSUM = 1, PKC_OP_LOSS = 2, PKC_OP_OPTIM = 3, PKC_OP_SLABSUM = 4,
       PKC_OP_GATHER = 5 };
typedef struct {
  int a_kcontig, b_kcontig, M, N, K, splits;
  const void* A; int64_t lda; const void* B; int64_t ldb;
  float* C; int64_t ldc; int64_t slab_stride;
  int kind; const void* X1; void* X2; void* X3;
  const int32_t* ktiles; int kmax;              /* block-sparse k-tile lists (device), or NULL */
} pkc_gemm_problem;
int pkc_gemm_grouped(int prec, const pkc_gemm_problem* probs, int n, void* stream);
/* The first half of a large-batch BatchNorm'd layer's backward in the epilogue of the dX matmul
 * that produces its output gradient g (neural_networks.py:306-317 under autograd): a PKC_OP_GEMM
 * problem of pkc_gemm_grouped with X1 = a HOST pointer to a pkc_bn_bwd_epi (read during the call)
 * stores dy = g * keep / (1 - drop_p) * act'(gamma * xhat + beta) in C instead of g, and per
 * 128-row block b the column sums sum dy and sum dy * xhat in part[b*2N + n], part[b*2N + N + n]
 * — what pkc_dense_bwd's statistics pass computes, without re-reading g.  The problem must be
 * one slab (splits = 1) with ldc = N and take the 128x128 body: pkc_gemm_bnbwd_ok says whether it
 * does.  pkc_dense_bwd_pre (dz = that C, part in work, part_rows = 128) finishes the backward. */
typedef struct pkc_bn_bwd_epi_s {
  const float* xhat; const uint8_t* keep; const float* gamma; const float* beta;
  float* part; int act; float drop_p;
} pkc_bn_bwd_epi;
int pkc_gemm_bnbwd_ok(int prec, int a_kcontig, int b_kcontig, int M, int N, int K, const void* A,
                      int64_t lda, const void* B, int64_t ldb);
/* Tile edge (128: the 128x128 body, else 64) a GEMM problem of pkc_gemm_grouped takes, so a
 * host can size the launch's split-K over the tiles it will really have. */
int pkc_gemm_grouped_tile(int prec, int a_kcontig, int b_kcontig, int M, int N, int K,
                          const void* A, int64_t lda, const void* B, int64_t ldb);

/* Large-batch forward matmul of a BatchNorm'd layer (neural_networks.py:306-311: BN(wx(x)) over
 * the batch) with the BatchNorm column statistics in the matmul's epilogue: one slab
 * C = A B^T (as pkc_gemm, splits = 1) and, per row block b of C, the block's column mean of
 * C + bias and M2 = sum (C - mean)^2 into part[b*2N + n], part[b*2N + N + n] — the partials
 * pkc_dense_fwd_pre merges, so no separate statistics pass reads C.  pkc_gemm_colstats_ok returns
 * the rows per partial block for the shape — 128 (128x128 tile body), 64 (64x64 body, 16-byte
 * operand paths), 0 (not available) — which is the part_rows to pass to pkc_dense_fwd_pre; bias
 * may be NULL; part holds 2 N ceil(M / rows) floats (a pkc_dense_work_size(M, N) buffer does). */
int pkc_gemm_colstats_ok(int prec, int a_kcontig, int b_kcontig, int M, int N, int K,
                         const void* A, int64_t lda, const void* B, int64_t ldb);
int pkc_gemm_colstats(int prec, int a_kcontig, int b_kcontig, int M, int N, int K,
                      const void* A, int64_t lda, const void* B, int64_t ldb, float* C,
                      int64_t ldc, const float* bias, float* part, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense layer epilogue, forward (neural_networks.py:306-317: drop(act(BN(z)))) where
 * z = sum_{s<nslab} zslab[s] + bias.  BN in training mode uses batch statistics over the M rows
 * (biased variance for normalisation, unbiased for running_var, momentum as nn.BatchNorm1d).
 * Outputs: out (M x N) and, for the backward, xhat (normalised z; == z when norm NONE) and the
 * dropout keep mask (u8; NULL when p == 0).  Dropout is inverted (x*keep/(1-p)) as nn.Dropout.
 * When keep_in != NULL the mask is read instead of generated (parity tests).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int M, N, nslab;
  const float* zslab; int64_t slab_stride;   /* nslab partial slabs, each M x N (ldz = N) */
  const float* bias;                          /* N or NULL */
  int norm;                                   /* PKC_NORM_* */
  const float* gamma; const float* beta;      /* N */
  float* running_mean; float* running_var;    /* N (updated in BN_TRAIN) */
  float momentum, eps;
  float* save_mean; float* save_invstd;       /* N (written in BN_TRAIN, read in backward) */
  int act;                                    /* PKC_ACT_* */
  float drop_p; uint64_t seed; const int64_t* step_ctr; int64_t stream_id;
  const uint8_t* keep_in;                     /* optional injected dropout mask (M x N) */
  uint8_t* keep_out;                          /* M x N, may be NULL when drop_p == 0 */
  float* xhat;                                /* M x N (BN input normalised), may be NULL in eval */
  float* out;        /* M x N; may be NULL when out_bf16 is set (no reader of the fp32 copy) */
  int64_t count_n;   /* rows BatchNorm1d sees for the unbiased running_var (0 -> M); a shared-
                        weight bidirectional layer normalises 2x duplicated rows (2*M) */
  void* out_bf16;    /* optional bf16 copy of out (M x N): the next layer's PKC_PREC_BF16IN operand */
} pkc_dense_fwd_args;
int pkc_dense_fwd(const pkc_dense_fwd_args* a, float* work, void* stream);
/* pkc_dense_fwd in BatchNorm training mode (norm == PKC_NORM_BN_TRAIN, nslab == 1) whose column
 * partials the producing matmul already wrote into work at part_rows rows per block
 * (pkc_gemm_colstats: 128): merges them (Chan, fixed order) and applies — the same outputs with
 * the statistics summed in that blocking. */
int pkc_dense_fwd_pre(const pkc_dense_fwd_args* a, float* work, int part_rows, void* stream);
/* A BatchNorm'd layer's matmul AND epilogue in one launch at M <= 128 rows (the reference's
 * batch_size_train; ABI 9): z = A W^T (A: M x K, lda; W: N x K, ldw; both k-contiguous), then
 * exactly pkc_dense_fwd's epilogue on z + bias (a->zslab / nslab / slab_stride are not read).
 * Each workgroup owns a 128-row x 16-column strip over the full contraction, so the BatchNorm
 * column statistics need nothing from other workgroups.  prec: PKC_PREC_BF16IN (A, W bf16) or
 * PKC_PREC_BF16 (fp32, rounded to bf16 on load: identical results); fp32 accumulation.
 * pkc_dense_gemm_fwd_ok: 1 when the shape / precision / alignment is supported (N % 16 == 0,
 * K % 8 == 0, lda and ldw multiples of 8, A and W 16-byte aligned). */
int pkc_dense_gemm_fwd_ok(int prec, int M, int N, int K, const void* A, int64_t lda, const void* W,
                          int64_t ldw);
int pkc_dense_gemm_fwd(int prec, const void* A, int64_t lda, const void* W, int64_t ldw, int K,
                       const pkc_dense_fwd_args* a, void* stream);
/* floats of device workspace pkc_dense_fwd / pkc_dense_bwd need (per-16-row column partials) */
int64_t pkc_dense_work_size(int M, int N);

/* Dense layer backward through dropout, activation, BN and bias (autograd of the same ops).
 * g = sum_s gslab[s] (dL/d out).  Writes dz (M x N, dL/dz), dgamma, dbeta, dbias (N).  A bias in
 * front of BatchNorm cancels in z - mean(z): its gradient is written as exactly 0 (the reference's
 * autograd value is rounding noise of order 1e-9 with no effect on any output). */
typedef struct {
  int M, N, nslab;
  const float* gslab; int64_t slab_stride;
  int norm, act;
  const float* gamma; const float* beta; const float* save_invstd;
  const float* xhat; const uint8_t* keep; float drop_p;
  float* dz; float* dgamma; float* dbeta; float* dbias;
  void* dz_bf16;     /* optional bf16 copy of dz (M x N): the dW / dX PKC_PREC_BF16IN operand */
  int dz_scratch;    /* 1 (training BatchNorm with dz_bf16): the caller reads only dz_bf16; dz is
                        scratch between the passes and the final fp32 gradient is not stored */
} pkc_dense_bwd_args;
int pkc_dense_bwd(const pkc_dense_bwd_args* a, float* work, void* stream);
/* pkc_dense_bwd after a dX matmul with the pkc_bn_bwd_epi epilogue: a->dz holds dy, work the
 * per-part_rows-block column sums; finalize (dgamma, dbeta) and apply only (BN training). */
int pkc_dense_bwd_pre(const pkc_dense_bwd_args* a, float* work, int part_rows, void* stream);
/* SyncBN (cross-rank BatchNorm statistics): the training-mode BatchNorm of
 * pkc_dense_fwd / pkc_dense_bwd split around a collective the caller runs (sync_bn of the
 * reference recipe; the reference itself has no multi-GPU training).
 *   pkc_dense_fwd_stats: this rank's column state (n, mean, M2) -> state[3N] (floats: N counts,
 *     N means, N M2).  The caller gathers the R ranks' states into states[R][3N] (e.g. an
 *     all-reduce SUM of a zero-filled buffer that rank r writes at row r);
 *   pkc_dense_fwd_sync_apply: merges them in rank order (Chan), writes save_mean / save_invstd /
 *     running statistics (unbiased over the global count) and applies BN / act / dropout to this
 *     rank's rows.
 *   pkc_dense_bwd_stats: this rank's column sums (sum dy, sum dy * xhat) -> sums[2N] and the LOCAL
 *     dgamma / dbeta (the gradient all-reduce sums them); after an all-reduce SUM of sums[2N],
 *   pkc_dense_bwd_sync_apply applies the BatchNorm backward with the global sums over total_rows.
 * work: pkc_dense_work_size(M, N) floats, the same buffer for both halves of a direction. */
int pkc_dense_fwd_stats(const pkc_dense_fwd_args* a, float* work, float* state, void* stream);
int pkc_dense_fwd_sync_apply(const pkc_dense_fwd_args* a, float* work, const float* states,
                             int nranks, void* stream);
int pkc_dense_bwd_stats(const pkc_dense_bwd_args* a, float* work, float* sums, void* stream);
int pkc_dense_bwd_sync_apply(const pkc_dense_bwd_args* a, float* work, const float* sums,
                             int total_rows, void* stream);
/* pkc_dense_fwd_sync_apply for several BatchNorms whose states share ONE gathered buffer (a
 * recurrent layer's G gate BatchNorms: states[R][G][3N], one collective per layer instead of G):
 * `states` points at rank 0's state of THIS BatchNorm and rank r's is rank_stride floats further
 * (rank_stride >= 3N; G * 3N for the gate buffer).  a->count_n > 0 gives the rows BatchNorm1d sees
 * of this rank's M (a shared-weight bidirectional layer normalises 2x duplicated rows: 2 * M); the
 * unbiased running_var correction then runs over the merged GLOBAL count times count_n / M.
 * count_n == 0: the merged count itself, as pkc_dense_fwd_sync_apply. */
int pkc_dense_fwd_sync_apply_packed(const pkc_dense_fwd_args* a, float* work, const float* states,
                                    int nranks, int64_t rank_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused LogSoftmax + NLLLoss(mean) + error rate + d(loss)/d(logits) for one output head
 * (neural_networks.py:73-74 LogSoftmax(dim=1); utils.py:1935-1952 NLLLoss; utils.py:1993-2011
 * cost_err; autograd backward softmax - onehot).  logits = sum_s zslab[s] + bias.
 * labels are int32, in [0, N), read from a strided column: labels[r * label_stride] (the
 * reference stores them as float columns of the chunk, core.py:94, cast with .long() at
 * utils.py:1942; here they arrive as integers).  labels == NULL is the forward mode: no dlogits,
 * row_loss and row_err stay unwritten.  Per-row loss/err go to row_loss / row_err (each optional);
 * row_loss is -log softmax at the label, before the prior; row_err is 1 when the first index of
 * the row's maximum is not the label.  dlogits = weight/M * (softmax - onehot) (NULL: no
 * backward; it needs labels).  logp (M x N) is the head output and is required: the form for
 * wide or many-slab heads stages the logits in it.  log_prior (N) is subtracted from logp when
 * non-NULL (core.py:242-245 posterior normalisation).
 * Forms, chosen by shape and alignment: register-resident for nslab <= 8 and N <= 511 (one wave
 * per row) or 512 <= N <= 2048 (four waves per row), with 16-byte accesses when N % 4 == 0,
 * slab_stride % 4 == 0 (nslab > 1), every fp32 pointer is 16-byte and dlogits_bf16 8-byte
 * aligned, scalar accesses otherwise; one general form per width beyond that.
 * pkc_nll_form (host only, no launch) names the form pkc_nll_fused takes for `a`: 8 * (16-byte
 * accesses) + 4 * (four waves per row) + log2(slab capacity 1, 2, 4, 8) in 0..15 for the
 * register-resident forms, -1 / -2 for the general form with one / four waves per row, -3 for
 * arguments without a shape (M, N <= 0 or nslab < 1).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int M, N, nslab;
  const float* zslab; int64_t slab_stride; const float* bias;
  const int32_t* labels; int64_t label_stride;
  float weight;
  float* logp; const float* log_prior;
  float* dlogits; float* row_loss; float* row_err;
  void* dlogits_bf16;  /* optional bf16 copy of dlogits (operand of the fused row backward) */
} pkc_nll_args;
int pkc_nll_fused(const pkc_nll_args* a, void* stream);
int pkc_nll_form(const pkc_nll_args* a);

/* mse cost (utils.py:2045-2048: torch.mean((y - target) ** 2) over all M x N elements) and its
 * backward in one pass: row_loss[r] = (1/N) sum_j (y[r,j] - target[r,j])^2, so that mean_r row_loss
 * is the cost and pkc_loss_finalize takes it as one more term; dy[r,j] = weight * 2/(M*N) *
 * (y[r,j] - target[r,j]) (dy == NULL: the loss only).  One wave per row and a fixed reduction tree:
 * reruns are bit-identical.  16-byte loads where every pointer and leading dimension allows them,
 * scalar otherwise (a target that is a column range of the batch buffer). */
int pkc_mse_fused(int M, int N, const float* y, int64_t ldy, const float* target, int64_t ldt,
                  float weight, float* dy, int64_t lddy, float* row_loss, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The [model] tensor operations on produced outputs (utils.py:2014-2043): one elementwise launch
 * forward, one backward, for a graph node that combines two row matrices (or one and a constant).
 *   CONCAT      out = [a | b] along the columns (utils.py:2014-2016), N = Na + Nb
 *   SUM         out = a + b                     (utils.py:2025-2026 on tensors)
 *   MULT        out = a * b                     (utils.py:2020-2021)
 *   AVG         out = (a + b) * 0.5f            (utils.py:2040-2041, / 2)
 *   SUM_CONST   out = a + c                     (utils.py:2035-2036)
 *   MULT_CONST  out = a * c                     (utils.py:2030-2031 on a tensor)
 * a is (M x Na, lda), b (M x Nb, ldb); Na == Nb except for CONCAT; the constant forms read c and
 * neither b nor Nb (0 or Na).  Either operand may be a column range of the batch buffer (ld = F,
 * a pointer at any 4-byte offset).  fp32 arithmetic, one rounding per operation as written above,
 * never contracted into an fma.
 * forward: out (M x N, tight), and when out_bf16 is non-NULL the round-to-nearest-even bf16 copy
 *   of the same values (the operand copy the bf16 matmuls read).
 * backward: g = gslab[0] + gslab[1] + ... (nslab slabs of M x N, slab_stride floats apart, summed
 *   left to right in fp32); da (M x Na, tight) and / or db (M x Nb, tight), either NULL for an
 *   operand that takes no gradient (not both; the constant forms take da only):
 *   CONCAT the two column ranges of g; SUM / SUM_CONST g; AVG g * 0.5f; MULT da = g * b,
 *   db = g * a (the only form that reads a / b); MULT_CONST g * c.
 * No atomics and no cross-thread sums: reruns are bit-identical.  16-byte loads and stores when
 * every pointer, leading dimension, slab stride and width (for CONCAT Na too) allows them, the
 * scalar form with identical results otherwise.
 * Refused (PKC_ERR_ARG): unequal widths outside CONCAT, M or a width <= 0, a leading dimension
 * below its width, nslab < 1, both da and db NULL.
 * ------------------------------------------------------------------------------------------- */
enum { PKC_COMBINE_CONCAT = 0, PKC_COMBINE_SUM = 1, PKC_COMBINE_MULT = 2, PKC_COMBINE_AVG = 3,
       PKC_COMBINE_SUM_CONST = 4, PKC_COMBINE_MULT_CONST = 5 };
typedef struct {
  int op, M, Na, Nb;
  const float* a; int64_t lda;
  const float* b; int64_t ldb;
  float c;
  float* out; void* out_bf16;                              /* forward */
  int nslab; const float* gslab; int64_t slab_stride;      /* backward */
  float* da; float* db;
} pkc_combine_args;
/* 1 when the forward (backward != 0: the backward) takes these arguments, else 0 with the reason
 * in pkc_last_error() */
int pkc_combine_ok(const pkc_combine_args* a, int backward);
int pkc_combine_fwd(const pkc_combine_args* a, void* stream);
int pkc_combine_bwd(const pkc_combine_args* a, void* stream);

/* LogSoftmax backward for an upstream gradient dy (M x N, row-major): dz = dy - exp(logp) *
 * rowsum(dy).  The architecture plug-in's trainable head forward (neural_networks.py:73-74 under
 * the reference's autograd, core.py:221-232); dz may alias dy. */
int pkc_logsoftmax_bwd(int M, int N, const float* logp, const float* dy, float* dz, void* stream);

/* Reduce per-row losses of up to 8 heads: loss_final = sum_h w_h * mean(row_loss_h),
 * err = mean(row_err_of_err_head); writes out[0]=loss_final, out[1]=err, out[2+h]=mean loss h and
 * accumulates acc[0]+=loss_final, acc[1]+=err (core.py:251-252 loss_sum/err_sum on device). */
int pkc_loss_finalize(int nheads, const float* const* row_loss, const float* weights, int M,
                      const float* row_err, float* out, float* acc, int64_t* advance_ctr,
                      void* stream);   /* advance_ctr (optional): += 1 after the reduction */
/* Several heads' pkc_nll_fused in one launch (n <= 4). */
int pkc_nll_fused_multi(const pkc_nll_args* args, int n, void* stream);

/* Column sums over rows of sum_s slabs (bias gradient of a head: autograd of + bias). */
int pkc_colsum(int M, int N, int nslab, const float* x, int64_t slab_stride, float* out,
               int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-tensor optimizer step (torch.optim SGD / RMSprop / Adam as built by utils.py:1833-1881,
 * stepped at core.py:230-232) fused with the reference's per-forward weight preparation:
 * p <- clamp(p_new * mask, -clampv, clampv) when mask / clampv>0 are given — the in-place HCGS /
 * pattern multiply (neural_networks.py:258, 858-861, 980-983) and the in-place QuantizeLinear
 * clamp (quantized_modules.py:79) that the next forward would otherwise apply.
 * ------------------------------------------------------------------------------------------- */
typedef struct pkc_opt_tensor_s {
  float* p; const float* g; float* s1; float* s2; float* s3; const float* mask;
  int64_t n;
  int kind;            /* PKC_OPT_* */
  float lr, wd, momentum, dampening, alpha, eps, beta1, beta2, clampv;
  int nesterov, centered, amsgrad, step;   /* step = 1-based count for this tensor */
  float* qout; int qbits;   /* QuantizeLinear: also write the fake-quantised weight (qbits > 0) */
  void* bout;               /* optional bf16 copy of the updated parameter (MFMA operand) */
} pkc_opt_tensor;
int pkc_optim_step(const pkc_opt_tensor* tensors_dev, int ntensors, const int32_t* chunk_map_dev,
                   int nchunks, void* stream);
/* One run of work items of a direct PKC_OP_OPTIM operation (pkc_gemm_grouped): chunks
 * [chunk0, chunk0 + nchunks) (pkc_optim_chunks' 2048-element items) of tensor `tensor` of the
 * descriptor array.  p .. bout and n repeat that descriptor's, except that s1 / s2 / s3 / qout are
 * NULL where the update keeps no such state (SGD without momentum: s1 NULL; qout NULL unless
 * qbits > 0): the kernel decides which streams to touch from these pointers alone. */
#define PKC_OPT_SEGS_MAX 8     /* direct segments per grouped launch */
typedef struct pkc_opt_seg_s {
  int tensor, chunk0, nchunks, reserved;
  float* p; const float* g; float* s1; float* s2; float* s3; const float* mask;
  float* qout; void* bout;
  int64_t n;
} pkc_opt_seg;
/* Host helper: size of the chunk map (pairs tensor,start) for pkc_optim_step. */
int pkc_optim_chunks(const int64_t* sizes, int ntensors, int32_t* map_out, int cap);

/* p <- clamp(p * mask) (mask may be NULL, clampv <= 0 disables the clamp). */
int pkc_apply_mask(float* p, const float* mask, int64_t n, float clampv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batch assembly for non-sequential models (core.py:203-205: inp = data_set[b:b+B]):
 * copy rows [i*B, (i+1)*B) of the chunk's feature matrix and label columns into static buffers,
 * with i read from a device counter (so the step can be replayed from a hipGraph); the counter
 * is incremented by the last block when `advance` is set (otherwise by the step's loss
 * reduction, pkc_loss_finalize's advance_ctr).
 * ------------------------------------------------------------------------------------------- */
int pkc_batch_gather(const float* feats, int64_t ld_feats, int F, const int32_t* labels, int nlab,
                     int B, int64_t n_batches, int64_t* step_ctr, float* x_out, int32_t* lab_out,
                     int advance, void* x_bf16, void* stream);   /* x_bf16: optional bf16 copy */

/* ---------------------------------------------------------------------------------------------
 * LayerNorm of the reference (neural_networks.py:40-51, used by MLP dnn_use_laynorm /
 * dnn_use_laynorm_inp): y = gamma * (x - mean) / (std + eps) + beta per row over N features,
 * std unbiased, x = sum_s xslab[s] + bias.  Saves xhat = (x - mean)/(std + eps) and
 * rowstat[2r] = std + eps, rowstat[2r+1] = std for the backward.
 * ------------------------------------------------------------------------------------------- */
int pkc_layernorm_fwd(int M, int N, int nslab, const float* xslab, int64_t slab_stride,
                      const float* bias, const float* gamma, const float* beta, float eps,
                      float* y, float* xhat, float* rowstat, void* stream);
/* dx from dy = sum_s dy[s] (split-K slabs of the consumers' dX); dgamma = sum_rows dy*xhat,
 * dbeta = sum_rows dy, dbias = sum_rows dx (each optional) */
int pkc_layernorm_bwd(int M, int N, int nslab, const float* dy, int64_t slab_stride,
                      const float* xhat, const float* gamma,
                      const float* rowstat, float* dx, float* dgamma, float* dbeta, float* dbias,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Magnitude pruning (quantized_modules.py:15-28): thr = np.percentile(|W|, perc) (numpy 'linear'),
 * W *= (|W| > thr) in place; mask (optional) receives the {0,1} mask.  Exact order statistics by
 * GPU radix select, no host round trip.  work: pkc_prune_work_size() bytes of device memory.
 * ------------------------------------------------------------------------------------------- */
int64_t pkc_prune_work_size(void);
int pkc_prune(float* w, int64_t n, double perc, float* mask, void* work, void* stream);

/* ---------------------------------------------------------------------------------------------
 * [model] regularisers cost_l1 / cost_l2 / cost_gl (utils.py:24-60, 1954-1991): the loss term
 * lam * sum of block norms (l1: |.|_1 per parameter; l2: |.|_2 per parameter; gl: |.|_2 per
 * torch.chunk block) and its gradient.  A block is cut into row-slice items; items of one block are
 * contiguous and block_start[b]..block_start[b+1] indexes them.
 *   pkc_reg_partial : partial[i] = sum |x| (L1) or sum x^2 (L2) over item i
 *   pkc_reg_finalize: coef[b] = lam (L1) or lam / ||block b|| (L2, 0 for a zero block);
 *                     loss_rows[0..nrows) = lam * sum_b ||block b||  (a pseudo loss head)
 *   pkc_reg_grad    : g += coef[block] * sign(x) (L1) or coef[block] * x (L2), items with g set
 *                     (g = ... for items with assign set)
 * ------------------------------------------------------------------------------------------- */
enum { PKC_REG_L1 = 1, PKC_REG_L2 = 2 };
typedef struct pkc_reg_item_s {
  const float* p;     /* parameter (row-major, leading dimension ld) */
  float* g;           /* its gradient buffer (NULL: loss term only) */
  int64_t ld;
  int r0, r1, c0, c1; /* the item's rectangle */
  int block;          /* block index */
  int assign;         /* 1: g = term gradient (a parameter only the term trains); 0: g += */
} pkc_reg_item;
int pkc_reg_partial(int kind, const pkc_reg_item* items_dev, int nitems, float* partial,
                    void* stream);
int pkc_reg_finalize(int kind, const int32_t* block_start_dev, int nblocks, const float* partial,
                     float lam, float* coef, float* loss_rows, int nrows, void* stream);
int pkc_reg_grad(int kind, const pkc_reg_item* items_dev, int nitems, const float* coef,
                 void* stream);

/* dst (bf16) = src (fp32), n elements (bf16 operand copies for the MFMA matmuls) */
int pkc_cast_bf16(const float* src, void* dst, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Chunk preparation on the GPU (data_io.py:105-145 context_window + load_chunk normalisation,
 * data_io.py:269-270 frame shuffle as a row permutation):
 *   cw_stats : column mean / population std (fp64) of the context-expanded chunk;
 *   cw_apply : out[r] = (expand(raw)[perm[r]] - mean) / std as fp32, labels shifted by -lab_min.
 * raw is N x D (length-sorted concatenated utterances); expanded row r (0 <= r < N-L-R), block b
 * (0..L+R) holds raw[(r + 2L - b) mod N] (np.roll order, future frame first).
 * ------------------------------------------------------------------------------------------- */
int pkc_cw_stats(const float* raw, int64_t N, int D, int L, int R, double* mean, double* std,
                 double* work, void* stream);
int64_t pkc_cw_stats_work_size(int64_t N, int D, int L, int R);
int pkc_cw_apply(const float* raw, int64_t N, int D, int L, int R, const double* mean,
                 const double* std, const int64_t* perm, float* out, int64_t ld_out, void* stream);
/* One feature stream of a multi-stream chunk (data_io.py:184-263, ABI 9): expanded rows
 * row0 + perm[j] (row0 + j without perm), j < nrows, of this stream's own expansion and statistics
 * — the rows the reference keeps after trimming every stream to the widest context window
 * (row0 = cw_left_max - L, nrows = N - cw_left_max - cw_right_max) — written to out (the stream's
 * first column in the chunk matrix) with row stride ld_out (the chunk's width). */
int pkc_cw_apply_rows(const float* raw, int64_t N, int D, int L, int R, const double* mean,
                      const double* std, const int64_t* perm, int64_t row0, int64_t nrows,
                      float* out, int64_t ld_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kaldi feature front-end (replaces the `apply-cmvn ... | add-deltas ...` stages of the fea_opts
 * pipe that data_io.py:18 runs through read_mat_ark, data_io.py:645-664; Kaldi's ApplyCmvn and
 * DeltaFeatures restated).  raw: Nsrc x D frames of whole utterances; output row r (of Nout, in
 * the sorted / split load_dataset order) is source frame src_row[r] of utterance u = utt_of_row[r],
 * whose frames are [utt_beg[u], utt_end[u]) of raw.  cmvn_mode 0 none, 1 means (x + offset),
 * 2 means+vars (x * scale + offset); norm[utt_norm[u]] = {offset[D], scale[D]} (fp32, computed by
 * the host as ApplyCmvn does in double).  scales: (order+1) x (2*maxoff+1) delta windows (zero
 * outside each order's own window); frames clamp to the utterance.  out: Nout x D*(order+1).
 * order <= 7.
 * ------------------------------------------------------------------------------------------- */
int pkc_feat_frontend(const float* raw, int D, int64_t Nout, const int32_t* src_row,
                      const int32_t* utt_of_row, const int32_t* utt_beg, const int32_t* utt_end,
                      const int32_t* utt_norm, const float* norm, int cmvn_mode,
                      const float* scales, int order, int maxoff, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Raw-waveform framing (the `pkc-wav-frames` fea_opts stage; save_raw_fea.py:73-104 restated, an
 * entry point added under ABI 9 without a struct change).  samples: the int16 audio of whole
 * utterances; utterance u is samples[utt_beg[u] .. utt_beg[u] + utt_len[u]) with peak
 * utt_peak[u] = max|s| in 1..32768.  Output row r (of Nout, any order) is frame
 * f = frame_of_row[r] of utterance u = utt_of_row[r]: with S = lab_wshift, Lw = lab_wlen (samples)
 *   c = (2*f*S + Lw - 2) / 2,  b = c - W/2,
 *   out[r][j] = 0 <= b + j < len_u ? (float)((double)s_u[b + j] / (double)peak_u) : 0.0f.
 * sig_work: one float per sample of `samples` (the normalised signal, written by the first of the
 * two launches: row r normalises the samples of its own frame — [f*S, (f+1)*S), to the end of the
 * utterance for its last frame — so the row maps must name every frame of each utterance they
 * name, as the loader's and the writer's do; frames are those with f*S + Lw < len_u).
 * out: Nout x W; rows are written as 16-byte stores when W % 4 == 0.  W even and > 0, Lw >= 2,
 * S >= 1; Nout == 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
int pkc_wav_frames(const int16_t* samples, const int64_t* utt_beg, const int32_t* utt_len,
                   const int32_t* utt_peak, const int32_t* utt_of_row, const int32_t* frame_of_row,
                   int64_t Nout, int W, int lab_wlen, int lab_wshift, float* sig_work, float* out,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * Recurrent layers: the per-time-step loops of liGRU (neural_networks.py:1573-1584), LSTM
 * (neural_networks.py:1077-1097), GRU (:1390-1396, gates z, r, h), minimalGRU (:1751-1755, gates
 * z, h) and RNN (:1905-1907, gate h).  wpre holds the gate pre-activations W x (+BN) for the T*B input
 * rows, gate-major (G, T, B, H): liGRU gates (z, h), LSTM gates (f, i, o, c).  Bidirectional
 * layers (liGRU's shared-weight cat/flip convention, :1536-1538) run 2B rows per step; rows >= B
 * read time T-1-t and write the second half of the (T, B, 2H) output y.  Forward saves
 * hs (T+1, B2, H) [hs[0] = 0], cs (LSTM, T+1, B2, H) and gate activations (G, T, B2, H) for BPTT.
 * Dropout: bernoulli(1-p) mask per (row, unit), shared by all steps and NOT rescaled; (1-p) at eval.
 * pkc_rnn_bwd: dy = dL/dy (layer output layout); writes dgates (G, T, B2, H) = dL/d pre-activation
 * per direction and dpre (G, T, B, H) = the same folded over directions (input of the BN / W
 * backward); work = 8*B2*H floats (carries + per-gate partial products).
 * ------------------------------------------------------------------------------------------- */
enum { PKC_CELL_LIGRU = 0, PKC_CELL_LSTM = 1, PKC_CELL_GRU = 2, PKC_CELL_MINGRU = 3, PKC_CELL_RNN = 4 };
typedef struct {
  int cell, T, B, H, bidir, act, train;
  const float* wpre;
  const float* U[4];
  float drop_p; uint64_t seed; const int64_t* step_ctr; int64_t stream_id;
  const float* drop_mask_in;   /* optional injected (B2, H) mask */
  float* drop_mask;            /* (B2, H) mask in use */
  float* hs; float* cs; float* gates; float* y;
  const float* dy; int dy_nslab; int64_t dy_slab_stride;   /* dL/dy as split-K partial slabs */
  float* dgates; float* work;
  /* QuantizeLinear U layers with input quantisation (quantized_modules.py:99-119): h_{t-1} is
   * re-quantised once per gate (q1..q4, per-tensor max-abs) before each U product; U[] then points
   * at the fake-quantised weights.  hq (T+1, B2, H) receives q4(h_{t-1}) — the value the reference
   * keeps as hiddens[t-1] and as the saved input of the U backward. qbits = 0: off. */
  int qbits; float* hq;
  /* GRU / minimalGRU: r*h_{t-1} (z*h_{t-1}) per step, (T, B2, H) — the input of the Uh product
   * and of its gradient matmul.  NULL for the other cells. */
  float* rh;
  /* pkc_rnn_bwd: G x H x H scratch for the transposed U (the B operand of the BPTT products) */
  float* ut;
  /* LayerNorm of h after every step (use_laynorm; neural_networks.py:40-51 applied at :1093-1094,
   * :1581-1582 ...): gamma / beta (H), NULL = off; xhat (T, B2, H) and stat (T, B2, 2) saved by the
   * forward; g (T, B2, H) the post-norm gradients, dgamma / dbeta (H) written by the backward. */
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  float* ln_xhat; float* ln_stat; float* ln_g; float* ln_dgamma; float* ln_dbeta;
  /* Block-sparse U (static HCGS masks, HCGS.py:24-28; every cell, no quantised h; the RNN with
   * fp32 step products only): per workgroup tile, the indices of the 16-wide contraction blocks
   * holding a nonzero of the mask (-1 = empty slot: never read, a tile whose row is all -1 gives a
   * zero product), kmap_s* slots per tile (16, 32 or 64; 16 lane groups x kmap_s/16 blocks).
   *   kmap_fwd, one-phase cells (liGRU, LSTM, RNN) [ceil(H / (16/G))][kmap_s_fwd]: blocks of k
   *     (h_{t-1} / U columns) that the forward tile of 16/G units x G gates reads;
   *   kmap_fwd, two-phase cells (GRU, minimalGRU; NG = G - 1 gates read h_{t-1}): ONE allocation,
   *     first the phase-0 table [ceil(H / (16/NG))][kmap_s_fwd] (tiles of 16/NG units x NG gates),
   *     then the phase-1 table [ceil(H/16)][kmap_s_fwd] (tiles of 16 units of the candidate gate's
   *     U, whose contraction runs over r*h / z*h), both with the same kmap_s_fwd;
   *   kmap_bwd [G][ceil(H/16)][kmap_s_bwd]: blocks of j (U rows) that the BPTT tile of 16 columns k
   *     of gate g reads (two-phase cells: the candidate gate's table serves its d(r*h) product).
   * NULL: dense contraction over all H. */
  const int32_t* kmap_fwd; const int32_t* kmap_bwd; int kmap_s_fwd, kmap_s_bwd;
  /* bf16 step products (the performance mode of the sequence configs; liGRU / LSTM / RNN, dense U,
   * no quantised h, no LayerNorm): step_bf16 = 1 runs U h_{t-1} and the BPTT products dgates U^T on
   * v_mfma_f32_16x16x32_bf16 with fp32 accumulation, reading bf16 copies of their operands:
   *   hs_h (T+1, B2, H) bf16 copy of hs, written by the forward steps (hs_h[0] = 0);
   *   U_h[g] (H x H) bf16 copies of U[g] (the caller keeps them current);
   *   ut_h (G x H x H) bf16 U^T, written by pkc_rnn_bwd's transpose;
   *   dgates_h (G, T, B2, H) bf16 copy of dgates, written by the backward steps.
   * Cell state, gates, h and every other quantity stay fp32.  0: exact-fp32 products. */
  int step_bf16;
  void* hs_h; const void* U_h[4]; void* ut_h; void* dgates_h;
  /* Persistent time loops (liGRU with bf16 step products and a block-sparse U, H <= 576): the
   * whole forward (and BPTT) time loop of a layer in ONE launch of ceil(B2 / rows_per_wg)
   * workgroups, each owning its batch rows for all T steps with the layer's nonzero U (U^T)
   * blocks held in registers and LDS as MFMA operands and h_{t-1} (dgates_t) in LDS — no per-step
   * launch, no cross-workgroup hand-off (rows are independent).  persist_fwd / persist_bwd:
   * [nwaves][nslots] int32 fragment plans (pkc_rnn_persist_geometry): bits 0-7 the output tile
   * (16 units; BPTT: 16 columns k), 8-15 the 32-wide contraction block + 1 (0 = none), bit 16 the
   * last fragment of this wave's part of the tile, bit 17 valid, bit 18 set on that flush when
   * the part is the second of a tile cut between two waves, bits 19-21 its spill-over tile index
   * (distinct per cut tile, < nwaves - 1).  persist_kb = the forward plan's nslots.
   * NULL (or a layer outside these limits): the per-step launches. */
  const int32_t* persist_fwd; const int32_t* persist_bwd; int persist_kb;
  /* Exact quantised-h step products (qbits > 0, step_bf16 = 0): the caller guarantees U[g] lies on
   * a weight grid of <= 8 bits (m / 2^(b-1), |m| <= 2^(b-1): exact in bf16) and passes its bf16
   * copies in U_h[g].  The forward step then writes the grid integers k of q_g (|k| <= 2^(qbits-1))
   * as two exact bf16 parts and evaluates U q_g = var 2^-(qbits-1) U k on the bf16 MFMA with fp32
   * accumulation (exact integer sums up to H = 512): the fp32 products to within their own
   * rounding.  Each step leaves its per-wave max|h| partials in work (two slots by step parity,
   * at most 2 x H floats; work's 8 x B2 x H hold them) for the next step's var.
   * 0: the exact-fp32 chain. */
  int qh_exact;
} pkc_rnn_args;
int pkc_fakequant_weight(const float* w, float* q, int64_t n, int bits, void* stream);
/* out = q1..q_reps (reps consecutive n-float tensors) of the in-place input quantisation that
 * `reps` successive QuantizeLinear calls apply to one tensor; work >= 136 floats. */
int pkc_fakequant_input(const float* x, float* out, int64_t n, int bits, int reps, float* work,
                        void* stream);
/* Pattern mask (sparsity.py:1112-1146) of W (rows x cols, multiples of ph x pw) for P <= 32
 * patterns (P x ph x pw, {0,1}); ties select every maximal pattern (mask values can exceed 1). */
int pkc_pattern_mask(const float* W, int rows, int cols, const float* patterns, int P, int ph,
                     int pw, float* mask, void* stream);
/* Sequence batch assembly (core.py:183-214): sentence k of the batch starts at chunk row beg[k],
 * has len[k] frames and is placed at time offset left[k] (python random.randint(0, max_len-len),
 * drawn on the host in the reference's order); the rest of the (max_len, B, F) input is zero and
 * the labels of padded frames are 0 (they count in the loss, as in the reference). */
int pkc_seq_gather(const float* feats, int64_t ld_feats, int F, const int32_t* labels, int nlab,
                   const int64_t* beg, const int32_t* len, const int32_t* left, int B, int max_len,
                   float* x_out, int32_t* lab_out, void* stream);
/* Geometry of the persistent liGRU loops' plan tables (pkc_rnn_args.persist_*): waves per
 * workgroup, fragment slots per wave of the forward plan (= persist_kb) and of the BPTT plan,
 * batch rows per workgroup, largest H. */
int pkc_rnn_persist_geometry(int* nwaves, int* nslots_fwd, int* nslots_bwd, int* rows_per_wg,
                             int* hmax);
/* Which time-loop form pkc_rnn_fwd (bwd = 0) / pkc_rnn_bwd (bwd = 1) takes for these arguments:
 * 1 the persistent liGRU loops (persist_* plans above); 2 the persistent grid-synchronised loops —
 * qh_exact LSTM (uni-directional, B <= 16; forward H in {512, 768, 1024}, BPTT H = 512), dense LSTM
 * in bf16 or exact-fp32 step mode (B2 <= 32, H in {512, 768, 1024}; fp32: no quantised h, the
 * grid of H / 16 x ceil(B2 / 16) (BPTT: ceil(B2 / 8)) workgroups within the device's compute
 * units) and liGRU in exact-fp32 step mode (B2 <= 16, H <= 768): the layer's units dealt to H / 16
 * (liGRU forward: H / 8) workgroups that hand h_t / dgates_t to each other every step; work's
 * 288 floats [4 B2 H, 4 B2 H + 288) hold the launch's counter block (a timeout word at
 * 4 B2 H + 1 and eight step-counter shards on 128-byte lines of their own), which lies inside the
 * 8 B2 H floats of work, so form 2 needs 4 B2 H >= 288; 0 one launch per time step.
 * Environment: PKC_RNN_LSTM_PERSIST=0 and PKC_RNN_LIGRU_GRID=0 disable form 2 for LSTM / liGRU,
 * PKC_RNN_LSTM_F32=0 for the exact-fp32 LSTM alone. */
int pkc_rnn_persist_form(const pkc_rnn_args* a, int bwd);
int pkc_rnn_fwd(const pkc_rnn_args* a, void* stream);
int pkc_rnn_bwd(const pkc_rnn_args* a, float* dpre, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Standard-cell recurrent layers: the time loops of LSTM_cudnn, GRU_cudnn and RNN_cudnn
 * (neural_networks.py:364-465: torch.nn.LSTM / GRU / RNN).  Additive to ABI 9: a new struct and new
 * entry points only.  One layer, both directions; direction d (1: reverse, walks time T-1 .. 0) has
 * its own operands and is a grid dimension of every step launch.
 *   wpre[d] (T, B, G*H), rows in natural time: the packed input projection weight_ih x + bias_ih;
 *   U[d]    (G*H, H): weight_hh as torch packs it, gate rows i,f,g,o (LSTM), r,z,n (GRU);
 *   bhh[d]  (G*H): bias_hh, or NULL (bias = False).  The step adds it to the recurrent product.
 * Cells (a = wpre, u = U h_{t-1} + bhh):
 *   LSTM  i,f,o = sig(a + u), g = tanh(a_g + u_g), c = f c_{t-1} + i g, h = o tanh(c)
 *   GRU   r,z = sig(a + u), n = tanh(a_n + r u_n), h = (1 - z) n + z h_{t-1}
 *         (torch's cell: the reset gate multiplies AFTER the recurrent product, and b_hn is inside
 *         it — so b_hn can not be folded into the projection: its gradient is sum r da_n)
 *   RNN   h = act(a + u), act = PKC_ACT_TANH or PKC_ACT_RELU
 * Forward: one launch per time step.  Saves hs (ndir, T+1, B, H) — direction 0 keeps the state
 * after time t in slot t+1 (slot 0 = the zero initial state), direction 1 in slot t (slot T = 0), so
 * that h_{t-1} of the T steps are T consecutive slots in natural time —, cs (LSTM, same layout),
 * the gate activations gates (ndir, T, B, G*H), un (GRU: u_n, (ndir, T, B, H)) and writes the layer
 * output y (T, B, ndir*H).  Inter-layer dropout (train != 0 and drop_p > 0; the caller passes
 * drop_p = 0 for the last layer): y = h keep / (1 - p) with keep ~ Bernoulli(1 - p) per element of
 * y, drawn from the counter-hash stream of pkc_dense_fwd (index = the element's flat index in y) or
 * read from keep_in; keep (u8, the layout of y) is written for the backward.  hs stays undropped.
 * Backward (pkc_rnn_std_bwd): dy = dL/dy as dy_nslab partial slabs; writes dgates
 * (ndir, T, B, GD*H), rows in natural time, the gradients of the pre-activations: GD = G slabs in
 * gate order, except the GRU's GD = 4 slabs [r, z, n_rec, n_in] with n_in = da_n (input side: dW_in,
 * db_in, dx) and n_rec = r da_n (recurrent side: dU_n, db_hn).  So per direction
 *   d weight_ih = dA^T x, d bias_ih = colsum dA, dx += dA weight_ih    (dA: the G input-side slabs)
 *   d weight_hh = dR^T h_{t-1}, d bias_hh = colsum dR                  (dR: the G recurrent-side slabs;
 *   LSTM / RNN: dR = dA), all plain matmuls over the T*B rows.  ut: (ndir, H, G*H) floats of scratch
 *   (the transposed weight_hh), work: (ndir, 2, B, H) floats (carries).
 * No atomics: reruns are bit-identical, and a bidirectional call equals two one-direction calls.
 * H <= 2048; PKC_ERR_ARG with a pkc_last_error() text for a null pointer or a bad shape.
 * ------------------------------------------------------------------------------------------- */
enum { PKC_STD_LSTM = 0, PKC_STD_GRU = 1, PKC_STD_RNN = 2 };
typedef struct {
  int cell, T, B, H, ndir, act, train;
  const float* wpre[2];
  const float* U[2];
  const float* bhh[2];
  float* hs; float* cs; float* gates; float* un; float* y;
  float drop_p; uint64_t seed; const int64_t* step_ctr; int64_t stream_id;
  const uint8_t* keep_in;      /* optional injected keep mask (T, B, ndir*H) */
  uint8_t* keep;               /* (T, B, ndir*H) mask in use */
  const float* dy; int dy_nslab; int64_t dy_slab_stride;
  float* dgates; float* ut; float* work;
} pkc_rnn_std_args;
int pkc_rnn_std_fwd(const pkc_rnn_std_args* a, void* stream);
int pkc_rnn_std_bwd(const pkc_rnn_std_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Projected LSTM (LSTMP; Sak et al., Interspeech 2014): the time loops of LSTM_cudnn with
 * proj_size = P, i.e. torch.nn.LSTM(..., proj_size=P), 0 < P < H, zero initial state.  Additive to
 * ABI 9: a new struct and new entry points only (pkc_rnn_std_args is untouched).  One layer, both
 * directions; direction d (1: reverse, walks time T-1 .. 0) has its own operands and is a grid
 * dimension of every step launch.
 *   wpre[d] (T, B, 4H), rows in natural time: the packed input projection weight_ih x + bias_ih;
 *   U[d]    (4H, P): weight_hh as torch packs it, gate rows i,f,g,o;
 *   bhh[d]  (4H): bias_hh, or NULL (bias = False).  The step adds it to the recurrent product;
 *   Whr[d]  (P, H): weight_hr, the recurrent projection (no bias).
 * Cell (a = wpre, u = U h_{t-1} + bhh):
 *   i,f,o = sig(a + u), g = tanh(a_g + u_g), c = f c_{t-1} + i g, ht = o tanh(c)   (H wide)
 *   h = Whr ht                                                                      (P wide)
 * h is both the layer output and the recurrent state.  U Whr is never folded into one matrix.
 * Forward: two dependent launches per time step (the cell update, skipping the product at step
 * 0; the projection).  Saves hs (ndir, T+1, B, P) and cs (ndir, T+1, B, H) in the slot layout of
 * pkc_rnn_std_args — direction 0 keeps the state after time t in slot t+1 (slot 0 = the zero
 * initial state), direction 1 in slot t (slot T = 0), so that h_{t-1} of the T steps are T
 * consecutive slots in natural time —, the gate activations gates (ndir, T, B, 4H), the
 * unprojected ht (ndir, T, B, H) that the weight_hr gradient contracts with, and writes the layer
 * output y (T, B, ndir*P).  Inter-layer dropout (train != 0 and drop_p > 0; the caller passes
 * drop_p = 0 for the last layer): y = h keep / (1 - p) with keep ~ Bernoulli(1 - p) per element of
 * y, drawn from the counter-hash stream of pkc_dense_fwd (index = the element's flat index in y) or
 * read from keep_in; keep (u8, the layout of y) is written for the backward.  hs stays undropped.
 * Backward (pkc_lstmp_bwd): dy = dL/dy as dy_nslab partial slabs.  U and Whr are transposed once
 * per call, then two dependent launches per step, last step first:
 *   dhp_t = (sum of the dy slabs) keep / (1 - p) + dgates_{next step} U      (over 4H; not at the
 *           first BPTT step), the total gradient arriving at h_t: dhp (ndir, T, B, P), natural time;
 *   dht_t = dhp_t Whr (over P), then the LSTM gate gradients with the dc f carry: dgates
 *           (ndir, T, B, 4H), natural time, the gradients of the pre-activations.
 * So per direction, all plain matmuls over the T*B rows:
 *   d weight_ih = dgates^T x, d bias_ih = d bias_hh = colsum dgates, dx += dgates weight_ih,
 *   d weight_hh = dgates^T h_{t-1} (4H x P), d weight_hr = dhp^T ht (P x H).
 * Caller-provided scratch: ut (ndir, P, 4H) floats (the transposed weight_hh), wt (ndir, H, P)
 * floats (the transposed weight_hr), work (ndir, B, H) floats (the dc f carries).
 * No atomics: reruns are bit-identical, and a bidirectional call equals two one-direction calls.
 * PKC_ERR_ARG with a pkc_last_error() text for a null pointer, P <= 0, P >= H, H > 2048, ndir not
 * 1 or 2, or drop_p outside [0, 1).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int T, B, H, P, ndir, train;
  const float* wpre[2];
  const float* U[2];
  const float* bhh[2];
  const float* Whr[2];
  float* hs; float* cs; float* gates; float* ht; float* y;
  float drop_p; uint64_t seed; const int64_t* step_ctr; int64_t stream_id;
  const uint8_t* keep_in;      /* optional injected keep mask (T, B, ndir*P) */
  uint8_t* keep;               /* (T, B, ndir*P) mask in use */
  const float* dy; int dy_nslab; int64_t dy_slab_stride;
  float* dgates; float* dhp; float* ut; float* wt; float* work;
} pkc_lstmp_args;
int pkc_lstmp_fwd(const pkc_lstmp_args* a, void* stream);
int pkc_lstmp_bwd(const pkc_lstmp_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Simple Recurrent Unit (Lei et al., EMNLP 2018, the v2 cell with the highway scaling alpha): the
 * time loop of one layer, both directions, as ONE launch.  A pkc extension: the reference keeps its
 * SRU class commented out, so nothing here is pinned against it.  Additive to ABI 9: a new
 * struct and new entry points only.  n_out = ndir * d; column j belongs to direction j / d, and
 * direction 1 walks t = T-1 .. 0.  k = 4 when the skip term is on and n_in != n_out, else 3.
 *   u        (T, B, n_out*k), rows in natural time: the projection X weight, gate g of column j at
 *            j*k + g (k = 4: 16-byte aligned, one 16-byte load per thread);
 *   x, ldx   k = 3 with the skip term: the layer's (undropped) input rows, (T*B) rows of ldx >= n_out
 *            floats whose first n_in = n_out columns are read; else unused;
 *   weight_c (2 n_out) = [v_f | v_r], bias (2 n_out) = [b_f | b_r].
 * Forward (c_{-1} = 0; pads are ordinary rows):
 *   f = sig(u1 + v_f c_{t-1} + b_f), r = sig(u2 + v_r c_{t-1} + b_r), c = f c_{t-1} + (1 - f) u0,
 *   x' = u3 (k = 4) | alpha x (k = 3, skip != 0) | 0 (skip == 0),
 *   h = r g(c) m_c + (1 - r) x',   g = act: PKC_ACT_LINEAR, PKC_ACT_RELU or PKC_ACT_TANH.
 * Saves cs (T, B, n_out) = c and writes y (T, B, n_out) = h.  m_c[b, j] = keep / (1 - drop_p) in
 * training with drop_p > 0, else 1: ONE mask for all t, keep ~ Bernoulli(1 - drop_p) drawn from the
 * counter-hash stream of pkc_dense_fwd (index b * n_out + j) or read from keep_in; keep (u8,
 * (B, n_out)) is written for the backward.
 * Backward (pkc_sru_bwd; carry dc from 0, dh = the sum of the dy_nslab slabs of dy):
 *   dr = dh (g(c) m_c - x'), dx' = dh (1 - r), dc += dh r m_c g'(c),
 *   du0 = dc (1 - f), du1 = da_f = dc (c_{t-1} - u0) f (1 - f), du2 = da_r = dr r (1 - r),
 *   du3 = dx' (k = 4); k = 3 with skip: dxh[t, b, j] = alpha dx';  dc <- dc f + da_f v_f + da_r v_r.
 * Writes du (the layout of u), dxh (T, B, n_out), dwc = [sum da_f c_{t-1} | sum da_r c_{t-1}] and
 * dbias = [sum da_f | sum da_r]: summed over T in registers, the per-sentence sums stored in work
 * ((B, 4, n_out) floats) and added over b in fixed order by a second small kernel.  The gates are
 * recomputed from u and cs.  The caller then takes d weight = X^T dU and dX = dU weight^T (+ dxh) as
 * plain matmuls.  No atomics: reruns are bit-identical and a bidirectional call equals two
 * one-direction calls bit for bit.  n_in is only checked: k = 3 with skip needs n_in == n_out, k = 4
 * needs skip and n_in != n_out.  PKC_ERR_ARG with a pkc_last_error() text for a null pointer or a bad
 * shape.
 * pkc_sru_mask_x: the recurrent ("rnn") dropout of the projection's input, xt[t, b, i] =
 * x[t, b, i] m_x[b, i] with m_x = keep / (1 - drop_p), ONE (B, n_in) mask for all t from the same
 * stream (index b * n_in + i) or keep_in; xt is (T*B, n_in) contiguous, keep (u8) is written.
 * pkc_sru_dx: dx = m_x * (slab_0 + .. + slab_{nslab-1}) + dxh as ONE (T*B, n_in) slab; keep == NULL:
 * no mask, dxh == NULL: no highway gradient.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int T, B, d, ndir, k, act, train, skip;
  int n_in; float alpha;
  const float* u;
  const float* x; int64_t ldx;
  const float* weight_c; const float* bias;
  float* cs; float* y;
  float drop_p; uint64_t seed; const int64_t* step_ctr; int64_t stream_id;
  const uint8_t* keep_in;      /* optional injected keep mask (B, n_out) */
  uint8_t* keep;               /* (B, n_out) mask in use */
  const float* dy; int dy_nslab; int64_t dy_slab_stride;
  float* du; float* dxh; float* dwc; float* dbias; float* work;
} pkc_sru_args;
int pkc_sru_fwd(const pkc_sru_args* a, void* stream);
int pkc_sru_bwd(const pkc_sru_args* a, void* stream);
int pkc_sru_mask_x(int T, int B, int n_in, const float* x, int64_t ldx, float drop_p, uint64_t seed,
                   const int64_t* step_ctr, int64_t stream_id, const uint8_t* keep_in, uint8_t* keep,
                   float* xt, void* stream);
int pkc_sru_dx(int T, int B, int n_in, const float* slabs, int nslab, int64_t slab_stride,
               const uint8_t* keep, float drop_p, const float* dxh, float* dx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Host-side Kaldi ark I/O (data_io.py:770-806 write_mat; 645-711 read_mat_ark binary FM/DM).
 * ------------------------------------------------------------------------------------------- */
int pkc_ark_write_mat(const char* path, int append, const char* key, int64_t rows, int64_t cols,
                      const float* data);
/* Index a binary ark of FM matrices: fills up to cap entries of (data byte offset, rows, cols)
 * and key offsets into keys_buf; returns the number of matrices or <0. */
int64_t pkc_ark_index(const char* path, int64_t* offsets, int64_t* rows, int64_t* cols, int64_t cap,
                      char* keys_buf, int64_t keys_cap);
int pkc_ark_read_rows(const char* path, int64_t offset, int64_t rows, int64_t cols, float* dst);
/* Kaldi "CM " compressed matrix (data_io.py:729-766): blob = the bytes after "\0BCM ";
 * pkc_ark_cm_size -> its byte length; pkc_ark_decode_cm -> rows x cols float32, row-major. */
int64_t pkc_ark_cm_size(const unsigned char* blob, int64_t nbytes);
int pkc_ark_decode_cm(const unsigned char* blob, int64_t nbytes, float* out);

/* ---------------------------------------------------------------------------------------------
 * Chunk-level data parallelism (the reference trains on one GPU, core.py:216-232):
 * one RCCL all-reduce (SUM) of the flat fp32 gradient buffer per step over xGMI, for hosts that
 * do not use torch.distributed.  Rank 0: pkc_dp_unique_id (pkc_dp_unique_id_bytes() bytes),
 * shipped to the other ranks by the host; every rank: pkc_dp_comm_init on its GPU (device < 0:
 * the current one), then pkc_dp_allreduce(comm, grads, n, stream) between the backward and the
 * optimizer launches of each step, with the loss gradient pre-scaled by 1/world (or by the
 * rank's share of the frames) so the sum is the gradient of the global mean loss.
 * ------------------------------------------------------------------------------------------- */
int pkc_dp_unique_id_bytes(void);
int pkc_dp_unique_id(void* id_out);
int pkc_dp_comm_init(void** comm_out, int world, const void* id, int rank, int device);
int pkc_dp_allreduce(void* comm, float* buf, int64_t n, void* stream);
int pkc_dp_comm_destroy(void* comm);

/* ---------------------------------------------------------------------------------------------
 * Conv1d + max-pool layer of the CNN architecture (neural_networks.py:1934-2033; per layer
 * :2017-2029  x = drop(act(norm(F.max_pool1d(conv(x), pool))))  over (B, C, L)).  Additive to
 * ABI 9: new entry points and new structs only.
 *
 * pkc_conv1d_fwd (replaces nn.Conv1d + F.max_pool1d, :2021/:2025/:2028): stride 1, no padding,
 * bias; floor-mode pooling with stride = kernel (the tail L_conv mod pool is dropped).  One
 * launch: an implicit GEMM on the exact-fp32 MFMA over an LDS strip of x (no im2col tensor), W
 * read in its native (C_out, C_in * len) layout, bias + max-pool in the epilogue.  Writes the
 * pooled z (B, C_out, L_out) and, per window, the offset of its first maximum (u8) for the
 * backward; the pre-pool tensor is never stored.  L_conv = L_in - len + 1, L_out = L_conv / pool.
 *
 * pkc_conv1d_bwd (autograd of the same): dz is the gradient of the pooled z.  The un-pooling is
 * part of the operand load (the value at conv position l is dz[l / pool] where off == l % pool,
 * else 0).  dx (nullable) = the transposed convolution; dW and dbias are summed per sample group
 * into partial slabs in `work` (pkc_conv1d_bwd_work_size floats: the same for every B, so a buffer
 * sized once serves any row count of the layer) and then over the slabs in
 * slab order: no floating-point atomics, so equal inputs give bit-identical outputs.
 *
 * x / dx rows: sample b starts at x + b * ldx (dx + b * lddx), channel-major (C_in, L_in) inside.
 * pkc_conv1d_ok: 1 when the shape is supported (pool <= 64, len <= 4033).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int B, C_in, L_in, C_out, len, pool;
  const float* x; int64_t ldx;              /* (B, C_in, L_in), sample stride ldx floats */
  const float* W;                           /* (C_out, C_in, len) */
  const float* bias;                        /* C_out */
  float* z;                                 /* (B, C_out, L_out): forward output */
  uint8_t* off;                             /* (B, C_out, L_out): forward output, backward input */
  const float* dz;                          /* backward: (B, C_out, L_out) */
  float* dx; int64_t lddx;                  /* backward: (B, C_in, L_in) or NULL */
  float* dW; float* dbias;                  /* backward: (C_out, C_in, len), (C_out) */
} pkc_conv1d_args;
int pkc_conv1d_ok(const pkc_conv1d_args* a);
int pkc_conv1d_fwd(const pkc_conv1d_args* a, void* stream);
int64_t pkc_conv1d_bwd_work_size(const pkc_conv1d_args* a);   /* floats; -1: unsupported shape */
int pkc_conv1d_bwd(const pkc_conv1d_args* a, float* work, void* stream);

/* The rest of the layer over the pooled z (B, C, L), one launch per direction:
 *   norm PKC_CONV_NORM_LN : the reference's own LayerNorm (neural_networks.py:40-51) over the last
 *        dimension L of every (b, c) row: gamma[c, l] (z - mean) / (std + eps) + beta[c, l] with
 *        the unbiased std; ln_stat (B * C, 2) keeps 1 / (std + eps) and std;
 *   norm PKC_NORM_BN_TRAIN / _EVAL : nn.BatchNorm1d per channel over B * L (:1988-1990, where the
 *        second positional argument makes eps = L_out: pass that eps), running statistics
 *        updated in training (unbiased variance);
 *   norm PKC_NORM_NONE;
 * then the activation and inverted dropout on the counter-based streams of pkc_dense_fwd (index
 * = the element's flat (B, C * L) index; keep_in: an injected mask; keep: the mask written /
 * read by the backward).  out (B, C * L) channel-major and an optional bf16 copy of it.
 * Backward: g = sum_s gslab[s] (dL/d out); writes dz (B, C, L), dgamma / dbeta ((C, L) for LN,
 * (C) for BN).  Eval: PKC_NORM_BN_EVAL and drop_p = 0. */
#define PKC_CONV_NORM_LN 3
typedef struct {
  int B, C, L;
  int norm;                                   /* PKC_NORM_* or PKC_CONV_NORM_LN */
  const float* z;                             /* (B, C, L) */
  const float* gamma; const float* beta;      /* BN: (C); LN: (C, L) */
  float* running_mean; float* running_var;    /* BN: (C) */
  float momentum, eps;
  float* save_mean; float* save_invstd;       /* BN training: (C) */
  float* ln_stat;                             /* LN: (B * C, 2) */
  int act; float drop_p; uint64_t seed; const int64_t* step_ctr; int64_t stream_id;
  const uint8_t* keep_in;                     /* optional injected dropout mask (B, C * L) */
  uint8_t* keep;                              /* (B, C * L); may be NULL when drop_p == 0 */
  float* xhat;                                /* (B, C, L) normalised z (LN / BN) */
  float* out; void* out_bf16;                 /* (B, C * L); either may be NULL, not both */
  int nslab; const float* gslab; int64_t slab_stride;    /* backward: dL/d out slabs */
  float* dz; float* dgamma; float* dbeta;     /* backward outputs */
} pkc_conv_post_args;
int pkc_conv_post_fwd(const pkc_conv_post_args* a, void* stream);
int pkc_conv_post_bwd(const pkc_conv_post_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sinc filter bank: layer 0 of the SincNet architecture (neural_networks.py:2036-2143; SincConv
 * :2146-2283).  Its convolution weights are N band-pass filters of K taps generated before every
 * forward from two learned vectors low_hz_ and band_hz_ (N each):
 *   low = min_low_hz / sr + |low_hz_|,  high = low + min_band_hz / sr + |band_hz_|,
 *   lp(f)[k] = 2 f sinc(2 pi (f n_[k]) sr)   (sin(x) / x on the left half, 1 at the centre, the
 *   right half the flip of the left),  bp = lp(high) - lp(low),  filters = bp / max_k bp * window.
 * n_ and window (K floats each) are computed by the caller with the reference's own expressions
 * (:2226-2232), so their rounding is the reference's.  Additive to ABI 9.
 *
 * pkc_sinc_filters_fwd: filters (N, K) fp32 in the reference's operation order with the precise
 * sinf: the (C_out, 1, K) weight pkc_conv1d_fwd reads (C_in = 1, len = K, a zero bias).  Per filter
 * it also writes max_ and the index of the first maximum (torch.max's; always in the left half or
 * the centre, since the right half repeats the left).
 *
 * pkc_sinc_filters_bwd: dW (N, K), the filters' gradient as pkc_conv1d_bwd writes it, -> dlow and
 * dband (N): through the window, the division by the maximum (whose index is the forward's), the
 * flip and |.| (gradient 0 at exactly 0).  It re-evaluates the formula in fp64 from the two
 * parameters, so max_ is an output of the forward only.  One workgroup per filter, sums in a fixed
 * order, no atomics: equal inputs give bit-identical outputs.
 *
 * pkc_sinc_ok: 1 when the shape is supported: K odd, 1 <= K <= 4033 (pkc_conv1d's longest
 * filter), 1 <= N <= 65535, sr > 0, min_low_hz >= 0, min_band_hz >= 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int N, K;
  const float* low_hz; const float* band_hz;  /* (N): the parameters low_hz_, band_hz_ */
  const float* n_; const float* window;       /* (K): SincConv.n_, SincConv.window_ */
  float sr, min_low_hz, min_band_hz;
  float* filters;                             /* (N, K): forward output */
  float* max_; int* max_idx;                  /* (N): forward outputs; max_idx backward input */
  const float* dW;                            /* backward: (N, K) */
  float* dlow; float* dband;                  /* backward outputs: (N) */
} pkc_sinc_args;
int pkc_sinc_ok(const pkc_sinc_args* a);
int pkc_sinc_filters_fwd(const pkc_sinc_args* a, void* stream);
int pkc_sinc_filters_bwd(const pkc_sinc_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kaldi fbank / MFCC features from int16 audio (the `pkc-fbank` / `pkc-mfcc` fea_opts stages:
 * compute-fbank-feats / compute-mfcc-feats with snip-edges, no dither, no VTLN, restated from
 * Kaldi's published algorithm).  Additive to ABI 9.
 *
 * samples / utt_beg / utt_len: as pkc_wav_frames (the int16 audio of n_utts whole utterances).
 * Output row r (of `rows`, any order) is frame f = frame_of_row[r] of utterance u = utt_of_row[r],
 * the L samples from f * S; a row whose (u, f) names no whole frame (u outside 0..n_utts-1, f < 0
 * or f * S + L > utt_len[u]) is left unwritten.  Per frame (x, y, E, m and out are float32; the
 * FFT, p and every sum are carried in fp64):
 *   1. x = the L samples;  remove_dc: x -= mean(x) (the sum is an exact integer sum)
 *   2. raw_energy: E = log(max(sum x^2, FLT_EPSILON))
 *   3. y[i] = x[i] - preemph * x[i-1] (i >= 1), y[0] = x[0] - preemph * x[0];  y *= window
 *   4. !raw_energy: E = log(max(sum y^2, FLT_MIN))
 *   5. y zero-padded to N, real FFT, p[k] = |Y[k]|^2 (use_power) or |Y[k]| for k < N/2
 *   6. m[b] = log(max(sum_{i < mel_count[b]} mel_weight[mel_offset[b] + i] * p[mel_first[b] + i],
 *                     FLT_EPSILON));  the Nyquist bin enters no band (mel_first + mel_count <= N/2)
 *   7. fbank: out = [E if use_energy] m;  D = num_bins + use_energy
 *      mfcc:  out[k] = lifter[k] * sum_n dct[k][n] * m[n], out[0] = E if use_energy;  D = num_ceps
 *      where E = max(E, log_energy_floor) (pass -INFINITY for no floor).
 * Host-built device tables (evaluated in double, stored as float): window (L); twiddle (N/2 pairs
 * cos(2 pi k / N), -sin(2 pi k / N), kept as doubles); the mel bands as first bin / count / offset into mel_weight
 * (num_bins each); dct (num_ceps x num_bins) and lifter (num_ceps), mfcc only.
 * Every sum runs in a fixed order, there are no atomics and a row reads only its own samples:
 * equal inputs give equal bits, and a row does not depend on the other rows of the call.
 *
 * pkc_kaldi_feats_ok: 1 when the shape is supported (else 0 and a pkc_last_error() text): N a
 * power of two in 4..4096, 2 <= L <= N, S >= 1, 1 <= num_bins <= 256, D <= 256 and consistent with
 * the kind, 1 <= num_ceps <= num_bins for mfcc.  pkc_kaldi_feats launches nothing for rows == 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int L, S, N;                      /* frame length, frame shift (samples); FFT length */
  int num_bins, num_ceps, D;
  int mfcc;                         /* 0: fbank, 1: mfcc */
  int use_energy, raw_energy, use_power, remove_dc;
  float preemph, log_energy_floor;
  int n_utts;
  int64_t rows;
  const int16_t* samples; const int64_t* utt_beg; const int32_t* utt_len;      /* (n_utts) */
  const int32_t* utt_of_row; const int32_t* frame_of_row;                      /* (rows) */
  const float* window; const double* twiddle;
  const int32_t* mel_first; const int32_t* mel_count; const int32_t* mel_offset;
  const float* mel_weight;
  const float* dct; const float* lifter;
  float* out;                       /* (rows, D) */
} pkc_kaldi_feats_args;
int pkc_kaldi_feats_ok(const pkc_kaldi_feats_args* a);
int pkc_kaldi_feats(const pkc_kaldi_feats_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * splice-feats and transform-feats (the fea_opts stages of the fMLLR feature pipe; Kaldi's
 * SpliceFrames of feat/feature-functions.cc and featbin/transform-feats.cc restated, parity
 * unpinned against Kaldi itself).  Additive to ABI 9.
 *
 * in / src_row / utt_of_row / utt_beg / utt_end: the row maps of pkc_feat_frontend — output row r
 * (of Nout) is source frame s = src_row[r] of utterance u = utt_of_row[r] (of n_utts), whose frames
 * are [utt_beg[u], utt_end[u]) of the N x D matrix `in`.  Per row, with K = D * (L + R + 1):
 *   spl[j*D + d] = in[clamp(s + j - L, utt_beg[u], utt_end[u] - 1)][d],  j = 0..L+R  (past first)
 *   mats != NULL: out[r][o] = (sum_{k < K} A[o][k] * spl[k]) + A[o][K],  o < Dout, where A is
 *     matrix utt_mat[u] (matrix 0 when utt_mat is NULL) of the n_mats row-major Dout x (K + affine)
 *     matrices of `mats`; a linear matrix (affine == 0) has no offset column.  The offset is added
 *     after the sum (AddMatMat, then AddVecToRows).
 *   mats == NULL: out[r] = spl, copied bit for bit (Dout must be K).
 * Products and sums are fp32 (each element one fused multiply-add chain over ascending k from 0,
 * then one addition); there are no atomics and a row reads only its own utterance: equal inputs
 * give equal bits, whatever the order of the rows and whatever else the call computes.
 *
 * tiles: n_tiles pairs {first output row, row count}; the rows of a tile are consecutive output
 * rows that are consecutive frames of one utterance, at most pkc_feat_transform_tile(...) of them,
 * and the tiles together cover the output rows to write.  One workgroup takes one tile: it stages
 * the tile's frames with their context and the utterance's matrix in LDS, and writes a row's
 * outputs as 16-byte stores when Dout % 4 == 0.  A tile that names rows outside 0..Nout-1, or an
 * utterance or matrix out of range, is left unwritten.
 *
 * pkc_feat_transform_ok: 1 when the shape is supported (else 0 and a pkc_last_error() text):
 * D >= 1, 0 <= L, R <= 64, K <= 4096, 1 <= Dout <= 512 with a transform, Dout == K without.
 * pkc_feat_transform_tile: the row count of a full tile for that shape (0 when unsupported).
 * pkc_feat_transform returns PKC_ERR_UNSUPPORTED and launches nothing outside that range, and
 * launches nothing for Nout == 0 or n_tiles == 0.
 * ------------------------------------------------------------------------------------------- */
int pkc_feat_transform_ok(int D, int L, int R, int Dout, int has_mat);
int pkc_feat_transform_tile(int D, int L, int R, int Dout, int has_mat);
int pkc_feat_transform(const float* in, int D, int L, int R, int64_t Nout, const int32_t* src_row,
                       const int32_t* utt_of_row, const int32_t* utt_beg, const int32_t* utt_end,
                       int n_utts, const int32_t* utt_mat, const float* mats, int n_mats, int Dout,
                       int affine, const int32_t* tiles, int n_tiles, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PKC_H_ */
