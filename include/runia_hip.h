/*
 * runia_hip.h — C ABI of the MI355X (gfx950) scoring library `librunia_hip.so`.
 *
 * This is the drop-in boundary for the post-hoc OOD scoring hot path of
 * CEA-LIST/runia_core (reference paths below are relative to
 * /root/reference/runia_core/).  The reference is pure Python: each entry point
 * replaces one host numerical call (NumPy / SciPy / scikit-learn / faiss /
 * entropy_estimators) that the reference makes on this path, and is what a
 * `ctypes` stub in the reference would bind.
 *
 * Conventions (last row):
 *   - every pointer is a DEVICE pointer (HBM) unless the name says `host`;
 *   - matrices are row-major and dense unless a leading dimension is given;
 *   - `stream` is a hipStream_t passed as void*; calls are stream-ordered,
 *     never synchronise, never allocate, and are re-entrant;
 *   - return value: 0 on success, negative RUNIA_E_* code otherwise
 *     (`runia_error_string` gives the text).
 */
#ifndef RUNIA_HIP_H
#define RUNIA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RUNIA_OK 0
#define RUNIA_E_INVALID (-1)   /* bad shape / null pointer / unsupported size */
#define RUNIA_E_LAUNCH (-2)    /* hipGetLastError() after the launch was not hipSuccess */
#define RUNIA_E_NODEVICE (-3)  /* no HIP device visible */
#define RUNIA_E_WORKSPACE (-4) /* caller-provided workspace too small */
#define RUNIA_E_STEPCAP (-5)   /* a bounded device loop ran into its step cap (runia_cc_label); the output is not valid */

typedef void* runia_stream_t;

/* ---- library ------------------------------------------------------------ */
int runia_abi_version(void);
const char* runia_error_string(int code);
/* number of visible HIP devices (0 when none; never fails) */
int runia_device_count(void);
/* Clock reading for measurement records (no counterpart upstream: bench.py brackets its timed regions with it).  One wave
 * runs `chain` (16 .. 2^24, rounded up to 16) dependent v_fma_f32 between two readings of the shader-clock counter
 * (s_memtime) and of the constant 100 MHz counter (s_memrealtime):
 *   out4[0] = shader-clock ticks, out4[1] = 100 MHz ticks, out4[2] = FMAs executed, out4[3] unused.
 * Clock held = out4[0] / (out4[1] * 10 ns). */
int runia_clock_probe(uint64_t* out4, int chain, runia_stream_t stream);
/* Kernel-only timing of ONE launch (measurement records): the next call of this thread to an entry point with a timed launch
 * site (runia_mc_entropy_from_table_f32: the dominant kernel of the headline step) attaches the two hipEvent_t to its dispatch
 * - they then carry the kernel's own start and end timestamps, as rocprofv3's kernel trace does, without the dispatch gap an
 * event pair recorded around the launch includes.  Both events must exist (have been recorded once); (NULL, NULL) clears. */
int runia_time_next_launch(void* start_event, void* stop_event);
/* The ordered keys of the kernels (csrc/order.hpp) on HOST memory, through the same header code, no GPU touched; pins the key
 * layer.  values: f32 or f64 [n] (is_f64); keys: uint64 [n], a 32-bit key zero-extended, the signed one as its two's complement;
 * back (or NULL): [n] of the values' type, the inverse of every key.
 *   ASC / DESC             by the bits alone: -0 next to +0 on the smaller value's side, a NaN by its sign and payload;
 *   ASC_FOLD / DESC_FOLD   -0 on the key of +0;
 *   DESC_ONE_NAN           f64: DESC_FOLD with every NaN on the key of the positive quiet NaN, in front of +inf's;
 *   DESC_SIGNED            f64: DESC_FOLD as int64 of the same order (runia_sel_key_of_f64_host);
 *   ASC_NONNEG             f32: ASC without the sign test, for values >= +0.
 * RUNIA_E_INVALID for a form of the other width. */
#define RUNIA_ORDER_ASC 0
#define RUNIA_ORDER_DESC 1
#define RUNIA_ORDER_ASC_FOLD 2
#define RUNIA_ORDER_DESC_FOLD 3
#define RUNIA_ORDER_DESC_ONE_NAN 4
#define RUNIA_ORDER_DESC_SIGNED 5
#define RUNIA_ORDER_ASC_NONNEG 6
int runia_order_keys_host(const void* values, int64_t n, int is_f64, int form, uint64_t* keys, void* back);

/* ---- a1  MC-dropout latent stacking ------------------------------------- *
 * Replaces MCSamplerModule.forward (feature_extraction/abstract_classes.py:81-101)
 * = n_mc x DropBlock2D (dropblock==0.3.0) + get_mean_or_fullmean_ls_sample("fullmean")
 * (feature_extraction/utils.py:88-92), for a batch of N latent maps.
 *   x     [N, C, H, W] f32 (NCHW)
 *   rand  uniform draws of the drop layers, [n_mc, H, W] per image; image i reads
 *         rand + i*rand_image_stride (stride 0 = the same draws for every image)
 *   out   [N*n_mc, C] f32, image-major (the n_mc rows of one image are contiguous)
 * drop_prob == 0 -> plain full mean replicated n_mc times (DropBlock identity). */
int runia_mc_stack_f32(const float* x, const float* rand, int64_t rand_image_stride, float* out,
                       int64_t N, int C, int H, int W, int n_mc, double drop_prob, int block_size,
                       runia_stream_t stream);

/* layer_type "FC" / "RPN" of the same module (feature_extraction/abstract_classes.py:95-99: no fullmean, each drop
 * layer's output is flattened):  out [N*n_mc, C*H*W] f32 = ((x * bm) * numel) / sum(bm), image-major. */
int runia_mc_drop_flat_f32(const float* x, const float* rand, int64_t rand_image_stride, float* out,
                           int64_t N, int C, int H, int W, int n_mc, double drop_prob, int block_size,
                           runia_stream_t stream);

/* Reductions of dropped activation maps for the other options of FastMCDSamplesExtractor
 * (feature_extraction/image_level.py:205-236 through feature_extraction/utils.py:70-92, 113-126):
 *   x [maps, H, W] f32 (e.g. the output of runia_mc_drop_flat_f32 seen as N*n_mc*C maps)
 *   mode 0: reduction_method="mean" = torch.mean(dim=3)            -> out [maps, H]
 *   mode 1: return_stds = torch.std(torch.std(., dim=3), dim=2)    -> out [maps]  (unbiased; NaN when H or W is 1) */
int runia_map_reduce_f32(const float* x, float* out, int64_t maps, int H, int W, int mode, runia_stream_t stream);

/* The reduction MCDSamplesExtractor applies to the hooked activation after EACH of its mcd_nro_samples stochastic forward
 * passes (feature_extraction/image_level.py:366-410: get_mean_or_fullmean_ls_sample / avg_pool2d / squeeze, reshape(1, -1),
 * two levels of torch.cat), for a whole batch, written into the pass's rows of an existing sample table.
 *   x      the hooked activation seen as (B, C, H, W): element strides sb, sc, sh, sw (>= 0; NCHW, channels_last and sliced
 *          views are read in place; a (B, F) activation is H = W = 1).  dtype 0 f32, 1 f16, 2 bf16.
 *   mode   RUNIA_MCD_FULLMEAN: mean over H and W -> D = C values per image;  RUNIA_MCD_MEAN: mean over W -> D = C * H
 *          values, channel-major;  RUNIA_MCD_AVGPOOL: torch.nn.functional.avg_pool2d(kernel, stride, padding) with its
 *          defaults (floor, padding counted, divisor kernel^2; 2 * padding <= kernel) -> D = C * Ho * Wo values in
 *          (C, Ho, Wo) order;  RUNIA_MCD_COPY: the flattened activation, D = C * H * W.  kernel / stride / padding are read
 *          by RUNIA_MCD_AVGPOOL only.
 *   table  [table_rows, ld] f32, ld >= D: the D values of image b go to row row0 + b * row_step; other rows and the columns
 *          from D on are not touched.  row0 = s, row_step = mcd: pass s of a batch fills its slot of an image-major
 *          (B * mcd, D) block.
 * f32 accumulation (f16 / bf16 widened exactly).  One launch; a channels_last fullmean of fewer images than fill the device (or of
 * maps with more than 512 pixels per pixel slot of a workgroup) splits the pixels of an image over several workgroups, which add their partial means with float atomics into rows zeroed by
 * a small launch in front (the only case whose last bits depend on the order of arrival). */
#define RUNIA_MCD_FULLMEAN 0
#define RUNIA_MCD_MEAN 1
#define RUNIA_MCD_AVGPOOL 2
#define RUNIA_MCD_COPY 3
int runia_mcd_reduce_rows(const void* x, int dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t sb, int64_t sc,
                          int64_t sh, int64_t sw, int mode, int kernel, int stride, int padding, float* table,
                          int64_t table_rows, int64_t ld, int64_t row0, int64_t row_step, runia_stream_t stream);

/* The row tables of get_aggregated_data_dict (feature_extraction/utils.py:160-191: per field one torch.cat over the images
 * that have rows, with torch.log(logits + 1e-10) per image when probs_as_logits) from the caller's per-image tensors.
 *   table      device array of n_seg segment descriptors, 4 int64 each: {pointer to the segment's (rows, D) tensor, rows,
 *              row stride, column stride (elements)}.  Every tensor is read in place through its own strides.  The caller
 *              checks the shapes (the kernel trusts the table); segments of 0 rows are legal.
 *   row_start  device array of n_seg + 1 int64: exclusive prefix sum of the rows (row_start[n_seg] == total).
 *   dtype      0 f32, 1 f16, 2 bf16 (all segments and out of one call).
 *   mode       RUNIA_RAGGED_COPY: the rows as they are (bit copies);  RUNIA_RAGGED_LOG_EPS: log(x + 1e-10) as torch forms
 *              it on a tensor of that dtype: the sum in f32 rounded to dtype, the logarithm in f32 rounded to dtype (an f16
 *              zero gives -inf, an f32 zero log(1e-10f)).
 *   out        [total, ld] of dtype, ld >= D: segment s fills rows row_start[s] .. row_start[s + 1] - 1; the columns from D
 *              on are not touched.
 *   seg_of_row [total] int32 or NULL: the segment every output row came from.
 * One launch whatever n_seg is (none when total or n_seg is 0).  Segments whose columns are contiguous, whose pointer is
 * 16-byte aligned and whose rows lie a whole number of 16-byte vectors apart move 16 bytes per lane (out 16-byte aligned,
 * ld a multiple of the vector as well); every other segment moves element by element. */
#define RUNIA_RAGGED_COPY 0
#define RUNIA_RAGGED_LOG_EPS 1
int runia_ragged_rows(const int64_t* table, const int64_t* row_start, int64_t n_seg, int64_t total, int64_t D, int dtype,
                      int mode, void* out, int64_t ld, int32_t* seg_of_row, runia_stream_t stream);

/* ---- a2  Kozachenko-Leonenko kNN entropy --------------------------------- *
 * Replaces the loops of get_dl_h_z / single_image_entropy_calculation
 * (evaluation/entropy.py:20-93) over entropy_estimators.continuous.get_h(col, k,
 * norm="max", min_dist).
 *   z  [N*n_mc, D] f32 image-major;  h  [N, D] f64;  h_mvn [N] f64
 * 2 <= n_mc <= 64, 1 <= k < n_mc. */
int runia_kl_entropy_per_dim_f32(const float* z, double* h, int64_t N, int n_mc, int64_t D, int k,
                                 double min_dist, runia_stream_t stream);
int runia_kl_entropy_joint_f32(const float* z, double* h_mvn, int64_t N, int n_mc, int64_t D, int k,
                               double min_dist, runia_stream_t stream);
/* Both outputs of one get_dl_h_z call (evaluation/entropy.py:67-84: the joint entropy AND the per-dimension entropies of every
 * image) from ONE pass over z: h_mvn [N] f64 and h [N, D] f64 carry the bits of the two entry points above.  The single-read
 * kernel covers 5 <= n_mc <= 32 with k = 5 (n_mc <= 8 also k = 4) on rows of whole 16-byte (n_mc <= 16) / 8-byte vectors;
 * runia_kl_entropy_both_fused tells (1 / 0); other shapes run the two kernels one after the other inside the same call. */
int runia_kl_entropy_both_fused(int n_mc, int64_t D, int k);
/* Which kernel runia_kl_entropy_joint_f32 / runia_kl_entropy_per_dim_f32 launch for a shape (host-only; the two entry points
 * choose through these very functions, so the answer is the dispatch).  byte_offset: the operands' distance from a 16-byte
 * boundary - z & 15 for the joint call, (z | h) & 15 for the per-dimension one.  RUNIA_E_INVALID for arguments the entry points
 * refuse (n_mc outside 2 .. 64, D <= 0, k outside 1 .. n_mc - 1) and for byte_offset < 0.
 *   joint          LDS: any shape (n_mc > 32, rows that are not whole aligned vectors);  REG8 / REG16 / REG32: the register form
 *                  with room for 8 / 16 / 32 samples (n_mc <= 8 / 16 / 32; rows of whole 16- / 16- / 8-byte aligned vectors);
 *                  PAIR16: the pair-group form (9 <= n_mc <= 16, even D, 8-byte aligned rows).
 *   per dimension  GENERIC: the insertion-sort kernel for any k;  RUNIA_KL_PER_DIM_REG(NP, K, VEC) = 100 NP + 10 K + VEC: the
 *                  register kernel with room for NP = 4 .. 64 samples (the power of two >= n_mc), K = k compiled in and
 *                  VEC = 4 (float4 loads: NP <= 16, D % 4 == 0, byte_offset % 16 == 0) or 1 adjacent dims per thread. */
#define RUNIA_KL_JOINT_LDS 0
#define RUNIA_KL_JOINT_REG8 1
#define RUNIA_KL_JOINT_REG16 2
#define RUNIA_KL_JOINT_REG32 3
#define RUNIA_KL_JOINT_PAIR16 4
#define RUNIA_KL_PER_DIM_GENERIC 0
#define RUNIA_KL_PER_DIM_REG(np, k, vec) (100 * (np) + 10 * (k) + (vec))
int runia_kl_entropy_joint_form(int n_mc, int64_t D, int byte_offset);
int runia_kl_entropy_per_dim_form(int n_mc, int k, int64_t D, int byte_offset);
int runia_kl_entropy_both_f32(const float* z, double* h_mvn, double* h, int64_t N, int n_mc, int64_t D, int k,
                              double min_dist, runia_stream_t stream);

/* ---- dense f64 weights, packed once at setup ------------------------------ *
 * The f64 contractions (PCA projection, quadratic forms) read their constant
 * right-hand matrix B [K, n] (row-major, ld = ldb) from a fragment-ordered copy
 * so that every MFMA operand load is one coalesced 512-byte wave access.
 * `runia_packed_weights_bytes` gives the size of that copy. */
size_t runia_packed_weights_bytes(int64_t K, int64_t n);
int runia_pack_weights_f64(const double* B, int64_t ldb, int64_t K, int64_t n, double* packed,
                           runia_stream_t stream);

/* ---- a4  PCA transform ---------------------------------------------------- *
 * Replaces apply_pca_transform (dimensionality_reduction.py:75-87) = sklearn
 * PCA.transform:  Y = X @ C.T - mean @ C.T;  Y /= scale  (when whiten != 0).
 *   x [N, D] (f64 or f32), packed_ct = pack(C.T [D, n]), bias [n] = mean @ C.T,
 *   scale [n] = max(sqrt(explained_variance_), eps), y [N, n] f64. */
int runia_pca_transform_f64(const double* x, const double* packed_ct, const double* bias,
                            const double* scale, double* y, int64_t N, int64_t D, int64_t n,
                            int whiten, runia_stream_t stream);
int runia_pca_transform_f32in(const float* x, const double* packed_ct, const double* bias,
                              const double* scale, double* y, int64_t N, int64_t D, int64_t n,
                              int whiten, runia_stream_t stream);

/* ---- a5  LaREM = MDLatentSpace.postprocess -------------------------------- *
 * Replaces -np.diag(diff @ P @ diff.T) (inference/postprocessors.py:241-242).
 *   x [N, n], mean [n], packed_p = pack(P [n, n]), score [N] f64.
 * `diff` follows NumPy's dtype rules: f32 - f32 is rounded to f32 before the f64
 * quadratic form (the reference's own unit test feeds f32 features); every other
 * combination subtracts in f64 (an f32 mean against f64 rows is widened by the caller). */
int runia_md_score_f64(const double* x, const double* mean, const double* packed_p, double* score,
                       int64_t N, int64_t n, runia_stream_t stream);
int runia_md_score_f32(const float* x, const float* mean, const double* packed_p, double* score,
                       int64_t N, int64_t n, runia_stream_t stream);
int runia_md_score_f32x_f64mean(const float* x, const double* mean, const double* packed_p,
                                double* score, int64_t N, int64_t n, runia_stream_t stream);
/* runia_md_score_tril_*: the same score from the TRIANGULAR factor of the precision (round 6): precision = W^T W with W lower
 *   triangular (e.g. the reversed Cholesky factor, see runia_cholesky_f64), packed_wt = runia_pack_weights_f64 of W^T [n, n]:
 *   score = -|| W (x - mean) ||^2 = -(x - mean) precision (x - mean)^T (inference/postprocessors.py:241-242) with only the
 *   k <= column part of every 256-column block multiplied - n^2 + 256 n multiply-adds per row instead of 2 n^2.  Same dtype
 *   combinations and centring rules as runia_md_score_*.  The caller keeps runia_md_score_* for a precision that has no such
 *   factor (rank-deficient pinvh).  workspace (optional): runia_md_score_workspace_bytes(N, n) bytes, as runia_md_score_ws_*
 *   (few rows of wide features: column blocks on separate workgroups + a replay launch, same bits). */
int runia_md_score_tril_f64(const double* x, const double* mean, const double* packed_wt, double* score, void* workspace,
                            size_t workspace_bytes, int64_t N, int64_t n, runia_stream_t stream);
int runia_md_score_tril_f32(const float* x, const float* mean, const double* packed_wt, double* score, void* workspace,
                            size_t workspace_bytes, int64_t N, int64_t n, runia_stream_t stream);
int runia_md_score_tril_f32x_f64mean(const float* x, const double* mean, const double* packed_wt, double* score,
                                     void* workspace, size_t workspace_bytes, int64_t N, int64_t n, runia_stream_t stream);
/* The same scores (bit for bit) with a workspace (round 4): for few rows of wide features - MD on un-reduced 2048-d features,
 * one image at a time - the 256-column blocks of a 16-row tile go to separate workgroups and a second launch adds their
 * products in the one-launch kernel's order (0.9 -> 0.1 ms at <= 512 rows x 2048).  runia_md_score_workspace_bytes returns
 * 0 where the one launch is taken anyway (then NULL / 0 may be passed). */
size_t runia_md_score_workspace_bytes(int64_t N, int64_t n);
int runia_md_score_ws_f64(const double* x, const double* mean, const double* packed_p, double* score, void* workspace,
                          size_t workspace_bytes, int64_t N, int64_t n, runia_stream_t stream);
int runia_md_score_ws_f32(const float* x, const float* mean, const double* packed_p, double* score, void* workspace,
                          size_t workspace_bytes, int64_t N, int64_t n, runia_stream_t stream);
int runia_md_score_ws_f32x_f64mean(const float* x, const double* mean, const double* packed_p, double* score,
                                   void* workspace, size_t workspace_bytes, int64_t N, int64_t n, runia_stream_t stream);

/* ---- a6  class-conditional Mahalanobis ------------------------------------ *
 * Replaces mahalanobis_postprocess (inference/funcs.py:69-102): for each row and
 * class c, t = x - mu_c (in the dtype of the inputs), s_c = -t P t^T in f64,
 * NaN -> -inf, max over classes.
 *   x [N, D] f32 (…_f32) or f64 (…_f64); class_mean [C, D] same dtype as x;
 *   packed_p = pack(P [D, D]); mu_p [C, D] f64 = class_mean @ P; score [N] f64.
 *   workspace: C <= 16: not touched (the class terms come out of the GEMM accumulators).  C > 16: holds G = X P for a
 *   chunk of rows (runia_mahalanobis_workspace_bytes; any size >= one row works, rows are processed in chunks that
 *   fit); with runia_mahalanobis_workspace_bytes_classes(N, D, C) bytes (16-byte aligned) the class terms become a
 *   second contraction on the matrix cores - S = G M^T ranks the classes, the f32-difference formula is evaluated for the
 *   classes within 1e-3 of the best - instead of a loop over all classes per row (same scores; C = 1000: 20x faster). */
size_t runia_mahalanobis_workspace_bytes(int64_t N, int64_t D);
size_t runia_mahalanobis_workspace_bytes_classes(int64_t N, int64_t D, int C);
int runia_mahalanobis_score_f32(const float* x, const float* class_mean, const double* packed_p,
                                const double* mu_p, double* score, void* workspace,
                                size_t workspace_bytes, int64_t N, int64_t D, int C,
                                runia_stream_t stream);
int runia_mahalanobis_score_f64(const double* x, const double* class_mean, const double* packed_p,
                                const double* mu_p, double* score, void* workspace,
                                size_t workspace_bytes, int64_t N, int64_t D, int C,
                                runia_stream_t stream);

/* ---- a7  Energy / MSP ------------------------------------------------------ *
 * Replaces scipy.special.logsumexp(x, axis=1) and np.max(softmax(x, axis=1), axis=1)
 * (inference/postprocessors.py:549, 606).  logits [N, C] f32; outputs [N] f32;
 * either output pointer may be NULL. */
int runia_row_lse_msp_f32(const float* logits, float* lse, float* msp, int64_t N, int64_t C,
                          runia_stream_t stream);

/* ---- a8  kNN ---------------------------------------------------------------- *
 * normalizer (inference/funcs.py:105-115): y = x / (||x||_2 + 1e-10), f32. */
int runia_l2_normalize_f32(const float* x, float* y, int64_t N, int64_t D, runia_stream_t stream);
/* faiss.IndexFlatL2(D).add(bank); search(q, k) -> -D[:, -1]
 * (inference/postprocessors.py:396-397,419,850-851,878).  q [N, D] and bank [M, D]
 * are already normalised f32; score [N] f32 = -(k-th smallest squared L2), or
 * -FLT_MAX when k > M.  `workspace` holds the distance tiles
 * (runia_knn_workspace_bytes) and, for large problems, the bf16 planes of the
 * candidate-distance kernel: with a workspace of the size asked for, the
 * candidates of a large problem come from bf16 piece products
 * (runia_knn_piece_products of them, 0 = the f32 matrix-core kernel); with a
 * smaller workspace always from the f32 kernel.  The score is the exactly
 * re-measured f32 distance on either path (identical bits). */
size_t runia_knn_workspace_bytes(int64_t N, int64_t M, int64_t D, int k);
int runia_knn_piece_products(int64_t N, int64_t M, int64_t D);
/* The same search against a bank prepared once (the index of a deployed postprocessor; faiss does its `add` once, too):
 * `state` (runia_knn_bank_state_bytes, 16-byte aligned) receives |b|^2, their maximum and - for banks the bf16 kernel can
 * take - the bf16 pieces; a call then needs runia_knn_prepared_workspace_bytes of workspace (one chunk of distances,
 * |q|^2, the chunk's pieces) and skips the bank passes.  Same scores, bit for bit, as runia_knn_kth_f32; a state of only
 * (M + 1) floats (rounded up to 256 bytes) or a smaller workspace keeps the f32 kernel. */
size_t runia_knn_bank_state_bytes(int64_t M, int64_t D);
int runia_knn_prepare_bank_f32(const float* bank, void* state, size_t state_bytes, int64_t M, int64_t D,
                               runia_stream_t stream);
size_t runia_knn_prepared_workspace_bytes(int64_t N, int64_t M, int64_t D, int k);
int runia_knn_kth_prepared_f32(const float* q, const float* bank, const void* state, size_t state_bytes, float* score,
                               void* workspace, size_t workspace_bytes, int64_t N, int64_t M, int64_t D, int k,
                               runia_stream_t stream);
int runia_knn_kth_f32(const float* q, const float* bank, float* score, void* workspace,
                      size_t workspace_bytes, int64_t N, int64_t M, int64_t D, int k,
                      runia_stream_t stream);

/* ---- a9  LaRED = KernelDensity.score_samples (gaussian) --------------------- *
 * Replaces DetectorKDE.get_density_scores (inference/postprocessors.py:118-128):
 * logsumexp_i(-|x - t_i|^2 / (2 h^2)) - log(M) - D log(h) - (D/2) log(2 pi).
 *   train [M, D] f64, x [N, D] f64, score [N] f64 */
int runia_kde_score_f64(const double* train, const double* x, double* score, int64_t M, int64_t N,
                        int64_t D, double bandwidth, runia_stream_t stream);
/* runia_kde_score_kernel_f64: the same log-density for every kernel sklearn's KernelDensity offers (DetectorKDE(kernel=...)
 * forwards any, inference/postprocessors.py:78-128): kind 0 gaussian (= runia_kde_score_f64), 1 tophat, 2 epanechnikov,
 * 3 exponential, 4 linear, 5 cosine, with sklearn's normalisation; a query with no training row in range scores -inf. */
int runia_kde_score_kernel_f64(const double* train, const double* x, double* score, int64_t M, int64_t N, int64_t D,
                               double bandwidth, int kind, runia_stream_t stream);
/* The same log-density with the pair distances on the f64 matrix cores, |x - t|^2 = |x|^2 + |t|^2 - 2 x.t (for
 * wide embeddings, D > 64): packed_train_t = runia_pack_weights_f64 of train^T [D, M] and train_sqnorm [M] =
 * runia_row_sqnorm_f64(train), both made once at setup; workspace: N doubles (the query norms).  The logsumexp over
 * the M training rows is kept online in the accumulator lanes; no [N, M] matrix is written. */
int runia_row_sqnorm_f64(const double* x, double* out, int64_t N, int64_t D, runia_stream_t stream);
/* workspace of runia_kde_score_packed_f64: the N query norms, plus room for the column-split units (same bits) that take
 * either a batch of fewer 16-row tiles than the chip has compute units (a fraction of the latency) or, since ABI 4, the rows
 * of a large batch behind its last whole round of 32-row tiles (no last round on part of the chip); N doubles are the minimum */
size_t runia_kde_workspace_bytes(int64_t N, int64_t M);
int runia_kde_score_packed_f64(const double* packed_train_t, const double* train_sqnorm, const double* x,
                               double* score, void* workspace, size_t workspace_bytes, int64_t M, int64_t N,
                               int64_t D, double bandwidth, runia_stream_t stream);

/* ---- a11 fused LaREM row pipeline ------------------------------------------- *
 * LaRExInference.get_score after the backbone (inference/image_level.py:115-119) as two
 * launches per batch.
 * (1) runia_mc_entropy_f32 = MCSamplerModule.forward fused with the per-dimension loop of
 *     get_dl_h_z: latent maps x [N, C, H, W] f32 + DropBlock draws (layout as
 *     runia_mc_stack_f32) -> entropies h [N, C] f64; the MC samples never leave registers.
 *     z_out (optional, may be NULL): [N*n_mc, C] f32 copy of the samples, drop layers in
 *     mask-sum order (entropy is invariant to their order).  Shapes outside
 *     runia_mc_entropy_supported() return RUNIA_E_INVALID: use the two unfused calls.
 *     zero_fill (optional, may be NULL): [N] f64 set to 0.0 by the launch - the accumulator that
 *     runia_proj_sq_accumulate_f64 adds into, cleared here for free instead of by a launch of its own.
 *     workspace: runia_mc_entropy_workspace_bytes(N, H, W, n_mc) bytes of device memory, 16-byte
 *     aligned (the per-image keep-flag table a first small launch derives from the draws;
 *     RUNIA_E_WORKSPACE if missing or short).
 * (2) runia_pca_md_score_f64 = apply_pca_transform + MDLatentSpace.postprocess:
 *     h [N, D] f64 -> score [N] f64; packed_ct/bias/scale as runia_pca_transform_f64
 *     (packed_ct NULL = no PCA, n == D), md_mean [n], packed_p = pack(P [n, n]);
 *     y_out (optional) receives the projected rows [N, n]. */
int runia_mc_entropy_supported(int H, int W, int n_mc, int k);
size_t runia_mc_entropy_workspace_bytes(int64_t N, int H, int W, int n_mc);
/* The two launches of runia_mc_entropy_f32 on their own (same arguments, same workspace): the keep-flag table
 * of the draws (the DropBlock2D mask of feature_extraction/abstract_classes.py:91-96, drop layers sorted by mask
 * sum), then sampler + entropy from that table.  A table may be reused for other latents of the same batch
 * geometry (upstream draws the masks once per forward pass and applies them to every hooked layer). */
int runia_mc_mask_table_f32(const float* rand, int64_t rand_image_stride, void* workspace,
                            size_t workspace_bytes, int64_t N, int H, int W, int n_mc, double drop_prob,
                            int block_size, runia_stream_t stream);
/* runia_mc_stack_table_f32 = runia_mc_stack_f32 (same samples, same order, same bits) on the table path, for the
 * map shapes of runia_mc_entropy_supported(H, W, n_mc, 5); workspace as for runia_mc_entropy_f32. */
int runia_mc_stack_table_f32(const float* x, const float* rand, int64_t rand_image_stride, float* z,
                             void* workspace, size_t workspace_bytes, int64_t N, int C, int H, int W, int n_mc,
                             double drop_prob, int block_size, runia_stream_t stream);
int runia_mc_entropy_from_table_f32(const float* x, const void* workspace, size_t workspace_bytes, double* h,
                                    float* z_out, double* zero_fill, int64_t N, int C, int H, int W, int n_mc,
                                    int k, double min_dist, runia_stream_t stream);
int runia_mc_entropy_f32(const float* x, const float* rand, int64_t rand_image_stride, double* h,
                         float* z_out, double* zero_fill, void* workspace, size_t workspace_bytes, int64_t N,
                         int C, int H, int W, int n_mc, double drop_prob, int block_size, int k, double min_dist,
                         runia_stream_t stream);
/* The product case of runia_mc_entropy_f32 as ONE launch, without the keep-flag launch and its per-image table: 4x4 maps,
 * n_mc == 16, k == 5, explicit draws, drop_prob > 0, no z_out (runia_mc_entropy_lut_supported; anything else: the entry
 * points above).  What the keep-flag launch derives from a drop layer's 16 seed bits depends on (H, W, block_size) alone, so
 * it is a table over all 65 536 seed words, built once on the HOST: runia_mc_flag_lut_fill writes
 * runia_mc_flag_lut_bytes(H, W, block_size) bytes (0: geometry not supported) of records of 20 dwords - the 16 keep flags
 * (2^-a or 0, in the kernel's operand order), zh, zl as the keep-flag table holds them (a fully dropped layer: zh = NaN,
 * flags 0), a sort word (class << 27 | record byte offset; class = (m - 1) / 2, 8 for a fully dropped layer) and the odd
 * part m of the mask sum (0 for a fully dropped layer) - followed by zero records up to the largest byte offset a sort word
 * can carry (2^23), so that the kernel's reads stay inside lut_bytes whatever a caller's table holds.  host_out: 4-byte aligned (RUNIA_E_INVALID if NULL, misaligned or the
 * geometry is not supported; RUNIA_E_WORKSPACE if `bytes` is short).
 * runia_mc_entropy_lut_f32: `lut` = a DEVICE copy of exactly those bytes for the same block_size (lut_bytes short or lut NULL:
 * RUNIA_E_WORKSPACE); x 16-byte aligned; rand [N, 16, 4, 4] with rand_image_stride >= 0 elements between images; h, zero_fill
 * as runia_mc_entropy_f32.  Each wave forms its image's seed bits from the draws with four ballots and reads its operands from
 * the table through the scalar cache.  h is bit-identical to runia_mc_entropy_f32 on the same arguments. */
size_t runia_mc_flag_lut_bytes(int H, int W, int block_size);
int runia_mc_flag_lut_fill(void* host_out, size_t bytes, int H, int W, int block_size);
int runia_mc_entropy_lut_supported(int H, int W, int n_mc, int k, int block_size);
int runia_mc_entropy_lut_f32(const float* x, const float* rand, int64_t rand_image_stride, const void* lut,
                             size_t lut_bytes, double* h, double* zero_fill, int64_t N, int C, int H, int W, int n_mc,
                             double drop_prob, int block_size, int k, double min_dist, runia_stream_t stream);
/* Throughput mode of the sampler: the DropBlock draws are not read from memory but made
 * inside the keep-flag launch by a counter generator - Philox4x32-10 keyed by `seed`; draw i (= layer*H*W + position)
 * of image g is component (i/64)&3 of philox(counter = (g.lo, g.hi, i%64 + 64*(i/256), 0)), u = (bits >> 8) * 2^-24.
 * Image ids are first_image .. first_image+N-1, so a batch scored whole, in chunks or sharded draws the same masks.
 * runia_mc_draws_f32 writes the same draws out, [N, n_mc, H, W]: feeding them to the `rand` argument of
 * runia_mc_entropy_f32 / runia_mc_stack_f32 gives the same bits as the counter entry points. */
int runia_mc_draws_f32(float* out, int64_t N, int n_mc, int H, int W, uint64_t seed, int64_t first_image,
                       runia_stream_t stream);
/* redraw_dead_layers != 0 (opt-in, ABI 3): a drop layer whose block mask removes the WHOLE map - 0 * numel / 0 = NaN in
 * the reference as well (dropblock==0.3.0 does not guard it) - draws again from the same image's next counter block
 * (fourth Philox counter word = attempt 1, 2, ... up to 16), so that a batched caller gets no NaN score.  Not the
 * reference's semantics (it has no redraw); counter mode is not the reference's random stream to begin with. */
int runia_mc_mask_table_counter_f32(uint64_t seed, int64_t first_image, void* workspace, size_t workspace_bytes,
                                    int64_t N, int H, int W, int n_mc, double drop_prob, int block_size,
                                    int redraw_dead_layers, runia_stream_t stream);
int runia_mc_entropy_counter_f32(const float* x, uint64_t seed, int64_t first_image, double* h, float* z_out,
                                 double* zero_fill, void* workspace, size_t workspace_bytes, int64_t N, int C, int H,
                                 int W, int n_mc, double drop_prob, int block_size, int k, double min_dist,
                                 int redraw_dead_layers, runia_stream_t stream);
int runia_pca_md_score_f64(const double* h, const double* packed_ct, const double* bias,
                           const double* scale, const double* md_mean, const double* packed_p,
                           double* score, double* y_out, int64_t N, int64_t D, int64_t n,
                           runia_stream_t stream);
/* (2') runia_proj_sq_score_f64: the same LaREM score from ONE contraction, score = -|| M h + c ||^2, where the
 *     caller folded PCA transform, centring and the factor W of precision = W^T W into M [r, D] = W diag(1/scale) C
 *     and c [r] = W (-bias/scale - md_mean) at setup (exact algebra, f64): packed_m = pack(M.T [D, r]). */
/*     workspace (optional: NULL / 0 is accepted): runia_proj_sq_workspace_bytes(N) bytes let batches of a few
 *     row tiles per compute unit be cut in column halves (two partial row sums + one small combine launch). */
size_t runia_proj_sq_workspace_bytes(int64_t N);
/*     runia_proj_sq_accumulate_f64: the same score ADDED into `score`, which the caller zeroed earlier in the
 *     stream (runia_mc_entropy_f32's zero_fill): the column halves of a row tile each add their row sums with one
 *     f64 atomic - two addends per row, so the result does not depend on their order - and no combine launch or
 *     workspace is needed.  Bit-identical to runia_proj_sq_score_f64. */
int runia_proj_sq_accumulate_f64(const double* h, const double* packed_m, const double* c, double* score,
                                 int64_t N, int64_t D, int64_t r, runia_stream_t stream);
int runia_proj_sq_score_f64(const double* h, const double* packed_m, const double* c, double* score,
                            void* workspace, size_t workspace_bytes, int64_t N, int64_t D, int64_t r,
                            runia_stream_t stream);
/*     runia_proj_sq_*_trap_f64: the same two calls for an upper-TRAPEZOIDAL M (r <= D and M[j][k] = 0 for k < j, the
 *     caller's promise; runia_qr_trapezoid_f64 makes one).  Column tile t of M^T holds only zeros in its rows k < 16 t, so
 *     the contraction starts behind them: 0.78 of the matrix instructions at r = 256, D = 512.  Same packed layout (zero
 *     blocks stored), same summation order, and on such a matrix the same bits as the plain calls for finite h.  A row
 *     with a NaN h scores NaN in both (column tile 0 skips nothing); a row with an infinite h never scores a finite
 *     value, but where the plain call says NaN (0 * inf in a zero block) the trap call may say -inf: that happens for an
 *     infinity at the last k of a skipped chunk (k = 32 q - 1), whose only zeros lie in skipped blocks. */
int runia_proj_sq_accumulate_trap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                      int64_t N, int64_t D, int64_t r, runia_stream_t stream);
int runia_proj_sq_score_trap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                 void* workspace, size_t workspace_bytes, int64_t N, int64_t D, int64_t r,
                                 runia_stream_t stream);
/*     runia_qr_trapezoid_f64: r_out [r, D] = Q m, c_out [r] = Q c for the orthogonal Q (Householder reflections on
 *     [m | c], r <= D, r <= 4096) that makes r_out upper-trapezoidal: r_out^T r_out = m^T m, || r_out h + c_out || =
 *     || m h + c ||, and r_out[j][k] is exactly 0.0 for k < j.  A column that is already zero below the diagonal gets
 *     no reflection (rank-deficient m is fine).  One workgroup, every sum in an order fixed by the code: the same input
 *     gives the same bits on every call and every rank.  r_out may be m and c_out may be c (in place). */
int runia_qr_trapezoid_f64(const double* m, const double* c, double* r_out, double* c_out, int64_t r, int64_t D,
                           runia_stream_t stream);
/*     Balanced block order (csrc/trap_order.hpp).  Block b of an upper-trapezoidal R (rows 32 b .. 32 b + 31) is zero for
 *     k < 32 b, and a row permutation of [R | c] does not change || R h + c ||.  With the column split, the 32-column
 *     groups 0-3 of a 256-column block of R^T belong to one workgroup and 4-7 to another; in the natural order they skip
 *     6 and 22 of their 64 chunk-waves.  The balanced order gives the first R blocks {0, 3, 5, 6} and the second
 *     {1, 2, 4, 7} of every FULL 256-row block (14 each); a last partial block and every r < 256 keep the natural order.
 *     runia_trap_balance_order: src_rows [r] (HOST memory) = the row of R that stands at each row of the balanced matrix.
 *     runia_trap_balance_rows_f64: r_out [r, D] and c_out [r] = r_in and c_in with their rows in that order (device,
 *     not in place: r_out != r_in, c_out != c_in).
 *     runia_proj_sq_*_btrap_f64: runia_proj_sq_*_trap_f64 for such a matrix (the caller's promise, r <= D): every column
 *     group starts at the first live chunk of the block it holds.  Same packed layout, same summation order, same bits
 *     as the plain calls on that matrix for finite h; NaN and infinity as documented for the trap calls (R block 0 stays
 *     in column tile 0, which skips nothing). */
int runia_trap_balance_order(int64_t* src_rows, int64_t r);
int runia_trap_balance_rows_f64(const double* r_in, const double* c_in, double* r_out, double* c_out, int64_t r, int64_t D,
                                runia_stream_t stream);
int runia_proj_sq_accumulate_btrap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                       int64_t N, int64_t D, int64_t r, runia_stream_t stream);
int runia_proj_sq_score_btrap_f64(const double* h, const double* packed_m, const double* c, double* score,
                                  void* workspace, size_t workspace_bytes, int64_t N, int64_t D, int64_t r,
                                  runia_stream_t stream);

/* ---- f1  setup-time covariance on the device (SURVEY 8f "next #1") ----------- *
 * Replaces np.cov(X.T, bias=1) inside sklearn EmpiricalCovariance.fit
 * (inference/postprocessors.py:217-220, inference/funcs.py:62-66):
 * mean [D] = column means, cov [D, D] = (X - mean)^T (X - mean) / N, f64 (f32 rows are promoted).
 * x [N, D]; workspace from runia_covariance_workspace_bytes. */
size_t runia_covariance_workspace_bytes(int64_t N, int64_t D);
int runia_covariance_f64(const double* x, double* mean, double* cov, void* workspace,
                         size_t workspace_bytes, int64_t N, int64_t D, runia_stream_t stream);
int runia_covariance_f32in(const float* x, double* mean, double* cov, void* workspace,
                           size_t workspace_bytes, int64_t N, int64_t D, runia_stream_t stream);

/* ---- f3  the step in front of the sampler for object-level inference ------------------------ *
 * torchvision.ops.roi_align as the reference calls it (feature_extraction/object_level.py:283-292, 340-349):
 *   input [B, C, H, W] f32, boxes [K, 4] f32 (x1, y1, x2, y2 in image pixels), batch_idx [K] int32 (NULL when B == 1),
 *   out [K, C, PH, PW] f32; bins average sampling_ratio^2 bilinear samples (ceil(roi / pooled) per axis when
 *   sampling_ratio <= 0); aligned != 0 shifts the box by -0.5 pixel.  The output is the (N, C, H, W) input of
 *   runia_mc_entropy_f32 / runia_mc_stack_f32: roi_align -> per-ROI MC DropBlock -> entropy with no host round trip. */
int runia_roi_align_f32(const float* input, const float* boxes, const int* batch_idx, float* out, int64_t K, int64_t B,
                        int C, int H, int W, int PH, int PW, double spatial_scale, int sampling_ratio, int aligned,
                        runia_stream_t stream);
/* roi_align folded into the sampler + entropy launch (round 4; _dropblock_rois_get_entropy, feature_extraction/
 * object_level.py:312-367, as ONE pass from the hooked feature map to the per-ROI entropies - the (K, C, PH, PW) tensor is
 * never written).  runia_nchw_to_nhwc_f32: the hooked map [B, C, H*W] -> [B, H*W, C] once per image batch (channel = lane:
 * every bilinear tap of a wave is one contiguous run).  runia_roi_mc_entropy_f32: feat_nhwc [B, H, W, C], boxes [K, 4] xyxy,
 * batch_idx [K] or NULL (B == 1), draws / workspace as runia_mc_entropy_f32 (workspace:
 * runia_roi_mc_entropy_workspace_bytes: the keep-flag table + 16 bytes per sample row and sample column of every ROI) -> h [K, C] f64,
 * the same bits as runia_roi_align_f32 followed by runia_mc_entropy_f32.  Supported (runia_roi_mc_entropy_supported): the
 * fused sampler's map shapes with sampling_ratio 1 or 2; others take the two calls. */
int runia_nchw_to_nhwc_f32(const float* in, float* out, int64_t B, int C, int64_t HW, runia_stream_t stream);
int runia_roi_mc_entropy_supported(int PH, int PW, int n_mc, int k, int sampling_ratio);
size_t runia_roi_mc_entropy_workspace_bytes(int64_t K, int PH, int PW, int n_mc, int sampling_ratio);
int runia_roi_mc_entropy_f32(const float* feat_nhwc, const float* boxes, const int* batch_idx, const float* rand,
                             int64_t rand_image_stride, double* h, float* z_out, void* workspace, size_t workspace_bytes,
                             int64_t K, int64_t B, int C, int H, int W, int PH, int PW, double spatial_scale,
                             int sampling_ratio, int aligned, int n_mc, double drop_prob, int block_size, int k,
                             double min_dist, runia_stream_t stream);
/* roi_align(...).mean((2, 3)) as ONE pass from the channels-last map (the per-box reduction of BoxInferenceYolo,
 * inference/object_level.py; _reduce_features_to_rois, feature_extraction/object_level.py:254-309): feat_nhwc [B, H, W, C]
 * (runia_nchw_to_nhwc_f32), boxes [K, 4] xyxy, batch_idx [K] or NULL (B == 1), roi_align's PH, PW, spatial_scale,
 * sampling_ratio, aligned -> out[k * ldo + col_offset + c] f32 for c < C: each hooked layer writes its own column slice of one
 * (K, C_total) matrix.  The (K, C, PH, PW) tensor is never written: the mean is the separable sum of per-axis bilinear
 * weights (f64) over the box's pixels.  A batch index outside [0, B) gives a row of zeros.  A non-finite pixel whose weight
 * for a box is exactly zero (every sample next to it on an integer coordinate) is unspecified: this form skips it, roi_align's
 * 0 * inf would not.  Limits: H + W <=
 * RUNIA_ROI_MEANS_MAX_HW, H * W * C * 4 < 2^30 bytes per image (RUNIA_E_INVALID otherwise); any K (K = 0: nothing).  No
 * workspace, no atomics. */
#define RUNIA_ROI_MEANS_MAX_HW 2048
int runia_roi_means_f32(const float* feat_nhwc, const float* boxes, const int* batch_idx, float* out, int64_t ldo,
                        int64_t col_offset, int64_t K, int64_t B, int C, int H, int W, int PH, int PW, double spatial_scale,
                        int sampling_ratio, int aligned, runia_stream_t stream);

/* Symmetric eigen-decomposition without a vendor solver: two-sided cyclic Jacobi, f64, parallel ordering.  What
 * scipy.linalg.pinvh (EmpiricalCovariance.fit, inference/postprocessors.py:213-220, inference/funcs.py:52-66), the
 * "covariance_eigh" / "full" PCA fit (dimensionality_reduction.py:70-71) and eigen_score (llm_uncertainty/scores.py:49-66)
 * need.  runia_eigh_init_f64: V = I, matrix norm.  runia_eigh_sweep_f64: ONE sweep in place (A -> J^T A J, V -> V J);
 * `rotations` (device, unsigned) grows by the number of rotations applied - the caller repeats the call until a sweep adds
 * none (typically 8-10 sweeps), then diag(A) holds the eigenvalues and the columns of V the eigenvectors.
 * A, V [n, n] f64 row-major (A symmetric, overwritten); workspace: runia_eigh_workspace_bytes(n), 16-byte aligned. */
size_t runia_eigh_workspace_bytes(int64_t n);
int runia_eigh_init_f64(const double* A, double* V, int64_t n, void* workspace, size_t workspace_bytes,
                        runia_stream_t stream);
int runia_eigh_sweep_f64(double* A, double* V, int64_t n, void* workspace, size_t workspace_bytes,
                         unsigned* rotations, runia_stream_t stream);
/* Blocked form of the same cyclic Jacobi method (csrc/eigh_block.hip): a sweep is (n/32 - 1) steps of two launches -
 * one 64 x 64 sub-problem per pair of 32-column blocks solved in LDS, then A <- R^T A R, V <- V R as 64^3 products on the
 * f64 matrix cores - instead of 2 (n - 1) launches of scalar rotations.  Works on PADDED matrices: N =
 * runia_eigh_block_padded(n) (an even number of whole blocks), A zero outside its n x n corner;
 * runia_eigh_block_init_f64(A, V, N, ...) first (V = I, norm in a fixed summation order), with a workspace of
 * runia_eigh_block_workspace_bytes(n) bytes, 16-byte aligned. */
int64_t runia_eigh_block_padded(int64_t n);
size_t runia_eigh_block_workspace_bytes(int64_t n);
int runia_eigh_block_init_f64(const double* A, double* V, int64_t N, void* workspace, size_t workspace_bytes,
                              runia_stream_t stream);
int runia_eigh_block_sweep_f64(double* A, double* V, int64_t N, void* workspace, size_t workspace_bytes,
                               unsigned* rotations, runia_stream_t stream);
/* C [M, N] = A [M, K] * B  (B [K, N], or B [N, K] read transposed when transpose_b != 0); f64, setup-time sizes. */
int runia_matmul_f64(const double* A, const double* B, double* C, int64_t M, int64_t N, int64_t K, int transpose_b,
                     runia_stream_t stream);
/* f4: Gram form of eigen_score's covariance: G [n, n] = Ec Ec^T / denom with Ec = E - column means, E [n, H] f32
 * (torch.cov(E.T) is Ec^T Ec / (n-1), [H, H] of rank < n: its non-zero spectrum is that of G). */
int runia_centred_gram_f32(const float* E, double* G, int64_t n, int64_t H, double denom, runia_stream_t stream);

/* ---- f2  metrics after the path (SURVEY 8f "next #2") -------------------------------------- *
 * AUROC, FPR@95 and AUPR of in-distribution (positive) against out-of-distribution scores as get_auroc_results
 * computes them (evaluation/metrics.py:37-100: torchmetrics binary auroc / roc / precision_recall_curve +
 * sklearn.metrics.auc): sigmoid in the dtype of the scores when any score is outside [0, 1], descending sort, one
 * curve point per run of equal scores, float32 curve points and trapezoid terms.  Device-resident: bucket sort + scans.
 *   ind_scores [n_ind], ood_scores [n_ood] (device), out3 [3] f64 (device) = {auroc, fpr@95, aupr} (float32 values);
 *   workspace: runia_ood_metrics_workspace_bytes(n_ind + n_ood) bytes, 256-byte aligned. */
size_t runia_ood_metrics_workspace_bytes(int64_t n_total);
int runia_ood_metrics_f64(const double* ind_scores, int64_t n_ind, const double* ood_scores, int64_t n_ood,
                          double* out3, void* workspace, size_t workspace_bytes, runia_stream_t stream);
int runia_ood_metrics_f32(const float* ind_scores, int64_t n_ind, const float* ood_scores, int64_t n_ood,
                          double* out3, void* workspace, size_t workspace_bytes, runia_stream_t stream);
/* The same launch sequence, additionally leaving torchmetrics' _binary_clf_curve on the device (what get_auroc_results'
 * roc / precision_recall_curve calls are built from, evaluation/metrics.py:70-81): tps / fps [n_ind + n_ood] u32 =
 * cumulative true / false positives at the end of every run of equal scores, descending score order; *n_points (device,
 * int64) = number of runs.  The caller copies n_points entries to the host and forms the float32 curves there. */
int runia_ood_clf_curve_f64(const double* ind_scores, int64_t n_ind, const double* ood_scores, int64_t n_ood,
                            double* out3, unsigned* tps, unsigned* fps, int64_t* n_points, void* workspace,
                            size_t workspace_bytes, runia_stream_t stream);
int runia_ood_clf_curve_f32(const float* ind_scores, int64_t n_ind, const float* ood_scores, int64_t n_ood,
                            double* out3, unsigned* tps, unsigned* fps, int64_t* n_points, void* workspace,
                            size_t workspace_bytes, runia_stream_t stream);

/* ---- (e) multi-GPU: one-shot all-gather of the score shards (SURVEY section 5's fallback for a latency-bound gather) -- *
 * The path's only exchange is the (N / world,) score shard of every rank to every rank, one per postprocessor call
 * (the reference has no distributed code).  Instead of a ring, every rank WRITES its shard into every peer's
 * receive buffer over xGMI (buffers mapped through HIP IPC) and raises a flag; a second launch waits for the world flags of
 * the step and copies the gathered vector out.  Stream-ordered, no host synchronisation; a wait that never sees a peer
 * gives up after timeout_ms and sets a status word (runia_p2p_status) instead of hanging.
 *   runia_p2p_alloc   : this rank's receive buffer (fine-grained device memory, zeroed), world <= 16
 *   runia_p2p_export  : its 64-byte HIP IPC handle (send it to the peers over any host channel)
 *   runia_p2p_open    : map a peer's buffer from its handle;  runia_p2p_close / runia_p2p_free: undo
 *   runia_p2p_all_gather(local_shard, shard_bytes, out [world * shard_bytes], peer_buffers [world] (HOST array of the
 *                       mapped device pointers, own buffer at index rank), ..., seq = 1, 2, 3, ... (+1 per call on every
 *                       rank; slots alternate, a slot is rewritten two calls later), timeout_ms, stream) */
size_t runia_p2p_buffer_bytes(int world, size_t shard_capacity_bytes);
int runia_p2p_alloc(int world, size_t shard_capacity_bytes, void** buffer);
int runia_p2p_free(void* buffer);
int runia_p2p_export(void* buffer, void* handle64);
int runia_p2p_open(const void* handle64, void** peer_buffer);
int runia_p2p_close(void* peer_buffer);
int runia_p2p_all_gather(const void* local_shard, size_t shard_bytes, void* out, void* const* peer_buffers, int world,
                         int rank, size_t shard_capacity_bytes, uint64_t seq, int timeout_ms, runia_stream_t stream);
int runia_p2p_status(void* buffer, int* status);
/* runia_p2p_debug(1): the launches that follow ASSERT the ordering argument slot reuse rests on - a writer reads, over the
 * link, the step its peer last copied out of the slot and expects exactly seq - 2; a mismatch sets bit 1 (value 2) of the
 * status word.  The acknowledgements themselves are always recorded, so the check may be switched on at any step of a live
 * buffer and by the ranks independently.  Returns the previous setting; off by default. */
int runia_p2p_debug(int on);

/* ---- f4  remaining logits/features postprocessors (SURVEY 8f "next #4") ------- *
 * runia_linear_f32: out [N, C] = min(x, clip_max) @ w.T + bias on the f32 matrix cores - the final linear layer
 *   that ReAct / ASH / DICE re-apply to (transformed) features (inference/postprocessors.py:1193, 1441, 1466;
 *   RouteDICE.forward inference/funcs.py:180-189 with the masked weight).  x [N, D], w [C, D] K-contiguous rows,
 *   bias [C] or NULL, clip_max = +inf for no clipping.  Energy = runia_row_lse_msp_f32 on `out`.
 * runia_ash_s_f32: ASH-S pruning + sharpening of 2-D activations (ash_s_linear_layer, inference/funcs.py:234-261).
 * runia_gen_score_f32: generalized_entropy(softmax(logits), gamma, M) (inference/funcs.py:347-375). */
int runia_linear_f32(const float* x, const float* w, const float* bias, float* out, int64_t N, int64_t D,
                     int64_t C, float clip_max, runia_stream_t stream);
int runia_ash_s_f32(const float* x, float* y, int64_t N, int64_t D, int percentile, runia_stream_t stream);
int runia_gen_score_f32(const float* logits, float* score, int64_t N, int64_t C, int M, double gamma,
                        runia_stream_t stream);
/* runia_gen_entropy_f32: generalized_entropy(probs, gamma, M) on rows that already are probabilities - the reference's
 *   free function (inference/funcs.py:347-375) as its own tests call it (tests/unit_test_baselines.py).
 * runia_mcd_uncertainty_f32: get_predictive_uncertainty_score / get_mcd_pred_uncertainty_score (inference/funcs.py:
 *   430-465, 378-427): logits [N * n_mc, C] f32, the n_mc rows of an image consecutive -> pred_h [N] = H[mean_s softmax],
 *   mi [N] = pred_h - mean_s H[softmax]; probs (optional) [N * n_mc, C] receives the softmax rows (the first value the
 *   dataloader form returns).  One launch: a wave per image with the rows in registers up to C = 4096; wider heads
 *   (ImageNet-21k, LLM vocabularies) a workgroup per image with the rows re-read from L2 (n_mc <= 4096 there).  The GEN entry
 *   points take any C the same way.
 * runia_ash_s_rows_f32: ASH-S for rows of any length - ash_s_conv_layer (inference/funcs.py:194-227) on the flattened
 *   (B, C*H*W) maps and ash_s_linear_layer beyond 4096 features.  y = pruned row * exp(sum / kept sum); `pruned`
 *   (optional, may be x itself: the reference's view + scatter_ prunes its argument in place) = the pruned row.
 *   keep_all_when_k_is_zero: NumPy's x[:, -0:] semantics (linear form) instead of torch.topk(k = 0) (conv form). */
int runia_gen_entropy_f32(const float* probs, float* score, int64_t N, int64_t C, int M, double gamma,
                          runia_stream_t stream);
int runia_mcd_uncertainty_f32(const float* logits, float* probs, float* pred_h, float* mi, int64_t N, int n_mc, int64_t C,
                              runia_stream_t stream);
int runia_ash_s_rows_f32(const float* x, float* y, float* pruned, int64_t N, int64_t D, int percentile,
                         int keep_all_when_k_is_zero, runia_stream_t stream);

/* ---- per-pixel uncertainty maps of a segmentation head ---------------------- *
 * get_predictive_uncertainty_score (inference/funcs.py:430-465), Energy.postprocess and MSP.postprocess
 * (inference/postprocessors.py:529-551, 586-608) for every pixel of G images from the logits of n_mc stochastic forward
 * passes, read where they lie.  (On a 4-D tensor the reference's function sums its expected-entropy term over W instead of
 * the classes; the definition taken is that function on one row per (image, pixel, sample).)
 *   table      DEVICE array of base pointers.  single == 0: n_mc pointers, pass s is a (G, C, H, W) block at table[s].
 *              single == 1: one pointer to a (G * n_mc, C, H, W) block whose rows g * n_mc + s are the samples of image g
 *              (torch.split(x, n_mc) order).  dtype 0 f32, 1 f16, 2 bf16 (the codes of runia_mcd_reduce_rows), widened
 *              exactly; all arithmetic in f32.
 *   sn sc sh sw element strides (>= 0) of the row, class, h and w dimensions, shared by all blocks: NCHW, channels_last
 *              (sc == 1) and sliced views are read in place.
 *   outputs    f32 (G, H, W) contiguous, each may be NULL, at least one set:
 *                pred_h    -sum_c pbar_c log pbar_c,  pbar = mean_s softmax_c(x_s)
 *                mi        pred_h - mean_s(-sum_c p_sc log p_sc)        (n_mc == 1: exactly 0, or NaN)
 *                msp       max_c pbar_c
 *                energy    mean_s logsumexp_c x_sc                       (unflipped)
 *                max_logit max_c mean_s x_sc
 *                label     int32 argmax_c pbar_c, lowest index on ties
 *                mean_probs  f32 (G, C, H, W) contiguous: pbar
 *              The arithmetic is runia_mcd_uncertainty_f32's: 0 * log 0 is NaN as in the reference's torch expression (a
 *              class more than ~104 below the maximum of a sample makes pred_h and mi of that pixel NaN); sums over classes
 *              in ascending class order inside one lane: run-to-run bit identical, no atomics.
 * One launch.  C <= 24 and no max_logit: logits and means in registers, every logit read once.  Otherwise two passes in the
 * launch (row statistics, then the classes; the logits are re-read from the caches); the statistics live in LDS up to
 * n_mc = 21 and beyond that in `workspace` (runia_pixel_maps_workspace_bytes, 0 when none is needed; 4-byte aligned;
 * RUNIA_E_WORKSPACE if missing or short).  Four pixels per lane and load (16 bytes f32, 8 bytes f16 / bf16) when w has unit
 * stride and the other strides and bases are multiples of four elements; element loads through the strides otherwise.
 * G, C, H, W < 2^31, G * H * W < 2^39, n_mc <= 2^20; RUNIA_E_INVALID otherwise.  G == 0 or H * W == 0: 0, nothing launched.
 *
 * runia_pixel_map_reduce_f32: per image the mean, max and count of the pixels of map (G, HW) f32 whose `valid` byte is
 *   non-zero (valid NULL: all) -> mean [G] f32, max [G] f32, count [G] int64 (each may be NULL, one set).  One workgroup
 *   per image, f64 partial sums in a fixed order: deterministic.  No valid pixel: NaN, -inf, 0.  A NaN pixel makes the mean
 *   NaN and is skipped by the max. */
size_t runia_pixel_maps_workspace_bytes(int64_t G, int64_t C, int64_t H, int64_t W, int n_mc, int want_max_logit);
int runia_pixel_uncertainty_maps(const void* const* table, int single, int dtype, int64_t G, int n_mc, int64_t C, int64_t H,
                                 int64_t W, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float* pred_h, float* mi,
                                 float* msp, float* energy, float* max_logit, int32_t* label, float* mean_probs,
                                 void* workspace, size_t workspace_bytes, runia_stream_t stream);
int runia_pixel_map_reduce_f32(const float* map, const uint8_t* valid, int64_t G, int64_t HW, float* mean, float* max,
                               int64_t* count, runia_stream_t stream);
/* runia_tril_inverse_f64: inv [batch, D, D] = inverse of the lower-triangular factors tril [batch, D, D] (row-major f64; the strict
 *   upper triangle of inv is zero).  Setup of the class-wise Gaussians of GMMLatentSpace / DDU (inference/postprocessors.py:
 *   426-492, 694-786; torch.distributions.MultivariateNormal keeps scale_tril): the precision of a class is inv^T inv. */
int runia_tril_inverse_f64(const double* tril, double* inv, int64_t batch, int64_t D, runia_stream_t stream);
/* runia_cholesky_*: a [batch, D, D] row-major, in place: the lower triangle of every matrix is replaced by its Cholesky factor L
 *   (a + jitter I = L L^T), the strict upper triangle by zeros; info[b] = 0, or j + 1 when the pivot of column j was not positive
 *   (LAPACK potrf's convention; the matrix is then partly overwritten).  f32: the factorisation inside torch's
 *   MultivariateNormal(covariance_matrix=...) that gmm_fit's jitter ladder retries (inference/funcs.py:310-342); f64: the factor
 *   of a precision matrix for runia_md_score_tril_*.  One fixed summation order: same bits from run to run. */
int runia_cholesky_f32(float* a, int* info, int64_t batch, int64_t D, double jitter, runia_stream_t stream);
int runia_cholesky_f64(double* a, int* info, int64_t batch, int64_t D, double jitter, runia_stream_t stream);
/* runia_select_hist_f32: one histogram pass of a radix select over a flat f32 array - hist [2048] (u32, cleared by the call) counts,
 *   among the elements whose order-preserving key k satisfies (k & prefix_mask) == prefix, the digit (k >> shift) & 2047.  Three
 *   passes (shift 21, 10, 0) give an exact order statistic; two neighbouring ones give np.percentile(train.flatten(), p), the
 *   clipping threshold of ReAct / DICE+ReAct (inference/postprocessors.py:1441, 1466).  n < 2^32; NaNs sort above +inf. */
int runia_select_hist_f32(const float* x, unsigned* hist, int64_t n, unsigned prefix, unsigned prefix_mask, int shift,
                          runia_stream_t stream);
/* runia_gmm_log_prob_f32: class-wise Gaussian log densities, all classes in one pass - replaces gmm.log_prob(x[:, None, :]) of
 *   the torch MultivariateNormal that gmm_fit builds (inference/funcs.py:265-344), as called by GMMLatentSpace.postprocess and
 *   DDU.postprocess (inference/postprocessors.py:490-491, 778-779), and the scipy logsumexp that follows it.
 *   x [N, D] f32; means [C, D] f32; w_tril [C, D, D] f32 row-major = L_c^-1, the inverse of torch's scale_tril, LOWER TRIANGULAR
 *   with exact zeros above the diagonal; consts [C] f64 = -D/2 log(2 pi) - sum log diag L_c.
 *   log_prob [N, C] f32 (optional) = consts[c] - 0.5 || w_c (x_n - means_c) ||^2, the difference formed in f32 as torch forms it,
 *   the products on the f32 matrix cores with only the k <= column half of w_c multiplied (D^2 flop per (row, class));
 *   lse [N] f32 (optional) = logsumexp over the classes of the f32 log_prob values (NaN in -> NaN).  At least one output.
 *   workspace: runia_gmm_log_prob_workspace_bytes(N, D, C) bytes, 8-byte aligned (per-column-tile sums of squares, f64); a smaller
 *   one is accepted as long as it holds 128 rows (the rows are then scored in chunks). */
size_t runia_gmm_log_prob_workspace_bytes(int64_t N, int64_t D, int C);
int runia_gmm_log_prob_f32(const float* x, const float* means, const float* w_tril, const double* consts, float* log_prob,
                           float* lse, void* workspace, size_t workspace_bytes, int64_t N, int64_t D, int C,
                           runia_stream_t stream);
/* runia_proj_norm_*: ViM residual norm || (x - u) @ NS ||_2 per row (inference/postprocessors.py:1106):
 *   x [N, D], u [D] (same dtype as x; f32 - f32 is rounded to f32 first, as NumPy), packed_ns = pack(NS [D, n]),
 *   norm [N] f64. */
int runia_proj_norm_f32(const float* x, const float* u, const double* packed_ns, double* norm, int64_t N,
                        int64_t D, int64_t n, runia_stream_t stream);
int runia_proj_norm_f64(const double* x, const double* u, const double* packed_ns, double* norm, int64_t N,
                        int64_t D, int64_t n, runia_stream_t stream);

/* ---- RAUQ  attention-based uncertainty of one LLM generation -------------- *
 * Replaces rauq_uncertainty / rauq_uncertainty_mean_heads / rauq_uncertainty_rollout / RAUQ
 * (llm_uncertainty/scores.py:155-344) and their helpers (llm_uncertainty/attention_aggregation.py).
 *   table  device array of n_gen * L map descriptors, step-major, 6 int64 each: {pointer to batch 0 of the step's
 *          (B, H, q, k) attention tensor, head stride, row stride, column stride (elements), k, q}.  The caller checks
 *          the shapes (the kernels trust the table): every step has H heads; "original" gathers need k >= 2 from step 1 on;
 *          rollout needs step 0 = (H, input_length or 1, input_length) and step g >= 1 = (H, 1, input_length + g).
 *   dtype  0 f32, 1 f16, 2 bf16 (all maps of one call).  token_agg 0 "original", 1 "mean_all_tokens".
 * runia_rauq_gather: w [L, H, N] f32, N = n_gen - 1 ("original": attn[0, h, 0, -2] of steps 1 .. n_gen-1) or n_gen
 *   ("mean_all_tokens": mean of query row 0 over k, formed in f32 and rounded to the map dtype).  One launch.
 * runia_rauq_score: one launch.  head_mode 0: per layer the head argmax_h mean(w[l, h, 1:]) (NaN counts as the maximum,
 *   the first index wins; heads [L] int32 receives it), 1: mean over heads, 2: att is one series [N] (rollout; L = H = 1).
 *   Then per layer and alpha conf[0] = exp(lp[0]), conf[i] = a exp(lp[i]) + (1 - a) att[i] conf[i-1] in f32 in the
 *   reference's order, u = -mean log conf; scores [n_alpha] f32 = max over layers.  log_probs [>= N] f32, alphas
 *   [n_alpha] f64.  workspace: runia_rauq_workspace_bytes(L, N, 0, 0, 0, n_alpha).
 * runia_rauq_rollout_rows: the row pass over every layer's T x T reconstructed map (T = input_length + n_gen): row sums
 *   of mean_h A + I and the diagonal / sub-diagonal of its row normalisation into the workspace; *upper_flag (device
 *   int) = 1 when some prompt-block entry above the diagonal is non-zero.  workspace as for runia_rauq_rollout_att.
 * runia_rauq_rollout_att: att [n] f32 of the rollout joint = A^_{L-1} ... A^_0 after the row pass:
 *   token_agg 0: joint.diagonal(-1)[-n:], token_agg 1: joint[:, -n:].mean(0).
 *   route 0: one pass over the diagonals (token_agg 0 and a clear upper_flag only); route 1: the chain over causal maps
 *   (clear upper_flag: prompt rows are read up to the diagonal); route 2: the chain over general maps.  The chain
 *   carries k = 1 (token_agg 1) or n (token_agg 0) rows.
 *   workspace: runia_rauq_workspace_bytes(L, n_gen, input_length, n, k, 1), k = 0 for route 0, 16-byte aligned. */
size_t runia_rauq_workspace_bytes(int64_t L, int64_t n_gen, int64_t input_length, int64_t n, int64_t chain_rows,
                                  int n_alpha);
int runia_rauq_gather(const void* table, int dtype, int64_t n_gen, int64_t L, int64_t H, int token_agg, float* w,
                      runia_stream_t stream);
int runia_rauq_score(const float* att, int64_t L, int64_t H, int64_t N, int head_mode, const float* log_probs,
                     const double* alphas, int n_alpha, float* scores, int* heads, void* workspace, size_t workspace_bytes,
                     runia_stream_t stream);
int runia_rauq_rollout_rows(const void* table, int dtype, int64_t n_gen, int64_t L, int64_t H, int64_t input_length,
                            int* upper_flag, void* workspace, size_t workspace_bytes, runia_stream_t stream);
int runia_rauq_rollout_att(const void* table, int dtype, int64_t n_gen, int64_t L, int64_t H, int64_t input_length,
                           int token_agg, int route, int64_t n, float* att, void* workspace, size_t workspace_bytes,
                           runia_stream_t stream);

/* ---- batched RAUQ  every row of a left-padded batch of generations ---------- *
 * Row b is scored as the runia_rauq_* calls score its own slices: step 0 [b, :, pad_b:, pad_b:], step g >= 1
 * [b, :, :, pad_b:] for g < n_b, with input_length - pad_b as its input length (llm_uncertainty.rauq_batch).
 *   table  device array of n_gen * L descriptors, step-major, 7 int64 each: {pointer to batch 0 of the step's (B, H, q, k)
 *          tensor, batch stride, head stride, row stride, column stride (elements), k, q}.  Shapes as for runia_rauq_*,
 *          with k = input_length at step 0 and input_length + g at step g; a step 0 of one query row only without padding.
 *   rows   device array of B {pad_b, n_b} int64 pairs, 0 <= pad_b < input_length, 1 <= n_b <= n_gen (the kernels trust
 *          it; runia_rauqb_rollout_att checks host_rows, its host copy).
 * Outputs keep the one-row summation orders, roundings and fixed-order chain reductions, so row b's bits equal the one-row
 * calls' on its slices and depend on that row alone.
 * runia_rauqb_gather: w [B, L, H, N] f32, N = n_gen - 1 (token_agg 0) or n_gen; row b fills N_b = n_b - 1 or n_b tokens.
 * runia_rauqb_score: one workgroup per row.  att [B, L, H, N] (head_mode 0 / 1) or [B, N] (head_mode 2, L = H = 1);
 *   log_probs row b at log_probs + b * lp_stride; scores [B, n_alpha] f32.  A row with N_b < 1, or n_b < 2 for head_mode
 *   2, gets NaN (its one-row call raises).  workspace: runia_rauqb_workspace_bytes(B, L, N, 0, 0, n_alpha).
 * runia_rauqb_rollout_rows: the row pass of every row with n_b >= 2 over its T_b = input_length - pad_b + n_b rows;
 *   upper_flags [B] device int.  workspace: runia_rauqb_workspace_bytes(B, L, n_gen, input_length, 0, 1) or larger.
 * runia_rauqb_rollout_att: att [B, n_gen] f32, row b's n_b values first.  host_upper is the host copy of upper_flags.
 *   token_agg 0: one launch over the rows with a clear flag (one pass), the n_b-row chain for the others; token_agg 1: the
 *   1-row chain (causal or general, by the flag).  Chains run row after row in one workspace, each the one-row chain
 *   over the row's own map table, which one small launch writes into the workspace first:
 *   runia_rauqb_workspace_bytes(B, L, n_gen, input_length, k, 1), k the largest chain's rows (0 when there is none). */
size_t runia_rauqb_workspace_bytes(int64_t B, int64_t L, int64_t n_gen, int64_t input_length, int64_t chain_rows,
                                   int n_alpha);
int runia_rauqb_gather(const void* table, const void* rows, int dtype, int64_t B, int64_t n_gen, int64_t L, int64_t H,
                       int token_agg, float* w, runia_stream_t stream);
int runia_rauqb_score(const float* att, const void* rows, int64_t B, int64_t L, int64_t H, int64_t N, int head_mode,
                      int token_agg, const float* log_probs, int64_t lp_stride, const double* alphas, int n_alpha,
                      float* scores, void* workspace, size_t workspace_bytes, runia_stream_t stream);
int runia_rauqb_rollout_rows(const void* table, const void* rows, int dtype, int64_t B, int64_t n_gen, int64_t L, int64_t H,
                             int64_t input_length, int* upper_flags, void* workspace, size_t workspace_bytes,
                             runia_stream_t stream);
int runia_rauqb_rollout_att(const void* table, const void* rows, const int64_t* host_rows, const int* upper_flags,
                            const int* host_upper, int dtype, int64_t B, int64_t n_gen, int64_t L, int64_t H,
                            int64_t input_length, int token_agg, float* att, void* workspace, size_t workspace_bytes,
                            runia_stream_t stream);

/* ---- logit scores  per-token log-probabilities and entropies of an LLM generation -------------------------- *
 * Replaces HuggingFace model.compute_transition_scores(sequences, scores, normalize_logits) as compute_uncertainties calls it
 * (llm_uncertainty/scores.py:452-456, 495-499), generation_entropy's softmax per step (scores.py:135-152, utils.py:83-99),
 * perplexity and normalized_entropy (scores.py:69-85, 121-132), for every row of a generate() output in one pass.
 *   table   device array of n_steps step descriptors, 2 int64 each: {pointer to row 0 of the step's (B, V) or (B, 1, V)
 *           logits, row stride (elements)}.  The vocabulary axis has unit stride.  dtype 0 f32, 1 f16, 2 bf16 (one per call).
 *   tokens  int64, row b of the generated token ids at tokens + b * token_stride (>= n_steps when B > 1), each in [0, V)
 *           (the caller checks the range: the kernels trust it).  Needed for log_prob only.
 * Outputs (any may be NULL, not all), [B, n_steps] f32 row-major:
 *   lse       log-sum-exp of the row;
 *   log_prob  x[tok] - lse (normalize != 0) or x[tok];  a -inf logit gives -inf exactly;
 *   entropy   -sum p log p / log V with p = softmax(x), as H = log1p(s') + u / (1 + s') from the max m, s' = sum e^(x-m)
 *             without the max's own term and u = sum e^(x-m) (m - x): no cancellation.  The reference's clamp of p at 1e-12
 *             (at most V e^-1 1e-12 nats) is not applied.
 *   A row holding NaN or +inf, or only -inf, gives NaN in lse, entropy and the normalised log_prob.
 *   seq       [3B + 1] f64 (needs log_prob and entropy): mean over steps of entropy (generation entropy), -mean of log_prob
 *             (perplexity), the mean of the log_prob values that are not -inf, then normalized_entropy = -mean over rows of
 *             those means.
 * Rows are split into chunks of 4 096 logits, one workgroup each; partials merge in chunk order (f64), no atomics: two calls
 * give equal bits and a row's outputs depend on its own logits only.  Three launches (two without seq), no synchronisation.
 * workspace: runia_logit_stats_workspace_bytes(n_steps, B, V) bytes, 16-byte aligned (16 bytes per row and chunk); 0 for
 * sizes the kernels do not take. */
size_t runia_logit_stats_workspace_bytes(int64_t n_steps, int64_t B, int64_t V);
int runia_logit_stats(const void* table, int dtype, int64_t n_steps, int64_t B, int64_t V, const int64_t* tokens,
                      int64_t token_stride, int normalize, float* lse, float* log_prob, float* entropy, double* seq,
                      void* workspace, size_t workspace_bytes, runia_stream_t stream);

/* ---- batched eigen_score (llm_uncertainty/scores.py:49-66, utils.py:102-117; csrc/eigen_score.hip) --------
 * runia_eigen_score_batch: e holds groups * k rows of `hidden` values, dtype 0 f32, 1 f16, 2 bf16, unit column stride,
 *   row_stride elements between rows (hidden_states[-1][layer] of generate(num_return_sequences=k), read in place).
 *   out[g] (f64) = [sum over the top min(k, hidden) eigenvalues lambda of the centred Gram matrix Ec Ec^T / (k - 1) of rows
 *   g*k .. g*k+k-1 of log(max(lambda, 0) + alpha) + (hidden - min(k, hidden)) log(alpha)] / hidden.
 *   One workgroup per group, one launch, no synchronisation: f64 column means and products, cyclic Jacobi in LDS until a
 *   sweep applies no rotation (NaN after 30 sweeps).  No atomics: a group's bits do not depend on the other groups.
 *   2 <= k <= 64, hidden > 0, row_stride >= 0, 1 <= groups < 2^31; RUNIA_E_INVALID otherwise.  No workspace. */
int runia_eigen_score_batch(const void* e, int dtype_code, int64_t groups, int64_t k, int64_t hidden, int64_t row_stride,
                            double alpha, double* out, runia_stream_t stream);

/* ---- open-set object detection evaluation (evaluation/open_set.py; csrc/open_set.hip) --------------------
 * quantize: out[i] = float(f"{v:.{decimals}f}") of v = x[i] (+1 in x's own dtype when bit (i % period) of add_one_mask is
 *   set: process()'s xmin + 1, ymin + 1).  dtype 0 f32, 1 f64, 2 int32, 3 int64.  key_out (nullable): key_max - k with
 *   k = v * 10^decimals rounded half-to-even, the descending-confidence sort key; a k outside [0, key_max] sets *bad to 1.
 * bucket_sort: stable ascending counting sort of keys in [0, nb), nb <= 8192: perm[j] = input index of output j,
 *   bucket_start[nb + 1] (int64) = first output of each bucket.  Workspace: runia_osod_sort_workspace_bytes(n, nb).
 * overlaps: per detection (f64 quantised boxes [n, 4]) the (ovmax, jmax) of the reference IoU against the ground truth of
 *   group det_group[d] and of unk_group in image det_img[d] (-1: not annotated -> -inf, -1).  gt_off[n_groups * n_img + 1]:
 *   ground-truth boxes [.., 4] f64 ordered by (group, image).  ov [n, 2] f64, jpos [n, 2] int32 (global positions).
 * match: per (method m, sorted position p) with d = perm[p]: class c = K (= n_classes - 1) when relabelled (open_set:
 *   label == unk_label; else mscore[m, d] < thr[m], both already in the comparison dtype), else label; c = n_classes when
 *   c is out of range or conf[d] >= min_conf fails (conf nullable).  key[m, p] = m * (n_classes + 1) + c; flags[m, p]:
 *   1 TP, 2 FP, 0 skipped, | 4 when the unknown overlap exceeds ovthresh.  A candidate (ovmax > ovthresh) is a TP when no
 *   earlier candidate of the same (m, c, ground-truth slot) exists; slot = cbase[c] + jpos - gstart[group_of_class[c]].
 *   Workspace: runia_osod_match_workspace_bytes(n_methods, n_slots).
 * gtu_keys: GTU / UU partition keys from a one-method match: c for rows overlapping unknown ground truth, n_classes + c for
 *   the others, 2 n_classes for rows not evaluated.
 * gather_f64: out[i] = src[idx1[idx0[i]]] (idx1 nullable: src[idx0[i]]).
 * curves: one workgroup per (method, class) segment of bucket_start (from bucket_sort of match's keys; part = its perm):
 *   summary [n_methods, n_classes, 8] f64 = {ap, rec[-1], prec[-1], tp+fp and fp_os at the first argmin |rec - 0.8|,
 *   open-set FP count, max(tp+fp), rows}; rec / prec / tpfp / fpos (nullable, all or none) [n_methods * n] at partition
 *   positions.  use_07: 11-point AP.  Workspace: runia_osod_curves_workspace_bytes(n_methods * n).
 * No float atomics anywhere: two calls give equal bits. */
int runia_osod_quantize(const void* x, int dtype, int64_t n, int period, unsigned add_one_mask, int decimals, double* out,
                        int32_t* key_out, int key_max, int32_t* bad, runia_stream_t stream);
size_t runia_osod_sort_workspace_bytes(int64_t n, int nb);
int runia_osod_bucket_sort(const int32_t* keys, int64_t n, int nb, int32_t* perm, int64_t* bucket_start, void* workspace,
                           size_t workspace_bytes, runia_stream_t stream);
int runia_osod_overlaps(const double* boxes, const int32_t* det_img, const int32_t* det_group, int64_t n,
                        const double* gt_boxes, const int32_t* gt_off, int n_img, int n_groups, int unk_group, double* ov,
                        int32_t* jpos, runia_stream_t stream);
size_t runia_osod_match_workspace_bytes(int n_methods, int64_t n_slots);
int runia_osod_match(const int32_t* perm, int64_t n, int n_methods, int n_classes, const int32_t* label,
                     const int32_t* det_img, const double* ov, const int32_t* jpos, const double* mscore, const double* thr,
                     int open_set, int unk_label, const double* conf, double min_conf, const int32_t* group_of_class,
                     const int32_t* gstart, const int64_t* cbase, int64_t n_slots, double ovthresh, int32_t* key,
                     uint8_t* flags, void* workspace, size_t workspace_bytes, runia_stream_t stream);
int runia_osod_gtu_keys(const int32_t* key, const uint8_t* flags, int64_t n, int n_classes, int32_t* out,
                        runia_stream_t stream);
int runia_osod_gather_f64(const double* src, int64_t n_src, const int32_t* idx0, const int32_t* idx1, int64_t n, double* out,
                          runia_stream_t stream);
size_t runia_osod_curves_workspace_bytes(int64_t rows);
int runia_osod_curves(const int32_t* part, const int64_t* bucket_start, const uint8_t* flags, int64_t n, int n_methods,
                      int n_classes, const int64_t* npos, int use_07, double* summary, double* rec, double* prec,
                      double* tpfp, double* fpos, void* workspace, size_t workspace_bytes, runia_stream_t stream);

/* ---- greedy NMS and the YOLOv8 candidate filter (nms.hip) ------------------------------------------------------------ *
 * torchvision.ops.nms, which ObjectDetectionExtractor.yolo_get_logits calls (feature_extraction/abstract_classes.py:606-715).
 *
 * runia_yolo_candidates_f32: one image's head pred [4 + nc + nm, A] f32, channel-major (row r of anchor a at r * A + a).
 *   Per anchor: best = max of the nc class rows, j = the first class index reaching it; candidate when no class score is
 *   NaN, best > conf_thres (strict) and, when n_classes > 0, (float)j equals one of classes[n_classes] (f32).  The
 *   candidates are compacted in anchor order (deterministic: no atomics) into cand_boxes [A, 4] = rows 0-3 + j * max_wh
 *   (f32; max_wh = 0 for class-agnostic NMS), cand_scores [A] = best, cand_anchor [A], cand_cls [A]; *count (int64) = their
 *   number.  Rows 0-3 are taken as they are (xyxy in the reference's reading).  A <= RUNIA_YOLO_MAX_ANCHORS.
 *   Workspace: runia_yolo_candidates_workspace_bytes(A) = 8 * A + 4 * ceil(A / 256).
 * runia_nms_keys_f32: keys[i] = (desc(scores[i]) << 31) | i, int64, desc = the order-reversing uint32 image of the f32 score
 *   (-0 folded onto +0); a NaN score - either sign, any payload - has desc = 0, the one value in front of +inf's that no
 *   other score takes.  Ascending keys = descending score with every NaN first, ties and NaNs by ascending index: the
 *   order of torch.sort(descending=True, stable=True).
 * runia_nms_sort_keys: sorts n <= RUNIA_NMS_SORT_MAX keys in place (one workgroup, LDS bitonic sort).  Longer lists may be
 *   sorted by any device sort of the same keys: they are distinct, so the order is the same.
 * runia_nms_sorted_f32: boxes [*, 4] xyxy f32 indexed by key & 0x7fffffff; the first m sorted keys (m <=
 *   RUNIA_NMS_MAX_BOXES) are walked greedily: a box is kept unless a kept box before it has IoU > iou_threshold with it
 *   (torchvision's f32 expression and order; a 0/0 IoU suppresses nothing).  keep[0 : *count] (int64) = the kept boxes'
 *   indices in sorted order, at most max_det of them.  Workspace: runia_nms_workspace_bytes(m) = m * ceil(m / 64) * 8 (the
 *   IoU bitmask). */
#define RUNIA_YOLO_MAX_ANCHORS (1 << 22)
#define RUNIA_NMS_SORT_MAX 4096
#define RUNIA_NMS_MAX_BOXES 65536
size_t runia_yolo_candidates_workspace_bytes(int64_t A);
int runia_yolo_candidates_f32(const float* pred, int64_t A, int nc, int nm, float conf_thres, const float* classes,
                              int n_classes, float max_wh, float* cand_boxes, float* cand_scores, int* cand_anchor,
                              int* cand_cls, int64_t* count, void* workspace, size_t workspace_bytes, runia_stream_t stream);
int runia_nms_keys_f32(const float* scores, int64_t n, int64_t* keys, runia_stream_t stream);
int runia_nms_sort_keys(int64_t* keys, int64_t n, runia_stream_t stream);
size_t runia_nms_workspace_bytes(int64_t m);
int runia_nms_sorted_f32(const float* boxes, const int64_t* sorted_keys, int64_t m, float iou_threshold, int64_t max_det,
                         int64_t* keep, int64_t* count, void* workspace, size_t workspace_bytes, runia_stream_t stream);

/* ---- PaCMAP embedding (pacmap.hip) ---------------------------------------------------------------------------------- *
 * The device half of runia_core_amd.embedding.PaCMAP (the reference's fit_pacmap / apply_pacmap_transform /
 * plot_samples_pacmap on pacmap==0.7.0, dimensionality_reduction.py:88-177).
 *
 * runia_pacmap_knn_f32: exact kNN of q [Q, D] among bank [N, D] (f32, row-major).  Squared distance = the f32 sum over the
 *   columns in order of (q - b)^2 (fma); lists sorted by (squared distance, bank index) ascending.  exclude_self: bank row i
 *   is left out of query row i's list by index (the fit, q == bank; duplicates of the row stay, at distance 0).
 *   idx [Q, K] int32, dist [Q, K] f32 = sqrt of the squared distance.  1 <= K <= RUNIA_PACMAP_MAX_K, K <= N - exclude_self,
 *   N < 2^31; RUNIA_E_INVALID otherwise.  No workspace.
 * runia_pacmap_pairs: the pair lists of R rows x [R, D] against bank [Nb, D] from their kNN table knn_idx / knn_dist [R, K]
 *   (runia_pacmap_knn_f32).  Fit (transform = 0; x = bank, R = Nb): sig_i = max(mean(dist_i[3 : min(6, K)]), 1e-10)
 *   (1e-10 when K <= 3); the n_nb candidates with the smallest (dist^2 / sig_i) / sig_j (f32; ties: earlier candidate) ->
 *   pair_nb [R * n_nb, 2] = (i, j) in that order; n_mn MN pairs per row -> pair_mn [R * n_mn, 2]: the second closest
 *   (squared distance as in the kNN, ties: earlier draw) of 6 uniform draws among the other rows; n_fp FP pairs -> pair_fp
 *   [R * n_fp, 2]: distinct uniform rows that are neither the row nor an NB partner.  Transform (transform = 1, n_mn = 0): NB
 *   = the first n_nb candidates, FP rows are not NB partners (the row itself is a bank row like any other).  Draws:
 *   Philox4x32-10, counter (row, (kind << 16) | slot, candidate, attempt), key (seed.lo, seed.hi), word 0; kind 0 = MN,
 *   1 = FP; index = floor(u32 * M / 2^32) with M = Nb - 1 for MN (j' -> j' + (j' >= row)) and M = Nb for FP (a rejected
 *   draw takes the next attempt).  Limits: n_nb <= K <= RUNIA_PACMAP_MAX_K, n_mn <= RUNIA_PACMAP_MAX_MN, n_fp <=
 *   RUNIA_PACMAP_MAX_FP and <= Nb - n_nb - (1 for the fit), rows <= RUNIA_PACMAP_MAX_ROWS.  Workspace (fit only):
 *   runia_pacmap_pairs_workspace_bytes(R) = 4 * R.
 * runia_pacmap_phase_weights: w[3] = (w_NB, w_MN, w_FP) of iteration t (t < 100: 2, (1 - t/100) 1000 + (t/100) 3, 1;
 *   t < 200: 3, 3, 1; then 1, 0, 1), f32.  Host only.
 * runia_pacmap_step_f32: one Adam iteration t (beta1 0.9, beta2 0.999, eps 1e-7, lr_t = lr sqrt(1 - beta2^(t+1)) /
 *   (1 - beta1^(t+1))) of the R rows y_in [R, C] -> y_out [R, C] (a different buffer), m / v [R, C] updated in place.  Row
 *   r's pairs are entries[offsets[r] : offsets[r+1]] (offsets [R + 1] int64), each (kind << 30) | partner with kind
 *   RUNIA_PACMAP_KIND_*; the partner's coordinates are y_part[partner] (= y_in for a fit, the frozen fitted rows for a
 *   transform).  With d = 1 + |y_r - y_p|^2 the gradient is w (y_r - y_p) summed over the entries: NB w = w_NB 20 /
 *   (10 + d)^2, MN w = w_MN 2e4 / (1e4 + d)^2, FP w = -w_FP 2 / (1 + d)^2 (the kind fixes the sign).  Fixed summation order
 *   (no atomics): the same inputs give the same bits.  1 <= C <= RUNIA_PACMAP_MAX_COMPONENTS.  No workspace. */
#define RUNIA_PACMAP_MAX_K 192
#define RUNIA_PACMAP_MAX_MN 128
#define RUNIA_PACMAP_MAX_FP 256
#define RUNIA_PACMAP_MAX_COMPONENTS 16
#define RUNIA_PACMAP_MAX_ROWS (1 << 30)
#define RUNIA_PACMAP_KIND_NB 0
#define RUNIA_PACMAP_KIND_MN 1
#define RUNIA_PACMAP_KIND_FP 2
int runia_pacmap_knn_f32(const float* q, int64_t Q, const float* bank, int64_t N, int64_t D, int K, int exclude_self,
                         int32_t* idx, float* dist, runia_stream_t stream);
size_t runia_pacmap_pairs_workspace_bytes(int64_t R);
int runia_pacmap_pairs(const float* x, int64_t R, const float* bank, int64_t Nb, int64_t D, const int32_t* knn_idx,
                       const float* knn_dist, int K, int n_nb, int n_mn, int n_fp, uint64_t seed, int transform,
                       int32_t* pair_nb, int32_t* pair_mn, int32_t* pair_fp, void* workspace, size_t workspace_bytes,
                       runia_stream_t stream);
int runia_pacmap_phase_weights(int t, float* w);
int runia_pacmap_step_f32(const float* y_in, const float* y_part, float* y_out, float* m, float* v, const int64_t* offsets,
                          const int32_t* entries, int64_t R, int n_components, int t, float lr, runia_stream_t stream);

/* ---- MaxLogit, KL-Matching, fDBD (logit_baselines.hip; inference/extended_postprocessors.py) ------------------ *
 * Baselines the reference does not ship; the definitions are restated in f64 in tests/extended_baseline_cases.py.
 *
 * runia_row_logit_stats_f32: one pass over logits [N, C] f32.  Any output pointer may be NULL (not all four).
 *     max_logit   f32 [N]  the row maximum (NaN entries are skipped, as by fmaxf)
 *     lse         f32 [N]  scipy.special.logsumexp of the row, the arithmetic of runia_row_lse_msp_f32
 *     neg_entropy f32 [N]  sum_k p_k log p_k, p = softmax(row).  A class with p_k == 0 (a logit of -inf, or more than ~104
 *                          below the maximum) contributes 0 - NOT the 0 * log 0 = NaN of pred_h in
 *                          runia_mcd_uncertainty_f32 / runia_pixel_uncertainty_maps.  A NaN logit makes lse and neg_entropy NaN.
 *     argmax      i32 [N]  first index of the maximum (np.argmax on rows without NaN)
 *   Launch shapes of runia_row_lse_msp_f32: C <= 16 a row per lane in registers, C <= 64 a row per lane through LDS, beyond
 *   that a wave per row (16-byte loads and the row in registers for C % 4 == 0, aligned, C <= 2048; re-read otherwise).
 *   Sums in a fixed order that does not depend on N or on the row's place in the batch: bit identical from run to run.
 * runia_klm_score_f32: score[n] = max over classes c with valid[c] != 0 of sum_k p[n, k] log_q[c, k], minus neg_entropy[n],
 *   with p[n, k] = exp(logits[n, k] - lse[n]): -min_c KL(softmax(logits[n]) || q_c).  logits [N, C], log_q [K, C] f32
 *   row-major, lse / neg_entropy [N] (runia_row_logit_stats_f32), valid [K] int32 or NULL (all classes), score [N] f32.
 *   The N x C x K contraction runs on the f32 matrix cores (k-ordered fma chains); neither p nor the N x K products are
 *   written.  No atomics, no workspace; a row's score does not depend on the other rows of the call.  A NaN product makes
 *   the row NaN; no valid class gives -inf.  N < 2^38.
 * runia_fdbd_score_f32: with c = first argmax of logits[n]: score[n] = (sum over k != c of |logits[n, c] - logits[n, k]| *
 *   inv_dist[c, k]) / ((C - 1) * feat_dist[n]).  inv_dist [C, C] f32 (1 / ||w_c - w_k||_2, 0 where the norm is 0), feat_dist
 *   [N] f32.  IEEE results as they fall (feat_dist == 0: inf, or NaN for a zero sum).  A wave per row, the row in registers
 *   up to C = 4096, re-read beyond.  C >= 2.
 * runia_row_dist_f32: out[n] = || x[n] - mu ||_2, x [N, D], mu [D], f32. */
int runia_row_logit_stats_f32(const float* logits, float* max_logit, float* lse, float* neg_entropy, int32_t* argmax,
                              int64_t N, int64_t C, runia_stream_t stream);
int runia_klm_score_f32(const float* logits, const float* lse, const float* neg_entropy, const float* log_q,
                        const int32_t* valid, float* score, int64_t N, int64_t C, int64_t K, runia_stream_t stream);
int runia_fdbd_score_f32(const float* logits, const float* inv_dist, const float* feat_dist, float* score, int64_t N,
                         int64_t C, runia_stream_t stream);
int runia_row_dist_f32(const float* x, const float* mu, float* out, int64_t N, int64_t D, runia_stream_t stream);

/* ---- Confidence calibration (calibration.hip; evaluation/calibration.py) ------------------------------------- *
 * runia_calib_rows: one read of logits [N, C] (row-contiguous; `dtype` 0 f32, 1 f16, 2 bf16, widened exactly, f32 arithmetic)
 *   at the temperature 1 / beta (0 < beta < inf).  labels [N] int32 (labels_i64 == 0) or int64, or NULL (no labels: pred and
 *   conf only; the other four pointers must be NULL).  With m = max_k x_k, d_k = x_k - m, p = softmax(beta x) and y the label:
 *     pred  i32 [N]  first index of the maximum (np.argmax on rows without NaN)
 *     conf  f32 [N]  1 / sum_k exp(beta d_k) = max_k p_k
 *     nll   f32 [N]  log sum_k exp(beta d_k) - beta d_y          (+inf for x_y = -inf)
 *     brier f32 [N]  sum_k p_k^2 - 2 p_y + 1
 *     g     f32 [N]  sum_k p_k d_k - d_y                          = d nll / d beta
 *     h     f32 [N]  max(0, sum_k p_k d_k^2 - (sum_k p_k d_k)^2)  = d2 nll / d beta2
 *   Any output pointer may be NULL (not all six).  A class at -inf contributes 0; a NaN logit (and a row without a finite
 *   logit) makes the row's five float outputs NaN.  A row whose label equals ignore_index (has_ignore != 0) writes pred and
 *   NaN elsewhere; so does a label outside [0, C) - callers validate labels, the kernel only never reads through one.
 *   Launch shapes (the same for the three dtypes, so a 16-bit call gives the bits of the f32 call on the widened values):
 *   C <= 16 a row per lane in registers; C <= 64 a row per lane through LDS; beyond, a wave per row: C % 4 == 0 and the base
 *   aligned to four elements: four elements per lane and load, the row in registers up to C = 2048 (1, 2, 4 or 8 loads per
 *   lane); longer or unaligned rows in ONE chunked pass that rescales its sums when the running maximum moves.  Sums in a
 *   fixed order that depends on C alone: bit identical from run to run and wherever the row sits in the batch.  C < 2^31.
 * runia_calib_reduce_f32: the per-row table -> out, (6 + 3 n_bins) 8-byte slots:
 *     [0] n_used  [1] n_correct (int64)   [2] sum nll  [3] sum brier  [4] sum g  [5] sum h (f64)
 *     [6 ..) count[n_bins]  n_correct[n_bins] (int64)  conf_sum[n_bins] (f64)
 *   over the rows whose label is not ignore_index, with the bin b = clamp((int)ceilf(conf * (float)n_bins) - 1, 0, n_bins - 1)
 *   (f32 arithmetic; a NaN conf counts in bin 0).  nll, brier, g, h, pred may be NULL (their sums / counts stay 0); conf may be
 *   NULL when n_bins == 0.  0 <= n_bins <= 512.  Two launches: per-workgroup partials over contiguous row ranges (f64 sums in a
 *   fixed order, integer counts), then one pass that adds the partials in order - no floating-point atomics, the same inputs give
 *   the same bits.  workspace: runia_calib_reduce_workspace_bytes(N, n_bins) bytes (RUNIA_E_WORKSPACE if short).  N == 0: zeros. */
int runia_calib_rows(const void* logits, int dtype, const void* labels, int labels_i64, int has_ignore, int64_t ignore_index,
                     float beta, int32_t* pred, float* conf, float* nll, float* brier, float* g, float* h, int64_t N, int64_t C,
                     runia_stream_t stream);
size_t runia_calib_reduce_workspace_bytes(int64_t N, int n_bins);
int runia_calib_reduce_f32(const int32_t* pred, const float* conf, const float* nll, const float* brier, const float* g,
                           const float* h, const void* labels, int labels_i64, int has_ignore, int64_t ignore_index, int64_t N,
                           int n_bins, void* out, void* workspace, size_t workspace_bytes, runia_stream_t stream);

/* ---- Conformal prediction sets (conformal.hip; evaluation/conformal.py) -------------------------------------- *
 * logits [N, C], row r at logits + r * row_stride elements (row_stride >= C); `dtype` 0 f32, 1 f16, 2 bf16, widened exactly,
 * f32 arithmetic.  Per row, with m = max_k x_k, e_k = exp(beta (x_k - m)), S0 = sum e_k, p_k = e_k / S0 (0 < beta < inf):
 *   order : classes by logit, descending; equal logits by lower class index first (the stable argsort of -x)
 *   r_c   : the 1-based rank of class c;  B_c: the sum of p_k over the classes ordered before c
 *   method 0 lac : s_c = 1 - p_c
 *          1 aps : s_c = B_c + u p_c
 *          2 raps: s_c = B_c + u p_c + lam * max(0, r_c - k_reg)        (lam >= 0, k_reg >= 0)
 *   u f32 [N] in [0, 1], one number per row; NULL: u = 1.
 * A class at -inf has p = 0 and is ordered last.  A row with a NaN or +inf logit, or without a finite logit, has no softmax:
 * NaN scores, rank 0, size 0, no members, not covered.  labels [N] int32 (labels_i64 == 0) or int64; a row whose label equals
 * ignore_index (has_ignore != 0) or lies outside [0, C) gets a NaN score, rank 0, covered 0 - callers validate labels.
 * runia_conformal_label_scores: score f32 [N] = s_y and rank i32 [N] = r_y (either may be NULL) from one read of the logits and
 *   no sort: B_y = sum_k p_k [x_k > x_y or (x_k == x_y and k < y)].  C <= 64 a row per lane through LDS; beyond, a wave per row,
 *   four consecutive classes per lane and load (one aligned load when C % 4 == 0, row_stride % 4 == 0 and the base is aligned to
 *   four elements, four guarded loads otherwise: the same sums either way), the row in registers up to C = 2048, ONE chunked pass
 *   that rescales its sums when the running maximum moves beyond.  C < 2^31 - 2048.
 * runia_conformal_sets: the set {c : s_c <= qhat} (f32 compare; qhat = +inf: every class) of every row.  size i32 [N]; members
 *   i32 [N, ceil(C / 32)] or NULL, bit c % 32 of word c / 32 is class c; covered u8 [N] or NULL (needs labels): the label's bit.
 *   size is the population count of the row's words.  The row is ordered inside the workgroup (a bitonic network on (key, index)
 *   in LDS; lac skips it), the logits are read once and nothing [N, C] is written.  1 <= C <= runia_conformal_max_classes()
 *   (8192), RUNIA_E_INVALID beyond.
 * Both: sums in a fixed order that depends on C alone - the same bits from run to run, wherever the row sits in the batch, and
 *   for a 16-bit call the bits of the f32 call on the widened values.
 * runia_conformal_reduce: size / covered / labels -> out, runia_conformal_record_slots(C) = 3 + H + 2 C int64 slots, H = min(C + 1, 512):
 *     [0] rows used  [1] rows covered  [2] sum of sizes  [3 ..) hist[H] (the last slot: that size or more)
 *     class_count[C]  class_covered[C]
 *   over the rows whose label lies in [0, C) and is not ignore_index.  Integer atomics only: exact in any order.  N == 0: zeros. */
int runia_conformal_max_classes(void);
int runia_conformal_label_scores(const void* logits, int dtype, int64_t row_stride, const void* labels, int labels_i64,
                                 int has_ignore, int64_t ignore_index, const float* u, int method, float beta, float lam,
                                 int k_reg, float* score, int32_t* rank, int64_t N, int64_t C, runia_stream_t stream);
int runia_conformal_sets(const void* logits, int dtype, int64_t row_stride, const void* labels, int labels_i64, int has_ignore,
                         int64_t ignore_index, const float* u, int method, float beta, float lam, int k_reg, float qhat,
                         int32_t* size, int32_t* members, uint8_t* covered, int64_t N, int64_t C, runia_stream_t stream);
int64_t runia_conformal_record_slots(int64_t C);
int runia_conformal_reduce(const int32_t* size, const uint8_t* covered, const void* labels, int labels_i64, int has_ignore,
                           int64_t ignore_index, int64_t N, int64_t C, void* out, runia_stream_t stream);

/* ---- Conformal sets of rows of any width (conformal_wide.hip; llm_uncertainty/conformal.py) ------------------- *
 * The sets of runia_conformal_sets - the same definitions, methods, u, qhat and labels - for 1 <= V <= 2^20 classes, read in place
 * through the step table of runia_logit_stats: table [n_steps, 2] int64 on the device, {pointer to row 0, row stride in
 * elements} per step, n_steps steps of B rows of V logits (unit stride along V).  A plain [N, V] matrix is n_steps = 1, B = N.
 * Output row b * n_steps + t: size i32 [B * n_steps]; members i32 [B * n_steps, ceil(V / 32)] or NULL; covered u8 [B * n_steps]
 * or NULL (needs labels); u f32 [B * n_steps] or NULL.  labels: token ids, int32 or int64, the id of (b, t) at
 * labels[b * label_stride + t]; NULL: none.  B * n_steps <= 2^26.
 * The row is not ordered: for aps and raps the set is a prefix of the order, and the cut (a key value and how many of the
 * classes with that key are in, lower index first) is found by a radix descent over the 32-bit key of the logit, 11 / 11 / 10
 * bits, with per-bin counts and fixed-point masses (e * 2^40, 64-bit integer adds in LDS: exact in any order) - five reads of
 * the row by one workgroup, three for lac.  No workspace, nothing [N, V] written but the members.  The same bits from run to
 * run, wherever the row sits and however the steps are allocated; a 16-bit call gives the bits of the f32 call on the widened
 * values.  The scores differ from runia_conformal_sets' by f32 rounding (sums are formed in another order), so the two can
 * disagree on a class whose score lies within ~1e-6 of qhat. */
int runia_conformal_sets_wide(const void* table, int dtype, int64_t n_steps, int64_t B, int64_t V, const void* labels,
                              int labels_i64, int64_t label_stride, int has_ignore, int64_t ignore_index, const float* u,
                              int method, float beta, float lam, int k_reg, float qhat, int32_t* size, int32_t* members,
                              uint8_t* covered, runia_stream_t stream);

/* ---- Bootstrap replicates of the OoD metrics (bootstrap.hip; evaluation/bootstrap.py) ------------------------ *
 * Poisson bootstrap: in replicate b, row r of the score table (InD rows 0 .. n_ind - 1, OoD rows n_ind .. n - 1) is present
 * w(b, id(r)) times, id(r) = r or group_of_row[r] (cluster bootstrap; the caller keeps InD and OoD group ids apart):
 *   blk  = philox4x32_10(counter = (id, b >> 2, 0, 0x626f6f74), key = (seed.lo, seed.hi)),  word = component b & 3 of blk,
 *   w    = number of k in 0 .. 12 with T_k <= word,  T_k = floor(2^32 e^-1 sum_{j<=k} 1/j!)       (Poisson(1), at most 13)
 * - a pure function of (seed, b, id): methods scored on the same rows see the same resample, and replicates may be computed in
 * any chunking.
 * runia_boot_keys_f32/_f64: keys int64 [n_ind + n_ood], ascending signed order = descending order of the score as the metrics
 *   step sees it (sigmoid in the scores' dtype if any score lies outside [0, 1] or is NaN; f64 key; equal keys = a tie).
 *   any_outside: one device word, set to whether the sigmoid was applied.  n_ind, n_ood >= 1, n < 2^31.
 * runia_boot_metrics: sorted_keys [n] ascending with sorted_rows [n] int32 the row each key belongs to (a permutation of
 *   0 .. n - 1), group_of_row [n] int32 or NULL.  out f64 [n_boot, 3] = (AUROC, FPR@95, AUPR) of the replicates
 *   first_replicate .. first_replicate + n_boot - 1, one curve point per run of equal keys, TP / FP = cumulative InD / OoD
 *   weight, P / N their totals:
 *     AUROC  = sum_g (FP_g - FP_g-1)(TP_g + TP_g-1) / (2 P N), the sum in unsigned 64-bit integers;
 *     FPR@95 = FP_g / N at the first run with 20 TP_g >= 19 P (integers);
 *     AUPR   = sum_g ((TP_g - TP_g-1) / P)(prec_g + prec_g-1) / 2, prec = TP / (TP + FP), 1 where TP + FP = 0; f64, fixed order;
 *   P = 0 or N = 0: three NaN.  The same bits from call to call and for any split of a replicate range into calls.
 *   RUNIA_E_INVALID (before anything else is looked at) unless 1 <= n_ind < n < 2^31 and n_ind * (n - n_ind) < 2^55 (the bound of
 *   the integer sum: 13^2 * 2 * n_ind * n_ood < 2^64), n_boot >= 1, first_replicate >= 0, first_replicate + n_boot <= 2^31.
 *   workspace: runia_boot_workspace_bytes(n, n_boot) bytes, 8-byte aligned, uninitialised.
 * runia_boot_tile_rows: rows of a tile of the walk (test sizes are derived from it).
 * runia_boot_weight_of_word_host: the weight of one 32-bit random word (host; pins the threshold table).
 * runia_boot_weights_host: HOST pointers, no GPU touched: out u8 [n_boot, n], out[r * n + i] = w(first_replicate + r, ids[i]). */
int runia_boot_tile_rows(void);
int runia_boot_keys_f32(const float* ind_scores, int64_t n_ind, const float* ood_scores, int64_t n_ood, int64_t* keys,
                        unsigned* any_outside, runia_stream_t stream);
int runia_boot_keys_f64(const double* ind_scores, int64_t n_ind, const double* ood_scores, int64_t n_ood, int64_t* keys,
                        unsigned* any_outside, runia_stream_t stream);
size_t runia_boot_workspace_bytes(int64_t n, int64_t n_boot);
int runia_boot_metrics(const int64_t* sorted_keys, const int32_t* sorted_rows, int64_t n, int64_t n_ind,
                       const int32_t* group_of_row, uint64_t seed, int64_t first_replicate, int64_t n_boot, double* out,
                       void* workspace, size_t workspace_bytes, runia_stream_t stream);
int runia_boot_weight_of_word_host(uint32_t word);
int runia_boot_weights_host(uint64_t seed, int64_t first_replicate, int64_t n_boot, const int32_t* ids, int64_t n, uint8_t* out);

/* ---- Connected components and component-level overlap statistics (components.hip; evaluation/components.py) - *
 * runia_cc_label: labels int32 [N, H, W] of N binary images: 0 = background, 1 .. counts[n] in raster order of each
 *   component's first pixel (the per-image contract of scipy.ndimage.label), connectivity 4 or 8; counts int32 [N].  Nothing
 *   links across the left / right edge of a row or from one image to the next.  The images come from ONE of
 *     mask   uint8 [N, H, W] (non-zero = set), score == NULL, T == 1, N = G;   valid uint8 [N, H, W] or NULL;
 *     score  f32 [G, H, W] with thresholds f32 [T], mask == NULL: N = G * T and image n = t * G + g is score[g] > thresholds[t]
 *            (less != 0: <; a NaN score is never set), compared inside the tile kernel;   valid uint8 [G, H, W] or NULL.
 *   A pixel whose valid byte is 0 is background.  The same labels from call to call (canonical numbering; integer atomics only).
 *   Tiles of RUNIA_CC_TILE_H x RUNIA_CC_TILE_W pixels (runia_cc_tile_h / _w report what the library was built with).
 *   N * H * W < 2^31 (parents are int32), RUNIA_E_INVALID otherwise.  N == 0 or H * W == 0: 0, nothing launched.
 *   workspace: runia_cc_label_workspace_bytes(N, H, W) bytes, 16-byte aligned, uninitialised (RUNIA_E_WORKSPACE if short).
 *   Unlike the other entry points this one waits for the stream before it returns: every device loop carries a step cap
 *   derived from the image size, and a cap that was hit comes back as RUNIA_E_STEPCAP.
 * runia_cc_overlap: from gt_labels int32 [G, H, W] and pred_labels int32 [G * T, H, W] (image t * G + g) with the exclusive
 *   prefix sums of their counts, gt_offsets int32 [G] and pred_offsets [G * T] (component k of image g is row gt_offsets[g] + k - 1):
 *     stats != 0: ADDS to  gt_size [Kg] (NULL: skipped)  the pixels of every GT component (counted for t = 0 only),
 *                          gt_inter [T, Kg]              its pixels that are predicted under threshold t,
 *                          pred_size / pred_inter [Kp]   the pixels of every predicted component / those inside any GT component;
 *     n_keys (one uint64, ADDED to): the number of candidate pairs - pixels set in both whose left neighbour in the row holds
 *       another (k, k_hat) pair; keys != NULL: the candidates, int64 ((t * Kg + k) << 32 | k_hat) (rows as above), in arrival
 *       order, at most key_capacity of them (sort + unique gives the distinct pairs).
 *   Either label image may be NULL (sizes of the other one only; no keys).  Integer atomics: order-independent.
 *   G * T * H * W < 2^31, T * Kg < 2^31; RUNIA_E_INVALID otherwise.  No workspace.
 * runia_cc_relabel: labels[n, p] = map[offsets[n] + labels[n, p] - 1] where labels[n, p] > 0, in place. */
#ifndef RUNIA_CC_TILE_H
#define RUNIA_CC_TILE_H 32
#endif
#ifndef RUNIA_CC_TILE_W
#define RUNIA_CC_TILE_W 32
#endif
int runia_cc_tile_h(void);
int runia_cc_tile_w(void);
size_t runia_cc_label_workspace_bytes(int64_t N, int64_t H, int64_t W);
int runia_cc_label(const uint8_t* mask, const float* score, const float* thresholds, int64_t T, int less, const uint8_t* valid,
                   int64_t G, int64_t H, int64_t W, int connectivity, int32_t* labels, int32_t* counts, void* workspace,
                   size_t workspace_bytes, runia_stream_t stream);
int runia_cc_overlap(const int32_t* gt_labels, const int32_t* gt_offsets, const int32_t* pred_labels, const int32_t* pred_offsets,
                     int64_t G, int64_t T, int64_t H, int64_t W, int64_t Kg, int32_t* gt_size, int32_t* gt_inter,
                     int32_t* pred_size, int32_t* pred_inter, int64_t* keys, int64_t key_capacity, uint64_t* n_keys, int stats,
                     runia_stream_t stream);
int runia_cc_relabel(int32_t* labels, const int32_t* offsets, const int32_t* map, int64_t N, int64_t H, int64_t W,
                     runia_stream_t stream);

/* ---- Selective prediction: risk-coverage curve, AURC, AUGRC, equal-mass bins (selective.hip; evaluation/selective.py) *
 * A table of n rows, each with a confidence kappa (higher = kept first) and a finite loss l.  Rows are ordered by descending
 * confidence; -0.0 == +0.0, +-inf are ordinary values, NaN is an error.  A run is a maximal set of equal confidences at the
 * sorted positions s + 1 .. e (1-based); L_k / S_k: cumulative loss / confidence of the first k sorted rows.  For s < k <= e
 *     Lbar_k = L_s + (k - s)(L_e - L_s) / (e - s)      (the mean of L_k over the orders of the rows inside the tie; Sbar_k likewise)
 *     aurc   = (1 / n)   sum_k Lbar_k / k              (without ties: mean(cumsum(l_sorted) / arange(1, n + 1)))
 *     augrc  = (1 / n^2) sum_k Lbar_k
 * - nothing depends on the order in which tied rows arrive.
 * runia_sel_keys_f32/_f64: keys int64 [n], ascending signed order = descending confidence; f32 is widened to f64 exactly (one key
 *   space), the two zeros share a key.  bad: one device word, set to whether any confidence is NaN.  1 <= n < 2^31.
 * runia_sel_key_of_f64_host: the same key of one value (host; pins the order).
 * runia_sel_curve: sorted_keys [n] ascending with sorted_rows [n] int32 the row each key belongs to (a permutation of 0 .. n - 1;
 *   the pair has the shape of the bootstrap's ordered table), loss [n] f32 (loss_f64 == 0) or f64, read through the rows.  The
 *   confidences are not an argument: a key is the f64 confidence, one to one (but for the sign of zero), and is turned back
 *   into it, so the order and the confidence sums cannot disagree and nothing but the loss is gathered.
 *   record f64 [5] = (n_points, L_n, S_n, aurc, augrc).  run_end / cum_loss / cum_conf: all three NULL, or
 *   room for n entries each - the compacted curve, one point per run: run_end int32 ascending (= e), cum_loss = L_e and
 *   cum_conf = S_e f64; n_points: one device int64 (needed with the curve, otherwise optional).
 *   Every sum is f64 in an order fixed by n alone; no floating-point atomics; the same inputs give the same bits.  Cumulative sums
 *   of integer-valued losses (the 0/1 error) are exact: every output is then bit-identical under ANY permutation of the input
 *   rows.  The cost does not depend on the lengths of the runs.
 *   RUNIA_E_INVALID (before anything else is looked at) unless 1 <= n < 2^31.
 *   workspace: runia_sel_workspace_bytes(n) bytes, 8-byte aligned, uninitialised (RUNIA_E_WORKSPACE if short).
 * runia_sel_query: from the compacted curve (device pointers; n_points is read on the device, clamped to n).
 *   targets int64 [n_targets]: k_c = ceil(c n) of the coverage targets, formed exactly by the caller, 1 <= k_c <= n (clamped);
 *     risk_at / coverage_at f64 [n_targets] = L_e / e and e / n at the first run end e >= k_c (a cut falls between distinct
 *     confidences only).
 *   risks f64 [n_risks]: coverage_at_risk f64 [n_risks] = the largest e / n over ALL run ends with L_e <= r * e (f64, as
 *     written), 0 if none: a reduction by integer atomicMax, not a search - the curve is not monotone.
 *   n_bins = B >= 1: bins f64 [B, 3] = (count, loss sum, confidence sum) of the equal-mass bins counted from the LEAST confident
 *     row: bin b holds the ascending positions [floor(b n / B), floor((b + 1) n / B)), its sums are differences of Lbar and Sbar
 *     at the two boundaries (a tie that straddles a boundary is shared in proportion); an empty bin holds three zeros.
 *     B == 0: no table.
 *   RUNIA_E_INVALID (before anything else is looked at) unless 1 <= n < 2^31, n_targets and n_risks in 0 .. 64, n_bins in 0 .. 512.
 *   workspace: 256 bytes or more, 8-byte aligned, uninitialised (runia_sel_workspace_bytes(n) covers it).
 * runia_sel_tile_rows: rows of a tile of the scan (test sizes are derived from it). */
int runia_sel_tile_rows(void);
int runia_sel_keys_f32(const float* conf, int64_t n, int64_t* keys, unsigned* bad, runia_stream_t stream);
int runia_sel_keys_f64(const double* conf, int64_t n, int64_t* keys, unsigned* bad, runia_stream_t stream);
int64_t runia_sel_key_of_f64_host(double conf);
size_t runia_sel_workspace_bytes(int64_t n);
int runia_sel_curve(const int64_t* sorted_keys, const int32_t* sorted_rows, const void* loss, int loss_f64, int64_t n,
                    double* record, int32_t* run_end, double* cum_loss, double* cum_conf, int64_t* n_points, void* workspace,
                    size_t workspace_bytes, runia_stream_t stream);
int runia_sel_query(const int32_t* run_end, const double* cum_loss, const double* cum_conf, const int64_t* n_points, int64_t n,
                    const int64_t* targets, int n_targets, const double* risks, int n_risks, int n_bins, double* risk_at,
                    double* coverage_at, double* coverage_at_risk, double* bins, void* workspace, size_t workspace_bytes,
                    runia_stream_t stream);

/* ---- bootstrap replicates of the selective-prediction summaries (csrc/boot_selective.hip) ------------------------------------
 * Replicate b gives row r the Poisson(1) weight w(seed, b, id(r)) of the bootstrap section above, unchanged - id(r) = r, or
 * group_of_row[r] - so two methods scored on the same rows, and runia_boot_metrics on the same ids, see the same resample.  A
 * replicate is the tie-aware definition of the selective section on the table with every row physically repeated w times.
 * For a run of equal keys write s, e for the cumulative weight before the run and at its end, L_s, L_e for the cumulative
 * weighted loss sum w l there, m = e - s, d = L_e - L_s, n' for the total weight.  A run with m == 0 is no curve point; else
 *     sum_{k = s+1 .. e} Lbar_k     = m L_s + d (m + 1) / 2
 *     sum_{k = s+1 .. e} Lbar_k / k = L_s dH + (d / m)(m - s dH),    dH = sum_{k = s+1 .. e} 1 / k
 *     aurc = (1 / n') sum_runs sum Lbar_k / k,    augrc = (1 / n'^2) sum_runs sum Lbar_k,    risk = L_n' / n'.
 * dH: the per-copy terms themselves for m <= 32; beyond, the first terms up to s0 = max(s, 32) directly and
 *     log1p((e - s0) / s0) + t(e) - t(s0), t(x) = 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6): no loop over the copies of a run.
 * runia_boot_sel_metrics: sorted_keys [n] ascending with sorted_rows [n] int32 (the ordered table of runia_sel_keys_* and
 *   runia_sel_curve), loss [n] f32 (loss_f64 == 0) or f64, finite, read through the rows; group_of_row int32 [n] or NULL.
 *   out f64 [n_boot, 4] = (aurc, augrc, risk, n') of the replicates first_replicate .. first_replicate + n_boot - 1; a
 *   replicate with n' == 0 holds three NaN and 0.
 *   One workgroup per Philox block of four replicates walks the table once, tile by tile; the weight counts are integers, the
 *   weighted loss sums f64 in an order fixed by n alone; no atomics, no workspace: the same bits from call to call and for
 *   any split of the replicates into calls.  Integer-valued losses (the 0/1 error) give exact cumulative sums.
 *   RUNIA_E_INVALID (before any pointer is looked at) unless 1 <= n < 2^31, n_boot >= 1, first_replicate >= 0 and
 *   first_replicate + n_boot <= 2^31.
 * runia_boot_sel_tile_rows: rows of a tile of the walk (test sizes are derived from it). */
int runia_boot_sel_tile_rows(void);
int runia_boot_sel_metrics(const int64_t* sorted_keys, const int32_t* sorted_rows, const void* loss, int loss_f64, int64_t n,
                           const int32_t* group_of_row, uint64_t seed, int64_t first_replicate, int64_t n_boot, double* out,
                           runia_stream_t stream);

/* ---- per-pixel Mahalanobis maps from segmentation features (csrc/pixel_features.hip) ------------------------------------------
 * runia_pixfeat_score: the distance of every pixel of G feature maps to the nearest of K class Gaussians with one shared
 * covariance, ONE launch, the maps read where the model left them.
 *   features   base of a (G, C, H, W) map, dtype 0 f32, 1 f16, 2 bf16 (the codes of runia_pixel_uncertainty_maps), widened
 *              exactly; all arithmetic in f32.
 *   sn sc sh sw element strides (>= 0) of the image, channel, h and w dimensions: NCHW, channels_last (sc == 1) and sliced
 *              views are read in place.
 *   m0         f32 [C]: the centre that is subtracted first.
 *   W          f32 [C, C] row-major, LOWER TRIANGULAR (= L^-1 of the pooled covariance): what lies above the diagonal is
 *              never read past the 128-column block of its row, and must be zero.
 *   mz         f32 [K, C]: mz_c = W (mu_c - m0).  A row whose first entry is +inf marks an excluded (empty) class.
 *   outputs    contiguous, each may be NULL, at least one set:
 *                distance        f32 (G, H, W)    min_c |W (x - m0) - mz_c|^2
 *                nearest         int32 (G, H, W)  its argmin, lowest index on ties
 *                class_distances f32 (G, K, H, W)
 *              The sum over the channels is the difference form sum_j (z_j - mz_cj)^2 (the expanded form cancels in f32 when
 *              the features sit away from zero).  An excluded class scores +inf and is never `nearest` unless all are
 *              excluded (then 0).  A distance that is not finite - NaN or inf among the pixel's features - is written as NaN
 *              in every output of THAT pixel (nearest 0); no other pixel is touched by it.
 *   A 256-thread workgroup owns 128 consecutive pixels of the flattened G * H * W axis; 32 channels at a time are staged into
 *   LDS (16- / 8-byte loads of four pixels when w has unit stride and the other strides, H * W resp. W and the base are
 *   multiples of four elements; 16-byte loads of neighbouring channels when sc == 1, C >= 16 and the other strides and the
 *   base are multiples of 16 bytes - channels_last; element loads through the strides otherwise: the same bits on every
 *   path) and multiplied on the f32 matrix cores; the zero blocks of W are skipped.  Fixed summation order, no atomics: run-to-run bit identical, and a pixel's result does not
 *   depend on its position in the batch.  The running sums of 32 classes live in registers: K > 32 repeats the product per
 *   group of 32 classes.
 *   1 <= C <= 1024, 1 <= K <= 256, G, H, W < 2^31, G * H * W <= 2^37; RUNIA_E_INVALID otherwise (checked on the host before
 *   anything else).  G == 0 or H * W == 0: 0, nothing launched.  workspace: runia_pixfeat_workspace_bytes(C, K) bytes - a
 *   function of C and K alone, never of the pixels (0 today: the arguments are kept for the ABI).
 * runia_pixfeat_label_hist: labels [N] int64 (label_dtype 0), int32 (1) or uint8 (2) -> counts int64 [K] of the labels in
 *   [0, K) other than ignore_index, dropped int64 [1] of all the others.  Integer counts: deterministic.  1 <= K <= 256,
 *   0 <= N <= 2^37.
 * runia_pixfeat_gather_rows: a deterministic subsample of the labelled pixels as rows.  Pixel p (row-major over H * W) of
 *   image g is kept iff its label l is in [0, K), is not ignore_index, and the Philox4x32-10 draw with counter
 *   ((image_offset + g) * H * W + p, 0) and key `seed` (first word, 24 bits) is below keep_prob[l] (f32 [K] on the device:
 *   1 keeps all, 0 none).  The subset depends on (seed, image_offset + g, p) alone, not on the batching.
 *   labels (G, H, W) contiguous; features as for runia_pixfeat_score.  n_out: one device int64, the number of kept pixels
 *   (always written).  rows f32 (n, C) = the widened features, row_labels int32 (n): both NULL (count only) or both given
 *   with room for max_rows rows; rows beyond max_rows are not written.  Rows come in pixel order: a count per 1024-pixel
 *   chunk, a scan, then the write - no atomic decides a position.
 *   workspace: runia_pixfeat_gather_workspace_bytes(G * H * W) bytes, 8-byte aligned (RUNIA_E_WORKSPACE if short).
 *   Limits as for runia_pixfeat_score; 0 <= image_offset < 2^31. */
size_t runia_pixfeat_workspace_bytes(int64_t C, int64_t K);
int runia_pixfeat_score(const void* features, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                        int64_t sh, int64_t sw, const float* m0, const float* Wmat, const float* mz, int64_t K, float* distance,
                        int32_t* nearest, float* class_distances, void* workspace, size_t workspace_bytes,
                        runia_stream_t stream);
int runia_pixfeat_label_hist(const void* labels, int label_dtype, int64_t N, int64_t K, int64_t ignore_index, int64_t* counts,
                             int64_t* dropped, runia_stream_t stream);
size_t runia_pixfeat_gather_workspace_bytes(int64_t pixels);
int runia_pixfeat_gather_rows(const void* features, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn,
                              int64_t sc, int64_t sh, int64_t sw, const void* labels, int label_dtype, int64_t K,
                              int64_t ignore_index, const float* keep_prob, uint64_t seed, int64_t image_offset, float* rows,
                              int32_t* row_labels, int64_t max_rows, int64_t* n_out, void* workspace, size_t workspace_bytes,
                              runia_stream_t stream);

/* ---- kernel two-sample tests: MMD and energy distance with a permutation null (csrc/shift.hip) -------------------------------
 * Two row tables X [n, D], Y [m, D] of one dtype (0 f32, 1 f16, 2 bf16), read where they lie through their row strides (in
 * elements, >= D); pooled Z = [X; Y], N = n + m <= 2^18.  Rows are centred by the pooled column mean (f64 column sums in a fixed
 * order, rounded to f32) unless kind is linear.
 *   kind       0 rbf: k = sum_b exp(-d^2 / (2 sigma_b^2)) over 1 .. 8 bandwidths;  1 energy: k = -d;  2 linear: k = z_i . z_j.
 *              d^2 = max(0, |z_i|^2 + |z_j|^2 - 2 z_i . z_j) in f32, and 0 exactly where i == j.
 *   memberships  permutation p (p = 0: the identity, the first n rows) puts row i in the first set iff the pair (word, i), word =
 *              component p & 3 of philox4x32_10(counter = (i, p >> 2, 0, 0x73686674), key = (seed.lo, seed.hi)), is among the n
 *              smallest pairs in lexicographic order: exactly n members, a pure function of (seed, p, i, n, N).
 *   sums       with K = k(Z, Z):  t_p = a_p^T K a_p,  u_p = a_p^T K 1,  S = 1^T K 1;  AA = t, AB = u - t, BB = S - 2 u + t.
 *   estimator  0 biased: AA / n^2 + BB / m^2 - 2 AB / (n m);  1 unbiased (n, m >= 2): (AA - dA) / (n (n - 1)) + (BB - dB) / (m (m - 1))
 *              - 2 AB / (n m), dA / dB the sums of k_ii over either side (rbf: n / m times n_bandwidths, energy: 0, linear: the
 *              squared norms).
 * runia_shift_perm_bits: rows first_perm .. first_perm + n_rows - 1 of the membership table as packed bits, bits[r * row_words +
 *   (i >> 5)] bit i & 31, row_words >= ceil(N / 32); every word of a row is written, bits past N are 0.  1 <= n < N.
 * runia_shift_perm_bits_host: the same on HOST memory through the same header code (csrc/shift_perm.hpp), no GPU touched.
 * runia_shift_sample_rows: M = min(N, 2048), the rows of the bandwidth sample.
 * runia_shift_pairwise_sample: out f32 [M (M - 1) / 2], the distances |z_a - z_b| (direct differences, which centring would not
 *   change) of the sample rows floor(k N / M), k = 0 .. M - 1, upper triangle row by row.
 * runia_shift_mmd: bandwidths is a HOST array of n_bandwidths sigmas (> 0; read for kind 0 only).  Outputs on the device: t, u,
 *   stats f64 [1 + n_perm] (entry 0: the observed split), S f64 [1], count int64 [1] = #{p >= 1: stats[p] >= stats[0]}, p_value f64
 *   [1] = (1 + count) / (1 + n_perm), NaN when stats[0] is NaN (any non-finite input).  The N x N kernel matrix is never
 *   formed: Gram tiles on the f32 matrix cores are turned into kernel values in registers, split into three exact bf16 pieces and
 *   multiplied with the 0/1 memberships on the bf16 matrix cores, at most 1024 columns (identity and ones columns included) per
 *   launch, f32 chains of at most 2048 terms, then f64 sums in an order fixed by the shape.  No float atomics: the same bits
 *   from call to call.
 *   RUNIA_E_INVALID (before anything else is looked at) unless n, m >= 1, N <= 2^18, 1 <= D < 2^31, 1 <= n_perm < 2^31.
 *   workspace: runia_shift_workspace_bytes(n, m, D, n_perm) bytes, 16-byte aligned, uninitialised (RUNIA_E_WORKSPACE if short). */
size_t runia_shift_workspace_bytes(int64_t n, int64_t m, int64_t d, int64_t n_perm);
int runia_shift_perm_bits(uint64_t seed, int64_t n, int64_t N, int64_t first_perm, int64_t n_rows, uint32_t* bits,
                          int64_t row_words, runia_stream_t stream);
int runia_shift_perm_bits_host(uint64_t seed, int64_t n, int64_t N, int64_t first_perm, int64_t n_rows, uint32_t* bits,
                               int64_t row_words);
int64_t runia_shift_sample_rows(int64_t N);
int runia_shift_pairwise_sample(const void* x, int64_t n, int64_t x_stride, const void* y, int64_t m, int64_t y_stride,
                                int64_t d, int dtype, float* out, runia_stream_t stream);
int runia_shift_mmd(const void* x, int64_t n, int64_t x_stride, const void* y, int64_t m, int64_t y_stride, int64_t d,
                    int dtype, int kind, const double* bandwidths, int n_bandwidths, int estimator, uint64_t seed,
                    int64_t n_perm, double* t, double* u, double* S, double* stats, int64_t* count, double* p_value,
                    void* workspace, size_t workspace_bytes, runia_stream_t stream);

/* ---- per-feature Kolmogorov-Smirnov statistics with a permutation null (csrc/ks_perm.hip) -----------------------------------
 * Two row tables X [n, D], Y [m, D] of one dtype (0 f32, 1 f16, 2 bf16), read where they lie through their row strides (in
 * elements, >= D); pooled Z = [X; Y], N = n + m <= runia_ks_max_rows().
 *   statistic  for column d and permutation p: walk the pooled values of the column in ascending order, v = 0, v += m for a member
 *              of the first set of p and v -= n otherwise; T[p, d] = max |v| over the LAST positions of the runs of equal values.
 *              An exact integer <= n m; the two-sample KS statistic is T / (n m).
 *   order      values compare as numbers: f16 / bf16 widened exactly, -0 == +0, +-inf ordinary extreme values.  A column that holds
 *              a NaN is invalid: valid[d] = 0 and T[:, d] = -1; otherwise valid[d] = 1.
 *   memberships  those of runia_shift_perm_bits with the same (seed, n, N): p = 0 the identity (rows i < n), exactly n members.
 * runia_ks_max_rows: the largest pooled N of one call (16384: one column's (key, row) pairs are sorted in 128 KiB of LDS; n m <=
 *   2^26, so the walk's counters are 32-bit).
 * runia_ks_columns_per_pass: the columns ordered and walked per pass, min(4096, 64 MiB / (4 ceil(N / 64) 64)) >= 1024: the row
 *   orders of a pass take at most 64 MiB of the workspace whatever D is.  0 for an invalid shape.
 * runia_ks_workspace_bytes: the orders of one pass (bounded, above) plus the membership bits twice (as rows of permutations and
 *   as rows of pooled rows), which are NOT bounded: about N / 4 bytes per permutation, so the workspace grows linearly in n_perm -
 *   4 MB at N = 16384, n_perm = 999, 4 GiB at N = 16384, n_perm = 2^20 - 1.  0 for invalid shapes.
 * runia_ks_perm_table: table int64 [1 + n_perm, D] and valid int32 [D] on the device.  Integer work only: the same bits from call
 *   to call.  RUNIA_E_INVALID (before anything is dereferenced or launched) unless n, m >= 1, N <= runia_ks_max_rows(),
 *   1 <= D < 2^31, 0 <= n_perm < 2^20, dtype in 0 .. 2, strides >= D and no NULL pointer.
 *   workspace: runia_ks_workspace_bytes(n, m, D, n_perm) bytes, 16-byte aligned, uninitialised (RUNIA_E_WORKSPACE if short). */
int64_t runia_ks_max_rows(void);
int64_t runia_ks_columns_per_pass(int64_t n, int64_t m, int64_t n_perm);
size_t runia_ks_workspace_bytes(int64_t n, int64_t m, int64_t d, int64_t n_perm);
int runia_ks_perm_table(const void* x, int64_t n, int64_t x_stride, const void* y, int64_t m, int64_t y_stride, int64_t d,
                        int dtype, uint64_t seed, int64_t n_perm, int64_t* table, int32_t* valid, void* workspace,
                        size_t workspace_bytes, runia_stream_t stream);

/* ---- per-pixel kNN maps from segmentation features and the k-center coreset (csrc/pixel_knn.hip) ----------------------------
 * runia_pixknn_score: the k smallest SQUARED Euclidean distances of every pixel of G feature maps to the M rows of a bank, and
 * the indices of those rows, ONE launch, the maps read where the model left them.
 *   features, dtype, G, C, H, W, sn sc sh sw   as for runia_pixfeat_score (NCHW, channels_last and sliced views in place).
 *   center     f32 [C]: subtracted from every pixel first (x~ = x - center).
 *   bank       f32 [M, C] row-major, ALREADY centred (b~ = b - center);  bank_sq f32 [M] = |b~|^2.
 *   outputs    contiguous, each may be NULL, at least one set:
 *                distances     f32 (G, k, H, W)   ascending along k
 *                indices       int32 (G, k, H, W) on equal distances the lower bank index first
 *                kth_distance  f32 (G, H, W)      the bits of distances[:, k - 1]
 *                mean_distance f32 (G, H, W)      (d_0 + ... + d_{k-1}) / k, summed in that order in f32
 *              d = max(0, |x~|^2 + (|b~|^2 - 2 x~ . b~)) in f32; the products run on v_mfma_f32_32x32x2_f32 (exact f32 chains in
 *              channel order), |x~|^2 is one fmaf chain per lane half in channel order.  A pixel whose |x~|^2 is not finite -
 *              NaN or inf among its features - has NaN distances and index -1 in every output; no other pixel is touched by it.
 *   A 256-thread workgroup owns 128 consecutive pixels of the flattened G * H * W axis and walks the bank in blocks of 128 rows,
 *   32 channels at a time through LDS (the load forms of runia_pixfeat_score: the same bits on every path); the k best of a
 *   pixel are a sorted list in registers.  No (pixels, C) table, no f32 copy of the map, no pixels x M matrix.  Fixed
 *   summation order, no atomics: run-to-run bit identical, and a pixel's result does not depend on its position in the batch.
 *   1 <= C <= 1024, 1 <= k <= 16, k <= M <= 2^22, G, H, W < 2^31, G * H * W < 2^31; RUNIA_E_INVALID otherwise (checked on the
 *   host before anything else).  G == 0 or H * W == 0: 0, nothing launched.  workspace: runia_pixknn_workspace_bytes(C, M, k)
 *   bytes - never a function of the pixels (0 today: the arguments are kept for the ABI).
 * runia_kcenter_greedy_f32: greedy k-center (farthest-point) selection of n_pick rows of rows f32 [N, D] row-major.  Pick 0 is
 *   row `first`; pick t + 1 is the row with the largest squared distance to its nearest picked row, the lowest index on ties.
 *   Distances in difference form, sum_c (x_c - centre_c)^2 in f32 in a fixed order.  One launch per pick, queued back to back.
 *   picked int32 [n_pick], radius f32 [n_pick] (the largest min-distance at the moment of each pick: radius[0] = +inf, then
 *   non-increasing), n_picked one device int64.  Selection stops when the largest remaining distance is not positive (every
 *   remaining row duplicates a picked one; n_pick >= N runs out the same way): the rest of picked is -1, of radius 0.
 *   1 <= D <= 1024, 1 <= N < 2^31, 0 <= first < N, 1 <= n_pick < 2^31; RUNIA_E_INVALID otherwise or on a NULL pointer.
 *   workspace: runia_kcenter_workspace_bytes(N, D) bytes, 16-byte aligned, uninitialised (RUNIA_E_WORKSPACE if missing or short). */
size_t runia_pixknn_workspace_bytes(int64_t C, int64_t M, int64_t k);
int runia_pixknn_score(const void* features, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                       int64_t sh, int64_t sw, const float* center, const float* bank, const float* bank_sq, int64_t M,
                       int64_t k, float* distances, int32_t* indices, float* kth_distance, float* mean_distance,
                       void* workspace, size_t workspace_bytes, runia_stream_t stream);
size_t runia_kcenter_workspace_bytes(int64_t N, int64_t D);
int runia_kcenter_greedy_f32(const float* rows, int64_t N, int64_t D, int64_t first, int64_t n_pick, int32_t* picked,
                             float* radius, int64_t* n_picked, void* workspace, size_t workspace_bytes, runia_stream_t stream);

/* ---- Calibration of a segmentation head (pixel_calibration.hip; evaluation/pixel_calibration.py) --------------- *
 * runia_pixel_calib_accumulate: ONE pass over logits (G, C, H, W), read in place through the element strides sn, sc, sh, sw
 *   (`dtype` 0 f32, 1 f16, 2 bf16, widened exactly, f32 arithmetic) at the temperature 1 / beta (0 < beta < inf), against
 *   labels (G, H, W) contiguous (`label_dtype` 0 int64, 1 int32, 2 uint8).  The row of a pixel is x = logits[g, :, i, j]; its
 *   pred, conf, nll, brier, g and h are those of runia_calib_rows (the same arithmetic, csrc/calib_core.hpp).  A pixel is
 *   USED when 0 <= y < C and not (has_ignore and y == ignore_index); a pixel whose label is outside [0, C) and is not the
 *   ignore value is BAD: counted, not scored.  The call ADDS into `record` (the caller zeroes it once; int64 / f64 slots of 8
 *   bytes, 8-byte aligned), whose layout depends on C and n_bins alone:
 *     [0] n_used  [1] n_correct  [2] n_bad (int64)   [3] sum nll  [4] sum brier  [5] sum g  [6] sum h (f64)   [7] reserved
 *     RUNIA_PIXCAL_HEAD_SLOTS = 8 ..      count[n_bins]  correct[n_bins] (int64)  conf_sum[n_bins] (f64)      top-label table
 *     8 + 3 n_bins ..                     support[C]  predicted[C]  hit[C] (int64)                            per-class counters
 *     8 + 3 n_bins + 3 C ..               cw_count[C][n_bins]  cw_pos[C][n_bins] (int64)  cw_conf_sum[C][n_bins] (f64)
 *   over the used pixels: bin b = clamp((int)ceilf(conf * (float)n_bins) - 1, 0, n_bins - 1) of the top-label table (f32
 *   arithmetic); support[k] pixels labelled k, predicted[k] pixels with pred == k, hit[k] both; for every class k the
 *   probability p_k = e_k / S0 enters bin b(p_k) of row k of the class-wise table, cw_pos counting the entries with y == k.
 *   A used pixel with a NaN logit (or without a finite one) counts in n_used, with pred the first maximum among its non-NaN
 *   logits (0 without one) - so in n_correct, support, predicted and hit like any other - and in bin 0 of every table row it
 *   enters, whose conf_sum it makes NaN, as it makes the four float sums (the rule of runia_calib_reduce_f32 for a NaN row).
 *   mode: RUNIA_PIXCAL_MODE_HEAD      the head only (n_bins must be 0): what a Newton iteration of the temperature fit reads
 *         RUNIA_PIXCAL_MODE_TOP       the head, the top-label table and the per-class counters (1 <= n_bins <= 512)
 *         RUNIA_PIXCAL_MODE_CLASSWISE all of it; C * n_bins <= RUNIA_PIXCAL_MAX_CLASSWISE (4096)
 *   conf_map f32 / pred_map int32 (G, H, W) contiguous, either may be NULL: conf and pred of EVERY pixel, whatever its label.
 *   record may be NULL when a map is asked for (labels are then not read).
 *   Load forms, picked from the strides: four neighbouring pixels of a class plane per lane and load when w has unit stride,
 *   every other stride and the base are multiples of four elements and the row (rows that follow one another, sh == W * sw,
 *   count as one) is a multiple of four pixels; a pixel per lane over its contiguous classes when sc == 1 (channels_last); a
 *   pixel per lane through the strides otherwise.  C <= 24 keeps a pixel's logits in registers (one read); wider heads walk
 *   the class planes twice, three times with the class-wise table.
 *   Counts by integer atomics; the conf sums as integer multiples of 2^-30 (each confidence rounded to the nearest one); the
 *   four float sums in f64 in a fixed order (per-workgroup partials, one ordered pass): the same calls give the same bits.
 *   1 <= C <= RUNIA_PIXCAL_MAX_CLASSES (1024), G, H, W < 2^31, G * H * W <= 2^34, strides >= 0; RUNIA_E_INVALID otherwise,
 *   before anything is launched.  G == 0 or H * W == 0: 0, nothing launched, the record untouched.
 *   workspace: runia_pixel_calib_workspace_bytes(G, C, H, W, n_bins, mode) bytes (0 for sizes the call refuses or has nothing
 *   to do for), 8-byte aligned, uninitialised (RUNIA_E_WORKSPACE if missing or short).  (The query returns int64_t: its values
 *   are pinned on a grid of their own in tests/test_pixel_calibration_host.py.) */
#define RUNIA_PIXCAL_HEAD_SLOTS 8
#define RUNIA_PIXCAL_MAX_BINS 512
#define RUNIA_PIXCAL_MAX_CLASSES 1024
#define RUNIA_PIXCAL_MAX_CLASSWISE 4096
#define RUNIA_PIXCAL_MODE_HEAD 0
#define RUNIA_PIXCAL_MODE_TOP 1
#define RUNIA_PIXCAL_MODE_CLASSWISE 2
int64_t runia_pixel_calib_workspace_bytes(int64_t G, int64_t C, int64_t H, int64_t W, int n_bins, int mode);
int runia_pixel_calib_accumulate(const void* logits, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn,
                                 int64_t sc, int64_t sh, int64_t sw, const void* labels, int label_dtype, int has_ignore,
                                 int64_t ignore_index, float beta, int n_bins, int mode, void* record, float* conf_map,
                                 int32_t* pred_map, void* workspace, size_t workspace_bytes, runia_stream_t stream);

/* ---- Standardized Max Logits maps with boundary smoothing (pixel_sml.hip; inference/pixel_sml.py) --------------- *
 * The three entry points read logits (G, C, H, W) in place through the element strides sn, sc, sh, sw (`dtype` 0 f32, 1 f16,
 * 2 bf16, widened exactly) in the load forms of runia_pixel_calib_accumulate (four pixels of a class plane per lane; a pixel per
 * lane over its contiguous classes when sc == 1; a pixel per lane through the strides) and its two kernels (C <= 24: every load
 * of a pixel is issued before the first compare; any C <= 1024: one walk).  Per pixel m = max_c x_c and label = argmax_c x_c as
 * torch.max(dim=1) on the CPU gives them: a NaN logit gives m = NaN and the index of the first NaN, ties give the lowest index.
 * runia_pixel_sml_accumulate: ONE pass that ADDS into `record` (the caller zeroes it once; int64 slots, 8-byte aligned):
 *     [0] n_used  [1] n_masked  [2] n_bad  [3 .. 7] reserved                         RUNIA_PIXSML_HEAD_SLOTS = 8
 *     8 ..        count[C]  sum_q[C] (int64)  sq_hi[C]  sq_lo[C] (uint64)
 *   valid: uint8 / bool (G, H, W) contiguous, or NULL (every pixel).  A pixel whose valid entry is 0 counts in n_masked.  A valid
 *   pixel is USED when m is finite and |m| < 2^14, and counts in n_bad otherwise.  A used pixel adds q = rint(m * 2^16) (an
 *   integer, |q| < 2^30; m * 2^16 is exact in f32): count[label] += 1, sum_q[label] += q, and q * q = hi * 2^30 + lo (0 <= lo <
 *   2^30) as sq_hi[label] += hi, sq_lo[label] += lo.  hi, lo < 2^30, so neither sum overflows a uint64 within the 2^34 pixels
 *   that ONE RECORD admits over all its calls (the caller keeps the total; a call admits G * H * W <= 2^34 as well).
 *   Integer adds only (LDS tables per workgroup, 28 bytes a class; 64-bit global integer atomics into the record): the record is
 *   bit-identical from run to run, under any split of the data into calls, any order of the calls, and adds across GPUs.
 *   The 2^-16 grid holds every bf16 logit with |x| >= 2^-9 and every f16 logit with |x| >= 2^-6 exactly; an f32 logit is at most
 *   2^-17 off.  mean_c = sum_q / (count 2^16), var_c = (sumsq - sum_q^2 / count) / (count - 1) / 2^32 with sumsq = sq_hi 2^30 +
 *   sq_lo: exact in integers / rationals on the host.
 * runia_pixel_sml_maps: ONE launch.  mean, inv_std f32 [C] on the device.  Outputs (G, H, W) contiguous, each may be NULL, at
 *   least one set: sml f32 = (m - mean[label]) * inv_std[label] (two f32 operations in this order, no contraction), label int32,
 *   max_logit f32 = m.  IEEE: a NaN pixel gives sml NaN, a row of -inf gives -inf (inv_std > 0).  Higher = more in-distribution.
 * Both: 1 <= C <= RUNIA_PIXSML_MAX_CLASSES, G, H, W < 2^31, G * H * W <= 2^34, strides >= 0, no NULL where a pointer is needed;
 *   RUNIA_E_INVALID otherwise, before anything is launched.  G == 0 or H * W == 0: 0, nothing launched.  No workspace.
 * runia_pixel_boundary_smooth_f32: score f32 and label int32 (G, H, W) contiguous -> out f32 (G, H, W) contiguous (out must not
 *   overlap score).  Per image; out-of-image neighbours are taken by clamping coordinates (replicate padding).
 *   boundary   B[p] = 1 iff the label of p differs from that of one of its in-image 4-neighbours.  dist[p]: the Chebyshev distance
 *              to the nearest boundary pixel of the image; E_r = {p : dist[p] <= r}.
 *   suppression  boundary_width Wb in 0 .. 8, boundary_iterations I in 0 .. 8; Wb == 0 or I == 0: skipped; otherwise Wb % I == 0.
 *              For t = 0 .. I - 1: r_t = Wb - (Wb / I) t - 1, and r_{I-1} = 0.  Every p in E_{r_t} takes the mean of the entries
 *              of its clamped 3 x 3 window of the PREVIOUS iterate that are not in E_{r_t} (a clamped duplicate counts each time
 *              it appears; summed row by row in f32, divided by their number n); n == 0 or p outside E_{r_t}: the value stays.
 *              Entries in E_{r_t} are selected out, not multiplied by 0: a NaN there does not spread.
 *   smoothing  kernel_size K in {3, 5, 7} (0: skipped), dilation d in 1 .. 8, taps: K f32 values ON THE HOST (copied into the
 *              launch).  out[i, j] = sum_a g[a] (sum_b g[b] x[clamp(i + (a - (K-1)/2) d), clamp(j + (b - (K-1)/2) d)]), both
 *              sums in ascending tap order in f32.  Both steps skipped: out = score.
 *   A workgroup owns a RUNIA_PIXSML_TILE_H x RUNIA_PIXSML_TILE_W tile of one image; suppression and smoothing are one launch
 *   each, the suppressed map between them in the workspace.  One thread per output pixel, fixed order: run-to-run bit identical.
 *   G, H, W < 2^31, G * H * W <= 2^34, fewer than 2^31 tiles; RUNIA_E_INVALID otherwise or for a parameter out of range, before
 *   anything is launched.  workspace: runia_pixel_boundary_smooth_workspace_bytes(G, H, W, Wb, I, K) bytes (4 G H W when both
 *   steps run, else 0; 0 for what the call refuses), 4-byte aligned, uninitialised (RUNIA_E_WORKSPACE if missing or short).  (The
 *   query returns int64_t: its values are pinned on a grid of their own in tests/test_pixel_sml_host.py.) */
#define RUNIA_PIXSML_HEAD_SLOTS 8
#define RUNIA_PIXSML_MAX_CLASSES 1024
#define RUNIA_PIXSML_TILE_H 32
#define RUNIA_PIXSML_TILE_W 64
#define RUNIA_PIXSML_MAX_WIDTH 8
#define RUNIA_PIXSML_MAX_DILATION 8
#define RUNIA_PIXSML_MAX_KERNEL 7
int runia_pixel_sml_accumulate(const void* logits, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                               int64_t sh, int64_t sw, const void* valid, void* record, runia_stream_t stream);
int runia_pixel_sml_maps(const void* logits, int dtype, int64_t G, int64_t C, int64_t H, int64_t W, int64_t sn, int64_t sc,
                         int64_t sh, int64_t sw, const float* mean, const float* inv_std, float* sml, int32_t* label,
                         float* max_logit, runia_stream_t stream);
int64_t runia_pixel_boundary_smooth_workspace_bytes(int64_t G, int64_t H, int64_t W, int boundary_width,
                                                    int boundary_iterations, int kernel_size);
int runia_pixel_boundary_smooth_f32(const float* score, const int32_t* label, int64_t G, int64_t H, int64_t W,
                                    int boundary_width, int boundary_iterations, int kernel_size, int dilation,
                                    const float* taps, float* out, void* workspace, size_t workspace_bytes,
                                    runia_stream_t stream);

/* ---- sample-consistency scores of LLM generations (llm_uncertainty/consistency.py; csrc/consistency.hip) ----
 * Black-box scores from the sampled token ids alone: lexical similarity (mean pairwise ROUGE-L, Fomicheva et al. 2020) and
 * NumSet / Deg / Ecc / EigV over a pairwise similarity (Lin, Trivedi and Sun 2023).  Rows are prompt-major: group g = rows
 * g*k .. g*k+k-1.
 * runia_cons_pairs: ids holds groups * k rows of T ids, id_bytes 4 (int32) or 8 (int64, compared on all 64 bits), row_stride
 *   and col_stride in elements (both >= 0: sequences[:, start:] is passed as a view).  The content of a row ends before its
 *   first id that equals one of eos[0 .. n_eos-1] (int64, device; n_eos <= RUNIA_CONS_MAX_EOS, 0: none) and at lengths[row]
 *   (int64, device, nullable; clamped to [0, T]).  `what` = RUNIA_CONS_LCS | RUNIA_CONS_JACCARD selects the tables (int32):
 *     len   [groups * k]     content length n_i (always written);
 *     lcs   [groups, k, k]   length of the longest common subsequence of contents i and j, lcs[i, i] = n_i;
 *     uniq  [groups * k]     distinct ids of content i;          inter [groups, k, k]  distinct ids common to i and j.
 *   One wave per row (len), per unordered pair (lcs: the longer content across the lanes in registers, the shorter walked
 *   one wave-uniform id per step, row = prefix-max of the candidates; inter: binary search in the sorted distinct ids), one
 *   workgroup per row for the sort (bitonic in LDS, duplicates dropped).  Two launches for lcs, three for Jaccard, no
 *   synchronisation, no atomics: an entry depends on its own two rows only and two calls give equal bits.
 *   workspace: runia_cons_pairs_workspace_bytes(groups, k, T, what) bytes (the sorted distinct ids; 0 without
 *   RUNIA_CONS_JACCARD; the query returns int64_t), 8-byte aligned (RUNIA_E_WORKSPACE if missing or short).
 *   2 <= k <= RUNIA_CONS_MAX_K, 0 <= T <= RUNIA_CONS_MAX_T, groups >= 1, groups * k * k < 2^31; RUNIA_E_INVALID otherwise.
 * runia_cons_graph: W [groups, k, k] f64, contiguous; only the upper triangle is read and the diagonal is taken as 1.  With
 *   d_i = sum_j w_ij and L = I - D^-1/2 W D^-1/2 (eigenvalues lambda ascending, cyclic Jacobi in LDS with eigenvectors,
 *   eigen_score_kernel's rotation rule, ordering and stopping rule):
 *     eigenvalues [groups, k];  lexsim = mean_{i<j} w_ij;  u_deg = 1 - sum_ij w_ij / k^2;  c_deg[i] = d_i / k;
 *     u_eigv = sum_r max(0, 1 - lambda_r);  with s_i = the norm of row i of the eigenvectors of lambda < eigv_threshold,
 *     centred over the rows: c_ecc[i] = -s_i, u_ecc = sqrt(sum_i s_i^2);
 *     num_sets (int32) = connected components of the graph {w_ij >= set_threshold}.
 *   One workgroup per group, one launch, no atomics: a group's bits depend on that group alone.  A non-finite entry in the
 *   upper triangle of a group makes all its float outputs NaN and num_sets -1; a group still rotating after 30 sweeps gets
 *   NaN in eigenvalues, u_eigv, u_ecc and c_ecc.  2 <= k <= RUNIA_CONS_MAX_K, 1 <= groups < 2^31; RUNIA_E_INVALID otherwise. */
#define RUNIA_CONS_MAX_K 64
#define RUNIA_CONS_MAX_T 4096
#define RUNIA_CONS_MAX_EOS 16
#define RUNIA_CONS_LCS 1
#define RUNIA_CONS_JACCARD 2
int64_t runia_cons_pairs_workspace_bytes(int64_t groups, int64_t k, int64_t T, int what);
int runia_cons_pairs(const void* ids, int id_bytes, int64_t groups, int64_t k, int64_t T, int64_t row_stride,
                     int64_t col_stride, const int64_t* eos, int n_eos, const int64_t* lengths, int what, int32_t* len,
                     int32_t* lcs, int32_t* uniq, int32_t* inter, void* workspace, size_t workspace_bytes,
                     runia_stream_t stream);
int runia_cons_graph(const double* W, int64_t groups, int64_t k, double eigv_threshold, double set_threshold,
                     double* eigenvalues, double* u_deg, double* u_eigv, double* u_ecc, double* lexsim, double* c_deg,
                     double* c_ecc, int32_t* num_sets, runia_stream_t stream);

/* ---- anomaly maps of a mask classifier: RbA, max score, EAM (mask_level.hip; inference/mask_level.py) ----------- *
 * A mask classifier (MaskFormer, Mask2Former) gives Q class rows and Q low-resolution mask maps per image.  The reference
 * project has no such scores; this is the definition.
 *   class_logits (G, Q, Kc) through the element strides cg, cq, ck; Kc = K + 1 with has_void (the last column is "no object"),
 *   Kc = K without.  mask_logits (G, Q, h, w) through sn, sc, sh, sw.  Both f32 / f16 / bf16 (`*_dtype` 0, 1, 2), read in place,
 *   widened exactly, no f32 copy.  Target size (H, W), any ratio to (h, w).
 * class weights  P[g,q,k] = softmax_j(class_logits[g,q,:])[k], k < K: max-subtracted (the maximum skips NaNs, which then come
 *   back through exp), e_j = exp(x_j - max), the sum over ascending j in f32, P = e_k / sum.  a[g,q] = max_{k<K} P[g,q,k] (NaN if
 *   one is).
 * upsample  bilinear in logit space, the align_corners=False geometry of F.interpolate with the coordinates in integers:
 *   n = max((2Y + 1) h - H, 0), y0 = n div 2H, ly = (n mod 2H) / 2H rounded once to f32, y1 = min(y0 + 1, h - 1); x likewise.
 *   u = (1 - ly) ((1 - lx) m00 + lx m01) + ly ((1 - lx) m10 + lx m11), every operation rounded to f32, none contracted.  All four
 *   taps enter whatever the weights are (0 * inf = NaN, as in torch).  (H, W) == (h, w): u = m itself, no arithmetic.
 * sigmoid   s = 1 / (1 + exp(-u)) with the device's exp2-based exp and its reciprocal: exactly 0 and 1 at saturation, NaN for NaN.
 * scores    S[g,k,Y,X] = sum_q P[g,q,k] s[g,q,Y,X] over ascending q as an f32 fma chain (v_mfma_f32_32x32x2_f32).
 * outputs (each may be NULL, at least one set; (G, H, W) contiguous):
 *   rba f32       -sum_{k<K} tanh(S_k): the rows k with (k >> 2) even in ascending order, those with (k >> 2) odd likewise, then
 *                 the first sum plus the second.  Higher = anomalous.
 *   max_score f32 max_{k<K} S_k; NaN if an S_k is.  (Mask2Anomaly's score is 1 - max_score.)
 *   label int32   the lowest k attaining the max; -1 when the max is NaN.
 *   eam f32       -sum_q a[g,q] s[g,q,Y,X] (row K of the same product).  Higher = anomalous.
 *   semseg f32    (G, K, H, W) contiguous: S itself.
 *   A NaN mask logit makes the scores of the pixels whose four taps touch it NaN, and no others; a NaN class logit those of
 *   its own image.  No atomics, every sum in a fixed order: two calls give the same bits, and so does any subset of outputs.
 * Two launches: the prologue writes the weights Wt[g][row][q] (rows 0 .. K - 1 = P, row K = a, rows and q zero-padded to
 *   multiples of 32) and the interpolation tables (y0, ly)[H], (x0, lx)[W] into the workspace; the main launch gives a workgroup
 *   128 consecutive pixels of ONE image.
 * 1 <= K <= RUNIA_MASKQ_MAX_CLASSES, 1 <= Q <= RUNIA_MASKQ_MAX_QUERIES, G < 2^31, h, w, H, W <= RUNIA_MASKQ_MAX_SIDE (ly and lx
 *   are then one correctly rounded f32 division), G * H * W <= 2^RUNIA_MASKQ_MAX_PIXELS_LOG2, strides >= 0, the plane of one
 *   query spans fewer than 2^31 elements ((h - 1) sh + (w - 1) sw < 2^31); RUNIA_E_INVALID otherwise or for a missing pointer,
 *   before anything is launched.  G == 0 or H * W == 0: 0, nothing launched (h * w == 0 with H * W > 0 is invalid).
 *   workspace: runia_maskq_workspace_bytes(G, Q, K, H, W, h, w) bytes (0 for what the call refuses), 16-byte aligned,
 *   uninitialised (RUNIA_E_WORKSPACE if missing or short). */
#define RUNIA_MASKQ_MAX_CLASSES 255
#define RUNIA_MASKQ_MAX_QUERIES 1024
#define RUNIA_MASKQ_MAX_SIDE (1 << 23)
#define RUNIA_MASKQ_MAX_PIXELS_LOG2 34
int64_t runia_maskq_workspace_bytes(int64_t G, int64_t Q, int64_t K, int64_t H, int64_t W, int64_t h, int64_t w);
int runia_maskq_maps(const void* class_logits, int class_dtype, int64_t cg, int64_t cq, int64_t ck, int has_void,
                     const void* mask_logits, int mask_dtype, int64_t G, int64_t Q, int64_t K, int64_t h, int64_t w,
                     int64_t sn, int64_t sc, int64_t sh, int64_t sw, int64_t H, int64_t W, float* rba, float* max_score,
                     int32_t* label, float* eam, float* semseg, void* workspace, size_t workspace_bytes,
                     runia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RUNIA_HIP_H */
