/* cra5_amd - MI355X (gfx950) native VAEformer encode/decode path: C ABI.
 *
 * This is the drop-in boundary.  Plain pointers and sizes
 * only; no torch / pybind types.  Every function returns 0 on success; device
 * launchers return the hipError_t of the launch (as int) otherwise, host functions
 * a negative cra5 status.  No function allocates device memory; the caller owns all
 * buffers and passes the hipStream_t to launch on (as void*).
 *
 * Reference interfaces each entry point replaces (paths relative to the reference
 * tree taohan10200/CRA5):
 *   - FFI #1 `compressai.ans`  cra5/models/compressai/cpp_exts/rans/rans_interface.cpp:361-381
 *   - FFI #2 `compressai._CXX` cra5/models/compressai/cpp_exts/ops/ops.cpp:111-118
 *   - the ATen op sites of the hot path (the reference has no device kernels of its
 *     own): cra5/models/vaeformer/vit_nlc.py and
 *     cra5/models/compressai/entropy_models/entropy_models.py, cited per function.
 */
#ifndef CRA5_AMD_H
#define CRA5_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (host functions) ------------------------------------------- */
#define CRA5_OK 0
#define CRA5_ERR_ALLOC (-1)
#define CRA5_ERR_INDEX (-2)     /* cdf index out of range                         */
#define CRA5_ERR_PMF_DOMAIN (-3)/* negative / non-finite pmf entry (ops.cpp:46-52) */
#define CRA5_ERR_PMF_ZERO (-4)  /* all-zero pmf (ops.cpp:60-64)                    */
#define CRA5_ERR_PMF_STEAL (-5) /* no bin can donate frequency                     */
#define CRA5_ERR_STREAM (-6)    /* truncated / corrupt rANS stream                 */
#define CRA5_ERR_ARG (-7)
#define CRA5_ERR_UNAVAILABLE (-8) /* entry point not compiled into this build flavour */
#define CRA5_ERR_RANGE (-9)     /* a value does not fit the compact record type: use the 32-bit entry point */
#define CRA5_ERR_DESYNC (-10)   /* every symbol decoded, but the coder is not back at its initial state / words are left
                                 * over: the indexes or tables are not the encoder's (or the stream is damaged) - the
                                 * decoded symbols are NOT the coded ones.  One-shot decoders only (the whole stream). */

int cra5_abi_version(void);

/* ============================ host: entropy coding ============================ */

/* RansEncoder.encode_with_indexes (rans_interface.cpp:202-213 -> :108-200).
 * `cdfs` is a dense int32 matrix [n_cdfs][cdf_stride] (the `_quantized_cdf`
 * buffer), `cdf_sizes` = `_cdf_length`, `offsets` = `_offset`.  The stream
 * (little-endian 32-bit words) is malloc'ed into *out; release with cra5_free.
 * Thread-safe: no global state, so many frames can be coded concurrently. */
int cra5_rans_encode_with_indexes(const int32_t *symbols, const int32_t *indexes, size_t n,
                                  const int32_t *cdfs, int n_cdfs, int cdf_stride,
                                  const int32_t *cdf_sizes, const int32_t *offsets,
                                  uint8_t **out, size_t *out_len);

/* The same encoder fed with symbols ALREADY resolved against their tables (the table
 * lookups move to the GPU, cra5_rans_resolve_symbols_i32 below, the host loop is pure state update).
 * start_range[i] = start | range << 16 of the bin (the escape bin for out-of-range symbols);
 * esc[i] = 0 for a regular symbol, 1 + number of 4-bit payload nibbles (1..9) for an escape whose
 * payload is raw[i] (rans_interface.cpp:121-150), 255 = invalid index (-> CRA5_ERR_INDEX).
 * Produces byte-for-byte the stream of cra5_rans_encode_with_indexes. */
int cra5_rans_encode_resolved(const uint32_t *start_range, const uint32_t *raw, const uint8_t *esc, size_t n,
                              uint8_t **out, size_t *out_len);
/* The same on COMPACT records (6 instead of 9 bytes per latent between device and host): rec16[i] = 0 for a regular
 * symbol, (1 + payload nibbles) << 12 | payload for an escape whose payload fits 12 bits; a record 0xFFFF (payload
 * beyond 12 bits / invalid index) returns CRA5_ERR_RANGE - encode from the 32-bit records then; a record with payload
 * bits above its nibble count returns CRA5_ERR_INDEX.  Same bytes. */
int cra5_rans_encode_resolved_compact(const uint32_t *start_range, const uint16_t *rec16, size_t n, uint8_t **out,
                                      size_t *out_len);

/* RansDecoder.decode_with_indexes (rans_interface.cpp:215-284). `out` has n slots.
 * Unlike the reference (which reads past the end of a corrupt stream) a truncated
 * stream returns CRA5_ERR_STREAM, and a stream that decodes to the end WITHOUT returning the coder to its initial
 * state (RANS64_L, every word consumed) returns CRA5_ERR_DESYNC: the reference hands back garbage silently there. */
int cra5_rans_decode_with_indexes(const uint8_t *encoded, size_t len, const int32_t *indexes,
                                  size_t n, const int32_t *cdfs, int n_cdfs, int cdf_stride,
                                  const int32_t *cdf_sizes, const int32_t *offsets, int32_t *out);

/* The same decoder on COMPACT records (the frame path's device <-> host traffic: 3 bytes per latent instead of 8):
 * uint8 CDF indexes (the Gaussian tables have 64 rows), int16 symbols out.  A decoded symbol outside int16 returns
 * CRA5_ERR_RANGE with `out` partially written: decode again with cra5_rans_decode_with_indexes (same stream). */
int cra5_rans_decode_with_indexes_u8_i16(const uint8_t *encoded, size_t len, const uint8_t *indexes, size_t n,
                                         const int32_t *cdfs, int n_cdfs, int cdf_stride, const int32_t *cdf_sizes,
                                         const int32_t *offsets, int16_t *out);

/* Code `n_streams` independent streams on a pool of `n_threads` host threads
 * (frames are independent units: entropy_models.py:263-272). Arrays of per-stream
 * pointers; tables may be shared between streams. rc[i] receives each status. */
int cra5_rans_encode_batch(int n_streams, const int32_t *const *symbols,
                           const int32_t *const *indexes, const size_t *n,
                           const int32_t *const *cdfs, const int *n_cdfs, const int *cdf_stride,
                           const int32_t *const *cdf_sizes, const int32_t *const *offsets,
                           uint8_t **out, size_t *out_len, int *rc, int n_threads);
int cra5_rans_decode_batch(int n_streams, const uint8_t *const *encoded, const size_t *len,
                           const int32_t *const *indexes, const size_t *n,
                           const int32_t *const *cdfs, const int *n_cdfs, const int *cdf_stride,
                           const int32_t *const *cdf_sizes, const int32_t *const *offsets,
                           int32_t *const *out, int *rc, int n_threads);

void cra5_free(void *p);

/* Stateful forms of the same coder (class decls rans_interface.hpp:49-113):
 *   BufferedRansEncoder: push() any number of (symbols, indexes, tables) groups, then flush()
 *   codes them all - last pushed symbol first - into ONE stream (rans_interface.cpp:108-200);
 *   RansDecoder.set_stream()/decode_stream(): the decoder keeps its state between calls
 *   (rans_interface.cpp:286-359).  Handles are not thread-safe; use one per thread. */
void *cra5_rans_encoder_new(void);
int cra5_rans_encoder_push(void *enc, const int32_t *symbols, const int32_t *indexes, size_t n,
                           const int32_t *cdfs, int n_cdfs, int cdf_stride,
                           const int32_t *cdf_sizes, const int32_t *offsets);
int cra5_rans_encoder_flush(void *enc, uint8_t **out, size_t *out_len);
void cra5_rans_encoder_free(void *enc);
void *cra5_rans_decoder_new(void);
int cra5_rans_decoder_set_stream(void *dec, const uint8_t *encoded, size_t len);
int cra5_rans_decoder_decode_stream(void *dec, const int32_t *indexes, size_t n, const int32_t *cdfs,
                                    int n_cdfs, int cdf_stride, const int32_t *cdf_sizes,
                                    const int32_t *offsets, int32_t *out);
void cra5_rans_decoder_free(void *dec);

/* pmf_to_quantized_cdf (ops.cpp:40-108). cdf has n+1 slots. */
int cra5_pmf_to_quantized_cdf(const float *pmf, int n, int precision, uint32_t *cdf);

/* ============================ device: dense projections ======================= */

/* C[M,N] = epilogue( A[M,K] . W[N,K]^T ), fp32 in / fp32 MFMA accumulate
 * (v_mfma_f32_32x32x2_f32).  Replaces every nn.Linear / 1x1 Conv2d / im2col'ed
 * Conv2d / ConvTranspose2d GEMM on the path (vit_nlc.py:57-59,96,111,216-217,302,
 * 629-632,741; vaeformer.py:154-155).
 *   flags: CRA5_EPI_BIAS  -> + bias[n]
 *          CRA5_EPI_GELU  -> exact-erf GELU after bias (nn.GELU(), vit_nlc.py:52-69)
 *          CRA5_EPI_RES   -> + res[m*ldr + n] (residual stream / pos_embed; res may
 *                            alias C)
 * Requirements: K % 4 == 0, lda % 4 == 0, ldw % 4 == 0, 16-byte aligned A, W. */
#define CRA5_EPI_BIAS 1
#define CRA5_EPI_GELU 2
#define CRA5_EPI_RES 4
/* The mode word of the split-f16 engine: cra5_gemm_nt_split takes these bits in `flags` beside the CRA5_EPI_* ones,
 * cra5_gemm_nt_split_unembed and cra5_window_attention_split[_ws] take them as their `mode` (each names the words it
 * accepts; any other word is CRA5_ERR_ARG before a launch).
 * CRA5_GEMM_HI_ONLY: reduced-precision mode, hi.hi product only (plain f16 operands, fp32 accumulate, 1 MFMA per
 * product instead of 3) - BASELINE.json configs[4], RMSE-gated.  Only the hi plane of A / W is read, and only the hi
 * plane of C_split is WRITTEN (its lo halves, those of the pad columns included, keep whatever they held: a consumer of
 * that matrix must run in this mode too).  Kp > 8192 is taken in the chained form only (an fp32 output alone, no GELU:
 * CRA5_FORM_CHAINED); with a split output or a GELU it is CRA5_ERR_ARG - the one-launch long-K kernel has no
 * reduced-precision instantiation. */
#define CRA5_GEMM_HI_ONLY 8
/* With CRA5_GEMM_HI_ONLY, where the launch takes 64-wide k-steps (cra5_gemm_split_form; CRA5_ERR_ARG otherwise): the
 * operand / the split output is a PLAIN f16 matrix - a row is its k-values as contiguous halves (`lda_kp` / `ldw_kp` /
 * `ldc_split_kp` then count HALVES per row: a plain row may live in the first half of a split-layout row, pitch
 * 2 * Kp).  One full 128-byte line per row and 64-wide k-step instead of two half-lines: -13..-18 % per launch,
 * bit-identical results. */
#define CRA5_GEMM_A_PLAIN 16
#define CRA5_GEMM_W_PLAIN 32
#define CRA5_GEMM_OUT_PLAIN 64
/* With CRA5_GEMM_HI_ONLY, Kp % 64 == 0 and Kp <= 8192 (CRA5_ERR_ARG otherwise): take the wide form - 64-wide k-steps,
 * the summation order of every launch with >= 256 128 x 128 tiles - whatever the problem size.  A slice of such a GEMM
 * computed on its own (the rows / columns of a subset decode) then rounds exactly like the big launch; without the flag
 * a smaller problem takes the 32-wide k-step form, whose other summation order rounds differently.  Plain operands are
 * accepted at any size with it. */
#define CRA5_GEMM_WIDE_K 128
int cra5_gemm_nt_f32(const float *A, int lda, const float *W, int ldw, float *C, int ldc,
                     const float *bias, const float *res, int ldr, int M, int N, int K,
                     int flags, void *stream);

/* Same contraction, fp32-accurate, on the f16 matrix cores (3 x v_mfma_f32_32x32x16_f16 per
 * product, fp32 accumulate) with both operands in the "split-f16" layout: every fp32 value
 * x is stored as hi = f16(x), lo = f16(x - hi); a row is a sequence of 128-byte chunks of
 * [32 hi halves | 32 lo halves], Kp = K rounded up to a multiple of 32 with zero padding
 * (so a row has 2*Kp halves = the bytes of Kp floats).
 *   C = epi(wscale_inv * A . W^T); `wscale_inv` undoes the power-of-two scale applied to W
 *   when it was split.  Outputs: C (fp32, may be NULL) and/or C_split (split-f16 with row
 *   length ldc_split_kp, may be NULL) - e.g. fc1+GELU writes the split matrix fc2 reads.
 *   lda_kp / ldw_kp: row length (in K elements, multiples of 32) of the A / W buffers. */
int cra5_gemm_nt_split(const uint16_t *A, int lda_kp, const uint16_t *W, int ldw_kp, float *C,
                       int ldc, uint16_t *C_split, int ldc_split_kp, const float *bias,
                       const float *res, int ldr, int M, int N, int Kp, float wscale_inv,
                       int flags, void *stream);

/* The form a cra5_gemm_nt_split call of this shape, these flags and these outputs takes - THE rule, evaluated on the
 * host without a device: the launcher picks its kernel from this answer, and a caller that must name another launch's
 * form (a slice that promises the whole GEMM's bits) asks here instead of restating it.  CRA5_ERR_ARG: the launcher
 * refuses the combination.  Otherwise the tile's rows (64 / 128 / 192 / 256, form & CRA5_FORM_TILE) plus
 *   CRA5_FORM_K64      64-wide k-steps (reduced-precision mode, Kp % 64 == 0 and >= 256 128 x 128 tiles or
 *                      CRA5_GEMM_WIDE_K); else 32-wide.  Two calls sum a product's K terms in the same order exactly
 *                      when they agree in this bit (and in HI_ONLY and Kp),
 *   CRA5_FORM_CHAINED  Kp > 8192 with an fp32 output alone and no GELU: K is cut into chunks of <= 8192 (multiples of
 *                      64 in reduced-precision mode when Kp is one) that add up through C, every chunk in this form.
 *                      Any other Kp > 8192 runs one 128-row-tile launch with 32-wide steps in the fp32-accurate mode and
 *                      is CRA5_ERR_ARG with CRA5_GEMM_HI_ONLY,
 *   CRA5_FORM_PLAIN    plain rows are taken (some CRA5_GEMM_*_PLAIN bit is set: they need CRA5_FORM_K64). */
#define CRA5_FORM_TILE 0x1c0
#define CRA5_FORM_K64 1
#define CRA5_FORM_CHAINED 2
#define CRA5_FORM_PLAIN 4
int cra5_gemm_split_form(int M, int N, int Kp, int flags, int has_f32_out, int has_split_out);


/* fp32 [rows][K] (row stride ldx) * scale -> split-f16 [rows][2*Kp]. Used once per weight
 * tensor at load time and for the few activations no fused producer emits. */
int cra5_split_f16(const float *x, int ldx, uint16_t *out, int rows, int K, int Kp, float scale,
                   void *stream);

/* LayerNorm over the last dim (eps inside the sqrt), one row per wavefront
 * (partial(nn.LayerNorm, eps=1e-6): vit_nlc.py:266,278,381,626). D % 4 == 0, D <= 2048.
 * Outputs: y (fp32, may be NULL) and/or y_split (split-f16 rows of 2*split_kp halves, pad
 * columns zeroed, may be NULL).  split_plain != 0 (reduced-precision mode): y_split rows are PLAIN f16 - D
 * contiguous halves (+ zero pad to split_kp) at the start of each 2*split_kp-halves row - for a consumer
 * running with CRA5_GEMM_A_PLAIN. */
int cra5_layernorm_f32(const float *x, int ldx, const float *gamma, const float *beta, float *y,
                       int ldy, uint16_t *y_split, int split_kp, int rows, int D, float eps,
                       int split_plain, void *stream);

/* ============================ device: attention =============================== */

/* Streaming-softmax multi-head attention over windows of a (H, W) token grid, fp32
 * MFMA.  qkv: [H*W][3*C] rows = [q | k | v], each [heads][hd].  Windows are (wh, ww)
 * tiles of the grid zero-padded bottom/right to multiples of (wh, ww); a padded token
 * carries q = k = v = pad_row (the qkv bias) and attention is UNMASKED over the 576
 * tokens of a window (vit_nlc.py:219-258); wh = H, ww = W gives the global attention
 * of vit_nlc.py:94-112.  out: [H*W][C] (pre-projection), padded queries dropped.
 * hd must be 64 or 72.  out (fp32) and/or out_split (split-f16, rows of 2*split_kp halves;
 * pad columns are NOT written: zero the buffer once) may be NULL. */
int cra5_window_attention_f32(const float *qkv, const float *pad_row, float *out,
                              uint16_t *out_split, int split_kp, int C, int heads, int H, int W,
                              int wh, int ww, float scale, void *stream);

/* Same attention, fp32-accurate on the f16 matrix cores (hi/lo operand split, see
 * cra5_gemm_nt_split), reading the split-f16 qkv matrix [H*W][3C] the qkv projection wrote
 * (qkv_kp = 3C) and a split pad row, writing fp32 `out` and/or split-f16 `out_split`.
 * Requires head dim 64 and wh*ww % 32 == 0 (the 576-token windows and the 10 368-token global
 * attention); a window that is not the whole grid must have <= 1152 tokens (CRA5_ERR_ARG otherwise);
 * other shapes use cra5_window_attention_f32.  mode (the CRA5_GEMM_* mode word): 0, or CRA5_GEMM_HI_ONLY: the
 * reduced-precision mode (plain f16 q/k/v/p operands, 8 MFMAs per tile instead of 24; fp32 softmax statistics; only the
 * hi plane of out_split is written) on split rows, or CRA5_GEMM_HI_ONLY | CRA5_GEMM_A_PLAIN | CRA5_GEMM_OUT_PLAIN: that
 * mode on PLAIN f16 rows (qkv, the pad row and out_split: element n at half n, row pitches unchanged - plain rows in
 * means plain rows out, and the pad row goes with the input).  Any other mode: CRA5_ERR_ARG. */
int cra5_window_attention_split(const uint16_t *qkv_split, int qkv_kp, const uint16_t *pad_row_split,
                                float *out, uint16_t *out_split, int out_kp, int C, int heads,
                                int H, int W, int wh, int ww, float scale, int mode,
                                void *stream);

/* The same call with a caller-owned device workspace.  With it, the whole-grid (global) launch runs the BALANCED
 * schedule (vit_nlc.py:94-112): every head owns CUs / heads work-group slots of 12 waves (3 per SIMD); a slot first runs
 * full passes of 12 query tiles over the whole key loop, then the remaining query tiles - grouped by 12 - are laid end to
 * end with their key loops and cut into one equal piece per slot, whose un-normalised partial softmaxes a merge kernel
 * combines in fixed order (deterministic): 324 + 222.75 key steps per CU instead of 2 x 324 on 256 CUs at 10 368 tokens
 * x 16 heads.  cra5_attention_balanced_plan: 1 when a plan exists for (n_tokens, heads) on the current device - the
 * bytes it needs go to *workspace_bytes (0 is possible: a plan without a key-split part; `workspace` may then be NULL) -
 * 0 when the shape has no balanced schedule (the call is then cra5_window_attention_split).  The plan depends on the
 * device's CU count, and tokens of the key-split part differ from the plain launch by fp32 rounding (same accuracy
 * class): outputs of g_a / g_s are reproducible per device and schedule, not across them - only the hyper-prior path
 * (its own kernels) has to be bit-stable between encoder and decoder.  cra5_attention_workspace_bytes: the bytes alone
 * (0 also when no plan exists - kept for callers that only size a buffer). */
int cra5_attention_balanced_plan(int n_tokens, int heads, size_t *workspace_bytes);
size_t cra5_attention_workspace_bytes(int n_tokens, int heads);
int cra5_window_attention_split_ws(const uint16_t *qkv_split, int qkv_kp, const uint16_t *pad_row_split,
                                   float *out, uint16_t *out_split, int out_kp, int C, int heads,
                                   int H, int W, int wh, int ww, float scale, int mode,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* Un-embed as ONE fused launch pair (vit_nlc.py:628-630, 666-669: ConvTranspose2d(D -> C, kernel (11, 10), stride
 * (10, 10)) on the token grid): x[C][H][W] = overlap-add(A[M = Hp*Wp tokens][K] . W[N = C*110][K]^T) (* std + mean per
 * channel when both are given - the de-normalisation of cra5_api.py:268-271 fused as in cra5_col2im_f32).  The GEMM's
 * epilogue stores every accumulator straight into the image (the nine rows of a patch row that have one contribution)
 * or into `side` (the ky = 0 / ky = 10 rows: [C][Hp][2][W] floats, cra5_unembed_side_bytes), and a small second kernel
 * adds the overlap pairs in fixed order: no [tokens][C*110] column matrix, no pass over it, deterministic, and
 * bit-identical to cra5_gemm_nt_split + cra5_col2im_f32.  Only this geometry (kh 11, kw 10, strides 10, W % 4 == 0,
 * Kp <= 8192); cra5_unembed_side_bytes returns 0 and the launcher CRA5_ERR_ARG for anything else - use the two-call
 * form then.  mode (the CRA5_GEMM_* mode word): 0, or CRA5_GEMM_HI_ONLY with any of CRA5_GEMM_A_PLAIN (the A rows are
 * plain f16 rows) and CRA5_GEMM_W_PLAIN (the weight is a packed plain [N][Kp] f16 matrix); any other word is
 * CRA5_ERR_ARG.  The launch is the 256 x 256 tile; with CRA5_GEMM_HI_ONLY it takes the form cra5_gemm_split_form gives
 * for mode | CRA5_GEMM_WIDE_K - 64-wide k-steps whenever Kp % 64 == 0, which the plain rows need - and 32-wide steps
 * where that is refused. */
size_t cra5_unembed_side_bytes(int C, int H, int W, int kh, int kw, int sh, int sw);
int cra5_gemm_nt_split_unembed(const uint16_t *A, int lda_kp, const uint16_t *W_split, int ldw_kp, float *x,
                               float *side, size_t side_bytes, const float *mean, const float *stdv, int M, int Kp,
                               float wscale_inv, int C, int H, int W, int kh, int kw, int sh, int sw, int mode,
                               void *stream);

/* ============================ device: layout / conv edges ===================== */

/* Patch gather for a strided Conv2d as GEMM (vit_nlc.py:302-308), fused with the API's
 * normalisation (x - mean[c]) / std[c] (cra5_api.py:264-266) when mean != NULL.
 * x: [C][H][W]; cols: [Hp*Wp][ldk], column (c*kh + i)*kw + j; columns >= C*kh*kw are
 * left untouched (keep them zero).  cols (fp32) and/or cols_split (split-f16, Kp = ldk,
 * ldk % 32 == 0) may be NULL.  split_plain != 0 (reduced-precision mode): cols_split rows are PLAIN f16 - C*kh*kw
 * contiguous halves, zero padded to ldk, at the start of each 2*ldk-halves row (ERA5 patch geometry, or ldk == C*kh*kw). */
int cra5_im2col_f32(const float *x, const float *mean, const float *std, float *cols,
                    uint16_t *cols_split, int C, int H, int W, int kh, int kw, int sh, int sw,
                    int Hp, int Wp, int ldk, int split_plain, void *stream);

/* Overlap-add scatter of a ConvTranspose2d computed as GEMM (vit_nlc.py:628-630,
 * 666-669), fused with de-normalisation x*std[c] + mean[c] (cra5_api.py:268-271) when
 * mean != NULL.  cols: [Hp*Wp][ldn], column (c*kh + i)*kw + j;  x: [C][H][W] with
 * H = (Hp-1)*sh + kh, W = (Wp-1)*sw + kw. */
int cra5_col2im_f32(const float *cols, const float *mean, const float *std, float *x, int C,
                    int H, int W, int kh, int kw, int sh, int sw, int Hp, int Wp, int ldn,
                    void *stream);

/* Subset decode (csrc/subset.hip): the two copies around the un-embed of a patch-aligned superset of a lat/lon box.
 * cra5_gather_token_rows: dst row r = i * n_tj + j (i < n_ti, j < n_tj) <- src row (ti0 + i) * Wp + (tj0 + j) mod Wp of a
 * token-major matrix of Hp * Wp rows (the token columns wrap at the grid's east edge); `row_bytes` bytes per row copied
 * verbatim (split-f16, plain f16 or fp32 rows alike).  row_bytes, both pitches and both pointers 16-byte aligned;
 * 0 <= ti0, ti0 + n_ti <= Hp, 0 <= tj0 < Wp, 1 <= n_tj <= Wp - CRA5_ERR_ARG otherwise.
 * cra5_crop_f32: dst[c][i][j] = src[c][r0 + i][(c0 + j) mod Ws] for c < C, i < Hb, j < Wb; src [C][Hs][Ws], dst
 * [C][Hb][Wb], both contiguous, any element offset.  0 <= r0, r0 + Hb <= Hs, 0 <= c0 < Ws, 1 <= Wb <= Ws - CRA5_ERR_ARG
 * otherwise. */
int cra5_gather_token_rows(const void *src, size_t src_pitch_bytes, void *dst, size_t dst_pitch_bytes,
                           size_t row_bytes, int Hp, int Wp, int ti0, int n_ti, int tj0, int n_tj, void *stream);
int cra5_crop_f32(const float *src, int C, int Hs, int Ws, float *dst, int r0, int Hb, int c0, int Wb, void *stream);

/* Thinned decode (csrc/subset.hip; cra5_amd/subset.py stride_plan / scatter_tables): every s_lat-th row and s_lon-th
 * column of the global grid.  The tokens fall into classes that keep the same un-embed taps; each class pair is one small
 * GEMM (cra5_gemm_nt_split / cra5_gemm_nt_f32) on the class's token rows and the chosen channels' rows of its taps.
 * cra5_gather_token_lattice: cra5_gather_token_rows for a strided lattice - dst row r = i * n_tj + j <- src row
 * (ti0 + i * ti_step) * Wp + (tj0 + j * tj_step) mod Wp; same alignment rules; 0 <= ti0, ti0 + (n_ti - 1) * ti_step < Hp,
 * 0 <= tj0 < Wp, (n_tj - 1) * tj_step < Wp (one wrap at most, no token twice), steps >= 1 - CRA5_ERR_ARG otherwise.
 * cra5_strided_scatter_f32: x[c][i][j] (contiguous [C][Ho][Wo]) from the class matrices that lie in the workspace g of
 * g_elems floats.  Device tables: rows int32 [Ho][6] = (rc, ti, ky) of the row's first contribution and of its second
 * (rc = -1: none) - a seam row (image row 10 t, 0 < t < Hp) is token row t - 1's last tap, the UPPER partner, first, plus
 * token row t's tap 0; cols int32 [Wo][3] = (cc, tj, kx); cls int64 [n_rc * n_cc][5] = (offset, row pitch, n_tj, n_kx,
 * n_ky * n_kx) of class (rc, cc), whose matrix element is g[offset + (ti * n_tj + tj) * pitch + c * n_ky * n_kx + ky * n_kx
 * + kx] (ti, tj, ky, kx: indices within the class).  x = (first [+ second]) [* std[c] + mean[c] when mean != NULL] - the
 * order and arithmetic of the full decode's stores.  An element outside [0, g_elems) is not read: the point becomes NaN.
 * mean and std both NULL or both given; pointers aligned to their element size - CRA5_ERR_ARG otherwise. */
int cra5_gather_token_lattice(const void *src, size_t src_pitch_bytes, void *dst, size_t dst_pitch_bytes,
                              size_t row_bytes, int Hp, int Wp, int ti0, int ti_step, int n_ti, int tj0, int tj_step,
                              int n_tj, void *stream);
int cra5_strided_scatter_f32(const float *g, size_t g_elems, const int *rows, const int *cols, const long long *cls,
                             int n_rc, int n_cc, const float *mean, const float *stdv, float *x, int C, int Ho, int Wo,
                             void *stream);

/* Point decode (csrc/points.hip; cra5_amd/points.py Points.plan): the decoded frame at P (lat, lon) positions, [C][P].
 * cra5_gather_token_list: dst row r <- src row tok[r] (tok: int32 device [n_tok]), verbatim in 16-byte units - split,
 * plain and fp32 rows alike; cra5_gather_token_rows' alignment rules.  A tok[r] outside [0, n_src_rows) reads nothing and
 * fills the row with 0xFF bytes (a NaN as f16 and as fp32).
 * cra5_points_from_cols: the points out of the two-call un-embed's column matrix cols [M][pitch] (pitch in floats,
 * >= C * taps_per_channel; channel c's kh * kw products at column c * taps_per_channel) of the M gathered tokens.  Device
 * tables: nodes int32 [n_nodes][4] = (m0, tap0, m1, tap1), the node's value
 *   v = cols[m0][c * tpc + tap0];  if (m1 >= 0) v = v + cols[m1][c * tpc + tap1];  if (mean) v = v * std[c] + mean[c]
 * (a seam row's UPPER partner first: cra5_strided_scatter_f32's expression, order and contraction); pnode int32 [P][4]:
 * the node of (row tap t, column tap u) at entry 2 t + u, -1 = no such tap; rw, cw fp64 [P][2]: the taps' weights.
 * nearest != 0: out[c][p] = v(pnode[p][0]), copied (-0.0 and NaN payloads survive; rw / cw may be NULL).  Otherwise, in
 * fp64, every operation rounded on its own (no contraction), sums from 0.0, north to south over west to east:
 *   out[c][p] = (float) sum_t rw[p][t] * (sum_u cw[p][u] * (double)v(node[p][t][u]))     - cra5_regrid_f32's arithmetic.
 * cra5_points_from_image: the same two rules with the node value read from the image x [C][H][W]; rows, cols int32 [P][2]:
 * the row taps / column taps, -1 = no second tap.
 * A table entry outside its source (a node outside [0, n_nodes), a token row outside [0, M), a tap outside [0, tpc), a
 * row / column outside the image) is never read: the point becomes NaN.  CRA5_ERR_ARG, before any device work, for NULL /
 * misaligned pointers, sizes <= 0, C > 65535, C * P or C * taps_per_channel or H * W beyond int32, C * taps_per_channel >
 * pitch, mean without std. */
int cra5_gather_token_list(const void *src, size_t src_pitch_bytes, void *dst, size_t dst_pitch_bytes, size_t row_bytes,
                           int n_src_rows, const int *tok, int n_tok, void *stream);
int cra5_points_from_cols(const float *cols, size_t pitch, int M, int C, int taps_per_channel, const int *nodes,
                          int n_nodes, const int *pnode, const double *rw, const double *cw, int P, int nearest,
                          const float *mean, const float *stdv, float *out, void *stream);
int cra5_points_from_image(const float *x, int C, int H, int W, const int *rows, const int *cols, const double *rw,
                           const double *cw, int P, int nearest, float *out, void *stream);

/* Area-weighted coarsening (csrc/window_reduce.hip; cra5_amd/subset.py coarsen_plan): the first-order
 * conservative regrid of src - fp32 [C_src][Hs][Ws], contiguous, whose element [.][0][0] is the GLOBAL grid point (src_r0,
 * src_c0) of an H x W grid; whole_circle != 0: Ws == W and src_c0 == 0, windows wrap at the east edge - onto the Ho x Wo
 * points of global rows out_r0 + i * k_lat and global columns (out_c0 + j * k_lon) mod W -> dst fp32 [C_out][Ho][Wo],
 * contiguous.  Output channel c reads source channel chan_map[c] (int32 [C_out] on the device) or c when chan_map is NULL
 * (then C_out <= C_src); a mapped channel outside [0, C_src) gives NaN.  Device tables: row0 / ntap int32 [Ho] - the first
 * global source row and the row count (<= rw_pitch) of output row i's window; rw fp64 [Ho][rw_pitch] - its row weights.
 * Per output point, in fp64, every operation rounded on its own (no contraction):
 *   acc = 0;  for t < ntap[i], north to south:  inner = 0;  for w = col - k_lon / 2 .. col + k_lon / 2 (mod W), west to
 *   east:  inner = inner + ov * (double)src[row0[i] + t][w]  (ov = 1/2 on the two edge columns of an even k_lon, else 1);
 *   acc = acc + rw[i][t] * inner;   dst = (float)acc.
 * The order depends on the global (row, column) only: a region's result is the sub-block of the globe's, bit for bit.
 * Non-finite samples propagate (IEEE); nothing is filtered.  One pass, no atomics, 64-bit element offsets; any 4-byte
 * aligned src / dst.  A table row outside the source is not read: the output row becomes NaN.  CRA5_ERR_ARG, before any
 * device work, for NULL / misaligned pointers (chan_map may be NULL), sizes <= 0, a source box outside the grid, a
 * whole-circle flag on another box, Wo * k_lon > W, output rows beyond H - 1, a window (out_r0 - k_lat / 2 .. last row +
 * k_lat / 2 clipped to the grid; out_c0 - k_lon / 2 .. eastward) that leaves the source, and k_lon > 8175. */
int cra5_coarsen_f32(const float *src, int C_src, int Hs, int Ws, int src_r0, int src_c0, int H, int W, int whole_circle,
                     int out_r0, int k_lat, int Ho, int out_c0, int k_lon, int Wo, const int *row0, const int *ntap,
                     const double *rw, int rw_pitch, const int *chan_map, int C_out, float *dst, void *stream);

/* Regridding onto any rectilinear lat/lon grid (csrc/window_reduce.hip; cra5_amd/regrid.py Grid.plan):
 * bilinear interpolation or first-order conservative remapping of src - fp32 [C_src][Hs][Ws], contiguous, whose element
 * [.][0][0] is the GLOBAL grid point (src_r0, src_c0) of an H x W grid; Ws == W: the whole circle, src_c0 == 0, windows
 * wrap at the east edge - onto Ho x Wo target points -> dst fp32 [C_out][Ho][Wo], contiguous.  chan_map: as in
 * cra5_coarsen_f32.  Device tables: row0 / ntap int32 [Ho], rw fp64 [Ho][rw_pitch] - the first global source row, the row
 * count (<= rw_pitch) and the weights of target row i's window; order int32 [Ho] - the target rows from north to south
 * (the walk; row order[k] is written); col0 / ctap int32 [Wo], cw fp64 [Wo][cw_pitch] - the same along the columns, window
 * column u is source column (col0[j] + u) mod W; tiles int32 [n_tiles][4] - (first target column, column count <=
 * tile_cols, first global source column of the tile's span, span length <= max_span) per column tile.
 *   inner(h, j)  = sum over u, west to east,   of cw[j][u] * (double)src(h, (col0[j] + u) mod W)
 *   dst[c][i][j] = (float) sum over t, north to south, of rw[i][t] * inner(row0[i] + t, j)
 * in float64, every sum from 0, every product and add rounded on its own: bit-identical from run to run, a sub-grid's
 * result is the sub-block of the whole target grid's.  Non-finite samples propagate (IEEE).  One pass, no atomics, any
 * 4-byte aligned src / dst.  A table entry that names a row, a column window or a span outside the source is not read:
 * those outputs become NaN.  CRA5_ERR_ARG, before any device work, for NULL / misaligned pointers (chan_map may be NULL),
 * sizes <= 0, a source box outside the grid, a box as wide as the grid that does not start at column 0, rw_pitch > H,
 * cw_pitch > 64 or > W, tile_cols > 256 or tile_cols * cw_pitch > 4096, n_tiles > Wo, max_span > 7936 or > 2 W. */
int cra5_regrid_f32(const float *src, int C_src, int Hs, int Ws, int src_r0, int src_c0, int H, int W, int Ho, int Wo,
                    const int *row0, const int *ntap, const double *rw, int rw_pitch, const int *order, const int *col0,
                    const int *ctap, const double *cw, int cw_pitch, const int *tiles, int n_tiles, int tile_cols,
                    int max_span, const int *chan_map, int C_out, float *dst, void *stream);

/* Finiteness probe of the range guard: partials[b] = sum of x[i * stride] over block b's share of i = 0 .. ceil(n / stride)
 * - 1, b = 0 .. CRA5_PROBE_PARTIALS - 1 (written, never accumulated: no memset, deterministic).  A partial is non-finite as
 * soon as one addend is; the caller copies the partials to the host with the phase's other results and tests them there. */
#define CRA5_PROBE_PARTIALS 256
int cra5_probe_sums_f32(const float *x, size_t n, size_t stride, float *partials, void *stream);

/* Per-channel reconstruction error of a frame (csrc/metrics.hip): x_hat, x [C][H][W] fp32 (any W; 16-byte aligned
 * bases take the float4 path), d = x_hat - x.  out [C][CRA5_RECON_FIELDS] fp64, per channel c:
 *   BIAS = mean d,  MSE = mean d^2,  WMSE = mean lat_w[h] d^2 (lat_w [H] fp32; NULL: weight 1),  MAE = mean |d|,
 *   MAX_ABS = max |d| (the fp32 value, exact),  NONFINITE = count of (h, w) where x or x_hat is NaN / +-inf;
 * means are over all H*W positions; a channel with NONFINITE > 0 has NaN in the other five fields.  `slab`: caller-owned
 * device scratch of >= cra5_recon_error_slab_bytes(C, H, W) bytes (one fp64 record per block, overwritten: no memset).
 * Two launches on `stream`, fixed reduction order: bit-identical from run to run.  slab_bytes returns 0 for bad
 * dimensions (C, H, W > 0, H * W < 2^31); the launcher returns CRA5_ERR_ARG for those, for NULL pointers (lat_w may be
 * NULL) and for a slab that is too small. */
#define CRA5_RECON_FIELDS 6
#define CRA5_RECON_BIAS 0
#define CRA5_RECON_MSE 1
#define CRA5_RECON_WMSE 2
#define CRA5_RECON_MAE 3
#define CRA5_RECON_MAX_ABS 4
#define CRA5_RECON_NONFINITE 5
size_t cra5_recon_error_slab_bytes(int C, int H, int W);
int cra5_recon_error_f32(const float *x_hat, const float *x, int C, int H, int W, const float *lat_w, double *slab,
                         size_t slab_bytes, double *out, void *stream);

/* Packed int16 output (csrc/pack.hip; DESIGN.md section 4, "Packed int16 output").  x [C][plane] fp32, contiguous,
 * 4-byte aligned (a 16-byte aligned base and plane % 4 == 0 are not needed).  Per channel c:
 *   an element is finite when its exponent bits are not all ones; NONFINITE = the count of the others; VMIN / VMAX = the
 *   fp32 min / max over the finite elements (exact; NaN when there are none; of +0 and -0 either may be reported);
 *   range (lo, hi) in float64 = fixed[c] when `fixed` is given and fixed[c][0] is not NaN (the caller guarantees finite
 *   lo < hi), else ((double)VMIN, (double)VMAX);
 *   no finite element and no fixed range: SCALE = 1, OFFSET = 0;  lo == hi: SCALE = 1, OFFSET = lo;  otherwise
 *   SCALE = (hi - lo) / 65534.0 and OFFSET = (lo + hi) * 0.5, in IEEE float64.
 * cra5_pack_range_f32 writes out [C][CRA5_PACK_FIELDS] fp64 (VMIN, VMAX, NONFINITE, SCALE, OFFSET).  fixed: device fp64
 * [C][2] or NULL.  `slab`: caller-owned device scratch of >= cra5_pack_range_slab_bytes(C, plane) bytes, 16-byte aligned
 * (one record per block, overwritten: no memset, no atomics).  Two launches on `stream`, fixed reduction order: the table
 * is bit-identical from run to run.
 * cra5_pack_i16_f32 reads SCALE / OFFSET of such a table (device, [C][CRA5_PACK_FIELDS]) and writes q [C][plane] int16
 * (2-byte aligned), nothing outside it: a non-finite x gives CRA5_PACK_FILL, any other
 *   q = (int16) clamp(rint(((double)x - OFFSET) / SCALE), -32767, 32767),
 * the subtraction and a true division in float64, rint to nearest-even, the clamp in float64 before the conversion.
 * unpack(q) = (double)q * SCALE + OFFSET; for every finite x inside (lo, hi):
 *   |unpack(q) - x| <= SCALE * (0.5 + 2^-30) + 2^-50 * max(|lo|, |hi|).
 * slab_bytes returns 0 and the launchers CRA5_ERR_ARG, before any device work, for C <= 0, plane == 0 or >= 2^31, NULL
 * (fixed may be NULL) or misaligned pointers and a slab that is too small. */
#define CRA5_PACK_FIELDS 5
#define CRA5_PACK_VMIN 0
#define CRA5_PACK_VMAX 1
#define CRA5_PACK_NONFINITE 2
#define CRA5_PACK_SCALE 3
#define CRA5_PACK_OFFSET 4
#define CRA5_PACK_FILL (-32768)
size_t cra5_pack_range_slab_bytes(int C, size_t plane);
int cra5_pack_range_f32(const float *x, int C, size_t plane, const double *fixed, void *slab, size_t slab_bytes,
                        double *out, void *stream);
int cra5_pack_i16_f32(const float *x, int C, size_t plane, const double *table, int16_t *q, void *stream);

/* Packed int16 input (csrc/pack.hip; DESIGN.md section 4, "Packed int16 input"): the inverse direction, for frames that
 * arrive as int16 codes with scale_factor / add_offset / _FillValue (the NetCDF layout of ERA5).  q [C][plane] int16
 * (2-byte aligned), x [C][plane] fp32 (4-byte aligned), table device fp64 [C][CRA5_UNPACK_FIELDS] = (SCALE, OFFSET, FILL,
 * MUL); MUL holds a value that is exact in fp32.  Per channel c and code q:
 *   q == FILL[c] (FILL[c] not NaN: a NaN FILL is "no fill code")  ->  x = the quiet NaN 0x7fc00000; otherwise
 *   d = (double)q * SCALE[c], rounded to float64;  d = d + OFFSET[c], rounded to float64 (two roundings, never a fused
 *   multiply-add);  x = (float)d, to nearest even;  x = x * (float)MUL[c], one fp32 multiply.
 * flags: CRA5_UNPACK_SWAPPED - the two bytes of every code are in the other order (NetCDF-3 stores big-endian) and are
 * swapped in registers.  One launch on `stream`; nothing outside x is written, q and table are only read.  Any NULL or
 * misaligned pointer, C <= 0, plane == 0 or >= 2^31 and any unknown flag bit return CRA5_ERR_ARG before any device work. */
#define CRA5_UNPACK_FIELDS 4
#define CRA5_UNPACK_SWAPPED 1u
int cra5_unpack_i16_f32(const int16_t *q, int C, size_t plane, const double *table, unsigned flags, float *x,
                        void *stream);

/* Zonal power spectra of a frame pair (csrc/spectrum.hip): x_hat, x [C][H][W] fp32, d = x_hat - x in
 * fp32.  For a row f(c, h, .):  F(c, h, k) = sum_w f(c, h, w) e^(-2 pi i k w / W),  k = 0 .. K - 1,  K = W / 2 + 1, and
 *   P_f(c, k) = (1 / H) sum_h L(h) m_k |F(c, h, k)|^2 / W^2,   m_k = 1 for k = 0 and for k = W / 2 of an even W, else 2,
 * L(h) = (double)lat_w[h] (fp32 [H]; NULL: 1); every operation after the fp32 subtraction is float64.  sum_k P_f(c, k) =
 * mean_(h,w) L(h) f^2 (Parseval): sum_k P_d is the WMSE of cra5_recon_error_f32.  out [3][C][K] fp64: P_x, P_x_hat, P_d.
 * nonfinite [C] fp64: the count of (h, w) where x or x_hat is NaN / +-inf, as CRA5_RECON_NONFINITE; such a channel has NaN
 * in every bin of its three spectra, the other channels are unaffected.  W >= 2 with no prime factor above 5, W <=
 * CRA5_SPECTRUM_MAX_W.  twiddle: device fp64 [W][2], (cos, sin) of -2 pi j / W, 16-byte aligned.  `slab`: caller-owned
 * device scratch of >= cra5_zonal_spectrum_slab_bytes(C, H, W) bytes (one partial per block, overwritten: no memset).  16-byte
 * aligned frames with W % 4 == 0 take the float4 path, any other 4-byte aligned frames go element by element.  Two launches
 * on `stream`, no atomics, fixed order of operations: bit-identical from run to run.  slab_bytes returns 0 for bad
 * dimensions (C in 1 .. 65535, H > 0, H * W < 2^31, an unsupported W); the launcher returns CRA5_ERR_ARG, before any device
 * work, for those, for NULL / misaligned pointers (lat_w may be NULL) and for a slab that is too small. */
#define CRA5_SPECTRUM_MAX_W 1440
size_t cra5_zonal_spectrum_slab_bytes(int C, int H, int W);
int cra5_zonal_spectrum_f32(const float *x_hat, const float *x, int C, int H, int W, const float *lat_w,
                            const double *twiddle, double *slab, size_t slab_bytes, double *out, double *nonfinite,
                            void *stream);

/* Exact quantiles of a frame pair (csrc/quantile.hip; DESIGN.md section 4, "Quantiles"): x_hat, x [C][H][W] fp32, 4-byte
 * aligned.  Per channel three fields: truth x, recon x_hat, abs_error |x_hat - x| (the fp32 difference of the metric).
 * row_w: device uint32 [H], the integer weight of every row (<= 2^20; a row of weight 0 does not count), or NULL = all 1.
 * targets: device uint64 [Q], 1 <= targets[q] <= W * sum_h row_w[h] (the caller's duty).  Q_f(c, q) = the smallest value v
 * of field f in channel c for which the summed weight of the points with value <= v reaches targets[q]: an element of the
 * field with its own fp32 bits (-0 and +0 are one value, the sign of a returned zero is unspecified), nothing interpolated.
 * out, device fp64 [3 * C * Q + C]: the three [C][Q] blocks in the order truth, recon, abs_error, every fp32 result
 * widened exactly, then the [C] counts of points where x or x_hat is NaN / +-inf (as CRA5_RECON_NONFINITE); a channel
 * with such a point has NaN in all its 3 * Q results, the other channels are unaffected.  `ws`: caller-owned device
 * scratch of >= cra5_frame_quantiles_ws_bytes(C, H, W, Q) bytes, 8-byte aligned; the launcher initialises it on `stream`.
 * Nine launches on `stream` (init, then four 8-bit digit passes of count + select); all counting is in unsigned integers,
 * so the result is bit-identical from run to run.  ws_bytes returns 0 for bad dimensions (C, H, W < 1, H * W >= 2^31, Q
 * outside 1 .. CRA5_QUANTILE_MAX_Q); the launcher returns CRA5_ERR_ARG, before any device work, for those, for NULL
 * pointers (row_w may be NULL), a misaligned or short workspace. */
#define CRA5_QUANTILE_MAX_Q 16
size_t cra5_frame_quantiles_ws_bytes(int C, int H, int W, int Q);
int cra5_frame_quantiles_f32(const float *x_hat, const float *x, int C, int H, int W, const uint32_t *row_w,
                             const uint64_t *targets, int Q, void *ws, size_t ws_bytes, double *out, void *stream);

/* Per-grid-point statistics over many frames (csrc/timestats.hip): flat fp32 frames x of n elements, accumulators of the
 * same n elements - sum / sumsq fp64, mn / mx fp32.  Each accumulator pointer may be NULL (that statistic is not kept: it
 * is neither read nor written); at least one is given.  Per element i, v = (double)x[i]:
 *   first != 0:  sum = v,  sumsq = v * v,  mn = mx = x[i]   (plain stores: no memset, uninitialised accumulators are fine)
 *   first == 0:  sum += v, sumsq += v * v, mn = min(mn, x[i]), mx = max(mx, x[i])
 * v * v is exact in fp64, every update rounds once: calls in frame order on one stream (or chained by events) leave in
 * sum / sumsq the bits of a sequential float64 loop.  min / max return NaN if either operand is NaN (numpy's minimum /
 * maximum); the sign of a zero result is unspecified.  Non-finite samples are not filtered.  16-byte aligned bases take
 * the float4 / double2 path, anything else goes element by element; pointers aligned to their element size.
 * cra5_time_finish_f32 (mean / std may each be NULL, not both), every operation in fp64, uncontracted, in this order:
 *   mean[i] = (float)(sum[i] / count)
 *   std[i]  = (float)sqrt(max(0, (sumsq[i] - sum[i] * sum[i] / count) / (count - ddof)))
 * std needs sum and sumsq, mean needs sum; ddof >= 0 and count - ddof >= 1.  CRA5_ERR_ARG, before any device work, for
 * n == 0, no accumulator / no output, std without sumsq, count - ddof < 1 and misaligned pointers. */
int cra5_time_accumulate_f32(const float *x, size_t n, int first, double *sum, double *sumsq, float *mn, float *mx,
                             void *stream);
int cra5_time_finish_f32(size_t n, long long count, int ddof, const double *sum, const double *sumsq, float *mean,
                         float *stdv, void *stream);

/* Error-bounded residual layer (csrc/residual.hip; DESIGN.md section 4, "Residual layer").  x (truth), x_hat (the plain
 * decode) [C][H][W] fp32, tol [C] fp32 on the device: finite > 0, or +inf = the channel is not corrected.  Per point of a
 * corrected channel, step = fp32 2 * tol:  d = (double)x - (double)x_hat,  q = rint(d / (double)step);  d not finite or
 * |q| > 32767: an ESCAPE;  t = x_hat for q == 0, else fl32(x_hat + fl32((float)q * step)) (two roundings, no FMA);
 * |(double)x - (double)t| <= (double)tol: accepted - q != 0 stores the RECORD (idx, q), q == 0 nothing -, else an ESCAPE
 * (idx, the 32 bits of x).  idx = (c * H + r) * W + col as uint32: C * H * W < 2^32 (and H * W < 2^31).
 * Quantise = three calls on one stream, no atomics, the arrays identical from run to run and ascending in idx:
 *   count: counts [S][2] uint32 = (records, escapes) of every span of CRA5_RESIDUAL_SPAN elements (spans never straddle a
 *     channel; S = cra5_residual_spans = C * ceil(H * W / span), 0 for unsupported dimensions);
 *   scan:  offs [S + 1][2] uint32 = exclusive prefix sums of counts (last row: the totals n, m), chan [C][2] int64 = the
 *     totals per channel (one block);
 *   emit:  idx [n] uint32, q [n] int16, eidx [m] uint32, ebits [m] uint32 at the scanned offsets (n, m: the capacities, the
 *     totals of the scan; nothing is stored past them; n == m == 0 launches nothing and the four pointers may be NULL).
 * Frames: any 4-byte aligned base; a span whose two start addresses are 16-byte aligned is read with 16-byte loads.
 * Apply: out [Cs][Ho][Wo] fp32, the decode's output for chan_lut [C] int32 (output channel of c, -1 = absent; NULL = the
 * identity), the rows r of [r0, r1) with r % s_lat == 0 and the columns col with (col - c0) mod W < nc and col % s_lon == 0
 * (W % s_lon == 0), in that order - Ho / Wo must be their counts.  One thread per entry: a record adds fl32((float)q *
 * step[c]) to its point (step [C] fp32), an escape stores its bits; entries outside the output are skipped.  gather: got
 * [nw][2] uint32 = (1, the bits of out at widx[i]) or (0, 0) for a point outside the output - the witness check, run before
 * the apply.  CRA5_ERR_ARG, before any device work, for bad dimensions / geometry, NULL or misaligned pointers. */
#define CRA5_RESIDUAL_SPAN 4096
size_t cra5_residual_spans(int C, int H, int W);
int cra5_residual_count_f32(const float *x, const float *x_hat, const float *tol, int C, int H, int W, uint32_t *counts,
                            void *stream);
int cra5_residual_scan(const uint32_t *counts, int C, int H, int W, uint32_t *offs, long long *chan, void *stream);
int cra5_residual_emit_f32(const float *x, const float *x_hat, const float *tol, int C, int H, int W, const uint32_t *offs,
                           uint32_t *idx, int16_t *q, size_t n, uint32_t *eidx, uint32_t *ebits, size_t m, void *stream);
int cra5_residual_apply_f32(float *out, int Cs, int Ho, int Wo, int C, int H, int W, const int *chan_lut, int r0, int r1,
                            int s_lat, int c0, int nc, int s_lon, const float *step, const uint32_t *idx, const int16_t *q,
                            size_t n, const uint32_t *eidx, const uint32_t *ebits, size_t m, void *stream);
int cra5_residual_gather_f32(const float *out, int Cs, int Ho, int Wo, int C, int H, int W, const int *chan_lut, int r0,
                             int r1, int s_lat, int c0, int nc, int s_lon, const uint32_t *widx, size_t nw, uint32_t *got,
                             void *stream);

/* out[c][r] = in[r][c] (token-major <-> NCHW plumbing, vit_nlc.py:484, 684). */
int cra5_transpose_f32(const float *in, int ld_in, float *out, int ld_out, int rows, int cols,
                       void *stream);

/* 'b h w (p1 p2 c) -> b c (h p1) (w p2)' (vit_nlc.py:672-679): lin [Hz*Wz][p1*p2*Cout]
 * -> out [Cout][Hz*p1][Wz*p2]. */
int cra5_pixel_shuffle_f32(const float *lin, float *out, int Hz, int Wz, int p1, int p2,
                           int Cout, void *stream);

/* CNN zoo (bmshj2018-factorized / -hyperprior, mbt2018-mean: cra5/models/compressai/models/google.py:64-508;
 * conv / deconv of models/utils.py:128-147).  Conv2d(k, s, padding p): zero-padded patch gather into the
 * split-f16 GEMM operand, cols_split [Ho*Wo][2*ldk], column (c*kh + i)*kw + j, pad columns zero.
 * ConvTranspose2d(k, s, padding p, output_padding): cols = in^T . W (GEMM, fp32 [Hi*Wi][ldn], column
 * (co*kh + i)*kw + j), then out[co][y][x] = bias[co] + sum of the contributions with y = yi*s - p + i. */
int cra5_conv_im2col_f32(const float *x, uint16_t *cols_split, int C, int H, int W, int kh, int kw, int sh, int sw,
                         int ph, int pw, int Ho, int Wo, int ldk, void *stream);
int cra5_deconv_col2im_f32(const float *cols, const float *bias, float *out, int Cout, int Hi, int Wi, int kh, int kw,
                           int sh, int sw, int ph, int pw, int Ho, int Wo, int ldn, void *stream);
/* y = leaky_relu(x, slope) (op 0, any slope), |x| (op 1) or relu(x) (op 2), each bit-identical to torch's;
 * x == y allowed. */
int cra5_unary_f32(const float *x, float *y, size_t n, int op, float slope, void *stream);

/* ============================ device: entropy models ========================== */

/* GaussianConditional, eval mode (entropy_models.py:645-685, 155-201):
 *   s = max(scale, bound);  idx = (n_table-1) - #{t in table[0:n_table-1] : s <= t}
 *   sym = (int)rintf(y - mean);  y_hat = sym + mean
 *   lik = max(Phi((.5-|y_hat-mean|)/s) - Phi((-.5-|y_hat-mean|)/s), lik_bound)
 * Any output pointer may be NULL.  If y == NULL and sym_in != NULL the kernel
 * de-quantises instead: y_hat = sym_in + mean (decode side, :192-201). */
int cra5_gaussian_conditional_f32(const float *y, const int32_t *sym_in, const float *scales,
                                  const float *means, const float *scale_table, int n_table,
                                  float scale_bound, float lik_bound, int32_t *idx, int32_t *sym,
                                  float *y_hat, float *lik, size_t n, void *stream);
/* Decode-side halves of the same op on compact records: idx8 = the CDF index as uint8 (n_table <= 256), or - with
 * sym16_in - y_hat = sym16_in + mean.  Same arithmetic as cra5_gaussian_conditional_f32 (bit-identical idx / y_hat). */
int cra5_gaussian_conditional_compact_f32(const float *scales, const float *means, const float *scale_table, int n_table,
                                          float scale_bound, const int16_t *sym16_in, uint8_t *idx8, float *y_hat,
                                          size_t n, void *stream);

/* EntropyBottleneck, eval mode (entropy_models.py:434-510, 529-542): z is [C][n_per_ch];
 *   sym = (int)rintf(z - median[c]);  z_hat = sym + median[c]
 *   lik = max(sigmoid(logits(z_hat+.5)) - sigmoid(logits(z_hat-.5)), lik_bound)
 * params: per channel 58 floats: softplus(M0)[3] b0[3] tanh(f0)[3] | softplus(M1)[9] b1[3]
 * tanh(f1)[3] | M2.. | M3.. | softplus(M4)[3] b4[1]  (prepared on the host).
 * If z == NULL and sym_in != NULL: z_hat = sym_in + median (decode side). */
int cra5_entropy_bottleneck_f32(const float *z, const int32_t *sym_in, const float *medians,
                                const float *params, float lik_bound, int32_t *sym, float *z_hat,
                                float *lik, int C, int n_per_ch, void *stream);

/* GDN / IGDN (cra5/models/compressai/layers/gdn.py:76-92): x, y: [B][C][HW];
 * y = x * rsqrt(beta[i] + sum_j gamma[i][j] x_j^2)   (inverse: * sqrt).
 * beta / gamma are the re-parametrised (effective) values. */
/* Device side of cra5_rans_encode_resolved: symbols / indexes / tables are DEVICE pointers (the
 * model's _quantized_cdf [n_cdfs][cdf_stride], _cdf_length, _offset buffers); writes start_range,
 * raw and esc (n entries each) as described there.  rans_interface.cpp:121-150 per element. */
int cra5_rans_resolve_symbols_i32(const int32_t *symbols, const int32_t *indexes, size_t n, const int32_t *cdfs,
                                  int n_cdfs, int cdf_stride, const int32_t *cdf_sizes, const int32_t *offsets,
                                  uint32_t *start_range, uint32_t *raw, uint8_t *esc, void *stream);
/* Device side of cra5_rans_encode_resolved_compact; *overflow (device int32) is zeroed on the stream, then set to 1 when
 * any record is 0xFFFF. */
int cra5_rans_resolve_symbols_compact(const int32_t *symbols, const int32_t *indexes, size_t n, const int32_t *cdfs,
                                      int n_cdfs, int cdf_stride, const int32_t *cdf_sizes, const int32_t *offsets,
                                      uint32_t *start_range, uint16_t *rec16, int32_t *overflow, void *stream);

int cra5_gdn_f32(const float *x, const float *beta, const float *gamma, float *y, int B, int C,
                 int HW, int inverse, void *stream);

/* ---- hyper-prior path (HyperpriorEncoder / HyperpriorDecoder, vit_nlc.py:488-551, 696-748) --------
 * Latency-bound sizes (648 tokens x 360 channels): csrc/hyper.hip.  Both are deterministic (fixed
 * reduction order) - h_s runs on the encode and on the decode side and must agree bit for bit. */

/* cra5_gemm_nt_split for small M: one wave per 32 x 32..128 tile, operands straight from L2, optional
 * in-block split-K.  Same arguments; C_split pad columns (N .. ldc_split_kp) are written as zeros.
 * ps_Hz > 0 selects the fused un-embed store of HyperpriorDecoder (vit_nlc.py:672-679,
 * `b h w (p1 p2 c) -> b c (h p1) (w p2)`): M = ps_Hz * ps_Wz tokens, the N = Cout * ps_p1 * ps_p2 weight
 * rows must be in (c, p1, p2) order (ps_p2 must be 4), and C is the image [Cout][ps_Hz*ps_p1][ps_Wz*4]. */
int cra5_small_gemm_nt_split(const uint16_t *A, int lda_kp, const uint16_t *W, int ldw_kp, float *C, int ldc,
                             uint16_t *C_split, int ldc_split_kp, const float *bias, const float *res, int ldr,
                             int M, int N, int Kp, float wscale_inv, int flags, int ps_Hz, int ps_Wz, int ps_p1,
                             int ps_p2, void *stream);

/* Attention.forward (vit_nlc.py:94-112) over all n_tok tokens, exact fp32 MFMA, head dim 72 | 64:
 * qkv fp32 [n_tok][3C] -> out fp32 [n_tok][C] and / or out_split (pad columns must already be zero). */
int cra5_hyper_attention_f32(const float *qkv, float *out, uint16_t *out_split, int split_kp, int n_tok, int C,
                             int heads, float scale, void *stream);

/* Device-side timing helpers for bench.py (HIP events on the launch stream). */
int cra5_event_create(void **ev);
int cra5_event_record(void *ev, void *stream);
int cra5_event_elapsed_ms(void *start, void *stop, float *ms);
int cra5_event_destroy(void *ev);

/* Host <-> device frame copies through a caller-owned PINNED staging buffer of >= `bytes` (csrc/runtime.hip): the copy
 * is cut into `chunk_bytes` chunks; `n_threads` host threads (the caller is one of them) memcpy chunk c + 1 between
 * pageable and pinned memory while the DMA engine moves chunk c on `stream`.  Replaces the `.to(device)` / `.cpu()` of
 * a 1.11 GB frame in cra5_api.py:81-125,153-192.  h2d: returns once the DMA engine has read the last chunk out
 * of `pinned` (the staging buffer and `dst_dev` are the caller's again: the next frame may re-use both); the team is
 * capped at the CPUs the process may run on and its wait loops yield; d2h: returns when `dst_host` holds
 * all bytes (the copies are queued behind whatever `stream` already holds). */
int cra5_copy_h2d_staged(void *dst_dev, const void *src_host, void *pinned, size_t bytes, size_t chunk_bytes,
                         int n_threads, void *stream);
int cra5_copy_d2h_staged(void *dst_host, const void *src_dev, void *pinned, size_t bytes, size_t chunk_bytes,
                         int n_threads, void *stream);

/* Shader-clock telemetry for bench.py (csrc/runtime.hip).  cra5_clock_probe: ONE wave that stays for `window_ticks`
 * of the 100 MHz wall clock (<= 10 ms) and stores {wall0, cycles0, wall1, cycles1} into slot4_dev[0..3]: effective
 * shader clock of the window = (cycles1 - cycles0) / (wall1 - wall0) x 100 MHz, on the CU the wave landed on, beside
 * whatever else runs.  Short probes on purpose: a resident sampler wave would block every stream that shares its
 * hardware queue.  cra5_clock_stamp writes the wall clock into one device word in stream order (brackets queued work). */
int cra5_clock_probe(uint64_t *slot4_dev, int window_ticks, void *stream);
int cra5_clock_stamp(uint64_t *slot_dev, void *stream);

/* Range audit of the split-f16 producers (csrc/split.h): out[0] = elements with |x| >= 65504 (clipped
 * by the saturating split), out[1] = non-finite elements, counted since the last reset by every
 * LayerNorm / GEMM-epilogue / attention / patch-gather store.  Only in the `rangecheck` build flavour
 * (python -m cra5_amd.build --flavour rangecheck, -DCRA5_RANGE_CHECK); CRA5_ERR_UNAVAILABLE otherwise.
 * Synchronises the device. */
int cra5_debug_range_counts(uint64_t *out2, int reset);

#ifdef __cplusplus
}
#endif
#endif /* CRA5_AMD_H */
