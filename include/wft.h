/*
 * wft.h — C ABI of libwft.so, the MI355X (gfx950) kernel library behind the
 * whisper_finetune training hot path.
 *
 * The reference (i4Ds/whisper-finetune) has no FFI of its own: its hot path is
 * Python calling PyTorch / openai-whisper / torchaudio ops.  Each entry point
 * below names the reference call site (path relative to the reference root,
 * file:line) whose arithmetic it replaces.  The Python host side
 * (whisper-finetune_amd/whisper_finetune/engine/lib.py) binds these with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    the name ends in _host; the caller (PyTorch's allocator) owns every buffer
 *    including workspaces;
 *  - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*):
 *    no host sync, no allocation, no default-stream use, no device state and no
 *    mutable host state kept in the library — re-entrant across streams and
 *    threads.  Everything that selects a launch mode or a kernel variant is a
 *    FIELD of the call's argument struct (wft_gemm_args / wft_attn_args:
 *    launch_mode, variant, q_prescaled); the only process-wide inputs are read
 *    ONCE when the library is loaded: WFT_NT256_PERSISTENT / WFT_ATTN_PERSISTENT
 *    (=0: one workgroup per tile everywhere) and, in libwft_timing.so only, the
 *    developer switches of DESIGN.md §3;
 *  - return value: WFT_OK (0) or a negative wft_status; wft_last_error() gives
 *    a thread-local message for the last failure on the calling thread;
 *  - matrices are row-major; `ld*` are leading dimensions in ELEMENTS;
 *  - "bf16" buffers hold IEEE bfloat16 (uint16_t storage), "f32" IEEE float;
 *  - RNG-dependent ops take ALREADY-DRAWN parameters so the host keeps the
 *    reference's CPU-generator draw order (SURVEY.md §7 "RNG parity").
 */
#ifndef WFT_H
#define WFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  WFT_OK = 0,
  WFT_ERR_ARG = -1,     /* bad shape / alignment / null pointer            */
  WFT_ERR_LAUNCH = -2,  /* hipLaunchKernel failed (message has the reason) */
  WFT_ERR_UNSUPPORTED = -3
} wft_status;

typedef uint16_t wft_bf16;

const char* wft_last_error(void);
/* library version + compiled arch string, e.g. "wft 0.1 gfx950" */
const char* wft_version(void);

/* ------------------------------------------------------------------ casts */
/* fp32 master weight -> bf16 shadow (what `W.to(x.dtype)` does on every
 * whisper.model.Linear.forward under autocast).        */
int wft_cast_f32_bf16(const float* src, wft_bf16* dst, int64_t n, void* stream);
int wft_cast_bf16_f32(const wft_bf16* src, float* dst, int64_t n, void* stream);
/* src f32 [rows, cols] -> dst bf16 [rows_pad, cols_pad] (zero padded, row
 * stride ld_dst) and, if dst_t != NULL, dst_t bf16 [cols_pad, rows_pad] (row
 * stride ld_dst_t: the transposed shadow the backward-data GEMM consumes).
 * The strides let several weights (q/k/v) share one concatenated shadow.
 * fwd_scale (0 is read as 1): dst = bf16(fwd_scale * src) — one rounding of the
 * scaled value — while dst_t stays bf16(src): the softmax scale * log2(e) of a
 * self-attention q projection folded into its FORWARD shadow
 * (wft_attn_args.q_prescaled; whisper's `q * scale`, App. A.1).               */
int wft_cast_pad_transpose_f32_bf16(const float* src, int64_t rows, int64_t cols,
                                    wft_bf16* dst, wft_bf16* dst_t,
                                    int64_t rows_pad, int64_t cols_pad,
                                    int64_t ld_dst, int64_t ld_dst_t, float fwd_scale, void* stream);
/* W_eff = W + scaling * B @ (A * mask): the weight minLoRA's parametrization produces for every adapted Linear
 * (reference call sites model/lora.py:30-71 apply, :83-89 merge).  W f32 [rows, cols], B f32
 * [rows, rank], A f32 [rank, cols], mask f32 [cols] or NULL (the already-drawn dropout mask), rank <= 64.
 * Outputs (any subset): dst bf16 [rows_pad, cols_pad] (ld_dst) and dst_t bf16 [cols_pad, rows_pad] (ld_dst_t), zero
 * padded — the GEMM shadows of the training forward/backward; dst_f32 f32 [rows, cols] (may alias W) — merge_lora.
 * fwd_scale: as in wft_cast_pad_transpose_f32_bf16 (dst only; dst_t and dst_f32 are never scaled).                  */
int wft_lora_merge(const float* W, int64_t rows, int64_t cols, const float* B, const float* A, const float* mask,
                   int rank, float scaling, wft_bf16* dst, wft_bf16* dst_t, int64_t rows_pad, int64_t cols_pad,
                   int64_t ld_dst, int64_t ld_dst_t, float* dst_f32, float fwd_scale, void* stream);
/* Operands of the rank-r adapter-gradient GEMMs (du = dy (sB), u = x (s A*mask)^T; minLoRA parametrization, model/lora.py:30-71)
 * of ONE adapter, written into its Linear group's zero-initialised padded bf16 buffers: Am [rpad, K] rows ro..ro+rank (and
 * AmT [K, rpad]) = scaling * A * mask; Bb [npad, rpad] block (no..no+n, ro..ro+rank) (and BbT [rpad, npad]) = scaling * B.
 * A f32 [rank, K], B f32 [n, rank], mask f32 [K] or NULL.                                                                */
int wft_lora_pack(const float* A, const float* mask, const float* B, int rank, int64_t K, int64_t n, float scaling,
                  wft_bf16* Am, wft_bf16* AmT, wft_bf16* Bb, wft_bf16* BbT, int64_t rpad, int64_t npad, int64_t ro,
                  int64_t no, void* stream);
/* wft_lora_merge (dst + dst_t) and wft_lora_pack of EVERY adapter of a model in one launch — issued once per training forward,
 * right after the dropout masks are drawn, instead of two launches per Linear (2 x 512 for large-v3).  tab: device array of n
 * rows x 20 int64:
 *   0 W, 1 rows, 2 cols, 3 B, 4 A, 5 mask (or 0), 6 rank, 7 scaling (the float's bits in bits 0..31; bits 32..63: fwd_scale as float bits, 0 = 1 —
 *   dst = bf16(fwd_scale * w), dst_t unscaled, as in wft_cast_pad_transpose_f32_bf16), 8 dst, 9 dst_t (or 0), 10 ld_dst,
 *   11 ld_dst_t, 12 Am, 13 AmT, 14 Bb, 15 BbT (12-15 all 0: no pack), 16 rpad, 17 npad, 18 ro, 19 no
 * with the meanings of the two per-adapter entry points; rows % 64 == 0, cols % 64 == 0, rank <= 64, W 16-byte and dst / dst_t
 * 8-byte aligned, ld_dst % 4 == 0, ld_dst_t % 4 == 0 (the caller checks: a model that does not fit keeps the per-adapter calls).
 * tile_start: device int32 [n + 1], prefix sums of (rows / 64) * (cols / 64); total_tiles = tile_start[n].  Values are
 * bit-identical to the per-adapter entry points. */
int wft_lora_refresh_mt(const void* tab, const int32_t* tile_start, int n, int total_tiles, void* stream);
/* n small f32 vector copies in one launch.  tab: DEVICE int64 [n][3] = source address, destination address, element count (bits 0..31;
 * bits 32..63: a scale as float bits, 0 = plain copy — the q slice of a fused q/k/v bias under wft_attn_args.q_prescaled)
 * (disjoint ranges).  The host mirror uses it to restack the bias vectors of every fused q/k/v group after an optimizer step
 * (whisper.model.Linear biases: the GEMM epilogue reads ONE bias vector per fused group). */
int wft_mt_copy_f32(const void* tab, int n, void* stream);
/* Per-row (output channel) symmetric int8 image of a bf16 shadow, the weight operand of wft_gemm_nt_stream_q8.  W bf16 [rows, cols]
 * (ldw), Q int8 [rows, cols] (ldq), scale f32 [rows].  Per row, in f32, every operation correctly rounded and none fused:
 *   amax  = max_k |w[k]|
 *   scale = amax / 127.0f
 *   inv   = amax > 0 ? 127.0f / amax : 0.0f
 *   q[k]  = clamp(rintf(w[k] * inv), -127, 127)        (rintf: round half to even)
 * so a numpy float32 restatement gives the same bytes (tests/_q8_cases.py).  An all-zero row (the padding rows of a shadow) gives
 * scale = 0 and q = 0.  cols % 64 == 0, ldw % 8 == 0, ldq % 16 == 0, W and Q 16-byte aligned.  Runs once per shadow refresh.       */
int wft_quantize_rows_i8(const wft_bf16* W, int64_t rows, int64_t cols, int64_t ldw, int8_t* Q, int64_t ldq, float* scale,
                         void* stream);
/* y[i] = a[i] + b[i] (bf16) — gradient accumulation on the residual stream. */
int wft_add_bf16(const wft_bf16* a, const wft_bf16* b, wft_bf16* y, int64_t n, void* stream);
/* out = a*x + b*y over n bf16 elements (y may be NULL).  StochasticDepthMixin's train-time rescale
 * x + (block(x) - x)/(1-p) (model/model_utils.py:241-250) and its backward in one pass each.   */
int wft_axpby_bf16(float a, const wft_bf16* x, float b, const wft_bf16* y, wft_bf16* out, int64_t n, void* stream);
/* Stochastic depth with the skip decision in device memory (*skip, int32; a captured HIP graph reads the value its host
 * wrote before the replay).  Forward: out = *skip ? x : a*x + b*f  (a = 1 - s, b = s = 1/keep).  Backward, one pass over dy:
 * dx = *skip ? dy : a*dy  and  df = *skip ? 0 : s*dy.  Kept blocks are bit-identical to wft_axpby_bf16 (forward: (a, x, b, f);
 * backward: (a, dy) and (s, dy) without y); a skipped block is a select, not a multiply by zero.                          */
int wft_sd_select_fwd_bf16(const int32_t* skip, float a, const wft_bf16* x, float b, const wft_bf16* f, wft_bf16* out,
                           int64_t n, void* stream);
int wft_sd_select_bwd_bf16(const int32_t* skip, float a, float s, const wft_bf16* dy, wft_bf16* dx, wft_bf16* df, int64_t n,
                           void* stream);
/* out[i] = dy[i] * gelu'(pre[i]) (exact-erf GELU) — backward through F.gelu in the
 * conv stem (model/model_utils.py:276-277).                                  */
int wft_dgelu_mul_bf16(const wft_bf16* dy, const wft_bf16* pre, wft_bf16* out, int64_t n, void* stream);
/* out[c] (+)= sum_r x[r, c] — bias gradients.  x bf16 [rows, ld], out f32[cols] */
int wft_colsum_bf16(const wft_bf16* x, int64_t rows, int64_t cols, int64_t ld,
                    float* out, int accumulate, void* stream);
/* The same sums for LARGE inputs (rows >= 8 192; round 6, was 65 536) through a caller workspace of wft_colsum_workspace_bytes(rows, cols): the
 * rows are cut into 64 chunks summed by (column group, chunk) workgroups and folded in chunk order (fixed order, HBM rate;
 * the one-pass kernel above occupies cols / 32 workgroups only).  Falls back to wft_colsum_bf16 when the workspace is
 * missing or the input small.  Replaces: the bias gradient torch.autograd forms for nn.Conv1d in
 * whisper.model.AudioEncoder (src/whisper_finetune/model/model_utils.py:271-281 via loss.backward(), :63-72).        */
int64_t wft_colsum_workspace_bytes(int64_t rows, int64_t cols);
int wft_colsum_bf16_ws(const wft_bf16* x, int64_t rows, int64_t cols, int64_t ld, float* out, int accumulate,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------- LayerNorm */
/* whisper.model.LayerNorm.forward = F.layer_norm(x.float()).type(x.dtype)
 * (call sites model/model_utils.py:287,324 and every
 * ResidualAttentionBlock).  x,y bf16 [rows, cols]; gamma,beta f32[cols];
 * mean,rstd f32[rows] are saved for the backward.  cols % 8 == 0, <= 2048.
 * Optional deep-SpecAugment masks (model/model_utils.py:409-417): if
 * rows_per_batch > 0, rows t in [t0,t1) of every batch item and columns in
 * [c0,c1) are zero-filled in y (time mask then "frequency"=channel mask).   */
int wft_layernorm_fwd(const wft_bf16* x, const float* gamma, const float* beta,
                      wft_bf16* y, float* mean, float* rstd,
                      int64_t rows, int cols, float eps,
                      int rows_per_batch, int t0, int t1, int c0, int c1,
                      void* stream);
/* The same with the deep-SpecAugment span read from device memory: span = int32[4] {t0, t1, c0, c1}, rows_per_batch > 0.
 * An empty span (t0 == t1 and c0 == c1) gives the bits of the unmasked call.  (A captured HIP graph: the host writes the
 * span before each replay.)                                                                                        */
int wft_layernorm_fwd_dspan(const wft_bf16* x, const float* gamma, const float* beta,
                            wft_bf16* y, float* mean, float* rstd,
                            int64_t rows, int cols, float eps,
                            int rows_per_batch, const int32_t* span, void* stream);
/* dx = LN'(dy) (+ dres if dres != NULL); dgamma/dbeta are WRITTEN (=; no zero-fill needed) or both NULL (frozen LayerNorm
 * parameters: with dx_colsum NULL as well — a LoRA run — the partial sums and the two reduce launches are skipped and
 * `partial` may be NULL).
 * partial: f32 workspace of wft_layernorm_bwd_workspace(rows, cols) bytes.
 * The same mask arguments zero the masked positions of dy first.
 * dx_colsum (f32 [cols] or NULL): column sums of the bf16 dx just written — dx is the gradient of the residual
 * stream, i.e. dy of the Linear (out / mlp.2) whose output was added to it, so this IS that Linear's bias
 * gradient and saves a separate pass over [rows, cols].                                          */
int64_t wft_layernorm_bwd_workspace(int64_t rows, int cols);
int wft_layernorm_bwd(const wft_bf16* dy, const wft_bf16* x, const float* gamma,
                      const float* mean, const float* rstd, const wft_bf16* dres,
                      wft_bf16* dx, float* dgamma, float* dbeta, float* dx_colsum, void* partial,
                      int64_t rows, int cols,
                      int rows_per_batch, int t0, int t1, int c0, int c1,
                      void* stream);
/* wft_layernorm_bwd with the span read from device memory (see wft_layernorm_fwd_dspan). */
int wft_layernorm_bwd_dspan(const wft_bf16* dy, const wft_bf16* x, const float* gamma,
                            const float* mean, const float* rstd, const wft_bf16* dres,
                            wft_bf16* dx, float* dgamma, float* dbeta, float* dx_colsum, void* partial,
                            int64_t rows, int cols,
                            int rows_per_batch, const int32_t* span, void* stream);

/* ------------------------------------------------------------------- GEMM */
/* Epilogue selector for wft_gemm_nt_bf16. */
enum {
  WFT_EPI_NONE = 0,
  WFT_EPI_GELU = 1,   /* C = gelu_erf(acc + bias); if aux != NULL also store pre-activation there */
  WFT_EPI_DGELU = 2,  /* C = acc * gelu'(aux)  (backward through GELU; aux = saved pre-activation) */
  /* The training pair of the MLP (mlp.0 -> GELU -> mlp.2): the forward GEMM stores gelu'(pre) instead of pre — same
   * bytes — and the backward-data GEMM multiplies by it, so the derivative's exp/rcp/polynomial (about 30 % of a
   * K = 1280 tile's time when done in the backward epilogue) is computed once, beside gelu() itself.  bf16 C only. */
  WFT_EPI_GELU_GRAD = 3, /* C = gelu_erf(acc + bias); aux (required) <- gelu'(acc + bias) */
  WFT_EPI_MUL_AUX = 4,   /* C = acc * aux */
  /* The same pair with gelu' stored in ONE BYTE per element (round 6): code = round(200 gelu') + 26, a 1/200 grid on which
   * gelu' = 0 and gelu' = 1 are exact, range [-0.13, 1.145] (gelu' lies in [-0.129, 1.129]), |error| <= 0.0025 — about the bf16
   * half-ulp near 1.  `aux` is then NOT an [M, N] matrix but an opaque buffer of wft_gemm_nt_aux8_bytes(args) bytes in the
   * FRAGMENT order of gemm_nt4w_kernel (16 KiB per 256x256 tile and wave; lda / strides of aux are ignored): the writer (mlp.0's
   * forward GEMM) and the reader (mlp.2's backward-data GEMM) have the same M and N, hence the same tiles.  Only the
   * one-wave-per-SIMD kernel carries them: ask wft_gemm_nt_aux8_bytes (0 = not served: use the bf16 pair).  batch 1, alpha 1.
   * Halves the bytes of the pair's second tensor on the store / load path that prices these epilogues, and saves one byte per
   * MLP activation element of saved-for-backward memory (21 GiB at 87 clips of large-v3).  Reference: `F.gelu` in
   * whisper.model.ResidualAttentionBlock.mlp (keys mlp.0 / mlp.2, scripts/convert_openai_to_hf.py:91-92).                     */
  WFT_EPI_GELU_GRAD8 = 5, /* C = gelu_erf(acc + bias); aux <- codes of gelu'(acc + bias) */
  WFT_EPI_MUL_AUX8 = 6    /* C = acc * decode(aux) */
};
/* C[b][m, n] = alpha * sum_k A[b][m, k] * B[b][n, k]  (+ bias[n]) (epilogue)
 *              (+ residual[b][m, n]);  bf16 inputs, fp32 MFMA accumulation.
 * Replaces whisper.model.Linear / Conv1d / the tied logits matmul
 * (model/model_utils.py:276-277,325).
 *  A: bf16, row m at A + b*strideA + m*lda, K contiguous (lda may be < K:
 *     overlapping rows = im2col-free conv1d windows);
 *  B: bf16 [N, K] K contiguous (a Linear weight as stored, or a transposed
 *     shadow for backward-data);  C: bf16 or f32 (c_is_f32), ldc;
 *  accumulate: C += result (only with c_is_f32);
 *  valid_rows_period/valid_rows: if period > 0, rows with (m % period) >=
 *     valid_rows are written as zero (keeps conv pad rows zero);
 *  K % 64 == 0, N % 128 == 0, M >= 1; all base pointers 16-byte aligned,
 *  lda/ldb % 8 == 0.                                                         */
typedef struct {
  const wft_bf16* A; int64_t lda; int64_t strideA;
  const wft_bf16* B; int64_t ldb; int64_t strideB;
  void* C; int64_t ldc; int64_t strideC; int c_is_f32; int accumulate;
  const float* bias;                    /* f32 [N] or NULL                    */
  const wft_bf16* residual; int64_t ldr; int64_t strideR;  /* or NULL         */
  wft_bf16* aux; int64_t ldaux; int64_t strideAux;         /* see epilogues    */
  int epilogue; float alpha;
  int64_t M; int64_t N; int64_t K; int batch;
  int valid_rows_period; int valid_rows;
  int residual_first;  /* != 0: add the residual BEFORE the epilogue op (gelu / dgelu) instead of after */
  /* wft_gemm_tn_bf16 only: optional caller-owned scratch for split-K partial tiles.  With at least
   * wft_gemm_tn_workspace_bytes(args) bytes the partials are written with plain stores and summed in a
   * fixed order by a second kernel (bitwise reproducible); with NULL / too small they are added to C
   * with fp32 atomics (order-dependent in the last bits).                                            */
  void* workspace; int64_t workspace_bytes;
  /* wft_gemm_nt_bf16 only: scale of the residual term, C = alpha*acc (+bias)(epilogue) + beta*residual.
   * 0 is read as 1 so that zero-initialised structs keep the plain residual add.  (Newton-Schulz steps of the
   * Muon optimizer: B = b*A + c*A@A, X' = a*X + B@X — muon.py zeropower_via_newtonschulz5.)            */
  float beta;
  /* wft_gemm_tn_bf16 only (P = 128, f32 C): if 0 < p_valid <= 64, columns >= p_valid of A are known to be zero (a rank-r LoRA
   * operand in its 128-wide padded buffer).  Selects the load-stream kernel for rank-r operands: only the first
   * 16*ceil(p_valid/16) columns of A are read, the split-K workspace holds only those rows (wft_gemm_tn_workspace_bytes
   * accounts for it), rows >= 16*ceil(p_valid/16) of C are written as zero (left alone when accumulating).  Results are
   * bit-identical to p_valid = 0.
   * wft_gemm_nt_bf16 (N = 128, bf16 C, batch 1, no bias / residual / epilogue): rows >= p_valid of B are zero padding (the
   * other two adapter products, u = x (sA*mask)^T and du = dy (sB)): only rows < 16*ceil(p_valid/16) of B are read and ONLY
   * those columns of C are written — the rest of the 128-wide buffer is left as it was (its consumer is the call above with the
   * same p_valid); bit-identical to p_valid = 0 in the written columns. */
  int p_valid;
  /* wft_gemm_nt_bf16 only: if != NULL (bf16 C, batch == 1), colsum[n] = sum over rows of the C just written — the bias
   * gradient of the Linear that consumes C as its dy (C = d(pre-activation) from the DGELU epilogue).  With `workspace`
   * of wft_gemm_nt_colsum_workspace_bytes(args) bytes the sums are formed in the epilogue of the 256x256 kernel (no
   * second pass over C); otherwise the library runs wft_colsum_bf16 over C after the GEMM.                      */
  float* colsum;
  /* wft_gemm_tn_bf16 with p_valid > 0 only (the two LoRA adapter gradients; both need the workspace, whose size
   * wft_gemm_tn_workspace_bytes reports with these fields set).  Applied by the kernel that sums the split-K partials, so the
   * adapter gradients leave the library in the layout autograd hands to the optimizer — no element-wise pass after the GEMM:
   *  tn_col_scale: f32 [S][Q] or NULL; C[p][q] *= tn_col_scale[p / tn_scale_rows][q] (tn_scale_rows = 0: S = 1, one row for
   *    all p).  dA = (du^T x) * mask, the dropout mask of each adapter of the group (model/lora.py via minLoRA's
   *    dropout-on-A).  In this form C is a [p_valid][ldc] matrix: rows >= p_valid are NOT written (the
   *    adapter gradients keep no 128-row buffer alive);
   *  tn_block_n > 0: C is NOT a [128][ldc] matrix but Q / tn_block_n contiguous blocks [tn_block_n][tn_block_r], block b
   *    holding the TRANSPOSE of rows b*tn_block_r .. +tn_block_r, columns b*tn_block_n .. +tn_block_n of the product (the
   *    off-diagonal blocks are not stored): dB of adapter b of a group of equally shaped Linears, as [out, r] row-major. */
  const float* tn_col_scale; int tn_scale_rows;
  int tn_block_n; int tn_block_r;
  /* wft_gemm_tn_bf16 on its 256x256 paths (ask wft_gemm_tn_segments_ok): tn_seg_count in 1..4 row ranges of the product go to
   * SEPARATE contiguous f32 [rows_i][Q] destinations instead of C — tn_seg_ptr[i] receives rows [tn_seg_end[i-1], tn_seg_end[i])
   * (tn_seg_end[count-1] = P) — with `accumulate` read-modify-write like C.  One weight-gradient GEMM of a fused Linear group
   * (q, k, v share one [3d, d] product) then writes each parameter's gradient where it lives: the `gradient_as_bucket_view` slices
   * of torch DDP's buckets (reference: scripts/finetune.py:698-705), no copy between the last dW GEMM and the bucket's all-reduce.
   * Always through the workspace (wft_gemm_tn_workspace_bytes with these fields set), summed by the reduce kernel in the same
   * fixed order as the unsegmented call: bit-identical values.  C must still be a valid pointer (it is not written).           */
  int tn_seg_count; int tn_seg_end[4]; float* tn_seg_ptr[4];
  /* Per-call launch state (zero = defaults; nothing is kept in the library):
   *  launch_mode: 0 = persistent grids for the 256x256 NT kernels (one workgroup per CU walks the tiles), 1 = one workgroup per tile
   *    (the backward pass beside RCCL's collective kernels: runtime.exchange_launch_mode; scripts/finetune.py:694-710).
   *  variant: != 0 forces the 8-wave ping-pong kernels (gemm_nt256_kernel / gemm_tn256_kernel) where the one-wave-per-SIMD kernels
   *    would apply (bit-identity tests, A/B runs; NT: same k order, bit-identical C).                                            */
  int launch_mode; int variant;
} wft_gemm_args;
int wft_gemm_nt_bf16(const wft_gemm_args* args, void* stream);
/* The queries below and wft_gemm_nt_bf16 itself read ONE plan of the call (csrc/gemm.hip nt_plan, over the rules kept beside
 * each kernel in csrc/gemm_*.hip: kernel, grid, K splits, workspace), so a query answers what the launcher will do with the same arguments; wft_gemm_tn_* likewise (tn_plan).  All pure
 * host functions: no device call, nothing launched.
 * Which kernel wft_gemm_nt_bf16 dispatches these arguments to: 4 (gemm_nt4w_kernel: 256x256 tiles, four waves with 128x128
 * accumulators each), 256 (gemm_nt256_kernel, the 8-wave ping-pong 256x256 kernel) or 128 (gemm_nt_kernel and its rank-r form;
 * used by bench.py to attribute HIP-event timings to the kernel names rocprofv3 reports).        */
int wft_gemm_nt_variant(const wft_gemm_args* args);
/* 1 if wft_gemm_tn_bf16 takes these arguments' tn_seg_* fields (the plan puts the call on a 256x256 kernel, and the segment
 * list is well formed), 0 if the caller has to use C and copy.                                                              */
int wft_gemm_tn_segments_ok(const wft_gemm_args* args);
/* Bytes of `workspace` with which the plan forms `colsum` in the GEMM's epilogue (wft_gemm_args.colsum above); 0: it runs
 * wft_colsum_bf16 over C after the GEMM whatever is granted.                                                                */
int64_t wft_gemm_nt_colsum_workspace_bytes(const wft_gemm_args* args);
/* Split-K form of the 128-tile kernel (round 6): bytes of fp32 partial tiles [nsplit][M][N] if a PLAIN bf16 product (batch 1, no bias /
 * residual / epilogue / colsum) has so few output tiles and so deep a K that the library would split K over the idle CUs when given
 * `workspace` of at least this size (the tied-embedding backward-data product of a short decoder batch, dX[B*S, d] = dlogits[B*S, V] E[V, d],
 * whisper.model.TextDecoder.forward's logits matmul reached from model_utils.py:83-84: 1 024 x 512 x 51 968 runs on 32 of 256 CUs
 * unsplit).  0: the plan does not split the call.  Partials are summed in split order: bitwise reproducible.                    */
int64_t wft_gemm_nt_splitk_workspace_bytes(const wft_gemm_args* args);
/* Size of the one-byte gelu' buffer of WFT_EPI_GELU_GRAD8 / WFT_EPI_MUL_AUX8 for these arguments, or 0 if the call would not be
 * served in that form (the plan does not put it on gemm_nt4w_kernel; MUL_AUX8 takes no bias): wft_gemm_nt_bf16 then refuses
 * it with WFT_ERR_UNSUPPORTED before any device call.                                                                       */
int64_t wft_gemm_nt_aux8_bytes(const wft_gemm_args* args);
/* Weight-streaming form of the same product for the projections of a KV-cached decoding step (csrc/gemm_stream.hip; whisper.decoding's
 * per-token decoder forward, M = batch): K is split over the whole chip as a function of (N, K) and the CU count only — never of M, so row m
 * of C does not depend on the batch it sat in —, every weight byte is read once straight into registers, fp32 partials go to `workspace`
 * [split][M][N] and a second launch sums them in split order and applies the epilogue (bitwise reproducible, no atomics).
 * Served (wft_gemm_nt_stream_ok = 1): 1 <= M <= 32, batch 1, bf16 C, alpha 1, the plain epilogue or the gelu one of the enum above
 * (aux NULL or the pre-activation), optional f32 bias, optional bf16 residual added AFTER the epilogue (residual_first 0, beta 1),
 * N % 128 == 0, K % 64 == 0, the alignment rules of wft_gemm_nt_bf16 (bias 16-byte, residual / aux 8-byte aligned, ldr / ldaux % 4 == 0).
 * Everything else — an f32 or accumulated C, batch > 1, colsum, p_valid, valid_rows_period, the other epilogues, larger M — is refused
 * with WFT_ERR_UNSUPPORTED before any device call; wft_gemm_nt_bf16 takes those calls.  `workspace` must hold
 * wft_gemm_nt_stream_workspace_bytes(args) bytes (0 = not served), 16-byte aligned.  Both queries are pure host functions.       */
int wft_gemm_nt_stream_bf16(const wft_gemm_args* args, void* stream);
int wft_gemm_nt_stream_ok(const wft_gemm_args* args);
int64_t wft_gemm_nt_stream_workspace_bytes(const wft_gemm_args* args);
/* Weight-only int8 twin of wft_gemm_nt_stream_bf16 for the same cached steps (CTranslate2's int8 deployment of a fine-tuned checkpoint is
 * what it stands next to; activations stay bf16 here):
 *   C[m][n] = bf16( epi( b_scale[n] * sum_k A[m][k] * Q[n][k] + bias[n] ) + residual[m][n] )
 * args->B points at int8, row-major [N, K], ldb in elements with ldb % 16 == 0, 16-byte aligned; b_scale f32 [N], 16-byte aligned (what
 * wft_quantize_rows_i8 writes).  Everything else is wft_gemm_nt_stream_bf16's rule, plan (the same split of K: a function of N, K and the
 * CU count) and workspace layout.  Definition, closed form: every Q[n][k] is converted to bf16 exactly and the products are accumulated
 * by the same MFMAs in the same order as wft_gemm_nt_stream_bf16 on Q.to(bf16); the slices are summed in slice order; ONE correctly
 * rounded f32 multiply by b_scale[n] (never fused with the bias add); then bias, gelu (aux = the pre-activation), residual, one bf16
 * rounding.  With b_scale = 1, or any power of two folded into the bf16 weights instead, the result equals wft_gemm_nt_stream_bf16's bit
 * for bit.  Refusals: WFT_ERR_UNSUPPORTED before any device call; wft_gemm_nt_stream_bf16 on the bf16 shadow takes those calls.       */
int wft_gemm_nt_stream_q8(const wft_gemm_args* args, const float* b_scale, void* stream);
int wft_gemm_nt_stream_q8_ok(const wft_gemm_args* args);
int64_t wft_gemm_nt_stream_q8_workspace_bytes(const wft_gemm_args* args);
/* W8A8 product on the int8 matrix cores (csrc/gemm_i8.hip; v_mfma_i32_16x16x64_i8) for the products of decoding's weights="w8a8" mode
 * with M > 32 — the encoder, the prefill, the cross key / value projections; CTranslate2's int8 deployment quantises every Linear and its
 * activations per row, which is what this stands next to.  args->A is int8 [M, K] row-major (lda), args->B int8 [N, K] row-major (ldb),
 * a_scale f32 [M], b_scale f32 [N] — what wft_quantize_rows_i8 writes for an activation matrix and for a weight shadow —, C bf16 [M, N].
 * Definition, closed form; every f32 operation correctly rounded and none fused:
 *   acc  = sum_k (int32)A[m][k] * (int32)B[n][k]          exact, order-free
 *   f    = (float)acc                                      round to nearest even (matters above 2^24)
 *   s    = a_scale[m] * b_scale[n]
 *   v    = f * s
 *   v    = v + bias[n]                                     if bias
 *   v    = gelu(v)                                         if WFT_EPI_GELU (the formula of the bf16 kernels' epilogue)
 *   v    = v + (float)residual[m][n]                       if residual (residual_first 0, beta 1)
 *   C    = bf16(v)                                         one rounding
 * One launch, no workspace, no split of K, no atomics; bitwise reproducible; row m of C does not depend on M.
 * Served (wft_gemm_nt_i8_ok = 1, a pure host function): any M >= 1 (rows past M of the last row tile are neither read into a result nor
 * written), N % 128 == 0, K % 64 == 0 and K <= 65536 (|acc| < 2^31 even for -128 bytes), batch 1, bf16 C, alpha 1, the plain or the gelu
 * epilogue with aux NULL, optional f32 bias, optional bf16 residual added after the epilogue; lda % 16 == 0, ldb % 16 == 0, ldc % 4 == 0,
 * A / B / C 16-byte aligned, the bias / residual alignment rules of wft_gemm_nt_stream_bf16.  Everything else — an f32 or accumulated C,
 * batch > 1, colsum, p_valid, valid_rows_period, the other epilogues, aux — is refused with WFT_ERR_UNSUPPORTED and the reason in
 * wft_last_error() before any device call.  A NULL or not 16-byte aligned scale vector is WFT_ERR_ARG.
 * What still reads bf16 under weights="w8a8": the cached steps' activations (their weights are int8: wft_gemm_nt_stream_q8), products with
 * M <= 32, the conv stem, the embedding lookup, the prefill's tied logits product, attention (DESIGN.md §3 "W8A8").                    */
int wft_gemm_nt_i8(const wft_gemm_args* args, const float* a_scale, const float* b_scale, void* stream);
int wft_gemm_nt_i8_ok(const wft_gemm_args* args);
/* C[p, q] (+)= alpha * sum_r A[r, p] * B[r, q]   (weight gradients dW = dY^T X:
 * what autograd's mm-backward computes for whisper.model.Linear).
 *  A bf16 [R, P] (row r at A + r*lda, P contiguous), B bf16 [R, Q];
 *  C f32 or bf16 [P, Q].  P % 128 == 0, Q % 128 == 0, any R >= 1.
 *  Uses the same wft_gemm_args: M:=P, N:=Q, K:=R; bias/residual/aux ignored.
 *  batch > 1 sums over the batch as extra reduction (conv weight grads).     */
int wft_gemm_tn_bf16(const wft_gemm_args* args, void* stream);
/* Which kernel wft_gemm_tn_bf16 dispatches these arguments to: 4 (gemm_tn4w_kernel, one wave per SIMD), 256 (gemm_tn256_kernel, the
 * 8-wave ping-pong 256x256 kernel) or 128 (the 128-tile kernel and its rank-r form).  Read from the launcher's plan, workspace
 * fields included (a split-K plan without its workspace runs on the 8-wave kernel); tests assert the dispatch.               */
int wft_gemm_tn_variant(const wft_gemm_args* args);
/* Two independent rank-r products (p_valid > 0) in ONE launch of the load-stream kernels — the backward of an adapted Linear
 * group in the reference's parametrization (src/whisper_finetune/model/lora.py:30-71 via minLoRA; loss.backward() at
 * model/model_utils.py:63-72) needs {u = x (sA*m)^T, du = dy (sB)} and then {dA = du^T x, dB^T = u^T dy}: each pair is one call.
 * Same arguments, same results (bit for bit) as two calls of wft_gemm_nt_bf16 / wft_gemm_tn_bf16, which is also the fallback
 * for anything the load-stream kernels do not take.  The TN pair needs a separate workspace per product
 * (wft_gemm_tn_workspace_bytes each); its two split-K reduces (column scale / block layout included) are one launch too.   */
int wft_gemm_nt_rank_pair_bf16(const wft_gemm_args* args0, const wft_gemm_args* args1, void* stream);
int wft_gemm_tn_rank_pair_bf16(const wft_gemm_args* args0, const wft_gemm_args* args1, void* stream);
/* Bytes of `workspace` the plan of wft_gemm_tn_bf16 wants for these arguments (split-K partial tiles; 0: none).              */
int64_t wft_gemm_tn_workspace_bytes(const wft_gemm_args* args);

/* -------------------------------------------------------------- Attention */
/* whisper.model.MultiHeadAttention.qkv_attention:
 * softmax(q k^T / sqrt(64) [+ causal mask]) v, head_dim fixed to 64.
 * q: bf16, element (b, t, h, d) at q + b*q_bs + t*ldq + h*64 + d (so a fused
 * [B*T, 3*d_model] QKV buffer is consumed in place); same for k, v, o, do,
 * dq, dk, dv.  lse f32 [B, H, Tq] = log-sum-exp of the scaled scores (saved
 * for backward).  causal != 0: key j visible to query i iff j <= i.          */
typedef struct {
  const wft_bf16* q; int64_t ldq; int64_t q_bs;
  const wft_bf16* k; int64_t ldk; int64_t k_bs;
  const wft_bf16* v; int64_t ldv; int64_t v_bs;
  wft_bf16* o; int64_t ldo; int64_t o_bs;
  float* lse;
  int B; int H; int Tq; int Tk; int causal; float scale;
  /* backward only */
  const wft_bf16* d_o; int64_t lddo; int64_t do_bs;
  float* delta;                 /* f32 workspace [2, B, H, Tq] (kernel-internal contents: -rowsum(dO*O), then -lse/scale) */
  wft_bf16* dq; int64_t lddq; int64_t dq_bs;
  wft_bf16* dk; int64_t lddk; int64_t dk_bs;
  wft_bf16* dv; int64_t lddv; int64_t dv_bs;
  /* optional (backward): bias gradients of the q and v projections formed in the kernels' epilogues instead of a
   * second pass over dq / dv.  dq_colsum / dv_colsum: f32 [H*64] outputs (sum over batch and time of the bf16 values
   * written); colsum_ws: f32 scratch of wft_attn_bwd_colsum_workspace_bytes(args) bytes.  All three or none.      */
  float* dq_colsum; float* dv_colsum; float* colsum_ws;
  /* Per-call launch state (zero-initialised structs get the defaults; nothing here is kept in the library):
   *  launch_mode: 0 = the kernel's default grid (the dK/dV kernel: persistent, one workgroup per CU), 1 = one work item per workgroup
   *    (the backward pass that runs beside RCCL's collective kernels in a multi-process job: runtime.exchange_launch_mode; the
   *    reference's DDP wrap, scripts/finetune.py:694-710).  Same results either way.
   *  variant: bit 0 forward on attn_fwd_kernel, bit 1 dQ on the 8-wave kernel, bit 2 dK/dV on the 8-wave kernel even where the
   *    pipelined / one-wave-per-SIMD kernels apply (bit-identity tests, A/B runs).
   *  q_prescaled != 0: q (forward and backward) already holds (x Wq^T + bq) * scale * log2(e) — the factor folded into the bf16
   *    forward shadow of the q projection (wft_cast_pad_transpose_f32_bf16 / wft_lora_merge `fwd_scale`), ONE bf16 rounding of the
   *    scaled value, what `q * scale` costs upstream (whisper.model.MultiHeadAttention.qkv_attention) — so no kernel multiplies the
   *    scores.  `scale` must still be the softmax scale: dq is returned w.r.t. the UNSCALED projection output (dq = scale dS K),
   *    dk = dS^T q_prescaled * ln 2, lse stays the natural-log lse of the scaled scores.                                          */
  int launch_mode; int variant; int q_prescaled;
} wft_attn_args;
int wft_attn_fwd_bf16(const wft_attn_args* args, void* stream);
int wft_attn_bwd_bf16(const wft_attn_args* args, void* stream);
int64_t wft_attn_bwd_colsum_workspace_bytes(const wft_attn_args* args);
/* Which kernel wft_attn_fwd_bf16 / wft_attn_bwd_bf16 dispatch these arguments to (pure host function, like wft_gemm_nt_variant):
 * which = 0 forward: 2 attn_fwd_pipe_kernel, 1 attn_fwd_kernel; which = 1 dQ: 4 attn_bwd_dq4w_kernel, 8 attn_bwd_dq_kernel;
 * which = 2 dK/dV: 4 attn_bwd_dkdv4w_kernel, 8 attn_bwd_dkdv_kernel.  Only the shape / stride / causal fields are read.            */
int wft_attn_variant(const wft_attn_args* args, int which);

/* -------------------------------------------------------------- Embedding */
/* TextDecoder: x = token_embedding(tokens) + positional_embedding[:S]
 * (model/model_utils.py:317-318).  tokens i64 [B*S]; emb f32 [V, d];
 * pos f32 [n_ctx, d]; out bf16 [B*S, d].                                     */
int wft_embed_fwd(const int64_t* tokens, const float* emb, const float* pos,
                  wft_bf16* out, int64_t B, int64_t S, int d, int64_t V, void* stream);
/* demb[tokens[i], :] += dout[i, :], dpos[s, :] += sum_b dout[b, s, :].  No atomics: every embedding row adds the positions
 * that hold its id in position order (i = 0, 1, ...), dpos the clips in order (b = 0, 1, ...), so the result is the same bits
 * on every run.  An id outside [0, V) (wft_embed_fwd clamps it) adds nothing to demb and still counts in dpos.                 */
int wft_embed_bwd(const int64_t* tokens, const wft_bf16* dout, float* demb, float* dpos,
                  int64_t B, int64_t S, int d, int64_t V, void* stream);

/* ---------------------------------------------------------- Cross entropy */
/* F.cross_entropy(logits.transpose(1,2), y_out, label_smoothing=eps),
 * ignore_index = -100, mean over non-ignored targets
 * (model/model_utils.py:66).  logits bf16 [rows, ld] (only the first V
 * columns are read); targets i64 [rows].
 * fwd: row_loss f32[rows] (0 for ignored rows), row_lse f32[rows],
 *      stats f32[2] = {sum of row losses, number of valid rows} (zeroed by
 *      the call, then accumulated) — loss = stats[0] / stats[1].
 * bwd: dlogits (bf16, may alias logits) = (softmax - ((1-eps) onehot + eps/V))
 *      * valid * gscale[0] / stats[1]; columns [V, ld) are written as 0.
 *      gscale: device f32[1] (the upstream grad of the mean loss).
 * argmax (optional, may be NULL): i64 [rows] = argmax over the V columns,
 *      lowest index on ties (eval/evaluator.py:70-73 teacher-forced argmax).  */
int wft_ce_fwd(const wft_bf16* logits, int64_t ld, const int64_t* targets,
               int64_t rows, int64_t V, float label_smoothing,
               float* row_loss, float* row_lse, float* stats, int64_t* argmax,
               void* stream);
int wft_ce_bwd(const wft_bf16* logits, int64_t ld, const int64_t* targets,
               int64_t rows, int64_t V, float label_smoothing,
               const float* row_lse, const float* stats, const float* gscale,
               wft_bf16* dlogits, void* stream);

/* Teacher-forced evaluation reductions (eval/evaluator.py:70-73 argmax;
 * eval/metrics.py:106-137 log_softmax / softmax / CE / entropy / max-prob) in ONE
 * pass over the logits: out4[row] = {lse, max logit, E_p[logit], target logit (0 if
 * the target is -100)}, argmax[row] = lowest index of the maximum.  targets may be
 * NULL.  nll = lse - x_t; log p(pred) = max - lse; confidence = exp(max - lse);
 * entropy = lse - E_p[logit].                                                  */
int wft_token_stats(const wft_bf16* logits, int64_t ld, const int64_t* targets,
                    int64_t rows, int64_t V, float* out4, int64_t* argmax, void* stream);

/* -------------------------------------------------------- Greedy decoding */
/* KV-cached greedy decoding (csrc/decode_attn.hip, csrc/decode_pick.hip): the single-token shapes of upstream's `whisper.decoding.GreedyDecoder` /
 * `DecodingTask._main_loop` with `DecodingOptions(without_timestamps=True)` and the `kv_cache` hooks of
 * whisper.model.MultiHeadAttention.forward (none of it is in the reference tree, whose evaluator is teacher-forced:
 * eval/evaluator.py:70-73).  Everything that changes from token to token is DEVICE state — len i32 [B] (tokens a row holds,
 * prompt included), tokens i64 [B, ld_tokens], finished i32 [B], sum_logprob f32 [B] — so no argument depends on the step.
 *
 * Single-token attention, head_dim 64: o[b, h] = softmax(q[b, h] . K[b, :n, h] * scale) V[b, :n, h], fp32 softmax.
 *  q: bf16, row b at q + b*ldq, head h at + h*64; o likewise (ldo);
 *  cache: key t of sequence b at k_cache + b*cache_bs + t*ld_cache + h*64, values at v_cache + the same offsets (one buffer
 *    of [B, Tk, 2d] rows {k | v} serves both: v_cache = k_cache + d, ld_cache = 2d);
 *  self-attention form (len != NULL): n = len[b] (clamped to 1..Tk, Tk = the cache's capacity); the step's k / v rows
 *    (k_new / v_new + b*ld_new: the k and v thirds of the fused [B, 3d] projection output) are WRITTEN to cache row len[b] - 1
 *    and take part as key len[b] - 1 — the append is fused, no other byte of the cache changes;
 *  cross-attention form (len == NULL): n = Tk for every sequence, the cache is only read;
 *  q_prescaled: as in wft_attn_args (q already carries scale * log2(e); `scale` is still required);
 *  workspace: wft_attn_decode_workspace_bytes(args) bytes (0: none needed) — when B*H alone does not fill the chip the keys
 *    are split over several workgroups whose partial (max, sum, o) are merged by a second kernel in split order.  No atomics:
 *    the same arguments give the same bits.  The split depends on B, H and Tk only.                                          */
typedef struct {
  const wft_bf16* q; int64_t ldq;
  const wft_bf16* k_new; const wft_bf16* v_new; int64_t ld_new;
  wft_bf16* k_cache; wft_bf16* v_cache; int64_t ld_cache; int64_t cache_bs;
  wft_bf16* o; int64_t ldo;
  const int32_t* len;
  int B; int H; int Tk; float scale; int q_prescaled;
  void* workspace; int64_t workspace_bytes;
} wft_attn_decode_args;
int wft_attn_decode_bf16(const wft_attn_decode_args* args, void* stream);
int64_t wft_attn_decode_workspace_bytes(const wft_attn_decode_args* args);
/* out[b, :] = emb[tokens[b, len[b] - 1], :] + pos[len[b] - 1, :] (bf16): wft_embed_fwd for ONE token per sequence at the
 * position device memory names (TextDecoder.forward's `offset` under a kv_cache upstream).  Same bits as wft_embed_fwd.   */
int wft_decode_embed(const int64_t* tokens, int64_t ld_tokens, const int32_t* len, const float* emb, const float* pos,
                     wft_bf16* out, int B, int n_ctx, int d, int64_t V, void* stream);
/* Greedy pick for every sequence from its bf16 logits row (logits + b*ld; only the first V columns are read):
 *  columns with suppress[col] != 0 are removed (u8 [V] or NULL: upstream's SuppressTokens); suppress_first (u8 [V] or NULL)
 *    removes more for a row's FIRST generated token only, i.e. while len[b] == first_len[b] (upstream's SuppressBlank);
 *  pick = argmax of what is left, lowest index on ties (the rule of wft_ce_fwd / wft_token_stats); logprob = its
 *    log-probability under the softmax of the SUPPRESSED logits (upstream's GreedyDecoder.update runs after the filters);
 *  an unfinished row: tokens[b, len[b]] = pick, sum_logprob[b] += logprob, len[b] += 1,
 *    finished[b] = pick == eot || len[b] == max_len.  A finished row is frozen: nothing of its state changes (upstream stops
 *    adding log-probabilities once the last token is eot).  unfinished[0] = number of rows still unfinished after the update.
 *  pick_out i64 [B] / logprob_out f32 [B] (optional): what the step computed for every row, finished or not.                */
typedef struct {
  const wft_bf16* logits; int64_t ld; int64_t V;
  const uint8_t* suppress; const uint8_t* suppress_first; const int32_t* first_len;
  int64_t* tokens; int64_t ld_tokens;
  int32_t* len; int32_t* finished; float* sum_logprob; int32_t* unfinished;
  int64_t* pick_out; float* logprob_out;
  int B; int eot; int max_len;
} wft_decode_pick_args;
int wft_decode_pick(const wft_decode_pick_args* args, void* stream);

/* ---------------------------------------------------------- Beam search */
/* Beam-search decoding on a KV cache shared between the beams (csrc/decode_attn.hip, csrc/decode_beam.hip; DESIGN.md §3 "Beam-search layouts"): upstream's
 * `BeamSearchDecoder` + `MaximumLikelihoodRanker` with `without_timestamps=True`, restated in engine/decode/beam.py (neither is in the
 * reference tree and openai-whisper is not a dependency: parity with the upstream binary is unpinned).  W = beam size (1..8);
 * audio a owns the R = B*W slot rows r = a*W + j.
 *
 * Single-token attention for beams; q / o / scale / q_prescaled / head_dim 64 as in wft_attn_decode_args.
 *  self form (len != NULL; anc != NULL; group must be 1): R hypotheses over a cache of R slot rows.  Key t < len[r] - 1 of row r
 *    is read at slot anc[r*ld_anc + t] (i32; a value outside 0..R-1 reads slot r), i.e. at k_cache + slot*cache_bs + t*ld_cache;
 *    the step's k / v rows (k_new / v_new + r*ld_new) are written to slot r at position len[r] - 1 and take part as that key;
 *    anc[r, len[r] - 1] is not used.  Nothing else is written: a beam reorder permutes rows of `anc`, keys never move.  Same
 *    key-to-lane dealing, split and merge order as wft_attn_decode_bf16: the output is bit-identical to that call on a cache
 *    gathered by `anc`.
 *  cross form (len == NULL; anc ignored): R = A*group query rows over a read-only cache of A = R/group audios, the `group`
 *    consecutive rows of an audio share its keys / values.  One workgroup per (audio, head, split) reads each K / V block once
 *    and runs the online softmax of all `group` rows against it.  Split rule: the keys of an (audio, head) are cut in
 *    nsplit = clamp(ceil(256 / (A*H)), 1, min(ceil(Tk / 512), 16)) — the rule of wft_attn_decode_bf16 with its B set to A, the
 *    number of AUDIOS.  Per query row the arithmetic order is that of wft_attn_decode_bf16 at the same split: wherever this
 *    nsplit equals the one that call takes at B = R rows, the output is bit-identical to it on a group-times replicated cache.
 *  workspace: wft_attn_decode_beam_workspace_bytes(args) bytes (0: none needed).  No atomics: reruns are bit-identical.        */
typedef struct {
  const wft_bf16* q; int64_t ldq;
  const wft_bf16* k_new; const wft_bf16* v_new; int64_t ld_new;
  wft_bf16* k_cache; wft_bf16* v_cache; int64_t ld_cache; int64_t cache_bs;
  wft_bf16* o; int64_t ldo;
  const int32_t* len;
  const int32_t* anc; int64_t ld_anc;
  int R; int H; int Tk; int group; float scale; int q_prescaled;
  void* workspace; int64_t workspace_bytes;
} wft_attn_decode_beam_args;
int wft_attn_decode_beam_bf16(const wft_attn_decode_beam_args* args, void* stream);
int64_t wft_attn_decode_beam_workspace_bytes(const wft_attn_decode_beam_args* args);
/* The k = W + 1 best continuations of every logits row (bf16, logits + i*ld; only the first V columns are read), i = 0..rows-1.
 * Logits row i belongs to state row r = i*row_step (row_step = 1: one logits row per hypothesis; row_step = W: the prefill's one
 * row per audio).  Masks exactly as wft_decode_pick: `suppress` always, `suppress_first` while len[r] == first_len[r].
 *  cand_logp[r*k + c] = log-softmax over the live columns of the c-th largest live logit, cand_tok[r*k + c] = its column;
 *  descending, ties to the lower column.  Fewer than k live columns: the rest is (-1, -inf).  2 <= k <= 9.                   */
typedef struct {
  const wft_bf16* logits; int64_t ld; int64_t V;
  const uint8_t* suppress; const uint8_t* suppress_first; const int32_t* first_len; const int32_t* len;
  int32_t* cand_tok; float* cand_logp;
  int rows; int row_step; int k;
} wft_decode_topk_args;
int wft_decode_topk(const wft_decode_topk_args* args, void* stream);
/* Timestamp rules: upstream's `whisper.decoding.ApplyTimestampRules`, restated (openai-whisper is not a dependency: parity with the
 * upstream binary is unpinned).  Columns ts_begin .. V-1 are timestamps (eot < ts_begin < V); no_timestamps: a column or -1;
 * max_initial: upstream's max_initial_timestamp_index, or -1 for none.  The SAMPLED tokens of state row r are
 * tokens[r, first_len[r] : len[r]]; the kernels read them, there is no other rule state.  After the `suppress` / `suppress_first`
 * masks, in upstream's order:
 *  1. column no_timestamps is removed;
 *  2. last_ts = the last sampled token is >= ts_begin; pen_ts = fewer than two sampled tokens, or the one before the last is >=
 *     ts_begin.  last_ts && pen_ts: columns ts_begin..V-1 are removed; last_ts && !pen_ts: columns 0..eot-1 are removed;
 *  3. t = the last sampled token that is a timestamp, if any: columns ts_begin..t-1 are removed, and t too unless last_ts && !pen_ts;
 *  4. no sampled token yet: columns 0..ts_begin-1 are removed and, with max_initial >= 0, the columns above ts_begin + max_initial;
 *  5. over what is still live: if logsumexp of the timestamp columns is STRICTLY greater than the largest log-probability of a
 *     column below ts_begin (both under the softmax of the live row, so log sum_ts exp(x - m) > max_text - m; an empty side is
 *     -inf), every column below ts_begin is removed.
 * The pick / the candidates and their log-probabilities are taken under the softmax of the finally live columns, as with the
 * static masks alone.  Every column removed: the pick is eot with log-probability 0, the candidates are (-1, -inf).  first_len and
 * len are required.  wft_decode_topk_ts reads the token rows of the state rows r = i*row_step at tokens + r*ld_tokens.          */
typedef struct { int ts_begin; int no_timestamps; int max_initial; } wft_ts_rules;
int wft_decode_pick_ts(const wft_decode_pick_args* args, const wft_ts_rules* rules, void* stream);
int wft_decode_topk_ts(const wft_decode_topk_args* args, const wft_ts_rules* rules, const int64_t* tokens, int64_t ld_tokens, int eot,
                       void* stream);
/* One beam-search step for every audio that is not done, from the candidate lists of wft_decode_topk (k = W + 1 per row):
 *  candidates (j, i), j = beam, i = list position, score = sum_logprob[a*W + j] + cand_logp[a*W + j][i] (one fp32 add); `first`
 *    != 0: only j = 0 contributes (the W copies of the prompt are one hypothesis).  Order: score descending, ties to the lower
 *    j, then the lower i (ranked by counting).  Walked in that order: an `eot` candidate is a newly finished sequence (beam j's
 *    tokens + eot, that score), any other one becomes the next beam slot s = 0, 1, .. until W are saved; eot candidates below
 *    that point are dropped.  Newly finished sequences are appended in walk order while the audio's list holds fewer than C.
 *  written per audio: tokens[a*W + s, :len] = old row of the source beam, tokens[.., len] = the token, sum_logprob = the score,
 *    len + 1 on all W rows; anc rows permuted the same way IN PLACE and anc[a*W + s, len - 1] = a*W + source j (the slot whose
 *    step wrote that position); fin_tokens[a, p, :] (i64, row stride ld_tokens; padded with eot), fin_len[a, p] (eot counted),
 *    fin_score[a, p], fin_n[a]; done[a] = fin_n[a] == C || new len == max_len.  A done audio is frozen: nothing of it changes.
 *  unfinished[0] = number of audios not done after the update.  src_out i32 [B*W] (optional): the source beam j of every new
 *    slot of an audio that was updated (others untouched).                                                                    */
typedef struct {
  const int32_t* cand_tok; const float* cand_logp;
  int64_t* tokens; int64_t ld_tokens;
  int32_t* anc; int64_t ld_anc;
  int32_t* len; float* sum_logprob;
  int32_t* done; int32_t* unfinished;
  int64_t* fin_tokens; int32_t* fin_len; float* fin_score; int32_t* fin_n;
  int32_t* src_out;
  int B; int W; int C; int eot; int max_len; int first;
} wft_beam_update_args;
int wft_beam_update(const wft_beam_update_args* args, void* stream);

/* ------------------------------------------------------ Sampled decoding */
/* wft_decode_pick / wft_decode_pick_ts with a temperature per state row (csrc/decode_pick.hip): upstream's `GreedyDecoder.update` at
 * temperature > 0 (`Categorical(logits / temperature).sample()`), restated with a counter-based generator on the device
 * (openai-whisper is not a dependency: parity with the upstream binary and with torch's random stream is unpinned).
 *  rows: args->B = R state rows; state row r reads logits row r / group (group >= 1, R % group == 0), so the prefill's one row per
 *    audio feeds all `group` samples of that audio.  Everything else in `args` is per state row, as in wft_decode_pick.
 *  temperature f32 [R], seed u64 [R]: DEVICE memory, read by the kernel; nothing of the launch depends on their values (one
 *    captured graph serves every temperature and every seed).
 *  live columns: exactly those of wft_decode_pick / wft_decode_pick_ts — the suppress / suppress_first masks, then the timestamp
 *    rules; rule 5 is decided on the UNTEMPERED row (upstream's filters run before the division by the temperature).
 *  t = temperature[r] <= 0: the row behaves as wft_decode_pick(_ts) does, bit for bit in pick, log-probability and state.
 *  t > 0: key(col) = x[col] * (1.0f / t) + g(col) in fp32 over the live columns; pick = arg-max of the key, ties to the lower
 *    column; a live column whose logit is -inf is never picked (the Gumbel-max rule: the pick is a draw from softmax(x / t)).
 *  logprob: the pick's log-softmax over the live columns at temperature 1 (upstream sums F.log_softmax(logits) of the sampled
 *    token, not the tempered one).
 *  state update: that of wft_decode_pick word for word — a finished row is frozen; tokens / sum_logprob / len / finished /
 *    max_len / unfinished[0] / pick_out / logprob_out as there; no live column: the pick is eot with log-probability 0.
 *  noise: g(col) = -logf(-logf(v)) with the accurate logf; v from Philox4x32-10 (Salmon et al. 2011: multipliers 0xD2511F53 /
 *    0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) under key = (low, high 32 bits of seed[r]), counter = (col >> 2, L, 0, 0)
 *    with L = len[r] before the update (the position the token is written to); output word col & 3; k = word >> 9;
 *    v = (2k + 1) * 2^-24 — an odd 24-bit integer scaled: exact in fp32, inside (0, 1).  Known answers: counter 0, key 0 ->
 *    6627e8d5 e169c58d bc57ac4c 9b00dbd8; all-ones counter and key -> 408f276d 41c83b0e a20bc7c6 6d5451fd.  The noise depends on
 *    (seed, position, column) only — not on masks, batch, group or launch shape.  No atomics: reruns are bit-identical.
 *  errors (returned without a launch): NULL temperature / seed; group < 1 or R % group != 0; whatever wft_decode_pick /
 *    wft_decode_pick_ts reject.                                                                                                  */
typedef struct { const float* temperature; const uint64_t* seed; int group; } wft_sample_rules;
int wft_decode_sample(const wft_decode_pick_args* args, const wft_sample_rules* sample, void* stream);
int wft_decode_sample_ts(const wft_decode_pick_args* args, const wft_sample_rules* sample, const wft_ts_rules* rules, void* stream);

/* ------------------------------------------------- Word-level alignment */
/* The device stages of upstream's `whisper/timing.py: find_alignment` (csrc/align.hip; DESIGN.md §3 "Word timestamps"): the
 * cross-attention probabilities of the alignment heads, their standardisation / median filter / head mean, and dynamic time
 * warping with its backtrace.  Upstream's behaviour is restated (openai-whisper is not a dependency: parity with its binary is
 * unpinned); the reference tree only carries the `alignment_heads` state (model/model_utils.py:171-174, :363-377).
 * Per-audio lengths are DEVICE int32 [B] arrays, as in the decode kernels; every kernel clamps them to its static extents (a
 * negative length is 0, a length above the extent is the extent), so no length can make a kernel address out of bounds.
 *
 * wft_attn_probs_bf16: probs[b, s, t, j] = softmax_j(scale * q[b, t, heads[s]] . k[b, j, heads[s]]) over j < n_key[b], for
 *  t < n_tok[b], in fp32.
 *  args: q / ldq / q_bs, k / ldk / k_bs, B, H, Tq, Tk, scale of wft_attn_args, in its addressing (element (b, t, h, d) at
 *    q + b*q_bs + t*ldq + h*64 + d, so the cross-attention [B, Tk, 2d] {k | v} buffer is consumed in place); rows 16-byte
 *    aligned; q_prescaled must be 0 (only the self-attention q projection is prescaled) — the kernel multiplies the fp32
 *    score by scale * log2(e), callers fold a `qk_scale` into scale; the other fields are not read;
 *  heads i32 [n_heads]: distinct head indices in any order (an index outside [0, H) is clamped); slice s of the output belongs
 *    to heads[s];
 *  n_tok[b] query rows are used, n_key[b] keys take part: upstream's `weights[:, :, :num_frames // 2]` cut BEFORE the softmax,
 *    so keys at or beyond n_key[b] carry no mass;
 *  probs f32: element (b, s, t, j) at probs + b*p_bs + s*p_hs + t*ldp + j (an offset pointer per layer fills one
 *    [B, n_sel_total, Tq, Tk] buffer); rows t >= n_tok[b] and columns j >= n_key[b] are NOT written;
 *  scores: bf16 MFMA products with fp32 accumulation, recomputed for the second pass; exp2 of the hardware; one normalised
 *    write (p = exp2(s - max) * (1 / sum)).  No atomics: reruns are bit-identical.
 *
 * wft_align_matrix: matrix[b, t, j] = mean over the n_sel heads of median_filter_j((p - mean_t p) / std_t p), t < n_tok[b],
 *  j < n_key[b]; other elements are NOT written.
 *  1. every frame column of every head is standardised over the n_tok[b] token rows with the BIASED deviation (upstream's
 *     `torch.std_mean(weights, dim=-2, unbiased=False)`), the mean first and the deviation from the differences, in fp32, IEEE division and square root; a column that is
 *     constant over the tokens has deviation 0 and yields non-finite values, as upstream;
 *  2. median over a window of `width` (odd, 1..31; upstream's default 7) frames, reflect-padded by width / 2 (torch's
 *     F.pad(mode="reflect"): column -i reads column i, column n - 1 + i reads n - 1 - i);
 *  3. n_key[b] <= width / 2: no filter for that audio (upstream's early return of `median_filter`);
 *  4. the heads are summed in slice order in fp32 and divided by n_sel.
 *  probs: as written by wft_attn_probs_bf16 with n_sel slices; Tq <= 448; matrix element (b, t, j) at matrix + b*m_bs + t*ldm + j.
 *
 * wft_dtw_f32: the path of upstream's `dtw_cpu` / `dtw_cuda` in fp32 (its CUDA path is fp32, its CPU path fp64: this is the
 *  fp32 one) over x = -matrix[b, row0 : row0 + n_rows[b], 0 : n_cols[b]] (negate != 0; negate == 0 reads the matrix as it is —
 *  negation is exact), N = n_rows[b] <= n_rows_max <= 448, M = n_cols[b] <= n_cols_max:
 *    cost[0, 0] = 0, cost[0, j] = cost[i, 0] = inf; for i in 1..N, j in 1..M with c0 = cost[i-1, j-1], c1 = cost[i-1, j],
 *    c2 = cost[i, j-1]:  c0 < c1 && c0 < c2 -> (c0, trace 0);  else c1 < c0 && c1 < c2 -> (c1, trace 1);  else (c2, trace 2);
 *    cost[i, j] = x[i-1, j-1] + c.
 *  Every cell is ONE fp32 add of a fixed pair of operands, so the anti-diagonal sweep gives the serial loop's bits and path.
 *  Backtrace from (N, M): record (i-1, j-1), then trace 0 -> (i-1, j-1), 1 -> (i-1, j), 2 -> (i, j-1), until (0, 0).
 *  path_text / path_time i32 [B, ld_path] (ld_path >= n_rows_max + n_cols_max - 1): the recorded pairs in FORWARD order,
 *    path_len[b] of them; entries beyond path_len[b] are not written; N == 0 or M == 0 gives path_len[b] = 0.
 *  matrix_rows: the rows a matrix holds per audio (row0 + n_rows_max <= matrix_rows is checked on the host).
 *  workspace: wft_dtw_workspace_bytes(B, n_rows_max, n_cols_max) bytes (the trace, kernel-internal).
 *
 * wft_word_spans: upstream's arithmetic behind the path (`jumps`, `jump_times`, the word boundaries, the mean token probability)
 *  for a ragged batch in one launch, on the paths of wft_dtw_f32 where they lie — frames stay integers, the caller divides.
 *  path_text / path_time i32 [B, ld_path], path_len i32 [B]: as wft_dtw_f32 writes them (rows in [0, n_rows_max), n_rows_max <= 448).
 *  bounds i32 [B, ld_bounds]: bounds[b, w] = the path row at which word w starts, w = 0 .. n_words[b] (n_words[b] + 1 entries,
 *    bounds[b, 0] = 0, strictly increasing, the last one the row of the eot): np.pad(np.cumsum(counts[:-1]), (1, 0)) of upstream.
 *  n_words i32 [B]; token_probs f32 [n_probs], packed over the audios; tok_off i32 [B]: the first element of audio b in it.
 *  first[b, r] = path_time[b, p] at the LOWEST p < path_len[b] with path_text[b, p] == r — on a DTW path (rows never decrease,
 *    every row occurs) upstream's `jumps`: position 0 and every position at which the text index changes; a row that does not
 *    occur gives -1.
 *  start_frame[b, w] = first[b, bounds[b, w]], end_frame[b, w] = first[b, bounds[b, w + 1]]  (i32, at b*ld_words + w);
 *  prob[b, w] = (sum in ascending i of token_probs[tok_off[b] + i], bounds[b, w] <= i < bounds[b, w + 1], one fp32 running sum)
 *    / (float)count, one IEEE division.
 *  Lengths are clamped to the static extents: path_len to [0, ld_path], n_words to [0, min(ld_bounds - 1, ld_words, n_rows_max)],
 *    a bound to [0, n_rows_max - 1], tok_off to [0, n_probs]; a token index at or beyond n_probs adds 0.  Elements with
 *    w >= n_words[b] are NOT written; path_len[b] == 0 or n_words[b] == 0 writes nothing for that audio.
 *  One workgroup per audio, one owner per row and per word: no atomics, reruns are bit-identical.                                  */
int wft_attn_probs_bf16(const wft_attn_args* args, const int32_t* heads, int n_heads, const int32_t* n_tok, const int32_t* n_key,
                        float* probs, int64_t p_bs, int64_t p_hs, int64_t ldp, void* stream);
int wft_align_matrix(const float* probs, int64_t p_bs, int64_t p_hs, int64_t ldp, const int32_t* n_tok, const int32_t* n_key,
                     float* matrix, int64_t m_bs, int64_t ldm, int B, int n_sel, int Tq, int Tk, int width, void* stream);
int64_t wft_dtw_workspace_bytes(int B, int n_rows_max, int n_cols_max);
int wft_dtw_f32(const float* matrix, int64_t m_bs, int64_t ldm, int matrix_rows, int row0, const int32_t* n_rows,
                const int32_t* n_cols, int B, int n_rows_max, int n_cols_max, int negate, int32_t* path_text, int32_t* path_time,
                int64_t ld_path, int32_t* path_len, void* workspace, int64_t workspace_bytes, void* stream);
int wft_word_spans(const int32_t* path_text, const int32_t* path_time, int64_t ld_path, const int32_t* path_len, const int32_t* bounds,
                   int64_t ld_bounds, const int32_t* n_words, const float* token_probs, int64_t n_probs, const int32_t* tok_off,
                   int32_t* start_frame, int32_t* end_frame, float* prob, int64_t ld_words, int B, int n_rows_max, void* stream);

/* ------------------------------- Language detection and long-form windows */
/* csrc/transcribe.hip: the two device stages of upstream's `detect_language` and of the window loop of `transcribe()`
 * (engine/transcribe.py), restated; openai-whisper is not a dependency: parity with its binary is unpinned.
 *
 * wft_lang_probs: upstream masks every column that is not a language token with -inf, then takes the argmax and the softmax.
 *  logits bf16 [B, ld] in the layout of the tied logits product (only columns < V are meaningful); lang_ids i32 [n_lang] in device
 *    memory, strictly increasing, each in [0, V) (the caller checks that; an id outside is clamped), 1 <= n_lang <= 1024.
 *  probs[b, j] (at probs + b*ld_probs + j) = exp(x[b, lang_ids[j]] - lse_b) with lse_b over the n_lang language columns only, in
 *    fp32: d = x - max, s = sum exp(d), p = exp(d - log(s)), accurate expf / logf.
 *  best[b] = lang_ids[j*], j* the LOWEST j that attains the maximum (the tie rule of wft_token_stats and wft_decode_pick).
 *  One workgroup per row reads the n_lang gathered values, never the whole row: what the other columns hold (inf, NaN) does not
 *  matter.  Fixed summation order, no atomics: the same arguments give the same bits.
 *
 * wft_mel_windows: out[r] = pad_or_trim(mel_a[:, seek[r] : seek[r] + n_win], n_win) with a = audio[r], for R rows at once.
 *  mel f32: the A recordings' long log-mels packed in one buffer, recording a = [n_mels, ld_frames[a]] row-major from element
 *    mel_off[a]; content_frames[a] = ld_frames[a] - n_win, the frames that are not the trailing padding of n_win frames.
 *    mel_off i64 [A], ld_frames / content_frames i32 [A], audio / seek i32 [R]: all in device memory.
 *  out f32 [R, n_mels, n_win]: out[r, m, t] = mel_a[m, seek[r] + t] bit for bit for t < min(n_win, content_frames[a] - seek[r]),
 *    and 0.0f from there on — upstream's zero pad, NOT the log-mel of the padding that the source holds at those frames.
 *  A seek outside [0, content_frames[a]) is the caller's argument error; the kernel clamps audio, seek and the frame counts so
 *  that it never addresses anything outside [mel_off[a], mel_off[a] + n_mels * ld_frames[a]).
 *  n_win % 4 == 0 and mel / out 16-byte aligned: every store is 16 bytes; the source start has any alignment (aligned 16-byte
 *  loads, the four frames selected from two neighbouring chunks).                                                            */
int wft_lang_probs(const wft_bf16* logits, int64_t ld, int64_t V, const int32_t* lang_ids, int n_lang, float* probs,
                   int64_t ld_probs, int64_t* best, int B, void* stream);
int wft_mel_windows(const float* mel, const int64_t* mel_off, const int32_t* ld_frames, const int32_t* content_frames,
                    const int32_t* audio, const int32_t* seek, float* out, int R, int A, int n_mels, int n_win, void* stream);

/* ------------------------------------------------- Log-mel + SpecAugment */
/* whisper.audio.log_mel_spectrogram (data/data_loader.py:278; SURVEY.md App.
 * A.2): reflect-pad 200, Hann-400 STFT hop 160, |.|^2, mel filterbank,
 * log10(clamp 1e-10), floor at clip max - 8, (x+4)/4.
 * audio f32 [B, n_samples] (n_samples = 160 * n_frames); filters f32
 * [n_mels, 201]; out f32 [B, n_mels, n_frames]; clipmax f32 [B] workspace.   */
int wft_logmel(const float* audio, const float* filters, float* out, float* clipmax,
               int B, int n_samples, int n_mels, int n_frames, void* stream);
/* SpecAugment on a batch of log-mels, all parameters already drawn on the
 * host in the reference's order (data/data_loader.py:284-290,
 * data/utils.py:41-143,146-190): per clip 8 ints
 *   {apply_warp, warp_p, warp_d, t0, t1, f0, f1, unused} and 2 ints
 *   {extreme_low_len, extreme_high_len}.
 * in/out f32 [B, n_mels, T]; must not alias.                                  */
int wft_specaug(const float* in, float* out, const int32_t* params, const int32_t* extremes,
                int B, int n_mels, int T, void* stream);
/* mel f32 [B, n_mels, T] -> time-major, channel-padded, row-padded bf16
 * [B, T+2, c_pad] with zero rows 0 and T+1 (the conv1d k=3 p=1 halo) — the
 * layout the conv-as-GEMM stem consumes (model/model_utils.py:276).          */
int wft_mel_to_tmajor_bf16(const float* mel, wft_bf16* out, int B, int n_mels, int T,
                           int c_pad, void* stream);
/* d(mel) is never needed (inputs carry no grad). */
/* Sample-rate conversion in front of the log-mel: torchaudio's `sinc_interp_hann` resampler with its defaults
 * (lowpass_filter_width 6, rolloff 0.99), restated; torchaudio is not a dependency: parity with its binary is unpinned.
 *  With o = orig, n = new_rate (already divided by their gcd), base = 0.99 * min(o, n), width = ceil(6 * o / base) and
 *    g(t) = (base / o) * sinc(pi t) * cos^2(pi t / 12) for |t| < 6, exactly 0 otherwise:
 *    out[m] = sum_j x[j] * g((j / o - m / n) * base), 0 <= m < n_out = ceil(n_in * n / o), x[j] = 0 outside [0, n_in).
 *  Polyphase form: m * o = j0 * n + r, 0 <= r < n; only j = j0 + k, k in [-width + 1, width], can contribute, with the weight
 *    taps[r][k + width - 1] = g((k - r / n) * base / o).  taps f32 [new_rate, 2 * width] in device memory, 8-byte aligned: the
 *    caller builds it (data/gpu_frontend.py `resample_taps`: float64, rounded once to f32).
 *  Row b reads in + b * ld_in and writes out + b * ld_out, B <= 65535.  Elements j >= n_in of an input row are never read (they
 *    count as zeros, like j < 0); elements m >= n_out of an output row are never written.
 *  Each output is ONE f32 fma chain in ascending k from 0.0f: its bits do not depend on B, on the row, or on how the outputs
 *    are tiled over workgroups.  No atomics.  m * o is formed in 64 bits (at 44.1 kHz it passes 2^31 after 304 s of audio).
 *  WFT_ERR_ARG, before any launch: orig / new_rate not coprime, n_out != ceil(n_in * new_rate / orig), a leading dimension
 *    smaller than its row, or a rate pair whose tile does not fit (wft_resample_tile == 0).  Loads of the input are 16 bytes
 *    wherever a chunk lies inside the row; stores are 4 bytes per lane, neighbouring lanes writing neighbouring outputs (a thread
 *    holds outputs of ONE phase r, n apart, so that a table row is loaded once for all of them).
 * wft_resample_tile: outputs per workgroup for a rate pair — a pure host function, at most 1024 and a multiple of 4, smaller when
 *  the input span of 1024 outputs would not fit the 8192-float staging buffer; 0 = the pair is not supported.              */
int wft_resample_f32(const float* in, int64_t ld_in, int64_t n_in, const float* taps, int orig, int new_rate, int width,
                     float* out, int64_t ld_out, int64_t n_out, int B, void* stream);
int wft_resample_tile(int orig, int new_rate, int width);

/* ------------------------------------------------- Time stretch (audio-domain augmentation) */
/* The reference's baseline pipeline is audiomentations' TimeStretch(min_rate, max_rate, leave_length_unchanged=False, p=1.0) on the
 * raw clip, in front of the log-mel.  The algorithm restated here is the one audiomentations calls `librosa_phase_vocoder`, i.e.
 * librosa.effects.time_stretch.  Neither library is a dependency: parity with their binaries is unpinned.  DEVIATION: current
 * audiomentations defaults to a C++ time-stretching library (method "signalsmith_stretch") that cannot be restated; this is the
 * phase-vocoder method, not that default.
 *
 * For one row y of n samples and a float64 rate, with N = 2048 and H = 512:
 *  1. STFT.  y is zero-padded by N/2 samples on both sides (center=True, pad_mode="constant": NOT reflect).  F = 1 + n / H frames
 *     (integer division); frame t is the padded samples t H .. t H + N - 1 times the periodic Hann w_i = 0.5 - 0.5 cos(2 pi i / N);
 *     D[t, k], k = 0 .. 1024, is its one-sided DFT.
 *  2. Vocoder.  T = ceil(F / rate) in float64 (the length of numpy's arange(0, F, rate)); D is extended by two zero frames.
 *     For t = 0 .. T - 1: step = t * rate in float64, i = floor(step), alpha = step - i,
 *       mag = (1 - alpha) |D[i]| + alpha |D[i + 1]|,  S[t] = mag * P[t],
 *       P[0] = u(D[0]),  P[t + 1] = P[t] * u(D[i + 1]) * conj(u(D[i])),
 *     u(c) = c / |c|, and u(c) = 1 whenever |c| == 0, whatever the signs of its zeros (numpy's angle(-0 + 0j) = pi must not leak
 *     into a bin: the loader's clips are zero-padded).  This is librosa's accumulator phase_acc += phi_advance + wrap(dangle -
 *     phi_advance) taken modulo 2 pi (the phi_advance terms cancel modulo 2 pi); in float64 the two forms agree to 1e-9 on the
 *     test cases (tests/test_stretch_host.py).  The product needs no fp32 angle accumulator, which would reach 2e6 rad and lose
 *     every bit of the phase; P is renormalised every step.  step, its floor and alpha are formed in double in the kernel: a
 *     column pair chosen one off is an O(1) error.
 *  3. ISTFT.  The inverse one-sided DFT of every S[t] (the imaginary parts of bins 0 and 1024 do not count) times the same window,
 *     overlap-added at hop H — each output sample sums its <= 4 frames in ascending t — and divided by the window's sum of squares
 *     over the same frames wherever that exceeds FLT_MIN; the first N/2 samples are dropped; the output has
 *     n_out = (int)rint(n / rate) samples in float64 (half to even), zeros where no frame reaches.
 * rate == 1.0 is not special-cased.  Rates lie inside [rate_lo, 2.0] with 0.5 <= rate_lo: rate_lo is the HOST's lower bound of the
 * device-side rates, and sizes the grids and the workspace.  A row whose rate lies outside (or is NaN) is not processed: nothing of
 * its output row is written and n_out[b] = -1; no store leaves the buffers whatever the device-side rates hold.
 *
 *  in f32: row b at in + b * ld_in, n_in samples (1 <= n_in <= 2^26), what lies behind them is never read.  rates f64 [B], n_out
 *  i32 [B] (written), both in device memory.  out f32: row b at out + b * ld_out, ld_out >= rint(n_in / rate_lo); exactly
 *  n_out[b] samples of row b are written and what lies behind them is left untouched.
 *  workspace: wft_time_stretch_workspace_bytes(B, n_in, rate_lo) bytes (-1: bad arguments), 8-byte aligned:
 *    D f32 [B, F, 1025, 2] followed by S f32 [B, T_max, 1025, 2], T_max = ceil(F / rate_lo).  At 30 s (n_in = 480000, F = 938) D
 *    is 7.7 MB per clip and S up to 15.4 MB at rate_lo = 0.5: the caller may process rows in chunks to cap it.
 *  The bits of a row depend on its samples, its rate and n_in only: not on B, its batch partners, rate_lo or the launch.  No atomics.
 *  All entry points enqueue on `stream`, do not synchronise and do not allocate; every argument is checked before the first launch.
 * The three stages, exported so that a failure can be localised; wft_time_stretch_f32 is exactly these three in order:
 *  wft_stretch_stft_f32     in -> D.  One workgroup per (frame, row), the 2048-point FFT in LDS (16 KiB of complex f32, twiddles from
 *                           a sincospif table built once per workgroup).
 *  wft_stretch_vocoder_f32  D -> S: frames t < T_b of row b are written, the others are left untouched.
 *  wft_stretch_istft_f32    S -> out, n_out.  S IS OVERWRITTEN: the windowed frame t takes the first 2048 floats of the 2050 that
 *                           S[b, t] occupies.                                                                                   */
int64_t wft_time_stretch_workspace_bytes(int B, int64_t n_in, double rate_lo);
int wft_time_stretch_f32(const float* in, int64_t ld_in, int64_t n_in, const double* rates, double rate_lo, float* out,
                         int64_t ld_out, int32_t* n_out, void* workspace, int64_t workspace_bytes, int B, void* stream);
int wft_stretch_stft_f32(const float* in, int64_t ld_in, int64_t n_in, float* D, int B, void* stream);
int wft_stretch_vocoder_f32(const float* D, int64_t n_in, const double* rates, double rate_lo, float* S, int B, void* stream);
int wft_stretch_istft_f32(float* S, int64_t n_in, const double* rates, double rate_lo, float* out, int64_t ld_out,
                          int32_t* n_out, int B, void* stream);
/* Log-mel of rows of different lengths (the stretched clips), same filters and per-frame arithmetic as wft_logmel (one device
 * body: equal samples give equal bits).  Row b at audio + b * ld_audio has n_samples[b] samples (device i32, clamped to
 * [0, max_samples]; max_samples > 400 is the host's upper bound and sizes the grid) and frames_b = n_samples[b] / 160 frames; the
 * reflect padding uses n_samples[b], which need not be a multiple of 160.  The `max - 8` floor takes the maximum over ALL frames_b
 * frames, also those at or beyond T_out (the reference takes the log-mel of the whole stretched clip before pad_or_trim).
 * out f32 [B, n_mels, T_out]: columns < kept = min(keep_frames[b], frames_b, T_out) hold the normalised log-mel, the columns behind
 * them the minimum of the kept columns (the reference's min-value pad_or_trim and its cut at a partial segment; the clamp and
 * (v + 4) / 4 are monotone, so it is the minimum of the computed values bit for bit); kept == 0: the whole row is 0.
 * stats: f32 [2 B] workspace.                                                                                                  */
int wft_logmel_ragged(const float* audio, int64_t ld_audio, const int32_t* n_samples, const int32_t* keep_frames,
                      const float* filters, float* out, float* stats, int B, int max_samples, int n_mels, int T_out, void* stream);

/* ------------------------------------------------- IIR filter (audio-domain augmentation) */
/* A cascade of S second-order sections over every row of a batch, each row with its own coefficients and its own length: the
 * primitive behind the seven filters of the reference's advanced pipeline (low-/high-/band-pass, band-stop, low/high shelf, peaking;
 * data/filters.py designs and draws them) and behind any user-supplied filter.
 *
 * Arithmetic (the contract).  sos f64 [B, S, 6] in device memory, section s of row b = b0 b1 b2 a0 a1 a2 with a0 == 1 (a0 is NOT
 * read: the caller normalises).  Every section is direct form II transposed in fp64, as scipy.signal.sosfilt does it:
 *     y = b0 x + z0;   z0 = b1 x - a1 y + z1;   z1 = b2 x - a2 y
 * sections in index order (the y of one is the x of the next), zero initial state.  The input sample is widened to fp64 and the last
 * section's output is rounded to f32 ONCE.  Row b filters its first n[b] samples (n: device i32 [B], clamped to [0, n_max] inside the
 * kernels; NULL = n_max for every row); out[b, n[b] .. n_max) is written as zero; nothing at or behind n_max of an output row is
 * touched and nothing at or behind n[b] of an input row is read.  A row whose S sections are all exactly 1 0 0 . 0 0 is copied bit
 * for bit (the sign of zero included).  out == in with ld_out == ld_in is allowed (in place); any other overlap is refused.
 *
 * Parallel form.  The cascade is one linear system with 2 S states.  A row is cut into chunks of L = wft_sos_filter_chunk() samples:
 * (1) every chunk runs from zero state and keeps its final state z_c; (2) column j of the L-step zero-input transition matrix M is
 * the state after L zero-input steps of the same code from the unit state e_j; (3) a sequential scan per row, s_0 = 0,
 * s_(c+1) = M s_c + z_c (the products summed in ascending column order, then z_c), gives every chunk its true initial state;
 * (4) every chunk runs again from s_c and writes its outputs.  Exact in exact arithmetic; in fp64, with products and sums free to
 * contract into FMAs, a row stays within delta = 2^-30 of the sequential recurrence, relative to the row's largest output
 * (tests/_filter_cases.py measures the scheme and states the bound).  A workgroup owns G = wft_sos_filter_group() consecutive chunks,
 * staged through LDS so that global traffic is coalesced.  L and G are compile-time constants; the bits of a row depend on its
 * samples, its coefficients, n[b], L and G only: not on B, its batch partners or the launch.
 *
 *  in / out f32: row b at in + b * ld_in / out + b * ld_out, ld >= n_max, 1 <= n_max <= 2^30, 1 <= B <= 65535, 1 <= S <= 4.
 *  workspace: wft_sos_filter_workspace_bytes(B, n_max, S) bytes (-1: bad arguments), 8-byte aligned: f64 [B, ceil(n_max / L), 2 S].
 *  No atomics, no allocation, no synchronisation: three launches on `stream`.  Every host-visible argument is checked before the
 *  first launch (WFT_ERR_ARG: null pointer, S outside 1..4, B or n_max out of range, a leading dimension smaller than n_max, a short
 *  workspace, misalignment, partial overlap of in and out).                                                                       */
int64_t wft_sos_filter_workspace_bytes(int B, int64_t n_max, int S);
int wft_sos_filter_chunk(void);
int wft_sos_filter_group(void);
int wft_sos_filter_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const double* sos, int S, float* out,
                       int64_t ld_out, void* workspace, int64_t workspace_bytes, int B, void* stream);

/* ------------------------------------------------- Wave effects (audio-domain augmentation) */
/* Additive noise, clipping and level changes over every row of a ragged batch (csrc/wavefx.hip; DESIGN.md §3 "Wave effects"): six
 * transforms of the reference's advanced pipeline that are plain arithmetic on the waveform (audiomentations' AddGaussianNoise,
 * AddGaussianSNR, ClippingDistortion, Gain, GainTransition, Shift), restated from the published source; the library is not a
 * dependency and parity with its binary is unpinned.  ONE call applies ONE stage to every row; composing stages is the caller's job.
 *
 * fx: DEVICE array of B records, 8-byte aligned, 88 bytes each.  A kind of 0 (or an unknown kind) means "none" for that stage.
 *
 * Shared rules.  Row b covers n[b] samples (n: device i32 [B], clamped to [0, n_max] inside the kernels; NULL = n_max for every row).
 * Out of place, out[b, n[b] .. n_max) is written as zero; in place nothing behind n[b] is touched.  Nothing at or behind n_max of an
 * output row is written and nothing at or behind n[b] of an input row is read.  A row whose kind for the stage is "none" passes
 * through bit for bit.  Arithmetic is fp64 with ONE rounding to f32, products and sums NOT contracted into FMAs (the file is compiled
 * with contraction off, so the operations are the ones written here).  No float atomics (integer atomics on counts only), no
 * allocation, no host synchronisation; reruns are bit-identical; a row's bits depend on its samples, its record and n[b] only.
 *
 * WFT_FX_NOISE.  out[i] = f32(x[i] + sigma * z(i)).
 *   WFT_FX_GAUSSIAN_NOISE: sigma = noise_value (an amplitude).
 *   WFT_FX_GAUSSIAN_SNR:   sigma = rms / 10^(noise_value / 20), noise_value in dB, rms = sqrt(sum x^2 / n[b]) over the row's n[b]
 *     samples.  The sum is fp64 in a fixed order: chunk c covers samples [c K, (c + 1) K), K = 4096; thread t of 256 adds its samples
 *     c K + t, c K + t + 256, ... in ascending order; the 256 sums are halved pairwise (s[t] += s[t + h], h = 128 .. 1); the chunks'
 *     sums are added in ascending order.  rms = 0 or n[b] = 0 gives sigma = 0.
 *   sigma == 0: the row passes through bit for bit.
 *   z(i): Philox4x32-10 as in "Sampled decoding" above (same multipliers, Weyl constants and known answers), key = (low, high 32
 *     bits of seed), counter = (i >> 2, 0, 0, 0); w = 2 * ((i >> 1) & 1); u1 from word w, u2 from word w + 1, each (2k + 1) * 2^-24
 *     with k = word >> 9 (so u1 is never 0); r = sqrt(-2 ln u1); z = r * cos(t) for even i, r * sin(t) for odd i, t = (2 pi) * u2 with
 *     2 pi = 6.283185307179586; log, sqrt, cos, sin in fp64.
 * WFT_FX_CLIP (WFT_FX_CLIPPING).  clip_q: an integer percent, clamped to 0..50 inside the kernels.  With s the row's n[b] samples
 *   sorted ascending under the total order of the key k(x) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) (so -0.0 sorts before
 *   +0.0): for p in {clip_q, 100 - clip_q}, m = p * (n[b] - 1) in 64-bit integers, j = m / 100, g = (m % 100) / 100.0;
 *   threshold = s[j] bit for bit when g == 0 (s[j + 1] is not touched), else f32(s[j] + g * (s[j + 1] - s[j])).  lo, hi = the two
 *   thresholds; out[i] = x[i] < lo ? lo : (x[i] > hi ? hi : x[i]) (a sample equal to a threshold, -0.0 against +0.0 included,
 *   keeps its own bits; NaN passes).  This is np.percentile(method="linear") and np.clip.  The selection is exact: a radix select over
 *   the keys in three passes (11, 11, 10 bits), the four ranks side by side; it runs over the clipping rows only (a device-side list;
 *   the launches are not sized by B).  n[b] = 0 does nothing, n[b] = 1 makes both thresholds the sample.
 *   The thresholds of row b are left in the workspace as f32 at byte offset 8 + 4 * ((B + 1) / 2 * 2) + 8 * b (lo, hi).
 * WFT_FX_LEVEL.
 *   WFT_FX_GAIN:  out[i] = x[i] * gain_ratio, one f32 multiply (the host computes gain_ratio = f32(10^(dB / 20))).
 *   WFT_FX_GAIN_TRANSITION:  dB(i) = db_start + (db_end - db_start) * min(max((double)(i - t0) / (double)max(ramp_len - 1, 1), 0), 1);
 *     out[i] = f32(x[i] * 10^(dB(i) / 20)).  t0 may be negative or beyond n[b]: db_start holds before the ramp, db_end after it.
 *   WFT_FX_SHIFT:  s = (i64) nearbyint(shift_fraction * n[b]) (ties to even), reduced to [0, n[b]); d = (i - s) mod n[b];
 *     out[i] = x[d] * w(i): a rotation with rollover (the padding inside n[b] rotates with the clip).  F = min(max(fade_len, 0),
 *     n[b] / 2), D = max(F - 1, 1).  s == 0 or F == 0: w = 1 everywhere (a copy).  Otherwise, with e = n[b] - 1 - d (the distance to
 *     the seam from below; the seam lies between output indices s - 1 and s, cyclically):
 *       d < F:  w = d / D   (the fade in: exactly 0 at output index s, exactly 1 at s + F - 1 when F >= 2)
 *       e < F:  w = e / D   (the fade out: exactly 0 at s - 1, exactly 1 at s - F when F >= 2)
 *       else    w = 1 and the sample is copied bit for bit.
 *     A faded sample is f32((double)x[d] * w), w in fp64.  F = 1 zeroes the two samples at the seam.
 *     A shift row needs out != in.  The records are device memory, so the library cannot see the kinds: a LEVEL call with
 *     out == in is accepted and is only defined when no row is a shift row (engine/kernels.py wave_fx decides that from its host copy
 *     of the records and goes through a temporary).
 *
 *  in / out f32: row b at in + b * ld_in / out + b * ld_out, ld >= n_max, 1 <= n_max <= 2^30, 1 <= B <= 65535; out == in with
 *  ld_out == ld_in is in place, any other overlap is refused.  workspace: wft_wave_fx_workspace_bytes(B, n_max, stage) bytes (-1: bad
 *  arguments), 8-byte aligned.  wft_wave_fx_tile(): the samples of one workgroup trip of the apply pass.
 *  WFT_ERR_ARG before any launch: null pointer (in, fx, out, workspace), unknown stage, B or n_max out of range, a leading dimension
 *  below n_max, a short workspace, misalignment (in / out / n 4 bytes, fx / workspace 8), partial overlap of in and out.         */
enum { WFT_FX_NOISE = 0, WFT_FX_CLIP = 1, WFT_FX_LEVEL = 2 };
enum { WFT_FX_NONE = 0, WFT_FX_GAUSSIAN_NOISE = 1, WFT_FX_GAUSSIAN_SNR = 2 };     /* noise_kind */
enum { WFT_FX_CLIPPING = 1 };                                                     /* clip_kind  */
enum { WFT_FX_GAIN = 1, WFT_FX_GAIN_TRANSITION = 2, WFT_FX_SHIFT = 3 };           /* level_kind */
typedef struct {
  int32_t noise_kind, clip_kind, level_kind, clip_q; /*  0  4  8 12 */
  uint64_t seed;                                     /* 16 */
  double noise_value;                                /* 24: amplitude (gaussian_noise) or SNR in dB (gaussian_snr) */
  float gain_ratio; int32_t reserved;                /* 32 36 */
  double db_start, db_end;                           /* 40 48 */
  int64_t t0, ramp_len;                              /* 56 64 */
  double shift_fraction;                             /* 72 */
  int64_t fade_len;                                  /* 80 */
} wft_wave_fx;
int64_t wft_wave_fx_workspace_bytes(int B, int64_t n_max, int stage);
int wft_wave_fx_tile(void);
int wft_wave_fx_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const wft_wave_fx* fx, int stage, float* out,
                    int64_t ld_out, void* workspace, int64_t workspace_bytes, int B, void* stream);

/* ------------------------------------------------- Per-row rate conversion (audio-domain augmentation) */
/* Resampling at a fractional rate that differs from row to row of a ragged batch (csrc/rate.hip; DESIGN.md §3 "Rate effects"): the
 * missing half of the advanced pipeline's PitchShift and the whole of its Aliasing.  Neither audiomentations nor librosa is a
 * dependency.  Shared rules: fp64 arithmetic with ONE rounding to f32, products and sums NOT contracted into FMAs (the file is compiled
 * with contraction off); no atomics, no allocation, no host synchronisation; every argument is checked before the launch; reruns are
 * bit-identical; a row's bits depend on its samples and its parameters only — not on B, its batch partners, the tiling or the host's
 * bound; index arithmetic is 64-bit; 1 <= B <= 65535; in and out must not overlap (a workgroup reads neighbours that another may
 * have written).
 *
 * wft_sinc_resample_rows_f32: the resampler of the pitch shift (a time stretch by 2^(-s/12), wft_time_stretch_f32, followed by this
 *  with the same rate as the ratio and n_out = the original length: librosa.effects.pitch_shift with its fix_length).  It is the
 *  continuous form of the filter of wft_resample_f32 above (torchaudio's sinc_interp_hann, width 6, rolloff 0.99).  For row b:
 *    rho = ratio[b] = output rate / input rate, float64 in DEVICE memory, inside [ratio_lo, 2.0], 0.5 <= ratio_lo <= 2.0; ratio_lo is
 *      the HOST's lower bound of the ratios and sizes the tile and the staging buffer only.
 *    N = n_in[b] (device i32) clamped to [0, n_in_max]; the -1 that wft_time_stretch_f32 writes for a refused row counts as 0.
 *    c = 0.99 * min(1, rho);  g(t) = c * sinc(pi c t) * cos^2(pi c t / 12) for |c t| < 6 and exactly 0 otherwise, sinc(0) = 1.
 *    out[m] = sum_j x[j] * g(j - t0),  t0 = (double)m / rho (ONE IEEE float64 division), x[j] = 0 outside [0, N),
 *      for 0 <= m < min(n_out, ceil(N * rho)) (the product and its ceil in float64); for m from there up to n_out, out[m] = 0.
 *    At rho = n / o this is the g((j / o - m / n) * base) of wft_resample_f32 algebraically: (j / o - m / n) * base =
 *      (j - m o / n) * 0.99 min(o, n) / o = c (j - t0), and base / o = c.
 *    The taps are summed in ascending j in fp64, t = (double)j - t0 and a = c * t each one rounding, the test |a| < 6 on that a;
 *      the weight is (c * (sinpi(a) / (pi * a))) * cospi(a / 12)^2, evaluated per tap (13 taps at rho >= 1, up to 25 at rho = 0.5).
 *    rho == 1.0 is not special-cased: it is a low-pass at 0.99 of Nyquist, not a copy.
 *    A row whose device-side ratio lies outside [ratio_lo, 2.0], or is NaN, is written as n_out zeros.  No load or store leaves the
 *      buffers whatever the device-side values hold.  Elements at or behind n_in[b] of an input row are never read; elements at or
 *      behind n_out of an output row are never written.
 *  in f32: row b at in + b * ld_in, ld_in >= n_in_max, 1 <= n_in_max <= 2^30; out f32: row b at out + b * ld_out, ld_out >= n_out,
 *  1 <= n_out <= 2^30.  WFT_ERR_ARG: a null pointer, ratio_lo outside [0.5, 2.0] (or NaN), a bad shape, a short leading dimension,
 *  misalignment (in / out / n_in 4 bytes, ratio 8), overlap.
 *  wft_sinc_resample_rows_tile(ratio_lo): outputs per workgroup, a pure host function: at most 1024, a multiple of 4, smaller when
 *  the input span of 1024 outputs at ratio_lo would not fit the 1600-float staging buffer (784 at 0.5); 0 = ratio_lo not supported.
 *
 * wft_alias_f32: audiomentations' Aliasing.apply, restated (parity with its binary unpinned; numpy's arithmetic held bit for bit):
 *    n = len(samples); x = np.linspace(0, n, num=n); d = round(n * float(new_rate) / sample_rate)
 *    u = np.linspace(0, n, num=d); out = np.interp(x, u, np.interp(u, x, samples))
 *  both interpolations in one pass.  In float64, as numpy forms them: step_x = n / (n - 1), x_i = i * step_x with the last point
 *  exactly n; d = (i64) rint(((double)n * new_rate) / sample_rate), half to even; step_u = n / (d - 1), u_k = k * step_u with the
 *  last point exactly n.  np.interp(t, grid, f): with j the largest index whose grid point is <= t, the value is f_j when j is the
 *  last index or grid_j == t, and otherwise ((f_{j+1} - f_j) / (grid_{j+1} - grid_j)) * (t - grid_j) + f_j.  j = floor(t / step),
 *  corrected against the formed grid values.  The result is numpy's float64 value rounded once to f32 for finite samples (numpy's
 *  second try after a NaN result, which only infinite samples reach, is not restated).
 *    n[b]: device i32, clamped to [0, n_max], or NULL (every row covers n_max samples).  new_rate f64 [B] in device memory.
 *    A row with new_rate[b] == 0, n[b] < 2 or d < 2 (also: a NaN rate, d above 2^32) is a copy of its bits.  out[b, n[b] .. n_max)
 *    is written as zero.  Nothing at or behind n[b] of an input row is read, nothing at or behind n_max of an output row is written.
 *  in / out f32: row b at in + b * ld_in / out + b * ld_out, ld >= n_max, 1 <= n_max <= 2^30.  WFT_ERR_ARG: a null pointer (in,
 *  new_rate, out), sample_rate outside (0, 1e9] (or NaN), a bad shape, a short leading dimension, misalignment, overlap.
 *  wft_alias_tile(): outputs per workgroup.
 * DEVIATIONS of the loader option built on these (data/rate_fx.py): its own gates, independent of the wave stages; a default
 * Aliasing maximum of the clip rate, not audiomentations' 30 000 Hz; the Hann-windowed sinc instead of librosa's soxr_hq; the
 * phase-vocoder pitch shift, not audiomentations' current default; timestamps untouched, as in the reference.                     */
int wft_sinc_resample_rows_f32(const float* in, int64_t ld_in, const int32_t* n_in, int64_t n_in_max, const double* ratio,
                               double ratio_lo, float* out, int64_t ld_out, int64_t n_out, int B, void* stream);
int wft_sinc_resample_rows_tile(double ratio_lo);
int wft_alias_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const double* new_rate, double sample_rate,
                  float* out, int64_t ld_out, int B, void* stream);
int wft_alias_tile(void);

/* ------------------------------------------------- Office effects (audio-domain augmentation) */
/* Room reverb and bit crush of the reference's office pipeline (get_audio_augments_office, model/augment.py) over a ragged batch
 * (csrc/office.hip; DESIGN.md §3 "Office effects").  Neither audiomentations nor pyroomacoustics is a dependency.  Shared rules: no
 * atomics, no allocation, no host synchronisation; every host-visible argument is checked before the first launch; reruns are
 * bit-identical; index arithmetic is 64-bit; 1 <= B <= 65535; 1 <= n_max <= 2^30; in / out f32: row b at in + b * ld_in /
 * out + b * ld_out, ld_in, ld_out >= n_max; N = n[b] (device i32) clamped to [0, n_max], n == NULL = n_max for every row;
 * out[b, N .. n_max) is written as zero; nothing at or behind n_max of an output row is written; nothing at or behind n[b] of an input
 * row is read.
 *
 * wft_fir_conv_f32: a causal FIR over every row, each row with an impulse response of its own length (the room simulation's shoebox
 *  response, or a measured one: audiomentations' ApplyImpulseResponse):
 *    out[b][i] = sum_{j < T} ir[b][j] * x[b][i - j]  for 0 <= i < N, with x = 0 outside [0, N); the tail is chopped at N (the
 *    reference's leave_length_unchanged=True).  T = n_taps[b] (device i32) clamped to [0, taps_max], n_taps == NULL = taps_max.
 *    ir f32: row b at ir + b * ld_ir, ld_ir >= taps_max, 1 <= taps_max <= 8192; nothing at or behind n_taps[b] of an IR row is read.
 *    A row with T == 0 is a copy of its bits.
 *  Method: uniform-partitioned overlap-save in f32 on a 2048-point radix-2 FFT, L = wft_fir_conv_block() = 1024 new outputs per
 *  block.  Pass 1: the IR of row b in P = ceil(taps_max / 1024) partitions, each zero-padded to 2048 and transformed into the
 *  workspace as H[b][p][0..1024].  Pass 2, one workgroup per (output block k, row): for each live partition p in ascending order
 *  (p < ceil(T / 1024) and p <= k; segments in front of the row's start are all zeros) the FFT of x[(k-p-1) * 1024 .. (k-p+1) * 1024),
 *  X * H_p accumulated over the one-sided bins, ONE inverse FFT of the Hermitian extension, the last 1024 reals scaled by 1 / 2048.
 *  The error of an element is bounded by C * 11 * 2^-24 * sum_p ||x_seg(k-p)||_2 * ||h_p||_2 over its block's live partitions
 *  (tests/_office_cases.py holds C and how it was measured).
 *    A row's bits depend on its samples, its IR, n[b], n_taps[b] and L only — not on B, its batch partners or taps_max: a partition
 *    that lies wholly behind n_taps[b] contributes nothing (not a sum with zeros, which would turn a -0.0 into +0.0).
 *    In place is impossible (a block reads samples that an earlier block's owner may have overwritten): ANY overlap of in and out is
 *    WFT_ERR_ARG, as is an overlap of either with ir or the workspace.  Also WFT_ERR_ARG: a null pointer (in, ir, out, workspace), a
 *    bad shape, a short leading dimension, a workspace below wft_fir_conv_workspace_bytes(B, taps_max) = B * P * 1025 * 8 bytes (-1:
 *    bad arguments), misalignment (in / out / ir / n / n_taps 4 bytes, workspace 8).
 *
 * wft_bitcrush_f32: audiomentations' BitCrush.apply, restated: q = 2^(bits-1) + 1 as an exact f32, y = rintf(x * q) / q — an f32
 *  multiply, round half to even, then a correctly rounded f32 divide, not contracted: numpy's np.round(samples * q) / q on an f32
 *  array, bit for bit.  bits: device i32 [B]; bits[b] == 0 makes the row a copy of its bits, and so does EVERY value outside
 *  {0} u [1, 24] (2^24 + 1 is not an f32).  In place (out == in and ld_out == ld_in) is allowed; any other overlap is WFT_ERR_ARG, as
 *  are a null pointer (in, bits, out), a bad shape, a short leading dimension, misalignment (4 bytes).
 * DEVIATIONS of the loader option built on these (data/office_fx.py): the image-source method only (audiomentations' default
 * use_ray_tracing=True is stochastic inside pyroomacoustics and is not restated: no late tail beyond max_order); no air absorption; no
 * output normalisation; Mp3Compression's slot is dropped; own gates (the reference's marginal rates: crush 0.25, room 0.5);
 * pyroomacoustics and audiomentations are not available, so parity with their binaries is unpinned; timestamps untouched.           */
int wft_fir_conv_block(void);
int64_t wft_fir_conv_workspace_bytes(int B, int taps_max);
int wft_fir_conv_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const float* ir, int64_t ld_ir,
                     const int32_t* n_taps, int taps_max, float* out, int64_t ld_out, void* workspace, int64_t workspace_bytes, int B,
                     void* stream);
int wft_bitcrush_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const int32_t* bits, float* out, int64_t ld_out,
                     int B, void* stream);

/* ------------------------------------------------- Loudness and background noise (audio-domain augmentation) */
/* LoudnessNormalization and AddBackgroundNoise of the reference's advanced pipeline (get_audio_augments_advanced, model/augment.py)
 * over a ragged batch (csrc/mix.hip; DESIGN.md §3 "Mix effects"), restated from the published sources of pyloudnorm
 * (Meter.integrated_loudness for one channel, normalize.loudness) and audiomentations (AddBackgroundNoise); neither is a dependency
 * and parity with their binaries is unpinned.  Shared rules: no float atomics, no allocation, no host synchronisation; every
 * host-visible argument is checked before the first launch; reruns are bit-identical; fp64 products and sums are NOT contracted into
 * FMAs; 1 <= B <= 65535; 1 <= n_max <= 2^30; in / out f32: row b at in + b * ld_in / out + b * ld_out, ld >= n_max; N = n[b] (device
 * i32) clamped to [0, n_max], n == NULL = n_max for every row; nothing at or behind n[b] of an input row is read; out == in with
 * ld_out == ld_in is in place (nothing behind n[b] is touched), any other overlap is WFT_ERR_ARG; out of place out[b, N .. n_max) is
 * written as zero; nothing at or behind n_max of an output row is written.
 *
 * wft_loudness_f32: the ITU-R BS.1770 integrated loudness of every row and, with an output, one gain per row.
 *   sos: HOST f64 [2][6], the two K-weighting sections b0 b1 b2 a0 a1 a2 with a0 == 1 (data/gpu_frontend.py k_weighting: the RBJ high
 *   shelf G = 4 dB, Q = 1/sqrt(2), fc = 1500 Hz and high pass Q = 0.5, fc = 38 Hz, each divided by its a0); it is read before the
 *   call returns.  hop = rate / 10 samples, 512 <= hop <= 2^24; block = 4 * hop.  target: device f64 [B] in LUFS; mode: device i32
 *   [B], 0 = copy the row, 1 = normalise it.  out == NULL measures only: EVERY row is measured, target and mode may be NULL.  With an
 *   output target and mode are required and only the rows of mode 1 are measured; a row of mode 0 is copied bit for bit and its
 *   stats are (-inf, -inf, 0, 1).  stats: device f64 [B, 4] = (L in LUFS, the relative gate Gr, the number of blocks over both
 *   gates, the gain applied).
 *   1. y = the two sections over the row's N samples from zero state, fp64, direct form II transposed per section
 *      (y = b0 x + z0; z0 = b1 x - a1 y + z1; z1 = b2 x - a2 y), the sample widened to fp64; y is never rounded to f32.
 *   2. with q, r = divmod(N - block, hop): nb = q + 1 + (1 if 2 r > hop or (2 r == hop and q odd) else 0) blocks, which is
 *      int(np.round((T - 0.4) / 0.1)) + 1 in integers (round half to even).
 *   3. block j covers samples [j hop, j hop + block); the rounded-up last block is cut at N and still divided by block:
 *      z_j = sum y^2 / block.   4. l_j = -0.691 + 10 log10(z_j).
 *   5. J1 = {j : l_j >= -70}; Gr = -0.691 + 10 log10(mean of z over J1) - 10.
 *   6. J2 = {j : l_j > Gr and l_j > -70}; L = -0.691 + 10 log10(mean of z over J2).
 *   7. J1 or J2 empty, or N < block: L = -inf (Gr = -inf when J1 is empty) and the row is copied bit for bit (pyloudnorm raises for
 *      the short clip: a stated deviation).  A target or an L that is not finite copies the row as well.
 *   8. gain = f32(10^((target - L) / 20)), formed in fp64; out = x * gain, ONE f32 multiply; no clipping afterwards.
 *   Parallel form.  The recurrence is cut as wft_sos_filter_f32 cuts it, at S = 2: chunks of 512 samples from zero state, the per-row
 *   scan of the chunk states, the chunks again from their true state (within delta = 2^-30 of the sequential recurrence, relative
 *   to the row's largest |y|).  The second pass adds y^2 in ascending sample order into the at most two hop-slots
 *   [k hop, (k + 1) hop) its chunk touches; a slot's sum is its chunks' partials in chunk order; z_j = (((e_j + e_j+1) + e_j+2) +
 *   e_j+3) / block over the slots that exist.  A gate's mean: thread t of 256 adds its blocks t, t + 256, ... in ascending order,
 *   the 256 sums are halved pairwise (s[t] += s[t + h], h = 128 .. 1).  A row's bits depend on its samples, N, hop, sos and target
 *   only — not on B, its batch partners or the launch.
 *   workspace: wft_loudness_workspace_bytes(B, n_max, hop) bytes (-1: bad arguments), 8-byte aligned.  WFT_ERR_ARG: a null pointer
 *   (in, sos, stats, workspace; target or mode with an output), a bad shape or hop, a short leading dimension or workspace,
 *   misalignment (in / out / n / mode 4 bytes, the rest 8), a section that is not finite or has a0 != 1, partial overlap.
 *
 * wft_bg_mix_f32: a scaled entry of a noise bank added to every row.  bank: device f32 [total], the entries back to back; bank_off:
 *   device i64 [K + 1], entry e = bank[bank_off[e] .. bank_off[e + 1]), K >= 1; rec: device array of B records, 8-byte aligned, 24
 *   bytes each.  kind 0 (or unknown) = none: the row is copied bit for bit, its stats are (0, 0, 0).  entry is clamped to
 *   [0, K - 1] and offset into the entry inside the kernels (the caller checks them: engine/kernels.py bg_mix).
 *   stats: device f64 [B, 3] = (clean RMS, noise RMS, scale).
 *   1. for entry e of length m: s(i) = e[(offset + i) mod m], i < N; offset is 0 when m <= N (a short entry repeats), and at most
 *      m - N otherwise (a long one does not wrap).
 *   2. noise RMS over the first min(m, N) samples of s (audiomentations measures the loaded segment before it tiles it).
 *   3. clean RMS over the row's N samples.
 *   4. both sums of squares are fp64 in the fixed order of WFT_FX_GAUSSIAN_SNR above: chunks of 4096, thread t of 256 adds its
 *      samples c K + t, c K + t + 256, ... ascending, the 256 sums are halved pairwise, the chunks' sums are added in ascending order.
 *   5. noise RMS < 1e-9 (or N == 0, or a db that is not finite): the row is copied bit for bit, scale = 0.
 *   6. WFT_BG_SNR: desired = clean RMS / 10^(db / 20); WFT_BG_ABSOLUTE: desired = 10^(db / 20).
 *   7. scale = desired / noise RMS in fp64; out[i] = f32((double)x[i] + scale * (double)s(i)), one rounding.
 *   The sums run over the rows whose kind is not none.  workspace: wft_bg_mix_workspace_bytes(B, n_max) bytes (-1: bad arguments),
 *   8-byte aligned.  WFT_ERR_ARG: a null pointer, a bad shape, K < 1, a short leading dimension or workspace, misalignment (in / out
 *   / n / bank 4 bytes, the rest 8), partial overlap of in and out.
 * DEVIATIONS of the loader option built on these (data/mix_fx.py): own gates at the reference's marginal rates; the offset is drawn
 * as an integer, not in seconds; the short clip is copied where pyloudnorm raises; the block count is in integers; no
 * noise_transform; the bank is .npy arrays (no audio decoding).                                                                 */
enum { WFT_BG_NONE = 0, WFT_BG_SNR = 1, WFT_BG_ABSOLUTE = 2 };                    /* kind */
typedef struct {
  int32_t kind, entry; /*  0  4 */
  int64_t offset;      /*  8 */
  double db;           /* 16: the SNR (snr) or the noise's RMS level (absolute), in dB */
} wft_bg_rec;
int64_t wft_loudness_workspace_bytes(int B, int64_t n_max, int hop);
int wft_loudness_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const double* sos, int hop, const double* target,
                     const int32_t* mode, float* out, int64_t ld_out, double* stats, void* workspace, int64_t workspace_bytes, int B,
                     void* stream);
int64_t wft_bg_mix_workspace_bytes(int B, int64_t n_max);
int wft_bg_mix_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const float* bank, const int64_t* bank_off, int K,
                   const wft_bg_rec* rec, float* out, int64_t ld_out, double* stats, void* workspace, int64_t workspace_bytes, int B,
                   void* stream);

/* ------------------------------------------------- PCM decode (audio files) */
/* The sample data of audio files — the `data` chunk of a WAV file, or headerless PCM — to mono f32 over a ragged batch of
 * recordings, ONE launch (csrc/pcm.hip; DESIGN.md §3 "Audio files").  The header is parsed on the host (data/audio_io.py
 * parse_wav); the bytes go to the device as they are in the file.  Conventions of libsndfile and scipy.io.wavfile; neither is a
 * dependency.
 *
 * raw: device bytes, ANY alignment; rows: device table of B records, 8-byte aligned; out f32: row b at out + b * ld_out,
 * ld_out >= n_max; 1 <= B <= 65535; 1 <= n_max <= 2^30; raw_bytes >= 1.  Row b decodes `frames` frames of `channels` interleaved
 * little-endian samples that start at raw + byte_off:
 *   1. every channel sample becomes an exact fp64 value:
 *        WFT_PCM_U8     (b - 128) / 128                    WFT_PCM_S16LE  v / 2^15
 *        WFT_PCM_S24LE  v / 2^23, three bytes sign-extended WFT_PCM_S32LE  v / 2^31
 *        WFT_PCM_F32LE, WFT_PCM_F64LE  the value as it is
 *        WFT_PCM_ALAW, WFT_PCM_ULAW    G.711 expanded to its 16-bit integer in integer arithmetic (no table), then / 2^15:
 *          u-law: u = ~code; t = (((u & 15) << 3) + 132) << ((u >> 4) & 7); v = (u & 128) ? 132 - t : t - 132
 *                 (0x00 -> -32124, 0x80 -> +32124, 0x7F and 0xFF -> 0);
 *          A-law: a = code ^ 0x55; s = (a >> 4) & 7; t = (a & 15) << 4; t = s == 0 ? t + 8 : (t + 264) << (s - 1);
 *                 v = (a & 128) ? t : -t  (0x55 -> -8, 0xD5 -> +8, 0x2A -> -32256, 0xAA -> +32256).
 *   2. channel >= 0 takes that channel's value; channel == -1 adds the values in channel order 0 .. C - 1 in fp64 and divides the
 *      sum by C in fp64 (a division, not a multiplication by a reciprocal).
 *   3. ONE rounding, fp64 -> f32, to nearest even: F32LE mono or picked comes out bit for bit (finite values, infinities and f32
 *      subnormals); NaN stays NaN, its payload is unpinned.
 *   4. out[b, j] = 0 for frames <= j < n_max; columns n_max .. ld_out - 1 are never written.
 * A row's bits depend on its own bytes and its table row only — not on B, its batch partners or the launch.
 * Memory safety: the table is device memory, so the kernel checks every row itself: a row decodes as frames = 0 (all zeros) when
 * format is outside the enum, channels outside 1..8, channel outside -1..channels-1, frames outside 0..n_max, byte_off < 0 or
 * byte_off + frames * frame_bytes > raw_bytes.  Global loads are 16-byte loads of aligned 16-byte granules; a byte outside
 * [raw, raw + raw_bytes) is touched only inside a granule that also holds a byte of the row's frames.
 * wft_pcm_decode_tile(): the output frames per workgroup (the seams the tests walk over).
 * WFT_ERR_ARG, nothing launched: a null raw / rows / out, raw_bytes < 1, B or n_max outside its range, ld_out < n_max, rows not
 * 8-byte or out not 4-byte aligned.                                                                                             */
enum { WFT_PCM_U8 = 0, WFT_PCM_S16LE, WFT_PCM_S24LE, WFT_PCM_S32LE, WFT_PCM_F32LE, WFT_PCM_F64LE, WFT_PCM_ALAW, WFT_PCM_ULAW };
typedef struct {       /* one row, 32 bytes, in DEVICE memory */
  int64_t byte_off;    /*  0: first byte of the row's first frame inside raw; any alignment */
  int32_t frames;      /*  8: frames to decode */
  int32_t channels;    /* 12: 1..8, interleaved */
  int32_t format;      /* 16: WFT_PCM_* */
  int32_t channel;     /* 20: -1 = mean of all channels; 0..channels-1 = that channel */
  int32_t reserved[2]; /* 24: 0 */
} wft_pcm_row;
int wft_pcm_decode_tile(void);
int wft_pcm_decode_f32(const uint8_t* raw, int64_t raw_bytes, const wft_pcm_row* rows, float* out, int64_t ld_out, int64_t n_max,
                       int B, void* stream);

/* ---------------------------------------------------------------- Edit counts */
/* Hits, substitutions, deletions and insertions of the Levenshtein alignment of a ragged batch of (reference, hypothesis) pairs,
 * ONE launch (csrc/edit.hip; DESIGN.md §3 "Edit counts"): the evaluator's WER / CER (jiwer.wer / jiwer.cer in the reference,
 * eval/evaluator.py:105-106) and how the errors split.
 *
 * A pair is a reference r[0..n) and a hypothesis h[0..m) of int32 symbols; only equality of symbols matters (every int32 value is a
 * symbol, negative ones and the two extremes included).  Cell (i, j), 0 <= i <= n, 0 <= j <= m, holds a triple (S, D, I) with cost
 * S + D + I:
 *   (0, 0) = (0, 0, 0);  (i, 0) = (0, i, 0);  (0, j) = (0, 0, j);
 *   (i, j) takes the cheapest of three candidates, in this priority on equal cost:
 *     1. diagonal:  the triple of (i-1, j-1), with S + 1 if r[i-1] != h[j-1];
 *     2. deletion:  the triple of (i-1, j), with D + 1;
 *     3. insertion: the triple of (i, j-1), with I + 1.
 *   A later candidate replaces an earlier one only when it is strictly cheaper.
 * The result is (H, S, D, I) of cell (n, m) with H = n - S - D.  It follows that S + D + I is the Levenshtein distance (unique),
 * H + S + D = n and H + S + I = m.  The split into S, D and I is the one this priority selects: jiwer / rapidfuzz may pick another
 * optimal alignment — that parity is UNPINNED; the rates (S + D + I) / n are pinned.
 *
 * sym: device int32 [n_sym], n_sym >= 1; rows: device table of P records, 8-byte aligned; out int32: out[p * ld_out + 0..3] =
 * H, S, D, I of pair p, ld_out >= 4, no other element of out is written; 1 <= P <= 2^20; 1 <= max_len <= wft_edit_max_len() = 4096
 * (the cap per side; the launch's LDS is sized from max_len, so pass the longest side of the batch, not the cap).
 * A row's counts depend on its own symbols and its table row only — not on P, its batch partners or max_len.
 * Memory safety: the table is device memory, so the kernel checks every row itself: a row writes -1 four times and reads no symbol
 * when ref_len or hyp_len lies outside [0, max_len], an offset is negative, or offset + length > n_sym.  No table can make the
 * kernel read outside [sym, sym + n_sym).
 * wft_edit_threads(): the threads of a workgroup = the cells of a diagonal computed per pass (the seams the tests walk over).
 * WFT_ERR_ARG, nothing launched: a null sym / rows / out, n_sym < 1, P or max_len outside its range, ld_out < 4, rows not 8-byte or
 * sym / out not 4-byte aligned.                                                                                                  */
typedef struct {        /* one pair, 32 bytes, in DEVICE memory */
  int64_t ref_off;      /*  0: first symbol of the reference inside sym */
  int64_t hyp_off;      /*  8: first symbol of the hypothesis inside sym */
  int32_t ref_len;      /* 16: 0 .. max_len */
  int32_t hyp_len;      /* 20: 0 .. max_len */
  int32_t reserved[2];  /* 24: 0 */
} wft_edit_row;
int wft_edit_max_len(void);
int wft_edit_threads(void);
int wft_edit_counts_i32(const int32_t* sym, int64_t n_sym, const wft_edit_row* rows, int32_t* out, int64_t ld_out, int P,
                        int max_len, void* stream);

/* ---------------------------------------------------------------- AdamW */
/* torch.optim.AdamW single-tensor step over a flat f32 range
 * (model/optimizer.py:240-262 → optimizer.step() in model_utils.py:122).
 * g is multiplied by gscale[0] (device scalar: the clip_grad_norm_ coefficient,
 * model_utils.py:107) before use.  If p_bf16 != NULL the bf16 shadow is
 * refreshed in the same pass.                                                */
int wft_adamw_step(float* p, const float* g, float* m, float* v, wft_bf16* p_bf16,
                   int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float bias_corr1, float bias_corr2,
                   const float* gscale, void* stream);
/* out[0] += sum(g^2) over n elements (for the global grad norm).             */
int wft_sumsq_f32(const float* g, int64_t n, float* out, void* stream);

/* ------------------------------------------------ multi-tensor optimizer step */
/* One launch for a whole parameter list (model/optimizer.py:240-262, optimizer.step() at
 * model_utils.py:122, torch.nn.utils.clip_grad_norm_ at model_utils.py:107).
 * The tensor list is a caller-owned table in DEVICE memory:
 *   tab[row * n + t]  int64  address of tensor t's row-th array (row meaning per function)
 *   numel[t]          int64  elements of tensor t
 *   chunk_start[t]    int32  index of tensor t's first WFT_MT_CHUNK-element chunk; chunk_start[n] =
 *                            total_chunks = sum_t ceil(numel[t] / WFT_MT_CHUNK)                        */
#define WFT_MT_CHUNK 65536
/* out[0] = sum over all tensors of g^2 (tab row 0 = g, f32; a zero address = no gradient this step, contributes
 * nothing).  partial: f32 [total_chunks] scratch.  Two fixed-order stages: bitwise reproducible.   */
int wft_mt_sumsq_f32(const void* tab, const int64_t* numel, const int32_t* chunk_start, int n,
                     int total_chunks, float* partial, float* out, void* stream);
/* torch.optim.AdamW step for every tensor (tab rows: 0 p, 1 g, 2 exp_avg, 3 exp_avg_sq; all f32).
 * If sumsq != NULL, g is first scaled by min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)): clip_grad_norm_
 * folded into the same pass (28 B/parameter of HBM traffic in total).                           */
int wft_mt_adamw(const void* tab, const int64_t* numel, const int32_t* chunk_start, int n,
                 int total_chunks, float lr, float beta1, float beta2, float eps,
                 float weight_decay, float bias_corr1, float bias_corr2, const float* sumsq,
                 float max_norm, void* stream);

/* 8-bit AdamW: `bnb.optim.AdamW8bit` / `Adam8bit` of the reference's `optimizer.8bit: True` (model/optimizer.py:241-256; the
 * third-party package bitsandbytes is neither vendored nor installed: published algorithm, Dettmers et al. 2022 — PARITY
 * UNPINNED, see oracle/adam8bit_oracle.py).  The two moments are stored as one byte per element in blocks of
 * WFT_Q8_BLOCK = 2 048 elements with an f32 absmax per block; byte c decodes to qmap[c] * absmax.
 * tab rows: 0 p (f32), 1 g (f32), 2 state1 (u8 codes of m), 3 state2 (u8 codes of v), 4 absmax1 (f32 [ceil(numel / 2048)]),
 * 5 absmax2.  qmap1 / qmap2: the two ascending 256-entry f32 maps (signed / unsigned dynamic quantisation) in device memory.
 * Per block: dequantise, m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2 (g scaled by the clip coefficient as in wft_mt_adamw),
 * p += -lr * sqrt(bias_corr2) / bias_corr1 * m / (sqrt(v) + sqrt(bias_corr2) * eps), p *= 1 - lr * weight_decay, then the new
 * absmax of the block and the nearest map entry of m / absmax1, v / absmax2.  16 B / parameter of HBM traffic (28 with f32
 * state).  Chunks (WFT_MT_CHUNK elements) hold whole blocks, so blocks never span tensors.                               */
#define WFT_Q8_BLOCK 2048
int wft_mt_adamw8(const void* tab, const int64_t* numel, const int32_t* chunk_start, int n,
                  int total_chunks, const float* qmap1, const float* qmap2, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float bias_corr1, float bias_corr2, const float* sumsq,
                  float max_norm, void* stream);

/* --------------------------------------------------------------------- Muon */
/* The reference builds `muon.MuonWithAuxAdam` (third-party package `muon`, git HEAD, not vendored:
 * pyproject.toml:29, model/optimizer.py:171-237).  Its update for a 2-D parameter is
 *   buf = lerp(buf, g, 1-beta);  u = lerp(g, buf, beta) (nesterov);
 *   X = bf16(u) (transposed if rows > cols);  X /= ||X||_F + 1e-7;
 *   5 x { A = X X^T;  B = b A + c A A;  X = a X + B X }   (a, b, c) = (3.4445, -4.7750, 2.0315);
 *   p = p (1 - lr wd) - lr sqrt(max(1, rows/cols)) X.
 * The three products per iteration are wft_gemm_nt_bf16 launches (beta = residual scale) batched over all
 * parameters of one shape; the functions below are the element-wise / layout steps around them.
 * Tables as above with n = n_mats same-shape [rows, cols] matrices (tab rows: 0 p, 1 g, 2 momentum).   */
/* Step 1: momentum + nesterov; g is overwritten with u (as grad.lerp_ does); U [n][rows][cols] = bf16(u);
 * partial [n][ceil(rows*cols / WFT_MT_CHUNK)] = per-chunk sum of bf16(u)^2.  sumsq/max_norm as above.
 * A zero entry in table row 1 is a parameter without a gradient this step: treated as an all-zero gradient (the package
 * materialises one: muon.py "force synchronization"), nothing is written back for it.   */
int wft_muon_momentum_mt(const void* tab, int n_mats, int64_t numel, float beta, int nesterov,
                         wft_bf16* U, float* partial, const float* sumsq, float max_norm, void* stream);
/* Step 2: normalise (norm rounded to bf16 like torch's bf16 .norm()) and lay out for the GEMMs:
 * X [n][rows_pad][cols_pad] with rows <= cols (U^T when the parameter is tall), Xt its transpose
 * [n][cols_pad][rows_pad]; pads are written as zeros.                                            */
int wft_muon_prepare(const wft_bf16* U, int rows, int cols, const float* partial, int chunks,
                     wft_bf16* X, wft_bf16* Xt, int rows_pad, int cols_pad, int n_mats, void* stream);
/* dst[b][c][r] = src[b][r][c] (keeps X and X^T in step between Newton-Schulz iterations).          */
int wft_transpose_bf16(const wft_bf16* src, int rows, int cols, wft_bf16* dst, int batch, void* stream);
/* Step 4: p = p (1 - lr wd) - lr * scale * O[t][r][c]; O bf16, row stride ldo, matrix stride stride_o. */
int wft_muon_apply_mt(const void* tab, int n_mats, int rows, int cols, const wft_bf16* O, int64_t ldo,
                      int64_t stride_o, float lr, float weight_decay, float scale, void* stream);

/* ------------------------------------------------------------ fp32 compute mode */
/* The reference runs TRUE fp32 when AMP is off (`training.mixed_precision_training: False`: autocast disabled at
 * model/model_utils.py:64, eval/evaluator.py:69), and the north star asks for parity within 1e-3 relative in that mode.
 * These entry points are that mode (csrc/f32.hip): fp32 tensors, v_mfma_f32_32x32x2_f32 products, fp32 everywhere else,
 * fixed summation orders.  It is the parity mode of the small configurations, not a throughput path.
 *
 * C[b][m, n] = alpha * sum_k A(b; m, k) * B(b; k, n) (+ beta * C[b][m, n]) (+ bias[n]);
 *   A(b; m, k) = A[b * a_bs + m * a_rs + k * a_cs],  B(b; k, n) = B[b * b_bs + k * b_rs + n * b_cs]  (element strides:
 *   NT / TN / NN products and the conv stem's overlapping-window rows — lda < K — are all stride choices);
 *   C row-major with row stride ldc.  Replaces F.linear / F.conv1d / the attention matmuls / the tied logits matmul of
 *   whisper.model in fp32 (model/model_utils.py:276-281,316-325).                                   */
typedef struct {
  const float* A; int64_t a_rs; int64_t a_cs; int64_t a_bs;
  const float* B; int64_t b_rs; int64_t b_cs; int64_t b_bs;
  float* C; int64_t ldc; int64_t c_bs;
  const float* bias;          /* f32 [N] or NULL */
  int64_t M; int64_t N; int64_t K; int batch;
  float alpha; float beta;
} wft_gemm_f32_args;
int wft_gemm_f32(const wft_gemm_f32_args* args, void* stream);
/* In place: row r of s [nrows, cols] (row stride ld) <- softmax(scale * s[r, :]); with causal != 0 the row belongs to
 * query r % rows_per_mat and columns beyond it are masked (the decoder's -inf upper-triangular mask buffer).
 * qkv_attention's softmax(qk.float()).                                                             */
int wft_softmax_fwd_f32(float* s, int64_t nrows, int64_t cols, int64_t ld, float scale, int causal,
                        int64_t rows_per_mat, void* stream);
/* dp <- scale * p * (dp - sum_c p[r, c] * dp[r, c])  (gradient w.r.t. the un-scaled scores). */
int wft_softmax_bwd_f32(const float* p, float* dp, int64_t nrows, int64_t cols, int64_t ld, float scale, void* stream);
/* whisper.model.LayerNorm in fp32 (+ the deep-SpecAugment mask, model/model_utils.py:409-417):
 * mask = int32 {rows_per_batch, t0, t1, c0, c1} in HOST memory or NULL.                                                 */
int wft_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                          int64_t rows, int cols, float eps, const int32_t* mask, void* stream);
int wft_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                          float* dx, float* dgamma, float* dbeta, int64_t rows, int cols, const int32_t* mask, void* stream);
int wft_gelu_fwd_f32(const float* x, float* y, int64_t n, void* stream);                 /* exact-erf GELU             */
int wft_gelu_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, void* stream);
int wft_axpby_f32(float a, const float* x, float b, const float* y, float* out, int64_t n, void* stream); /* y may be NULL */
int wft_colsum_f32(const float* x, int64_t rows, int64_t cols, int64_t ld, float* out, void* stream);     /* bias grads   */
/* out[b, s, :] = emb[tokens[b, s], :] + pos[s, :]  (model/model_utils.py:316-318); the backward needs demb zero-filled and
 * overwrites dpos[0..S).  Both kernels index emb / demb with the id as it is: every id must lie in [0, V) (there is no V
 * argument; unlike wft_embed_fwd / wft_embed_bwd nothing is clamped or skipped).  Sums in position / clip order, no atomics.   */
int wft_embed_fwd_f32(const int64_t* tokens, const float* emb, const float* pos, float* out, int64_t B, int64_t S, int d,
                      void* stream);
int wft_embed_bwd_f32(const int64_t* tokens, const float* dout, float* demb, float* dpos, int64_t B, int64_t S, int d,
                      void* stream);
/* F.cross_entropy(logits.transpose(1, 2), y_out, label_smoothing) on fp32 logits (model/model_utils.py:66): row losses,
 * row logsumexp, stats = {sum of row losses, number of non-ignored rows}; the backward overwrites the logits with
 * gscale / n_valid * (softmax - (1 - eps) onehot - eps / V).                                                            */
int wft_ce_fwd_f32(const float* logits, int64_t ld, const int64_t* targets, int64_t rows, int64_t V, float label_smoothing,
                   float* row_loss, float* row_lse, float* stats, void* stream);
int wft_ce_bwd_f32(float* logits, int64_t ld, const int64_t* targets, int64_t rows, int64_t V, float label_smoothing,
                   const float* row_lse, const float* stats, const float* gscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WFT_H */
