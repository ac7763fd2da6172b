/*
 * mmpt.h — C-ABI of the MI355X-native pre-training step library (libmmpt.so).
 *
 * The reference (tttyuntian/multimodal_llm_pretraining) has no native code and
 * no FFI: every op below replaces an ATen / DeepSpeed kernel that HF
 * transformers launches on the reference's behalf inside
 * `ManualTrainer.manual_training_step` / `manual_optimization_step`
 * (src/benchmarking/utils.py:61-80).  Each declaration cites the reference-side
 * interface it replaces.  `tf:` = transformers source.
 *
 * Conventions:
 *   - plain pointers + sizes, no torch types; all memory is caller-owned
 *     (PyTorch's caching allocator); the library never allocates on the hot path;
 *   - every call takes the caller's HIP stream as `void* stream` (hipStream_t);
 *   - return 0 on success, <0 for argument / unsupported errors, >0 = hipError_t;
 *     the message is in mmpt_last_error() (thread-local);
 *   - bf16 tensors are passed as `void*` (uint16 storage), fp32 as `float*`;
 *   - leading dimensions (`ld*`) are in elements.
 */
#ifndef MMPT_H_
#define MMPT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMPT_ABI_VERSION 16

enum mmpt_status { MMPT_OK = 0, MMPT_ERR_ARG = -1, MMPT_ERR_UNSUPPORTED = -2 };

int mmpt_abi_version(void);
const char* mmpt_last_error(void);
/* Number of compute units / clock of the current device (for roofline maths). */
int mmpt_device_info(int* cus, int* clock_khz, int* arch_gfx);
/* Test / measurement hook (ABI 9): kernel-variant switches are read ONCE from the
 * environment (MMPT_ATTN_PAIR: D = 256 dK/dV wave-pair kernel, MMPT_ATTN_DS: dQ through dS
 * tiles, MMPT_ATTN_NATIVE80: head_dim 80 computed over 80 dims; default 1 each; ABI 11:
 * MMPT_GEMM_KREV, gemm4p's odd tiles per workgroup walk K last-to-first, default 2 =
 * by shape; MMPT_GEMM_TAIL, the tail split, default 1; MMPT_GEMM_TAIL128 (round 6), tails of
 * <= 128 rows on the 128-row kernel, default 1; MMPT_GEMM_WTAIL (round 6), the weight-gradient
 * tail split, default 1 (2: tail tile columns only); MMPT_CE_REG, the register-resident
 * cross entropy, default 1); this overrides one for the rest of
 * the process.  value ∈ {0, 1} (2: KREV, WTAIL);
 * returns the previous value, MMPT_ERR_ARG for an unknown name. */
int mmpt_set_switch(const char* name, int value);

/* ------------------------------------------------------------------------
 * K1  nn.Linear → aten::addmm / mm (bf16 autocast).  tf:models/gpt_neox/
 * modeling_gpt_neox.py:38-49,176-177,190; tf:models/vit/modeling_vit.py:203-206,
 * 244-246; tf:models/llava/modeling_llava.py:92-100; lm_head :384.
 *
 * C[M,N] = op(A)[M,K] · op(B)[K,N], bf16 operands, fp32 accumulation.
 *   layout_a: MMPT_ROWS_K → A stored [M][K] (K contiguous, lda ≥ K)
 *             MMPT_K_ROWS → A stored [K][M] (M contiguous, lda ≥ M)
 *   layout_b: MMPT_ROWS_K → B stored [N][K] (K contiguous: nn.Linear weight)
 *             MMPT_K_ROWS → B stored [K][N] (N contiguous)
 * Forward Y = X·Wᵀ is (ROWS_K, ROWS_K); dX = dY·W is (ROWS_K, K_ROWS);
 * dW = dYᵀ·X is (K_ROWS, K_ROWS).
 * ---------------------------------------------------------------------- */
enum mmpt_layout { MMPT_ROWS_K = 0, MMPT_K_ROWS = 1 };
enum mmpt_epilogue {
  MMPT_EPI_BF16 = 0,       /* C(bf16) = bf16(acc + bias)                              */
  MMPT_EPI_BF16_GELU = 1,  /* C(bf16) = pre = bf16(acc + bias); C2(bf16) = bf16(gelu(pre)) */
  MMPT_EPI_BF16_DGELU = 2, /* C(bf16) = bf16(bf16(acc) * gelu'(aux))   [aux = pre, bf16] */
  MMPT_EPI_F32_ACC = 3,    /* C(f32) += f32(bf16(acc))   (weight-grad accumulation)     */
  MMPT_EPI_F32_STORE = 4,  /* C(f32)  = f32(bf16(acc))                                 */
  MMPT_EPI_F32_RESID = 5,  /* v = bf16(acc+bias); if aux: v = bf16(v + aux);
                              C(f32) = C2(f32 resid, may alias C) + v   (residual add)  */
  MMPT_EPI_BF16_DGELU_COLSUM = 6, /* as BF16_DGELU, plus per-tile column sums of the bf16
                              result into C2 (f32 [mmpt_gemm_colsum_rows][N]); finish with
                              mmpt_colsum_f32 -> the bias gradient of the layer whose
                              input gradient C is (fused addmm grad_bias)            */
  /* quick-GELU (x·sigmoid(1.702x), CLIP's hidden_act, tf:activations.py:70-123) forms of
     the three GELU epilogues, with autocast's bf16 roundings between its ops        */
  MMPT_EPI_BF16_QGELU = 7,
  MMPT_EPI_BF16_DQGELU = 8,
  MMPT_EPI_BF16_DQGELU_COLSUM = 9,
  /* SwiGLU MLP (LlamaMLP: down(silu(gate(x)) * up(x)), tf:models/llama/modeling_llama.py),
     with the fused gate|up projection stored BLOCKED: weight rows [256k, 256k+128) are
     gate rows f = 128k.., rows [256k+128, 256k+256) the up rows of the same features.
     SWIGLU (fwd, N = 2F, F % 128 == 0, no bias): C(bf16 [M][2F]) = the gate|up outputs in
     that blocked order; C2(bf16 [M][F]) = bf16(bf16(silu(gate)) * up).
     DSWIGLU (bwd, N = F): d = bf16(acc) is the act gradient; aux = the forward's C; writes
     C(bf16 [M][2F], blocked) = d gate, d up — autograd's bf16 mul / silu_backward. */
  MMPT_EPI_BF16_SWIGLU = 10,
  MMPT_EPI_BF16_DSWIGLU = 11,
  /* (ABI 12) weight + bias gradient in one pass: as F32_ACC, plus the sums over K of op(A)'s
     rows — Σ_k dY[k, m], addmm backward's grad_bias when A = dY (K_ROWS: [tokens][out]) — into
     C2 (f32 [mmpt_gemm_acc_colsum_rows][ldc2 ≥ M]: one partial row per K split and 256-column
     tile, each column summing its share of the K-tiles); finish with
     mmpt_colsum_f32(rows, M, C2, dbias, ...).  Both layouts K_ROWS, problems the big-tile
     kernel takes (mmpt_gemm_acc_colsum_rows > 0; since ABI 13 any K: token counts K % 64 != 0
     run the K-tail form); else MMPT_ERR_UNSUPPORTED. */
  MMPT_EPI_F32_ACC_COLSUM = 12
};
/* Rows of the column-sum partial buffer an EPI_BF16_DGELU_COLSUM call writes. */
int64_t mmpt_gemm_colsum_rows(int64_t M, int64_t N, int64_t K);
/* (ABI 12) Rows of the partial buffer an EPI_F32_ACC_COLSUM call writes (K splits x
 * ceil(N / 256), with a workspace of mmpt_gemm_workspace_bytes; rows a call with less workspace
 * leaves are zeroed),
 * or 0: the fused form does not take this problem (run F32_ACC + mmpt_colsum_bf16). */
int64_t mmpt_gemm_acc_colsum_rows(int64_t M, int64_t N, int64_t K);
/* Weight-gradient GEMMs (F32_ACC / F32_STORE) with K >> M·N are split along K into
 * fp32 slabs (workspace ≥ mmpt_gemm_workspace_bytes) summed in fixed order by a second
 * kernel — deterministic.  workspace may be NULL (then no split, same numerics). */
int64_t mmpt_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int epilogue);
int mmpt_gemm_bf16(int layout_a, int layout_b, int epilogue, int64_t M, int64_t N, int64_t K,
                   const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                   const void* bias_bf16, const void* aux_bf16, int64_t ld_aux, void* C2,
                   int64_t ldc2, void* workspace, int64_t workspace_bytes, void* stream);
/* Plan query (measurement / diagnostics): the tile edge (256 → the big-tile kernel,
 * gemm4p_kernel, when it takes the problem — else gemm128_kernel; 128 → gemm128_kernel) and
 * the split-K count that mmpt_gemm_bf16 would use for this problem given `workspace_bytes`. */
int mmpt_gemm_plan(int64_t M, int64_t N, int64_t K, int epilogue, int64_t workspace_bytes,
                   int* tile, int* splits);
/* The exact kernel (as rocprofv3 names it, without the namespace) of the main launch
 * mmpt_gemm_bf16 makes for this problem with `workspace_bytes` of workspace and 16-B aligned
 * operands: "gemm4p_kernel<LA, LB, E>" (4-wave pipelined, 256x256 tiles), its K-tail form
 * "gemm4p_kt_kernel<LA, LB, E>" (K % 64 != 0), or "gemm128_kernel<LA, LB, E>" (E = 100 / 102:
 * split-K slabs).  It is the name mmpt_gemm_last_kernel_name reports after such a call: both
 * read the same launch schedule (before, this query never answered gemm4p_kt_kernel, and named
 * the split launch where a weight-gradient tail split runs its main part unsplit).  (Round 5:
 * the 8-wave gemm256 kernel is retired.)  NUL-terminated into buf. */
int mmpt_gemm_kernel_name(int layout_a, int layout_b, int epilogue, int64_t M, int64_t N,
                          int64_t K, int64_t workspace_bytes, char* buf, int len);
/* (ABI 11) The kernel the calling thread's most recent mmpt_gemm_bf16 call launched (its
 * choice also depends on operand alignment, which mmpt_gemm_kernel_name assumes 16-B). */
int mmpt_gemm_last_kernel_name(char* buf, int len);
/* (ABI 11) Rows of the calling thread's most recent mmpt_gemm_bf16 call that ran as a "tail
 * split" (0: none): with the plain or residual epilogue on 256x256 tiles, the bottom tile rows
 * that would run as a partial last round of the persistent launch are computed as a split-K
 * GEMM over the caller's workspace (counted in mmpt_gemm_workspace_bytes) followed by an
 * epilogue kernel; MMPT_GEMM_TAIL=0 disables it.  The probe event (below) then marks the end of
 * the main launch, before the tail. */
int64_t mmpt_gemm_last_tail_rows(void);
/* Measurement hook (bench.py): the next mmpt_gemm_bf16 call on this thread records
 * `hip_event` (a hipEvent_t) on its stream right after the main GEMM kernel, before
 * the split-K reduce, so the main kernel can be timed alone.  One-shot. */
void mmpt_gemm_probe_event(void* hip_event);

/* Bias gradient: dbias[n] (+)= f32(bf16(Σ_rows dy[r, n]))  — addmm backward's
 * grad_bias (sum over rows) under autocast. Deterministic two-stage reduction.
 * dbias2 (nullable) receives the same value (two biases fed by one gradient, e.g.
 * GPTNeoX dense.bias and dense_4h_to_h.bias under the parallel residual).
 * `workspace` ≥ mmpt_colsum_workspace_bytes(rows, cols). */
int64_t mmpt_colsum_workspace_bytes(int64_t rows, int64_t cols);
/* dbias[n] (+)= f32(bf16(Σ_r part[r, n])) over an fp32 [rows][cols] partial-sum matrix
 * (e.g. the C2 output of EPI_BF16_DGELU_COLSUM); deterministic (fixed order). */
int mmpt_colsum_f32(int64_t rows, int64_t cols, const float* part, float* dbias, float* dbias2,
                    int accumulate, void* stream);
int mmpt_colsum_bf16(int64_t rows, int64_t cols, const void* dy, int64_t ld, float* dbias,
                     float* dbias2, int accumulate, void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * K4  nn.LayerNorm (fp32 under autocast), tf:modeling_gpt_neox.py:245-246
 * (two LNs on the same input: input_layernorm / post_attention_layernorm),
 * tf:modeling_vit.py:261-262,274,281.
 * y1 = bf16(LN(x; w1, b1)); optional y2 = bf16(LN(x; w2, b2)) sharing μ, rstd.
 * ---------------------------------------------------------------------- */
int mmpt_layernorm_fwd(int64_t rows, int64_t h, float eps, const float* x, int64_t ldx,
                       const float* w1, const float* b1, void* y1, const float* w2,
                       const float* b2, void* y2, float* mean, float* rstd, void* stream);
/* dx = dresid + LN'(dy1; w1) + LN'(dy2; w2)  (dresid / dy2 optional, dx may alias dresid);
 * dw*, db* accumulate (+=) into fp32 grads. `workspace` ≥ mmpt_layernorm_bwd_workspace_bytes. */
int64_t mmpt_layernorm_bwd_workspace_bytes(int64_t rows, int64_t h);
int mmpt_layernorm_bwd(int64_t rows, int64_t h, const float* x, int64_t ldx, const float* mean,
                       const float* rstd, const void* dy1, const float* w1, const void* dy2,
                       const float* w2, const float* dresid, float* dx, float* dw1, float* db1,
                       float* dw2, float* db2, void* workspace, void* stream);

/* Same backward with one workgroup per row (the fast path) and two optional fused
 * outputs: dx_bf16 (nullable) = bf16(dx), the operand of the next backward GEMMs
 * (replaces a separate cast); dsum (nullable, needs dx_bf16) += f32(bf16(Σ_rows
 * bf16(dx))) — the bias gradient autocast's addmm backward computes from that bf16
 * tensor (replaces a column sum); dsum2 (nullable) receives the same value.
 * `workspace` ≥ mmpt_layernorm_bwd_ex_workspace_bytes. */
int64_t mmpt_layernorm_bwd_ex_workspace_bytes(int64_t rows, int64_t h);
int mmpt_layernorm_bwd_ex(int64_t rows, int64_t h, const float* x, int64_t ldx, const float* mean,
                          const float* rstd, const void* dy1, const float* w1, const void* dy2,
                          const float* w2, const float* dresid, float* dx, void* dx_bf16,
                          float* dw1, float* db1, float* dw2, float* db2, float* dsum,
                          float* dsum2, void* workspace, void* stream);
/* fp32-output LayerNorm — CLIP's pre_layrnorm, whose output is the fp32 residual stream
 * (tf:models/clip/modeling_clip.py CLIPVisionTransformer.forward).  y, dy, dx fp32 [rows][h];
 * dw/db accumulate (+=); workspace = mmpt_layernorm_bwd_workspace_bytes(rows, h). */
int mmpt_layernorm_f32_fwd(int64_t rows, int64_t h, float eps, const float* x, const float* w,
                           const float* b, float* y, float* mean, float* rstd, void* stream);
int mmpt_layernorm_f32_bwd(int64_t rows, int64_t h, const float* x, const float* mean,
                           const float* rstd, const float* dy, const float* w, float* dx,
                           float* dw, float* db, void* workspace, void* stream);

/* RMSNorm (LlamaRMSNorm, tf:models/llama/modeling_llama.py, fp32 under autocast):
 * y = bf16(w · (x · rstd)), rstd = 1/sqrt(mean(x²) + eps).  Backward: dx = dresid +
 * RMS'(dy; w) (dresid optional, may alias dx), dw += Σ dy·x̂, optional dx_bf16 = bf16(dx);
 * deterministic two-stage dw reduction.  workspace ≥ mmpt_rmsnorm_bwd_workspace_bytes. */
int mmpt_rmsnorm_fwd(int64_t rows, int64_t h, float eps, const float* x, int64_t ldx,
                     const float* w, void* y, float* rstd, void* stream);
int64_t mmpt_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t h);
int mmpt_rmsnorm_bwd(int64_t rows, int64_t h, const float* x, int64_t ldx, const float* rstd,
                     const void* dy, const float* w, const float* dresid, float* dx,
                     void* dx_bf16, float* dw, void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * K6  partial rotary embedding, tf:modeling_gpt_neox.py:93-151 (rotate_half on the
 * first rot_dims of each head, fp32 cos/sin tables [seq][rot_dims]), applied in place
 * to the q and k parts of a fused qkv buffer.  inverse=1 applies the transpose
 * rotation (backward of the forward rotation).
 * qkv element (token t, head h, part p∈{q,k,v}, dim d) lives at
 *   qkv[t*ld + h*head_stride + p*part_stride + d]   (K7 layout, tf:...:204-207)
 * ---------------------------------------------------------------------- */
int mmpt_rope_inplace(int64_t tokens, int64_t seq, int64_t heads, int64_t head_dim,
                      int64_t rot_dims, void* qkv, int64_t ld, int64_t head_stride,
                      int64_t part_stride, int64_t parts, const float* cos, const float* sin,
                      int inverse, void* stream);
/* ABI 15: the same rotation with the table row of token t read from pos[t] (device int32,
 * 0 <= pos[t] < table_rows: the caller's contract) instead of t % seq — the positions of an
 * unpadded batch, where sequence b is rows [cu[b], cu[b+1]) and pos restarts at 0 in each.
 * The arithmetic is mmpt_rope_inplace's: with pos[t] = t % seq the results are bitwise equal. */
int mmpt_rope_inplace_pos(int64_t tokens, int64_t heads, int64_t head_dim, int64_t rot_dims,
                          void* qkv, int64_t ld, int64_t head_stride, int64_t part_stride,
                          int64_t parts, const float* cos, const float* sin, int64_t table_rows,
                          const int32_t* pos, int inverse, void* stream);

/* ------------------------------------------------------------------------
 * K2/K3  scaled-dot-product attention (torch SDPA, causal for GPTNeoX
 * tf:modeling_gpt_neox.py:214-229, non-causal for ViT tf:modeling_vit.py:221-232).
 * q/k/v are read in place from the fused qkv buffer (layout above);
 * out [tokens][heads*head_dim] bf16 (row stride ld_out), lse fp32 [batch*heads*seq].
 * ---------------------------------------------------------------------- */
int mmpt_attention_fwd(int64_t batch, int64_t seq, int64_t heads, int64_t head_dim,
                       const void* qkv, int64_t ld, int64_t head_stride, int64_t part_stride,
                       int causal, float scale, void* out, int64_t ld_out, float* lse,
                       void* stream);
/* dqkv has the same layout as qkv. `workspace` ≥ mmpt_attention_bwd_workspace_bytes. */
int64_t mmpt_attention_bwd_workspace_bytes(int64_t batch, int64_t seq, int64_t heads,
                                           int64_t head_dim);
int mmpt_attention_bwd(int64_t batch, int64_t seq, int64_t heads, int64_t head_dim,
                       const void* qkv, int64_t ld, int64_t head_stride, int64_t part_stride,
                       int causal, float scale, const void* out, const void* dout,
                       int64_t ld_out, const float* lse, void* dqkv, void* workspace,
                       void* stream);
/* K3 + K4 backward (ABI 10): mmpt_attention_bwd followed by the inverse rotation of the q and
 * k parts (= mmpt_rope_inplace(..., parts = 2, inverse = 1) on dqkv: the backward of
 * `apply_rotary_pos_emb`, tf:models/gpt_neox/modeling_gpt_neox.py:204-207).  head_dim 256 with
 * 64 rotary dims (Pythia) rotates inside the dK / dQ epilogues, bitwise the same as the two
 * calls; other shapes run them one after the other.  Same workspace as mmpt_attention_bwd. */
int mmpt_attention_bwd_rope(int64_t batch, int64_t seq, int64_t heads, int64_t head_dim,
                            const void* qkv, int64_t ld, int64_t head_stride, int64_t part_stride,
                            int causal, float scale, const void* out, const void* dout,
                            int64_t ld_out, const float* lse, void* dqkv, void* workspace,
                            int64_t rot_dims, const float* cos, const float* sin, void* stream);
/* K17  grouped-query attention (Llama-3: LlamaAttention + repeat_kv, tf:models/llama/
 * modeling_llama.py; SDPA with enable_gqa): query head h at qkv[t*ld + h*head_stride + d],
 * its kv head j = h / (heads / kv_heads) at qkv[t*ld + k_offset + j*head_stride + d] and
 * qkv[t*ld + v_offset + j*head_stride + d] (Llama's fused q|k|v projection: k_offset =
 * heads*head_dim, v_offset = k_offset + kv_heads*head_dim).  dqkv has the same layout; dK/dV
 * are summed over the query heads of the group inside one workgroup (no atomics).
 * mmpt_attention_fwd/bwd are the kv_heads = heads case (k_offset = part_stride,
 * v_offset = 2*part_stride). */
int mmpt_attention_gqa_fwd(int64_t batch, int64_t seq, int64_t heads, int64_t kv_heads,
                           int64_t head_dim, const void* qkv, int64_t ld, int64_t head_stride,
                           int64_t k_offset, int64_t v_offset, int causal, float scale, void* out,
                           int64_t ld_out, float* lse, void* stream);
int mmpt_attention_gqa_bwd(int64_t batch, int64_t seq, int64_t heads, int64_t kv_heads,
                           int64_t head_dim, const void* qkv, int64_t ld, int64_t head_stride,
                           int64_t k_offset, int64_t v_offset, int causal, float scale,
                           const void* out, const void* dout, int64_t ld_out, const float* lse,
                           void* dqkv, void* workspace, void* stream);
/* ABI 15  variable-length (unpadded) batches, the flash-attention varlen form: the token rows
 * of `batch` sequences are packed back to back, sequence b being rows [cu_seqlens[b],
 * cu_seqlens[b+1]) of qkv / out / dout / dqkv (total_tokens rows each).  cu_seqlens: device
 * int32 [batch + 1], ascending, cu[0] = 0, cu[batch] = total_tokens, every length in
 * [1, max_seq] — its contents are the caller's contract (the entry checks the pointer, max_seq
 * >= 1, batch <= total_tokens <= batch * max_seq and the 32-bit offset limits only).  Each
 * sequence is attended on its own, causal or not, and gets bitwise what mmpt_attention_gqa_fwd /
 * _bwd give for it alone (batch = 1, seq = its length).  lse is fp32 [batch][heads][max_seq];
 * entries past a sequence's length are left untouched, as is every row past total_tokens.
 * Layout arguments as mmpt_attention_gqa_*; every head dim of the dense path.  The backward
 * writes every q, k and v element of every dqkv row once (no atomics); at head_dim 256 it runs
 * the ring dK/dV and recomputing dQ kernels (what MMPT_ATTN_DS=0 selects for the dense entry),
 * so its workspace is δ only and the rope backward is a separate mmpt_rope_inplace_pos call. */
int mmpt_attention_varlen_fwd(int64_t batch, int64_t max_seq, int64_t total_tokens, int64_t heads,
                              int64_t kv_heads, int64_t head_dim, const void* qkv, int64_t ld,
                              int64_t head_stride, int64_t k_offset, int64_t v_offset, int causal,
                              float scale, const int32_t* cu_seqlens, void* out, int64_t ld_out,
                              float* lse, void* stream);
int64_t mmpt_attention_varlen_bwd_workspace_bytes(int64_t batch, int64_t max_seq, int64_t heads,
                                                  int64_t head_dim);
int mmpt_attention_varlen_bwd(int64_t batch, int64_t max_seq, int64_t total_tokens, int64_t heads,
                              int64_t kv_heads, int64_t head_dim, const void* qkv, int64_t ld,
                              int64_t head_stride, int64_t k_offset, int64_t v_offset, int causal,
                              float scale, const int32_t* cu_seqlens, const void* out,
                              const void* dout, int64_t ld_out, const float* lse, void* dqkv,
                              void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * K12  ForCausalLMLoss (tf:loss/loss_utils.py:32-68): fp32 upcast, CE with
 * ignore_index, reduction sum / num_items.  labels are ALREADY shifted (label of row r
 * is the target for logits row r).  Writes per-row loss (0 for ignored rows) and,
 * if dlogits != NULL, dlogits = (softmax - onehot) * grad_scale in bf16
 * (dlogits may alias logits: fused fwd+bwd, one read of the logits).
 * mmpt_cross_entropy_smooth adds TrainingArguments.label_smoothing_factor (HF Trainer's
 * LabelSmoother) in the same pass.
 * ---------------------------------------------------------------------- */
int mmpt_cross_entropy(int64_t rows, int64_t vocab, int64_t vocab_valid, const void* logits,
                       int64_t ld, const int64_t* labels, int64_t ignore_index, float grad_scale,
                       float* loss_rows, void* dlogits, int64_t ld_d, void* stream);
/* The same with label smoothing (F.cross_entropy(label_smoothing = eps); HF's LabelSmoother,
 * tf:trainer_pt_utils.py, which Trainer applies when label_smoothing_factor != 0).  With
 * V = vocab_valid, a scored row has
 *   loss = (1 - eps) (lse - x_y) + eps (lse - sum_{v<V} x_v / V),
 *   dlogits_v = grad_scale (softmax_v - (1 - eps) [v = y] - eps / V) for v < V, 0 past V;
 * an ignored row has loss 0 and gradient 0, a label outside [0, V) that is not ignore_index a
 * NaN loss row and a zero gradient (as in mmpt_cross_entropy).  sum x comes from the pass that computes the
 * softmax statistics: the same reads and writes as mmpt_cross_entropy.  label_smoothing must
 * be finite and in [0, 1) (else MMPT_ERR_ARG); exactly 0 runs mmpt_cross_entropy's kernels. */
int mmpt_cross_entropy_smooth(int64_t rows, int64_t vocab, int64_t vocab_valid, const void* logits,
                              int64_t ld, const int64_t* labels, int64_t ignore_index,
                              float grad_scale, float label_smoothing, float* loss_rows,
                              void* dlogits, int64_t ld_d, void* stream);
/* out[0] = Σ x[i] (deterministic).  workspace ≥ mmpt_sum_workspace_bytes(n). */
int64_t mmpt_sum_workspace_bytes(int64_t n);
int mmpt_sum_f32(int64_t n, const float* x, float* out, void* workspace, void* stream);

/* Loss-row compaction: the lm_head and the cross-entropy run only over rows whose
 * (shifted) label is not ignore_index (ForCausalLMLoss ignores the others: their logits are
 * never consumed and their gradient is exactly zero, so skipping them changes no result).
 * gather: dst[r] = src[idx[r]]; expand: dst[r] = map[r] >= 0 ? src[map[r]] : 0.  bf16 rows. */
int mmpt_gather_rows_bf16(int64_t rows, int64_t h, const int32_t* idx, const void* src,
                          int64_t ld_src, void* dst, int64_t ld_dst, void* stream);
int mmpt_expand_rows_bf16(int64_t rows, int64_t h, const int32_t* map, const void* src,
                          int64_t ld_src, void* dst, int64_t ld_dst, void* stream);

/* ------------------------------------------------------------------------
 * K8/K9  embedding gather + LLaVA image-token merge
 * (tf:modeling_gpt_neox.py:338; tf:models/llava/modeling_llava.py:243-248).
 * out[r] = img_map[r] >= 0 ? f32(img[img_map[r]]) : table[ids[r]]     (f32 rows)
 * bwd (aten::embedding_dense_backward, deterministic): the text rows sorted by id
 * (stable) form nseg segments; segment s covers perm[seg_off[s] .. seg_off[s+1]) and
 * dtable[seg_id[s]] += Σ (in position order, fp32) dout[perm[r]] — one writer per
 * table row, no atomics.  dimg[img_map[r]] = bf16(dout[r]) for image rows.  h % 8 == 0.
 * ---------------------------------------------------------------------- */
int mmpt_embed_fwd(int64_t rows, int64_t h, const int64_t* ids, const float* table,
                   const int32_t* img_map, const void* img, float* out, void* stream);
int mmpt_embed_bwd(int64_t rows, int64_t h, int64_t nseg, const int32_t* seg_id,
                   const int32_t* seg_off, const int32_t* perm, const int32_t* img_map,
                   const float* dout, float* dtable, void* dimg, void* stream);

/* K8 with NEFTune noise (TrainingArguments.neftune_noise_alpha; tf:integrations/neftune.py
 * neftune_post_forward_hook on the input embedding).  The noise rule (csrc/philox.h, host and
 * device): logical element e = r*h + col of noise site `site` takes word e % 4 of K16's
 * dropout_words(e / 4, site, seed);
 *   k = word >> 9 (23 bits),  s = (float)(2k + 1) * 2^-23 - 1   exact, in (-1, 1), never 0
 *   noise = fmul_rn(s, mag),  out = fadd_rn(value, noise)       two fp32 roundings, never an fma
 * mag = alpha / sqrt(S_in * h) computed in double and rounded once to fp32, S_in the width of
 * input_ids as the batch arrived (HF's output.size(1)); r is the kernel's own row.  Nothing is
 * stored: whoever needs the noise again (a backward that re-gathers, a recompute) draws it again.
 *   mmpt_embed_noise_fwd: mmpt_embed_fwd with the noise added to text rows in the same pass;
 *     rows with img_map[r] >= 0 receive f32(img[img_map[r]]) unchanged (masked_scatter
 *     overwrites them after the hook).  table / out 16-B aligned.
 *   mmpt_embed_noise: out[e] = noise of element e, fp32 dense [rows][h] (what mmpt_dropout_mask
 *     is to the masks).
 * h % 4 == 0, rows < 2^31, mag finite and >= 0, else MMPT_ERR_ARG before any launch.  Added
 * without a change of MMPT_ABI_VERSION: the entries are new, nothing existing changed. */
int mmpt_embed_noise_fwd(int64_t rows, int64_t h, const int64_t* ids, const float* table,
                         const int32_t* img_map, const void* img, float* out, float mag,
                         uint64_t seed, uint64_t site, void* stream);
int mmpt_embed_noise(int64_t rows, int64_t h, float mag, uint64_t seed, uint64_t site, float* out,
                     void* stream);

/* Device-side segment build for the embedding backward (ABI 8; replaces round 2's host
 * numpy argsort behind the same semantics): key[r] = ids[r] (rows with id == skip_id — the
 * LLaVA image slots, pass -1 for none — and out-of-range ids are excluded), stable counting
 * sort of (key, row) (hand-written LSD radix sort, linear in rows; ABI 9) → perm[0 .. text rows); segments as above with seg_id/seg_off sized [rows] / [rows+1]
 * and the segment count written to DEVICE memory *nseg; *bad = 1 iff some id lies outside
 * [0, vocab) and is not skip_id.  Workspace from mmpt_embed_segments_workspace_bytes (-1 on
 * bad sizes).  Replaces the CPU side of aten::embedding_dense_backward's index sort
 * (torch/nn/functional.py embedding → tf:modeling_gpt_neox.py:338 embed_in). */
int64_t mmpt_embed_segments_workspace_bytes(int64_t rows, int64_t vocab);
int mmpt_embed_segments(int64_t rows, const int64_t* ids, int64_t vocab, int64_t skip_id,
                        int32_t* seg_id, int32_t* seg_off, int32_t* perm, int32_t* nseg,
                        int32_t* bad, void* workspace, int64_t ws_bytes, void* stream);
/* mmpt_embed_bwd with the segment count read from device memory (grid sized by max_seg,
 * an upper bound such as the number of text rows). */
int mmpt_embed_bwd_dev(int64_t rows, int64_t h, int64_t max_seg, const int32_t* nseg,
                       const int32_t* seg_id, const int32_t* seg_off, const int32_t* perm,
                       const int32_t* img_map, const float* dout, float* dtable, void* dimg,
                       void* stream);

/* ABI 13: mmpt_embed_bwd_dev with segments longer than 1024 rows (one id padding most of a
 * batch, src/data/llava_data.py:95) split over 256-row chunks of the sorted order: each chunk
 * sums its piece of a long segment in position order, the pieces are added in chunk order
 * (deterministic; a different fp32 association than one serial loop for those segments only —
 * every segment of <= 1024 rows is summed bitwise as mmpt_embed_bwd_dev does).  max_seg <= rows
 * bounds the text rows; workspace from mmpt_embed_bwd_split_workspace_bytes(max_seg, h). */
int64_t mmpt_embed_bwd_split_workspace_bytes(int64_t rows, int64_t h);
int mmpt_embed_bwd_split(int64_t rows, int64_t h, int64_t max_seg, const int32_t* nseg,
                         const int32_t* seg_id, const int32_t* seg_off, const int32_t* perm,
                         const int32_t* img_map, const float* dout, float* dtable, void* dimg,
                         void* workspace, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * K10  ViT patch embedding (Conv2d k=s=patch, tf:modeling_vit.py:42-69) as
 * im2col (bf16, k-order = (c, ky, kx) = Conv2d weight flattening) + GEMM, then
 * CLS concat + position embedding (tf:modeling_vit.py:129-160).
 * ---------------------------------------------------------------------- */
int mmpt_im2col_patches(int64_t batch, int64_t channels, int64_t image, int64_t patch,
                        const float* pixels, void* cols, void* stream);
/* any patch size (CLIP-L/14: 14): cols [B·(S/p)²][ld_cols] bf16, ld_cols >= C·p·p, the
 * columns past C·p·p zero-filled (16-B GEMM rows; the patch weight carries zero columns). */
int mmpt_im2col_patches_ex(int64_t batch, int64_t channels, int64_t image, int64_t patch,
                           const float* pixels, void* cols, int64_t ld_cols, void* stream);
/* out[b, 0] = cls + pos[0];  out[b, 1+i] = f32(patch_out[b*np+i]) + pos[1+i]   (f32) */
int mmpt_vit_embed_fwd(int64_t batch, int64_t num_patches, int64_t h, const void* patch_out,
                       const float* cls, const float* pos, float* out, void* stream);
/* dcls += Σ_b dout[b,0]; dpos += Σ_b dout[b,:]; dpatch = bf16(dout[b, 1:]) */
int mmpt_vit_embed_bwd(int64_t batch, int64_t num_patches, int64_t h, const float* dout,
                       float* dcls, float* dpos, void* dpatch, void* stream);
/* LLaVA feature select (vision_feature_select_strategy="default": drop CLS,
 * tf:modeling_llava.py:163-166):  out[b*np+i] = bf16(x[b*(np+1)+1+i]). */
int mmpt_select_patches_fwd(int64_t batch, int64_t num_patches, int64_t h, const float* x,
                            void* out, void* stream);
/* dx[b*(np+1)+1+i] (+)= f32(dout[b*np+i]); dx[b*(np+1)] (+)= 0 */
int mmpt_select_patches_bwd(int64_t batch, int64_t num_patches, int64_t h, const void* dout,
                            float* dx, int accumulate, void* stream);

/* ------------------------------------------------------------------------
 * K13/K14  clip_grad_norm_ + Adam / AdamW step over one flat fp32 parameter
 * buffer (src/benchmarking/utils.py:66-76; torch.optim.Adam(W) single-tensor
 * semantics; DeepSpeed FusedAdam csrc/adam/multi_tensor_adam.cu).
 * Writes the bf16 shadow copy (autocast weight cast, K15) in the same pass.
 * ---------------------------------------------------------------------- */
int64_t mmpt_l2norm_workspace_bytes(int64_t n);
/* out[0] = Σ x[i]^2 (fp32, deterministic) */
int mmpt_sumsq_f32(int64_t n, const float* x, float* out, void* workspace, void* stream);
/* grad_scale_ptr (device, nullable): multiply g by *grad_scale_ptr (clip coefficient). */
int mmpt_adam_step(int64_t n, float* param, const float* grad, float* exp_avg,
                   float* exp_avg_sq, void* param_bf16, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int adamw, int64_t step,
                   const float* grad_scale_ptr, void* stream);
/* ABI 13: the same update, and the gradient zeroed as it is consumed (zero_grad fused: the
 * step's last read of g and the next step's zero are one pass; the optimizer overlapped with
 * the next forward runs it per parameter unit on its own stream).  16-B aligned buffers.
 * max_blocks > 0 caps the grid (256-thread workgroups, grid-stride): the overlapped update
 * runs one workgroup per CU beside the forward's persistent GEMMs. */
int mmpt_adam_step_zero_grad(int64_t n, float* param, float* grad, float* exp_avg,
                             float* exp_avg_sq, void* param_bf16, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int adamw, int64_t step,
                             const float* grad_scale, int max_blocks, void* stream);
/* clip coefficient from Σg²: coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) (device scalar) */
int mmpt_clip_coef(const float* sumsq, float max_norm, float* coef, void* stream);

/* elementwise helpers */
int mmpt_cast_f32_bf16(int64_t n, const float* src, void* dst, void* stream);
/* dst[c][r] = src[r][c] (bf16): the transposed weight shadow W^T that lets every
 * input-gradient GEMM dX = dY·W read both operands K-contiguous (refreshed once per
 * optimizer step, after the Adam kernel wrote the bf16 shadow). */
int mmpt_transpose_bf16(int64_t rows, int64_t cols, const void* src, int64_t ld_src, void* dst,
                        int64_t ld_dst, void* stream);
/* ABI 14: every W^T of a parameter store in one launch.  desc: DEVICE int64 [n][4] =
 * {offset, rows, cols, first_tile} per weight — src + offset holds [rows][cols] (dense),
 * dst + offset receives [cols][rows]; first_tile = the sum of ceil(rows/64)·ceil(cols/64)
 * over the weights before it, total_tiles the sum over all.  rows, cols, offsets multiples
 * of 8; the same bits as mmpt_transpose_bf16 per weight. */
int mmpt_transpose_bf16_batched(int64_t n, const int64_t* desc, int64_t total_tiles,
                                const void* src, void* dst, void* stream);


/* ------------------------------------------------------------------------
 * K16 (ABI 16)  hidden dropout: nn.Dropout at GPTNeoX's emb_dropout / post_attention_dropout /
 * post_mlp_dropout (tf:models/gpt_neox/modeling_gpt_neox.py) and at ViTEmbeddings.dropout /
 * ViTSelfOutput.dropout / ViTOutput.dropout (tf:models/vit/modeling_vit.py) in training mode.
 * The masks are never stored.  Logical element e = row*h + col (64-bit, independent of any
 * leading dimension) of dropout site `site` draws output word e % 4 of Philox4x32-10 with
 *   key = (lo32(seed), hi32(seed)),  counter = (lo32(e/4), hi32(e/4), lo32(site), hi32(site))
 * and is kept iff word >= floor(p * 2^32) (host arithmetic in double); kept elements are
 * multiplied by scale = float(1 / (1 - p)), dropped ones become +0.  The same (seed, site)
 * gives the same mask in every entry, so the backward is the forward's map on the gradient and
 * a recomputed forward repeats it.  0 <= p < 1, h % 8 == 0, 16-B aligned pointers, leading
 * dimensions multiples of 8 and >= h; else MMPT_ERR_ARG.
 * ---------------------------------------------------------------------- */
/* dst = keep ? bf16(f32(src) * scale) : +0  (one rounding: ATen's fused-dropout arithmetic).
 * dst may alias src (same leading dimension).  Forward and backward. */
int mmpt_dropout_bf16(int64_t rows, int64_t h, const void* src, int64_t ld_src, void* dst,
                      int64_t ld_dst, double p, uint64_t seed, uint64_t site, void* stream);
/* The same on dense fp32 [rows][h] (the embedding outputs, fp32 under autocast). */
int mmpt_dropout_f32(int64_t rows, int64_t h, const float* src, float* dst, double p,
                     uint64_t seed, uint64_t site, void* stream);
/* The forward's residual add in one pass: out = resid + f32(v), v = drop(y; site_y) when y2 is
 * NULL, else v = bf16(drop(y2; site_y2) + drop(y; site_y)) (GPTNeoX's parallel residual) — the
 * rounding order of MMPT_EPI_F32_RESID.  y, y2 bf16; resid, out dense fp32 [rows][h]; out may
 * alias resid. */
int mmpt_dropout_add_f32(int64_t rows, int64_t h, const void* y, int64_t ld_y, uint64_t site_y,
                         const void* y2, int64_t ld_y2, uint64_t site_y2, const float* resid,
                         float* out, double p, uint64_t seed, void* stream);
/* Test / diagnostic hook: keep[e] = 1 or 0 for the elements e = 0 .. n-1 of a site. */
int mmpt_dropout_mask(int64_t n, double p, uint64_t seed, uint64_t site, uint8_t* keep,
                      void* stream);

/* ------------------------------------------------------------------------
 * K19  attention-probability dropout: nn.Dropout on the softmax output (GPTNeoX / Llama / CLIP
 * `attention_dropout`, ViT `attention_probs_dropout_prob`; SDPA's dropout_p) inside the
 * flash-attention kernels.  The masks are never stored.  The keep bit is a pure function of
 * (seed, site, batch index b, QUERY head h, query position q, key position k) — positions inside
 * their sequence, b the index in cu_seqlens for a packed call — and of nothing else: not the
 * kernel, tile shape or head dim, not dense vs varlen, not the GQA grouping.  One Philox4x32-10
 * call covers a block of 4 queries x 4 keys:
 *   W    = philox4x32_10(ctr = {(q>>2) | ((k>>2) << 16), b*heads + h, lo32(site), hi32(site)},
 *                        key = {lo32(seed), hi32(seed)})
 *   byte = (W.w[q & 3] >> (8 * (k & 3))) & 0xFF
 *   keep iff byte >= t8,  t8 = floor(p * 256)  (host arithmetic in double)
 * p is thereby quantised: p_eff = t8 / 256 (mmpt_attn_dropout_p_eff), and kept probabilities are
 * multiplied by s = float(1 / (1 - p_eff)).  t8 == 0 (p < 1/256) is the p = 0 path: the drop
 * entries then run the kernels and write the bits of the plain entries.  A site must be one that
 * no hidden-dropout (K16) call of the same seed uses: both share the Philox key.
 * Arithmetic and rounding order (P = the undropped softmax, lse its log-sum-exp, unchanged):
 *   forward   O = bf16(acc * ((1 / l) * s)), acc = Σ_k bf16(keep ? P~ : 0) · V in fp32, P~ and the
 *             row sum l as in the plain kernel (the dropped P is zeroed before the bf16 pack, s is
 *             folded into the fp32 epilogue);
 *   dV        = bf16(s * Σ_q bf16(keep ? P : 0) · dO)  (s in the fp32 epilogue);
 *   dS        = bf16(P * ((keep ? dP * s : 0) - δ)) with dP, δ = rowsum(dO∘O) in fp32; dQ and dK
 *             from dS as in the plain kernels.
 * 0 <= p < 1 else MMPT_ERR_ARG; p >= 1/256 with max_seq > 262144 is MMPT_ERR_UNSUPPORTED (the
 * block indices are 16 bits each).  Added without a change of MMPT_ABI_VERSION: the entries are
 * new, nothing existing changed.
 * ---------------------------------------------------------------------- */
/* Arguments of mmpt_attention_varlen_fwd / _bwd, then p, seed, site.  cu_seqlens == NULL is the
 * dense call: max_seq is seq and total_tokens must be batch * seq (lse [batch][heads][seq]).
 * Every head dim of the dense path, causal or not, GQA.  With dropout on the backward runs the
 * ring dK/dV and recomputing dQ kernels at every head dim (head_dim 256 too) and fuses no rope
 * backward: run mmpt_rope_inplace(_pos) on dqkv afterwards. */
int mmpt_attention_drop_fwd(int64_t batch, int64_t max_seq, int64_t total_tokens, int64_t heads,
                            int64_t kv_heads, int64_t head_dim, const void* qkv, int64_t ld,
                            int64_t head_stride, int64_t k_offset, int64_t v_offset, int causal,
                            float scale, const int32_t* cu_seqlens, void* out, int64_t ld_out,
                            float* lse, double p, uint64_t seed, uint64_t site, void* stream);
/* δ only when dropout is on (t8 > 0); else what the plain dense (varlen = 0) or varlen entry
 * asks for. */
int64_t mmpt_attention_drop_bwd_workspace_bytes(int64_t batch, int64_t max_seq, int64_t heads,
                                                int64_t head_dim, int varlen, double p);
int mmpt_attention_drop_bwd(int64_t batch, int64_t max_seq, int64_t total_tokens, int64_t heads,
                            int64_t kv_heads, int64_t head_dim, const void* qkv, int64_t ld,
                            int64_t head_stride, int64_t k_offset, int64_t v_offset, int causal,
                            float scale, const int32_t* cu_seqlens, const void* out,
                            const void* dout, int64_t ld_out, const float* lse, void* dqkv,
                            void* workspace, double p, uint64_t seed, uint64_t site, void* stream);
/* Test / diagnostic hook: keep [batch][heads][seq_q][seq_k] = 1 or 0. */
int mmpt_attn_dropout_mask(int64_t batch, int64_t heads, int64_t seq_q, int64_t seq_k, double p,
                           uint64_t seed, uint64_t site, uint8_t* keep, void* stream);
double mmpt_attn_dropout_p_eff(double p);

/* ------------------------------------------------------------------------
 * K18  classification head: ViTForImageClassification (tf:models/vit/modeling_vit.py,
 * ViTModel(add_pooling_layer=False).layernorm then `classifier(sequence_output[:, 0, :])`).
 * HF runs vit.layernorm (fp32 under autocast) over every token and reads only the CLS row; these
 * entries compute that row alone.  The classifier itself is K1 (bias epilogue) and the loss the
 * cross entropy with `vocab_valid` = the label count (the head padded to a multiple of 8 rows).
 * Added without a change of MMPT_ABI_VERSION: the entries are new, nothing existing changed.
 * h % 8 == 0 (and h <= 4096), 16-B aligned pointers, leading dimensions multiples of 8 and
 * >= h, batch * tokens < 2^31; else MMPT_ERR_ARG.
 * ---------------------------------------------------------------------- */
/* y[b] = bf16(LN(x[b*tokens]; w, b)) for the CLS row of each of `batch` samples;
 * x fp32 dense [batch*tokens][h]; y bf16 [batch][ld_y]; mean, rstd fp32 [batch].  The bits of
 * mmpt_layernorm_fwd on a dense copy of those rows. */
int mmpt_cls_ln_fwd(int64_t batch, int64_t tokens, int64_t h, float eps, const float* x,
                    const float* w, const float* b, void* y, int64_t ld_y, float* mean,
                    float* rstd, void* stream);
int64_t mmpt_cls_ln_bwd_workspace_bytes(int64_t batch, int64_t h);
/* One pass writes EVERY row of dx (fp32 dense [batch*tokens][h]) and, if non-NULL, of dx_bf16
 * (bf16, same shape): row b*tokens = LN'(dy[b]; w), every other row +0 (the gradient of the
 * residual stream is non-zero on the CLS rows only) — no memset, scatter or cast beside it.
 * dy bf16 [batch][ld_dy].  dw, db (nullable) accumulate (+=).  dsum (nullable, needs dx_bf16) +=
 * f32(bf16(Σ_b bf16(dx[b*tokens]))): the top encoder layer's output-bias gradient.  Fixed-order
 * reductions, no atomics: the CLS rows, dw, db and dsum carry the bits of
 * mmpt_layernorm_bwd_ex(rows = batch) on a dense copy of the CLS rows.
 * `workspace` >= mmpt_cls_ln_bwd_workspace_bytes. */
int mmpt_cls_ln_bwd(int64_t batch, int64_t tokens, int64_t h, const float* x, const float* mean,
                    const float* rstd, const void* dy, int64_t ld_dy, const float* w, float* dx,
                    void* dx_bf16, float* dw, float* db, float* dsum, void* workspace,
                    void* stream);

/* ------------------------------------------------------------------------
 * K20  post-LN encoder (RoBERTa, tf:models/roberta/modeling_roberta.py): LayerNorm AFTER the
 * residual add, where every other model here normalises before its GEMMs.  fp32 statistics and
 * outputs (autocast runs aten::layer_norm in fp32), one pass per sub-layer where composing
 * mmpt_dropout_add_f32 + mmpt_layernorm_f32_fwd + mmpt_cast_f32_bf16 takes three.  The dropout
 * masks are K16's: element row*h + col of `site`, same keep rule and scale, so
 * mmpt_dropout_mask(site) describes them; p = 0 draws nothing.  Reductions over rows (dw, db,
 * dsum, dtype) are per-workgroup partials summed in a fixed order by a second kernel: no
 * atomics, bitwise reproducible.  Added without a change of MMPT_ABI_VERSION: the entries are
 * new, nothing existing changed.
 * rows in [1, 2^31), h % 8 == 0 and h <= 4096, 16-B aligned pointers, leading dimensions
 * multiples of 8 and >= h, 0 <= p < 1; else MMPT_ERR_ARG (nothing is launched).
 * ---------------------------------------------------------------------- */
/* RobertaSelfOutput / RobertaOutput.forward: `LayerNorm(dropout(dense(x)) + input_tensor)`.
 *   s   = resid + f32(drop(v; p, seed, site))   v bf16 [rows][ld_v]: bf16(f32(v) * scale) or +0
 *                                               (one rounding, mmpt_dropout_bf16), one fp32 add
 *   y32 = LN(s; w, b, eps)                      fp32; the row arithmetic of
 *                                               mmpt_layernorm_f32_fwd: the same bits on the same s
 *   y16 = bf16(y32)                             the next GEMM's operand
 * resid, s, y32 dense fp32 [rows][h]; s may alias resid; y16 bf16 [rows][ld_y16]; mean, rstd
 * fp32 [rows]. */
int mmpt_add_layernorm_fwd(int64_t rows, int64_t h, float eps, const float* resid, const void* v,
                           int64_t ld_v, const float* w, const float* b, float* s, float* y32,
                           void* y16, int64_t ld_y16, float* mean, float* rstd, double p,
                           uint64_t seed, uint64_t site, void* stream);
int64_t mmpt_add_layernorm_bwd_workspace_bytes(int64_t rows, int64_t h);
/* Its backward, as autograd under autocast produces it.  The gradient of the LayerNorm's output
 *   dy   = dy32 + f32(dyb)     dy32 (fp32 dense, nullable): from the next residual add; dyb (bf16
 *                              [rows][ld_dyb], nullable): the input gradient of the GEMM that
 *                              read bf16(y); at least one of the two, one fp32 add when both
 *   ds32 = LN'(dy; s, mean, rstd, w)            fp32, goes on down the residual; may alias dy32
 *   dvb  = drop(bf16(ds32); p, seed, site)      bf16 [rows][ld_dvb]: the branch Linear's output
 *                                               gradient, two roundings as ATen's
 *   dw  += Σ_rows dy · x̂,  db += Σ_rows dy      fp32 (nullable)
 *   dsum (and dsum2) += f32(bf16(Σ_rows f32(dvb)))   (nullable; dsum2 needs dsum): the branch
 *                              Linear's bias gradient, fp32 sum of the masked bf16 tensor rounded
 *                              to bf16 once (mmpt_layernorm_bwd_ex's dsum convention)
 * workspace >= mmpt_add_layernorm_bwd_workspace_bytes. */
int mmpt_add_layernorm_bwd(int64_t rows, int64_t h, const float* s, const float* mean,
                           const float* rstd, const float* w, const float* dy32, const void* dyb,
                           int64_t ld_dyb, float* ds32, void* dvb, int64_t ld_dvb, float* dw,
                           float* db, float* dsum, float* dsum2, double p, uint64_t seed,
                           uint64_t site, void* workspace, void* stream);
/* RobertaEmbeddings.forward: gather, sum, LayerNorm and dropout in one pass.
 *   e   = (word[ids[r]] + type_row) + pos_table[pos[r]]   fp32, HF's order (inputs_embeds +
 *                              token_type_embeddings, then + position_embeddings); type_row is
 *                              token_type_embeddings row 0 (type_vocab_size 1)
 *   y   = LN(e; w, b, eps)     fp32, the row arithmetic of mmpt_layernorm_f32_fwd
 *   h32 = drop(y; p, seed, site)   fp32: y * scale or +0 (mmpt_dropout_f32)
 *   h16 = bf16(h32)
 * e is not kept: the backward gathers it again.  ids int64 [rows] in [0, vocab), pos int64
 * [rows] in [0, max_pos) (ids outside are clamped: validate on the host); h32 fp32, h16 bf16,
 * both dense [rows][h]. */
int mmpt_roberta_embed_fwd(int64_t rows, int64_t h, float eps, const int64_t* ids,
                           const int64_t* pos, const float* word, int64_t vocab,
                           const float* pos_table, int64_t max_pos, const float* type_row,
                           const float* w, const float* b, float* h32, void* h16, float* mean,
                           float* rstd, double p, uint64_t seed, uint64_t site, void* stream);
int64_t mmpt_roberta_embed_bwd_workspace_bytes(int64_t rows, int64_t h);
/*   dy   = drop(dh + f32(dhb); p, seed, site)   fp32 (the forward's map on the gradient); dh fp32
 *                              dense: from the first residual add; dhb (bf16 dense, nullable):
 *                              the input gradient of the GEMM that read h16
 *   de   = LN'(dy; e, mean, rstd, w)            fp32 dense, may alias dh; e gathered again
 *   dw  += Σ_rows dy · x̂,  db += Σ_rows dy,  dtype += Σ_rows de   fp32, no bf16 rounding: the
 *                              embedding tables sit outside autocast (all nullable)
 * de then goes to the word and the position table through mmpt_embed_segments /
 * mmpt_embed_bwd_split keyed by ids and by pos (skip_id = padding_idx). */
int mmpt_roberta_embed_bwd(int64_t rows, int64_t h, const int64_t* ids, const int64_t* pos,
                           const float* word, int64_t vocab, const float* pos_table,
                           int64_t max_pos, const float* type_row, const float* mean,
                           const float* rstd, const float* w, const float* dh, const void* dhb,
                           float* de, float* dw, float* db, float* dtype, double p, uint64_t seed,
                           uint64_t site, void* workspace, void* stream);
/* The two entries above with NEFTune noise (K8's rule under noise_seed / noise_site) on
 * the word row, HF's order since the hook sits on word_embeddings:
 *   e = ((word[ids[r]] + noise) + type_row) + pos_table[pos[r]]
 * The backward gathers e again and draws the same noise, so dw, db, dtype and de see the
 * forward's x̂.  Everything else is the entries above, kernel body shared; mag = 0 gives their
 * bits.  mag finite and >= 0.  Added without a change of MMPT_ABI_VERSION. */
int mmpt_roberta_embed_noise_fwd(int64_t rows, int64_t h, float eps, const int64_t* ids,
                                 const int64_t* pos, const float* word, int64_t vocab,
                                 const float* pos_table, int64_t max_pos, const float* type_row,
                                 const float* w, const float* b, float* h32, void* h16,
                                 float* mean, float* rstd, double p, uint64_t seed, uint64_t site,
                                 float mag, uint64_t noise_seed, uint64_t noise_site,
                                 void* stream);
int mmpt_roberta_embed_noise_bwd(int64_t rows, int64_t h, const int64_t* ids, const int64_t* pos,
                                 const float* word, int64_t vocab, const float* pos_table,
                                 int64_t max_pos, const float* type_row, const float* mean,
                                 const float* rstd, const float* w, const float* dh,
                                 const void* dhb, float* de, float* dw, float* db, float* dtype,
                                 double p, uint64_t seed, uint64_t site, float mag,
                                 uint64_t noise_seed, uint64_t noise_site, void* workspace,
                                 void* stream);
/* RobertaLMHead.layer_norm, which reads the bf16 GELU output g [rows][ld_g]:
 *   n16 = bf16(LN(f32(g); w, b, eps))           bf16 [rows][ld_n16]: the decoder's operand
 * (the statistics within an fp32 ulp of mmpt_layernorm_f32_fwd's on f32(g), not its bits) */
int mmpt_mlm_ln_fwd(int64_t rows, int64_t h, float eps, const void* g, int64_t ld_g,
                    const float* w, const float* b, void* n16, int64_t ld_n16, float* mean,
                    float* rstd, void* stream);
int64_t mmpt_mlm_ln_bwd_workspace_bytes(int64_t rows, int64_t h);
/*   dg   = bf16(LN'(f32(dn16); f32(g), mean, rstd, w))     the LayerNorm's bf16 input gradient
 *   dpre = bf16(dg · gelu'(pre))                bf16 [rows][ld_dpre]: the head dense's output
 *                                               gradient (MMPT_EPI_BF16_DGELU's arithmetic;
 *                                               pre = the dense's bf16 pre-activation)
 *   dw  += Σ_rows dn · x̂,  db += Σ_rows dn      fp32 (nullable)
 *   dsum += f32(bf16(Σ_rows f32(dpre)))         the head dense's bias gradient (nullable) */
int mmpt_mlm_ln_bwd(int64_t rows, int64_t h, const void* g, int64_t ld_g, const float* mean,
                    const float* rstd, const float* w, const void* dn16, int64_t ld_dn16,
                    const void* pre, int64_t ld_pre, void* dpre, int64_t ld_dpre, float* dw,
                    float* db, float* dsum, void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * K21  ConvNeXt (tf:models/convnext/modeling_convnext.py): the 7x7 depthwise convolution of
 * ConvNextLayer (forward, input gradient, weight gradient), the layer-scale residual, the global
 * average pool and the 2x2/s2 patch permutations that make ConvNextStage's downsample conv a
 * GEMM.  Activations are NHWC: rows (b, y, x), columns c; H and W are separate arguments.
 * Depthwise weights are tap-major [49][C], tap = ky*7 + kx (HF's [C][1][7][7] transposed), padding
 * 3 with zeros outside the image — taps outside are predicated, never loaded.  Arithmetic is what
 * autocast(bf16) produces: bf16 operands, fp32 accumulation, one bf16 rounding of a conv result;
 * the fp32 residual stream and gamma stay fp32.  Reductions over rows are per-workgroup partials
 * summed in a fixed order by a second kernel: no atomics, bitwise reproducible.  Added without a
 * change of MMPT_ABI_VERSION: the entries are new, nothing existing changed.
 * C % 8 == 0 and C <= 4096, B, H, W >= 1 (planes smaller than the filter included) with
 * B*H*W < 2^31 (rows < 2^31), 16-B aligned pointers, leading dimensions multiples of 8 and >= C;
 * else MMPT_ERR_ARG (nothing is launched).
 * ---------------------------------------------------------------------- */
/* c = bf16(Σ_taps bf16(x)[b, y+ky-3, x+kx-3, ch] * w[tap][ch] + bias[ch]), fp32 accumulation over
 * the in-image taps.  x fp32 [B][H][W][C] (rounded to bf16 on the way in), w bf16 [49][C], bias
 * bf16 [C], c bf16 [B][H][W][C]. */
int mmpt_dwconv7_fwd(int64_t B, int64_t H, int64_t W, int64_t C, const float* x, const void* w,
                     const void* bias, void* c, void* stream);
/* dx_out = dx_in + f32(bf16(Σ_taps dc[b, y-ky+3, x-kx+3, ch] * w[tap][ch])).  dc bf16, dx_in fp32
 * (NULL: taken as zero; may alias dx_out), dx_out fp32, all [B][H][W][C]. */
int mmpt_dwconv7_bwd_input(int64_t B, int64_t H, int64_t W, int64_t C, const void* dc,
                           const void* w, const float* dx_in, float* dx_out, void* stream);
int64_t mmpt_dwconv7_bwd_weight_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C);
/* dw[tap][ch] += f32(bf16(Σ_{b,y,x} dc[b,y,x,ch] * bf16(x)[b, y+ky-3, x+kx-3, ch])),
 * db[ch] += f32(bf16(Σ_{b,y,x} dc[b,y,x,ch])): fp32 sums, one bf16 rounding, then += into the
 * fp32 gradients (the MMPT_EPI_F32_ACC convention).  dw fp32 [49][C], db fp32 [C]. */
int mmpt_dwconv7_bwd_weight(int64_t B, int64_t H, int64_t W, int64_t C, const float* x,
                            const void* dc, float* dw, float* db, void* workspace, void* stream);
/* ConvNextLayer's residual: out = resid + gamma * f32(y), the product and the sum each rounded to
 * fp32 (two roundings, as torch's mul then add).  resid, out fp32 dense [rows][C] (out may alias
 * resid); gamma fp32 [C]; y bf16 [rows][ld_y]. */
int mmpt_layerscale_add_fwd(int64_t rows, int64_t C, const float* resid, const float* gamma,
                            const void* y, int64_t ld_y, float* out, void* stream);
int64_t mmpt_layerscale_bwd_workspace_bytes(int64_t rows, int64_t C);
/* dy = bf16(gamma * g) (bf16 [rows][ld_dy]); dgamma[c] += Σ_rows g * f32(y) in fp32 (gamma is an
 * fp32 parameter outside autocast: no bf16 rounding).  g fp32 dense [rows][C]. */
int mmpt_layerscale_bwd(int64_t rows, int64_t C, const float* g, const float* gamma,
                        const void* y, int64_t ld_y, void* dy, int64_t ld_dy, float* dgamma,
                        void* workspace, void* stream);
int64_t mmpt_ln16_bwd_workspace_bytes(int64_t rows, int64_t h);
/* The backward of mmpt_mlm_ln_fwd (a LayerNorm that reads a bf16 activation c and feeds a GEMM):
 *   dc  = bf16(LN'(f32(dn16); f32(c), mean, rstd, w))   bf16 [rows][ld_dc]
 *   dw += Σ_rows dn · x̂,  db += Σ_rows dn               fp32 (nullable)
 * mmpt_mlm_ln_bwd without the dGELU and dsum. */
int mmpt_ln16_bwd(int64_t rows, int64_t h, const void* c, int64_t ld_c, const float* mean,
                  const float* rstd, const float* w, const void* dn16, int64_t ld_dn16, void* dc,
                  int64_t ld_dc, float* dw, float* db, void* workspace, void* stream);
/* p[b][c] = (Σ_hw x[b][hw][c]) / HW in fp32; x fp32 [B][HW][C], p fp32 [B][C]; B <= 65535.  Here
 * and in the backward the division is torch's device arithmetic for a division by a scalar: one
 * multiplication by the fp32 reciprocal float(1) / float(HW). */
int mmpt_avgpool_fwd(int64_t B, int64_t HW, int64_t C, const float* x, float* p, void* stream);
/* dx[b][hw][c] = dp[b][c] / HW: every row of dx is written, no memset beside it. */
int mmpt_avgpool_bwd(int64_t B, int64_t HW, int64_t C, const float* dp, float* dx, void* stream);
/* The 2x2/s2 downsample conv as a GEMM: rows[(b, oy, ox)][(ky*2 + kx)*C + c] =
 * x[b][2 oy + ky][2 ox + kx][c]; x bf16 [B][H][W][C] (H, W even), rows bf16 [B*H/2*W/2][4C]. */
int mmpt_patchify2_nhwc(int64_t B, int64_t H, int64_t W, int64_t C, const void* x, void* rows,
                        void* stream);
/* The inverse permutation, widened to fp32 (exact): dx fp32 [B][H][W][C] from bf16 rows. */
int mmpt_unpatchify2_nhwc(int64_t B, int64_t H, int64_t W, int64_t C, const void* rows, float* dx,
                          void* stream);

/* ------------------------------------------------------------------------
 * K21 stochastic depth (ConvNextDropPath, ConvNextConfig.drop_path_rate): in training, sample b of
 * a block with drop probability p is either kept, out_b = x_b + (gamma * y_b) / keep_prob, or
 * dropped, out_b = x_b.  A dropped sample's branch contributes nothing to the output or to any
 * gradient, so the block runs over its Bk kept samples only: the bf16 side of every kernel is
 * compact [Bk][...], the fp32 residual stream stays dense [B][...] and is addressed through
 *   idx  int32 [Bk], device memory, strictly increasing, idx[b'] in [0, B): the plane of compact
 *        sample b' in the stream;
 *   slot int32 [B], device memory: the compact index of plane b, or -1 where it is dropped.
 * The keep bits are K16's: sample b is element b of a dropout site, kept iff its Philox word >=
 * floor(p * 2^32), so mmpt_dropout_mask(n = B, p, seed, site) describes them; the caller decides
 * on the host (the rule is a pure function of p, seed, site) and passes idx / slot.
 * Roundings, with s = float(1 / (1 - p)) (philox.h dropout_scale: one fp32 factor; a device
 * division by a scalar is that multiplication):
 *   forward   out = resid + s * (gamma * f32(y)): the product gamma * f32(y) rounded to fp32, that
 *             times s rounded to fp32, the sum with the residual rounded to fp32;
 *   backward  g' = g * s rounded to fp32, then mmpt_layerscale_bwd with g' for g:
 *             dy = bf16(gamma * g'), dgamma += Σ g' * f32(y) over the kept samples' rows only.
 * A map entry outside [0, B) (or a slot outside [0, Bk)) is never followed: that sample is left
 * out (treated as dropped).  1 <= Bk <= B (mmpt_droppath_add_fwd: 0 <= Bk), C % 8 == 0 and
 * C <= 4096, 16-B aligned pointers (the int32 tables: 4-B), 0 <= p < 1; else MMPT_ERR_ARG
 * (nothing is launched).  Added without a change of MMPT_ABI_VERSION: the entries are new,
 * nothing existing changed.
 * ---------------------------------------------------------------------- */
/* mmpt_dwconv7_fwd over the kept planes: c[b'] = conv(x[idx[b']]).  x fp32 [B][H][W][C],
 * c bf16 [Bk][H][W][C]; there is no gather pass, the convolution reads x through the map. */
int mmpt_dwconv7_idx_fwd(int64_t B, int64_t Bk, int64_t H, int64_t W, int64_t C, const float* x,
                         const void* idx, const void* w, const void* bias, void* c, void* stream);
/* mmpt_dwconv7_bwd_input over the kept planes: dx_out[idx[b']] = dx_in[idx[b']] + f32(bf16(convT(
 * dc[b']))).  dc bf16 [Bk][H][W][C]; dx_in (NULL: zero; may alias dx_out) and dx_out fp32
 * [B][H][W][C].  Planes that idx does not name are neither read nor written. */
int mmpt_dwconv7_idx_bwd_input(int64_t B, int64_t Bk, int64_t H, int64_t W, int64_t C,
                               const void* dc, const void* idx, const void* w, const float* dx_in,
                               float* dx_out, void* stream);
/* mmpt_dwconv7_bwd_weight over the kept planes: x fp32 [B][H][W][C] read at idx[b'], dc bf16
 * [Bk][H][W][C].  Workspace: mmpt_dwconv7_bwd_weight_workspace_bytes(Bk, H, W, C). */
int mmpt_dwconv7_idx_bwd_weight(int64_t B, int64_t Bk, int64_t H, int64_t W, int64_t C,
                                const float* x, const void* idx, const void* dc, float* dw,
                                float* db, void* workspace, void* stream);
/* The block's residual in one pass over the dense stream: plane b with slot[b] >= 0 gets the
 * forward rule above from y's compact plane slot[b], every other plane is copied.  resid, out fp32
 * dense [B][rows_per_sample][C] (out may alias resid); y bf16 [Bk*rows_per_sample][ld_y] (NULL
 * allowed when Bk == 0); gamma fp32 [C]. */
int mmpt_droppath_add_fwd(int64_t B, int64_t Bk, int64_t rows_per_sample, int64_t C,
                          const float* resid, const float* gamma, const void* y, int64_t ld_y,
                          const void* slot, double p, float* out, void* stream);
int64_t mmpt_droppath_bwd_workspace_bytes(int64_t Bk, int64_t rows_per_sample, int64_t C);
/* The backward rule above: g fp32 dense [B][rows_per_sample][C] read at the planes idx names;
 * y bf16 [Bk*rows_per_sample][ld_y], dy bf16 [Bk*rows_per_sample][ld_dy] compact; dgamma fp32 [C]
 * += through mmpt_layerscale_bwd's two-stage reduction in fixed order (no atomics). */
int mmpt_droppath_bwd(int64_t B, int64_t Bk, int64_t rows_per_sample, int64_t C, const float* g,
                      const void* idx, const float* gamma, const void* y, int64_t ld_y, double p,
                      void* dy, int64_t ld_dy, float* dgamma, void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * K22  Mamba (tf:models/mamba/modeling_mamba.py MambaMixer): the causal depthwise conv1d and the
 * selective scan, the two ops the reference takes from causal-conv1d and mamba-ssm.  Rows are
 * tokens (b, t), T = B*L rows in all; channels are contiguous and every activation has an explicit
 * leading dimension, so x and z are read in place as the halves of the in_proj output [T][2I] and
 * B and C as columns of the x_proj output [T][R+2N].  L is an argument: no kernel reads across a
 * sequence boundary — a tap before t = 0 (or a gradient tap past t = L-1) is zero, never loaded.
 * The varlen entries at the end of this block take T packed rows of sequences of any lengths
 * instead (positions and chunk offsets from int32 device tables) with the same arithmetic.
 * bf16 activations, fp32 arithmetic, one bf16 rounding where a result is stored.  Reductions over
 * tokens or channels are per-workgroup partials summed in a fixed order by a second kernel: no
 * atomics, bitwise reproducible.  Added without a change of MMPT_ABI_VERSION: the entries are new.
 * B, L >= 1 with B*L < 2^31; bad arguments return MMPT_ERR_ARG and launch nothing.
 * ---------------------------------------------------------------------- */
/* Causal conv (K = 4, C % 8 == 0, C <= 65536; 16-B aligned pointers, leading dimensions multiples
 * of 8 and >= C):  c = bf16(Σ_k w[k][ch] * x[b, t-(K-1)+k, ch] + bias[ch]) in fp32 over the taps
 * with t-(K-1)+k >= 0, u = bf16(silu(f32(c))).  x bf16 [T][ld_x], w bf16 [K][C] (tap-major: HF's
 * [C][1][K] transposed), bias bf16 [C], u bf16 [T][ld_u]. */
int mmpt_causal_conv1d_fwd(int64_t B, int64_t L, int64_t C, int64_t K, const void* x, int64_t ld_x,
                           const void* w, const void* bias, void* u, int64_t ld_u, void* stream);
int64_t mmpt_causal_conv1d_bwd_workspace_bytes(int64_t B, int64_t L, int64_t C);
/* dc = bf16((f32(du) + f32(du2)) * silu'(c)), c recomputed from x as in the forward (not stored);
 * du2 (bf16 [T][ld_du2], NULL: zero) is a second gradient of u — u feeds the scan and x_proj, and
 * x_proj's input gradient needs the dB / dC the scan's backward writes, so it joins here;
 *   dx[b,t]  = bf16(Σ_k w[k] * dc[b, t+(K-1)-k])   over the taps with t+(K-1)-k < L
 *   dw[k][ch] += f32(bf16(Σ_{b,t} dc[b,t,ch] * x[b, t-(K-1)+k, ch])),  db[ch] += f32(bf16(Σ dc))
 * (the MMPT_EPI_F32_ACC convention).  du bf16 [T][ld_du], dx bf16 [T][ld_dx] (the first half of
 * the d[x|z] buffer), dw fp32 [K][C], db fp32 [C]. */
int mmpt_causal_conv1d_bwd(int64_t B, int64_t L, int64_t C, int64_t K, const void* x, int64_t ld_x,
                           const void* w, const void* bias, const void* du, int64_t ld_du,
                           const void* du2, int64_t ld_du2, void* dx, int64_t ld_dx, float* dw,
                           float* db, void* workspace, void* stream);
/* Selective scan (I % 8 == 0, N 8 or 16, B <= 65535; B, C, A_log, states and the workspace 16-B
 * aligned, ld_bc a multiple of 8, the other leading dimensions >= I), fp32 from these operands:
 *   δ = softplus(f32(dt_raw) + dt_bias)  (threshold 20),  a = -exp(A_log)
 *   h_t = exp(δ_t a) h_{t-1} + δ_t B_t u_t,  h_{-1} = 0
 *   y_t = bf16((Σ_n C_{t,n} h_{t,n} + D u_t) * silu(f32(z_t)))
 * u, dt_raw, z, y bf16 [T][ld]; B, C bf16 [T][ld_bc] (N columns each); dt_bias, D fp32 [I]; A_log
 * fp32 [I][N].  The sequence is cut into chunks of MMPT_SCAN_CHUNK tokens that run in parallel
 * (a chunk's decay is exp(a Σδ)); the chunk length does not depend on L, so the first L' outputs
 * of a longer sequence have the bits of a length-L' run when L' is a multiple of the chunk.
 * `states` (nullable: then they stay in the workspace) receives the chunk-entry states, fp32
 * [B][chunks][I][N], mmpt_selective_scan_states_bytes of them, for the backward. */
#define MMPT_SCAN_CHUNK 32
int64_t mmpt_selective_scan_chunk(void);
int64_t mmpt_selective_scan_states_bytes(int64_t B, int64_t L, int64_t I, int64_t N);
int64_t mmpt_selective_scan_fwd_workspace_bytes(int64_t B, int64_t L, int64_t I, int64_t N);
int mmpt_selective_scan_fwd(int64_t B, int64_t L, int64_t I, int64_t N, const void* u,
                            int64_t ld_u, const void* dt_raw, int64_t ld_dt, const float* dt_bias,
                            const float* A_log, const void* Bm, const void* Cm, int64_t ld_bc,
                            const float* D, const void* z, int64_t ld_z, void* y, int64_t ld_y,
                            float* states, void* workspace, void* stream);
int64_t mmpt_selective_scan_bwd_workspace_bytes(int64_t B, int64_t L, int64_t I, int64_t N);
/* From dy bf16 [T][ld_dy] and the forward's operands and states (needed when L > MMPT_SCAN_CHUNK):
 *   du  = bf16(f32(du_in) + scan gradient)  (du_in bf16, NULL: zero; may alias du)
 *   dz, ddt_raw bf16 [T][ld];  dB, dC bf16 [T][ld_dbc] (sums over channels)
 *   dA_log[I][N] += (Σ_t dα-terms) * a,  dD[I] +=,  ddt_bias[I] +=   fp32, summed over tokens from
 *   the unrounded fp32 values.
 * h_{t-1} in the backward is always recomputed forward from a chunk-entry state. */
int mmpt_selective_scan_bwd(int64_t B, int64_t L, int64_t I, int64_t N, const void* u,
                            int64_t ld_u, const void* dt_raw, int64_t ld_dt, const float* dt_bias,
                            const float* A_log, const void* Bm, const void* Cm, int64_t ld_bc,
                            const float* D, const void* z, int64_t ld_z, const float* states,
                            const void* dy, int64_t ld_dy, const void* du_in, int64_t ld_du_in,
                            void* du, int64_t ld_du, void* dz, int64_t ld_dz, void* ddt_raw,
                            int64_t ld_ddt, void* dB, void* dC, int64_t ld_dbc, float* dA_log,
                            float* dD, float* ddt_bias, void* workspace, void* stream);
/* K22 varlen: packed rows.  The T rows are n_seq sequences laid end to end (a Batch built from
 * position_ids or a padding mask), every sequence at least one token long; the arithmetic per
 * token and per chunk is that of the entries above (the same device code), so the per-token
 * results of a sequence — u, dx, y, the states, du, dz, ddt_raw, dB, dC — have the bits of a dense
 * call on that sequence alone (B = 1, L = its length).  The sums over tokens (dw, db, dA_log, dD,
 * ddt_bias) are the same partials summed in another fixed order.  Integer tables are int32 in
 * device memory, 4-byte aligned, passed as const void*; added without a change of
 * MMPT_ABI_VERSION: the entries are new.
 * Causal conv: pos [T], the position of each token inside its sequence.  Forward tap t-j exists
 * iff pos[t] >= j; for dx, tap t+j exists iff t+j < T and pos[t+j] >= j.  A row outside the
 * sequence is never loaded.  Other arguments as mmpt_causal_conv1d_fwd / _bwd. */
int mmpt_causal_conv1d_varlen_fwd(int64_t T, int64_t C, int64_t K, const void* pos, const void* x,
                                  int64_t ld_x, const void* w, const void* bias, void* u,
                                  int64_t ld_u, void* stream);
int64_t mmpt_causal_conv1d_varlen_bwd_workspace_bytes(int64_t T, int64_t C);
int mmpt_causal_conv1d_varlen_bwd(int64_t T, int64_t C, int64_t K, const void* pos, const void* x,
                                  int64_t ld_x, const void* w, const void* bias, const void* du,
                                  int64_t ld_du, const void* du2, int64_t ld_du2, void* dx,
                                  int64_t ld_dx, float* dw, float* db, void* workspace,
                                  void* stream);
/* Selective scan: chunks of MMPT_SCAN_CHUNK tokens are counted from each sequence's own start, so
 * no chunk straddles a boundary and every carry, forward and reverse, starts from zero at a
 * sequence's start and stops at its end.  cu_seqlens [n_seq + 1]: row offsets (cu[0] = 0,
 * cu[n_seq] = T); cu_chunks [n_seq + 1]: chunk offsets, cu_chunks[s+1] - cu_chunks[s] =
 * ceil(len_s / chunk); total_chunks = cu_chunks[n_seq] <= T / chunk + n_seq, given by the caller
 * (the host never reads the tables).  n_seq <= 65535.  states fp32 [total_chunks][I][N]; needed by
 * the backward when total_chunks > n_seq.  Other arguments as mmpt_selective_scan_fwd / _bwd. */
int64_t mmpt_selective_scan_varlen_states_bytes(int64_t total_chunks, int64_t I, int64_t N);
int64_t mmpt_selective_scan_varlen_fwd_workspace_bytes(int64_t total_chunks, int64_t I, int64_t N);
int mmpt_selective_scan_varlen_fwd(int64_t T, int64_t n_seq, int64_t total_chunks,
                                   const void* cu_seqlens, const void* cu_chunks, int64_t I,
                                   int64_t N, const void* u, int64_t ld_u, const void* dt_raw,
                                   int64_t ld_dt, const float* dt_bias, const float* A_log,
                                   const void* Bm, const void* Cm, int64_t ld_bc, const float* D,
                                   const void* z, int64_t ld_z, void* y, int64_t ld_y,
                                   float* states, void* workspace, void* stream);
int64_t mmpt_selective_scan_varlen_bwd_workspace_bytes(int64_t T, int64_t total_chunks, int64_t I,
                                                       int64_t N);
int mmpt_selective_scan_varlen_bwd(int64_t T, int64_t n_seq, int64_t total_chunks,
                                   const void* cu_seqlens, const void* cu_chunks, int64_t I,
                                   int64_t N, const void* u, int64_t ld_u, const void* dt_raw,
                                   int64_t ld_dt, const float* dt_bias, const float* A_log,
                                   const void* Bm, const void* Cm, int64_t ld_bc, const float* D,
                                   const void* z, int64_t ld_z, const float* states,
                                   const void* dy, int64_t ld_dy, const void* du_in,
                                   int64_t ld_du_in, void* du, int64_t ld_du, void* dz,
                                   int64_t ld_dz, void* ddt_raw, int64_t ld_ddt, void* dB,
                                   void* dC, int64_t ld_dbc, float* dA_log, float* dD,
                                   float* ddt_bias, void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * ZeRO++ quantized communication (sharding = "zero_3++"): replaces DeepSpeed's
 * `zero_quantized_weights` / `zero_quantized_gradients` kernels that
 * src/train.py:196-201 switches on.  Blockwise symmetric quantization, 256-element
 * blocks that never straddle a part (a rank's shard of `n_part` elements, a multiple
 * of 4), one fp32 scale per block, scales laid out [part][block].
 *   quant_int8: q = rint(x·127/absmax) ∈ [-127, 127], scale = absmax/127 (bf16 in);
 *   dequant_int8: y = bf16(q·scale);
 *   quant_int4: q = rint(x·7/absmax) ∈ [-7, 7], two per byte (low nibble = even
 *               element), scale = absmax/7 (fp32 in);
 *   dequant_int4_sum: dst[i] += Σ_{r<parts} q_r[i]·scale_r (rank order, fp32).
 * ---------------------------------------------------------------------- */
int64_t mmpt_quant_blocks(int64_t n_part);
int mmpt_quant_int8(int64_t n_part, int64_t parts, const void* src_bf16, void* dst_i8,
                    float* scales, void* stream);
int mmpt_dequant_int8(int64_t n_part, int64_t parts, const void* src_i8, const float* scales,
                      void* dst_bf16, void* stream);
int mmpt_quant_int4(int64_t n_part, int64_t parts, const float* src, void* dst_u8,
                    float* scales, void* stream);
int mmpt_dequant_int4_sum(int64_t n_part, int64_t parts, const void* src_u8, const float* scales,
                          float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMPT_H_ */
