/* snx.h -- C ABI of libsnx.so: the MI355X-native (gfx950) SPLADE-ModernBERT training hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI on this path -- its boundary is the
 * Python class API of src/model/splade_modern.py and src/model/losses.py, which dispatches
 * implicitly to aten/cuBLAS/SDPA kernels -- so each entry point below cites the reference
 * statement(s) whose device work it replaces.  `ref:` = /root/reference, `hf:` =
 * transformers/models/modernbert/modeling_modernbert.py (the third-party module the reference
 * wraps at ref:src/model/splade_modern.py:38,69-73).
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked [host];
 *   - caller owns all buffers; nothing is allocated, freed or synchronised inside;
 *   - work is enqueued on `stream` and is ordered with other work on that stream; the operator entry
 *     points are re-entrant across streams (no hidden state).  snx_model_backward additionally forks its
 *     weight-gradient GEMMs onto ONE process-wide internal stream (event fork/join, joined before it
 *     returns: callers still see everything ordered on `stream`); it is therefore not meant to be called
 *     from several host threads at once (one process drives one GPU).  SNX_BWD_OVERLAP=0 keeps everything
 *     on `stream`;
 *   - return 0 on success, a positive hipError_t if a launch failed, or a negative SNX_E_* code
 *     when the arguments violate a kernel's shape assumptions (checked on the host BEFORE any
 *     launch -- a mis-shaped call never reaches the GPU);
 *   - bf16 tensors are raw uint16 storage (`void*`), row-major, contiguous; "T" is the number
 *     of token rows (all sequences of a call laid end to end), sequence s owns rows
 *     cu_seqlens[s] .. cu_seqlens[s+1]-1 (int32, nseq+1 entries, cu_seqlens[0]=0,
 *     cu_seqlens[nseq]=T); `mask` is the reference's attention_mask flattened to [T] (int64,
 *     1 = token, 0 = padding).
 *   - constraints: head_dim == 64, hidden % 256 == 0 (<= 1024), intermediate % 64 == 0, GEMM K % 64 == 0,
 *     sequence length <= 65535.
 */
#ifndef SNX_H_
#define SNX_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(__HIP__) && !defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
typedef struct ihipStream_t* hipStream_t;
#endif

#define SNX_E_SHAPE (-2)
#define SNX_E_ARG (-3)
#define SNX_FWD_SAVE_FOR_BACKWARD 1
/* The caller does not need token_weights (a trainer whose loss reads the pooled vectors only): the decoder runs without
 * the row half of its epilogue and without the token_weights pass.  `token_weights` (may be NULL) and the arena's token
 * keys are NOT written, `sparse`, the saved keys and every gradient keep their bits; the arena is sized by
 * snx_model_workspace_bytes_fwd (no row maxima).  A backward handed a g_token_weights for such an arena returns SNX_E_ARG. */
#define SNX_FWD_NO_TOKEN_WEIGHTS 2

/* Architecture constants (ref:huggingface/v33/config.json; hf configuration_modernbert.py:113-162).
 * layer l is a global-attention layer iff l % global_every == 0; `window` is the HALF window
 * (local_attention / 2): key j visible to query i iff |i-j| <= window. */
typedef struct snx_model_desc {
  int32_t vocab, hidden, inter, layers, heads, head_dim;
  int32_t global_every, window, pad_id, reserved0;
  float ln_eps, reserved1;
} snx_model_desc;

int snx_version(void);

/* Number of parameter tensors in the canonical order used by `params` / `grads` arrays:
 *   tok_embeddings.weight, embeddings.norm.weight, then per layer [attn_norm.weight (l>=1)],
 *   attn.Wqkv.weight, attn.Wo.weight, mlp_norm.weight, mlp.Wi.weight, mlp.Wo.weight, then
 *   final_norm.weight, head.dense.weight, head.norm.weight, decoder.bias
 * (= the reference state-dict order, the tied decoder.weight counted once). */
int32_t snx_param_count(const snx_model_desc* d);

/* ---- whole-model entry points (native layer loop) --------------------------------------- */

/* bf16 copies of the fp32 master weights ([out,in] and transposed), refreshed after every
 * optimizer step.  Replaces autocast's per-forward weight casts (ref:train_v33_ddp.py:337). */
size_t snx_weight_cache_bytes(const snx_model_desc* d);
int snx_weight_cache_refresh(const snx_model_desc* d, const void* const* params /*[host] fp32 device ptrs*/,
                             void* cache, hipStream_t stream);

/* Activation arena size for one forward over T token rows (save_for_bwd=0: inference plan). */
size_t snx_model_workspace_bytes(const snx_model_desc* d, int32_t T, int32_t nseq, int32_t save_for_bwd);
/* ... for a forward called with `flags` (SNX_FWD_*): smaller with SNX_FWD_NO_TOKEN_WEIGHTS, else the size above.  Every
 * offset below is the same in both. */
size_t snx_model_workspace_bytes_fwd(const snx_model_desc* d, int32_t T, int32_t nseq, int32_t flags);
size_t snx_model_bwd_workspace_bytes(const snx_model_desc* d, int32_t T, int32_t nseq, int32_t max_seqlen);
/* byte offset, inside a save_for_bwd arena, of the packed arg-max keys u32 [nseq, vocab]
 * (bf16 bits of relu(logit) << 16 | 0xFFFF - row): lets a caller inspect the max-pool routing. */
size_t snx_model_keys_offset(const snx_model_desc* d, int32_t T, int32_t nseq);
/* byte offset, inside a save_for_bwd arena, of the per-token maximum keys u32 [T] (bf16 bits of relu(logit) << 16 |
 * 0xFFFF - v*, v* = first vocabulary column of the token's maximum; 0xFFFF for masked tokens and tokens whose maximum
 * is 0): the token_weights routing, written by every forward that saves for backward (which needs vocab <= 65535). */
size_t snx_model_token_keys_offset(const snx_model_desc* d, int32_t T, int32_t nseq);

/* SPLADEModernBERT.forward (ref:src/model/splade_modern.py:50-88):
 *   ids,mask [T] int64; pos [T] int32 (position of each row inside its sequence);
 *   rope_* [max_pos][32][2] fp32 (cos,sin) tables for theta_global / theta_local (hf:136-163);
 *   -> sparse [nseq, vocab] fp32, token_weights [T] fp32; `saved` = arena (see above).  With SNX_FWD_SAVE_FOR_BACKWARD
 * the arena also keeps every token's arg-max column (snx_model_token_keys_offset): both outputs are differentiable. */
int snx_model_forward(const snx_model_desc* d, const void* const* params /*[host]*/, const void* wcache,
                      const int64_t* ids, const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                      const float* rope_global, const float* rope_local, void* saved, float* sparse,
                      float* token_weights, const int32_t* groups /*[host] or NULL*/, int32_t T, int32_t nseq,
                      int32_t max_seqlen, int32_t flags, hipStream_t stream);
/* `groups` (optional): {n, (seq_begin, nseq, max_len) x n} -- consecutive sequence groups of different
 * maximum length laid end to end in ONE call (e.g. the query, positive and negative batches of a
 * training micro-step); NULL = one group of nseq sequences. */
/* One PASS of a micro-step into a row range of a larger arena: the reference calls model(...) three times per micro-step
 * (query, positive, negative: ref:src/train/cli/train_v33_ddp.py:339-343) and back-propagates once.  `saved`, `sparse_all`
 * [nseq_plan, vocab] and `token_weights_all` [T_plan] are laid out for the WHOLE micro-step (snx_model_workspace_bytes(T_plan,
 * nseq_plan, 1)); this call fills token rows [row0, row0 + T) and sequences [seq0, seq0 + nseq) from the pass's own
 * ids / mask / pos / cu_seqlens (cu_seqlens[0] = 0), groups = NULL, flags must save for backward.  After the last pass the
 * arena equals what one snx_model_forward over all rows (with the passes as sequence groups) leaves behind, so ONE
 * snx_model_backward(_units) over (T_plan, nseq_plan) with the concatenated ids / mask / pos / global cu_seqlens runs the
 * micro-step's backward on full-size launches.  row0 = seq0 = 0, T = T_plan, nseq = nseq_plan is snx_model_forward. */
int snx_model_forward_range(const snx_model_desc* d, const void* const* params /*[host]*/, const void* wcache,
                            const int64_t* ids, const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                            const float* rope_global, const float* rope_local, void* saved, float* sparse_all,
                            float* token_weights_all, const int32_t* groups /*NULL for a true sub-range*/, int32_t T_plan,
                            int32_t nseq_plan, int32_t row0, int32_t seq0, int32_t T, int32_t nseq, int32_t max_seqlen,
                            int32_t flags, hipStream_t stream);

/* Backward of the above (the autograd graph of ref:src/model/splade_modern.py:69-86 and of the HF
 * encoder): g_sparse [nseq, vocab] fp32 = dL/d sparse_repr; every grads[i] (fp32, same shape as
 * params[i]) is ACCUMULATED into (+=).  These entry points take no gradient for token_weights (it is zero); the _tw
 * variants below take one. */
int snx_model_backward(const snx_model_desc* d, const void* const* params /*[host]*/, void* const* grads /*[host]*/,
                       const void* wcache, const int64_t* ids, const int64_t* mask, const int32_t* cu_seqlens,
                       const int32_t* pos, const float* rope_global, const float* rope_local, const void* saved,
                       const float* g_sparse, void* scratch, const int32_t* groups /*[host] or NULL, as forward*/,
                       int32_t T, int32_t nseq, int32_t max_seqlen, hipStream_t stream);

/* The same backward as a chain of layers + 2 UNITS in execution order: unit 0 = SPLADE tail + tied decoder +
 * head + final norm, unit 1 + i = encoder layer (layers - 1 - i), unit layers + 1 = embeddings.  Consecutive
 * calls over [unit_begin, unit_end) ranges that together cover [0, layers + 2), with the SAME scratch buffer,
 * equal one snx_model_backward.  When a range returns, the gradients of its parameters are complete (except
 * the tied embedding matrix, which receives the decoder's share in unit 0 and the embedding's in the last):
 * `notify` (nullable) is made to wait for them (launch stream AND the internal weight-gradient stream), so
 * that a data-parallel caller can all-reduce that slice there while later units still run -- the overlap the
 * reference gets from DDP's bucketed reducer (ref:src/train/cli/train_v33_ddp.py:539-544,363-364). */
int snx_model_backward_units(const snx_model_desc* d, const void* const* params /*[host]*/,
                             void* const* grads /*[host]*/, const void* wcache, const int64_t* ids,
                             const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                             const float* rope_global, const float* rope_local, const void* saved,
                             const float* g_sparse, void* scratch, const int32_t* groups /*[host] or NULL*/,
                             int32_t T, int32_t nseq, int32_t max_seqlen, int32_t unit_begin, int32_t unit_end,
                             hipStream_t notify, hipStream_t stream);

/* ... over the first T rows / nseq sequences of an arena and scratch laid out for (T_plan, nseq_plan): the backward of a
 * micro-step that placed fewer passes than planned (snx_model_forward_range); `scratch` needs
 * snx_model_bwd_workspace_bytes(T_plan, nseq_plan, max_seqlen). */
int snx_model_backward_units_range(const snx_model_desc* d, const void* const* params /*[host]*/,
                                   void* const* grads /*[host]*/, const void* wcache, const int64_t* ids,
                                   const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                                   const float* rope_global, const float* rope_local, const void* saved,
                                   const float* g_sparse, void* scratch, const int32_t* groups /*[host] or NULL*/,
                                   int32_t T_plan, int32_t nseq_plan, int32_t T, int32_t nseq, int32_t max_seqlen,
                                   int32_t unit_begin, int32_t unit_end, hipStream_t notify, hipStream_t stream);
/* ... with g_token_weights [T] fp32 = dL/d token_weights in the arena's row order (NULL: exactly the entry point above):
 *   d logit[t, v*(t)] += g_token_weights[t] mask[t] / (1 + x),  x = relu(logit[t, v*(t)]) > 0,
 * added to the max-pool gradient of the same logit before its one bf16 rounding; every gradient deterministic. */
int snx_model_backward_units_range_tw(const snx_model_desc* d, const void* const* params /*[host]*/,
                                      void* const* grads /*[host]*/, const void* wcache, const int64_t* ids,
                                      const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                                      const float* rope_global, const float* rope_local, const void* saved,
                                      const float* g_sparse, const float* g_token_weights /*[T] or NULL*/, void* scratch,
                                      const int32_t* groups /*[host] or NULL*/, int32_t T_plan, int32_t nseq_plan,
                                      int32_t T, int32_t nseq, int32_t max_seqlen, int32_t unit_begin, int32_t unit_end,
                                      hipStream_t notify, hipStream_t stream);

/* The encoder WITHOUT the SPLADE tail (masked-language-model pre-training reads the head's output and applies a head of
 * its own, snx_mlm_ce_* below): the launches of snx_model_forward up to and including snx_gelu_ln_fwd -- no decoder runs,
 * no keys and no token keys are written.  `saved` needs snx_model_workspace_bytes(T, nseq, save_for_bwd); hd [T, hidden]
 * bf16, bit for bit the decoder's input of snx_model_forward, lies at snx_model_hd_offset() of a save_for_bwd arena. */
int snx_model_forward_hidden(const snx_model_desc* d, const void* const* params /*[host]*/, const void* wcache,
                             const int64_t* ids, const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                             const float* rope_global, const float* rope_local, void* saved,
                             const int32_t* groups /*[host] or NULL*/, int32_t T, int32_t nseq, int32_t max_seqlen,
                             int32_t save_for_bwd, hipStream_t stream);
/* byte offset, inside a save_for_bwd arena, of hd [T, hidden] bf16 (the head's output, the decoder's input) */
size_t snx_model_hd_offset(const snx_model_desc* d, int32_t T, int32_t nseq);
/* snx_model_backward_units_range_tw from the gradient of hd: g_hd [T, hidden] bf16 takes the place of g_sparse /
 * g_token_weights.  Unit 0 copies it where the SPLADE backward would have written it and runs no SPLADE backward; every
 * launch behind that is the one of the entry point above.  The gradients of the tied embedding matrix and of decoder.bias
 * through the caller's head are the caller's to add (before or after: both are accumulated). */
int snx_model_backward_units_range_hd(const snx_model_desc* d, const void* const* params /*[host]*/,
                                      void* const* grads /*[host]*/, const void* wcache, const int64_t* ids,
                                      const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                                      const float* rope_global, const float* rope_local, const void* saved,
                                      const void* g_hd, void* scratch, const int32_t* groups /*[host] or NULL*/,
                                      int32_t T_plan, int32_t nseq_plan, int32_t T, int32_t nseq, int32_t max_seqlen,
                                      int32_t unit_begin, int32_t unit_end, hipStream_t notify, hipStream_t stream);

/* ---- fp32 execution (csrc/f32_path.hip): what the reference computes OUTSIDE torch.autocast -- a bare
 * SPLADEModernBERT.forward (ref:src/model/splade_modern.py:50-88), its inference encoder (ref:benchmark/encoders.py:
 * 309-345) and the fp32 leg of the tolerance protocol.  Same contract as the entry points above with fp32 weights
 * (`params` themselves: no weight cache), fp32 activations and contraction, no bf16 cast point; any hidden size,
 * even head_dim <= 64, any intermediate size (the tiny parity configuration runs here).  rope_* tables are
 * [max_pos][head_dim / 2][2].  The precision path, not the throughput path. */
size_t snx_model_workspace_bytes_f32(const snx_model_desc* d, int32_t T, int32_t nseq, int32_t save_for_bwd);
size_t snx_model_bwd_workspace_bytes_f32(const snx_model_desc* d, int32_t T);
int snx_model_forward_f32(const snx_model_desc* d, const void* const* params /*[host]*/, const int64_t* ids,
                          const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos, const float* rope_global,
                          const float* rope_local, void* saved, float* sparse, float* token_weights, int32_t T,
                          int32_t nseq, int32_t flags, hipStream_t stream);
int snx_model_backward_f32(const snx_model_desc* d, const void* const* params /*[host]*/, void* const* grads /*[host]*/,
                           const int64_t* ids, const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                           const float* rope_global, const float* rope_local, const void* saved, const float* g_sparse,
                           void* scratch, int32_t T, int32_t nseq, hipStream_t stream);
/* ... with g_token_weights [T] fp32 or NULL (= snx_model_backward_f32). */
int snx_model_backward_f32_tw(const snx_model_desc* d, const void* const* params /*[host]*/, void* const* grads /*[host]*/,
                              const int64_t* ids, const int64_t* mask, const int32_t* cu_seqlens, const int32_t* pos,
                              const float* rope_global, const float* rope_local, const void* saved, const float* g_sparse,
                              const float* g_token_weights, void* scratch, int32_t T, int32_t nseq, hipStream_t stream);
/* fp32 GEMM on v_mfma_f32_32x32x2_f32 with strided operands: C[m,n] (+)= (R[m,n]) + sum_k A[m a_row + k a_k] B[n b_row + k b_k]
 * (nn.Linear in fp32: forward, dX and dW are the same kernel with different strides). */
int snx_gemm_f32(const float* A, int64_t a_row, int64_t a_k, const float* B, int64_t b_row, int64_t b_k, float* C, int64_t ldc,
                 const float* R, int64_t ldr, int32_t M, int32_t N, int32_t K, int32_t accumulate, hipStream_t stream);
/* The steps of the two model entry points above, one call each: snx_model_forward_f32 / snx_model_backward_f32_tw are
 * sequences of exactly these calls and of snx_gemm_f32's launch, so a test that runs one alone runs what the model runs
 * (tests/test_gpu_f32_per_element.py).  All tensors fp32 and row-major unless stated; shapes SNX_E_SHAPE, NULLs SNX_E_ARG.
 * seq_ids: seqid[t] = the sequence of token t (cu_seqlens as above).
 * ln_fwd: out [T, H] = LN(x) * w; src 0: x = in [T, H]; 1: x = in[ids[t]] (embedding gather, ids int64 [T]); 2: x = gelu(in).
 * ln_bwd: the backward of ln_fwd for upstream dy [T, H]; dw [H] += sum_t dy xhat (float atomics: dw is accumulated into).
 *   src 0: dst [T, H] = dx, or += dx with accumulate != 0; src 1: dst[ids[t]] += dx (float atomics), no row for
 *   ids[t] == pad_id; src 2: dst = dx * gelu'(in).  accumulate != 0 is legal with src 0 only.
 * rope: rotates the q and k thirds of qkv [T, 3, heads, head_dim] in place, table [max_pos][head_dim / 2][2] (cos, sin),
 *   pos int32 [T]; inverse != 0: the transposed rotation (the backward).  head_dim even, 2..64.
 * geglu_fwd: y [T, I] = gelu(u[:, :I]) * u[:, I:], u [T, 2 I]; geglu_bwd: du [T, 2 I] from u and dy [T, I].
 * attn_fwd: out [T, heads, head_dim], lse [heads, T] of softmax(q k^T / sqrt(head_dim)) v over the keys j of the query's
 *   own sequence with mask[j] != 0 and (window < 0 or |i - j| <= window); a query that sees no key gives out = 0, lse = 0.
 *   head_dim % 8 == 0 runs the MFMA-tiled form, where mask == NULL (every key valid) and lse == NULL (not stored) are
 *   legal and seqid is not read; any other even head_dim, and every one under "f32_attn_rows" = 1, runs one wave per
 *   (token, head), which needs seqid, mask and lse.
 * attn_bwd: dqkv [T, 3, heads, head_dim] (zeroed here, then dq written, dk / dv by float atomics) from qkv, the forward's
 *   out and lse, and dout [T, heads, head_dim].
 * tail_fwd: the tied decoder and the SPLADE tail: logits = Hd [T, H] E [V, H]^T + bias [V], w = log1p(relu(logits)) * mask;
 *   keys [nseq, V] (uint64: bits of max_t w << 32 | 0xFFFFFFFF - pos of the FIRST token of the maximum) and twkeys [T]
 *   (uint64: bits of max_v w << 32 | 0xFFFFFFFF - the FIRST v of the maximum) are zeroed and filled; sparse [nseq, V] and
 *   token_weights [T] are their high words.
 * tail_bwd: the routed backward of tail_fwd from its keys / twkeys: for every (b, v) with sparse > 0 and g_sparse != 0,
 *   c = g_sparse exp(-sparse): dHd[cu_seqlens[b] + pos] += c E[v], gradE[v] += c Hd[token], gradb[v] += c; the same per
 *   token with g_token_weights [T] (or NULL) through twkeys.  dHd [T, H] is zeroed here; gradE [V, H] and gradb [V] are
 *   accumulated into (float atomics). */
int snx_f32_seq_ids(const int32_t* cu_seqlens, int32_t* seqid, int32_t T, int32_t nseq, hipStream_t stream);
int snx_f32_ln_fwd(const float* in, const int64_t* ids, const float* w, float* out, int32_t T, int32_t H, float eps, int32_t src,
                   hipStream_t stream);
int snx_f32_ln_bwd(const float* dy, const float* in, const int64_t* ids, const float* w, float* dst, float* dw, int32_t T,
                   int32_t H, float eps, int32_t src, int32_t accumulate, int32_t pad_id, hipStream_t stream);
int snx_f32_rope(float* qkv, const float* table, const int32_t* pos, int32_t T, int32_t heads, int32_t head_dim,
                 int32_t inverse, hipStream_t stream);
int snx_f32_geglu_fwd(const float* u, float* y, int32_t T, int32_t I, hipStream_t stream);
int snx_f32_geglu_bwd(const float* u, const float* dy, float* du, int32_t T, int32_t I, hipStream_t stream);
int snx_f32_attn_fwd(const float* qkv, const int32_t* cu_seqlens, const int32_t* seqid, const int64_t* mask, float* out,
                     float* lse, int32_t T, int32_t nseq, int32_t heads, int32_t head_dim, int32_t window, hipStream_t stream);
int snx_f32_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, const int32_t* cu_seqlens,
                     const int32_t* seqid, const int64_t* mask, float* dqkv, int32_t T, int32_t nseq, int32_t heads,
                     int32_t head_dim, int32_t window, hipStream_t stream);
int snx_f32_tail_fwd(const float* Hd, const float* E, const float* bias, const int64_t* mask, const int32_t* seqid,
                     const int32_t* pos, void* keys, void* twkeys, float* sparse, float* token_weights, int32_t T,
                     int32_t nseq, int32_t V, int32_t H, hipStream_t stream);
int snx_f32_tail_bwd(const float* g_sparse, const float* g_token_weights, const void* keys, const void* twkeys,
                     const float* Hd, const float* E, const int32_t* cu_seqlens, float* dHd, float* gradE, float* gradb,
                     int32_t T, int32_t nseq, int32_t V, int32_t H, hipStream_t stream);

/* ---- dense teacher encoder (csrc/teacher.hip): the forward of an XLM-RoBERTa encoder with CLS pooling -- BGE-M3's dense
 * head, what ref:src/model/teachers/bge_m3.py:66-94 and ref:scripts/precompute_teacher_scores.py:89-159 run through
 * sentence-transformers.  `xr:` = transformers/models/xlm_roberta/modeling_xlm_roberta.py.  Post-LayerNorm with biases,
 * learned absolute positions, erf-GELU MLP, no RoPE, no window.  Same contract as the snx_model_* entry points: nothing
 * allocated inside, caller-owned arena, stream-ordered, shapes checked on the host before any launch.
 * precision: SNX_TEACHER_BF16 -- GEMM operands and GEMM outputs bf16 (snx_gemm_nt_bf16, snx_attn_fwd), the residual stream
 * h and all LayerNorm / GELU / softmax arithmetic fp32; SNX_TEACHER_F32 -- no cast point (snx_gemm_f32, fp32 attention).
 * Constraints: hidden % 256 == 0 (<= 1024), head_dim == 64, heads * 64 == hidden, inter % 64 == 0, layers <= 128. */
#define SNX_TEACHER_BF16 0
#define SNX_TEACHER_F32 1
typedef struct snx_teacher_desc {
  int32_t vocab, hidden, inter, layers, heads, head_dim;
  int32_t max_pos, type_vocab, pad_id, reserved0;
  float ln_eps, reserved1;
} snx_teacher_desc;
/* Number of parameter tensors of XLMRobertaModel(add_pooling_layer=False), in the canonical order of `params`:
 *   word_embeddings, position_embeddings, token_type_embeddings, embeddings.LayerNorm.{weight,bias}, then per layer
 *   query.{weight,bias}, key.{..}, value.{..}, attention.output.dense.{..}, attention.output.LayerNorm.{..},
 *   intermediate.dense.{..}, output.dense.{..}, output.LayerNorm.{..}      (5 + 16 layers; all fp32). */
int32_t snx_teacher_param_count(const snx_teacher_desc* d);
/* bf16 copies of the matrices, q / k / v stacked to [3 hidden, hidden] (the QKV GEMM's output then IS the [T, 3, heads, 64]
 * layout of the attention), and the stacked fp32 q / k / v bias [3 hidden].  Both precisions read the cache (the fp32
 * path its biases only); refresh it whenever the weights change. */
size_t snx_teacher_weight_cache_bytes(const snx_teacher_desc* d);
int snx_teacher_weight_cache_refresh(const snx_teacher_desc* d, const void* const* params /*[host] fp32 device ptrs*/,
                                     void* cache, hipStream_t stream);
size_t snx_teacher_workspace_bytes(const snx_teacher_desc* d, int32_t T, int32_t nseq, int32_t precision);
/* ids [T] int64 (unpadded, sequences end to end), pos_ids [T] int32 (XLM-R: cumsum(mask) * mask + pad_id, computed by the
 * caller on the padded batch) -> cls_out [nseq, hidden] fp32 = last_hidden_state[:, 0], emb_out [nseq, hidden] fp32 =
 * cls / max(||cls||_2, 1e-12).  Every sequence needs at least one token; max_seqlen = the longest sequence of the call.
 * cu_seqlens [nseq + 1]: ascending, cu_seqlens[0] = 0, cu_seqlens[nseq] = T, as for snx_model_forward_f32 -- the kernels
 * trust it. */
int snx_teacher_forward(const snx_teacher_desc* d, const void* const* params /*[host]*/, const void* wcache,
                        const int64_t* ids, const int32_t* pos_ids, const int32_t* cu_seqlens, void* workspace,
                        float* cls_out, float* emb_out, int32_t T, int32_t nseq, int32_t max_seqlen, int32_t precision,
                        hipStream_t stream);
/* The row kernels of the forward, exported for parity tests.  y_f32 != 0: `y` is fp32 (fp32 path), else bf16 (bf16 path);
 * x_out (bf16, nullable) receives bf16(h_out).  H as `hidden` above.
 * embed_ln (xr: XLMRobertaEmbeddings): h_out = LN((word[ids[t]] + type0) + pos[pos_ids[t]]) * w + b; ids and pos_ids are
 * clamped into their tables.
 * bias_resid_ln (xr: XLMRobertaSelfOutput / XLMRobertaOutput): h_out = LN((y + bias) + h) * w + b; h_out may be h.
 * bias_rows / bias_gelu: y += bias / y = gelu_erf(y + bias), in place on [T, N], N % 8 == 0, one rounding when y is bf16.
 * cls_normalize: cls[s] = h[cu_seqlens[s]], emb[s] = cls[s] / max(||cls[s]||_2, 1e-12) (F.normalize).
 * attn_f32: out [T, heads, 64] = softmax(q k^T / 8) v over the keys of the row's own sequence, qkv fp32 [T, 3, heads, 64];
 * the tiled forward of the fp32 path (snx_model_forward_f32) without mask or window.  qkv and out 16-byte aligned;
 * cu_seqlens as for snx_teacher_forward (ascending, from 0 to T): it is not checked on the device. */
int snx_teacher_embed_ln(const int64_t* ids, const int32_t* pos_ids, const float* word, const float* pos, const float* type0,
                         const float* w, const float* b, float* h_out, void* x_out, int32_t T, int32_t H, int32_t vocab,
                         int32_t max_pos, float eps, hipStream_t stream);
int snx_teacher_bias_resid_ln(const float* h, const void* y, int32_t y_f32, const float* bias, const float* w, const float* b,
                              float* h_out, void* x_out, int32_t T, int32_t H, float eps, hipStream_t stream);
int snx_teacher_bias_rows(void* y, int32_t y_f32, const float* bias, int32_t T, int32_t N, hipStream_t stream);
int snx_teacher_bias_gelu(void* y, int32_t y_f32, const float* bias, int32_t T, int32_t N, hipStream_t stream);
int snx_teacher_cls_normalize(const float* h, const int32_t* cu_seqlens, float* cls, float* emb, int32_t T, int32_t nseq,
                              int32_t H, hipStream_t stream);
int snx_teacher_attn_f32(const float* qkv, const int32_t* cu_seqlens, float* out, int32_t T, int32_t nseq, int32_t heads,
                         hipStream_t stream);

/* ---- inference post-processing (ref:benchmark/encoders.py:309-345 NeuralSparseEncoderV33._encode_batch) ---- */
/* Per row of rep [B,V] fp32: entries with rep > 0 and allowed[v] != 0 survive.  k > 0 and more than k survivors:
 * the k largest, weight descending, ties lowest id first (out_sorted[b] = 1); otherwise all survivors in id
 * order (out_sorted[b] = 0).  out_val / out_idx [B,cap] (cap >= min(k,V), or >= V when k <= 0), out_cnt [B].
 * k <= 16384. */
int snx_sparse_topk(const float* rep, const uint8_t* allowed, float* out_val, int32_t* out_idx, int32_t* out_cnt,
                    int32_t* out_sorted, int32_t B, int32_t V, int32_t k, int32_t cap, hipStream_t stream);

/* ---- exact sparse retrieval for the mid-training evaluator (ref:benchmark/searchers.py:155-188: the OpenSearch
 * neural-sparse search the reference benchmark runs; ref:benchmark/metrics.py:52-99: the hit ranks its metrics read) ----
 * Docs and queries are CSR rows: ptr [n+1] int64, term [nnz] int32 strictly ascending within a row, w [nnz] fp32 > 0.
 * Score definition (part of the ABI, bit-reproducible): s(q,d) = fp32 acc starting at +0, acc = fmaf(q_w, d_w, acc)
 * over the shared terms in ascending term id.
 * Index: term_ptr [V+1] int64, post_doc [nnz] int32, post_w [nnz] fp32 -- term-major, every posting list in doc-id
 * order, byte-identical from run to run; workspace: snx_sparse_index_workspace_bytes(nd, V) bytes.
 * Search: per query the top k (1 <= k <= 1024) docs with score > 0 -> out_doc / out_score [nq,k], score descending,
 * ties lowest doc id first; unused slots doc -1, score 0.  target [nq] (or NULL): out_tscore [nq] = s(q, target)
 * (bit-equal to the ranked value), out_rank [nq] = 1 + #{d: s_d > s_t} + #{d < t: s_d == s_t}, 0 when s_t == 0 or the
 * target is out of range.  chunk_docs: docs per LDS-resident score chunk (0: default; <= 32768); it changes no bit.
 * workspace: snx_sparse_search_workspace_bytes(nq, nd, k, chunk_docs) bytes. */
size_t snx_sparse_index_workspace_bytes(int32_t nd, int32_t V);
int snx_sparse_index_build(const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd, int32_t V,
                           int64_t nnz, int64_t* term_ptr, int32_t* post_doc, float* post_w, void* workspace,
                           size_t ws_bytes, hipStream_t stream);
size_t snx_sparse_search_workspace_bytes(int32_t nq, int32_t nd, int32_t k, int32_t chunk_docs);
int snx_sparse_search(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq, const int64_t* term_ptr,
                      const int32_t* post_doc, const float* post_w, const int64_t* doc_ptr, const int32_t* doc_term,
                      const float* doc_w, int32_t nd, int32_t V, const int32_t* target, int32_t k, int32_t chunk_docs,
                      int32_t* out_doc, float* out_score, int32_t* out_rank, float* out_tscore, void* workspace,
                      size_t ws_bytes, hipStream_t stream);

/* ---- hard-negative mining over the same index (src/train/mining) ----
 * Pair scores: out[i] = s(pair_q[i], pair_d[i]) for npairs (query row, doc row) pairs over the query and doc CSR,
 * bit-equal to the value the searches rank; a pair with an index out of range scores 0.
 * Band search: per query q an exclusion row ex_doc[ex_ptr[q] .. ex_ptr[q+1]) (doc ids ascending and distinct; ex_ptr
 * NULL: none) and ceiling[q] fp32 (NULL or +inf: none).  Doc d is ADMISSIBLE for q when s(q,d) > 0, d is not in the
 * row, and s(q,d) < ceiling[q] (strict, fp32; a NaN ceiling admits nothing).  The admissible docs are ranked score
 * descending, ties lowest doc id first (the search's order); ranks lo .. hi-1 (0-based, 0 <= lo < hi <= 1024) go to
 * out_doc / out_score [nq, hi-lo], unused slots doc -1, score 0; out_found [nq] = filled slots.  chunk_docs as for
 * the search: it changes no bit.  workspace: snx_sparse_search_band_workspace_bytes(nq, nd, hi, chunk_docs) bytes. */
int snx_sparse_pair_scores(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                           const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd,
                           const int32_t* pair_q, const int32_t* pair_d, int64_t npairs, float* out, hipStream_t stream);
size_t snx_sparse_search_band_workspace_bytes(int32_t nq, int32_t nd, int32_t hi, int32_t chunk_docs);
int snx_sparse_search_band(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                           const int64_t* term_ptr, const int32_t* post_doc, const float* post_w, int32_t nd, int32_t V,
                           const int64_t* ex_ptr, const int32_t* ex_doc, const float* ceiling, int32_t lo, int32_t hi,
                           int32_t chunk_docs, int32_t* out_doc, float* out_score, int32_t* out_found, void* workspace,
                           size_t ws_bytes, hipStream_t stream);

/* ---- SEISMIC approximate search over the same index (Bruch et al., SIGIR 2024; the `sparse_vector` ANN method of
 * ref:huggingface/v33/README.md, measured at ref:scripts/neural_sparse_search_aws.py:1314-1510).  A deterministic form
 * of the published algorithm with OpenSearch's parameter names; it does not reproduce OpenSearch's numbers (no centroid
 * sampling, fp32 summaries without quantization, one index per corpus).  s(a, b) is the score above, applied to
 * query.doc, doc.doc and query.summary alike; "search order" = score descending, ties lowest doc id first.
 * Build, for every term t (parameters n_postings >= 1, cluster_ratio r in (0, 1], summary_prune_ratio alpha in (0, 1]):
 *   1. P_t = the first min(|L_t|, n_postings) postings of t by (weight desc, doc asc); prune_ptr [V+1] (host scan of
 *      the kept counts), prune_doc / prune_w [npruned] hold each P_t in doc order;
 *   2. c_t = min(|P_t|, max(1, ceil(r |P_t|))), computed by the caller in float64: cent_cnt [V] int32, cent_ptr [V+1];
 *   3. centroid j = the doc at position floor(j |P_t| / c_t) of P_t in the order of 1. -> cent_doc [ncent];
 *   4. each doc of P_t goes to the centroid of highest s(doc, centroid) (full doc vectors), ties lowest j ->
 *      assign [npruned] (the centroid index, aligned with prune_doc), cent_size [ncent] (docs per centroid);
 *   5. block j = the docs of centroid j in ascending doc id; empty blocks are dropped, the others keep (t, j) order.
 *      snx_seismic_build_blocks writes them to blk_doc [npruned]: cursor [ncent] int64 holds each centroid's block start
 *      (the caller's exclusive scan of cent_size) on entry and its block end on return;
 *   6. per block (blk_ptr [nblocks+1] over blk_doc, empty blocks excluded): m_u = max weight of term u over its docs;
 *      entries sorted by (m desc, u asc); total = fp32 left fold of the m's; the shortest prefix whose fp32 left-fold
 *      sum is >= fp32(alpha) * total (fp32 multiply), at least one entry, stored in ascending term id.  Called twice:
 *      sum_ptr NULL -> sum_cnt [nblocks] = kept entries; then with sum_ptr [nblocks+1] (the caller's scan) -> sum_term /
 *      sum_w.  workspace: snx_seismic_build_workspace_bytes(V, nblocks) bytes.
 * Search (k in [1, 1024], top_n >= 1, heap_factor > 0 fp32, +inf allowed; rows of at most max_q_nnz <= 1024 terms --
 * a longer row is searched as an empty one): Q_cut = the top_n query entries by (weight desc, term asc); H = the top k,
 * in search order, of the docs scored so far with s > 0.  The terms of Q_cut are visited in that order, each term's
 * blocks (term_blk_ptr [V+1] over the blocks) in block order; with r = s(q, summary) (full q) a block is skipped iff
 * |H| == k and heap_factor * r < s_k (fp32 multiply; a NaN product skips nothing), otherwise every doc of the block is
 * scored with s(q, d) and offered to H (a doc already in H is not added again).  Output: H in search order -> out_doc /
 * out_score [nq,k], unused slots doc -1, score 0; target [nq] (or NULL): out_rank = the target's 1-based position in
 * the output (0: absent), out_tscore = s(q, target).  out_stats [nq,3] int64: blocks of the Q_cut lists, blocks scored,
 * docs scored (sum of the scored blocks' sizes).  No workspace. */
size_t snx_seismic_build_workspace_bytes(int32_t V, int64_t nblocks);
int snx_seismic_build_clusters(const int64_t* term_ptr, const int32_t* post_doc, const float* post_w,
                               const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd,
                               int32_t V, int32_t n_postings, const int64_t* prune_ptr, const int32_t* cent_cnt,
                               const int64_t* cent_ptr, int64_t npruned, int64_t ncent, int32_t* prune_doc,
                               float* prune_w, int32_t* cent_doc, int32_t* assign, int32_t* cent_size,
                               hipStream_t stream);
int snx_seismic_build_blocks(const int64_t* prune_ptr, const int32_t* prune_doc, const int32_t* assign,
                             const int64_t* cent_ptr, int32_t V, int64_t npruned, int64_t* cursor, int32_t* blk_doc,
                             hipStream_t stream);
int snx_seismic_build_summaries(const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd,
                                int32_t V, const int64_t* blk_ptr, const int32_t* blk_doc, int64_t nblocks, float alpha,
                                const int64_t* sum_ptr, int32_t* sum_cnt, int32_t* sum_term, float* sum_w,
                                void* workspace, size_t ws_bytes, hipStream_t stream);
int snx_seismic_search(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq, int32_t max_q_nnz,
                       const int64_t* term_blk_ptr, const int64_t* blk_ptr, const int32_t* blk_doc,
                       const int64_t* sum_ptr, const int32_t* sum_term, const float* sum_w, const int64_t* doc_ptr,
                       const int32_t* doc_term, const float* doc_w, int32_t nd, int32_t V, const int32_t* target,
                       int32_t k, int32_t top_n, float heap_factor, int32_t* out_doc, float* out_score,
                       int32_t* out_rank, float* out_tscore, int64_t* out_stats, hipStream_t stream);

/* ---- pruning and two-phase search over the same index (csrc/two_phase.hip): the reference's other serving path, its
 * `rank_features` index behind OpenSearch's neural_sparse_two_phase_processor (ref:benchmark/index_manager.py:197-238:
 * prune_ratio 0.4, expansion_rate 5, max_window_size 10000; :147: it and SEISMIC exclude each other), and the ingest-time
 * prune rules OpenSearch exposes as prune_type = max_ratio | abs_value | top_k | alpha_mass.  The thresholds below are
 * this project's deterministic definitions under OpenSearch's names; OpenSearch's own float arithmetic is not claimed.
 * Prune of one CSR row (ptr [n+1] int64, w [nnz] fp32 > 0; the terms ascend strictly within a row, so position order is
 * term order and the terms themselves are not read); `value` is taken as fp32:
 *   SNX_PRUNE_MAX_RATIO  r in [0, 1]       keep an entry iff w >= fp32(r) * w_max (fp32 multiply); a non-empty row always
 *                                          keeps its maximum;
 *   SNX_PRUNE_ABS_VALUE  a >= 0            keep iff w >= fp32(a); a row may become empty;
 *   SNX_PRUNE_TOP_K      n >= 1, integral  keep the first n entries by (weight desc, term asc) (n above 2^30 counts as 2^30);
 *   SNX_PRUNE_ALPHA_MASS alpha in (0, 1]   rule 6 of the SEISMIC section applied to the row: entries ordered by (weight
 *                                          desc, term asc), total = the fp32 left fold of the weights in that order; keep
 *                                          the shortest prefix whose fp32 left-fold sum is >= fp32(alpha) * total (fp32
 *                                          multiply), at least one entry.
 * Empty rows stay empty.  snx_sparse_prune_rows writes keep [nnz] uint8 (1: kept) and kept_cnt [n] int32; the caller
 * compacts the rows.  max_row_nnz: the caller's bound on the row length (rows of V entries are fine); it sizes the
 * workspace, snx_sparse_prune_workspace_bytes(prune_type, n, max_row_nnz) bytes -- 0 unless alpha_mass has to sort rows
 * that do not fit in LDS, each workgroup then sorts in a slot of its own.  An alpha_mass row longer than the declared
 * bound is not pruned: its keep flags are 0 and its kept_cnt is -1.  Unknown type or value outside its range: SNX_E_ARG.
 * Rescore: cand_doc [nq, W] int32 (1 <= W <= 1024; -1 or any id outside [0, nd): unused slot), k in [1, W].  Every
 * candidate is scored with the full s(q, d) of the exact index (the ascending-term fmaf chain: bit-equal to what
 * snx_sparse_search and snx_sparse_pair_scores return); the candidates with s > 0 are ranked in search order (score
 * descending, ties lowest doc id first), a doc id repeated within a row counts once, the top k go to out_doc /
 * out_score [nq, k], unused slots doc -1, score 0.  target [nq] (or NULL): out_tscore = s(q, target), out_rank = the
 * target's 1-based position in the output, 0 when absent (the SEISMIC search's conventions).  No workspace.
 * Two-phase search is a composition, not an entry point:
 *   Q_high = the kept entries of every query row under a prune (default SNX_PRUNE_MAX_RATIO 0.4);
 *   W = min(floor(k * expansion_rate), max_window_size), computed by the caller in float64, k <= W <= 1024 (the
 *       reference's settings at retrieval size 10: W = 50);
 *   phase 1: C = the out_doc of snx_sparse_search over the Q_high rows with k = W;
 *   phase 2: snx_sparse_rescore of C with the full query rows.
 * Deviation from OpenSearch: Lucene's rescorer adds the low-token partial sum to the phase-1 score; here a window doc
 * gets the exact single-chain s(q, d).  The two are the same number up to fp32 rounding, and this form keeps the rule
 * that every returned score is the exact index's, bit for bit.  Consequences: the output is exactly the top k of C
 * under the exact score; a prune that keeps everything (max_ratio 0) makes the result snx_sparse_search's bit for bit,
 * for any W >= k (there out_rank is the position in the output, 0 below k); a doc that matches only dropped query terms
 * is never found, whatever W -- a property of the method, not of this implementation. */
#define SNX_PRUNE_MAX_RATIO 0
#define SNX_PRUNE_ABS_VALUE 1
#define SNX_PRUNE_TOP_K 2
#define SNX_PRUNE_ALPHA_MASS 3
size_t snx_sparse_prune_workspace_bytes(int32_t prune_type, int32_t n, int32_t max_row_nnz);
int snx_sparse_prune_rows(const int64_t* ptr, const float* w, int32_t n, int64_t nnz, int32_t max_row_nnz,
                          int32_t prune_type, float value, uint8_t* keep, int32_t* kept_cnt, void* workspace,
                          size_t ws_bytes, hipStream_t stream);
int snx_sparse_rescore(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                       const int32_t* cand_doc, int32_t W, const int64_t* doc_ptr, const int32_t* doc_term,
                       const float* doc_w, int32_t nd, const int32_t* target, int32_t k, int32_t* out_doc,
                       float* out_score, int32_t* out_rank, float* out_tscore, hipStream_t stream);

/* ---- BM25 baseline and rank fusion (csrc/hybrid.hip): the lexical baseline the reference quotes every number against
 * (ref:huggingface/v33/README.md:189-233) and the fusion of ranked lists from several retrievers
 * (ref:benchmark/score_fusion.py, ref:benchmark/hybrid_searcher.py:501-522, ref:scripts/run_7way_benchmark.py).
 * Term counts: input_ids, attention_mask [n, S] int64 (what the tokenizer yields), allowed [V] uint8.  A position COUNTS
 * when its mask is non-zero, 0 <= id < V and allowed[id] != 0.  Per row: out_term [n, S] int32 = the distinct counted ids
 * strictly ascending, out_tf [n, S] int32 = their occurrence counts (unused slots: term -1, tf 0), out_cnt [n] = distinct
 * ids, out_len [n] = counted positions = sum of tf.  Integer exact.  1 <= S <= snx_term_counts_max_len() = 8192 (the
 * model's position limit; the row is sorted in LDS), beyond: SNX_E_SHAPE.
 * Document frequencies: df [V] int32, df[t] += the number of entries of term [nnz] equal to t -- over CSR rows, whose
 * terms are distinct within a row, the number of rows that contain t.  Integer atomics: exact, order-independent; it
 * ADDS, so batches accumulate (the caller zeroes df once).  Entries outside [0, V) are skipped.
 * BM25 weights, elementwise over a CSR (ptr [n+1] int64, term / tf [nnz] int32, dl [n] int32 = out_len), in float64 with
 * every operation rounded on its own (no fma contraction):
 *   norm_d = k1 * ((1.0 - b) + b * ((double)dl_d / avgdl))
 *   w(t,d) = (float)( idf[t] * ((double)tf / ((double)tf + norm_d)) )
 * idf [V] float64 is the caller's: numpy.log1p((N - df + 0.5) / (df + 0.5)) evaluated on the host (the `bm25` smoothing
 * of ref:tools/idf-compute/src/main.rs:202, Lucene's form; libm logs are not bit-reproducible across implementations and
 * the table has V entries); avgdl = the exact integer sum of dl over N, in float64, by the caller.  k1 >= 0 (default
 * 1.2), b in [0, 1] (default 0.75), avgdl > 0 when there are entries; otherwise SNX_E_ARG.  The BM25 score of a query is
 * s(q, d) of the exact index over these weights with query weights fp32(count): every guarantee of that section holds.
 * Deviations from OpenSearch: like Lucene >= 8 the (k1 + 1) factor is dropped; Lucene quantises the document length to
 * one byte, this form does not; the analyzer is the model's own tokenizer, not `nori`; lengths are taken after the
 * caller's truncation (the evaluator's doc_max_length); OpenSearch's numbers are not claimed.
 * Rank fusion: docs [L, nq, R] int32, scores [L, nq, R] fp32 (NULL allowed unless SNX_FUSE_LINEAR), 1 <= L <= 4, 1 <= R
 * <= 1024.  List l of query q = the leading entries of docs[l, q, :] up to the first negative doc id; the rank of an entry
 * is its position + 1.  Precondition: doc ids distinct within a list (search outputs are); a violation reads and writes
 * nothing out of bounds, its result is otherwise unspecified.  max_rank = max(len_0 + 1, ..., len_{L-1} + 1, 100) per
 * query; a doc absent from a list takes this rank.  All arithmetic is float64, every operation rounded on its own, in
 * the reference's operand order -- fused scores equal ref:benchmark/score_fusion.py and the triple RRF of
 * ref:benchmark/hybrid_searcher.py:501-522 bit for bit.  params [host] float64:
 *   SNX_FUSE_RRF           {k}: left fold over the lists, in list order, of 1.0 / (k + rank_l);
 *   SNX_FUSE_WEIGHTED_RRF  {k, w_0 .. w_{L-1}}: the same fold of w_l / (k + rank_l);
 *   SNX_FUSE_LINEAR        {alpha}, L == 2: per list min-max over its own scores widened to double, (s - min) / (max -
 *                          min), 1.0 for every entry when all scores are equal, 0.0 for an absent doc; fused = alpha * a
 *                          + (1.0 - alpha) * b (two products, one sum), list 0 weighted by alpha.
 * k >= 0 finite, w_l finite, alpha in [0, 1]; a violation, L out of range, an unknown method or linear with L != 2:
 * SNX_E_ARG.  R or top_k (1 <= top_k <= 4096) out of range: SNX_E_SHAPE.  The union of the lists is ordered by fused
 * score descending, ties lowest doc id first (the reference leaves ties to Python's set iteration; this rule is the
 * project's, as everywhere); the first top_k go to out_doc [nq, top_k] int32 / out_score [nq, top_k] float64, unused
 * slots doc -1, score 0; out_total [nq] = the size of the union (the reference's total_hits); target [nq] (or NULL):
 * out_rank = the target's 1-based position in the whole fused order, 0 when it is in no list.  No workspace. */
#define SNX_FUSE_RRF 0
#define SNX_FUSE_WEIGHTED_RRF 1
#define SNX_FUSE_LINEAR 2
int32_t snx_term_counts_max_len(void);
int snx_term_counts(const int64_t* input_ids, const int64_t* attention_mask, const uint8_t* allowed, int32_t n, int32_t S,
                    int32_t V, int32_t* out_term, int32_t* out_tf, int32_t* out_cnt, int32_t* out_len,
                    hipStream_t stream);
int snx_bm25_doc_freq(const int32_t* term, int64_t nnz, int32_t V, int32_t* df, hipStream_t stream);
int snx_bm25_weights(const int64_t* ptr, const int32_t* term, const int32_t* tf, const int32_t* dl, const double* idf,
                     int32_t n, int64_t nnz, int32_t V, double avgdl, double k1, double b, float* w, hipStream_t stream);
int snx_fuse_ranked(const int32_t* docs, const float* scores, int32_t L, int32_t nq, int32_t R, int32_t method,
                    const double* params /*[host]*/, const int32_t* target, int32_t top_k, int32_t* out_doc,
                    double* out_score, int32_t* out_total, int32_t* out_rank, hipStream_t stream);

/* ---- relevance judgments (csrc/qrels.hip): scoring against qrels with several relevant docs per query, the protocol of
 * the reference's headline numbers (ref:benchmark/hf_data_loader.py:21 query_relevant_docs; ref:benchmark/hf_runner.py:
 * 191-215: a hit is the first retrieved doc that is in the query's relevant SET; ref:benchmark/metrics.py:180-215: the
 * bootstrap interval).  A relevance row set is a CSR pair: rel_ptr [nq+1] int64, rel_doc [n] int32, every row ascending
 * and distinct (a violation reads and writes nothing out of bounds, its result is otherwise unspecified).  Ids outside
 * [0, nd) are skipped, never read through.
 * First relevant: query CSR, doc CSR and term-major index as for snx_sparse_search, s(q,d) the score of the "exact sparse
 * retrieval" section.  Per query the BEST RELEVANT DOC d* is the in-range row member with the highest s(q,d) > 0, ties
 * lowest doc id.  out_doc [nq] = d* (-1: none), out_score [nq] = s(q,d*) (0 when none), bit-equal to what
 * snx_sparse_search ranks; out_rank [nq] = 1 + #{d: s_d > s*} + #{d < d*: s_d == s*} over the WHOLE corpus, 0 when no
 * relevant doc scores > 0 -- the minimum over the row of snx_sparse_search's single-target out_rank; out_nrel [nq] = row
 * members in range.  One score accumulation per query whatever the row length; stream-ordered, no host synchronisation.
 * chunk_docs as for the search (0: default; <= 32768): it changes no bit.
 * workspace: snx_sparse_first_relevant_workspace_bytes(nq, nd, chunk_docs) bytes.
 * Ranked relevance: docs [nq, R] int32, 1 <= R <= 4096, any ranked lists (search, rescore, SEISMIC, fusion outputs); a list
 * ends at its first negative id, the position of an entry is its index + 1, an entry is RELEVANT when it lies in [0, nd)
 * and in the query's row (binary search); a doc id repeated in a list counts at every position.  cutoffs [host] int32,
 * 1 <= ncut <= 8 entries, strictly ascending, each in [1, R]; disc [R] float64 is the caller's device table, disc[p-1] the
 * discount of position p: the Python layer fills it with 1.0 / numpy.log2(p + 1) -- the kernel computes no logarithm (libm
 * is not bit-reproducible; snx_bm25_weights treats idf the same way).  out_first [nq] = position of the first relevant
 * entry of the whole list, 0 if none; out_hits [nq, ncut] int32 = relevant entries at positions <= cutoffs[j];
 * out_dcg [nq, ncut] float64 = the left fold from +0.0, in position order, of disc[p-1] over the relevant positions
 * p <= cutoffs[j], every add rounded on its own.  One wave per list: the launch geometry changes no bit.  Cutoffs out of
 * range or not ascending, ncut out of range: SNX_E_ARG; R out of range: SNX_E_SHAPE.  No workspace.
 * Bootstrap means: values [n, M] float64 (1 <= M <= 16), idx [nboot, n] int32 (resample b draws rows idx[b, 0..n));
 * out [nboot, M] float64, out[b,m] = (sum over i of values[idx[b,i], m]) / (double)n.  THE SUMMATION ORDER IS PART OF THE
 * ABI: i = 0 .. n-1 is cut into segments of SNX_BOOTSTRAP_SEGMENT = 64 consecutive positions (the last may be shorter);
 * inside a segment the terms are added in ascending i, a left fold starting from +0.0; the segment sums are then added in
 * ascending segment order, again a left fold from +0.0; one IEEE division by (double)n ends it.  Every add is rounded on
 * its own.  Bit-identical from run to run and independent of the launch shape.  Precondition: every index lies in [0, n).
 * The kernel does not read through an index outside the range (the term is left out), but it cannot report it without a
 * host synchronisation: the caller checks the indices where they are drawn (snx.retrieval.bootstrap_means does, and
 * raises the SNX_E_ARG error).  n < 1, M out of range, nboot < 0: SNX_E_SHAPE.  No workspace. */
#define SNX_BOOTSTRAP_SEGMENT 64
size_t snx_sparse_first_relevant_workspace_bytes(int32_t nq, int32_t nd, int32_t chunk_docs);
int snx_sparse_first_relevant(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                              const int64_t* term_ptr, const int32_t* post_doc, const float* post_w,
                              const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd, int32_t V,
                              const int64_t* rel_ptr, const int32_t* rel_doc, int32_t chunk_docs, int32_t* out_doc,
                              float* out_score, int32_t* out_rank, int32_t* out_nrel, void* workspace, size_t ws_bytes,
                              hipStream_t stream);
int snx_ranked_relevance(const int32_t* docs, int32_t nq, int32_t R, int32_t nd, const int64_t* rel_ptr,
                         const int32_t* rel_doc, const int32_t* cutoffs /*[host]*/, int32_t ncut, const double* disc,
                         int32_t* out_first, int32_t* out_hits, double* out_dcg, hipStream_t stream);
int snx_bootstrap_means(const double* values, int32_t n, int32_t M, const int32_t* idx, int32_t nboot, double* out,
                        hipStream_t stream);

/* ---- exact dense retrieval (csrc/dense.hip): what the reference does with dense teacher embeddings -- the teacher
 * scores of ref:scripts/precompute_teacher_scores.py:162-224, the hard-negative search of
 * ref:scripts/mine_multi_negatives.py:141-222 (torch.mm into a [4096, n_docs] matrix, then torch.topk) and the
 * SemanticSearcher of ref:benchmark/searchers.py:97-127.  No [nq, nd] score buffer exists here.
 * Operands: docs E [nd, D] and queries Q [nq, D], fp32, row-major, every value finite; 1 <= D <= 4096; nd < 2^31.
 * Score definition (part of the ABI, bit-reproducible): s(q,d) = fp32 acc starting at +0, acc = fmaf(Q[q,j], E[d,j], acc)
 * for j = 0 .. D-1 ascending, then acc + 0.0f (a -0, which arises when a negative product underflows, becomes +0).  The
 * search computes this chain on v_mfma_f32_32x32x2_f32, the pair scores by a serial fmaf loop: the same bits.  The
 * results are defined while every partial sum stays finite.
 * Order: score descending as real numbers, ties lowest doc id first.  EVERY doc is a candidate: negative and zero scores
 * rank like any other (no score > 0 rule, unlike the sparse search).
 * Search: per query the top k (1 <= k <= 1024) -> out_doc / out_score [nq,k]; unused slots (k > nd) doc -1, score 0.
 * target [nq] (or NULL): out_tscore [nq] = s(q, target), bit-equal to the ranked value, out_rank [nq] = 1 + #{d: s_d >
 * s_t} + #{d < t: s_d == s_t} (>= 1 for a target in [0, nd); 0 and score 0 for one out of range).  chunk_docs: docs per
 * split of the doc range (0: default; otherwise >= 128, rounded up to a multiple of 128); neither it nor any slicing of
 * the queries changes a bit.  workspace: snx_dense_search_workspace_bytes(nq, nd, k, chunk_docs) bytes -- it grows with
 * nq * k * splits, never with nq * nd.
 * Band search: exclusion rows and ceiling as for snx_sparse_search_band.  Doc d is ADMISSIBLE for q when it is not in
 * the row and s(q,d) < ceiling[q] (strict, fp32; NULL or +inf admits all, a NaN ceiling nothing); ranks lo .. hi-1
 * (0 <= lo < hi <= 1024) of the admissible docs go to out_doc / out_score [nq, hi-lo], unused slots doc -1, score 0;
 * out_found [nq] = filled slots.  workspace: snx_dense_search_band_workspace_bytes(nq, nd, hi, chunk_docs) bytes.
 * Pair scores: out[i] = s(pair_q[i], pair_d[i]); a pair with an index out of range scores 0. */
size_t snx_dense_search_workspace_bytes(int32_t nq, int32_t nd, int32_t k, int32_t chunk_docs);
int snx_dense_search(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D, const int32_t* target, int32_t k,
                     int32_t chunk_docs, int32_t* out_doc, float* out_score, int32_t* out_rank, float* out_tscore,
                     void* workspace, size_t ws_bytes, hipStream_t stream);
size_t snx_dense_search_band_workspace_bytes(int32_t nq, int32_t nd, int32_t hi, int32_t chunk_docs);
int snx_dense_search_band(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D, const int64_t* ex_ptr,
                          const int32_t* ex_doc, const float* ceiling, int32_t lo, int32_t hi, int32_t chunk_docs,
                          int32_t* out_doc, float* out_score, int32_t* out_found, void* workspace, size_t ws_bytes,
                          hipStream_t stream);
int snx_dense_pair_scores(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D, const int32_t* pair_q,
                          const int32_t* pair_d, int64_t npairs, float* out, hipStream_t stream);

/* ---- two-phase dense retrieval (csrc/dense_two_phase.hip): the result of the exact dense section with most of the work
 * on the bf16 MFMA.  Phase 1 scores bf16 copies of the operands and proposes k1 candidates per query; phase 2 scores the
 * candidates by the exact section's chain on the fp32 operands; a per-query certificate proves, from norms computed once,
 * that phase 1 hid no better doc.  Operands as in the exact section (fp32, finite, 1 <= D <= 4096, nd < 2^31).
 * snx_dense2_prepare (once per operand): X [n, D] fp32 -> Xb [n, Dp] bf16 bits, Dp = D rounded up to a multiple of 32,
 * xhat = x rounded to nearest even (a value past the bf16 range becomes an infinity), columns D .. Dp-1 zero; and per row,
 * in float64, norm2 = sum x^2, hat2 = sum xhat^2, res2 = sum (x - xhat)^2, each a left fold over ascending j from 0.0
 * (every square is exact in float64, so each array is bit-reproducible).  Xb must be 16-byte aligned.
 * snx_dense2_scan: a(q, d) = the fp32 accumulation of qhat[j] * dhat[j] on v_mfma_f32_32x32x16_bf16, k-steps of 16 in
 * ascending order, then + 0.0f: a pure function of the two bf16 rows.  Per query the k1 best docs (1 <= k1 <= 1024) by
 * a, descending, ties lowest doc id first -> cand_doc / cand_approx [nq, k1]; unused slots (k1 > nd) doc -1, score 0.
 * Neither chunk_docs (as in the exact section) nor any slicing of the queries changes a bit.
 * workspace: snx_dense2_workspace_bytes(nq, nd, k1, chunk_docs) bytes.
 * snx_dense2_rescore: for every candidate s(q, d) of the exact section, bit for bit; a candidate is ADMISSIBLE under the
 * rules of snx_dense_search_band (ex_ptr / ex_doc / ceiling, each may be NULL); ranks lo .. hi-1 (0 <= lo < hi <= k1) of the
 * admissible candidates, score descending, ties lowest doc id first -> out_doc / out_score [nq, hi-lo], unused slots doc
 * -1, score 0; out_found [nq] = filled slots.  q_norm2 / q_hat2 / q_res2 [nq]: the queries' arrays from
 * snx_dense2_prepare; doc_norm, doc_hat, doc_res: the maxima over the docs of sqrt(norm2), sqrt(hat2), sqrt(res2).
 * certified [nq] (uint8).  With n_q, nh_q, r_q the square roots of the query's three values, Dp as above,
 *   g23 = m / (1 - m) for m = 2 Dp 2^-23,   g24 = m / (1 - m) for m = D 2^-24,
 *   eps = (n_q doc_res + r_q doc_hat + g23 nh_q doc_hat + g24 n_q doc_norm) (1 + 2^-20) + D 2^-100 (1 + nh_q + doc_hat)
 * and t = cand_approx[q, k1-1], every doc d outside the candidates has s(q, d) <= t + eps.  certified[q] = 1 when nd <= k1,
 * or when out_found[q] == hi - lo and the score of rank hi-1 is > t + eps (float64, strict); it is 0 otherwise, and always
 * 0 when one of the six norms, a candidate's s or a candidate's a is not finite, or when n_q doc_norm or nh_q doc_hat
 * exceeds 2^127 (the bound takes every product and partial sum of both passes to stay inside the fp32 range).  A certified row equals
 * snx_dense_search's (snx_dense_search_band's with the same exclusions and ceiling) bit for bit, ties included. */
int snx_dense2_prepare(const float* X, int32_t n, int32_t D, uint16_t* Xb, double* norm2, double* hat2, double* res2,
                       hipStream_t stream);
size_t snx_dense2_workspace_bytes(int32_t nq, int32_t nd, int32_t k1, int32_t chunk_docs);
int snx_dense2_scan(const uint16_t* Qb, int32_t nq, const uint16_t* Eb, int32_t nd, int32_t D, int32_t k1,
                    int32_t chunk_docs, int32_t* cand_doc, float* cand_approx, void* workspace, size_t ws_bytes,
                    hipStream_t stream);
int snx_dense2_rescore(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D, const int32_t* cand_doc,
                       const float* cand_approx, int32_t k1, const double* q_norm2, const double* q_hat2,
                       const double* q_res2, double doc_norm, double doc_hat, double doc_res, const int64_t* ex_ptr,
                       const int32_t* ex_doc, const float* ceiling, int32_t lo, int32_t hi, int32_t* out_doc,
                       float* out_score, int32_t* out_found, uint8_t* certified, hipStream_t stream);

/* ---- IVF-Flat dense retrieval (csrc/ivf.hip): the approximate index of the reference's dense hard-negative miner, which
 * builds faiss.IndexIVFFlat over BGE-M3 embeddings and searches it with FAISS's default nprobe
 * (ref:src/preprocessing/miners/bge_m3_miner.py:91-136, 166-249).  The lists here are this index's own (deterministic
 * spherical k-means, below), not FAISS's: FAISS's sampling and random generator are not reproduced.
 * Definition.  s(x, y) is the score of the section above (the fp32 fmaf chain over ascending dimensions from +0, then
 * + 0.0f), with the same bits.  Given centroids C [nlist, D] (fp32, finite; 1 <= nlist <= 65536):
 *   list(d) = argmax_c s(E[d], C[c]), ties to the lowest c;
 *   P(q)    = the nprobe best centroids by s(q, C[c]), ties to the lowest c (1 <= nprobe <= min(nlist, 1024));
 *   result  = the top k (score descending, ties lowest ORIGINAL doc id first) over {d : list(d) in P(q)}, scores s(q, E[d]);
 *             unused slots doc -1, score 0;
 *   band    = ranks lo .. hi-1 of the ADMISSIBLE docs of that set (not in the exclusion row, s < ceiling[q]; the rules of
 *             snx_dense_search_band), out_found [nq] = filled slots.
 * Hence nprobe == nlist gives snx_dense_search's result, nprobe < nlist gives snx_dense_search_band's with the docs of the
 * lists outside P(q) excluded, and every score equals snx_dense_pair_scores'.  No result depends on how the queries are
 * sliced, on the workspace, on split_docs (how a long list is split over workgroups) or on how the docs arrived.
 * Both list rules are snx_dense_search over the centroids (k = 1 with the docs as queries; k = nprobe with the queries):
 * the caller runs it and hands the ids over (doc_list [nd]; probe [nq, nprobe], every entry in [0, nlist), no list twice
 * in a row).
 * snx_ivf_build: a stable counting sort of the docs by list -> list_ptr [nlist+1] int64, list_doc [nd] int32 (original
 * ids, ascending inside a list) and, when E_sorted is not NULL, E_sorted [nd, D] = the rows of E in list order.
 * workspace: snx_ivf_build_workspace_bytes(nd, nlist) bytes.
 * snx_ivf_search: lo = 0, hi = k is the plain search (ex_ptr, ceiling, out_found may be NULL).  max_list: an upper bound
 * of the longest list (the caller reads it once after the build; a smaller value is memory-safe and leaves docs
 * unscanned).  split_docs: docs per split of a list (0: default; otherwise >= 128, rounded up to a multiple of 128).
 * workspace: snx_ivf_search_workspace_bytes(nq, nd, nlist, nprobe, hi, max_list, split_docs) bytes; it grows with
 * nq * nprobe * splits * hi, never with nd.
 * snx_ivf_kmeans_update: one step of spherical k-means.  list_ptr / list_row: the training rows X [n, D] sorted by their
 * centroid (snx_ivf_build of the assignment with E_sorted NULL).  For centroid c with members r_0 < r_1 < ... and
 * dimension j: the float64 sum of X[r, j] in this FIXED order -- members ascending, serially inside segments of 1024
 * consecutive members (starting from 0.0), the segment sums added in ascending segment order (starting from 0.0); the sum
 * is divided by the member count in float64; the mean vector is divided, in float64, by the sqrt of its sum of squares
 * (serial over ascending j from 0.0, each square rounded before it is added); the quotient is rounded to fp32.  A zero
 * mean stays all zeros; a centroid without members keeps C_prev's row.  No float atomics, no dependence on the launch.
 * The initial centroids of snx.retrieval.IvfFlatIndex are this update applied to single-member lists of the rows
 * numpy.random.RandomState(seed).permutation(n)[:nlist]. */
size_t snx_ivf_build_workspace_bytes(int32_t nd, int32_t nlist);
int snx_ivf_build(const int32_t* doc_list, int32_t nd, int32_t nlist, const float* E, int32_t D, int64_t* list_ptr,
                  int32_t* list_doc, float* E_sorted, void* workspace, size_t ws_bytes, hipStream_t stream);
int snx_ivf_kmeans_update(const float* X, int32_t n, int32_t D, const int64_t* list_ptr, const int32_t* list_row,
                          int32_t nlist, const float* C_prev, float* C_out, hipStream_t stream);
size_t snx_ivf_search_workspace_bytes(int32_t nq, int32_t nd, int32_t nlist, int32_t nprobe, int32_t hi, int32_t max_list,
                                      int32_t split_docs);
int snx_ivf_search(const float* Q, int32_t nq, int32_t D, const float* E_sorted, const int64_t* list_ptr,
                   const int32_t* list_doc, int32_t nd, int32_t nlist, int32_t max_list, const int32_t* probe,
                   int32_t nprobe, const int64_t* ex_ptr, const int32_t* ex_doc, const float* ceiling, int32_t lo,
                   int32_t hi, int32_t split_docs, int32_t* out_doc, float* out_score, int32_t* out_found, void* workspace,
                   size_t ws_bytes, hipStream_t stream);

/* ---- graph dense retrieval (csrc/graph.hip): an approximate inner-product top-k in the ROLE of the HNSW field behind the
 * reference's dense benchmark rows (ref:benchmark/index_manager.py:98-110: "hnsw", faiss, innerproduct, ef_construction
 * 128, m 16; queried by ref:benchmark/searchers.py:97-127 and the dense legs of hybrid_searcher.py).  It is NOT FAISS's
 * graph: FAISS inserts sequentially with a random level per point.  This is a deterministic fixed-degree graph of the
 * CAGRA family -- kNN lists, rank-based pruning, reverse edges, a best-first beam -- and every result is a pure function
 * of the embeddings and the parameters.
 * Definition.  s(x, y) is the score of the exact dense section, with the same bits.  E [nd, D] fp32 finite, 1 <= D <= 4096,
 * nd < 2^31.
 *   Neighbour lists  N [nd, knn] int32, degree <= knn <= 128: N[u] = the min(knn, nd-1) docs x != u with the best
 *     s(E[u], E[x]), ties to the lowest id, the rest of the row -1.  This is snx_dense_search_band with lo = 0, hi = knn and
 *     the one-entry exclusion row {u}: the caller runs it and hands the ids over (or lists from elsewhere: every row
 *     distinct ids in [0, nd) other than u, then -1).
 *   Detours  With v_0 .. v_{K-1} the valid entries of N[u] and rank_w(x) the column of x in N[w] (infinity when absent):
 *     detour(u, j) = #{ i < j : rank_{v_i}(v_j) < j }, the two-hop routes u -> v_i -> v_j whose two edges both rank better
 *     than the direct edge (CAGRA's rule).
 *   Forward list  F[u] = the ids v_j of the min(degree, K) columns j with the smallest (detour(u, j), j), in that order.
 *   Reverse list  R[v] = the pairs (p, u) with F[u][p] == v, ordered by (p, u) ascending, the first `degree` kept.
 *   Graph  G [nd, degree] int32: G[v] = the first `degree` distinct ids of F[v][0], R[v][0], F[v][1], R[v][1], ...; when one
 *     list runs out the other continues; padded with -1.  Integers only: no float arithmetic, and no atomic whose order
 *     shows in the result.
 *   Entry sample  entry_i = floor(i * nd / nentry), i = 0 .. nentry-1, in int64; nentry clamped to [min(ef, nd), nd]
 *     (snx.retrieval.GraphIndex's default: 4 * ceil(sqrt(nd))).
 *   Seeds  the best min(ef, nentry) docs of the entry sample by s(q, E[entry_i]), ties to the lowest doc id: snx_dense_search
 *     over the gathered entry rows, run by the caller, ids mapped back -> seeds [nq, nseed] int32 (distinct docs; an id
 *     outside [0, nd) is skipped).  The kernel scores the seeds itself, to the same bits.
 *   Walk  1 <= ef <= 1024, 1 <= width <= 8, max_iter >= 0 (0: no cap).  The pool P holds at most ef entries (score, doc,
 *     expanded), score descending, doc ascending; it starts as the seeds, all unexpanded.  One iteration: take the first
 *     `width` unexpanded entries of P in pool order and mark them expanded; walk their G rows in parent order, then column
 *     order; drop -1, every doc already scored for this query (seeds included) and all but the first occurrence of a doc
 *     inside the batch; score the rest; merge into P and keep the best ef.  The walk stops when P has no unexpanded entry
 *     or after max_iter iterations; out_iters [nq] (or NULL) = iterations run.
 *   Result  search: lo = 0, hi = k <= ef: ranks 0 .. k-1 of P.  Band: ranks lo .. hi-1 (hi <= ef) of the ADMISSIBLE entries
 *     of the final P (not in the exclusion row, s < ceiling[q]: the rules and operands of snx_dense_search_band).  The band
 *     filter applies to the output only: the walk does not see it.  Unused slots doc -1, score 0; out_found [nq] (or NULL)
 *     = filled slots.
 * The kernel's visited filter is a bounded table that stores full doc ids and may forget; it never reports an unscored doc
 * as scored, and a doc scored twice cannot change P (a scored doc outside P lies below the worst entry of a full P, which
 * only rises; one inside P is found by its key).  Hence ef >= nd (every doc a seed) gives snx_dense_search's result bit
 * for bit, every returned score equals snx_dense_pair_scores', and no result depends on how the queries are sliced, on
 * the workspace or on how the docs arrived.
 * snx_graph_optimize: N -> G, and F [nd, degree] when `forward` is not NULL.  workspace:
 * snx_graph_optimize_workspace_bytes(nd, knn, degree) bytes.  snx_graph_search: workspace
 * snx_graph_search_workspace_bytes(nq, ef, width, degree) bytes (the final pools); it grows with nq * ef, never with nd. */
size_t snx_graph_optimize_workspace_bytes(int32_t nd, int32_t knn, int32_t degree);
int snx_graph_optimize(const int32_t* neighbors, int32_t nd, int32_t knn, int32_t degree, int32_t* graph, int32_t* forward,
                       void* workspace, size_t ws_bytes, hipStream_t stream);
size_t snx_graph_search_workspace_bytes(int32_t nq, int32_t ef, int32_t width, int32_t degree);
int snx_graph_search(const float* Q, int32_t nq, int32_t D, const float* E, int32_t nd, const int32_t* graph,
                     int32_t degree, const int32_t* seeds, int32_t nseed, int32_t ef, int32_t width, int32_t max_iter,
                     const int64_t* ex_ptr, const int32_t* ex_doc, const float* ceiling, int32_t lo, int32_t hi,
                     int32_t* out_doc, float* out_score, int32_t* out_found, int32_t* out_iters, void* workspace,
                     size_t ws_bytes, hipStream_t stream);

/* ---- MinHash near-duplicate removal (csrc/minhash.hip): the reference's MinHashDeduplicator
 * (ref:src/preprocessing/cleaners/deduplicator.py:10-187), whose two Python loops -- num_perm MD5 digests per character
 * n-gram (ref:deduplicator.py:71-80) and every new row against every kept row (ref:deduplicator.py:135-138) -- keep the
 * reference's own pipeline from using it (ref:src/preprocessing/pipeline.py:112).  Everything here is integer work and
 * every result equals the reference's bit for bit.
 * Signatures: rows are a CSR of Unicode code points, ptr [n+1] int64 and code_points int32, already lowered and stripped
 * by the host (ref:deduplicator.py:50).  The n-grams of a row are its windows of ngram_size code points; a row shorter
 * than ngram_size, the empty one included, has the single n-gram that is the whole row (ref:deduplicator.py:51-52).
 * sig [n, num_perm, 4] uint32: entry i is the minimum over the n-grams of int(md5(f"{i}_{ngram}".encode()).hexdigest(),
 * 16) (ref:deduplicator.py:76-77), the 128-bit digest read big-endian, stored MOST SIGNIFICANT WORD FIRST: comparing the
 * four words in order is the integer comparison.  The kernel encodes UTF-8, writes the decimal prefix, pads ONE 64-byte
 * MD5 block and hashes it.  Precondition: every message (prefix, underscore and the n-gram's UTF-8 bytes) is at most
 * SNX_MINHASH_MSG_MAX = 55 bytes; a longer one is hashed truncated (nothing is read or written out of bounds, the value
 * is unspecified) -- snx.minhash computes the batch's longest message and refuses it.  1 <= num_perm <=
 * SNX_MINHASH_PERM_MAX = 256 (prefixes of at most three digits), ngram_size >= 1; otherwise SNX_E_SHAPE.
 * Greedy removal (ref:deduplicator.py:112-144, 164-168): rows are taken in order; row i is a DUPLICATE iff an earlier
 * KEPT row has the same exact-key group, or an earlier KEPT row's signature equals its own at `need` positions or more
 * (all 128 bits of a position); dropped rows are never compared against.  `need` is the host's integer form of
 * `matches / num_perm >= threshold` (need <= 0: every kept row matches; need > num_perm: none does).  group [n] int32 or
 * NULL: the host's id in [0, n) of the row's exact key (ref:deduplicator.py:109-110).  duplicate_of [n] int32: -1 for a
 * kept row; for a dropped one the kept row with its group when there is one, otherwise the smallest kept index that
 * reaches `need` -- the first row the reference's loop meets.  The order dependence is resolved in blocks of 512 rows: one
 * launch compares a block with the kept rows of all earlier blocks (compacted) and with itself, one workgroup then walks
 * the block in order.  A 32-bit prefilter on the least significant word picks candidates; the count over all 128 bits
 * decides.  Stream-ordered, no host synchronisation, no kernel waits for another workgroup.
 * workspace: snx_minhash_dedup_workspace_bytes(n, num_perm) bytes.
 * First match (the incremental form, ref:deduplicator.py:112-144 called row by row): q_sig [nq, num_perm, 4] against
 * kept_sig [nk, num_perm, 4] -> out [nq] int32 = the smallest k whose signature reaches `need`, -1 when none; nq <= 65535. */
#define SNX_MINHASH_MSG_MAX 55
#define SNX_MINHASH_PERM_MAX 256
int snx_minhash_signatures(const int64_t* ptr, const int32_t* code_points, int32_t n, int32_t ngram_size,
                           int32_t num_perm, uint32_t* sig, hipStream_t stream);
size_t snx_minhash_dedup_workspace_bytes(int32_t n, int32_t num_perm);
int snx_minhash_dedup(const uint32_t* sig, int32_t n, int32_t num_perm, int32_t need, const int32_t* group,
                      int32_t* duplicate_of, void* workspace, size_t ws_bytes, hipStream_t stream);
int snx_minhash_first_match(const uint32_t* q_sig, int32_t nq, const uint32_t* kept_sig, int32_t nk, int32_t num_perm,
                            int32_t need, int32_t* out, hipStream_t stream);

/* ---- Corpus preparation (csrc/textprep.hip): the reference's MLM data script (ref:scripts/prepare_korean_mlm_data.py),
 * whose clean_text -> split_paragraphs -> is_valid_paragraph (ref:prepare_korean_mlm_data.py:31-53) and SHA-256 dedup
 * (ref:prepare_korean_mlm_data.py:56-58, 201-217) are single-threaded Python loops over tens of millions of paragraphs.
 * Everything here is integer work and every output is a pure function of the inputs, bit for bit, run to run.  Rows are
 * a CSR of Unicode code points as for the MinHash section, ptr [n+1] int64 and code_points int32, NOT lowered and NOT
 * stripped; every document is shorter than 2^31 code points.
 * Segmentation, per document (nothing carries from one document into the next):
 *   blank      U+0020 or U+0009; one whose predecessor is a blank is dropped, a kept one is emitted as U+0020
 *              (ref:prepare_korean_mlm_data.py:33).
 *   separator  a maximal run of U+000A of length >= 2 (ref:prepare_korean_mlm_data.py:34, 40); it is removed and cuts
 *              the document into pieces.  A single U+000A stays in the text.
 *   strip      the white space of Python's str.isspace (0009-000D 001C-0020 0085 00A0 1680 2000-200A 2028 2029 202F 205F
 *              3000, a compile-time range test) is removed from both ends of a piece; an empty piece is dropped
 *              (ref:prepare_korean_mlm_data.py:35, 40).  A piece is emitted from its first to its last code point that
 *              is not white space.
 *   hangul     counts U+AC00 .. U+D7AF inclusive (ref:prepare_korean_mlm_data.py:20).
 * One workgroup per document walks tiles of 256 code points; the blank and separator tests read the neighbouring code
 * points of the document, the piece state (last separator, first and last non-white-space position, running counts)
 * is carried from tile to tile.  Three passes, because a trailing white-space run is known to be trailing only at the
 * piece's end:
 *   snx_tx_segment_count  doc_pieces [n] int64 = surviving pieces of the document, doc_cps [n] int64 = their code points.
 *                         The host scans doc_pieces into piece_base [n+1] (0 and the running sums) and reads the two totals.
 *   snx_tx_segment_meta   for piece k of document d, at p = piece_base[d] + k: par_len [np] int64, par_doc [np] int32 = d,
 *                         par_hangul [np] int32.  The host scans par_len into par_ptr [np+1].
 *   snx_tx_segment_fill   par_cps [par_ptr[np]] int32: a code point is written iff its offset in the piece is below the
 *                         piece's length, which cuts the trailing white space without looking ahead.
 * SHA-256 of rows: digest [n, 8] uint32 = SHA-256 of the row's UTF-8 bytes (ref:prepare_korean_mlm_data.py:58), MOST
 * SIGNIFICANT WORD FIRST as the MinHash signatures: the eight words as %08x are hexdigest().  UTF-8 is encoded on the fly
 * into 64-byte blocks (a code point's bytes may straddle two), any length, 64-bit bit count; the empty row hashes the
 * empty message.  A value outside [0, 0x10FFFF] or a surrogate is encoded by the same bit rule (the host refuses them).
 * One lane per row: a wave takes as long as its longest row.
 * First-occurrence dedup (ref:prepare_korean_mlm_data.py:210-216): first [n] int32 = the smallest row index whose digest
 * equals row i's in all 256 bits, i itself for a first occurrence.  An open-addressed table of the power of two >= 2 n
 * slots of row indices: a row claims a free slot by compare-and-swap, or finds a slot whose row has its digest (compared
 * through the digest array), and lowers the slot to its own index by atomicMin; a second pass reads the minima.  Rows of
 * equal digest end in the same slot whatever the arrival order, so the result does not depend on it.  n <= 2^29;
 * workspace: snx_tx_first_equal_workspace_bytes(n) bytes.  Stream-ordered, no host synchronisation, no kernel waits for
 * another workgroup. */
int snx_tx_segment_count(const int64_t* ptr, const int32_t* code_points, int32_t n, int64_t* doc_pieces, int64_t* doc_cps,
                         hipStream_t stream);
int snx_tx_segment_meta(const int64_t* ptr, const int32_t* code_points, int32_t n, const int64_t* piece_base,
                        int64_t* par_len, int32_t* par_doc, int32_t* par_hangul, hipStream_t stream);
int snx_tx_segment_fill(const int64_t* ptr, const int32_t* code_points, int32_t n, const int64_t* piece_base,
                        const int64_t* par_ptr, int32_t* par_cps, hipStream_t stream);
int snx_tx_sha256_rows(const int64_t* ptr, const int32_t* code_points, int32_t n, uint32_t* digest, hipStream_t stream);
size_t snx_tx_first_equal_workspace_bytes(int64_t n);
int snx_tx_first_equal(const uint32_t* digest, int32_t n, int32_t* first, void* workspace, size_t ws_bytes,
                       hipStream_t stream);

/* ---- Character n-gram TF-IDF (csrc/tfidf.hip): the vectorizer of the reference's lexical hard-negative mining
 * (ref:scripts/mine_hard_negatives.py:141-146: scikit-learn's TfidfVectorizer(analyzer="char_wb", ngram_range=(2, 3),
 * max_features=30000, sublinear_tf=True), rows L2-normalised, searched by cosine), which scikit-learn and scipy hold to
 * 50,000 documents there.  Rows are a CSR of Unicode code points as for the MinHash section: ptr [n+1] int64, code_points
 * int32 in [0, 0x10FFFF].  The host lowers each text (str.lower) and splits it (str.split); a row is its words joined by
 * one U+0020, and U+0020 is the only separator the device knows (any run of them, in front, inside or behind, separates).
 * N-grams: a word w is padded to " " + w + " " (length L >= 3); for n ascending over min_n .. max_n it gives all its
 * L - n + 1 windows of n code points, or, when L <= n, the whole padded word once and nothing for a larger n.  No window
 * spans two words: a U+0020 between two words belongs to both padded words (as a 1-gram it counts twice).  An empty row
 * and a row of U+0020 only have no n-gram.  1 <= min_n <= max_n <= 3, otherwise SNX_E_SHAPE.
 * Key: an n-gram c0 [c1 [c2]] is the int64 (c0+1) << 42 | (c1+1) << 21 | (c2+1), an absent position 0.  Exact (U+10FFFF + 1
 * < 2^21), > 0, and ascending key order is the order of the n-gram strings by code point with a prefix first:
 * scikit-learn's feature order.
 * Row counts: row r owns the slots [(ptr[r] + 2 r) NS, (ptr[r+1] + 2 (r+1)) NS) of out_key (int64) and out_count (int32),
 * NS = max_n - min_n + 1 + (min_n == 1); both hold (ptr[n] + 2 n) NS entries.  The front out_cnt[r] slots of a row
 * receive its distinct keys ascending and how often each occurs; the rest is left unwritten.  One workgroup sorts a row's
 * slots in LDS when they are at most SNX_TFIDF_LDS_KEYS = 4096 (with the range (2, 3): rows up to 2046 code points); a
 * longer row is sorted in the workspace by the same code and gives the same result.  longest_row [host]: an upper bound
 * of the row lengths (a row beyond it comes out empty).  workspace: snx_tfidf_counts_workspace_bytes(longest_row, min_n,
 * max_n) bytes, 0 when every row fits the LDS form.
 * Weights (the transform): rows as a CSR of (key ascending, count >= 1), row_ptr [n+1] int64.  feat_key [F] int64 strictly
 * ascending are the vocabulary, feature id = position; idf [F] float64; tf_table [tmax + 1] float64 is the host's term
 * frequency function, tf_table[c] for a count c (1 + log(c) for sublinear tf, c otherwise; no logarithm is computed on the
 * device, as for snx_bm25_weights), every count <= tmax (a larger one is read as tmax).  A key found in feat_key by binary
 * search is KNOWN, the others are dropped.  u_i = tf_table[c_i] * idf[f_i] in float64, w_i = fp32(u_i / sqrt(sum_j u_j^2)):
 * the squares are summed in float64 per lane of one wave over the row's entries i = lane, lane + 64, ... ascending, from +0,
 * then folded by the xor tree 32, 16, .. 1 -- a fixed order, so the bits repeat from run to run; against a float64 sum in
 * another order a weight differs by at most one fp32 ulp.  Row r's known entries go to the front out_cnt[r] places of
 * out_fid (int32, ascending) and out_w (fp32, > 0 for idf > 0) from row_ptr[r]; a row with no known key is empty.
 * Compaction: rows whose filled fronts start at src_ptr[r] move to dst_ptr[r] .. dst_ptr[r+1], the CSR that
 * snx_sparse_index_build and snx_sparse_search take.
 * The fit between the two steps -- the distinct keys of a corpus with total count and document frequency, the max_features
 * keys of largest total count (ties: lowest key), idf = log((1 + n_docs) / (1 + df)) + 1 in float64 with numpy -- is the
 * Python layer's (snx.retrieval.TfidfIndex): one device-wide sort per corpus.  Stream-ordered, no host synchronisation. */
#define SNX_TFIDF_LDS_KEYS 4096
size_t snx_tfidf_counts_workspace_bytes(int64_t longest_row, int32_t min_n, int32_t max_n);
int snx_tfidf_row_counts(const int64_t* ptr, const int32_t* code_points, int32_t n, int64_t longest_row, int32_t min_n,
                         int32_t max_n, int64_t* out_key, int32_t* out_count, int32_t* out_cnt, void* workspace,
                         size_t ws_bytes, hipStream_t stream);
int snx_tfidf_weights(const int64_t* row_ptr, const int64_t* key, const int32_t* count, int32_t n, const int64_t* feat_key,
                      const double* idf, int32_t F, const double* tf_table, int32_t tmax, int32_t* out_fid, float* out_w,
                      int32_t* out_cnt, hipStream_t stream);
int snx_tfidf_compact_counts(const int64_t* src_ptr, const int64_t* dst_ptr, int32_t n, const int64_t* src_key,
                             const int32_t* src_count, int64_t* dst_key, int32_t* dst_count, hipStream_t stream);
int snx_tfidf_compact_rows(const int64_t* src_ptr, const int64_t* dst_ptr, int32_t n, const int32_t* src_fid,
                           const float* src_w, int32_t* dst_fid, float* dst_w, hipStream_t stream);

/* ---- WordPiece tokenizer (csrc/wordpiece.hip): the tokenizer the model ships (ref:huggingface/v33/tokenizer.json:
 * normalizer NFC, BertPreTokenizer, WordPiece, template "<s> $A </s>"), from code points to token ids.  Everything here is
 * integer work and every result equals the `tokenizers` library's bit for bit.  Rows are a CSR of Unicode code points as
 * for the MinHash section, ptr [n+1] int64 and code_points int32, NOT lowered and NOT stripped, already in NFC (the host
 * normalizes; the device knows no normalization); a value outside [0, 0x10FFFF] is read as a word character.
 * Pre-tokenizer: class [0x110000] uint8 is the host's table over all code points, 0 = word character, 1 = White_Space
 * (ends the current word and is dropped), 2 = punctuation (ends the current word and is a word of its own).
 * WordPiece: a word of more than max_word code points is the single id unk_id.  Otherwise at offset st the ends
 * min(len, st + max_entry) .. st + 1 are tried in that order, a candidate at st > 0 as a continuation entry; the first hit
 * emits its id and moves st behind it; an offset without a hit makes the WHOLE word the single id unk_id.
 * Vocabulary: E entries, entry e = (ent_cont[e] in {0, 1}: continuation entry; its code points
 * ent_cps[ent_ptr[e] .. ent_ptr[e+1]), the continuation prefix left out; ent_id[e]); ent_ptr [E+1], ent_cont [E],
 * ent_id [E], ent_cps: int32.  slots [n_slots] int32, n_slots a power of two >= E: an open-addressed table of entry
 * numbers, -1 = free.  The hash of (cont, c_0 .. c_{L-1}), all arithmetic modulo 2^32: h = 0; h = h * 0x9E3779B1 + (c_i + 1)
 * for each code point; x = h ^ (cont ? 0x85EBCA6B : 0) ^ L * 0xC2B2AE35; x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15;
 * x *= 0x846CA68B; x ^= x >> 16; the home slot is x & (n_slots - 1), a collision goes on to the next slot (linear probing,
 * wrapping).  A lookup compares cont, L and the stored code points; the hash only chooses where to start.  The prefix
 * hashes of a word are computed once, so a candidate's hash is two reads and a multiplication.  1 <= max_entry <= max_word
 * <= 128, otherwise SNX_E_SHAPE.
 * Pass 1, snx_wp_pieces: one workgroup per row, a thread per code point, the thread on a word's first code point walks its
 * word.  pieces [ptr[n]] int32 (caller-owned): the id of the piece that STARTS at a code point, -1 where none does (the
 * unk of a word stands on its first code point) -- pieces in text order are pieces in row order, no atomic decides a
 * place.  out_cnt [n] int64: min(pieces of the row, max_pieces) + 2, the length of the framed row; max_pieces < 0: no
 * limit (max_length m is max_pieces = m - 2).  A row of at most 4096 code points has its code points and prefix hashes in
 * LDS; a longer row goes through the workspace by the same code and gives the same result.  longest_row [host]: an upper
 * bound of the row lengths (a row beyond it comes out as bos, eos).  workspace: snx_wp_workspace_bytes(longest_row)
 * bytes, 0 when every row fits the LDS form.
 * Pass 2, snx_wp_fill: out_ptr [n+1] int64 = 0 and the running sums of out_cnt (the caller's scan; out_ptr[n] is the one
 * number the host reads, to size out_ids).  Row r of out_ids (int64) becomes bos_id, its first out_ptr[r+1] - out_ptr[r]
 * - 2 pieces, eos_id.  A row whose out_ptr span is larger than its pieces + 2 (the caller raised out_cnt) keeps the places
 * between unwritten: the Python layer puts the rows it tokenized itself there.
 * Padding, snx_wp_pad: input_ids [n, L] int64 = row r of out_ids, then pad_id; attention_mask [n, L] int64 = 1 on the row,
 * 0 behind it; a row longer than L is cut at L.  Stream-ordered, nothing allocated, no host synchronisation. */
size_t snx_wp_workspace_bytes(int64_t longest_row);
int snx_wp_pieces(const int64_t* ptr, const int32_t* code_points, int32_t n, int64_t longest_row, const uint8_t* cls,
                  const int32_t* slots, int32_t n_slots, const int32_t* ent_ptr, const int32_t* ent_cps,
                  const int32_t* ent_cont, const int32_t* ent_id, int32_t n_entries, int32_t max_entry, int32_t max_word,
                  int32_t unk_id, int64_t max_pieces, int32_t* pieces, int64_t* out_cnt, void* workspace, size_t ws_bytes,
                  hipStream_t stream);
int snx_wp_fill(const int64_t* ptr, const int32_t* pieces, int32_t n, const int64_t* out_ptr, int32_t bos_id,
                int32_t eos_id, int64_t* out_ids, hipStream_t stream);
int snx_wp_pad(const int64_t* out_ptr, const int64_t* out_ids, int32_t n, int64_t L, int64_t pad_id, int64_t* input_ids,
               int64_t* attention_mask, hipStream_t stream);

/* ---- Unigram tokenizer (csrc/unigram.hip): the dense teacher's tokenizer, XLM-RoBERTa's tokenizer.json (normalizer
 * Precompiled = SentencePiece's nmt_nfkc charsmap, WhitespaceSplit + Metaspace, a Unigram model, template "<s> $A </s>"),
 * from code points to token ids, equal to the `tokenizers` library's bit for bit.  Rows are a CSR of RAW code points, ptr
 * [n+1] int64 and code_points int32, each row shorter than 2^26.  The device normalizes code point by code point, which is
 * the library's result for a row without a code point that joins a grapheme cluster; the host keeps the other rows.
 * Normalizer: nmap [0x110000] int32 is the host's table over all code points, -1 = kept, else offset << 5 | length
 * (length <= 31, may be 0) of the replacement in pool (int32 code points); a value outside [0, 0x10FFFF] is kept.
 * snx_ug_norm_count: out_len [n] int64 = 1 + the replacement lengths of the row.  norm_ptr [n+1] int64 = 0 and the running
 * sums of out_len (the caller's scan; norm_ptr[n] and the largest out_len are read by the host, to size norm and the
 * workspace).  snx_ug_norm_fill: row r of norm (int32) = U+0020, then the replacements in order.  The leading white space
 * is the slot of the first word's U+2581: every word of a normalized row has white space in front of it.
 * Pre-tokenizer: white space is Rust's char::is_whitespace.  A UNIT starts at every U+2581 and at white space that is
 * directly followed by a word character (neither white space nor U+2581); that first entry is read as U+2581, the unit
 * goes on over the word characters behind it.  (A word receives a leading U+2581 unless it begins with one and is cut
 * before every further one.)  Entry 0 of a row must be white space.
 * Unigram, per unit w[0..len), float64: best[0] = 0; for st ascending and every vocabulary piece w[st..en): cand =
 * score + best[st] replaces best[en] when that is unset or cand > best[en]; when no piece of ONE code point starts at st,
 * cand = unk_score + best[st] competes for best[st+1] the same way, with unk_id.  The kernel evaluates the same candidates
 * end by end, longest piece first, the unknown last: the same order per end, single float64 additions, no multiplication.
 * The pieces of the best path are read back from the end; consecutive unk_id of one unit fuse into one.
 * Vocabulary: E entries, entry e = (its code points ent_cps[ent_ptr[e] .. ent_ptr[e+1]), ent_id[e], ent_score[e] float64),
 * the pieces no unit can hold left out (white space inside, U+2581 behind the first place); slots [n_slots] and the hash
 * as in the WordPiece section with cont = 0.  1 <= max_entry <= 32 (the hit lengths of a start are one uint32), otherwise
 * SNX_E_SHAPE.
 * snx_ug_pieces: one workgroup per row.  pieces [norm_ptr[n]] int32 (caller-owned): the id of the piece that STARTS at an
 * entry, -1 where none does; out_cnt [n] int64 = min(pieces of the row, max_pieces) + 2 (max_pieces < 0: no limit).  A row
 * of at most 4096 normalized code points (4097 entries) has its state in LDS, 25 bytes an entry: rows of
 * up to 512 in 12.7 KiB (seven workgroups per CU), longer ones in 100 KiB (one per CU of 160 KiB).  A longer row goes
 * through the workspace by the same code and gives the same result.  longest_row [host]: an upper bound of the rows'
 * entries (a row beyond it comes out as bos, eos).  workspace: snx_ug_workspace_bytes(longest_row) bytes, 0 when every row
 * fits LDS.  snx_wp_fill(norm_ptr, pieces, ...) and snx_wp_pad finish the rows as for WordPiece.
 * Stream-ordered, nothing allocated, no host synchronisation. */
size_t snx_ug_workspace_bytes(int64_t longest_row);
int snx_ug_norm_count(const int64_t* ptr, const int32_t* code_points, int32_t n, const int32_t* nmap, int64_t* out_len,
                      hipStream_t stream);
int snx_ug_norm_fill(const int64_t* ptr, const int32_t* code_points, int32_t n, const int32_t* nmap, const int32_t* pool,
                     const int64_t* norm_ptr, int32_t* norm, hipStream_t stream);
int snx_ug_pieces(const int64_t* norm_ptr, const int32_t* norm, int32_t n, int64_t longest_row, const int32_t* slots,
                  int32_t n_slots, const int32_t* ent_ptr, const int32_t* ent_cps, const int32_t* ent_id,
                  const double* ent_score, int32_t n_entries, int32_t max_entry, int32_t unk_id, double unk_score,
                  int64_t max_pieces, int32_t* pieces, int64_t* out_cnt, void* workspace, size_t ws_bytes,
                  hipStream_t stream);

/* ---- Co-occurrence and PMI (csrc/cooc.hip): the reference's src/pmi package -- windowed co-occurrence counts
 * (ref:src/pmi/cooccurrence.py:206-226) and PMI with Laplace and context-distribution smoothing
 * (ref:src/pmi/pmi_calculator.py:142-193).  Input is token ids, never text: rows as a CSR, ptr [n_rows+1] int64, ids int32
 * in [0, V) or -1 for a token outside the vocabulary (it stays in place: in a sliding window it occupies a slot; any id
 * outside [0, V) is read as -1).  1 <= V, V * V < 2^63; a cell's key is row * V + col in int64.
 * Windows: win_ptr == NULL: every row is one window (sentence and paragraph mode), window g is row g.  Otherwise sliding
 * with window_size = w >= 1 and win_ptr [n_rows+1] int64 the running window counts of the rows: a row of n tokens has no
 * window when n == 0, one (the whole row) when n <= w, else n - w + 1 windows of w tokens starting at 0 .. n - w
 * (ref:cooccurrence.py:321-331).  The kernel expands the windows; the host never copies the corpus.
 * A window's contribution: idx = its ids >= 0 in order, repeats included, m = len(idx); m < 2: nothing.  Otherwise for
 * every position pair i < j: C[idx_i, idx_j] += 1, and when symmetric also C[idx_j, idx_i] += 1.  So a term r times in a
 * window adds r (r - 1) to its diagonal cell when symmetric and r (r - 1) / 2 when not, and the non-symmetric C[a, b]
 * counts the pairs with a before b.
 * Records: a window gives ONE record per distinct (row term a, col term b) with a multiplicity > 0: key = a * V + b,
 * mult int64 = its additions to C[a, b], m int32 = the window's m (out_m may be NULL).  Symmetric: only a <= b is emitted
 * (mult r_a r_b, diagonal r (r - 1)); the caller mirrors once after the reduction.  The order of a window's records is
 * arbitrary; the caller's reduction (sort, integer sums) does not depend on it.
 * snx_cooc_windows serves the windows [first_window, first_window + n_windows), n_windows < 2^31.  rec_ptr == NULL is
 * pass 1: out_cnt [n_windows] int64 receives each window's record count.  rec_ptr [n_windows + 1] (the running sums of
 * those counts, from any start) is pass 2: window i's records go to out_*[rec_ptr[i] - rec_ptr[0] ..).
 * A window of at most 64 tokens is one wave's, one of at most SNX_COOC_LDS_TOKENS = 4096 one workgroup's in LDS (48 KiB:
 * three workgroups per CU of 160 KiB); a longer one takes the workspace with the same code and the same result.
 * longest_window [host]: an upper bound of the window lengths (a window beyond it gives no record); workspace:
 * snx_cooc_workspace_bytes(longest_window) bytes, 0 when every window fits LDS.
 * Normalised cells (weight 1 / m): cells as a CSR over (m ascending, adds), cell_ptr [n_cells+1] int64;
 * out[c] = fp32(sum_i adds_i / m_i) summed in float64 in ascending m from +0: the same bits from run to run.
 * PMI, all float64, c the fp32 cell value widened, k = laplace: c < min_cooccurrence: c = k when k > 0, else the result is
 * NONE = 0.0 under use_ppmi and -inf without; p_joint = (c + k) / (total + k * V * V); p1 = marginals[row], p2 =
 * marginals[col], either 0: NONE; pmi = log(p_joint / (p1 * p2)) as log2 (SNX_COOC_LOG2), log (SNX_COOC_LOGE) or
 * log(x) / ln_base (SNX_COOC_LOGB); under use_ppmi max(0, pmi).  snx_cooc_pmi_cells: every stored cell of the CSR (indptr
 * [V+1] int64, indices int32 ascending per row, data fp32) -> out float64 [nnz].  snx_cooc_pmi_pairs: (rows[i], cols[i])
 * int32 pairs, the cell found by binary search in its row, an absent cell c = 0, a negative (or >= V) index NONE
 * -> out float64 [n].  marginals float64 [V] and total are the host's (numpy, ref:pmi_calculator.py:92-116).
 * Stream-ordered, no host synchronisation. */
#define SNX_COOC_LDS_TOKENS 4096
#define SNX_COOC_LOG2 0
#define SNX_COOC_LOGE 1
#define SNX_COOC_LOGB 2
size_t snx_cooc_workspace_bytes(int64_t longest_window);
int snx_cooc_windows(const int64_t* ptr, const int32_t* ids, int32_t n_rows, const int64_t* win_ptr, int64_t window_size,
                     int64_t first_window, int64_t n_windows, int64_t longest_window, int64_t V, int32_t symmetric,
                     const int64_t* rec_ptr, int64_t* out_cnt, int64_t* out_key, int64_t* out_mult, int32_t* out_m,
                     void* workspace, size_t ws_bytes, hipStream_t stream);
int snx_cooc_normalized_cells(const int64_t* cell_ptr, const int32_t* m, const int64_t* adds, int64_t n_cells, float* out,
                              hipStream_t stream);
int snx_cooc_pmi_cells(const int64_t* indptr, const int32_t* indices, const float* data, int64_t V, int64_t nnz,
                       const double* marginals, double total, double laplace, double min_cooccurrence, int32_t use_ppmi,
                       int32_t base_mode, double ln_base, double* out, hipStream_t stream);
int snx_cooc_pmi_pairs(const int64_t* indptr, const int32_t* indices, const float* data, int64_t V, const int32_t* rows,
                       const int32_t* cols, int64_t n, const double* marginals, double total, double laplace,
                       double min_cooccurrence, int32_t use_ppmi, int32_t base_mode, double ln_base, double* out,
                       hipStream_t stream);

/* ---- exact L2 nearest neighbours (csrc/infogain.hip): the distance work of the reference's information-gain filter of
 * synonym pairs (ref:src/information_gain.py:156-195, 340-364: a float64 cdist of every target and every source against the
 * whole corpus of term embeddings, then one argsort over the corpus per pair in a Python loop).  The Kozachenko-Leonenko
 * estimator multiplies log(rho_k) by d and tells a distance of exactly 0 from a tiny one, so the distance is the
 * difference form in float64; the Gram form (|a|^2 + |b|^2 - 2 a.b) is ruled out, and with it MFMA.
 * Operands: corpus E [n, D] and queries fp32, row-major, every value finite; 1 <= D <= 4096; n < 2^31.
 * Distance (part of the ABI, bit-reproducible): d2(q, c) = float64 acc starting at +0.0; for j = 0 .. D-1 ascending
 * t = (double)q[j] - (double)c[j], acc = fma(t, t, acc).  Tiling, splits and which kernel computes it change no bit; a row
 * against an identical row gives exactly 0.0.  Order: d2 ascending, ties lowest corpus id first.
 * snx_l2_knn: per query the k nearest (1 <= k <= SNX_L2_KMAX = 256) -> out_id int32 / out_d2 float64 [nq, k]; unused slots
 * (k > n) id -1, d2 +inf.  chunk_rows: corpus rows per split (0: default; otherwise rounded up to a multiple of 64); neither
 * it nor any slicing of the queries changes a bit.  workspace: snx_l2_knn_workspace_bytes(nq, n, k, chunk_rows) bytes -- it
 * grows with nq * k * splits, never with nq * n.
 * snx_l2_gather_sorted: for pair i the distances d2(T[i], E[nb[i, r]]), r < K (1 <= K <= 256), by the same chain, an id
 * outside [0, n) skipped, the row sorted ascending with +inf in the unused slots -> out_d2 float64 [m, K].
 * Stream-ordered, no host synchronisation. */
#define SNX_L2_KMAX 256
size_t snx_l2_knn_workspace_bytes(int32_t nq, int32_t n, int32_t k, int32_t chunk_rows);
int snx_l2_knn(const float* Q, int32_t nq, const float* E, int32_t n, int32_t D, int32_t k, int32_t chunk_rows,
               int32_t* out_id, double* out_d2, void* workspace, size_t ws_bytes, hipStream_t stream);
int snx_l2_gather_sorted(const float* T, int32_t m, const float* E, int32_t n, int32_t D, const int32_t* nb, int32_t K,
                         double* out_d2, hipStream_t stream);

/* ---- term-expansion evaluation (csrc/expansion.hip): graded judgments of a source term's expansion, scored against the
 * model's own ranking of the vocabulary (ref:src/evaluation/ranking_metrics.py:435-680: per query a clone of the row, one
 * masked element per special id, torch.topk, up to 100 .item() pairs and a Python walk per metric and cutoff).
 * THE RANKING OF A ROW (part of the ABI): rep [B, V] fp32 contiguous, excluded [V] uint8.  Entry v is RANKED when
 * rep[v] > 0 and excluded[v] == 0 (NaN, -0.0 and negatives are not > 0).  Ranked entries are ordered by weight descending,
 * ties lowest id first -- the rule of snx_sparse_topk -- and the list is cut after max_k.  The position of a ranked entry t
 * is 1 + #{ranked v: rep[v] > rep[t]} + #{ranked v < t: rep[v] == rep[t]}: the kernel counts, it does not sort.  This is the
 * reference's _sparse_to_ranking (specials to -inf, topk(min(max_k, V)), values <= 0 dropped) wherever torch.topk's
 * unspecified order among equal weights does not matter.
 * Judgments, a CSR over the rows: j_ptr [B+1] int64 (starts at 0, does not decrease, ends at nj; a violation reads and
 * writes nothing out of bounds, its result is otherwise unspecified), j_tok [nj] int32 (per row distinct, any order; an id
 * outside [0, V) is never read through and is simply unranked), j_grade [nj] uint8 (gain grade 0 .. 3), j_rel [nj] uint8
 * (non-zero: the entry counts for out_first and out_hits).  Grade and relevance are separate inputs because the
 * reference's recall / MRR set and its DCG grade map are built differently (snx.expansion).  No cap on a row's judgments.
 * max_k >= 1.  cutoffs [host] int32, 1 <= ncut <= 8 entries >= 1, strictly ascending; an entry may exceed max_k and then
 * means the whole cut list.  gain [3, G] float64, the caller's device table, G >= min(max_k, cutoffs[ncut-1]):
 * gain[(g-1) * G + (p-1)] is the DCG term of grade g at position p.  The Python layer fills it with
 * (2**g - 1) / math.log2(p + 1); the kernel computes no logarithm and no division (as disc of snx_ranked_relevance).
 * Outputs: out_rank [nj] int32 = the entry's position, 0 when it is not in the cut list; out_nranked [B] int32 =
 * min(max_k, ranked entries of the row); out_first [B] int32 = smallest position among the row's j_rel members, 0 if none;
 * out_hits [B, ncut] int32 = j_rel members at positions <= cutoffs[j]; out_dcg [B, ncut] float64 = the left fold from +0.0,
 * in ascending position order, of gain[grade-1][p-1] over the row's judged entries with grade > 0 and position
 * p <= cutoffs[j], every add rounded on its own.
 * slices: column slices a row is split into over workgroups (0: the call chooses from B and V; otherwise forced, at most
 * V).  The slices' partial counts are integers added by atomics into the workspace, which the call itself clears on the
 * stream: the slicing changes no bit.  Stream-ordered, no host synchronisation.
 * workspace: snx_expansion_workspace_bytes(B, nj) bytes.  snx_expansion_ranks: the first two outputs alone.
 * Null pointers, bad cutoffs, G too small, nj < 0, slices < 0, a missing or short workspace: SNX_E_ARG; B < 0, V outside
 * [1, 2^30], max_k < 1: SNX_E_SHAPE.  B * V may exceed 2^31.  B == 0 launches nothing. */
size_t snx_expansion_workspace_bytes(int32_t B, int64_t nj);
int snx_expansion_ranks(const float* rep, int32_t B, int32_t V, const uint8_t* excluded, const int64_t* j_ptr,
                        const int32_t* j_tok, int64_t nj, int32_t max_k, int32_t slices, int32_t* out_rank,
                        int32_t* out_nranked, void* workspace, size_t ws_bytes, hipStream_t stream);
int snx_expansion_metrics(const float* rep, int32_t B, int32_t V, const uint8_t* excluded, const int64_t* j_ptr,
                          const int32_t* j_tok, const uint8_t* j_grade, const uint8_t* j_rel, int64_t nj, int32_t max_k,
                          const int32_t* cutoffs /*[host]*/, int32_t ncut, const double* gain, int32_t G, int32_t slices,
                          int32_t* out_rank, int32_t* out_nranked, int32_t* out_first, int32_t* out_hits, double* out_dcg,
                          void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- SPLADELossV33 (ref:src/model/losses.py:183-297) ------------------------------------- */
/* dims [host] = {B, Bp, k, V, label_off, bf16_mm}: q [B,V], p [Bp,V] (Bp > B: all-gathered
 * positives for cross-GPU in-batch negatives, own rows start at label_off), n [B*k,V]; bf16_mm=1
 * rounds the operands of the in-batch mm to bf16 as autocast does (ref:losses.py:155).
 * hp [host] = {temperature, lambda_q(t), lambda_d(t), lambda_neg(t), lambda_margin_mse, lambda_kd, kd_temperature}
 * (the lambda schedule ref:losses.py:75-90 is evaluated by the host caller).
 * tpos [B], tneg [B*k] teacher scores or NULL (MarginMSE, ref:losses.py:92-134).
 * tscores [B,B] teacher score matrix or NULL (KL distillation against the rank's own positives, ref:losses.py:239-253:
 * batchmean KL(softmax(tscores / T_kd) || softmax(q p^T / T_kd)), active when lambda_kd > 0 and tscores != NULL).
 * out9 = {loss, infonce, flops_q, flops_d, flops_neg, margin_mse, nonzero_q, nonzero_d, kd}. */
size_t snx_loss_workspace_bytes(int32_t B, int32_t Bp, int32_t k, int32_t V);
int snx_loss_fwd(const float* q, const float* p, const float* n, const float* tpos, const float* tneg,
                 const float* tscores, const float* hp /*[host]*/, const int32_t* dims /*[host]*/, void* workspace,
                 float* out9, hipStream_t stream);
/* gout = dL/dloss (device scalar); dq [B,V], dp [Bp,V], dn [B*k,V] are overwritten.  use_kd != 0: the forward that
 * filled `workspace` was given tscores with lambda_kd > 0. */
int snx_loss_bwd(const float* q, const float* p, const float* n, const float* gout, const float* hp /*[host]*/,
                 const int32_t* dims /*[host]*/, void* workspace, int32_t use_kd, float* dq, float* dp, float* dn,
                 hipStream_t stream);

/* ---- IDF (csrc/idf.hip): document frequencies, the IDF-aware FLOPS penalty and the inference-free ("doc-only") query.
 * Logarithms are the host's (snx/idf.py: float64, one rounding to fp32); nothing here calls libm.
 *
 * snx_idf_doc_freq -- replaces the counting loop of ref:tools/idf-compute/src/main.rs:150-180 (a HashSet per document,
 * one increment per distinct id).  input_ids, attention_mask [n, S] int64; df [V] int64 is ADDED to (the caller zeroes it
 * once; batches accumulate): df[t] += the number of rows that hold t at a position with mask != 0.  Ids outside [0, V) are
 * ignored (main.rs:166-174); there is no `allowed` filter and no cap on S.  num_docs (device int64, or NULL) += n: every row
 * is a document, also one with no counted position (the tool counts every non-empty text; emptiness is the caller's to
 * decide before tokenising).  Integer atomics: exact and independent of order.  1 <= V <= 2^20 (the presence bitmap is
 * V bits of LDS), S >= 1, n >= 0, otherwise SNX_E_SHAPE; n == 0 launches nothing.
 *
 * snx_idf_flops_fwd -- replaces the penalty of ref:docs/concepts/04-loss-functions.md §5 ("V26": sum_j w_j * mean_j) in the
 * form of ref:scripts/test_idf_math.py:176-215 with the quadratic term of SPLADELossV33 (ref:src/model/losses.py:136-152)
 * beside it.  x [R, V] fp32 (row stride V), w [V] fp32:
 *   a_j  = (x[0,j] + x[1,j] + ... + x[R-1,j]) / (float)R     fp32, rows ascending, one IEEE division (as snx_loss_fwd)
 *   t1_j = w_j * |a_j|,  t2_j = w_j * (a_j * a_j)             fp32, every product rounded on its own
 *   S1 = sum_j t1_j, S2 = sum_j t2_j                          float64, in an order fixed by (R, V) alone
 *   P  = (float)fma((double)beta, S2, S1)
 * out3 = {(float)S1, (float)S2, P}; loss (device scalar, or NULL): loss[0] = loss[0] + lambda * P, the product rounded to
 * fp32 first.  a is kept in the first V floats of `workspace` (snx_idf_flops_workspace_bytes(V) bytes, 8-byte aligned) for
 * the backward.  No float atomics, no host synchronisation: two runs give the same bits.
 *
 * snx_idf_flops_bwd_accum -- the gradient torch.autograd derives from that expression, ADDED in place to an existing
 * gradient block: dx[r, j] += ((w_j * (sign(a_j) + (2 beta) * a_j)) * ((g * lambda) / (float)R)) for every row r, fp32,
 * every operation rounded on its own (six roundings; 2 beta is exact), sign(0) = 0 as torch's abs backward.  A column whose
 * coefficient is zero is not written.  g = gout[0], the device scalar snx_loss_bwd takes; `workspace` as the forward left it.
 *
 * snx_idf_query_dense -- replaces ref:tests/test_korean_neural_sparse.py:417-427 (the doc-only query vector: idf[token] for
 * every token of the query, once however often it occurs): q [B, V] fp32, q[b, id] = idf[id] for each id in [0, V) at a
 * position of row b with mask != 0 and allowed[id] != 0, and 0 elsewhere.  The zero fill is part of the launch.
 * R < 1, V < 1, S < 1, B < 0: SNX_E_SHAPE; null pointers: SNX_E_ARG. */
int snx_idf_doc_freq(const int64_t* input_ids, const int64_t* attention_mask, int64_t n, int64_t S, int32_t V, int64_t* df,
                     int64_t* num_docs, hipStream_t stream);
size_t snx_idf_flops_workspace_bytes(int32_t V);
int snx_idf_flops_fwd(const float* x, int32_t R, int32_t V, const float* w, float beta, float lambda, void* workspace,
                      float* out3, float* loss, hipStream_t stream);
int snx_idf_flops_bwd_accum(float* dx, int32_t R, int32_t V, const void* workspace, const float* w, float beta,
                            float lambda, const float* gout, hipStream_t stream);
int snx_idf_query_dense(const int64_t* input_ids, const int64_t* attention_mask, const uint8_t* allowed, const float* idf,
                        int32_t B, int64_t S, int32_t V, float* q, hipStream_t stream);

/* ---- individual ops (used by the entry points above; exported for parity tests) ---------- */

/* fp32 -> bf16 (autocast weight / activation cast) and fp32 [R,C] -> bf16 [C,R]. */
int snx_cast_bf16(const float* in, void* out, int64_t n, hipStream_t stream);
int snx_cast_transpose_bf16(const float* in, void* out, int32_t R, int32_t C, hipStream_t stream);

/* nn.Linear under autocast (hf:271,300,90-91,490): C[M,N] = A[M,K] B[N,K]^T, bf16, fp32 acc. */
int snx_gemm_nt_bf16(const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, hipStream_t stream);
/* ... fused with the fp32 residual add of hf:331-332: Hout = Hin + bf16(A B^T). */
int snx_gemm_nt_resid(const void* A, const void* B, const float* Hin, float* Hout, int32_t M, int32_t N, int32_t K,
                      hipStream_t stream);
/* ... Wqkv fused with apply_rotary_pos_emb (hf:271-280): columns < rope_cols (q and k) rotated. */
int snx_gemm_nt_rope(const void* A, const void* B, void* C, const float* rope_tab, const int32_t* pos,
                     int32_t rope_cols, int32_t M, int32_t N, int32_t K, hipStream_t stream);
/* The same with the (cos, sin) row of every token resolved beforehand: rope_rows [M][32][2] fp32 = rope_tab[pos[row]]
 * (snx_rope_rows, once per forward pass and theta; NULL = resolve through pos inside the kernel).  Lets the 256x256
 * kernel's write-back read a row's 256 bytes without the dependent position load.  Same results. */
int snx_rope_rows(const float* cos_sin_tab, const int32_t* pos, float* rope_rows, int32_t T, hipStream_t stream);
int snx_gemm_nt_rope_rows(const void* A, const void* B, void* C, const float* rope_tab, const int32_t* pos,
                          const float* rope_rows, int32_t rope_cols, int32_t M, int32_t N, int32_t K, hipStream_t stream);
/* ... Wi fused with GeGLU (hf:90-91).  B = Wi rows in the interleaved order of snx_cast_geglu_interleave;
 * U [M,N] = Wi output in that column order (saved for backward), Y [M,N/2] = gelu(a) * g. */
int snx_gemm_nt_geglu_fwd(const void* A, const void* B_interleaved, void* U, void* Y, int32_t M, int32_t N,
                          int32_t K, hipStream_t stream);
/* ... dX of mlp.Wo fused with the GeGLU backward: dy = A B^T [M,N=I]; dU [M,2N] (interleaved). */
int snx_gemm_nt_geglu_bwd(const void* A, const void* B, const void* U, void* dU, int32_t M, int32_t N, int32_t K,
                          hipStream_t stream);
/* Dispatch of the five entry points above: from `min_m` rows on (default 8,192; env SNX_NT256_MIN_M) and N % 64 == 0
 * they run the 256x256 persistent kernel (csrc/gemm_nt256.hip), otherwise the 128x128 kernel (csrc/gemm.hip); same
 * results bit for bit (both sum k in the same order).  on = 0 (env SNX_NT256=0) keeps everything on the 128x128
 * kernel, 1 = the default shape policy (wide outputs with the plain / RoPE / GeGLU-forward epilogues), 2 = every
 * eligible shape (tests, A/B); min_m <= 0 leaves the threshold unchanged.  Process-wide host state. */
int snx_nt256_configure(int32_t on, int32_t min_m);
/* fp32 Wi [2I,C] -> bf16 interleaved copy out [2I,C] and/or its transpose out_t [C,2I]: every 64-row
 * group = [a rows 32q..32q+31 | g rows 32q..32q+31] (so a and its gate meet in one lane of the GEMM). */
int snx_cast_geglu_interleave(const float* in, void* out, void* out_t, int32_t I, int32_t C, hipStream_t stream);
/* weight gradient of a Linear: dW[N,K] += dY[M,N]^T X[M,K]  (N, K multiples of 128).
 * ORDERED REDUCTION (round 5; process switch "det_reduce", default 1): the token range is split over workgroups as
 * before, but every workgroup stores its partial tile into the caller-owned workspace `ws` and a second small kernel adds
 * a tile's partials to dW in a FIXED order -- two runs give the same bits, whatever order the workgroups finish in (the
 * role of torch's deterministic cuBLAS reduction; the float-atomic flush of rounds 1-4 stays behind "det_reduce" = 0).
 * `ws` needs snx_gemm_tn_workspace_bytes() bytes (0 for single-writer schedules; a bound that holds for every setting of
 * the process switches), is scratch (no state between calls) and may be shared by launches on ONE stream; launches on
 * different streams need workspaces of their own.  Missing or too small: SNX_E_ARG. */
typedef struct snx_tn_problem {
  const void* dY; /* [M, N] bf16 */
  const void* X;  /* [M, K] bf16 */
  float* dW;      /* [N, K] fp32, += */
  int32_t N, K;
  int32_t interleaved; /* dY columns in the interleaved GeGLU order (N = 2I) */
  int32_t reserved;
} snx_tn_problem;
size_t snx_gemm_tn_workspace_bytes(const snx_tn_problem* probs /*[host]; pointers unused*/, int32_t nprob, int32_t M);
int snx_gemm_tn_accum(const void* dY, const void* X, float* dW, int32_t M, int32_t N, int32_t K, void* ws,
                      size_t ws_bytes, hipStream_t stream);
/* same with dY's columns in the interleaved GeGLU order; dW rows land in the natural Wi order. */
int snx_gemm_tn_accum_interleaved(const void* dY, const void* X, float* dW, int32_t M, int32_t N, int32_t K, void* ws,
                                  size_t ws_bytes, hipStream_t stream);
/* up to 4 weight-gradient problems over the SAME M token rows (the four Linears of one encoder layer, whose
 * nn.Linear backward torch runs as four GEMMs) in one launch.  From 8,192 token rows on: the 256x256 persistent kernel
 * (csrc/gemm_tn256.hip: one workgroup per CU, one flush per workgroup); below, and for the ragged
 * rest of M % 64 rows: the concatenated 128x128 output tiles fill whole rounds of the resident workgroups
 * (csrc/gemm.hip).  The threshold is the process switch "tn256_min_m"; whatever it is set to, the persistent kernel is
 * taken only where the token range holds one whole 64-row K-step ((M & ~63) >= 64): M < 64 always runs the 128x128
 * kernel, with the 0 workspace bytes snx_gemm_tn_workspace_bytes() states for it.  N, K multiples of 128. */
int snx_gemm_tn_accum_group(const snx_tn_problem* probs /*[host]*/, int32_t nprob, int32_t M, void* ws, size_t ws_bytes,
                            hipStream_t stream);
/* Process-wide launch hint (host state, read at launch time): leave `n` CUs (0..128, rounded up to a multiple of 8)
 * to other kernels.  The persistent weight-gradient kernel takes one whole CU per workgroup; while RCCL's channel
 * workgroups run an overlapped gradient exchange (the role of DDP's reducer, ref:src/train/cli/train_v33_ddp.py:539-544)
 * a 256-workgroup launch would run its last workgroups as a second wave, so it launches 256 - n instead (its
 * schedule balances any count).  The token partition changes with the count: results differ from the 256-workgroup
 * launch's by fp32 summation order (each count is bit-reproducible by itself). */
/* Process-wide switches of the library (csrc/config.h).  The library reads no environment variable; the Python binding
 * maps its SNX_* variables onto these keys once, at load time (snx/_lib.py), tests and tools call them directly.
 * Keys (default): nt256 (1; 0 off, 2 every eligible shape), nt256_min_m (8192), tn256 (1), tn256_min_m (8192),
 * dec256 (1), dec256_min_t (2048), bwd_overlap (1), side_prio (1), attn_streaming (0), attn_bwd_onepass (1),
 * splade_dh_panels (64), f32_gemm64 (0), f32_attn_rows (0), wcache_per_tensor (0), resid_in_ln (1: the Wo GEMMs store
 * bf16 and the residual add happens inside the following LayerNorm; 0: in the GEMMs' fp32 epilogue, same bits),
 * stream_nt (1: non-temporal accesses for the streams nobody reads soon -- LayerNorm forward's loads of h and y and its
 * store of h_out, LayerNorm backward's loads of the saved h and of dy, the GeGLU-forward GEMM's stores of the saved u, the
 * weight-gradient GEMM's ordered reduce; 0: none of them; a cache hint, same bits.  A forward without
 * SNX_FWD_SAVE_FOR_BACKWARD runs its own streams plain whatever the value), nt_pipe (2), nt_pipe_min_m (4096),
 * det_reduce (1: weight gradients -- Linear dW, LayerNorm dw, embedding rows -- summed in a fixed order through the callers'
 * workspaces, bit-reproducible; 0: float atomics in arrival order); diagnostics builds (-DSNX_DIAG) add
 * gemm_cg, gemm_dbg, gemm_mid, tn_splits, nt256_cg, nt256_dbg, nt256_force, tn256_tail_pct, tn256_dbg.  Unknown key or
 * value out of range: SNX_E_ARG. */
int snx_configure(const char* key, int32_t value);
int snx_config_get(const char* key, int32_t* value);
/* The SNX_EXTRA_HIPCC_FLAGS the library was compiled with ("" for the product build); snx/_lib.py refuses a library
 * built with a timing-only diagnostics macro (wrong results by design) unless SNX_ALLOW_DIAG_LIB=1. */
const char* snx_build_flags(void);
int snx_set_reserved_cus(int32_t n);
int snx_get_reserved_cus(void);

/* LayerNorm without bias (hf:61,312,314,420,487), fp32 in -> bf16 out. */
int snx_ln_fwd(const float* h, const float* w, void* x_out, int32_t T, int32_t H, float eps, hipStream_t stream);
/* h_out = h + float(y) (y [T,H] bf16: a Linear's output joining the fp32 residual stream, hf:331-332), x_out = bf16(LN(h_out)):
 * the residual add done inside the LayerNorm that follows it (process switch "resid_in_ln"). */
int snx_ln_fwd_add(const float* h, const void* y, const float* w, float* h_out, void* x_out, int32_t T, int32_t H,
                   float eps, hipStream_t stream);
/* ModernBertEmbeddings.forward (hf:64-71): h = LN(E[ids]) fp32, x0 = bf16(h). */
int snx_embed_ln_fwd(const int64_t* ids, const float* E, const float* w, float* h_out, void* x0_out, int32_t T,
                     int32_t H, float eps, hipStream_t stream);
/* ModernBertPredictionHead tail (hf:489-490): LN(gelu(d)). */
int snx_gelu_ln_fwd(const void* d, const float* w, void* x_out, int32_t T, int32_t H, float eps, hipStream_t stream);
/* backward of the three above; dh (+)= dx, dw += ... (overwrite=1: dh = dx); dh_bf16 (nullable)
 * also receives bf16(dh), the gradient of the next bf16 branch output (saves a cast pass).
 * `ws` (snx_ln_bwd_workspace_bytes / snx_embed_ln_bwd_workspace_bytes; scratch, one stream at a time): the blocks'
 * partial dw rows, added to dw in block order by a second kernel; for the embeddings also the dx rows and the per-id
 * token lists from which gradE[id] += sum_t dx[t] is formed in ascending token order (nn.Embedding's backward, hf:64-71,
 * pad rows skipped).  With "det_reduce" = 0 `ws` may be NULL (float atomics, arrival order). */
size_t snx_ln_bwd_workspace_bytes(int32_t T, int32_t H);
size_t snx_embed_ln_bwd_workspace_bytes(int32_t T, int32_t H, int32_t V);
int snx_ln_bwd(const void* dy, const float* h, const float* w, float* dh, void* dh_bf16, float* dw, int32_t T,
               int32_t H, float eps, int32_t overwrite, void* ws, size_t ws_bytes, hipStream_t stream);
int snx_embed_ln_bwd(const float* dh, const int64_t* ids, const float* E, const float* w, float* gradE, float* dw,
                     int32_t T, int32_t H, int32_t V, float eps, int32_t pad_id, void* ws, size_t ws_bytes,
                     hipStream_t stream);
int snx_gelu_ln_bwd(const void* dy, const void* d, const float* w, void* dd, float* dw, int32_t T, int32_t H,
                    float eps, void* ws, size_t ws_bytes, hipStream_t stream);

/* apply_rotary_pos_emb (hf:196-219) in place on the q and k thirds of qkv [T,3,heads,64]. */
int snx_rope_inplace(void* qkv, const float* cos_sin_tab, const int32_t* pos, int32_t T, int32_t heads,
                     int32_t inverse, hipStream_t stream);

/* ModernBertMLP GeGLU (hf:90-91): y = gelu(u[:, :I]) * u[:, I:], and its backward. */
int snx_geglu_fwd(const void* u, void* y, int32_t T, int32_t I, hipStream_t stream);
int snx_geglu_bwd(const void* u, const void* dy, void* du, int32_t T, int32_t I, hipStream_t stream);

/* Attention (hf:286-297 -> SDPA; masks masking_utils.py:141-150).  window < 0: global layer. */
int snx_attn_fwd(const void* qkv, const int32_t* cu_seqlens, const int64_t* mask, void* out, float* lse, int32_t T,
                 int32_t nseq, int32_t max_seqlen, int32_t heads, int32_t head_dim, int32_t window,
                 hipStream_t stream);
/* Process-wide choice of the backward for sequence groups of <= 256 tokens: 1 (default) the one-pass kernel
 * (csrc/attention_1p.hip: every score formed once, dQ / dK / dV from one launch), 0 the dQ + dK/dV kernel pair
 * (csrc/attention_unit.hip; the second opinion of the parity tests).  Longer groups always stream tile by tile. */
int snx_attn_configure(int32_t bwd_onepass);
/* _ex: `groups` [host] = {n, (seq_begin, nseq, max_len) x n}, n <= 8, consecutive sequence groups with their own
 * maximum length (NULL: one group of max_seqlen) -- only sizes the launch, results are identical. */
int snx_attn_fwd_ex(const void* qkv, const int32_t* cu_seqlens, const int64_t* mask, void* out, float* lse,
                    const int32_t* groups, int32_t T, int32_t nseq, int32_t max_seqlen, int32_t heads,
                    int32_t head_dim, int32_t window, hipStream_t stream);
/* rope_tab/pos (both or neither): also apply the backward of apply_rotary_pos_emb to dq, dk. */
int snx_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu_seqlens,
                 const int64_t* mask, float* delta_scratch /*[heads,T]*/, void* dqkv, const float* rope_tab,
                 const int32_t* pos, int32_t T, int32_t nseq, int32_t max_seqlen, int32_t heads, int32_t head_dim,
                 int32_t window, hipStream_t stream);
int snx_attn_bwd_ex(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu_seqlens,
                    const int64_t* mask, float* delta_scratch /*[heads,T]*/, void* dqkv, const float* rope_tab,
                    const int32_t* pos, const int32_t* groups, int32_t T, int32_t nseq, int32_t max_seqlen,
                    int32_t heads, int32_t head_dim, int32_t window, hipStream_t stream);

/* Tied decoder GEMM + SPLADE tail fused (hf:550 + ref:src/model/splade_modern.py:76-86).  From 2,048 token rows on
 * the 256x192 persistent kernel (csrc/decoder256.hip: it zeroes `keys`, builds its row tables in `scratch` and ends
 * with a finalize pass), below the 128x128 kernel (csrc/splade_head.hip); same outputs, any mask: bit for bit
 * when every partial sum of the K loop is exact in fp32 (tests/splade_fwd_reference.py), else up to the order of the
 * fp32 accumulation.  keys[b, v] = bf16 bits of the maximum over the valid rows << 16 | 0xFFFF - its first sequence
 * position; a key whose value bits are 0 (no valid row with a positive logit, a fully masked sequence) is 0x0000FFFF in
 * both forms.  `scratch`: snx_splade_head_scratch_bytes(T, V) bytes (T = rows of the whole token buffer). */
size_t snx_splade_head_scratch_bytes(int32_t T, int32_t V);
int snx_decoder_splade_fwd_ex(const void* Hd, const void* W, const float* bias, const int32_t* cu_seqlens,
                              const int64_t* mask, float* sparse, uint32_t* keys, float* token_weights, void* scratch,
                              int32_t T, int32_t nseq, int32_t max_seqlen, int32_t V, int32_t K, int32_t finalize,
                              hipStream_t stream);
int snx_decoder_splade_fwd(const void* Hd, const void* W, const float* bias, const int32_t* cu_seqlens,
                           const int64_t* mask, float* sparse, uint32_t* keys, float* token_weights, void* scratch,
                           int32_t T, int32_t nseq, int32_t max_seqlen, int32_t V, int32_t K, hipStream_t stream);
/* snx_decoder_splade_fwd_ex that also records token_keys [T] u32 (see snx_model_token_keys_offset; written by the
 * finalising call; V <= 65535).  token_keys = NULL is snx_decoder_splade_fwd_ex. */
int snx_decoder_splade_fwd_rec(const void* Hd, const void* W, const float* bias, const int32_t* cu_seqlens,
                               const int64_t* mask, float* sparse, uint32_t* keys, float* token_weights,
                               uint32_t* token_keys, void* scratch, int32_t T, int32_t nseq, int32_t max_seqlen, int32_t V,
                               int32_t K, int32_t finalize, hipStream_t stream);
/* snx_decoder_splade_fwd_rec with forward flags (SNX_FWD_*; 0: exactly that entry point).  SNX_FWD_NO_TOKEN_WEIGHTS:
 * `sparse` and `keys` with the same bits, the kernels without the row half of their epilogue, no token_weights pass;
 * token_weights and token_keys are not written (may be NULL), `finalize` means nothing, and `scratch` needs only
 * snx_splade_head_scratch_bytes_notw(T) bytes (the row tables of the 256x192 form, no row maxima). */
size_t snx_splade_head_scratch_bytes_notw(int32_t T);
int snx_decoder_splade_fwd_flags(const void* Hd, const void* W, const float* bias, const int32_t* cu_seqlens,
                                 const int64_t* mask, float* sparse, uint32_t* keys, float* token_weights,
                                 uint32_t* token_keys, void* scratch, int32_t T, int32_t nseq, int32_t max_seqlen, int32_t V,
                                 int32_t K, int32_t finalize, int32_t flags, hipStream_t stream);
/* arg-max-routed backward: dHd [T,H] bf16 (overwritten), gradE [V,H] += , gradb [V] += ;
 * scratch: snx_splade_bwd_scratch_bytes() bytes (per-row bucket lists). */
size_t snx_splade_bwd_scratch_bytes(int32_t nseq, int32_t max_seqlen, int32_t V);
int snx_splade_bwd(const float* g, const uint32_t* keys, const void* Hd, const void* W, const int32_t* cu_seqlens,
                   void* dHd, float* gradE, float* gradb, void* scratch, int32_t T, int32_t nseq,
                   int32_t max_seqlen, int32_t V, int32_t H, hipStream_t stream);
/* ... plus the token_weights direction: g_tw [T] fp32 (NULL: snx_splade_bwd), token_keys from
 * snx_decoder_splade_fwd_rec, tw_scratch: snx_splade_tw_scratch_bytes(T, V) bytes. */
size_t snx_splade_tw_scratch_bytes(int32_t T, int32_t V);
int snx_splade_bwd_tw(const float* g, const uint32_t* keys, const float* g_tw, const uint32_t* token_keys, const void* Hd,
                      const void* W, const int32_t* cu_seqlens, void* dHd, float* gradE, float* gradb, void* scratch,
                      void* tw_scratch, int32_t T, int32_t nseq, int32_t max_seqlen, int32_t V, int32_t H,
                      hipStream_t stream);

/* ---- fused optimizer step (ref:src/train/cli/train_v33_ddp.py:367-374: clip_grad_norm_ + AdamW) ----
 * All four arrays are flat fp32 [n] (16-byte aligned).  hp [host] = {lr, beta1, beta2, eps, weight_decay,
 * max_norm (<= 0: no clipping)}; `step` is the 1-based optimizer step (bias correction); elements in
 * [nodecay_begin, nodecay_end) get weight_decay 0 (the reference's no-decay group = decoder.bias);
 * norm_out [1] receives the pre-clip global L2 norm; scratch: snx_adamw_scratch_bytes(). */
size_t snx_adamw_scratch_bytes(void);
int snx_adamw_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                        const float* hp /*[host]*/, int64_t step, int64_t nodecay_begin, int64_t nodecay_end,
                        float* norm_out, void* scratch, hipStream_t stream);

/* ---- masked-language-model pre-training (csrc/mlm.hip) ----
 * Token masking with the contract of DataCollatorForLanguageModeling.torch_mask_tokens (labels = -100 where no loss is
 * taken), the draws a pure function of the token: Philox4x32-10, key = the 64-bit seed, counter = (lo32(t), hi32(t),
 * epoch, 0) with t = sample_index * 65536 + position, outputs r0..r3.  Selected iff attended, id not in special_ids
 * [host, n_special <= 16] and r0 2^-32 < p; a selected token becomes mask_id if r1 2^-32 < p_mask, the id
 * (r2 * vocab) >> 32 if r1 2^-32 < p_mask + p_random, else stays.  input_ids, attention_mask, masked_ids, labels [B, S]
 * int64, sample_index [B] int64.  S > 65535: SNX_E_SHAPE. */
int snx_mlm_mask_tokens(const int64_t* input_ids, const int64_t* attention_mask, const int64_t* sample_index,
                        int64_t* masked_ids, int64_t* labels, int32_t B, int32_t S, const int64_t* special_ids /*[host]*/,
                        int32_t n_special, int64_t mask_id, int32_t vocab, int64_t seed, int32_t epoch, double p,
                        double p_mask, double p_random, hipStream_t stream);
/* Vp: the vocabulary rounded up to the 128-column tile of the cross-entropy kernels */
int64_t snx_mlm_vocab_padded(int32_t V);
/* E [V, H] bf16 (the weight cache's embedding matrix) -> E^T [H, Vp] bf16, pad columns zero: the operand of dh = g E.
 * Rebuilt by the caller when the weights change. */
int snx_mlm_transpose_embeddings(const void* E, void* ET, int32_t V, int32_t H, hipStream_t stream);
/* Cross-entropy of M gathered rows against the tied decoder:
 *   z[m,v] = bf16(sum_k h E in fp32 + float(bf16(bias[v]))),  lse[m] = logsumexp_v z[m,v] in fp32 over v < V,
 *   row_loss[m] = lse[m] - z[m, labels[m]],  loss[0] = sum_m row_loss[m] / M.
 * h [M, H] bf16, labels [M] int64 in [0, V) (a label outside gives that row, and the loss, NaN), z [M, Vp] bf16 (kept for
 * the backward; pad columns zero), part: (2 Vp / 128 + 1) * M floats of scratch.  H % 128 == 0, H <= 1024.
 * M == 0: nothing is launched and nothing written. */
int snx_mlm_ce_fwd(const void* h, const void* E, const float* bias, const int64_t* labels, void* z, float* part, float* lse,
                   float* row_loss, float* loss, int32_t M, int32_t V, int32_t H, hipStream_t stream);
/* Its backward: z becomes g[m,v] = bf16((exp(z - lse) - [v == labels[m]]) * upstream[0] / M) in place, then
 *   dh [M, H] bf16 = bf16(g E),  dE [V, H] fp32 += g^T h,  dbias [V] fp32 += sum_m g,
 * every sum in a fixed order (no float atomics).  ET from snx_mlm_transpose_embeddings, upstream [1] fp32 on the device,
 * ws: snx_mlm_ce_bwd_workspace_bytes() bytes of scratch. */
size_t snx_mlm_ce_bwd_workspace_bytes(int32_t M, int32_t V, int32_t H);
int snx_mlm_ce_bwd(void* z, const float* lse, const int64_t* labels, const float* upstream, const void* h, const void* ET,
                   void* dh, float* dE, float* dbias, void* ws, size_t ws_bytes, int32_t M, int32_t V, int32_t H,
                   hipStream_t stream);

/* ---- optional per-kernel-class timing inside the model entry points (HIP events recorded on
 * the launch stream around every kernel class; off by default).  snx_prof_read synchronises on
 * the recorded events and returns, per class, elapsed ms, launch count and algorithmic work
 * (FLOPs for MFMA-bound classes, bytes for HBM-bound ones). */
int snx_prof_enable(int32_t on);
int32_t snx_prof_num_classes(void);
const char* snx_prof_class_name(int32_t i);
int snx_prof_read(double* ms /*[host]*/, int64_t* launches /*[host]*/, double* work /*[host]*/);

#ifdef __cplusplus
}
#endif
#endif /* SNX_H_ */
