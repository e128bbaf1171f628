/* libullsam_hip.so -- C ABI of the MI355X (gfx950) uLLSAM hot path.
 *
 * The reference (ieellee/uLLSAM) has NO native/FFI layer: its hot path is PyTorch ATen calls inside nn.Module.forward
 * (SURVEY.md section 8(b)).  The drop-in boundary is therefore the Python module surface (ullsam_amd/modeling/*, same
 * names / signatures / state_dict keys as the reference); this header is the ABI those modules bind with ctypes --
 * each entry point names the reference call site (file:line under /root/reference) whose ATen ops it replaces.
 *
 * Conventions
 *   - plain pointers are DEVICE pointers (torch tensor.data_ptr()); no torch types cross this boundary
 *   - dtype: 0 = float32 (parity mode, exact-fp32 MFMA), 1 = bfloat16 (throughput mode, fp32 accumulate)
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); kernels are stream-ordered, never
 *     allocate, never synchronise, never throw
 *   - return 0 on success, < 0 on error; ullsam_last_error_string() describes the last error of the calling thread
 */
#ifndef ULLSAM_HIP_H
#define ULLSAM_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define ULLSAM_DT_F32 0
#define ULLSAM_DT_BF16 1
#define ULLSAM_ACT_NONE 0
#define ULLSAM_ACT_GELU 1   /* exact erf GELU (nn.GELU default) */
#define ULLSAM_ACT_RELU 2
#define ULLSAM_ACT_SWIGLU 3 /* paired 64-column gate/up blocks -> silu(gate)*up */

/* Bumped whenever the signature or the meaning of an EXISTING entry point changes.  The Python binding refuses a library that reports another
   version (a stale libullsam_hip.so would otherwise receive shifted arguments, e.g. a row count where the stream is expected).  An entry point
   that is only ADDED leaves the number alone (ullsam_sample_topk_topp did): a library built before it lacks the symbol, which the binding's
   load reports by name, and the in-tree build's stamp covers this header and every source, so a stale library is rebuilt either way. */
#define ULLSAM_ABI_VERSION 14

const char* ullsam_last_error_string(void);
int ullsam_abi_version(void); /* == ULLSAM_ABI_VERSION of the header the library was built from */
int ullsam_device_count(void);
/* GEMM kernel selection for A/B measurements and the kernel tests: 0 = auto (by shape), 1 = 128x128 tile, 3 = 256x256 two-buffer kernel,
   6 / 8 / 9 = ring kernel with 256x256 / 256x320 / 272x256 tiles; +64 = no split-K tail; +32768 = stamped diagnostic launch of the ring kernel (+65536 as well: of its persistent form,
   whose stamps are per tile: tile start, K loop done, epilogue done, stores acknowledged). */
int ullsam_set_gemm_variant(int variant);
/* measurement knob, not part of the reference's interface: key 0 = tile rows per raster group of the 256-row-tile GEMM kernels (default 4);
   key 1 = ring tile shapes the automatic dispatch may use (bit 0 256x256, bit 1 256x320, bit 2 272x256; default 7);
   key 2 = how ring launches of MORE than one round of tiles run (csrc/gemm_ring8p.h; both values give bit-equal outputs): 2 (default) = persistent grid,
   identical trips, both wave groups' epilogues together; 0 = one tile per workgroup (the kernel of rounds 2 - 5); every other value is rejected;
   key 3 = split-K on the ring kernel for launches of <= 128 tiles whose K cuts into ranges of >= 1280 that fill >= 224 workgroups: 1 (default) = where the caller allows it
   (ullsam_gemm's act | 256), 0 = never, 2 = wherever it fits;
   key 4 = the weight as K-panels (ullsam_gemm_panels): 1 (default) = ring launches that were handed panels read them, 0 = every launch reads the row-major weight (bit-equal);
   key 5 = activations as K-panels (ullsam_gemm_act_panels): 1 (default) = ring launches take the a_panels / out_panels flags where the query says so, 0 = the query
   answers no and a flag is refused, i.e. every launch runs as it did before the flags existed (bit-equal) */
int ullsam_set_gemm_tuning(int key, int value);
/* Attention kernel selection for A/B measurements and the kernel tests: 0 = production; 1 / 2 = windowed attention on the tiled kernel (7-wave /
   4-wave workgroups) instead of the whole-window kernel; 3..8 = start stagger of the whole-window kernel's second resident workgroup; 9 = global
   attention as two 4-wave workgroups; 11 = causal prefill on the tiled kernel instead of the LDS-DMA kernel (the bit-equality test's reference). */
int ullsam_set_attn_variant(int variant);
/* diagnostic hook, not part of the reference's interface: a device buffer (>= 8 x 8 bytes per wave of the launch) that the stamped build of the
   causal prefill attention kernel fills with s_memtime sums (request issue / compute / wait + barrier per wave); NULL (default) = the product kernel */
int ullsam_set_attn_debug(void* stamps);

/* C[M,N] = act(A[M,K] . W[N,K]^T + bias) + residual.  Replaces every nn.Linear / 1x1 conv / stride==kernel conv:
 * image_encoder.py:227,238,387-395,88-104; common.py:21-26; modeling_internvl_sam.py:88-100;
 * modeling_internlm2.py:261-264,359,421,1081; transformer.py:220-227 (image side); mask_decoder.py:53-59.
 * A, W in `dtype`; C float when out_f32 else `dtype`; bias/residual fp32 (nullable); residual row = m %% res_row_mod
 * when res_row_mod > 0 (pos_embed broadcast, image_encoder.py:107-109).  K %% (128/elem_size) == 0.
 * workspace (optional, caller-owned device scratch, >= 32 MiB useful, 128 MiB for every split-K form): lets launches whose last wave of tiles is mostly empty
 * split those tiles along K (fp32 partials in the workspace + a reduce kernel), and launches of few tiles (e.g. 1081 x 4096 outputs) run as up to 8 K ranges
 * side by side (S fp32 planes of the output in the workspace, added in order); null disables both.
 * act: 0 none, 1 GELU (erf), 2 ReLU, 3 SwiGLU pair; | 256 = ULLSAM_ACT_SPLITK_OK: the caller accepts the K-ranges form just described.  Every one-launch kernel adds the
 * 32-deep k steps of an output in sequence, so an image gets the same bits alone and inside a batch; K ranges summed apart do not -- the training step's frozen
 * linears set the flag (one image per step, train_joint_v2.py), the inference modules never do. */
#define ULLSAM_ACT_SPLITK_OK 256
int ullsam_gemm(int dtype, const void* A, long lda, const void* W, long ldw, void* C, long ldc, int out_f32,
                const float* bias, const float* residual, long ldr, int res_row_mod, int act, int M, int N, int K,
                void* workspace, long ws_bytes, void* stream);

/* InternLM2Attention's wqkv projection with `rearrange 'b q (h gs d)'`, apply_rotary_pos_emb and the KV-cache append in the GEMM
 * epilogue (modeling_internlm2.py:359-388, 233-247): q_out T [B*S, KVH*G*128] rotated, k_cache (rotated) / v_cache T [B, KVH, cap, 128]
 * rows cache_pos0..cache_pos0+S-1; pos int32 [B*S] rows of the fp32 cos / sin tables [tab_rows, 128] (clamped).  head_dim = 128. */
int ullsam_gemm_qkv_rope(int dtype, const void* A, long lda, const void* W, long ldw, const float* bias, int B, int S, int K, int KVH,
                         int G, const int* pos, const float* cos_tab, const float* sin_tab, int tab_rows, void* q_out, void* k_cache,
                         void* v_cache, int cap, int cache_pos0, void* workspace, long ws_bytes, void* stream);

/* ullsam_gemm / ullsam_gemm_qkv_rope with the bf16 weight handed over twice: row-major `W` [N, ldw] and the SAME values once more as K-panels
 * `w_panels` = [N / 16][K / 32][16 rows][32 k] (ullsam_amd.packing.pack_ring_panels; N % 16 == 0, K % 32 == 0, 1 KiB aligned, nullable), in which one
 * (16-row block, 32-deep k step) cell is one contiguous KiB.  The ring kernels read the panels when the launch covers whole tiles of a contiguous weight
 * (N a multiple of the tile width, ldw == K) and ullsam_set_gemm_tuning(4, 1) holds (the default); every other kernel the dispatch picks reads `W`.
 * The result is the same bit for bit: only the addresses the weight requests read from differ. */
int ullsam_gemm_panels(int dtype, const void* A, long lda, const void* W, long ldw, const void* w_panels, void* C, long ldc, int out_f32,
                       const float* bias, const float* residual, long ldr, int res_row_mod, int act, int M, int N, int K,
                       void* workspace, long ws_bytes, void* stream);
int ullsam_gemm_qkv_rope_panels(int dtype, const void* A, long lda, const void* W, long ldw, const void* w_panels, const float* bias, int B, int S,
                                int K, int KVH, int G, const int* pos, const float* cos_tab, const float* sin_tab, int tab_rows, void* q_out,
                                void* k_cache, void* v_cache, int cap, int cache_pos0, void* workspace, long ws_bytes, void* stream);

/* ... and with the bf16 ACTIVATIONS as K-panels: [ceil(M / 16)][K / 32][16 rows][32 k] (ullsam_amd.packing.pack_activation_panels: the cell of the weight
 * panels, the row count rounded up to 16; 1 KiB aligned; rows M .. the next multiple of 16 exist, are never written and never reach a stored value).  The
 * layout is written by the kernel that PRODUCES the activation -- the norm in front of wqkv / w13 (modeling_internlm2.py:598-618) and of qkv / lin1
 * (image_encoder.py:166,180), the SwiGLU epilogue of w13 in front of w2 (modeling_internlm2.py:261-264), the GELU epilogue of lin1 in front of lin2
 * (common.py:23-25) -- never by a repacking pass.  a_panels: A is laid out so (lda == K).  out_panels: C is written so (2-byte outputs without residual:
 * plain, bias, GELU / ReLU, SwiGLU; N_out % 32 == 0, ldc == N_out).  Only the two ring kernels take the flags: ask ullsam_gemm_act_panels_query for the launch
 * first; a flag on a launch that does not take it is an error before anything is launched.  w_panels is nullable.  Same result bit for bit. */
int ullsam_gemm_act_panels(int dtype, const void* A, long lda, const void* W, long ldw, const void* w_panels, void* C, long ldc, int out_f32,
                           const float* bias, const float* residual, long ldr, int res_row_mod, int act, int M, int N, int K,
                           void* workspace, long ws_bytes, int a_panels, int out_panels, void* stream);
/* modeling_internlm2.py:359-388 as ullsam_gemm_qkv_rope_panels, reading A as panels; q / k / v stay row-major */
int ullsam_gemm_qkv_rope_act_panels(int dtype, const void* A, long lda, const void* W, long ldw, const void* w_panels, const float* bias, int B, int S,
                                    int K, int KVH, int G, const int* pos, const float* cos_tab, const float* sin_tab, int tab_rows, void* q_out,
                                    void* k_cache, void* v_cache, int cap, int cache_pos0, void* workspace, long ws_bytes, int a_panels, void* stream);
/* Would this launch read A as panels, could it write C as panels?  Runs the dispatch of the launch itself and launches nothing.  The launch as the modules make
 * it: contiguous operands, act as for ullsam_gemm (4 = the wqkv + RoPE launch with N = KVH (G + 2) 128), ws_bytes of workspace, aligned = A and C on 1 KiB
 * boundaries, bias / residual on 16-byte ones. */
int ullsam_gemm_act_panels_query(int dtype, int M, int N, int K, int act, int out_f32, int has_bias, int has_residual, int aligned, long ws_bytes,
                                 int* reads_a_panels, int* writes_c_panels);

/* Decode step (InternVLSAMModel.generate's token loop, modeling_internlm2.py:1112-1149; M <= 4 rows, bf16 weights): the RMSNorm that
 * precedes a layer's wqkv / w13 (modeling_internlm2.py:75-89, 598-618) folded into the GEMM that consumes it:
 * C = act(bf16(x * rsqrt(mean(x^2) + eps) * norm_w) @ W^T + bias) (+ residual), x fp32 [M, K <= 4096], K % 2048 == 0; act as ullsam_gemm. */
int ullsam_gemm_rmsnorm(const float* x, long ldx, const float* norm_w, float eps, const void* W, long ldw, void* C, long ldc, int out_f32,
                        const float* bias, const float* residual, long ldr, int act, int M, int N, int K, void* stream);
/* ... and the decode step's wqkv: ullsam_gemm_qkv_rope with S = 1 and B <= 4, the activations either bf16 `a` [B, K] (norm_w NULL) or the
 * RMSNorm of fp32 x [B, K] as above. */
int ullsam_decode_qkv_rope(const void* a, const float* x, long ldx, const float* norm_w, float eps, const void* W, long ldw, const float* bias,
                           int B, int K, int KVH, int G, const int* pos, const float* cos_tab, const float* sin_tab, int tab_rows, void* q_out,
                           void* k_cache, void* v_cache, int cap, int cache_pos0, void* stream);

/* ---- Training slice: backward kernels of the segmentation branch of train_joint_v2.py:1026-1100, everything
 * downstream of the LLM's last hidden state (mlp2, prompt encoder, mask decoder, upsample, BCE + Dice).  fp32; torch.autograd.Function
 * wrappers in ullsam_amd/training.py.  Buffers that receive atomics (d* of colsum / ln_bwd / attn_bwd / resize_bwd / index_add_rows,
 * `sums`) are zeroed by the caller. */
/* C[b](m,n) = (accumulate ? C : 0) + sum_k A[b](m,k) B[b](k,n), explicit element strides (nn.Linear backward: dX = dY W, dW = dY^T X;
 * the hypernetwork product of mask_decoder.py:146-147 and its gradients) */
int ullsam_train_matmul(const float* A, const float* B, float* C, int M, int N, int K, int batch, long a_b, long a_m, long a_k, long b_b,
                        long b_k, long b_n, long c_b, long c_m, long c_n, int accumulate, void* stream);
/* the product with both fp32 operands rounded to bf16 on load and summed on the bf16 MFMA (fp32 accumulation and result): torch.autocast(bfloat16)'s matmul,
 * i.e. the attention products of the reference's trainer on its bf16 model (train_joint_v2.py:1665) */
int ullsam_train_matmul_bf16(const float* A, const float* B, float* C, int M, int N, int K, int batch, long a_b, long a_m, long a_k, long b_b,
                             long b_k, long b_n, long c_b, long c_m, long c_n, int accumulate, void* stream);
/* the product over (outer, head) pairs whose operands sit inside [rows, heads x hd] activations: entry (o, h) of operand X starts at o x_o + (h / x_hdiv) x_h elements
 * (x_hdiv = query heads per KV head for k / v, modeling_internlm2.py:250-259 repeat_kv); bf16 != 0: operands rounded to bf16 as ullsam_train_matmul_bf16.  The attention
 * products of a training step read q / k / v / dO and write out / dq / dk / dv in place instead of through head-major copies.  tri: the causal structure of a square
 * attention (0 none): 1 = C[query][key], 128 x 128 tiles wholly behind the diagonal are not formed (ullsam_train_attn_rows reads no entry behind the diagonal whose probability is 0 and writes zeros there);
 * 2 = the sum runs over queries, m is the key: it starts at the tile's first key; 3 = the sum runs over keys, m is the query: it stops after the tile's last query.
 * tri assumes every query sees an unpadded key: a row whose visible keys are all padded (left padding) is uniform over every single-masked entry, those behind the
 * diagonal included, as the reference's additive finfo.min masks make it -- such a batch takes tri = 0 (training.AttentionFn) */
int ullsam_train_matmul_heads(const float* A, const float* B, float* C, int M, int N, int K, int outer, int heads, long a_o, long a_h, int a_hdiv, long a_m, long a_k,
                              long b_o, long b_h, int b_hdiv, long b_k, long b_n, long c_o, long c_h, long c_m, long c_n, int accumulate, int bf16, int tri, void* stream);
/* the same product with its k range cut into `ksplit` pieces run by separate workgroups and added IN ORDER by a second kernel (few output tiles,
 * long sums: rel-pos table gradients, the hypernetwork gradient over 65536 pixels); partial: ksplit * batch * M * N floats of scratch */
int ullsam_train_matmul_splitk(const float* A, const float* B, float* C, int M, int N, int K, int batch, long a_b, long a_m, long a_k, long b_b,
                               long b_k, long b_n, long c_b, long c_m, long c_n, int accumulate, int ksplit, float* partial, void* stream);
/* the product above runs on the matrix pipe (exact fp32 MFMA, 128 x 128 tiles) from M >= 64, N >= 48, K >= 16; 0 keeps every launch on the
 * one-output-per-thread kernel (tests compare the two); returns the previous setting */
int ullsam_train_set_matmul_mfma(int on);
/* the bf16 product (ullsam_train_matmul_bf16 / _heads) fetches its k-fastest operands 16 bytes per lane where their strides and alignment allow (1, default) or element by
 * element as in round 4 (0); the LDS image and the MFMA order are the same: equal bits (tests compare); returns the previous setting */
int ullsam_train_set_matmul_vec(int on);
/* out[c] += sum_r x[r*ld + c] (bias gradients; gradients of parameters broadcast over the batch) */
int ullsam_train_colsum(const float* x, float* out, long rows, int cols, long ld, float* partial, void* stream);
/* (row blocks write partial sums that are added in order -- no atomics; partial: min(64, ceil(rows / 64)) * cols floats, may be NULL for rows <= 64) */
/* nn.LayerNorm / LayerNorm2d backward on rows of D (w NULL: no affine, prompt_encoder.py:141-144); dw / db may be NULL */
int ullsam_train_ln_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, long rows, int D, float eps, float* ws, void* stream);
/* (ws: 2 * rows + 2 * min(64, ceil(rows / 64)) * D floats when dw or db is given: row statistics and ordered partial sums) */
/* kind 1 exact GELU, 2 ReLU: dy NULL -> out = act(x), else out = dy * act'(x) */
int ullsam_train_act(const float* x, const float* dy, float* out, long n, int kind, void* stream);
/* prompt_encoder.py:148 y = x * llm_scale_factor + llm_bias (dy NULL), else out = dy * s, ds += sum dy x, dt += sum dy */
int ullsam_train_scale_shift(const float* x, const float* s, const float* t, const float* dy, float* out, float* ds, float* dt, long n, float* partial, void* stream);
/* (backward: partial = 2 * ceil(n / 1024) floats; ds / dt += the ordered sum of the per-block partials) */
/* softmax attention for the training path, forward (dout NULL: writes out) and backward (dout given: writes dq, adds dk / dv):
 * transformer.py:220-242 (groups 1, causal -1, no mask) and modeling_internlm2.py:383-419 with the additive finfo.min masks of :834-870
 * (groups = H / KV heads, causal = Sk - Sq, key_mask int32 [B, Sk]).  q / dq / out [B,Sq,H,hd], k, v / dk, dv [B,Sk,H/groups,hd] by
 * (batch, token, head) strides; hd <= 128 */
int ullsam_train_attention(const float* q, const float* k, const float* v, const float* dout, float* out, float* dq, float* dk, float* dv,
                           int B, int H, int groups, int hd, int Sq, int Sk, int causal, const int* key_mask, long q_bs, long q_ts, long q_hs,
                           long k_bs, long k_ts, long k_hs, long v_bs, long v_ts, long v_hs, long o_bs, long o_ts, long o_hs, float scale,
                           const float* bias_h, const float* bias_w, float* dbias_h, float* dbias_w, int kw, void* stream);
/* (bias_h [B,H,Sq,Sk/kw], bias_w [B,H,Sq,kw]: the ViT's decomposed relative-position terms, image_encoder.py:325-361, added to the logits
 * as bias_h[q][key / kw] + bias_w[q][key % kw]; NULL elsewhere.  The backward writes dbias_h / dbias_w.) */
/* adjoint of ullsam_im2col3x3 (neck conv3x3 as im2col + Linear): dcols [B*H*W, 9*C] -> dx [B,H,W,C] */
int ullsam_train_col2im3x3(const float* dcols, float* dx, int B, int H, int W, int C, void* stream);
/* Row pass of the training attention in matrix form (large problems: the atomics of the kernel above serialise).  S [B*H, Sq, Sk] holds
 * (q*scale) k^T from ullsam_train_matmul (have_p 0): logits = S + bias + masks, P = softmax in place.  dP NULL: forward, stop there (out = P v by
 * ullsam_train_matmul).  dP = dO v^T given: dS = P (dP - sum_j P_j dP_j) overwrites dP and the decomposed-bias gradient rows are written; have_p 1:
 * S already holds the P the forward kept. */
int ullsam_train_attn_rows(float* S, float* dP, const float* bias_h, const float* bias_w, float* dbias_h, float* dbias_w, const int* key_mask,
                           int B, int H, int Sq, int Sk, int kw, int causal, int have_p, void* stream);
/* 0: keep the row pass on its three-pass form (tests compare it with the register-resident form used for Sk <= 4096); returns the previous setting */
int ullsam_train_set_rows_reg(int on);
/* InternLM2RMSNorm backward (modeling_internlm2.py:75-89); dw_rows NULL (frozen LLM) or [rows, D]: the rows of dy * xhat, whose column sums
 * (ullsam_train_colsum: ordered, no atomics) are dw -- a trainable norm weight (train.py's SFT stage) gets the same bits in every run (version 12) */
int ullsam_train_rmsnorm_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw_rows, long rows, int D, float eps, void* stream);
/* apply_rotary_pos_emb (modeling_internlm2.py:233-247) on rows [tokens, heads, hd]; adjoint != 0: its transpose (the backward) */
int ullsam_train_rope(const float* x, const int* pos, const float* cos_tab, const float* sin_tab, float* out, long tokens, int heads, int hd,
                      int tab_rows, int adjoint, void* stream);
/* InternLM2MLP's silu(w1 x) * (w3 x) (modeling_internlm2.py:598-618): dy NULL -> out, else dg / du */
int ullsam_train_swiglu(const float* g, const float* u, const float* dy, float* out, float* dg, float* du, long n, void* stream);
/* adjoint of the bilinear upsample F.interpolate(align_corners=False) of train_joint_v2.py:1073-1078 (planes of oh x ow -> ih x iw) */
int ullsam_train_resize_bwd(const float* dout, float* din, long planes, int ih, int iw, int oh, int ow, void* stream);
/* calc_instance_loss (train_joint_v2.py:774-812) with BCELoss (:638-661) + DiceLoss (:605-636): x logits / t targets [P, npix];
 * sums [P][4], losses [3] = (total, bce, dice); the backward scales by gscale[0] (the incoming gradient of the total) */
int ullsam_train_seg_loss(const float* x, const float* t, float* sums, float* losses, int P, long npix, float smooth, float* partial, void* stream);
/* (partial: P * 4 * ceil(npix / 1024) floats) */
int ullsam_train_seg_loss_bwd(const float* x, const float* t, const float* sums, const float* gscale, float* dx, int P, long npix, float smooth, void* stream);
/* The language-model loss of InternLM2ForCausalLM.forward (modeling_internlm2.py:1084-1096: CrossEntropyLoss() over the shifted logits, mean over labels != -100):
 * fp32 logits [rows, V] with row stride ld, labels int64 [rows]; lse [rows], loss_rows [rows], out2 = {mean loss, 1 / #labelled rows};
 * the backward writes dlogits = (softmax - onehot) * gscale[0] * out2[1] (zero rows where the label is ignored).  Ordered sums: reproducible bits.
 * No labelled row at all: out2[0] is NaN, as torch's mean over zero rows (the reference's `0 * loss + seg` is NaN there too), out2[1] = 0.
 * Deviation: a label outside [0, V) other than -100 is treated as ignored here, where torch raises (device-side assert); the host wrapper (training.lm_loss)
 * rejects such labels when they arrive on the CPU. */
int ullsam_train_cross_entropy(const float* logits, long ld, const long long* labels, float* lse, float* loss_rows, float* out2, long rows, int V, void* stream);
int ullsam_train_cross_entropy_bwd(const float* logits, long ld, const long long* labels, const float* lse, const float* out2, const float* gscale, float* dlogits,
                                   long ldx, long rows, int V, void* stream);   /* dlogits rows of ldx >= V floats: columns V .. ldx - 1 are zeroed (GEMM padding) */
/* The same gradient for a TRAINABLE LM head (train.py:284-318, 400-480: the SFT stage leaves language_model.output trainable), in bf16 and in the head GEMMs' own
 * operand layouts, written in one pass over the logits: dlog [rows, ldd] row-major (dX = dlog W; ldd >= Vp) and dlogT [Vp, ldt] (dW = dlog^T h; ldt >= Rp), Vp / Rp = V /
 * rows rounded up to 64, the pads zero.  Each value is the round-to-nearest-even bf16 of what ullsam_train_cross_entropy_bwd writes.  dlog or dlogT NULL: that layout is skipped. */
int ullsam_train_cross_entropy_bwd_bf16(const float* logits, long ld, const long long* labels, const float* lse, const float* out2, const float* gscale,
                                        void* dlog, long ldd, void* dlogT, long ldt, long rows, int V, void* stream);
/* The gradient of the token embeddings nn.Embedding(V, D, padding_idx=pad_token_id) (modeling_internlm2.py:808,815; embedding_dense_backward) behind the
 * <IMG_CONTEXT> splice `input_embeds[selected] * 0.0 + vit_embeds` (modeling_internvl_sam.py:124-158): table_grad [V, D] (out_dtype 0 fp32 / 1 bf16, rounded
 * once from the fp32 sum) = sum of the dX rows [rows, ldx] of each id; rows whose id is padding_idx or whose skip[] entry is nonzero (skip may be NULL)
 * contribute nothing, ids outside [0, V) are ignored, rows no id names are zero; D % 4 == 0, D <= 8192.  sorted_ids / order = a STABLE sort of the ids and the positions they came
 * from (the caller's torch.sort(stable=True)): each id's rows are summed in ascending position order -- no atomics, two runs give the same bits. */
int ullsam_train_embedding_bwd(const float* dx, long ldx, const int* sorted_ids, const int* order, const int* skip, long rows, int D, int V, int padding_idx,
                               void* table_grad, int out_dtype, void* stream);
/* dst[idx[r]] += src[r]: gradient of the point-label embedding table (prompt_encoder.py:76-96) */
int ullsam_train_index_add_rows(const float* src, const int* idx, float* dst, long rows, int C, int nrows_dst, void* stream);

/* Row LayerNorm / RMSNorm, fp32 statistics.  image_encoder.py:151,161; common.py:38-43 (LayerNorm2d on NHWC rows);
 * modeling_internlm2.py:138-143 (rms=1); prompt_encoder.py:142-149 (no affine + post scale/shift); transformer.py norms. */
int ullsam_norm(const void* in, int in_dtype, long in_stride, void* out, int out_dtype, long out_stride, const float* w,
                const float* b, long rows, int D, float eps, int rms, int act, const float* post_scale,
                const float* post_shift, void* stream);
/* ullsam_norm with a bf16 output written as activation K-panels for the GEMM that follows (image_encoder.py:166,180; modeling_internlm2.py:598-618): out is the
 * 1 KiB aligned buffer of ceil(rows / 16) * 16 rows of D elements, D % 32 == 0.  out_panels == 0: row-major with stride D.  Same values, only where each goes. */
int ullsam_norm_panels(const void* in, int in_dtype, long in_stride, void* out, const float* w, const float* b, long rows, int D, float eps, int rms,
                       int act, const float* post_scale, const float* post_shift, int out_panels, void* stream);
int ullsam_set_norm_variant(int v);   /* developer switch: non-zero = wave-per-row kernel for every shape (A/B) */

/* LayerNorm whose result feeds three consumers at once: fp32 stream, compute-dtype copy, compute-dtype (y + pe[row % pe_rows]).
   transformer.py:182 (norm4) followed by :160-165 / :176-178 of the next block. */
int ullsam_norm_fanout(const float* in, long rows, int D, const float* w, const float* b, float eps, float* out_f32, void* out_c,
                       void* out_c_pe, int c_dtype, const float* pe, long pe_rows, void* stream);

/* SAM ViT attention on packed qkv [B, gh*gw, 3*heads*hd]; window > 0 fuses window_partition/unpartition and the pad-token
 * semantics; decomposed rel-pos computed in-kernel.  image_encoder.py:170-177,224-240,243-289,292-361.
 * Rel-pos tables, in the activation dtype, one size per side: global (window == 0) rel_h is [2*grid_h - 1, hd] and rel_w is
 * [2*grid_w - 1, hd] (index q - k + side - 1; grid_h != grid_w is allowed, both <= 64); windows (window <= 14) take [2*window - 1, hd]
 * for both, whatever the grid.  qkv, out, rel_h, rel_w and qkv_bias must be 16-byte aligned; another base is refused before any launch. */
int ullsam_vit_attention(int dtype, const void* qkv, void* out, const void* rel_h, const void* rel_w, const void* qkv_bias,
                         int B, int heads, int hd, int grid_h, int grid_w, int window, void* stream);

/* InternLM2 causal GQA attention (prefill), additive masks as modeling_internlm2.py:96-125,830-851; :383-419.
 * q, k, v and out must be 16-byte aligned; another base is refused before any launch. */
int ullsam_causal_attention(int dtype, const void* q, const void* k, const void* v, void* out, const int* key_mask, int B,
                            int H, int KVH, int hd, int Sq, int Sk, int k_cap, int q_pos0, void* stream);

/* Small-shape attention with explicit strides (decoder token attention transformer.py:220-242; q_len==1 decode). */
int ullsam_naive_attention(int dtype, const void* q, const void* k, const void* v, void* out, const int* key_mask, int B,
                           int H, int KVH, int hd, int Sq, int Sk, long q_bs, long q_ts, long q_hs, long k_bs, long k_ts,
                           long k_hs, long v_bs, long v_ts, long v_hs, long o_bs, long o_ts, long o_hs, float scale,
                           void* stream);

/* Decode step (q_len == 1): one bf16 query per head against the bf16 KV cache [B, KVH, cap, 128], the heads of a GQA group
   together, keys split over nsplit workgroups.  modeling_internlm2.py:383-419, mask :834.  workspace f32 [B*KVH*nsplit*(H/KVH)*130]. */
int ullsam_decode_attention(const void* q, const void* kc, const void* vc, const int* key_mask, void* out, int B, int H, int KVH,
                            int hd, int Sk, int cap, float scale, float* workspace, int nsplit, void* stream);

/* Image -> token cross attention (many queries, few keys), fp32.  transformer.py:178-181.  q_batch_stride (elements) = 0 when
   all B batches share one query set (layer 0 of the decoder when B prompts look at one image). */
int ullsam_fewkeys_attention(const float* q, const float* k, const float* v, float* out, int B, int H, int hd, int Sq,
                             int Sk, float scale, long q_batch_stride, void* stream);

/* Token -> image cross attention (T queries, N image keys, 8 heads x 16), K/V streamed once.  transformer.py:160-166,
   100-106.  k/v in kv_dtype with element batch strides (0 = shared image): fp32 K/V T <= 8 (VALU kernel); bf16 K/V T <= 16 (matrix-pipe kernel, queries and
   probabilities as two bf16 terms: fp32-level accuracy on the rounded K/V).  workspace f32 [P*nsplit*T*144]; the caller chooses nsplit (ops.py: from N alone,
   so that the softmax merge order does not depend on the prompt count). */
int ullsam_tok2img_attention(int kv_dtype, const float* q, const void* k, const void* v, float* out, int P, int H, int hd, int T,
                             int N, long k_batch_stride, long v_batch_stride, float scale, float* workspace, int nsplit,
                             void* stream);

/* ViT / projector data movement */
int ullsam_patch_im2col(int dtype, const float* pixels, void* out, int B, int C, int Hs, int Ws, int S, int patch,
                        const float* mean, const float* stdv, void* stream);            /* image_encoder.py:391-395, sam.py:164-174 */
int ullsam_im2col3x3(int dtype, const void* in, void* out, int B, int H, int W, int C, void* stream); /* image_encoder.py:96-102 */
int ullsam_add_cast(const void* a, int a_dtype, long a_rows, const float* b, long b_rows, void* out, int out_dtype,
                    long rows, int cols, void* stream);                                  /* transformer.py:165,181; mask_decoder.py:127 */
int ullsam_transpose_f32(const float* in, float* out, int B, int R, int C, void* stream);  /* image_encoder.py:114 permute */
/* in [R, C] (in_dtype: f32 or bf16) -> out bf16 [C, Rp], transposed, columns R..Rp-1 zero (training: the dW / dX GEMM operands, cast + transposed in one pass) */
int ullsam_transpose_to_bf16(int in_dtype, const void* in, void* out, int R, int C, int Rp, void* stream);
/* fp32 [R, C] -> bf16 [R, C] (out_rm, may be NULL) and bf16 [C, Rp] (out_t: transposed, zero columns behind R) and the column sums sum_r in[r][c] (colsum_out fp32 [C], may be NULL;
 * colsum_ws: ceil(Rp / 64) * C floats of scratch, 64-row blocks added in order) in ONE pass: what a bf16 Linear of the training step needs of an activation and of a gradient.
 * C and Rp multiples of 4. */
int ullsam_cast_transpose_bf16(const float* in, void* out_rm, void* out_t, float* colsum_out, float* colsum_ws, int R, int C, int Rp, void* stream);
int ullsam_pixel_shuffle_ln(int dtype, const float* in_nhwc, void* out, const float* w, const float* b, int B, int H, int W,
                            int C, float eps, void* stream);                             /* modeling_internvl_sam.py:226-251,89 */
int ullsam_pixel_unshuffle(const float* in, float* out_nhwc, int B, int H, int W, int C, void* stream); /* :256-268 */

/* LLM data movement */
int ullsam_scan_image_tokens(const long long* ids, int* rank, int* range, int B, int S, long long img_id, void* stream); /* :135-139,194-199 */
int ullsam_embed_tokens(int dtype, const void* table, const long long* ids, const int* rank, const float* vit_embeds,
                        float* out, int B, int S, int D, int n_img, long vocab, void* stream);                          /* :124-158 */
int ullsam_gather_rows(const void* in, void* out, const int* range, int B, int S, int n, int row_bytes, void* stream);  /* :198-200 */
int ullsam_rope_split(int dtype, const void* qkv, void* q_out, void* k_cache, void* v_cache, const int* pos,
                      const float* cos_tab, const float* sin_tab, int B, int S, int KVH, int G, int hd, int cap,
                      int cache_pos0, int tab_rows, void* stream);                       /* modeling_internlm2.py:361-388,233-247;
                                                                                            pos is clamped to [0, tab_rows) */
int ullsam_argmax(const float* logits, long long* out, int rows, long V, long ld, void* stream);
/* One token per row from temperature / top-k / top-p sampling on fp32 logits [rows, V] (row stride ld >= V), the caption path's policy: app.py:469-477
 * calls chat(do_sample=True, temperature=0.7, top_k=50, top_p=0.9), which reaches transformers' generate (modeling_internvl_sam.py:314 -> :433
 * language_model.generate(**generate_kwargs)) and its TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper + multinomial.  One launch; per row:
 *   candidates  the min(top_k, V) largest logits (NaN counts as -inf), descending, equal values by ascending id -- ties at the k-th value go to the
 *               lower ids, so exactly top_k tokens stay (transformers keeps every token tied with the k-th);
 *   p_j         exp((x_j - x_0) / temperature) / sum, fp32;
 *   nucleus     candidate j stays iff j == 0 or the mass strictly before it is < top_p (top_p >= 1: all stay); renormalised over those that stay;
 *   u           u_in[row], or Philox4x32-10 with key (seeds[row] & 0xffffffff, seeds[row] >> 32) and counter (step & 0xffffffff, step >> 32, 0, 0):
 *               u = (word 0 >> 8) * 2^-24 in [0, 1); written to u_out when that is not NULL;
 *   draw        the first remaining candidate whose inclusive cumulative mass exceeds u * total, else the last one of non-zero probability.
 * A row with a +inf yields the first +inf id, a row with nothing above -inf yields 0 (like ullsam_argmax), both with all mass on candidate 0; the result is
 * always in [0, V).  cand_ids int64 / cand_p fp32 [rows, top_k] (NULL or both kinds independently): the ordered candidates and their final probabilities
 * (0 for the removed ones; slots past min(top_k, V): -1 and 0).  The result is a pure function of (row, temperature, top_k, top_p, seed, step).
 * < 0 for top_k outside 1..1024, temperature <= 0, top_p <= 0. */
int ullsam_sample_topk_topp(const float* logits, long long* out, int rows, long V, long ld, float temperature, int top_k, float top_p,
                            const unsigned long long* seeds /* [rows], device */, unsigned long long step,
                            const float* u_in /* [rows] or NULL */, float* u_out /* [rows] or NULL */,
                            long long* cand_ids /* [rows, top_k] or NULL */, float* cand_p /* [rows, top_k] or NULL */, void* stream);

/* Prompt encoder / mask decoder */
int ullsam_small_linear(const float* x, long ldx, const float* W, const float* b, const float* res, long ldr, float* y,
                        long ldy, int M, int N, int K, int act, void* stream);           /* transformer.py:220-227; mask_decoder.py:171-176 */
/* The image -> token half of a two-way block (transformer.py:176-182) for many prompts in ONE pass over the image-side stream (bf16, embedding 256,
 * internal 128, 8 heads): q = xin Wq^T + bq (xin = keys + pe in bf16), a = softmax_heads(q k_tok^T scale) v_tok, upd = res + a Wo^T + bo (res = keys, fp32),
 * y = LayerNorm(upd) -> out_f32 / out_c (bf16) / out_c_pe = bf16(y + key_pe[row % pe_rows]), each optional.  xin / res have P*N rows, or in_mod / res_mod
 * rows shared by every prompt (layer 0: in_mod / res_mod / pe_rows are 0 or N); ktok / vtok fp32 [P, T, 128], T <= 16. */
int ullsam_i2t_block(const void* xin, long in_mod, const float* res, long res_mod, const void* Wq, const float* bq, const float* ktok,
                     const float* vtok, const void* Wo, const float* bo, const float* lnw, const float* lnb, float eps, const float* key_pe,
                     long pe_rows, float* out_f32, void* out_c, void* out_c_pe, int P, int T, int N, float scale, void* stream);

/* The token -> image attention's k / v projections of the image side in one pass (transformer.py:220-222 on the image tokens; bf16, embedding 256 -> internal 128):
 * K = xk Wk^T + bk, V = xv Wv^T + bv; xk = (keys + pe), xv = keys, bf16 [rows, 256]; Wk / Wv bf16 [128, 256]; bk / bv fp32 [128] or NULL; K / V bf16 [rows, 128]. */
int ullsam_kv_proj(const void* xk, const void* xv, const void* Wk, const void* Wv, const float* bk, const float* bv, void* K, void* V, long rows, void* stream);
/* The token side of a two-way block (transformer.py:153-184; bf16 weights [out, in], embedding 256, 8 heads, T <= 16 tokens per prompt, fp32 token rows) as two launches,
 * one workgroup per prompt (csrc/dectok.hip):
 *   dec_tok_attn: q_in = queries (+ qpe unless skip_pe); self attention (q, k of q_in, v of queries; scale 1 / sqrt(32) after the product, :233-235); out projection
 *     (+ queries unless skip_pe: layer 0 has no residual, :157-158); LayerNorm (norm1) -> queries_out; then q_t2i = (queries_out + qpe) Wq2^T + bq2, the q of the
 *     token -> image attention.  mode 1: q_t2i = (queries + qpe) Wq2^T + bq2 only (the final attention, transformer.py:99-104).
 *   dec_tok_mlp: y = LayerNorm(queries + attn Wo^T + bo) (norm2; with do_mlp 0 that is all: norm_final_attn); y = LayerNorm(y + W2 relu(W1 y + b1) + b2) (norm3) -> queries_out;
 *     k_out = (y + qpe) Wk^T + bk, v_out = y Wv^T + bv: the k / v of the image -> token attention (:176-178).
 * dec_heads: the four hypernetwork MLPs on tokens 1 .. 4 and the IoU head on token 0 (mask_decoder.py:141-149,154-176; three linears, ReLU between): w / b = HOST arrays
 *   of 15 device pointers (chain-major; a chain's last weight zero-padded to a multiple of 16 rows) -> hyper [P, nm, 32], iou [P, n_iou]. */
int ullsam_dec_tok_attn(const float* queries, const float* qpe, float* queries_out, float* q_t2i, const void* Wq, const float* bq, const void* Wk, const float* bk,
                        const void* Wv, const float* bv, const void* Wo, const float* bo, const float* ln_w, const float* ln_b, float eps, const void* Wq2,
                        const float* bq2, int P, int T, int skip_pe, int mode, void* stream);
int ullsam_dec_tok_mlp(const float* queries, const float* attn, const float* qpe, float* queries_out, float* k_out, float* v_out, const void* Wo, const float* bo,
                       const float* ln2_w, const float* ln2_b, float eps2, const void* W1, const float* b1, const void* W2, const float* b2, const float* ln3_w,
                       const float* ln3_b, float eps3, const void* Wk, const float* bk, const void* Wv, const float* bv, int P, int T, int do_mlp, void* stream);
int ullsam_dec_heads(const float* hs, const void* const* w, const float* const* b, float* hyper, float* iou, int P, int T, int n_iou, int m0, int nm, void* stream);
/* (hypernetwork chains m0 .. m0 + nm - 1 only -> hyper [P, nm, 32]: multimask output asks for masks 1 .. 3, mask_decoder.py:100-105) */
/* out[p][t] = t < n0 ? prefix[t] : rows[p][t - n0], fp32 rows of C: the decoder's token matrix (mask_decoder.py:119-123) */
int ullsam_concat_token_rows(const float* prefix, int n0, const float* rows, int n1, float* out, int P, int C, void* stream);
/* Second transposed convolution + GELU + hypernetwork product in one pass (mask_decoder.py:136-147, bf16): u1 bf16 [NB*H*W*4, 64] (first transposed convolution
 * after LayerNorm2d + GELU), w1 bf16 [128 = (ky2, kx2, c), 64], b1 fp32 [128] | NULL, hyper fp32 [NB, NM <= 8, 32] -> out fp32 [NB, NM, 4H, 4W]; the upscaled
 * embedding is never written. */
int ullsam_up2_hyper_masks(const void* u1, const void* w1, const float* b1, const float* hyper, float* out, int NB, int NM, int H, int W, void* stream);
/* First transposed convolution + LayerNorm2d + GELU in one pass (mask_decoder.py:131-138, bf16): src bf16 [rows, 256], w0 bf16 [256 = (ky, kx, c), 256],
 * b0 fp32 [256] | NULL, lnw / lnb fp32 [64] | NULL -> out bf16 [rows * 4, 64]; the fp32 result of the convolution is never written. */
int ullsam_up1_ln_gelu(const void* src, const void* w0, const float* b0, const float* lnw, const float* lnb, float eps, void* out, long rows, void* stream);
int ullsam_skinny_linear(const float* x, long ldx, const float* WT, const float* b, const float* res, long ldr, float* y,
                         long ldy, int M, int N, int K, int act, void* stream);
/* 0: keep ullsam_skinny_linear on its FMA kernel (tests compare it with the exact-fp32 MFMA kernel used for N % 32 == 0, K in {128 .. 2048}); returns the previous setting */
int ullsam_set_skinny_linear_mfma(int on); /* same layers at many prompts; WT = weight^T [K,N] */
int ullsam_sparse_embed(const float* coords, const int* labels, const float* boxes, const float* G, const float* emb,
                        float* out, int P, int Np, int pad, int C, float img_w, float img_h, void* stream); /* prompt_encoder.py:76-103 */
int ullsam_dense_pe(const float* G, float* out_nhwc, int H, int W, int C, void* stream);  /* prompt_encoder.py:230-241 */
int ullsam_mask_downscale(const float* masks, float* out_nhwc, int P, int H, int W, int C, int c1, int c2, const float* w0,
                          const float* b0, const float* g1, const float* be1, const float* w3, const float* b3,
                          const float* g4, const float* be4, const float* w6, const float* b6, void* stream); /* prompt_encoder.py:54-62 */
int ullsam_hyper_masks(int dtype, const void* up2, const float* hyper, float* out, int NB, int NM, int H, int W, int CU, void* stream); /* mask_decoder.py:143-144 */
int ullsam_resize_bilinear(const float* in, long in_plane_stride, int in_ld, int IH, int IW, float* out, unsigned char* mask,
                           int N, int OH, int OW, float thr, void* stream);              /* app.py:635-645; sam.py:154-162,123 */
int ullsam_mask_iou_counts(const unsigned char* a, const unsigned char* b, unsigned long long* counts, int N, long per,
                           void* stream);                                                /* train_joint_v2.py:683-694 */

/* Automatic-mask-generation helpers, bit-exact with utils/amg.py (integer / byte work).  mask_threshold / threshold_offset are doubles: the entries
   compare against (float)(thr + off), (float)(thr - off) and (float)thr, each rounded once from the double sum as the reference's Python floats are.  (They were floats before; ULLSAM_ABI_VERSION stayed 14 through
   that change -- the in-tree library and binding are rebuilt together by the build stamp, a caller compiled against the old header must be recompiled.) */
int ullsam_stability_score(const float* masks, long N, long per, double mask_threshold, double threshold_offset,
                           unsigned int* counts, float* score, void* stream);                 /* amg.py:156-176 */
int ullsam_mask_to_box(const unsigned char* masks, long N, int H, int W, int* boxes, void* stream);   /* amg.py:303-346 */
int ullsam_rle_pack(const unsigned char* masks, long N, int H, int W, unsigned long long* words, int* counts,
                    unsigned char* first, void* stream);                                      /* amg.py:107-135 (transpose + diff) */
int ullsam_rle_emit(const unsigned long long* words, const int* select, long N, int H, int W, const long* offsets, int* out,
                    void* stream);                                                            /* amg.py:119-133 (nonzero -> run edges) */
/* generator fast path: postprocess_masks + stability counts + mask->box + RLE change words in one pass, logits never stored */
int ullsam_amg_postprocess(const float* low, const int* index, long M, int LH, int LW, int S1, int nh, int nw, int CH, int CW,
                           int FH, int FW, int cx0, int cy0, double mask_threshold, double threshold_offset,
                           unsigned long long* words, int* rle_counts, unsigned char* first, int* boxes, unsigned int* stab,
                           void* stream);                      /* sam.py:154-162 + amg.py:156-176, 303-346, 107-135, 251-264 */
int ullsam_nms_mask(const float* boxes, int N, float iou_threshold, unsigned long long* mask, void* stream); /* torchvision.ops.nms (absent dependency) */
int ullsam_threshold_u8(const float* in, unsigned char* out, long n, float thr, void* stream); /* masks > mask_threshold */
/* Connected regions (8-connectivity) of N binary masks at once, for the generator's min_mask_region_area step.
   rle_to_mask: counts i32 = the records' uncompressed column-major counts, concatenated; offsets i64 [N + 1] into them; masks u8 [N, H, W].
     status i32 [N] (device) = 1 where a count is negative or a record's counts do not sum to H * W; no store leaves that record's mask
     (a stream-ordered call cannot know, so the binding reads `status` and raises).
   label_regions: labels i32 [N, H, W] = the row-major index, within the mask, of the raster-first pixel of the pixel's region, -1 outside
     the working set (background = 0: the non-zero pixels, 1: the zero pixels).
   remove_small_regions: mode 0 "holes" sets every region of zeros with size < area_thresh, mode 1 "islands" clears every region of ones
     with size < area_thresh (all of them small: the largest stays, the raster-first on a tie); area_thresh = ceil of the reference's float;
     changed u8 [N] = some region was small.  workspace: 16-byte aligned, N * (8 * H * W + 16) bytes, its first N * H * W int32 hold the
     labels on return; masks_out may be masks_in.  N <= 65535 per call. */
int ullsam_rle_to_mask(const int* counts, const long* offsets, long N, int H, int W, unsigned char* masks, int* status,
                       void* stream);                                                         /* amg.py:138-150 */
int ullsam_label_regions(const unsigned char* masks, long N, int H, int W, int background, int* labels,
                         void* stream);                                   /* amg.py:276 (cv2.connectedComponentsWithStats(.., 8)) */
int ullsam_remove_small_regions(const unsigned char* masks_in, unsigned char* masks_out, long N, int H, int W, int area_thresh, int mode,
                                void* workspace, long workspace_bytes, unsigned char* changed, void* stream);   /* amg.py:267-291 */
/* Instance label maps: the records of one frame painted into ONE label image, and the contingency table two label images are scored from
   (csrc/labels.hip; integer work, bit-exact with utils.amg's host forms).  N <= 65535, H * W < 2^31.
   rle_paint_labels: counts / offsets as rle_to_mask; rank i32 [N] = the paint order (a permutation of 0..N-1, larger = on top).
     raw i32 [W, H] -- TRANSPOSED, raw[x * H + y] -- is zero-filled, then = 1 + the largest rank among the records covering the pixel
     (the app's sequential overwrite).  status i32 [N] = 1 where a count is negative, the counts do not sum to H * W or the rank is outside
     0..N-1; no store leaves the frame and no label exceeds N.
   label_stats: areas i32 [N + 1], boxes i32 [N + 1, 4] (x0, y0, x1, y1 inclusive) of the pixels carrying each RAW label (entry 0 unused;
     a label that is not visible keeps area 0 and the box INT_MAX, INT_MAX, -1, -1).
   label_compact: a raw label is dropped when its visible area is 0 or < min_visible_area; the others are renumbered 1..K in paint order.
     map i32 [N + 1] (raw -> final label, 0 = dropped), label_of_record i32 [N], areas i32 [N] / boxes i32 [N, 4] (first K entries), K i32 [1].
   label_remap: labels i32 [H, W] (row-major) = map[raw[x * H + y]].
   label_overlap: a, b i32 [H, W] with ids in 0..na / 0..nb -> T u64 [na + 1, nb + 1], T[i, j] = #{p : a[p] = i and b[p] = j} (zeroed here);
     status i32 [1] = 1 when an id lies outside its range (that pixel is skipped).  (na + 1) * (nb + 1) <= 2^26.
   resize_nearest_i32: in i32 [IH, IW] (row stride in_ld) resized to a virtual [OH, OW] by src = min(((2 dst + 1) * in) / (2 * out), in - 1)
     per axis (Image.NEAREST); the window (top, left, h, w) of it is written to out (row stride out_ld). */
int ullsam_rle_paint_labels(const int* counts, const long* offsets, const int* rank, long N, int H, int W, int* raw, int* status,
                            void* stream);                                                    /* app.py:688-707 */
int ullsam_label_stats(const int* raw, long N, int H, int W, int* areas, int* boxes, void* stream);
int ullsam_label_compact(const int* areas_raw, const int* boxes_raw, const int* rank, long N, int min_visible_area, int* map,
                         int* label_of_record, int* areas, int* boxes, int* K, void* stream);
int ullsam_label_remap(const int* raw, const int* map, long N, int H, int W, int* labels, void* stream);   /* app.py:707 */
int ullsam_label_overlap(const int* a, const int* b, int H, int W, int na, int nb, unsigned long long* T, int* status, void* stream);
int ullsam_resize_nearest_i32(const int* in, long in_ld, int IH, int IW, int OH, int OW, int top, int left, int h, int w, int* out,
                              long out_ld, void* stream);                                     /* app.py:807-826, 145 reverse_padding */
/* Tiled segment-everything: per-tile label maps stitched into one label image (csrc/mosaic.hip; integer work, bit-exact with the host form
   utils.mosaic.stitch_label_maps; definition in DESIGN.md "7b, continued (mosaic)").  tiles i32 [T, th, tw], tile t with ids 0..K_t;
   base i32 [T + 1] = the exclusive sum of the K_t, G = base[T] <= 2^31 - 2; the global id of (t, l > 0) is base[t] + l.  T <= 65535.
   flags i32 [4]: [0] = 1 when an id lies outside 0..K_t (it reads as background) or a descriptor leaves its tile / the frame (it is not
   walked), [1] = 1 when the pair table refused a key, [2] = the number of distinct pairs; ([3] is free for K).
   mosaic_seams: seams i32 [S, 9] = (s, t, sy, sx, ty, tx, h, w, dir): the intersection of the boxes of tile s and its right (dir 0) or lower
     (dir 1) neighbour t, as an h x w window at (sy, sx) of s and (ty, tx) of t; max_rows = the largest h.  Zeroes its outputs, then counts
     areas i32 [G + 1, 4]: areas[g, c] = the pixels of g inside the seam on side c of its tile (0 left, 1 right, 2 up, 3 down), and the
     pairs: keys u64 [cap] (dir << 63 | g_a << 32 | g_b, 0 = empty slot, open addressing), counts i32 [cap] = #{p : s(p) = a, t(p) = b},
     a, b > 0.  cap a power of two >= 2 * max_pairs; more than max_pairs distinct pairs set flags[1] / show in flags[2].
   mosaic_union: parent i32 [G + 1] = the smallest global id of the component of g in the graph of the merged pairs; a pair of the table
     merges when n > 0 and n * den >= num * (A_s(a) + A_t(b) - n) (64-bit; 0 < num <= den < 2^31), every pair when areas is NULL
     (counts is not read then, and cap is any length).
   mosaic_stats: cores i32 [T, 6] = (top, left, h, w of the tile's core in the [H, W] frame, then the tile's origin oy, ox); max_rows = the
     largest h.  areas_raw i32 [G + 1], boxes_raw i32 [G + 1, 4] (inclusive XYXY) of the core pixels per REPRESENTATIVE; others keep area 0
     and the box INT_MAX, INT_MAX, -1, -1.
   mosaic_compact: a representative is dropped when its area is 0 or < min_visible_area, the others are renumbered 1..K by ascending id:
     label_of_global i32 [G + 1] (0 = dropped, members follow their representative), areas i32 [G] / boxes i32 [G, 4] (first K entries), K i32 [1].
   mosaic_paste: labels i32 [H, W][p] = label_of_global[base[t] + tile_t[p - origin_t]] for p in the core of t (0 where the tile says 0);
     the cores partition the frame, so every pixel is written once; the frame is indexed in 64 bits. */
int ullsam_mosaic_seams(const int* tiles, int T, int th, int tw, const int* base, long G, const int* seams, int S, int max_rows,
                        unsigned long long* keys, int* counts, long cap, int max_pairs, int* areas, int* flags, void* stream);
int ullsam_mosaic_union(const unsigned long long* keys, const int* counts, long cap, const int* areas, long G, long num, long den, int* parent,
                        int* flags, void* stream);
int ullsam_mosaic_stats(const int* tiles, int T, int th, int tw, const int* base, long G, const int* cores, int max_rows, const int* parent,
                        int H, int W, int* areas_raw, int* boxes_raw, int* flags, void* stream);
int ullsam_mosaic_compact(const int* areas_raw, const int* boxes_raw, const int* parent, long G, int min_visible_area, int* label_of_global,
                          int* areas, int* boxes, int* K, void* stream);
int ullsam_mosaic_paste(const int* tiles, int T, int th, int tw, const int* base, long G, const int* cores, int max_rows,
                        const int* label_of_global, int H, int W, int* labels, void* stream);
/* Z-stacks and time-lapse: per-plane label maps linked along the third axis into 3-D objects (csrc/stack.hip; integer work, bit-exact with the
   host form utils.stack.link_label_stack; definition in DESIGN.md "7b, continued (stacks)").  planes i32 [Z, H, W], plane z with ids 0..K_z;
   base i32 [Z + 1] = the exclusive sum of the K_z, G = base[Z] <= 2^31 - 2; the global id of (z, l > 0) is base[z] + l.  Z <= 65535,
   H, W <= 46340.  0 < num <= den < 2^31.  flags i32 [4]: [0] = 1 when an id lies outside 0..K_z (it reads as background) or a table holds
   what no stack produces (it is skipped), [1] = 1 when the pair table refused a key, [2] = the number of distinct pairs; ([3] is free for K).
   stack_pairs: zeroes its outputs, then counts areas i32 [G + 1] = the pixels of g in its own plane, and the pairs of every two consecutive
     planes: keys u64 [cap] (g_a << 32 | g_b, a in plane z, b in plane z + 1, both > 0; 0 = empty slot, open addressing), counts i32 [cap] =
     #{p : plane_z(p) = a, plane_z+1(p) = b}.  cap a power of two >= 2 * max_pairs; more than max_pairs distinct pairs set flags[1] / show
     in flags[2].
   stack_best: a slot is a candidate when n > 0 and n * den >= num * u, u = A(a) + A(b) - n.  succ i32 [G + 1][a] = the partner b of a's best
     candidate, pred i32 [G + 1][b] = the partner a of b's best candidate, 0 where there is none; best = the largest n / u, compared exactly
     (n1 * u2 against n2 * u1 in 64 bits), equal ones by the smaller partner id.  cap is any length; a key needs 1 <= g_a < g_b <= G.
   stack_link: parent i32 [G + 1] = the smallest global id of the component of g.  With succ / pred (stack_best's): (a, b) is linked iff
     succ[a] = b and pred[b] = a, components are chains (keys, counts, areas are not read).  With succ = pred = NULL: every candidate of
     the table is a link.
   stack_stats: voxels_raw i64 [G + 1], zrange_raw i32 [G + 1, 2] (first and last plane), boxes_raw i32 [G + 1, 4] (inclusive XYXY over all
     planes) per REPRESENTATIVE; others keep 0 voxels, the range INT_MAX, -1 and the box INT_MAX, INT_MAX, -1, -1.
   stack_compact: a representative is dropped when its voxels are 0 or < min_volume or it spans fewer than min_planes planes, the others
     are renumbered 1..K by ascending id: label_of_global i32 [G + 1] (0 = dropped, members follow their representative), voxels i64 [G] /
     zrange i32 [G, 2] / boxes i32 [G, 4] (first K entries), K i32 [1].
   stack_relabel: volume i32 [Z, H, W][z, p] = label_of_global[base[z] + plane_z[p]] (0 where the plane says 0); indexed in 64 bits. */
int ullsam_stack_pairs(const int* planes, int Z, int H, int W, const int* base, long G, unsigned long long* keys, int* counts, long cap,
                       int max_pairs, int* areas, int* flags, void* stream);
int ullsam_stack_best(const unsigned long long* keys, const int* counts, long cap, const int* areas, long G, long num, long den, int* succ,
                      int* pred, int* flags, void* stream);
int ullsam_stack_link(const int* succ, const int* pred, const unsigned long long* keys, const int* counts, long cap, const int* areas, long G,
                      long num, long den, int* parent, int* flags, void* stream);
int ullsam_stack_stats(const int* planes, int Z, int H, int W, const int* base, long G, const int* parent, long* voxels_raw, int* zrange_raw,
                       int* boxes_raw, int* flags, void* stream);
int ullsam_stack_compact(const long* voxels_raw, const int* zrange_raw, const int* boxes_raw, const int* parent, long G, int min_planes,
                         long min_volume, int* label_of_global, long* voxels, int* zrange, int* boxes, int* K, void* stream);
int ullsam_stack_relabel(const int* planes, int Z, int H, int W, const int* base, long G, const int* label_of_global, int* volume, void* stream);
/* Exact squared Euclidean distance transforms of a label image (csrc/distance.hip; integer work, bit-exact with the host forms of
   utils.distance; definition in DESIGN.md "7b, continued (distances)").  labels i32 [H, W], 0 = background, 1 <= H, W <= 32767.  INF = 2^31 - 1;
   in the 16-bit column maps 0xFFFF says "none".  flags i32 [4]: [0] = 1 when a label is negative or above K (the pixel is skipped, nothing is
   indexed with it); the entries only ever set it, the caller zeroes it.
   distance_columns: feature = 0: g u16 [H, W] = the vertical distance from a labelled pixel to the nearest pixel of its column with another
     label (the pixels just outside the frame count when edge is set; 0xFFFF at an open frame end; 0 on the background), nearest is not
     touched.  feature = 1: g = the vertical distance to the nearest labelled pixel of the column (0xFFFF: the column has none), nearest
     i32 [H, W] = its label, the smaller of the two at equal distance above and below (0 with 0xFFFF).
   distance_rows: the row pass over distance_columns' maps (feature = 0 for the modes 0, 3, 4; feature = 1 for 1, 2).  mode 0: out0 = D2, the
     squared distance of every labelled pixel to the nearest pixel with another label (0 on the background); 1: out0 = D2 to the nearest
     labelled pixel, out1 = the smallest label among the pixels that attain it, both (INF, 0) where D2 > limit; 2: out0 = the label, or on the
     background the nearest label where D2 <= limit, else 0; 3: out0 = the label where its D2 > limit, else 0; 4: best u64 [K] is zeroed and
     takes per label the maximum of D2 << 32 | (0xFFFFFFFF - linear index) over its pixels.  limit in 0..INF; the modes 0 and 4 need INF.  No
     scan looks farther than floor(sqrt(limit)) columns (W when limit = INF).  route 0: that reach <= 128 stages the row segment in LDS,
     a longer one reads global memory; 1: LDS (an error beyond 128); 2: global memory.  The outputs do not depend on the route.
   distance_depth_decode: r2 i32 [K] = best >> 32, xy i32 [K, 2] = (x, y) of the linear index; a zero word (an absent id) gives 0, (-1, -1). */
int ullsam_distance_columns(const int* labels, int H, int W, int feature, int edge, long K, unsigned short* g, int* nearest, int* flags,
                            void* stream);
int ullsam_distance_rows(const int* labels, const unsigned short* g, const int* nearest, int H, int W, int mode, int edge, long limit, int route,
                         long K, int* out0, int* out1, unsigned long long* best, int* flags, void* stream);
int ullsam_distance_depth_decode(const unsigned long long* best, long K, int W, int* r2, int* xy, void* stream);
/* The same transforms of a label volume with anisotropic voxels (csrc/distance3d.hip; integer work, bit-exact with the host forms of
   utils.distance3d; definition in DESIGN.md "7b, continued (3-D distances)").  volume i32 [Z, H, W], 0 = background, 1 <= Z, H, W <= 32767,
   Z * H * W <= 2^31 - 1.  (sz, sy, sx) in 1..46340: |p - q|^2 = sz^2 dz^2 + sy^2 dy^2 + sx^2 dx^2.  (ez, ey, ex): the voxels just outside the
   volume along that axis count as another label (inner modes only; the feature modes need 0, 0, 0).  The y and x entries refuse
   B = sum of s_a^2 (n_a - 1 + e_a)^2 > 2^31 - 2, so every finite result fits int32; INF = 2^31 - 1, 0xFFFF in the 16-bit map.  flags as above.
   distance3d_z: feature = 0: g u16 [Z, H, W] = the distance in voxels from a labelled voxel to the end of its run of equal label along z,
     plus 1 (0xFFFF where both ends are open; 0 on the background).  feature = 1: g = the distance in voxels to the nearest labelled voxel of
     the (y, x) column (0xFFFF: none), nearest i32 [Z, H, W] = its label, the smaller of the two at equal distance (0 with 0xFFFF).
   distance3d_y: feature = 0: h i32 [Z, H, W] = the inner distance within the (z, y) plane of the voxel (INF: none; 0 on the background),
     hlabel is not touched.  feature = 1: (h, hlabel) = the distance to the nearest labelled voxel of that plane and the smallest label that
     attains it.  No scan looks farther than floor(sqrt(limit) / sy) voxels; beyond limit h is some value above limit.
   distance3d_x: the x pass over distance3d_y's maps with distance_rows' modes 0..4 (out0, out1 i32 [Z, H, W]; best u64 [K], the linear index
     being (z * H + y) * W + x); the modes 0 and 4 need limit = INF.  No scan looks farther than floor(sqrt(limit) / sx) voxels.
   distance3d_depth_decode: r2 i32 [K] = best >> 32, xyz i32 [K, 3] = (x, y, z) of the linear index; a zero word gives 0, (-1, -1, -1). */
int ullsam_distance3d_z(const int* volume, int Z, int H, int W, int feature, int ez, long K, unsigned short* g, int* nearest, int* flags,
                        void* stream);
int ullsam_distance3d_y(const int* volume, const unsigned short* g, const int* nearest, int Z, int H, int W, int feature, int sz, int sy, int sx,
                        int ez, int ey, int ex, long limit, int* h, int* hlabel, void* stream);
int ullsam_distance3d_x(const int* volume, const int* h, const int* hlabel, int Z, int H, int W, int mode, int sz, int sy, int sx, int ez, int ey,
                        int ex, long limit, long K, int* out0, int* out1, unsigned long long* best, int* flags, void* stream);
int ullsam_distance3d_depth_decode(const unsigned long long* best, long K, int H, int W, int* r2, int* xyz, void* stream);
/* Splitting the touching objects of a label image: a watershed of every instance's own depth map without a flood (csrc/split.hip; integer
   work, bit-exact with the host form utils.split.split_labels; definition in DESIGN.md "7b, continued (splitting)").  labels i32 [H, W] with ids
   0..K, 0 = background, 1 <= H, W <= 32767; d2 i32 [H, W] = distance_rows' mode 0 of the same labels; p = y * W + x, n = H * W;
   key(p) = (d2[p], -p).  flags i32 [8], zeroed by the caller, only ever raised: [0] = a label below 0 or above K (the pixel counts as background)
   or a hand-made table entry outside the frame (skipped), [1] = a pair was refused, [2] = the pairs claimed, [3] = a chain longer than
   its bound, [4] = the representatives counted, [5] = the cursor of the list.
   split_ascent: up i32 [H, W][p] = the pixel of greatest key among p and its 8 neighbours with p's label; p on the background.  route 0 / 1: a
     workgroup stages its 64 x 4 pixels and a one-pixel halo in LDS; 2: global memory.  The output does not depend on the route.
   split_flatten: up[p] = the root of p's chain (up[r] = r), in place, after at most `steps` <= n hops (flags[3] otherwise).
   split_passes: keys u64 [cap] / vals i32 [cap]: the open-addressing pair table (cap a power of two >= 2 * max_pairs; both are zeroed here).  For
     every 8-adjacent pixel pair of one label whose roots a < b differ (up flattened), vals of key a << 32 | b takes the maximum of
     min(d2, d2).  Once more than max_pairs keys are held new ones are refused and flags[1] is set.
   split_round: one round of merging over a pair table (cap slots, key 0 = empty; hand-made ones need no power of two) and flat maps of n
     pixels.  Every edge whose ends lie in different components X = up[a] != Y = up[b] sends S << 32 | (0xFFFFFFFF - Y) to best[X] and the
     mirrored word to best[Y] (u64 [n], zeroed by the caller once; the round leaves it zero again) with a 64-bit atomicMax; then every root X
     with a word (S, Y) writes up[X] = Y and changed[0] = 1 when key(X) < key(Y) and, with t = d2[X] - S - h * h, t <= 0 or
     t * t <= 4 * h * h * S (unsigned 64-bit).  0 <= h <= 32767.  The caller flattens before the next round.
   split_collect: list = NULL: flags[4] += the number of representatives (up[p] = p on a labelled pixel); otherwise list u64 [room] takes
     label << 32 | p of each, in no particular order, from flags[5] on while there is room.
   split_relabel: list u64 [parts], sorted ascending.  Part i gets id i + 1: parent i32 [parts] = its label, peak_r2 i32 [parts] = d2 at its
     representative, peak_xy i32 [parts, 2] = (x, y) of it, parts_of i32 [K] (zeroed here) counts the parts per label; newid i32 [H, W] is
     scratch; out i32 [H, W][p] = the id of up[p]'s part, 0 on the background. */
int ullsam_split_ascent(const int* labels, const int* d2, int H, int W, long K, int route, int* up, int* flags, void* stream);
int ullsam_split_flatten(int* up, long n, long steps, int* flags, void* stream);
int ullsam_split_passes(const int* labels, const int* d2, const int* up, int H, int W, long K, unsigned long long* keys, int* vals, long cap,
                        int max_pairs, int* flags, void* stream);
int ullsam_split_round(const unsigned long long* keys, const int* vals, long cap, const int* labels, const int* d2, long n, long K, int h,
                       unsigned long long* best, int* up, int* changed, int* flags, void* stream);
int ullsam_split_collect(const int* labels, const int* up, long n, long K, unsigned long long* list, long room, int* flags, void* stream);
int ullsam_split_relabel(const unsigned long long* list, long parts, const int* labels, const int* d2, const int* up, int H, int W, long K,
                         int* newid, int* out, int* parent, int* peak_r2, int* peak_xy, int* parts_of, int* flags, void* stream);
/* The same split of a label volume (csrc/split3d.hip; integer work, bit-exact with the host form utils.split3d.split_labels3d; definition in
   DESIGN.md "7b, continued (3-D splitting)").  labels i32 [Z, H, W] with ids 0..K, 0 = background, 1 <= Z, H, W <= 32767 and
   n = Z * H * W <= 32767^2 (the bound of split_flatten / split_round / split_collect, which run on the flattened volume as they are);
   d2 i32 [Z, H, W] = distance3d_x's mode 0 of the same volume; p = (z * H + y) * W + x; key(p) = (d2[p], -p).  flags i32 [8] with split_*'s
   meanings.
   split3d_ascent: up i32 [Z, H, W][p] = the voxel of greatest key among p and its 26 neighbours with p's label; p on the background and on
     a label outside 1..K (flags[0]).  route 0 / 1: a workgroup stages its 64 x 4 x 4 voxels and a one-voxel halo in LDS (the volume's outside
     enters as label 0); 2: global memory.  The output does not depend on the route.
   split3d_passes: split_passes' table (same layout, same flags; cap a power of two >= 2 * max_pairs; keys and vals are zeroed here) over the
     13 forward neighbours (dz, dy, dx) > (0, 0, 0): every 26-adjacent voxel pair of one label whose roots a < b differ (up flattened) sends
     min(d2, d2) to the maximum under key a << 32 | b.  The table goes into split_round as it is.
   split3d_relabel: list u64 [parts] (split_collect's, sorted ascending).  Part i gets id i + 1: parent i32 [parts], peak_r2 i32 [parts] = d2 at
     its representative p, peak_xyz i32 [parts, 3] = (p % W, (p / W) % H, p / (W * H)), parts_of i32 [K] (zeroed here); newid i32 [Z, H, W] is
     scratch; out i32 [Z, H, W][p] = the id of up[p]'s part, 0 on the background. */
int ullsam_split3d_ascent(const int* labels, const int* d2, int Z, int H, int W, long K, int route, int* up, int* flags, void* stream);
int ullsam_split3d_passes(const int* labels, const int* d2, const int* up, int Z, int H, int W, long K, unsigned long long* keys, int* vals, long cap,
                          int max_pairs, int* flags, void* stream);
int ullsam_split3d_relabel(const unsigned long long* list, long parts, const int* labels, const int* d2, const int* up, int Z, int H, int W, long K,
                           int* newid, int* out, int* parent, int* peak_r2, int* peak_xyz, int* parts_of, int* flags, void* stream);
/* Outlines of a label image: every instance as closed polygon loops on the pixel lattice (csrc/outline.hip; integer work, bit-exact with the
   host form utils.outline.label_outlines; definition in DESIGN.md "7b, continued (outlines)").  labels i32 [H, W] with ids 0..K, 0 =
   background, 1 <= H, W and n = H * W < 2^29; p = y * W + x.  Side s of a pixel of label k > 0 whose 4-neighbour is not k (the frame's outside
   included) is a directed unit edge with the instance on its right: 0 = top (east), 1 = right (south), 2 = bottom (west), 3 = left (north); its
   id is 4 * p + s, its compact index its position among the E edges in id order.  flags i32 [8], zeroed by the caller, only ever raised: [0] = a
   label below 0 or above K (the pixel counts as background) or an index of a hand-made table outside its range (skipped), [1] = E, [2] = the
   corners, [3] = the leaders, [4] = the cursor of the list, [5] = a parent chain longer than L.
   outline_sides: mask u8 [n]: bit s = side s is an edge; off i32 [n] = the exclusive scan of popcount(mask), so edge (p, s) has the compact index
     off[p] + popcount(mask[p] & ((1 << s) - 1)); flags[1] = E.  sums i32 [ceil(n / 2048)] is scratch.
   outline_scan: off i32 [n] = the exclusive scan of (vals[i] != 0) over vals u8 [n], total[0] = their number; sums as above.
   outline_successors: eid i32 [E] = the edge ids; succ i32 [E] = the compact index of the edge of the same label that starts at the head.  With
     AL / AR the pixels ahead-left / ahead-right of the head: connectivity 8 turns left when AL == k, else goes straight when AR == k, else turns
     right; connectivity 4 turns right unless AR == k, and then left when AL == k too, else straight.  Left: side (s + 3) % 4 of AL; straight: side
     s of AR; right: side (s + 1) % 4 of the same pixel.  pdir u8 [E][succ[e]] = the side of e.
   outline_rank: ws i32 [2, E, 4], aligned to 16 bytes, is scratch (the words (mn, pos, jump, 0) of every edge, twice); `rounds` = ceil(log2 E)
     rounds of pointer doubling, never in place.  leader i32 [E] = the smallest compact index on e's cycle, rank i32 [E] = the steps from the
     leader to e.  flags[3] += the leaders (leader[e] = e), flags[2] += the corners (pdir[e] != eid[e] & 3).
   outline_collect: list u64 [room] takes labels[eid[e] >> 2] << 32 | e of every leader, in no particular order, from flags[4] on.
   outline_loops: loop_of i32 [E] holds, at every leader, the index of its loop in 0..L - 1.  edges i32 [L] = the edges of every loop, area2
     i64 [L] = the sum of x_t * y_h - x_h * y_t over them (tail t, head h): > 0 an outer loop, < 0 a hole.  Both are zeroed here.
   outline_order: estart i32 [L] = the exclusive scan of `edges`.  Slot estart[loop of e] + rank[e] of reid i32 [E] / corner u8 [E] takes eid[e] /
     (pdir[e] != eid[e] & 3): the edges loop after loop, each in travel order from its leader.
   outline_vertices: coff = outline_scan of corner; vertices i32 [N, 2][coff[i]] = the tail (x, y) of reid[i] where corner[i].
   outline_parents: lead i32 [L] = the compact index of every loop's leader.  parent i32 [L][i] = i for an outer loop; a hole walks left from its
     leader's pixel while the label lasts, takes the loop of that pixel's left side, and repeats from that loop's leader until area2 > 0. */
int ullsam_outline_sides(const int* labels, int H, int W, long K, unsigned char* mask, int* off, int* sums, int* flags, void* stream);
int ullsam_outline_scan(const unsigned char* vals, long n, int* off, int* sums, int* total, void* stream);
int ullsam_outline_successors(const int* labels, int H, int W, const unsigned char* mask, const int* off, long E, int connectivity, int* eid,
                              int* succ, unsigned char* pdir, int* flags, void* stream);
int ullsam_outline_rank(const int* succ, const int* eid, const unsigned char* pdir, long E, int rounds, int* ws, int* leader, int* rank, int* flags,
                        void* stream);
int ullsam_outline_collect(const int* labels, long n, const int* eid, const int* leader, long E, unsigned long long* list, long room, int* flags,
                           void* stream);
int ullsam_outline_loops(const int* eid, const int* leader, const int* loop_of, long E, long L, int W, int* edges, long long* area2, int* flags,
                         void* stream);
int ullsam_outline_order(const int* eid, const unsigned char* pdir, const int* leader, const int* rank, const int* loop_of, const int* estart, long E,
                         long L, int* reid, unsigned char* corner, int* flags, void* stream);
int ullsam_outline_vertices(const int* reid, const unsigned char* corner, const int* coff, long E, int W, long N, int* vertices, void* stream);
int ullsam_outline_parents(const int* labels, int H, int W, const unsigned char* mask, const int* off, const int* eid, const int* leader,
                           const int* loop_of, const int* lead, const long long* area2, long E, long L, int* parent, int* flags, void* stream);
/* Simplified outlines of a label image: Douglas-Peucker on label_outlines' loops with exact integer arithmetic, shared borders kept watertight
   (csrc/simplify.hip; integer work, bit-exact with the host form utils.simplify.simplify_outlines; definition in DESIGN.md "7b, continued
   (simplifying)").  1 <= H, W <= 32767 and H * W < 2^29.  reid i32 [E] / corner u8 [E] are outline_order's copy, estart i32 [L] the first slot
   of every loop.  A lattice point is packed as y << 16 | x.  C candidates, L loops, L <= C.  flags i32 [4], zeroed by the caller, only ever
   raised: [0] = an index or value of a hand-made table outside its range (skipped; nothing is indexed with it).
   simplify_flags: cand u8 [E]: bit 0 = the tail of slot i is a candidate (a corner, or a fixed point), bit 1 = a fixed point: at least three of the
     four pixel sides that meet there separate different values (the frame's outside is 0).
   simplify_candidates: coff = outline_scan of cand.  cxy i32 [C] = the points, cloop i32 [C] = their loops, kept u8 [C] = fixed, nfixed i32 [L] =
     the fixed candidates of every loop (all set here).
   simplify_anchors: in a loop with nfixed = 0 the candidate of smallest (y, x), and the one of largest squared distance from it (ties: smallest
     (y, x)), become kept.  ws u64 [2, L] is scratch.
   simplify_segments: koff = outline_scan of kept, total i32 [1] its sum (on the device); cstart i32 [L + 1]: loop l owns candidates cstart[l] :
     cstart[l + 1].  pa / pb i32 [C] = the kept candidates before / after every candidate that is not kept, cyclic in its loop (-1 for a kept
     one).  klist i32 [C] is scratch.
   simplify_rounds: `rounds` rounds.  In each, among the open candidates of a segment (those with the same pa) the one with the largest num against
     the chord pa -> pb (ties: smallest (y, x)) becomes kept iff num > (T2 * den) >> 16, and the others move pa or pb to it; a segment without
     such a candidate is closed (pa = -1).  T2 = T * T, T = the tolerance in 1/256 pixel, T <= 255 * 256.  counts i32 [rounds] (zeroed here)[r] =
     the candidates round r kept.  ws u64 [3, C] is scratch.
   simplify_rings: voff = outline_scan of kept, total i32 [1] = N its sum.  vertices i32 [N, 2][voff[i]] = (x, y) of every kept candidate; nvert
     i32 [L] / area2 i64 [L] = the vertices and the shoelace sum of every loop's ring (zeroed here).  klist i32 [C] is scratch. */
int ullsam_simplify_flags(const int* labels, int H, int W, const int* reid, const unsigned char* corner, long E, unsigned char* cand, int* flags,
                          void* stream);
int ullsam_simplify_candidates(const int* reid, const unsigned char* cand, const int* coff, const int* estart, long E, long L, long C, int H, int W,
                               int* cxy, int* cloop, unsigned char* kept, int* nfixed, int* flags, void* stream);
int ullsam_simplify_anchors(const int* cxy, const int* cloop, const int* nfixed, long C, long L, unsigned long long* ws, unsigned char* kept,
                            int* flags, void* stream);
int ullsam_simplify_segments(const unsigned char* kept, const int* koff, const int* total, const int* cloop, const int* cstart, long C, long L,
                             int* klist, int* pa, int* pb, int* flags, void* stream);
int ullsam_simplify_rounds(const int* cxy, const int* cloop, const int* cstart, long C, long L, long long T2, int rounds, unsigned long long* ws,
                           int* pa, int* pb, unsigned char* kept, int* counts, int* flags, void* stream);
int ullsam_simplify_rings(const int* cxy, const int* cloop, const unsigned char* kept, const int* voff, const int* total, const int* cstart, long C,
                          long L, long N, int* klist, int* vertices, int* nvert, long long* area2, int* flags, void* stream);
/* Polygons to an instance label image: exact scanline rasterisation in fixed point (csrc/raster.hip; integer work, bit-exact with the host form
   utils.raster.rasterize_polygons; definition in DESIGN.md "7b, continued (rasterising)").  q i32 [N, 2] = the vertices (x, y) in 1/256 pixel,
   |q| <= 65535 * 256; start i32 [R + 1]: ring r owns q[start[r] : start[r + 1]], open (the last vertex joins the first); ring_label i32 [R] in
   1..K; 1 <= H, W <= 32767, K <= 65535.  Edge i runs from vertex i to the next vertex of its ring; the centre of pixel (x, y) is (256 x + 128,
   256 y + 128).  flags i32 [4], zeroed by the caller, only ever raised: [0] = status bits (1 = a ring_label outside 1..K, 2 = a coordinate beyond
   the range, 4 = a total above 2^31 - 1, 8 = an index or value of a hand-made table outside its range; what is flagged is skipped, nothing is
   indexed with it), [1] = C, the crossings.
   raster_scan: off i32 [n] = the exclusive scan of vals i32 [n] (each in 0..32767, else it counts as 0 and bit 8), total[0] = their sum, held at
     2^31 - 1 with bit 4 when it is larger.  sums i32 [ceil(n / 2048)] is scratch.
   raster_edges: per edge row0 / cnt i32 [N] = the first and the number of the rows y in 0..H - 1 with min(y0, y1) <= 256 y + 128 < max(y0, y1)
     (row0 = 0 where cnt = 0), nxt i32 [N] = the index of the edge's second vertex, elab i32 [N] = its label (0 for a flagged edge: it crosses
     nothing); off i32 [N] = the exclusive scan of cnt, flags[1] = C.
   raster_keys: crossing c belongs to the edge e with off[e] <= c < off[e] + cnt[e] and to row y = row0[e] + c - off[e].  With the endpoints ordered
     by y, d = y1 - y0, cy = 256 y + 128: A = (x0 - 128) d + (cy - y0)(x1 - x0), B = 256 d, xs = clamp(ceil(A / B), 0, W): the crossing toggles the
     pixels x >= xs of the row.  keys i64 [C][c] = label << 32 | y << 16 | xs (0 for a flagged crossing).
   raster_covered: keys SORTED; entries 2 j, 2 j + 1 are span j = [xs_a, xs_b) of one (label, row).  covered i32 [K][k - 1] = the sum of the span
     lengths of label k (zeroed here); len i32 [C / 2] (may be null) = the span lengths.
   raster_paint: raw i32 [H, W] (zeroed here) = 1 + the largest rank[label - 1] (rank i32 [K], values in 0..K - 1) among the spans covering the
     pixel.  form 0: one wave per span; form 1: one lane per pixel, poff i32 [C / 2] = raster_scan of len and total i32 [1] its sum, on the device.
   raster_finish: label_of i32 [K + 1] = the label of every raw value (label_of[0] = 0).  labels i32 [H, W] = label_of[raw]; area i32 [K] = the
     pixels of every label, box i32 [K, 4] = their inclusive XYXY box, (INT_MAX, INT_MAX, -1, -1) where there are none (both set here). */
int ullsam_raster_scan(const int* vals, long n, int* off, int* sums, int* total, int* flags, void* stream);
int ullsam_raster_edges(const int* q, long N, const int* start, long R, const int* ring_label, int H, int W, long K, int* row0, int* cnt, int* nxt,
                        int* elab, int* off, int* sums, int* flags, void* stream);
int ullsam_raster_keys(const int* q, long N, const int* row0, const int* cnt, const int* nxt, const int* elab, const int* off, long C, int H, int W,
                       long K, long long* keys, int* flags, void* stream);
int ullsam_raster_covered(const long long* keys, long C, int H, int W, long K, int* covered, int* len, int* flags, void* stream);
int ullsam_raster_paint(const long long* keys, long C, const int* rank, int H, int W, long K, int form, const int* poff, const int* total, int* raw,
                        int* flags, void* stream);
int ullsam_raster_finish(const int* raw, int H, int W, const int* label_of, long K, int* labels, int* area, int* box, int* flags, void* stream);
/* Per-instance measurements and contacts from a label image (csrc/measure.hip; integer work, bit-exact with the host forms
   utils.measure.measure_instances / label_contacts; definition in DESIGN.md "7b, continued: measurements").  labels i32 [H, W] with ids
   0..K, 0 = background, 1 <= H, W <= 46340 (x * x and every area stay below 2^31, every sum below 2^62), K <= 2^31 - 2.  Row k - 1 of every
   table belongs to label k; both entries set all of their outputs themselves (init kernels), the caller zeroes nothing.
   flags i32 [4]: [0] = 1 when an id lies outside 0..K (it reads as background; no table is indexed with it), [1] = 1 when the pair table
   refused a key, [2] = the number of distinct pairs, [3] = the number of rows label_contacts wrote.
   measure_instances: area i64 [K]; box i32 [K, 4] inclusive XYXY, (INT_MAX, INT_MAX, -1, -1) for an absent label; moments i64 [K, 5] = sum x,
     sum y, sum x^2, sum y^2, sum xy in frame coordinates; perimeter i64 [K, 3] = boundary pixels (pixels of k with a 4-neighbour that is not
     k), edges (pixel sides of k facing "not k"), contact edges (those facing another instance); the frame's outside is "not k" and is no
     instance.  intensity: NULL with channels = 0, else u8 (sample_bytes 1) or u16 (2) interleaved [H, W, channels], channels <= 4, any
     element-aligned address: isum / isum2 i64 [K, channels] = sum v, sum v^2; imin / imax i32 [K, channels], (INT_MAX, -1) for an absent label.
     lds_slots: the entries of the per-workgroup LDS table the runs are summed in before one global atomic per quantity and label (0 or a
     power of two <= 128; 0 = every run straight to the global tables; the results are the same).
   label_contacts: keys u64 [cap] / counts i64 [cap]: the open-addressing pair table (key a << 32 | b, 0 < a < b; cap a power of two
     >= 2 * max_pairs), counts = the pixel sides shared by a pixel of a and a 4-neighbour pixel of b, every adjacent pixel pair counted once
     (right and down); rows i64 [max_pairs, 2] = (key, n) of the claimed slots in no particular order, flags[3] of them. */
int ullsam_measure_instances(const int* labels, int H, int W, int K, const void* intensity, int channels, int sample_bytes, int lds_slots,
                             long* area, int* box, long* moments, long* perimeter, long* isum, long* isum2, int* imin, int* imax, int* flags,
                             void* stream);
int ullsam_label_contacts(const int* labels, int H, int W, int K, unsigned long long* keys, long* counts, long cap, int max_pairs, long* rows,
                          int* flags, void* stream);
/* Per-object measurements and contacts from a label VOLUME (csrc/measure3d.hip; integer work, bit-exact with the host forms
   utils.measure3d.measure_objects / object_contacts; definition in DESIGN.md "7b, continued (3-D measurements)").  volume i32 [Z, H, W] with
   ids 0..K, 0 = background, 1 <= Z, H, W <= 32767 and Z * H * W <= 2^31 - 1 (x * x < 2^30 and every count < 2^31: every coordinate sum stays
   below 2^61, sum v^2 below 65535^2 (2^31 - 1) < 2^63), K <= 2^31 - 2.  Row k - 1 of every table belongs to id k; both entries set all of
   their outputs themselves (init kernels), the caller zeroes nothing.
   flags i32 [4]: [0] = 1 when an id lies outside 0..K (it reads as background; no table is indexed with it), [1] = 1 when the pair table
   refused a key, [2] = the number of distinct pairs, [3] = the number of rows object_contacts3d wrote.
   measure_objects3d: voxels i64 [K]; box i32 [K, 6] inclusive (x0, y0, z0, x1, y1, z1), (INT_MAX, INT_MAX, INT_MAX, -1, -1, -1) for an absent
     id; moments i64 [K, 9] = sum x, y, z, x^2, y^2, z^2, xy, xz, yz in voxel indices; surface i64 [K, 7] = boundary voxels (voxels of k with
     a 6-neighbour that is not k), fz, fy, fx (voxel faces of k normal to that axis facing "not k"), cz, cy, cx (those facing another object);
     the volume's outside is "not k" and is no object.  intensity: NULL with channels = 0, else u8 (sample_bytes 1) or u16 (2) interleaved
     [Z, H, W, channels], channels <= 4, any element-aligned address: isum / isum2 i64 [K, channels] = sum v, sum v^2; imin / imax i32
     [K, channels], (INT_MAX, -1) for an absent id.  lds_slots: the entries of the per-workgroup LDS table the runs are summed in before one
     global atomic per quantity and id (0 or a power of two <= 128; 0 = every run straight to the global tables; the results are the same).
   object_contacts3d: keys u64 [cap] / counts i64 [cap, 3]: the open-addressing pair table (key a << 32 | b, 0 < a < b; cap a power of two
     >= 2 * max_pairs), counts = (nz, ny, nx), the faces normal to each axis shared by a voxel of a and its neighbour voxel of b, every
     adjacent voxel pair counted once (looking forward along each axis); rows i64 [max_pairs, 4] = (key, nz, ny, nx) of the claimed slots in
     no particular order, flags[3] of them. */
int ullsam_measure_objects3d(const int* volume, int Z, int H, int W, int K, const void* intensity, int channels, int sample_bytes, int lds_slots,
                             long* voxels, int* box, long* moments, long* surface, long* isum, long* isum2, int* imin, int* imax, int* flags,
                             void* stream);
int ullsam_object_contacts3d(const int* volume, int Z, int H, int W, int K, unsigned long long* keys, long* counts, long cap, int max_pairs,
                             long* rows, int* flags, void* stream);

/* Surface meshes and Euler numbers of a label VOLUME (csrc/mesh3d.hip; integer work, bit-exact with the host forms
   utils.mesh3d.label_surfaces / object_topology, which drive these entries; definition in DESIGN.md "7b, continued (3-D surfaces)").  volume
   i32 [Z, H, W] with ids 0..K, 0 = background, 1 <= Z, H, W <= 32767 and Z * H * W <= 2^31 - 1.  Voxel p = (z H + y) W + x has a face towards
   d (0 = -z, 1 = +z, 2 = -y, 3 = +y, 4 = -x, 5 = +x) when its id k > 0 and the neighbour there is not k (the outside is not k); the face's id
   is 6 p + d < 2^34, lattice corner (cx, cy, cz) has the id (cz (H + 1) + cy) (W + 1) + cx < 2^34, a key is id | label << 34 with
   K <= 2^29 - 1 for the mesh entries.  flags i32 [4]: [0] = 1 when an id lies outside 0..K (it reads as background).
   mesh3d_masks: masks u8 [Z, H, W] = the six face bits of every voxel (bit d; 0 on the background and for an id with only[id] == 0; only u8
     [K + 1] or NULL = every id); a workgroup's tile is 64 x 4 x 4 voxels, tile_counts i32 [T] its faces, T = ceil(W / 64) ceil(H / 4)
     ceil(Z / 4); tile_offsets i64 [T + 1] = their exclusive sums, [T] = F.
   mesh3d_faces: fkeys u64 [F] = the face keys, a tile's at its offset (the caller sorts them).
   mesh3d_corners: ckeys u64 [4 F] = the keys of the four corners of every face of fkeys, counter-clockwise seen from outside (the caller
     sorts a copy).  mesh3d_heads: over n SORTED keys, 2048 a workgroup: block_counts i32 [B], B = ceil(n / 2048), = the keys that differ from
     their predecessor, block_offsets i64 [B + 1] their exclusive sums, [B] = V.  mesh3d_vertices: ukeys u64 [V] = those keys in order,
     vertices i32 [V, 3] = their (x, y, z).  mesh3d_quads: quads i32 [F, 4] = the index in ukeys of every corner key of fkeys (binary search).
   mesh3d_starts: start i64 [K + 1], start[k] = the number of the n sorted keys whose label is <= k.
   mesh3d_topology (K <= 2^31 - 2): euler i64 [K] = V - E + F - C of the cubical complex of id k's voxels (lattice corners, edges, faces
     touched, voxels: components - tunnels + cavities under 26-connectivity), pinch_edges i64 [K] = the lattice edges whose four voxels are
     k, not k, k, not k around the edge; both set here, 0 for an absent id. */
int ullsam_mesh3d_masks(const int* volume, int Z, int H, int W, int K, const unsigned char* only, unsigned char* masks, int* tile_counts,
                        long* tile_offsets, int* flags, void* stream);
int ullsam_mesh3d_faces(const int* volume, const unsigned char* masks, int Z, int H, int W, const long* tile_offsets, unsigned long long* fkeys, long F,
                        void* stream);
int ullsam_mesh3d_corners(const unsigned long long* fkeys, long F, int H, int W, unsigned long long* ckeys, void* stream);
int ullsam_mesh3d_heads(const unsigned long long* sorted, long n, int* block_counts, long* block_offsets, void* stream);
int ullsam_mesh3d_vertices(const unsigned long long* sorted, long n, const long* block_offsets, int H, int W, unsigned long long* ukeys, int* vertices,
                           long V, void* stream);
int ullsam_mesh3d_quads(const unsigned long long* fkeys, long F, const unsigned long long* ukeys, long V, int H, int W, int* quads, void* stream);
int ullsam_mesh3d_starts(const unsigned long long* sorted, long n, int K, long* start, void* stream);
int ullsam_mesh3d_topology(const int* volume, int Z, int H, int W, int K, long* euler, long* pinch_edges, int* flags, void* stream);

/* Skeletons of a label image: Guo and Hall's two-sub-iteration parallel thinning of every instance at once, and the links, degrees and node
   classes of the result (csrc/skeleton.hip; integer work, bit-exact with the host form utils.skeleton; definition in DESIGN.md "7b, continued
   (skeletons)").  An image i32 [H, W], 1 <= H, W <= 32767, holds a pixel's positive label while it stands and 0 on the background and once it is
   deleted; a neighbour is ON when it lies in the frame and holds the pixel's label; the code of a pixel has bit i for N, NE, E, SE, S, SW, W, NW
   (y down); sub-iteration `index` deletes the pixels whose code its table (by index & 1) holds, all judged on the state at its start.
   flags i32 [4], zeroed by the caller, only ever raised: [0] = a label below 0 (skel_measure: outside 0..K); it reads as background; [1] = a
   pixel was deleted in a sub-iteration whose index is >= limit.
   skel_step: dst = src after sub-iteration `index`; count[0] += the pixels deleted (one atomic per wave).  src and dst must differ.
   skel_tile: dst = src after the 8 sub-iterations index .. index + 7, run on tiles of 64 x 32 pixels staged in LDS with a halo of 8;
     counts[j] += the pixels sub-iteration index + j deleted, j = 0..7.  The outputs equal those of eight skel_step launches.
   skel_measure: two pixels of one label are linked when 4-adjacent, or diagonal with neither pixel 4-adjacent to both holding the label; the
     degree of a pixel = its links.  table i64 [7, K] (zeroed by the caller; NULL: none), row f column k - 1 += over id k's pixels: 1, degree
     == 1, degree >= 3, degree == 0, its links right and down, its links down-right and down-left, its degree.  d2 i32 [H, W] or NULL: d2_sum
     i64 [K] (zeroed) += d2, d2_min / d2_max i32 [K] (set to 2^31 - 1 / -1 by the caller) take the minimum / maximum.  nodes u8 [H, W] or NULL:
     0 off, 1 degree 1, 2 degree 2, 3 degree >= 3, 4 degree 0. */
int ullsam_skel_step(const int* src, int* dst, int H, int W, int index, int limit, int* count, int* flags, void* stream);
int ullsam_skel_tile(const int* src, int* dst, int H, int W, int index, int limit, int* counts, int* flags, void* stream);
int ullsam_skel_measure(const int* skeleton, const int* d2, int H, int W, long K, long* table, long* d2_sum, int* d2_min, int* d2_max,
                        unsigned char* nodes, int* flags, void* stream);

/* Point prompts, boxes and per-instance masks from one instance label image (csrc/prompts.hip; the reference's dataset loop
   train_joint_v2.py:313-468 as integer kernels, bit-exact with utils.prompts' host route; definitions in DESIGN.md "7b, continued (prompts)").
   labels i32 [H, W], 0 = background, ids 1..65535; H * W < 2^31; radius, hi <= 64; num_pos, num_neg <= 16.
   label_d1: d1 u8 [H, W] = min(radius + 1, city-block distance to the nearest pixel whose label differs, the outside of the frame counting as
     different); rowdist u8 [H, W] is scratch; status i32 [1] is set to 1 when a label lies outside 0..65535.
   prompt_choose: areas i32 [65536] (label_stats, N = 65535) -> sel i32 [max_instances] = the present ids in increasing order or, when there
     are more, max_instances of them by the draw rule; info[0] = how many.  present i32 [65535], sorted i32 [max_instances]: scratch.
   prompt_sets: for slot s < min(info[0], slots) with id sel[s], the interior {label = id, d1 > radius} and the ring {label != id,
     lo^2 <= D2 <= hi^2} as bit rows: bits u64 [2, slots, H, ceil(W / 64)] (only the words of the instance's window -- its box grown by hi --
     are written), rowcnt i32 [2, slots, H], sums u64 [slots, 2] = (sum x, sum y) over the instance.  boxes_t = label_stats' boxes of the
     label image read as a transposed map.  dbg_inner / dbg_ring u8 [slots, H, W] (both or neither): the two sets as images.
   prompt_points: coords f32 [slots, num_pos + num_neg, 2] (x, y), boxes f32 [slots, 4] XYXY inclusive, counts i32 [slots, 2] = (|inner|, |ring|),
     info[2 + 4 s ..] = (id, area, |inner|, |ring|); area 0 marks an absent id.  The negatives of a slot with |ring| < num_neg are left to the
     caller (the fallbacks).
   instance_masks: masks f32 [N, per] = (labels == ids[n]). */
int ullsam_label_d1(const int* labels, int H, int W, int radius, unsigned char* rowdist, unsigned char* d1, int* status,
                    void* stream);                                                            /* train_joint_v2.py:342 */
int ullsam_prompt_choose(const int* areas, int max_instances, unsigned long long seed, int* present, int* sorted, int* sel, int* info,
                         void* stream);                                                       /* train_joint_v2.py:319-327 */
int ullsam_prompt_sets(const int* labels, const unsigned char* d1, int H, int W, const int* areas, const int* boxes_t, const int* sel,
                       const int* info, int slots, int radius, int lo, int hi, unsigned long long* bits, int* rowcnt,
                       unsigned long long* sums, unsigned char* dbg_inner, unsigned char* dbg_ring, void* stream);   /* :342, 423-437 */
int ullsam_prompt_points(int H, int W, const int* areas, const int* boxes_t, const int* sel, int* info, int slots, int hi, int num_pos,
                         int num_neg, unsigned long long seed, const unsigned long long* bits, const int* rowcnt,
                         const unsigned long long* sums, float* coords, float* boxes, int* counts, void* stream);    /* :353-381, 439-442 */
int ullsam_instance_masks(const int* labels, const int* ids, long N, long per, float* masks, void* stream);          /* :332 */

/* Image preprocessing (csrc/imageprep.hip): Pillow's antialiased 8-bit resize as two integer passes, bit-exact with PIL.Image.resize
   (Resample.c, 8 bits per channel; definitions in DESIGN.md "7b, continued (image preprocessing)"), and the app's min-max normalisation to
   uint8.  The bounds (first tap, tap count) and 22-bit fixed-point coefficient tables are built on the host in float64 (ops.aa_tables).
   resize_u8_aa_h: src u8 addressed as y * s_row + x * s_col + c * s_chan (interleaved [IH, IW, C] or planar [C, IH, IW]), C in {1, 3, 4}, placed
     at (top, left) of a virtual [VH, VW] image that is zero elsewhere (the app's centred pad_to_square as a parameter); virtual rows
     row0 .. row0 + rows - 1 -- those the vertical pass reads -- are resampled to OW columns into tmp u8 [rows, OW, C].  bounds i32 [OW, 2],
     coef i32 [ksize, OW] (tap-major).
   resize_u8_aa_v: tmp -> OH rows; bounds i32 [OH, 2] (first row as a virtual row, row0 <= first, first + count <= row0 + rows), coef i32
     [OH, ksize].  Writes out_u8 [OH, OW, C] and / or out_f32: plane c = 0..2 at c * f_plane + y * f_row + x holds lut[c * 256 + v], lut f32
     [3, 256] (ToTensor + Normalize as 256 values per channel computed by the host with the reference's torch ops); only the OH x OW corner of
     each plane is written; C == 1 feeds all three planes (convert("RGB")), the fourth channel of C == 4 has no plane.
   minmax_*: mm u32 [2] = (min, max) as order-preserving keys (the value for u16; sign-flipped bits for f32), by integer atomics.
   normalize_to_u8_*: ((x - min) / (max - min + 1e-8) * 255).astype(uint8) as numpy evaluates it: u16 -- difference in uint16, quotient and
     product in float64; f32 -- all in float32; truncation.  NaN inputs are out of scope. */
int ullsam_resize_u8_aa_h(const unsigned char* src, long s_row, long s_col, long s_chan, int IH, int IW, int C, int top, int left, int VH,
                          int VW, int row0, int rows, const int* bounds, const int* coef, int ksize, int OW, unsigned char* tmp,
                          void* stream);                      /* utils/transforms.py:26-31, app.py:111-143, 232-248, train_joint_v2.py:271-275 */
int ullsam_resize_u8_aa_v(const unsigned char* tmp, int row0, int rows, int OW, int C, const int* bounds, const int* coef, int ksize, int OH,
                          unsigned char* out_u8, const float* lut, float* out_f32, long f_plane, long f_row,
                          void* stream);                      /* utils/transforms.py:26-31, app.py:242-249, train_joint_v2.py:299-300 */
int ullsam_minmax_u16(const unsigned short* x, long n, unsigned* mm, void* stream);                                  /* app.py:190-191 */
int ullsam_minmax_f32(const float* x, long n, unsigned* mm, void* stream);                                           /* app.py:226-228 */
int ullsam_normalize_to_u8_u16(const unsigned short* x, long n, const unsigned* mm, unsigned char* out, void* stream);   /* app.py:190-191 */
int ullsam_normalize_to_u8_f32(const float* x, long n, const unsigned* mm, unsigned char* out, void* stream);            /* app.py:226-228 */

/* The interactive loop's display tail (csrc/interactive.hip; definitions in DESIGN.md "7b, continued: the interactive loop"): one pass over
   the display image [H, W], which sits at (top, left) of the padded square of side `side` that the S x S model frame was resized from.
   Replaces, per click, the 1024^2 F.interpolate + threshold (app.py:635-645), postprocess_mask's Image.NEAREST (app.py:283-287; with the
   window, export_mask's resize-then-un-pad, app.py:807-820), save_instance's canvas write (app.py:692-707) and visualize_masks' blends
   (app.py:748-772).  low f32 [P, LH, LW] logits; per display pixel: frame pixel f = min(((2 (d + off) + 1) S) / (2 side), S - 1) per axis,
   v_p = the value ullsam_resize_bilinear gives at (fy, fx) of the [S, S] resize of low[p] (same bits), m_p = v_p > thr.
   flags & 1 (paint): canvas = first_id + p for the last p with m_p (canvas i32 [H, W], updated in place; otherwise only read, may be NULL).
   overlay u8 [H, W, 3] = image u8 [H, W, 3] through lut_inst[(id - 1) % K] (u8 [K, 3, 256]) where the canvas id > 0, then through lut_cur
   (u8 [3, 256]) where flags & 2 (highlight) and m_{P-1}.  mask u8 [P, H, W].  stats i32 [P, 5] = area, x0, y0, x1, y1 of m_p (inclusive
   maxima, zeros for an empty mask) with scratch i32 [5 P + 1].  mask, overlay and stats may each be NULL.  1 <= P <= 512. */
int ullsam_click_finish(const float* low, int P, int LH, int LW, int S, int H, int W, int side, int top, int left, float thr,
                        const unsigned char* image, int* canvas, int first_id, int flags, const unsigned char* lut_inst, int K,
                        const unsigned char* lut_cur, unsigned char* mask, unsigned char* overlay, int* stats, int* scratch,
                        void* stream);                        /* app.py:283-287, 635-645, 692-707, 748-772, 807-820 */

/* fp8 (OCP e4m3) ViT path -- BASELINE.json configs[4]; the reference's bf16 encoder linears image_encoder.py:227,171-181 with
   8-bit operands: rows quantised with a per-row scale (optionally behind the block's LayerNorm :166,180), GEMM on the
   block-scaled fp8 MFMA, scales applied in the epilogue */
int ullsam_rows_fp8(const void* in, int in_dtype, long in_stride, void* out_e4m3, long out_stride, float* row_scale, const float* ln_w,
                    const float* ln_b, long rows, int D, float eps, void* stream);
int ullsam_gemm_fp8(const void* A8, long lda, const float* a_scale, const void* W8, long ldw, const float* w_scale, void* C, long ldc,
                    int out_f32, const float* bias, const float* residual, long ldr, int act, int M, int N, int K, void* stream);

/* Weight-only fp8 (OCP e4m3) for the LLM's decode steps (InternLM2ForCausalLM.fp8_decode): the layers' wqkv / wo / packed w13 / w2 and the
   LM head `output` (modeling_internlm2.py:261-264, 341-426, 1081-1082) stored as e4m3 bytes [N, K] with one fp32 scale per output channel,
   streamed by the decode-step kernels in place of the bf16 rows; activations and accumulation as in the bf16 forms.
   ullsam_rows_fp8_pow2: per row, scale = the smallest power of two with amax / scale <= 448 (1 for a zero row), saturating round to nearest
   even.  q * scale of a bf16 weight is exact in bf16, so the kernels below compute what the bf16 kernels compute on those dequantised weights.
   ullsam_gemm_w8: C = act((a @ W8^T) * w_scale + bias) (+ residual) for M <= 8 rows, K % 512 == 0; a = bf16 `A` [M, K] (norm_w NULL) or
   bf16(RMSNorm(x) * norm_w) of fp32 x as ullsam_gemm_rmsnorm (M <= 4, K <= 4096, K % 2048 == 0); act 0..3 as ullsam_gemm.
   ullsam_decode_qkv_rope_w8: ullsam_decode_qkv_rope on e4m3 wqkv.  Shapes the decode-step kernels do not take are an error, not a fallback. */
int ullsam_rows_fp8_pow2(const void* in, int in_dtype, long in_stride, void* out_e4m3, long out_stride, float* row_scale, long rows, int D,
                         void* stream);
int ullsam_gemm_w8(const void* A, const float* x, long ldx, const float* norm_w, float eps, const void* W8, long ldw, const float* w_scale,
                   void* C, long ldc, int out_f32, const float* bias, const float* residual, long ldr, int act, int M, int N, int K,
                   void* stream);
int ullsam_decode_qkv_rope_w8(const void* a, const float* x, long ldx, const float* norm_w, float eps, const void* W8, long ldw,
                              const float* w_scale, const float* bias, int B, int K, int KVH, int G, const int* pos, const float* cos_tab,
                              const float* sin_tab, int tab_rows, void* q_out, void* k_cache, void* v_cache, int cap, int cache_pos0,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ULLSAM_HIP_H */
