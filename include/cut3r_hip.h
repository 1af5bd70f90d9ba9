/* cut3r_hip.h -- C ABI of libcut3r_hip.so: the MI355X (gfx950) kernels behind the CUT3R-SLAM hot path.
 *
 * Plain pointers + sizes only (device pointers unless stated), `stream` is a hipStream_t passed as void*.
 * Every entry point returns 0 on success, 1 on an argument/shape/alignment violation (nothing launched),
 * 2 if the launch itself failed.  Nothing here allocates, synchronises or touches the default stream, so every
 * call can be captured into a hipGraph.
 *
 * Each function cites the reference interface it replaces (paths relative to /root/reference).
 */
#ifndef CUT3R_HIP_H
#define CUT3R_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- version / probe ------------------------------------------------------------------------------------- */
int cut3r_abi_version(void);                         /* bumps when a signature changes */

/* ---- RoPE-2D -------------------------------------------------------------------------------------------------
 * replaces curope.rope_2d(tokens, positions, base, fwd)  (src/croco/models/curope/curope.cpp:49-67,
 * kernels.cu:17-108).  In place on a (B,N,H,D) view: element (b,n,h,d) at tokens + b*sB + n*sN + h*sH + d
 * (strides in elements, multiples of 4; the reference requires sH == D, stride(3) == 1; D % 16 == 0).  positions: int64 [B,N,2] contiguous,
 * may be negative.  dtype: 0 = fp32, 1 = fp16 (fp32 math, rounded on store -- the CUDA kernel's contract). */
int cut3r_rope2d(void* tokens, int dtype, const int64_t* positions, int B, int N, int H, int D,
                 long long sB, long long sN, long long sH, float base, float fwd, void* stream);
/* the two rope_2d calls of a self-attention (croco/models/blocks.py:127-128, dust3r/blocks.py:118-119: q then k, same
 * positions) in ONE launch: head stride == D for both; cos/sin are evaluated once per token. */
int cut3r_rope2d_qk(void* q, void* k, int dtype, const int64_t* positions, int B, int N, int H, int D, long long q_sB,
                    long long q_sN, long long k_sB, long long k_sN, float base, float fwd, void* stream);

/* the same rotation driven by the cos|sin table of cut3r_rope2d_table (identical bits: the table is filled by the expressions of
 * cut3r_rope2d), for fp16 tokens with head stride D: ONE launch rotates two token ranges -- q and k of a self-attention, or q of
 * one token stream and k of the other in a cross-attention (dust3r/blocks.py:118-119,226-227).  t_i: ntok_i tokens, token stride
 * stride_i elements (multiple of 8 when D % 32 == 0, else of 4), pos_i int64 [ntok_i,2]; t1 may be NULL.  Positions outside
 * [pmin, pmin+npos) are evaluated in place. */
int cut3r_rope2d_tab(void* t0, const int64_t* pos0, long long ntok0, long long stride0, void* t1, const int64_t* pos1, long long ntok1,
                     long long stride1, int H, int D, const float* table, int pmin, int npos, float base, float fwd, void* stream);

/* ---- LayerNorm (+adaLN modulation) -------------------------------------------------------------------------
 * replaces nn.LayerNorm(eps=1e-6) calls in croco/models/blocks.py:187-190, dust3r/blocks.py:292-297 and
 * ModLN (dust3r/blocks.py:356-379: y = LN(x)*(1+scale)+shift).  x fp32 [M,C] (row stride ldx).  Writes any of:
 * y16 (fp16, ld16) and y32 (fp32, ld32).  mod_scale/mod_shift: optional fp32 [C] (NULL = plain LN).
 * Every fp32 pointer 16-byte aligned, y16 8-byte aligned, every row stride a multiple of 4 (vector accesses). */
int cut3r_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float eps, int M, int C,
                    void* y16, int ld16, float* y32, int ld32, const float* mod_scale, const float* mod_shift,
                    void* stream);
/* one tensor, two affine parameter sets, two fp16 outputs (shared row statistics): norm1 of one decoder block and norm_y of
 * the other act on the same tokens (dust3r/blocks.py:292-297).  C in {768, 1024, 1536}. */
int cut3r_layernorm_dual(const float* x, int ldx, const float* g1, const float* b1, void* y1, int ld1, const float* g2,
                         const float* b2, void* y2, int ld2, float eps, int M, int C, void* stream);
/* the decoder's final norm of a view (dust3r/model.py:694-697) written where its consumers read it: x fp32 holds Wn groups of N + 1 rows
 * (pose token, N image tokens; row stride ldx).  Row 0 of group w goes to pose32 + w * pose32_gs (fp32) and pose16 + w * pose16_gs (fp16);
 * row 1 + n goes to tok16 + w * tok16_gs + n * C (fp16) and, if tok32 is not NULL, to tok32 + w * tok32_gs + n * C (fp32).  Group strides in
 * elements: >= the rows they separate, multiples of 4.  The row arithmetic is cut3r_layernorm's (the same kernels' row bodies), so the
 * bits are those of cut3r_layernorm followed by strided copies.  Alignment as for cut3r_layernorm; eps > 0; no modulation.  A bad
 * argument is refused with CUT3R_ERR_ARG before the launch. */
int cut3r_layernorm_tokens(const float* x, int ldx, const float* gamma, const float* beta, float eps, int Wn, int N, int C,
                           float* pose32, long long pose32_gs, void* pose16, long long pose16_gs, void* tok16, long long tok16_gs,
                           float* tok32, long long tok32_gs, void* stream);

/* ---- GEMM family ---------------------------------------------------------------------------------------------
 * replaces nn.Linear / nn.Conv2d / nn.ConvTranspose2d(+bias)(+GELU|ReLU)(+residual) in the ViT and DPT stacks
 * (croco/models/blocks.py:68-148, dust3r/blocks.py:87-243, croco/models/dpt_block.py:84-232,281-513).
 * C[M,N] = epi(A[M,K] * B[N,K]^T); A,B fp16, fp32 accumulate (v_mfma_f32_16x16x32_f16). */
typedef struct cut3r_gemm_desc {
    const void* A;        /* fp16 [M,K] row-major (lda) -- or NHWC [Bimg,H,W,Cin] when conv_k == 3 */
    const void* B;        /* fp16 [N,K] row-major (ldb) == nn.Linear.weight; conv: [Cout][ky][kx][Cin] */
    void* C;              /* fp16 or fp32 [M,N] (ldc) */
    const float* bias;    /* fp32 [N] or NULL */
    const void* res1;     /* optional residual [M,N] (ldr1), fp32 or fp16 */
    const void* res2;     /* optional second residual */
    int M, N, K, lda, ldb, ldc, ldr1, ldr2;
    int act;              /* 0 none, 1 exact GELU (erf), 2 ReLU */
    int out_f16, res1_f16, res2_f16;
    int batch;            /* >= 1: independent problems on blockIdx.z with the element strides below */
    long long strideA, strideB, strideC, strideBias, strideR1, strideR2;
    int conv_k;           /* 0/1 = plain GEMM (1x1 conv is a plain GEMM over pixels), 3 = implicit 3x3, pad 1 */
    int H, W, Cin, conv_stride, Ho, Wo;   /* conv_k == 3: input/output spatial sizes, M = Bimg*Ho*Wo, K = 9*Cin */
    int relu_in;          /* apply ReLU to A on load (ResidualConvUnit pre-activation) */
    int shuf;             /* > 0: ConvTranspose(k == stride == shuf) scatter; N = shuf*shuf*shuf_cout, ldc = Cout */
    int shuf_cout, shuf_Hin, shuf_Win;
    int tile;             /* 0 = auto (cut3r_gemm_tile_for), 16 (M <= 64 skinny), 64, 128, 192128 (192 x 128), 128192 (128 x 192) or 256 */
    int stages;           /* 0 = default; LDS ring depth override (tuning): 2|3 for tile 128, 2|3|4 for tile 64 */
    /* fused 2-D RoPE on the first rope_cols output columns (head dimension 64 only; fp16 output, no activation/residual):
     * what curope.rope_2d does to q / k right after the projection (croco/models/blocks.py:126-127, dust3r/blocks.py
     * :113-114,215-223), applied to the fp16-rounded projection exactly as the separate kernel would.  rope_pos int64 [M,2]
     * (y, x) per output row; rope_table from cut3r_rope2d_table (cos | sin for positions rope_pmin..rope_pmin+npos-1). */
    const void* rope_pos;
    const float* rope_table;
    int rope_cols, rope_pmin, rope_npos;
    int rope_d;           /* head dimension of the fused RoPE: 64 (default when 0) or 48 (forces the 128 x 192 tile) */
    /* LayerNorm folded into the GEMMs (round 4; replaces the nn.LayerNorm in front of qkv / projq / projk|projv / fc1:
     * croco/models/blocks.py:187-190, dust3r/blocks.py:292-297).  y = LN(x) W^T + b = rstd (x (gamma.W)^T - mu c) + d.
     * CONSUMER: A = fp16 copy of the UN-normalised rows x, B = fp16(gamma . W), bias = d = W beta + b, ln_colsum = c
     * (c_n = sum_k B_nk, fp32 [N]), ln_stats = fp32 [K/64][M][2] (slab-major): (sum, m2 = sum (x - sum/64)^2) of every 64-column
     * slab of every row, ln_nslab = K/64 <= 16 (K <= 1024; wider rows are a bad argument), ln_eps = the LayerNorm's eps.
     * The row's slabs are combined in slab order (parallel variance), the raw accumulator becomes acc*rstd - (rstd*mu)*c_n, then the usual epilogue runs (bias, GELU, RoPE, fp16).
     * PRODUCER: an fp32-output GEMM with an fp32 residual (the one that writes the residual stream) also stores out16 = fp16
     * copy of its output rows (ld16) and stats_out = their slab statistics, fp32 [N/64][M][2] (N % 64 == 0), computed in one
     * fixed order in every tile kernel.  Tiles 256 / 128 / 64 (producer), + 128 x 192 (consumer); not the skinny tile. */
    const float* ln_stats;
    const float* ln_colsum;
    int ln_nslab;
    float ln_eps;
    float* stats_out;
    void* out16;
    int ld16;
} cut3r_gemm_desc;
int cut3r_gemm_f16(const cut3r_gemm_desc* d, void* stream);
/* table[0][p][q] = cos((pmin+p) * fwd / base^(q/Q)), table[1][p][q] = sin(...), q < Q = head_dim/4, p < npos: the angles
 * of cut3r_rope2d, evaluated by the same device functions (fp32 [2][npos][Q]) */
int cut3r_rope2d_table(float* table, int pmin, int npos, int Q, float base, float fwd, void* stream);
/* the tile the launcher picks for this problem when desc->tile == 0: 256 (256x256x64 ping-pong kernel), 128 or 64.
 * tile 16 (M <= 64: skinny weight-streaming MFMA kernel) is never chosen automatically: its K-split changes the fp32
 * summation order, so callers request it for operands whose row count is the batch (one row per tracking window) and
 * keep every other GEMM on the tile kernels, whose rows are bit-identical across tile sizes and batch sizes. */
int cut3r_gemm_tile_for(const cut3r_gemm_desc* d);
/* TWO independent linear problems (same N, K; own operands, row counts and epilogues) in ONE launch: the state-side and the
 * image-side GEMM of a decoder layer -- both DecoderBlocks of a layer read the previous layer's pair
 * (src/dust3r/model.py:669-692), so they are independent; one grid over both fills the chip where each alone does not.
 * Linears only (no convolution / pixel shuffle / batch).  Rows are bit-identical to cut3r_gemm_f16.  Tile 256 / 128 on large combined
 * grids; below 128 tiles of 128 x 128 the 64 x 64 pair kernels (the one-window schedule: 2 x 156 tiles at M = 768 / 769), which also
 * carry the fused RoPE and both sides of the LayerNorm fold, each problem with its own flags. */
int cut3r_gemm_f16_pair(const cut3r_gemm_desc* d0, const cut3r_gemm_desc* d1, void* stream);
/* the kernel instance cut3r_gemm_f16 (cut3r_gemm_f16_pair) launches for this descriptor (pair), 0 if the call is refused.  Host only:
 * launches nothing and reads none of the operands (pointer VALUES count: null tests and alignment, as in the launch).  The launchers take
 * their kernel from the same selection, so the rule exists once.  The code is six decimal digits, the first the kernel family, the others
 * the instance's template arguments (csrc/gemm.hip), so two instances never share a code:
 *   1 T S W A E   gemm_kernel: T tile 1 = 64 x 64, 2 = 128 x 128, 3 = 128 x 192, 4 = 192 x 128, 5 = 256 x 128, 6 = 128 x 64; S depth of the
 *                 LDS ring; W waves 1 = 2 x 2, 2 = 2 x 4, 3 = 4 x 2; A addressing 0 generic, 1 plain operands with whole K-tiles, 2 3x3
 *                 convolution with a power-of-two Cin >= 64; E compile-time epilogue, 0 = decided at run time, 1 fp16 + bias, 2 + GELU,
 *                 3 fp32 + bias + fp32 residual, 4 fp16 + bias + ReLU, (7: cut3r_conv3x3_dpt_final only, never returned here)
 *   2 T S W A E   gemm_pair_kernel, the same digits
 *   3 C R F E L   gemm256_kernel (256 x 256): C 3x3 convolution, R ReLU on load, F fast addressing, E epilogue (as above; 5 fp16 + bias +
 *                 fp16 residuals, 6 fp16 + bias + RoPE of 64-wide heads), L LayerNorm-fold consumer
 *   400000        gemm256_pair_kernel
 *   5000 W M      gemm_skinny_kernel (tile 16): W = 4 | 8 waves splitting K, M = 1 | 2 | 4 row blocks of 16
 * e.g. 113213 = gemm_kernel<64, 64, 3, 2, 4, 1, 3>, 310140 = gemm256_kernel<true, false, true, 4>.  Whether the grid is 1-D (XCD-aware order)
 * and s_setprio (stages 12) are run-time arguments of an instance, not instances.
 * cut3r_gemm_kernel_count: how many distinct instances the two launchers can launch in this process -- every instance the selectors name,
 * those of the 64 x 64 ring depths that CUT3R_GEMM64_STAGES (read once per process) does not select left out.  (No reference counterpart.) */
int cut3r_gemm_kernel_for(const cut3r_gemm_desc* d);
int cut3r_gemm_pair_kernel_for(const cut3r_gemm_desc* d0, const cut3r_gemm_desc* d1);
int cut3r_gemm_kernel_count(void);

/* skinny M<=64 path: Y[M,N] = act(X[M,K] (fp32, optional SiLU on load) * W[N,K]^T (fp16) + bias) (+res).
 * act: 0 none or 1 exact GELU (anything else, ReLU's 2 included, is a bad argument); W 16-byte aligned, ldw % 8 == 0. */
int cut3r_gemv_f16w(const float* X, int ldx, const void* W, int ldw, const float* bias, float* Y, int ldy,
                    int M, int N, int K, int act, const float* res, int ldr, int silu_in, void* stream);

/* ---- fused attention ---------------------------------------------------------------------------------------------
 * replaces F.scaled_dot_product_attention(q,k,v, scale) (no mask, p=0) at croco/models/blocks.py:139-145 and
 * dust3r/blocks.py:123-129,233-239.  fp16 q/k/v, fp32 online softmax, fp16 out.
 * Element (b,n,h,d) of q lives at q + b*q_sb + n*q_sn + h*D + d (same for k,v with their strides; out likewise).
 * D in {16,32,48,64,128}.  scale must be finite and > 0 (anything else: bad argument, nothing is launched). */
int cut3r_attention_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D,
                        long long q_sb, long long q_sn, long long k_sb, long long k_sn, long long v_sb, long long v_sn,
                        long long o_sb, long long o_sn, float scale, void* stream);

/* cut3r_attention_f16 with Nk = 1, without the work: the softmax of one score is 1, so out[b, n, h, :] = v[b, 0, h, :] for all Nq query
 * rows -- the bits cut3r_attention_f16 writes (P = 1, l = 1, O = 1 v + 0).  The pose memory runs this: its write blocks attend to one
 * token per window, its read blocks have one token per window attending to itself (dust3r/model.py:204-222).  v and out as in
 * cut3r_attention_f16 (v_sn is checked, never used).  One difference: a non-finite score (non-finite q or k) gives NaN there and v here;
 * the network never forms the score on this path.  16-byte accesses: v, out 16-byte aligned, every stride a multiple of 8, D % 8 == 0,
 * D <= 256, o_sn >= H D and batches of out that do not overlap.  Anything else, a null pointer or B, H, Nq <= 0: CUT3R_ERR_ARG, nothing
 * is launched.  (No reference counterpart: the reference calls F.scaled_dot_product_attention here too.) */
int cut3r_attention_one_key_f16(const void* v, void* out, int B, int H, int Nq, int D, long long v_sb, long long v_sn, long long o_sb,
                                long long o_sn, void* stream);

/* which kernel serves the 48- and 64-wide heads: 1 (default) the software-pipelined LDS-DMA kernel, 0 the register-staged one.
 * Both give the same bits (tests/test_kernels_gpu.py); the switch exists for that test and for A/B timing.  v < 0 only queries.
 * Returns the previous setting.  (No reference counterpart: a tuning knob of this library.) */
int cut3r_attention_variant(int v);
/* the kernel instance cut3r_attention_f16 launches for this problem, as 100 * pipelined + waves per workgroup: 104 the pipelined
 * kernel (48- and 64-wide heads while cut3r_attention_variant is 1), 4 or 2 the register-staged kernel with 128 or 64 query rows per
 * workgroup (4 when B * H * ceil(Nq / 128) >= 384 or D = 128).  0: no instance (unsupported D, empty problem).  Host only, launches
 * nothing; the launcher itself asks this function, so the rule exists once.  (No reference counterpart.) */
int cut3r_attention_kernel_for(int B, int H, int Nq, int D);

/* ---- elementwise / layout helpers of the ViT path -------------------------------------------------------------- */
/* PatchEmbed conv 16x16/s16 as im2col (src/dust3r/patch_embed.py:18-32): img fp32 [B,C,H,W] -> fp16 [B*(H/P)*(W/P), C*P*P],
 * k ordered (c,py,px) == Conv2d weight.flatten(1).  If u8 != 0 the input is uint8 and (x/255-0.5)/0.5
 * (model.py:1111-1114 `normalize`) is fused into the load. */
int cut3r_im2col_patch(const void* img, int u8, int B, int C, int H, int W, int P, void* out, void* stream);
/* fp32 -> fp16 cast of a 2-D view (row strides in elements) */
int cut3r_cast_f32_f16(const float* x, int ldx, void* y, int ldy, int M, int C, void* stream);
/* column mean over rows: y[c] = mean_m x[m,c]  (model.py:732 `_get_img_level_feat`) ; x fp32 [M,C] */
int cut3r_colmean(const float* x, int ldx, int M, int C, float* y, void* stream);
/* B independent matrices (element strides stride_x / stride_y between them) in one launch; same summation order */
int cut3r_colmean_batched(const float* x, int B, long long stride_x, int ldx, int M, int C, float* y, long long stride_y, void* stream);

/* ---- DPT head helpers (NHWC fp16 activations) ------------------------------------------------------------------ */
/* bilinear x2 upsample, align_corners=True (dpt_block.py:215-221, :262-268): in [B,H,W,C] -> out [B,2H,2W,C] */
int cut3r_upsample2x_nhwc(const void* in, void* out, int B, int H, int W, int C, void* stream);
/* final 1x1 conv (Cin -> 4 or 3) + output activations (heads/postprocess.py:11-28,113-151):
 * mode 0: pts3d = xyz/|xyz| * expm1(|xyz|), conf = 1 + exp(c)   -> pts [P,3] fp32, conf [P] fp32
 * mode 1: rgb = (sigmoid(x)*(1-2e-6)+1e-6 - 0.5)*2              -> pts [P,3] fp32
 * in: fp16 [P,Cin]; w: fp32 [nout,Cin]; b: fp32 [nout] */
int cut3r_dpt_final(const void* in, int P, int Cin, const float* w, const float* b, int mode, float* pts, float* conf,
                    void* stream);
/* head.2 + head.4 + activations in one launch: the 3x3 convolution described by `d` exactly as for cut3r_gemm_f16 (conv_k = 3, stride 1,
 * Cin a power of two >= 64, N = 128 output channels, bias, act = 2 (ReLU), out_f16 = 1, no residual, batch 1; d->C is ignored: the fp16
 * output is never written), then on the fp16-rounded output the final 1x1 convolution w fp32 [4,128] (16-B aligned), b fp32 [4] and the
 * mode 0 activations of cut3r_dpt_final, in the convolution's epilogue.  Pixel q of view v (v = row / (Ho*Wo)) goes to
 * pts + v * pts_view_stride + 3 q and conf + v * conf_view_stride + q (element strides), so a view can be written straight into a slice
 * of a larger tensor.  Same bits as cut3r_gemm_f16 followed by cut3r_dpt_final.  Any other problem, mode 1 or a destination that is not
 * 4-byte aligned is refused with CUT3R_ERR_ARG before the launch. */
int cut3r_conv3x3_dpt_final(const cut3r_gemm_desc* d, const float* w, const float* b, int mode, float* pts, long long pts_view_stride,
                            float* conf, long long conf_view_stride, void* stream);
/* postprocess on raw fp32 [P,4|3] maps (linear head path, pos_z option: linear_head.py:316) */
int cut3r_postprocess_pts(const float* raw, int P, int nch, int pos_z, float* pts, float* conf, void* stream);
/* camera pose activation (heads/postprocess.py:30-63): in fp32 [B,7] -> out [B,7] (t*expm1|t|/|t|, unit quat w>=0) */
int cut3r_postprocess_pose(const float* raw, int B, float* out, void* stream);

/* ---- keyframe selection ---------------------------------------------------------------------------------------------
 * replaces compute_patch_overlap_ratio (hislam2/util/utils.py:726-736): rows 1.. of feat0/feat1 fp32 [N,C] are
 * L2-normalised, sim = f0 f1^T (exact fp32 MFMA), count = #rows with max_j sim > thr.  count: int32[1] (device),
 * zeroed by the call.  ws: 16-B aligned fp32 workspace of 2*(N-1)*C + (N-1) elements.  After the call it holds, in this
 * order: n0 fp32 [N-1][C], the normalised rows 1.. of feat0 (x / max(||x||, 1e-12)); n1 fp32 [N-1][C], the same of feat1;
 * rmax [N-1], the bit patterns of the fp32 row maxima max(0, max_j n0[r] . n1[j]).  The clamp at 0 and the unsigned maximum
 * on those bits are valid for thr >= 0 only: a negative or NaN thr is refused.  (cut3r_patch_overlap_chain keeps B+1
 * normalised sets [B+1][N-1][C] -- feat_last, then the candidates -- followed by the same [N-1] maxima, left cleared.) */
int cut3r_patch_overlap(const float* feat0, const float* feat1, int N, int C, float thr, void* ws, int32_t* count,
                        void* stream);
/* The keyframe decisions of a whole look-ahead batch with no host round trip per candidate: replaces the decision loop of
 * MotionFilter.kfFilter (hislam2/motion_filter.py:98-124) over B consecutive tested frames whose encoder features
 * feats fp32 [B,N,C] are already resident.  Candidate i is compared with the LAST KEYFRAME SO FAR -- feat_last [N,C] until
 * a candidate is taken, then that candidate (kept in *state on the device: -1 | index) -- with the arithmetic of
 * cut3r_patch_overlap (bit-identical counts), and is taken when (double)(float(count)/float(N-1)) < thr_ratio, or
 * unconditionally when forced_host[i] != 0 (first / second-last / last frame, :87-96; forced_host may be NULL).
 * counts, decisions: int32 [B] (device); state: int32 [1] (device).
 * ws: 16-B aligned fp32 workspace of (B+1)*(N-1)*C + (N-1) elements. */
int cut3r_patch_overlap_chain(const float* feat_last, const float* feats, int B, int N, int C, float thr_sim, double thr_ratio,
                              const int32_t* forced_host, void* ws, int32_t* state, int32_t* counts, int32_t* decisions,
                              void* stream);

/* ---- covisibility graph geometry ------------------------------------------------------------------------------------
 * replaces FactorGraph.cal_overlap_batch / cal_overlap_bi (hislam2/factor_graph.py:255-315).
 * w2c: fp32 [B,12] = top 3x4 of inverse(c2w) row-major; K4 = (fx,fy,cx,cy) HOST floats; counts int32[B] (device).
 * fwd: ONE pointmap pm [N,3] projected into B cameras (z clamped at 1e-5 for the divide, :272).  If P_host != NULL the
 *      points are first mapped p <- P*(s_align*p) (12 HOST floats, 3x4 row-major): the tracker's chained full-resolution
 *      pointmap (track_frontend.py:234,259) is then never materialised.
 * bwd: B pointmaps projected into ONE camera (raw z divide, :304).  Pointmap b starts at
 *      pms + slot(b)*N*3 with slot(b) = b when grp == 0, else (b/grp)*grp_stride + b%grp -- the keyframe order of the
 *      [submap][6 slots] store (hislam2/keyframe.py:28, track_frontend.py:251-255) without gathering a copy. */
int cut3r_overlap_fwd(const float* pm, int N, const float* P_host, float s_align, const float* w2c, int B, float fx, float fy,
                      float cx, float cy, int W, int H, int clamp_z /* 1: cal_overlap_batch, 0: cal_overlap_bi with B1 == 1 */,
                      int32_t* counts, void* stream);
int cut3r_overlap_bwd(const float* pms, int B, int N, int grp, int grp_stride, const float* w2c, float fx, float fy, float cx,
                      float cy, int W, int H, int32_t* counts, void* stream);

/* ---- whole-window update -------------------------------------------------------------------------------------------
 * One call for everything TrackFrontend.track does per pixel for a window of V <= 6 consecutive keyframes t0..t0+V-1
 * (hislam2/track_frontend.py:193-262 + factor_graph.py:148-197, :255-315): the V cut3r_align_view results (pm_ds, conf_ds,
 * depth are the V consecutive slots / rows of the resident stores) and, for every keyframe i = t0+v >= first, the forward
 * counts of its full-resolution chained pointmap in cameras 0..i-1 and the backward counts of stored pointmaps 0..i-1
 * (slot addressing as cut3r_overlap_bwd, over `store`) in camera i.  pts [V,H,W,3], conf [V,H,W] contiguous; P_host
 * V*12 HOST floats; w2c device [>= t0+V, 12]; counts int32 device [V][2][ldc] (row 0 forward, row 1 backward; ldc >=
 * t0+V), zeroed here.  w2c_new_host (optional, V*12 HOST floats): rows t0..t0+V-1 of w2c are written from it first (the
 * keyframe store's device mirror, hislam2/keyframe.py:24 pose) -- no separate upload.  lsum_reset (optional): a
 * cut3r_logdepth_accum accumulator zeroed for the next window.  Three launches instead of ~6 per keyframe; every count
 * equals the per-keyframe entry points'.  t0+V-1 <= 65535 (a grid dimension); like every other argument error this one is
 * returned before anything is launched. */
int cut3r_window_update(const float* pts, const float* conf, int V, int H, int W, const float* P_host, float s, int ds,
                        float* pm_ds, float* conf_ds, float* depth, const float* store, int grp, int grp_stride,
                        float* w2c, const float* w2c_new_host, int t0, int first, float fx, float fy, float cx, float cy,
                        int32_t* counts, int ldc, double* lsum_reset, void* stream);

/* ---- window alignment -----------------------------------------------------------------------------------------------
 * replaces the per-view tensor math of TrackFrontend.track (hislam2/track_frontend.py:193-243): pointmap = P*(s*pts),
 * conf <- 1-1/conf, depth = s*z, stride-`ds` downsample.  P_host: 12 HOST floats (chained c2w 3x4, row-major), s by value
 * (both are products of tiny 4x4 host math on the 7-float camera poses, exactly as in the reference). */
/* cut3r_logdepth_sum without the zeroing memset: *out += sum(log prev - log z) (the caller keeps *out zeroed, e.g. through
 * cut3r_window_update's lsum_reset) */
int cut3r_logdepth_accum(const float* prev_depth, const float* pts, int n, double* out, void* stream);

int cut3r_align_view(const float* pts, const float* conf, int H, int W, const float* P_host, float s, int ds,
                     float* pm_ds, float* conf_ds, float* depth, void* stream);
/* sum_i log(prev_depth[i]) - log(pts[i].z) -> out[0] (fp64 accumulate, device double[1], zeroed by the call) */
int cut3r_logdepth_sum(const float* prev_depth, const float* pts, int n, double* out, void* stream);

/* ---- Lie groups (slot of the un-vendored princeton-vl/lietorch 0.2, "lietorch_backends") -------------------------------
 * call sites: hislam2/track_backend.py:269-270,298-299,418-425,458-459 (SE3.exp / .matrix / .data),
 * hislam2/gs_backend_per_frame.py:721-731, hislam2/geom/projective_ops.py:17,51,67,69, hislam2/geom/ba.py:29,37.
 * group: 0 = SO3 (tangent 3, data 4 = q_xyzw), 1 = SE3 (6 = [tau,phi], 7 = [t,q_xyzw]), 2 = Sim3 (7, 8 = [t,q,s]).
 * All tensors fp32, contiguous, n elements.  op: 0 exp (tangent->data), 1 log (data->tangent), 2 inv (data->data),
 * 3 matrix (data -> 16 floats, row-major 4x4).  *_bwd are vector-Jacobian products w.r.t. the Euclidean components. */
int cut3r_lie_unary(int group, int op, const float* in, float* out, int n, void* stream);
int cut3r_lie_unary_bwd(int group, int op, const float* in, const float* grad_out, float* grad_in, int n, void* stream);
int cut3r_lie_mul(int group, const float* x, const float* y, float* out, int n, void* stream);
int cut3r_lie_mul_bwd(int group, const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int n,
                      void* stream);
/* element e acts on its P points p[e,:,pd] (pd = 3, or 4 = homogeneous [X,Y,Z,W] -> [R*XYZ*s + t*W, W]) */
int cut3r_lie_act(int group, const float* x, const float* p, float* out, int n, int P, int pd, void* stream);
int cut3r_lie_act_bwd(int group, const float* x, const float* p, const float* grad_out, float* grad_x, float* grad_p, int n, int P,
                      int pd, void* stream);
/* adjoint (transpose = 0) or transposed adjoint (1) of element e applied to tangent vector a[e] */
int cut3r_lie_adj(int group, const float* x, const float* a, float* out, int n, int transpose, void* stream);

/* ---- loop closure: fused submap-alignment optimiser -----------------------------------------------------------------
 * replaces the Adam loop over SE3.exp(xi).matrix() of TrackBackend.loop_closure_init
 * (hislam2/track_backend.py:256-299; lr 5e-4, `iteration` steps) and the pointmap rewrite (:301-310).
 * first/last: device pointers to slot 0 / slot 5 of the [B][6][N][3] submap store (sub_stride = floats between
 * consecutive submaps); mask: uint8 [B-1,N] (conf of `last` > 0) or NULL; cur/cur_lc: [N,3] current pointmap in the
 * global frame / in the matched submap's frame.  xi,adam_m,adam_v: [B,6], T: [B,12] row-major 3x4: the caller's state,
 * read and updated in place.  A fresh optimisation passes xi = adam_m = adam_v = 0 and T = identity; a resumed state is
 * accepted as long as T = matrix(exp(xi)) row by row (T is what the residuals are evaluated with, xi what the step is
 * taken from).  Row 0 is the fixed identity: T row 0 is read (pass the identity), row 0 of xi, adam_m, adam_v and T is
 * never written.  The step count of Adam's bias correction restarts at 1 in every call, whatever the state.
 * workspace: cut3r_lc_workspace_floats(B,N) floats, written before it is read (rows of 28 floats per pair and block of
 * 2048 points, 25 used: after the call it holds the last iteration's partial sums); loss_out: NULL or float[iters].
 * Two launches per iteration, deterministic (no float atomics). */
int cut3r_lc_workspace_floats(int B, int N);
int cut3r_lc_optimize(const float* first, const float* last, long long sub_stride, const unsigned char* mask, const float* cur,
                      const float* cur_lc, int B, int N, long long n_masked, int iters, float lr, float* xi, float* adam_m,
                      float* adam_v, float* T, float* workspace, float* loss_out, void* stream);
/* General form for the second and later loop closures (TrackBackend.loop_closure, hislam2/track_backend.py:400-461: the
 * chain term + the matched-submap term + the current-vs-lc term, Adam over `_align_lie` AND `matched_lie`).  The objective
 * is a LIST of L1 terms  w * sum_n | T[ia] a_n - T[ic] c_n |_1  over [N,3] point arrays; T[0] is the fixed identity, every
 * other row of T [P,12] is exp of a row of xi [P,6] and is optimised.  terms_dev: DEVICE array of n_terms cut3r_lc_term.
 * workspace: cut3r_lc_workspace_floats(n_terms, N) floats.  xi/adam_m/adam_v/T [P,..]: the caller's state, under the
 * same rules as cut3r_lc_optimize (zero / identity for a fresh run, else T = matrix(exp(xi)); row 0 read, never
 * written; bias correction restarts at step 1).  Two launches per iteration, deterministic. */
typedef struct cut3r_lc_term {
    const float* a;              /* [N,3] points moved by T[ia] */
    const float* c;              /* [N,3] points moved by T[ic] */
    const unsigned char* mask;   /* NULL or uint8 [N]: points with mask 0 are skipped */
    int ia, ic;                  /* transform indices, 0 = fixed identity */
    float w;                     /* weight of the term (1 / (3 * #points of its mean)) */
    int pad;
} cut3r_lc_term;
int cut3r_lc_optimize_terms(const void* terms_dev, int n_terms, int P, int N, int iters, float lr, float* xi, float* adam_m,
                            float* adam_v, float* T, float* workspace, float* loss_out, void* stream);
/* The same two optimisers over sim(3): one 7-vector [tau(3), phi(3), sigma] per transform, T = [e^sigma R | W tau] (Sophus /
 * lietorch Sim3.exp), so that a loop whose two ends disagree in SCALE can be closed.  No counterpart in the reference (its
 * loop closure is rigid); the objective, the accumulate launch, the workspace (cut3r_lc_workspace_floats) and every rule
 * above are those of the se(3) entry points -- only xi/adam_m/adam_v are [B,7] / [P,7]. */
int cut3r_lc_optimize_sim3(const float* first, const float* last, long long sub_stride, const unsigned char* mask, const float* cur,
                           const float* cur_lc, int B, int N, long long n_masked, int iters, float lr, float* xi, float* adam_m,
                           float* adam_v, float* T, float* workspace, float* loss_out, void* stream);
int cut3r_lc_optimize_terms_sim3(const void* terms_dev, int n_terms, int P, int N, int iters, float lr, float* xi, float* adam_m,
                                 float* adam_v, float* T, float* workspace, float* loss_out, void* stream);
/* in place p <- T_b p for the points_per_submap points of each of the B submaps (pts: [B, points_per_submap, 3]); T_b is any
 * 3x4 (rigid or a similarity) */
int cut3r_transform_submaps(float* pts, const float* T, int B, long long points_per_submap, void* stream);
/* in place planes[i] <- scale[i] * planes[i] for the n planes of per_plane floats each (planes: [n, per_plane], n <= 65535): the
 * depth maps of the keyframes a sim(3) correction rescales.  One fp32 multiply per element, one launch. */
int cut3r_scale_planes(float* planes, const float* scale, int n, long long per_plane, void* stream);

/* ---- legacy dense-BA operators (`droid_backends` sources are absent from the reference) --------------
 * corr_index: replaces droid_backends.corr_index_forward/backward (call sites hislam2/modules/corr.py:12,19).
 * volume [BN,h1,w1,h2,w2], coords [BN,2,h1,w1] (x,y), out [BN,2r+1,2r+1,h1,w1]: bilinear lookup with zero padding,
 * out[n,i,j,y,x] = volume[n,y,x] sampled at (x0 - r + i, y0 - r + j). */
int cut3r_corr_index_forward(const float* volume, const float* coords, float* out, int BN, int h1, int w1, int h2, int w2,
                             int radius, void* stream);
int cut3r_corr_index_backward(const float* coords, const float* grad_out, float* grad_volume, int BN, int h1, int w1, int h2, int w2,
                              int radius, void* stream);
/* one Gauss-Newton step of geom.ba.BA (hislam2/geom/ba.py:32-107, geom/chol.py:47-78, geom/projective_ops.py:44-74):
 * Gij [N,7] = G_j*G_i^-1 (SE3 data), disps [P,ht*wd], intr [P,4], target/weight [N,ht*wd,2], eta [M,ht*wd];
 * ii,jj int32 [N]; CSR of edges by source frame (src_ptr [M+1], src_edges [N], kx [M] = sorted unique(ii));
 * present uint8 [P-fixedp, M] marks the non-zero E blocks.  Outputs dx [P-fixedp,6], dz [M,ht*wd], flag[0] = 1 if
 * the Cholesky failed (dx = 0, as geom/chol.py:13-18).  Requires 6*(P-fixedp) <= 192 (otherwise: CUT3R_ERR_ARG, nothing written).
 * workspace: cut3r_ba_workspace_floats(P, ht, wd, N, M, fixedp) floats, for cut3r_ba_step and for the staged entry points alike;
 * no entry point reads or writes outside them. */
long long cut3r_ba_workspace_floats(int P, int ht, int wd, int N, int M, int fixedp);
int cut3r_ba_step(const float* Gij, const float* disps, const float* intr, const float* target, const float* weight, const float* eta,
                  const int* ii, const int* jj, const int* src_ptr, const int* src_edges, const int* kx, const unsigned char* present,
                  int P, int ht, int wd, int N, int M, int fixedp, float ep, float lm, float* workspace, float* dx, float* dz, int* flag,
                  void* stream);
/* The same step in three stages, so that EDGES CAN BE SHARDED by source frame over several GPUs (north_star: all-reduce of the
 * normal-equation blocks): every rank assembles the UNDAMPED reduced system S = H - E C^-1 E^T, vS = v - E C^-1 w of ITS edges
 * (each source frame m -- with its depth blocks C_m, w_m, E_.m -- lives on exactly one rank) plus diag(H); S, vS and the
 * diagonal (6(P-fixedp))^2 + 2*6(P-fixedp) floats are summed over ranks; every rank then damps (S + (ep + lm*diag H) I,
 * geom/chol.py:56-57), solves, and back-substitutes dz for its own source frames.  motion_only != 0 drops the Schur
 * correction: the reduced system of MoBA (geom/ba.py:110-158).  S_out [n,n], vS_out [n], hdiag_out [n], n = 6(P-fixedp);
 * scratch: n*n floats. */
int cut3r_ba_assemble(const float* Gij, const float* disps, const float* intr, const float* target, const float* weight, const float* eta,
                      const int* ii, const int* jj, const int* src_ptr, const int* src_edges, const int* kx, const unsigned char* present,
                      int P, int ht, int wd, int N, int M, int fixedp, int motion_only, float* workspace, float* S_out, float* vS_out,
                      float* hdiag_out, void* stream);
int cut3r_ba_solve(const float* S, const float* vS, const float* hdiag, int n, float ep, float lm, float* scratch, float* dx, int* flag,
                   void* stream);
int cut3r_ba_backsub(float* workspace, const float* dx, const unsigned char* present, int P, int ht, int wd, int N, int M, int fixedp,
                     float* dz, void* stream);
/* droid_backends.proj_trans (call site hislam2/geom/ba.py:200): per-source depth normal equations with the poses held fixed,
 * C [M,ht*wd] = sum_e w Jz^2, w [M,ht*wd] = sum_e w r Jz.  workspace: N * ceil(ht*wd/256) * 120 floats. */
int cut3r_ba_proj_trans(const float* Gij, const float* disps, const float* intr, const float* target, const float* weight, const int* ii,
                        const int* jj, const int* src_ptr, const int* src_edges, const int* kx, int P, int ht, int wd, int N, int M,
                        float* workspace, float* C_out, float* w_out, void* stream);
/* geom.chol.schur_solve_mono_prior (/root/reference/hislam2/geom/chol.py:80-107; call site geom/ba.py:235): the scale-grid block of
 * JDSA reduced over the per-pixel disparities.  H [n,n], E [n,cols], v [n] with n = M*D scale nodes (<= 192) and cols = M*ht*wd
 * disparities, in the layout the reference builds with permute + reshape; C, w [cols].  S = H + (ep + lm diag H) I - E C^-1 E^T,
 * in-LDS Cholesky, dso = S^-1 (v - E C^-1 w), dz = C^-1 (w - E^T dso), dzcov = |L^-1 E C^-1|^2 column-wise + C^-1 (NULL: skipped).
 * A failed factorisation gives dso = 0 (CholeskySolver, chol.py:13-18) and sets flag[0].  workspace:
 * cut3r_schur_mono_prior_workspace_floats(n, cols) floats. */
long long cut3r_schur_mono_prior_workspace_floats(int n, long long cols);
int cut3r_schur_mono_prior(const float* C, const float* w, const float* H, const float* E, const float* v, int n, long long cols, float ep,
                           float lm, float* workspace, float* dso, float* dz, float* dzcov, int* flag, void* stream);
/* the normal-equation blocks of geom.ba.JDSA's scale grids (/root/reference/hislam2/geom/ba.py:213-228): per source frame m,
 * Jso = -[prior > 0] prior Jbi[m] ([HW,D], Jbi from cut3r_bi_inter), H_m = alpha Jso^T Jso, E_m = alpha Jso^T, v_m = -alpha Jso^T rd,
 * written as the block-diagonal dense H [M*D, M*D], E [M*D, M*HW], v [M*D] that cut3r_schur_mono_prior takes. */
int cut3r_jdsa_blocks(const float* prior, const float* Jbi, const float* rd, float alpha, int M, int HW, int D, float* H, float* E, float* v,
                      void* stream);
/* droid_backends.bi_inter (call site hislam2/geom/ba.py:167): bilinear interpolation of per-frame scale grids scales [M,hs,ws] at
 * grid [M,ht,wd,2] (x, y) -> vals [M,ht,wd] and the dense Jacobian J [M,ht,wd,hs*ws] w.r.t. the grid nodes. */
int cut3r_bi_inter(const float* scales, const float* grid, int M, int hs, int ws, int ht, int wd, float* vals, float* J, void* stream);
/* droid_backends.depth_filter (call site hislam2/util/droid_visualization.py:100; the extension is absent from the reference tree,
 * semantics from the published DROID-SLAM kernel): poses [n,7] world->camera SE3 data (t, q_xyzw), disps [n,ht,wd] inverse depths,
 * intr [4] (fx, fy, cx, cy), inds [M] int64 frame indices (each must lie in [0, n): checked by the Python mirror), thresh [M] ->
 * count [M,ht,wd]: in how many of the six neighbour frames {ix-1, ix-2, ix-3, ix+3, ix+4, ix+5} the pixel's depth is confirmed. */
int cut3r_depth_filter(const float* poses, const float* disps, const float* intr, const long long* inds, const float* thresh, int n, int M,
                       int ht, int wd, float* count, void* stream);
/* droid_backends.altcorr_forward / altcorr_backward (call sites hislam2/modules/corr.py:79,87): on-the-fly correlation of fmap1
 * [BN,H,W,C] with fmap2 [BN,H2,W2,C] sampled bilinearly in a (2r+1)^2 window around coords [BN,S,H,W,2] ->
 * corr [BN,S,(2r+1)^2,H,W]; backward gives the gradients w.r.t. both feature maps (coords get none). */
int cut3r_altcorr_forward(const float* fmap1, const float* fmap2, const float* coords, int BN, int S, int H, int W, int H2, int W2, int C,
                          int radius, float* corr, void* stream);
int cut3r_altcorr_backward(const float* fmap1, const float* fmap2, const float* coords, const float* grad_corr, int BN, int S, int H, int W,
                           int H2, int W2, int C, int radius, float* grad1, float* grad2, void* stream);

/* ---- stream preprocessing -------------------------------------------------------------------------------------------
 * replaces cv2.resize(image, (w1, h1)) of demo_s.py:72,83 (default INTER_LINEAR, 8-bit): OpenCV's fixed-point bilinear
 * and its exact-2x box special case, restated from the published algorithm (OpenCV is not in the reference tree and cv2 is
 * not in the build image: parity unpinned, see oracle/oracle_geom.c).  src u8 [H0,W0,C] interleaved (device); dst u8
 * [C,H1,W1] when chw_out != 0 (the layout demo_s.py:73 permutes to) else [H1,W1,C]. */
int cut3r_resize_linear_u8(const void* src, int H0, int W0, int C, void* dst, int H1, int W1, int chw_out, void* stream);
/* cv2.undistort's resampling step (demo_s.py:63-64 `cv2.undistort(image, K, calib[4:])` = initUndistortRectifyMap + remap with
 * INTER_LINEAR, BORDER_CONSTANT 0): src/dst uint8 HWC; map_ix/map_iy int32 [Ho,Wo] = source coordinates in 1/32 pixel
 * (round(32 u)), built once per sequence on the host (cut3r_slam_amd/stream.py:undistort_map).  PARITY UNPINNED vs cv2
 * (absent from the build image): follows the published fixed-point algorithm (5 fraction bits, 15-bit weights). */
int cut3r_remap_linear_u8(const void* src, int H, int W, int C, const int32_t* map_ix, const int32_t* map_iy, void* dst, int Ho, int Wo,
                          void* stream);

/* ---- Gaussian-splatting rasteriser ---------------------------------------------------------------
 * replaces diff_gaussian_rasterization._C.rasterize_gaussians (thirdparty/diff-gaussian-rasterization/rasterize_points.cu:55-195,
 * bound at ext.cpp:16; called from diff_gaussian_rasterization/__init__.py:75-84, hislam2/gaussian/renderer/__init__.py:132-140),
 * split into its three stages so that the caller owns every buffer.  All pointers are device pointers except the *_host ones
 * (16 / 16 / 3 / 3 floats read on the host when the call is made).  Matrices as the reference passes them: the TRANSPOSED 4x4s
 * (p_view = [p,1] @ viewmatrix).  geom: P records of 32 floats (xy, view depth, ray distance, conic + opacity, rgb, view point,
 * camera plane, ray plane, normal, radius, tile rectangle): the render stages gather from it.
 *   preprocess: forward.cu:308-421 per Gaussian + inclusive scan of the covered-tile counts -> offsets[P] (offsets[P-1] = number of
 *               instances, read back by the caller to size the binning buffers, as rasterizer_impl.cu:346-354 does).
 *   bin:        rasterizer_impl.cu:70-112,151-176: instance keys (tile << 32 | depth bits), radix sort, per-tile [start, end).
 *               overflow == NULL: n_instances is offsets[P-1] read back by the caller.  overflow != NULL (capacity mode, for callers
 *               that must not stop the host, e.g. inside a captured graph): n_instances is a capacity, unused entries are padded
 *               behind the last tile, *overflow is set to 1 on the device if the scene needed more.
 *   render:     forward.cu:429-692.  color/coord/mcoord/normal [3,H,W]; depth/mdepth/alpha [1,H,W]; n_contrib uint32 [2,H,W];
 *               aux float [2,H,W] (final transmittance, normal length: kept for the backward pass).
 *   A refused call (CUT3R_ERR_ARG: a missing pointer or workspace, P <= 0, sh_degree outside 0..3, sh_coeffs < (sh_degree + 1)^2,
 *   non-positive W, H or tanfov) writes nothing: every argument is checked before the first write. */
int cut3r_gs_preprocess(int P, const float* means, const float* scales, const float* rots, const float* opacities, const float* shs,
                        int sh_degree, int sh_coeffs, const float* colors_precomp, const float* viewmatrix_host, const float* projmatrix_host,
                        const float* campos_host, int W, int H, float tanfovx, float tanfovy, float kernel_size, float scale_modifier, float* geom,
                        int* radii, unsigned* tiles_touched, unsigned* offsets, void* scan_ws, long long scan_ws_bytes, void* stream);
long long cut3r_gs_workspace_bytes(int P, long long n_instances);
int cut3r_gs_bin(int P, const float* geom, const unsigned* offsets, long long n_instances, int W, int H, unsigned long long* keys_tmp,
                 unsigned* vals_tmp, unsigned long long* keys_sorted, unsigned* point_list, unsigned* ranges, void* sort_ws,
                 long long sort_ws_bytes, int* overflow, void* stream);
int cut3r_gs_render_forward(const unsigned* ranges, const unsigned* point_list, const float* geom, int W, int H, float tanfovx, float tanfovy,
                            const float* bg_host, float* out_color, float* out_coord, float* out_mcoord, float* out_depth, float* out_mdepth,
                            float* out_alpha, float* out_normal, unsigned* n_contrib, float* aux, void* stream);
/* backward of the rasteriser (replaces _C.rasterize_gaussians_backward, rasterize_points.cu:197-330 -> backward.cu:145-1160).
 *   render_backward:     per-pixel gradients of the seven images -> dgeom [P,32]: gradients of the record fields (record layout; it is
 *                        zeroed here; slot 2 carries the |d/dxy| sum of backward.cu:1005).  Needs the forward's geom, point_list,
 *                        ranges, n_contrib, aux and its alpha / coord / depth / normal images.
 *   preprocess_backward: dgeom -> d_means [P,3], d_scales [P,3], d_rots [P,4], d_opacities [P], d_shs [P,sh_coeffs,3] (rows beyond the
 *                        active degree are left untouched: pass zeros) or d_colors [P,3] when shs == NULL, d_means2D [P,3] (x, y in
 *                        NDC units as backward.cu:1002-1003, z the |.| sum).  Gaussians culled by the forward pass are not written:
 *                        pass zero-initialised outputs.  Exact derivatives of the forward function (forward-mode duals). */
int cut3r_gs_render_backward(const unsigned* ranges, const unsigned* point_list, const float* geom, int P, int W, int H, float tanfovx,
                             float tanfovy, const float* bg_host, const unsigned* n_contrib, const float* aux, const float* out_alpha,
                             const float* out_coord, const float* out_depth, const float* out_normal, const float* g_color, const float* g_coord,
                             const float* g_mcoord, const float* g_depth, const float* g_mdepth, const float* g_alpha, const float* g_normal,
                             float* dgeom, void* stream);
int cut3r_gs_preprocess_backward(int P, const float* means, const float* scales, const float* rots, const float* opacities, const float* shs,
                                 int sh_degree, int sh_coeffs, const float* viewmatrix_host, const float* projmatrix_host,
                                 const float* campos_host, int W, int H, float tanfovx, float tanfovy, float kernel_size, float scale_modifier,
                                 const float* geom, const float* dgeom, float* d_means, float* d_scales, float* d_rots, float* d_opacities,
                                 float* d_shs, float* d_colors, float* d_means2D, void* stream);
/* ---- the mapper's training step without an autograd tape (csrc/gs_train.hip) ------------------------------------------------------
 * What the reference spreads over torch autograd per rendered view: `render` moves the Gaussians into the camera frame
 * (hislam2/gaussian/renderer/__init__.py:89-152 with utils/slam_utils.py:93-102 get_pose: pose = exp([tau, phi]) * T_w2c), the
 * activations of scene/gaussian_model.py:77-101, torch.optim.Adam of every parameter group (:374-417) and of the pose increments
 * (hislam2/gs_backend_per_frame.py:451-475), update_pose (slam_utils.py:77-91).
 * pose_state: 32 floats per view -- [0:7] world->camera (t, q_xyzw), [7:13] increment (tau, phi), [13:19] / [19:25] Adam moments, [25] steps.
 *   activate:          theta [P,14] (xyz | DC colour | opacity logit | log scale | quaternion rxyz) -> camera-frame means [P,3], scales
 *                      [P,3], rotations [P,4] (rxyz, pose rotation applied), opacities [P], colours [P,3]: the rasteriser's inputs.
 *   activate_backward: their gradients (cut3r_gs_preprocess_backward's outputs) -> gtheta [P,14] += (NULL: poses only) and pose_sums [16]
 *                      += (NULL: Gaussians only); iso_coef != 0 adds the gradient of iso_coef * sum_visible |s - mean s| / max(3 n_visible, 1)
 *                      (gs_backend_per_frame.py:533-538; radii > 0 = visible, nvis_ws: one float of scratch).
 *   pose_step:         gradient of the increments from pose_sums through exp() + 2 * prior * (2 - *ratio) * delta (the pull of pose_refine,
 *                      :262; ratio NULL: factor 1), Adam (lr_trans for tau, lr_rot for phi), fold != 0: T <- exp(delta) T, delta <- 0.
 *   adam:              GaussianMap.step over n = 14 P elements with the per-column rates lr14 [14] and host-side bias corrections.
 *   map_coef / refine_coef: the scalar algebra between cut3r_pixel_loss_forward / cut3r_refine_loss_forward and their backward passes
 *                      (upstream gradient g, resp. g_rgb / g_var); loss_acc (nullable) += the weighted loss value.
 * Exposure compensation (Training.compensate_exposure, gs_backend_per_frame.py:516, :992: a per-view affine colour model between the
 * rasteriser's colour image and the losses, its 12 parameters in the same torch.optim.Adam as the pose increments, :467-475, :959-967).
 * exposure_state: 40 floats per view -- [0:9] A row-major (A[i][j] = exposure_a[i, j], i the rendered channel, j the compensated one),
 * [9:12] b, [12:24] / [24:36] Adam moments, [36] steps, [37:40] zero.
 *   exposure_forward:  color [3,H,W] -> out [3,H,W], out[j,p] = b[j] + sum_i color[i,p] A[i][j] (fp32).
 *   exposure_backward: g = g_out + g_out2 (g_out2 nullable) -> g_color[i,p] = sum_j A[i][j] g[j,p].  g_color MAY be g_out or g_out2
 *                      itself (the same pointer, not a shifted overlap); it must not overlap color.  partials (nullable: a frozen exposure)
 *                      [cut3r_exposure_partial_rows(H, W), 12]: one row per workgroup, sum_p color[i,p] g[j,p] in the order of A, then
 *                      sum_p g[j,p]; every row is written (no zeroing needed), without atomics: the same inputs give the same bits.
 *   exposure_partial_rows: the number of those rows (-1 for a size the launchers refuse: 1 is a valid count).
 *   gs_exposure_step:  the 12 gradients = the sum of the `rows` partial rows in a fixed order, then one torch.optim.Adam step of A and b
 *                      (betas 0.9 / 0.999, eps 1e-8, step size lr / bc1, the step count kept in the state).
 * H * W must fit an int.
 * Pose-only backward against a frozen map (gs_backend_per_frame.py:123-177 pose_estimator, whose `loss.backward()` reaches only
 * cam_trans_delta / cam_rot_delta; run for every non-keyframe by util/trajectory_filler.py:60-85):
 *   gs_pose_backward:  dgeom [P,32] (cut3r_gs_render_backward) -> pose_sums [16] = M (9) | s (3) | r (4), the sums
 *                      cut3r_gs_activate_backward(gtheta = NULL) accumulates after cut3r_gs_preprocess_backward -- in ONE kernel that writes
 *                      no per-Gaussian gradient, plus a fixed-order finish.  means / scales / rots / opacities: cut3r_gs_activate's outputs
 *                      for theta and pose_state; camera arguments as cut3r_gs_preprocess_backward.  NO spherical-harmonics arguments:
 *                      colour must be view-independent (sh_degree 0 with one coefficient, or precomputed colours), where it has no
 *                      gradient to the mean -- so no campos either.  Gaussians culled by the forward pass (geom radius <= 0) contribute
 *                      exactly 0.  partials [cut3r_gs_pose_partial_rows(P), 16]: scratch, one row per workgroup, every row written (no
 *                      zeroing needed); pose_sums is WRITTEN (not accumulated) as the sum of the rows in a fixed order.  No atomics: the
 *                      same inputs give the same bits.  Each per-Gaussian term is formed in fp64 and rounded once, so every sum is within
 *                      n_visible * 2^-24 * sum |term| of the exact sum of the per-Gaussian gradients' contraction.
 *   gs_pose_partial_rows: the number of those rows (-1 for P <= 0). */
int cut3r_gs_pose_backward(int P, const float* means, const float* scales, const float* rots, const float* opacities,
                           const float* viewmatrix_host, const float* projmatrix_host, int W, int H, float tanfovx, float tanfovy,
                           float kernel_size, float scale_modifier, const float* geom, const float* dgeom, const float* theta,
                           const float* pose_state, float* partials, float* pose_sums, void* stream);
long long cut3r_gs_pose_partial_rows(int P);
int cut3r_gs_activate(int P, const float* theta, const float* pose_state, float* means, float* scales, float* rots, float* opac, float* shs,
                      void* stream);
int cut3r_gs_activate_backward(int P, const float* theta, const float* pose_state, const float* d_means, const float* d_scales,
                               const float* d_rots, const float* d_opac, const float* d_shs, const int* radii, float iso_coef, float* nvis_ws,
                               float* gtheta, float* pose_sums, void* stream);
int cut3r_gs_pose_step(float* pose_state, const float* pose_sums, float prior, const float* ratio, float lr_rot, float lr_trans, int fold,
                       void* stream);
int cut3r_gs_adam(long long n, float* theta, float* m, float* v, const float* grad, const float* lr14, float b1, float b2, float bc1, float bc2,
                  float eps, void* stream);
int cut3r_gs_map_coef(const float* sums, float w_rgb, float w_depth, float w_normal, float g, int H, int W, float* coef, float* loss_acc,
                      void* stream);
int cut3r_gs_refine_coef(const float* sums, float g_rgb, float g_var, int H, int W, float* coef, float* ratio_out, float* loss_acc,
                         void* stream);
int cut3r_exposure_forward(const float* color, const float* exposure_state, int H, int W, float* out, void* stream);
long long cut3r_exposure_partial_rows(int H, int W);
int cut3r_exposure_backward(const float* color, const float* g_out, const float* g_out2, const float* exposure_state, int H, int W,
                            float* g_color, float* partials, void* stream);
int cut3r_gs_exposure_step(float* exposure_state, const float* partials, int rows, float lr, void* stream);
/* simple_knn._C.distCUDA2 (call sites hislam2/gaussian/scene/gaussian_model.py:191,313; the extension is not vendored in the
 * reference tree): points [P,3] -> out [P], the mean squared distance to the 3 nearest other points.  P >= 4.
 * workspace: cut3r_knn3_chunks(P) * P * 3 floats (the candidates are searched in that many chunks, merged by a second kernel). */
int cut3r_knn3_chunks(int P);
int cut3r_knn3_mean_dist2(const float* points, int P, float* out, float* workspace, void* stream);
/* the same quantity (exact: the three nearest squared distances of the exhaustive search) through a uniform grid, for large maps
 * (P >= ~2e5: `gaussian_reinit` over every keyframe's pointmap, hislam2/gs_backend_per_frame.py:865-944): counting sort by cell, shells of
 * growing Chebyshev radius until the third-best distance is covered.  workspace: cut3r_knn3_grid_workspace_bytes(P) bytes. */
long long cut3r_knn3_grid_workspace_bytes(int P);
int cut3r_knn3_grid_mean_dist2(const float* points, int P, float* out, void* workspace, long long workspace_bytes, void* stream);
/* SSIM of the mapper's colour loss (hislam2/gaussian/utils/loss_utils.py:129-170: 11x11 Gaussian window, sigma 1.5, zero padding,
 * per channel).  forward: a, b [C,H,W] -> ssim_map [C,H,W] and the three partials the backward pass filters (d S / d mu1,
 * d S / d E[a^2], d S / d E[ab]).  backward: grad_a = grad_scale[0] * d(sum ssim_map)/d a  (grad_scale: ONE device float, e.g. the
 * upstream gradient over C*H*W for a mean).  b is treated as constant (the keyframe image). */
int cut3r_ssim_forward(const float* a, const float* b, int C, int H, int W, float* ssim_map, float* d_mu1, float* d_x11, float* d_x12,
                       void* stream);
int cut3r_ssim_backward(const float* a, const float* b, const float* d_mu1, const float* d_x11, const float* d_x12, int C, int H, int W,
                        const float* grad_scale, float* grad_a, void* stream);
/* the mapper's per-pixel loss terms (hislam2/gs_backend_per_frame.py:516-531: colour L1, inverse-depth L1, agreement of the normals
 * of the rendered depth with those of the keyframe depth) in one pass.  img, gt_img [3,H,W]; depth, gt_depth [H,W]; gt_normal [3,H,W]
 * (camera-frame normals of gt_depth, borders zero).  forward: sums[4] = {sum |gt - img|, sum_mask |1/d - 1/gt_d|,
 * sum_mask (1 - n(d) . gt_normal), |mask|}, mask = gt_d > 0.001 and d > 0.001.  backward: coef[3] (device) = upstream gradient times
 * weight over the normaliser of each term -> grad_img [3,H,W], grad_depth [H,W]. */
int cut3r_pixel_loss_forward(const float* img, const float* gt_img, const float* depth, const float* gt_depth, const float* gt_normal, int H,
                             int W, float fx, float fy, float cx, float cy, float* sums, void* stream);
int cut3r_pixel_loss_backward(const float* img, const float* gt_img, const float* depth, const float* gt_depth, const float* gt_normal, int H,
                              int W, float fx, float fy, float cx, float cy, const float* coef, float* grad_img, float* grad_depth,
                              void* stream);
/* global_BA's rendered-normal term (hislam2/gs_backend_per_frame.py:996-1001): mean over ALL pixels of 1 - N . n(depth), N the rendered
 * normal image [3,H,W], n(depth) the camera-frame normal of the rendered depth [H,W] (central differences of the back-projected
 * neighbours, zero on the border).  forward: sum[0] (device) = the pixel sum.  backward: coef = upstream gradient * weight / (H W);
 * grad_normal [3,H,W] is written, grad_depth [H,W] is ACCUMULATED into (after cut3r_pixel_loss_backward wrote it).  An image without
 * interior pixels (H < 3 or W < 3) is accepted: its sum is H W, grad_normal 0 and grad_depth unchanged. */
int cut3r_normal_agree_forward(const float* normal, const float* depth, int H, int W, float fx, float fy, float cx, float cy, float* sum,
                               void* stream);
int cut3r_normal_agree_backward(const float* normal, const float* depth, int H, int W, float fx, float fy, float cx, float cy, float coef,
                                float* grad_normal, float* grad_depth, void* stream);
/* densification statistics of one rendered view (hislam2/gaussian/scene/gaussian_model.py:779-790 add_densification_stats and the
 * max_radii2D update of gs_backend_per_frame.py:1021-1027): for visible Gaussians (radii > 0) max_radii2D = max(., radius),
 * grad_accum += |d_means2D.xy|, grad_accum_abs += |d_means2D.z| (the absolute-gradient statistic of the rasteriser's backward, :781), denom += 1. */
int cut3r_gs_densify_stats(int P, const int* radii, const float* d_means2D, float* max_radii2D, float* grad_accum, float* grad_accum_abs,
                           float* denom, void* stream);
/* the pose-refinement loss terms (hislam2/gs_backend_per_frame.py:240-262) in one pass: a = alpha > alpha_th, m = a and both depths >
 * 0.001.  forward: sums[5] = {sum_a |gt - img|, |a|, sum_m diff, sum_m diff^2, |m|}, diff = log d - log gt_d.  backward: coef[3] (device)
 * = {c_rgb, c_var, mean diff} -> grad_img = c_rgb sign(img - gt) on a, grad_depth = 2 c_var (diff - mean) / d on m. */
int cut3r_refine_loss_forward(const float* img, const float* gt_img, const float* depth, const float* gt_depth, const float* alpha,
                              float alpha_th, int H, int W, float* sums, void* stream);
int cut3r_refine_loss_backward(const float* img, const float* gt_img, const float* depth, const float* gt_depth, const float* alpha,
                               float alpha_th, int H, int W, const float* coef, float* grad_img, float* grad_depth, void* stream);

/* ---- TSDF fusion and mesh extraction (csrc/tsdf.hip) -------------------------------------------------------------------------------
 * A DENSE grid replaces the Open3D VoxelBlockGrid of tsdf_integrate.py: fp32 planes tsdf [N], weight [N], color [3][N] (0..255), N =
 * X*Y*Z < 2^31, voxel n = (k*Y + j)*X + i, centre (ox + voxel*i, oy + voxel*j, oz + voxel*k).  Initial values tsdf = 1, weight = color = 0.
 *
 * integrate replaces VoxelBlockGrid.integrate (tsdf_integrate.py:31-62): B in 1..16 views applied in order, each voxel read and written
 * at most once per call.  depth [B,H,W] fp32 metres, rgb u8 [B,3,H,W] or NULL (colours untouched), conf [B,ch,cw] at stride ds or NULL
 * (a pixel with conf[min(v/ds,ch-1), min(u/ds,cw-1)] < conf_min is skipped), w2c [B,12] world->camera rows, K [B,4] fx fy cx cy, all on
 * the device.  Per view in fp32: x_c = ((r0 . p) + t); skip z_c <= 0; u = fx x_c / z_c + cx rounded floor(u + 0.5), outside the image
 * skipped; skip !(0 < d <= depth_max); sdf = d - z_c, skip sdf < -trunc; t = min(1, sdf / trunc); running weighted means, weight + 1.
 *
 * mesh_count / mesh_emit replace VoxelBlockGrid.extract_triangle_mesh (tsdf_integrate.py:83-88) by marching tetrahedra over the Kuhn split
 * (six tetrahedra per cell along the corner 0 -> 7 diagonal).  A cell is valid when its 8 corners have weight >= weight_threshold; inside
 * = tsdf < 0; triangles face from negative to positive tsdf.  count writes per-voxel counts into `workspace`
 * (cut3r_tsdf_mesh_workspace_bytes: 18 B per voxel + scan scratch), scans them and writes totals [2] = (vertices, faces) as int64 on the
 * device; emit (same workspace, untouched in between) writes verts [nv,3] fp32, colors [nv,3] u8 (NULL: none) and faces [nf,3] int32:
 * vertices in (owning voxel, direction mask) order, faces in (cell, tetrahedron, triangle) order, only referenced vertices. */
int cut3r_tsdf_integrate(float* tsdf, float* weight, float* color, int X, int Y, int Z, float ox, float oy, float oz, float voxel,
                         const float* depth, const unsigned char* rgb, const float* conf, int B, int H, int W, int ch, int cw, int ds,
                         float conf_min, const float* w2c, const float* K, float trunc, float depth_max, void* stream);
long long cut3r_tsdf_mesh_workspace_bytes(int X, int Y, int Z);       /* -1 on bad dimensions */
int cut3r_tsdf_mesh_count(const float* tsdf, const float* weight, int X, int Y, int Z, float weight_threshold, void* workspace,
                          long long workspace_bytes, long long* totals, void* stream);
int cut3r_tsdf_mesh_emit(const float* tsdf, const float* color, int X, int Y, int Z, float ox, float oy, float oz, float voxel,
                         const void* workspace, long long workspace_bytes, float* verts, unsigned char* colors, int* faces, long long nv,
                         long long nf, void* stream);

/* ---- Sparse brick TSDF volume (csrc/tsdf_sparse.hip) --------------------------------------------------------------------------------
 * The dense volume above restricted to allocated bricks of 8x8x8 voxels: the same lattice over a VIRTUAL grid X x Y x Z (each <= 2^20),
 * the same per-voxel fusion, so an allocated voxel holds the dense grid's bits.  B* = ceil(dim / 8), T = BX*BY*BZ <= 2^28 table entries.
 *   flags  u8 [T]     1 = brick allocated (t = (bz*BY + by)*BX + bx)
 *   table  int32 [T]  pool slot or -1; slots number the flagged bricks by ascending t
 *   bricks int32 [nb] t of every slot, ascending; nb * 512 < 2^31
 *   pool   tsdf [nb*512], weight [nb*512], color [3][nb*512]; voxel (lk*8 + lj)*8 + li inside its brick; initial values 1 / 0 / 0
 *
 * mark sets (never clears) the flag of every brick that a view of the batch (any B >= 1, B*H*W < 2^31) can give a negative tsdf or a
 * 26-neighbour of one: per pixel with 0 < d <= depth_max the slab u +- 0.5, v +- 0.5, z in [d, d + trunc] in two z-segments, the world
 * AABB of each segment's 8 corners through c2w [B,12] (camera->world rows, the inverse of w2c), dilated by 1.5 voxels.  assign numbers
 * the flagged bricks (exclusive scan) into table and writes their count to total [1] (int64, device).  The caller builds `bricks` and
 * sizes the pool; a brick allocated after views were integrated has missed those views.
 *
 * integrate = cut3r_tsdf_integrate over the pool: one workgroup per brick, views whose frustum the brick's bounding sphere misses are
 * dropped for the whole brick.  mesh_count / mesh_emit = the dense pair over the pool voxels; an in-grid voxel of a brick that is not
 * allocated reads as tsdf = 1, weight = 0.  Vertices in (pool voxel, direction mask) order, faces in (pool cell, tetrahedron,
 * triangle) order.  Workspace: 18 B per pool voxel + scan scratch. */
int cut3r_tsdf_sparse_mark(unsigned char* flags, int X, int Y, int Z, float ox, float oy, float oz, float voxel, const float* depth, int B,
                           int H, int W, const float* c2w, const float* K, float trunc, float depth_max, void* stream);
long long cut3r_tsdf_sparse_assign_workspace_bytes(int X, int Y, int Z);       /* -1 on bad dimensions */
int cut3r_tsdf_sparse_assign(const unsigned char* flags, int* table, int X, int Y, int Z, void* workspace, long long workspace_bytes,
                             long long* total, void* stream);
int cut3r_tsdf_sparse_integrate(float* tsdf, float* weight, float* color, const int* bricks, int nb, int X, int Y, int Z, float ox, float oy,
                                float oz, float voxel, const float* depth, const unsigned char* rgb, const float* conf, int B, int H, int W,
                                int ch, int cw, int ds, float conf_min, const float* w2c, const float* K, float trunc, float depth_max,
                                void* stream);
long long cut3r_tsdf_sparse_mesh_workspace_bytes(int nb);                      /* -1 on a bad brick count */
int cut3r_tsdf_sparse_mesh_count(const float* tsdf, const float* weight, const int* table, const int* bricks, int nb, int X, int Y, int Z,
                                 float weight_threshold, void* workspace, long long workspace_bytes, long long* totals, void* stream);
int cut3r_tsdf_sparse_mesh_emit(const float* tsdf, const float* color, const int* table, const int* bricks, int nb, int X, int Y, int Z,
                                float ox, float oy, float oz, float voxel, const void* workspace, long long workspace_bytes, float* verts,
                                unsigned char* colors, int* faces, long long nv, long long nf, void* stream);

/* ---- Live TSDF volume (csrc/tsdf_live.hip) -------------------------------------------------------------------------------------------
 * The sparse brick volume above (its lattice, flags, table and bricks; mark and assign as they are) with integer accumulators, so that
 * views are added, removed and re-posed exactly while a run goes on:
 *   acc int32 [5][nb*512]   sum_q, count, sum_r, sum_g, sum_b of pool voxel slot * 512 + (lk*8 + lj)*8 + li; all zero at the start
 * A view that updates a voxel under the gates of cut3r_tsdf_integrate, with t = min(1, sdf / trunc), adds q = (int)rintf(t * 32768.f)
 * (|q| <= 32768, exact), 1 and its three u8 colour values (colour only with rgb != NULL: a volume is coloured or not for its whole life).
 * The sums depend on the set of views that are in, not on their order, the batch split or the history; at most 65535 views may be in
 * (65535 * 32768 < 2^31).
 *
 * integrate: B <= 16 views in one launch over the pool slots listed in `slots` (int32 [ns] on the device, 1 <= ns <= nb, each in
 * 0..nb-1 and listed once: the caller's contract) or over all nb when slots == NULL -- the bricks allocated after earlier views went in
 * catch up through it.  Bit b of subtract_mask takes view b out (its contribution is negated); bits at or above B are an error.  One
 * workgroup per slot, one thread per voxel, the sparse integrate's brick-versus-frustum view mask; a voxel no view touches is neither read
 * nor written, no atomics.
 *
 * resolve: the accumulators of the listed slots (or all) as the fp32 pool planes that cut3r_tsdf_sparse_mesh_* and
 * cut3r_tsdf_sparse_ray_cast read (all four pointers 16-byte aligned): count == 0 gives tsdf 1, weight 0, colour 0; else
 * tsdf = (float)((double)sum_q / ((double)count * 32768.0)), weight = (float)count, color[c] = (float)((double)sum_c / (double)count) --
 * correctly rounded means.
 * CUT3R_ERR_ARG: a null pointer, B outside 1..16, bad dims or nb, ns outside 1..nb with slots given, a subtract_mask bit >= B. */
int cut3r_tsdf_live_integrate(int* acc, const int* bricks, int nb, const int* slots, int ns, int X, int Y, int Z, float ox, float oy,
                              float oz, float voxel, const float* depth, const unsigned char* rgb, const float* conf, int B, int H, int W,
                              int ch, int cw, int ds, float conf_min, const float* w2c, const float* K, unsigned subtract_mask, float trunc,
                              float depth_max, void* stream);
int cut3r_tsdf_live_resolve(const int* acc, int nb, const int* slots, int ns, float* tsdf, float* weight, float* color, void* stream);

/* ---- Ray cast of the TSDF volumes (csrc/tsdf_raycast.hip) ----------------------------------------------------------------------------
 * Replaces Open3D VoxelBlockGrid.ray_cast, the third operation of the grid that tsdf_integrate.py:34 builds: depth, normal and colour
 * images of the fused model.  The planes / the pool with its table and brick list are those of the two families above.  c2w [B,12]
 * camera->world rows and K [B,4] fx fy cx cy on the device, B in 1..16 views of H x W, one thread per pixel, a wave per 8 x 8 tile.
 * Pixel (u, v): origin = the translation of c2w, direction d = R ((u - cx) / fx, (v - cy) / fy, 1), so the ray parameter is the
 * z-depth.  Samples t_k = t_min + (float)k * step while t_k <= t_max (at most 2^30); per axis g = ((c + t_k d) - origin) / voxel, cell =
 * floor(g).  A sample is valid when 0 <= cell < dim - 1 on every axis and the cell's eight corners are stored with weight >=
 * weight_threshold; its value is the trilinear interpolation of tsdf.  An invalid sample forgets the predecessor, a valid one with
 * value >= 0 becomes it, a valid one with value < 0 ends the ray: depth = t_{k-1} + (t_k - t_{k-1}) s_{k-1} / (s_{k-1} - s_k) when the
 * predecessor is there, else 0 (a miss: no ray looks through a back face or out of unknown space).
 * Outputs: depth [B,H,W] fp32; normal [B,H,W,3] fp32 or NULL, the normalised gradient of the interpolant at sample k (world frame,
 * towards positive tsdf; 0 on a miss); rgb u8 [B,3,H,W] or NULL, the interpolated colour rounded floor(c + 0.5) (0 on a miss);
 * samples int32 [B,H,W] or NULL, how many samples the ray looked up in the store.  Clipping to the grid and, in the brick pool, skipping
 * inside unallocated bricks leave every output bit as the plain march gives it.
 * CUT3R_ERR_ARG: a null plane, pose or depth, B outside 1..16, H, W, voxel or step <= 0, t_min < 0, t_max < t_min, bad dims or nb. */
int cut3r_tsdf_ray_cast(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox, float oy, float oz,
                        float voxel, const float* c2w, const float* K, int B, int H, int W, float t_min, float t_max, float step,
                        float weight_threshold, float* depth, float* normal, unsigned char* rgb, int* samples, void* stream);
int cut3r_tsdf_sparse_ray_cast(const float* tsdf, const float* weight, const float* color, const int* table, const int* bricks, int nb,
                               int X, int Y, int Z, float ox, float oy, float oz, float voxel, const float* c2w, const float* K, int B, int H,
                               int W, float t_min, float t_max, float step, float weight_threshold, float* depth, float* normal,
                               unsigned char* rgb, int* samples, void* stream);

/* ---- Reconstruction metrics (csrc/recon.hip) ----------------------------------------------------------------------------------------
 * mesh_area_cdf / mesh_sample replace trimesh.sample.sample_surface (scripts/eval_recon.py:104-107).  verts [V,3] fp32, faces [F,3] int32
 * (a face with an index outside 0..V-1 has area 0).  area_cdf: area [F] fp32 = 0.5 |(b - a) x (c - a)|, cdf [F] fp64 = inclusive scan of
 * the areas; workspace: cut3r_mesh_cdf_workspace_bytes(F).  sample: out [n,3]; sample i takes the first face with cdf[f] > u0 cdf[F-1]
 * and p = (a + u1 (b - a)) + u2 (c - a), (u1, u2) -> (1 - u1, 1 - u2) when u1 + u2 > 1; u_k from splitmix64 of (seed, stream_id, 3i + k):
 * u0 53 bits, u1 and u2 24 bits.  Sample i does not depend on n. */
long long cut3r_mesh_cdf_workspace_bytes(int F);                      /* -1 when F <= 0 */
int cut3r_mesh_area_cdf(const float* verts, int V, const int* faces, int F, float* area, double* cdf, void* workspace, long long workspace_bytes,
                        void* stream);
int cut3r_mesh_sample(const float* verts, int V, const int* faces, int F, const double* cdf, long long n, unsigned long long seed,
                      unsigned long long stream_id, float* out, void* stream);
/* exact 1-NN of every query point among the reference points: scipy cKDTree.query of eval_recon.py:22-41, pykdtree of
 * geometry_eval_utils.py:79-110 and the correspondence search of Open3D registration_icp (eval_recon.py:44-58).  build bins ref [P,3]
 * into a uniform grid inside `workspace` (cut3r_nn_workspace_bytes(P, Q) bytes; build needs (P, 0)); query (the same workspace, built for
 * the same P, untouched in between) transforms each query [Q,3] by T (fp32 3x4 row-major, NULL: identity) as it loads it and writes
 * dist2 [Q] fp32 (d2 = dx*dx + dy*dy + dz*dz, dx = ref.x - q.x) and idx [Q] int32, ties to the smallest reference index.  A query with no
 * reference point at d2 <= max_dist^2 gets idx -1, dist2 +inf (max_dist = +inf: no limit; < 0 or NaN is refused). */
long long cut3r_nn_workspace_bytes(int P, int Q);                     /* -1 when P <= 0 or Q < 0 */
int cut3r_nn_build(const float* ref, int P, void* workspace, long long workspace_bytes, void* stream);
int cut3r_nn_query(int P, const float* query, int Q, const float* T, float max_dist, float* dist2, int* idx, void* workspace,
                   long long workspace_bytes, void* stream);
/* the moments of one point-to-point ICP update (TransformationEstimationPointToPoint, eval_recon.py:54-56) in fp64 over the
 * correspondences (idx >= 0) of a query: out [17] = count, sum dist2, sum src [3], sum dst [3], sum src_a dst_b [3][3], src = the query
 * point under T as cut3r_nn_query loads it, dst = ref[idx].  Identical on every run.  workspace: cut3r_icp_moments_workspace_bytes(Q). */
long long cut3r_icp_moments_workspace_bytes(int Q);                   /* -1 when Q <= 0 */
int cut3r_icp_moments(const float* src, int Q, const float* ref, int P, const float* T, const float* dist2, const int* idx, double* out,
                      void* workspace, long long workspace_bytes, void* stream);

/* ---- Precision, recall, F-score (csrc/prstats.hip) ---------------------------------------------------------------------------------------
 * The reductions behind evaluate_3d_reconstruction.run_evaluation (scripts/eval_recon.py:232-235; the Tanks-and-Temples evaluation) over
 * the dist2 [Q] fp32 of cut3r_nn_query.  An entry s is BAD iff !(s >= 0) || s == +inf; it bumps counts[2] and nothing else.  A good entry
 * has d = fabs(sqrt((double)s)) (fp64; the fabs turns the -0 of s = -0.0 into +0) and goes into
 *   counts [3] int64   = (good entries, good entries with d < tau (strict), bad entries)
 *   moments [4] fp64   = (sum d, sum (double)s, min d, max d); min = +inf and max = -inf without a good entry
 *   hist [nbins] uint32: hist[k]++ for the largest integer k with (double)k * bin_width <= d, iff k < nbins -- np.histogram over
 *                        np.arange(0, nbins + 1) * bin_width, except that d == nbins * bin_width is dropped (numpy's last edge is closed)
 * nbins in 0..4096; hist may be NULL when nbins == 0.  The histogram is counted with integer atomics in LDS, then into hist; there is no
 * floating-point atomic.  Order of the two sums: G = min(ceil(Q / 1024), 1024) workgroups of 256 threads; thread t of workgroup b adds the
 * good ones among the entries 4 ((k G + b) 256 + t) + j, j = 0..3, k = 0, 1, ..., in increasing (k, j) from +0; the 256 thread sums fold
 * by the halving tree s[t] += s[t + o], o = 128, ..., 1; the G workgroup sums are added in increasing b from +0.  Identical on every run
 * and for every alignment of dist2.  One pass over dist2, nothing is read back.
 * CUT3R_ERR_ARG before any launch (outputs untouched): a null dist2, counts, moments or workspace (hist with nbins > 0), Q <= 0, tau or
 * bin_width <= 0 or NaN, nbins outside 0..4096, a workspace that is not 8-byte aligned or shorter than cut3r_dist_stats_workspace_bytes(Q). */
long long cut3r_dist_stats_workspace_bytes(int Q);                    /* -1 when Q <= 0 */
int cut3r_dist_stats(const float* dist2, int Q, double tau, double bin_width, int nbins, long long* counts, double* moments, unsigned* hist,
                     void* workspace, long long workspace_bytes, void* stream);
/* out [2] fp32 = the dist2 values of ascending ranks (n - 1) / 2 and n / 2 among the n good entries (-0.0 as +0.0), NaN when n == 0; n is
 * counted on the device.  A radix select in four 8-bit passes over the bit pattern of the non-negative float, both ranks in the same
 * passes (csrc/calib.hip's scheme); integer counts only, nothing is sorted.  Refusals as above. */
long long cut3r_dist_median_workspace_bytes(int Q);                   /* -1 when Q <= 0 */
int cut3r_dist_median(const float* dist2, int Q, float* out, void* workspace, long long workspace_bytes, void* stream);
/* cut3r_icp_moments with the moment that a similarity update needs: out [18], out[0..16] bit for bit cut3r_icp_moments' (the same grid and
 * order), out[17] = sum of ((double)x (double)x + (double)y (double)y) + (double)z (double)z of the fp32 source point under T, over the same
 * correspondences in the same order.  workspace: cut3r_icp_moments_scaled_workspace_bytes(Q), 8-byte aligned. */
long long cut3r_icp_moments_scaled_workspace_bytes(int Q);            /* -1 when Q <= 0 */
int cut3r_icp_moments_scaled(const float* src, int Q, const float* ref, int P, const float* T, const float* dist2, const int* idx, double* out,
                             void* workspace, long long workspace_bytes, void* stream);

/* ---- Mesh depth rasteriser and the 2-D depth-L1 metric (csrc/raster.hip) -----------------------------------------------------------------
 * mesh_raster replaces the off-screen Open3D window of scripts/eval_recon.py:162-213 (capture_depth_float_buffer of a mesh drawn with
 * mesh_show_back_face and set_constant_z_far(20)).  verts [V,3] fp32, faces [F,3] int32 (a face with an index outside 0..V-1 is not
 * drawn), w2c [B,12] world->camera rows (OpenCV camera: x right, y down, z forward), K [B,4] fx fy cx cy with fx, fy > 0, B in 1..16, H
 * and W in 1..65535.  depth [B,H,W] fp32, 0 where nothing is hit; face_id [B,H,W] int32 or NULL, -1 where nothing is hit.  Per pixel
 * (i, j), sampled at its centre, and triangle (a, b, c) in camera space (p_c = ((T0 x + T1 y) + T2 z) + T3, fp32): the ray d =
 * ((j - cx) / fx, (i - cy) / fy, 1) in fp32, then in fp64 e0 = d . (b x c), e1 = d . (c x a), e2 = d . (a x b); a hit when all three are
 * >= 0 or all three <= 0 (both faces), den = (e0 + e1) + e2 != 0 and z = float((a . (b x c)) / den) lies in (z_near, z_far].  A triangle
 * with no vertex in front of the camera plane is not drawn; one with all three in front is tried only inside the box of its projected
 * vertices padded by a pixel (in exact arithmetic both follow from the hit test; stated so that rounding cannot place a sliver outside
 * itself); nothing is clipped, a triangle across the camera plane is drawn where it is in front.  The pixel takes the smallest z, ties
 * the smallest face index; the result does not depend on the launch shape or on the order in which faces arrive.  The order of every
 * operation is fixed in csrc/raster.hip and restated by tests/raster_oracle.py.  z_near < 0 (or NaN) and z_far <= z_near are refused.
 * workspace: cut3r_mesh_raster_workspace_bytes(F, B, H, W). */
long long cut3r_mesh_raster_workspace_bytes(int F, int B, int H, int W);   /* -1 on bad sizes */
int cut3r_mesh_raster(const float* verts, int V, const int* faces, int F, const float* w2c, const float* K, int B, int H, int W, float z_near,
                      float z_far, float* depth, int* face_id, void* workspace, long long workspace_bytes, void* stream);
/* the per-view sums of the depth L1 (eval_recon.py:216-218): out [B,2] fp64 = (number of pixels with ours > 0, sum of |gt - ours| over
 * them), gt and ours [B,H,W] fp32.  Fixed reduction order: identical on every run.  workspace: cut3r_depth_l1_workspace_bytes(B). */
long long cut3r_depth_l1_workspace_bytes(int B);                      /* -1 when B <= 0 */
int cut3r_depth_l1(const float* gt, const float* ours, int B, int H, int W, double* out, void* workspace, long long workspace_bytes,
                   void* stream);
/* check_proj of eval_recon.py:60-89 for B in 1..16 candidate cameras at once: counts [B] int32 = how many of points [N,3] satisfy, with
 * p_c as above and z' = z - 1e-5, 0 <= z', edge < (fx x + cx z) / z' < W - edge and edge < (fy y + cy z) / z' < H - edge (the reference's
 * axis flips cancel to this). */
int cut3r_points_in_view(const float* points, int N, const float* w2c, const float* K, int B, int H, int W, float edge, int* counts,
                         void* stream);
/* which vertices a set of views sees (no reference counterpart: the reference reads GT meshes culled by an outside script): flags [V]
 * u8, flags[v] set to 1 (never cleared) when in one of the B views 0 < z <= z_far, the nearest pixel (floor(u + 0.5), u = fx (x / z) +
 * cx) is inside the image and the depth d of cut3r_mesh_raster there is 0 or z <= d + eps.  depth [B,H,W]. */
int cut3r_mesh_vertex_visible(const float* verts, int V, const float* depth, const float* w2c, const float* K, int B, int H, int W, float eps,
                              float z_far, unsigned char* flags, void* stream);

/* ---- Dense point clouds of depth maps (csrc/cloud.hip) ---------------------------------------------------------------------------------
 * depth_cloud replaces Open3D's RGBDImage.create_from_color_and_depth + PointCloud.create_from_rgbd_image(project_valid_depth_only) +
 * transform of scripts/eval7_scenes_dense.py:72-96, 111-147 for B in 1..16 views.  depth [B,H,W] fp32 metres and rgb [B,3,H,W] u8 (or
 * NULL) on the device; c2w [B,12] (any 3x4 affine, row-major) and K [B,4] = fx fy cx cy of the sampling grid are HOST arrays of doubles.
 * Grid pixel (i, j) of the H1 x W1 sampling grid reads source pixel (min(i H / H1, H - 1), min(j W / W1, W - 1)) in integer arithmetic
 * (nearest-neighbour resampling by the exact floor); it is valid iff its depth d is finite, d > 0 and d < depth_trunc.  In fp64: z = d,
 * x = (j - cx) z / fx, y = (i - cy) z / fy, each world coordinate ((r0 x + r1 y) + r2 z) + t, rounded once to fp32; the colour is the
 * source pixel's.  Output order: by view, then row-major grid pixel; count -> scan -> emit, the same bits on every run, and B views in one
 * launch give what B launches of one view give.  count fills counts [B] (device, valid pixels per view) and the workspace
 * (cut3r_depth_cloud_workspace_bytes(B, H1, W1)); emit, with that workspace untouched, writes the n = sum(counts) points [n,3] fp32 and
 * colors [n,3] u8 (colors and rgb both given or both NULL).  Refused: B outside 1..16, sizes <= 0, depth_trunc <= 0 or NaN, a non-finite
 * c2w or K, fx or fy <= 0, capacity (the points the output buffers hold) < n. */
long long cut3r_depth_cloud_workspace_bytes(int B, int H1, int W1);           /* -1 on bad sizes */
int cut3r_depth_cloud_count(const float* depth, int B, int H, int W, int H1, int W1, float depth_trunc, void* workspace,
                            long long workspace_bytes, long long* counts, void* stream);
int cut3r_depth_cloud_emit(const float* depth, const unsigned char* rgb, int B, int H, int W, int H1, int W1, const double* c2w,
                           const double* K, float depth_trunc, const void* workspace, long long workspace_bytes, float* points,
                           unsigned char* colors, long long n, long long capacity, void* stream);
/* out [7] fp32 (device) = min x y z, max x y z over the finite coordinates of points [N,3], and 1 when a coordinate is not finite (else 0):
 * exact and independent of the order.  workspace: cut3r_cloud_bounds_workspace_bytes(N). */
long long cut3r_cloud_bounds_workspace_bytes(int N);                          /* -1 when N <= 0 */
int cut3r_cloud_bounds(const float* points, int N, float* out, void* workspace, long long workspace_bytes, void* stream);
/* Open3D PointCloud.voxel_down_sample (eval7_scenes_dense.py:238-241).  lo, hi: HOST fp32 [3], the bounds of the points (cut3r_cloud_bounds).
 * Voxel index per axis floor(((double)p - ((double)lo - voxel / 2)) / voxel); one output per occupied voxel, sorted by (ix, iy, iz) (a
 * stable radix sort of the 63-bit key ix << 42 | iy << 21 | iz with the point index); the output point is the fp64 sum of the voxel's
 * points in ascending point index, one add at a time, divided by their number and rounded once to fp32; the colour (u8 [N,3] in, or NULL)
 * the same fp64 mean, floor(mean + 0.5); counts [M] int32 the points per voxel.  count sorts and writes *total = M (device); emit, with the
 * workspace (cut3r_voxel_downsample_workspace_bytes(N)) untouched, writes the M outputs.  Refused: N <= 0, voxel <= 0 or not finite,
 * non-finite or reversed bounds, an index >= 2^21 on some axis, M outside 1..N, capacity < M. */
long long cut3r_voxel_downsample_workspace_bytes(int N);                      /* -1 when N <= 0 */
int cut3r_voxel_downsample_count(const float* points, int N, double voxel, const float* lo, const float* hi, void* workspace,
                                 long long workspace_bytes, long long* total, void* stream);
int cut3r_voxel_downsample_emit(const float* points, const unsigned char* colors, int N, const void* workspace, long long workspace_bytes,
                                float* out_points, unsigned char* out_colors, int* out_counts, long long M, long long capacity, void* stream);

/* ---- Mesh clean-up after the extraction (csrc/mesh_clean.hip) ---------------------------------------------------------------------------
 * A mesh is verts [V,3] fp32, colors [V,3] u8 (or NULL) and faces [F,3] int32 on the device, 1 <= V, F <= 2^31 - 1.  Every output is one
 * definite set of bits: stable sorts, count -> scan -> emit compactions in input order, and integer atomics only.
 * faces_check runs first: *bad (device int) = 1 when a face index lies outside [0, V), else 0.  The kernels below skip such a face
 * instead of reading out of bounds, but the callers refuse the mesh. */
int cut3r_mesh_faces_check(const int* faces, int F, int V, int* bad, void* stream);
/* Vertex clustering (Open3D simplify_vertex_clustering with averaged positions, in a fixed order).  The clusters are the voxels of
 * cut3r_voxel_downsample over ALL vertices (same frame, key, stable sort and fp64 means: the same device code, lo and hi HOST fp32 [3] from
 * cut3r_cloud_bounds), numbered in ascending key order; c(v) is the cluster of vertex v.  A face becomes (c(a), c(b), c(c)); it is dropped
 * when two ids are equal (degenerate), else rotated cyclically so that the smallest id leads (orientation kept); among faces with the same
 * rotated triple the smallest input face index stays (duplicates: a stable radix sort of the triples with the face index, one 64-bit
 * pass when 3 ceil(log2 M) <= 64, else two; passes = 0 chooses, 1 or 2 force, 1 is refused when the key does not fit); the survivors come
 * out in ascending input face index; clusters that no survivor references are dropped and the rest renumbered in order.
 * count sorts the vertices and writes *total = M (device).  faces, given that M, writes totals [4] (device) = F', V', degenerate,
 * duplicate.  emit, given M, V' and F', writes out_verts [V',3], out_colors [V',3] (colors and out_colors both given or both NULL),
 * out_faces [F',3], vertex_map [V] (new index of c(v), or -1) and face_map [F'] (input index of each survivor); V' = F' = 0 is valid and
 * writes vertex_map only.  One workspace (cut3r_mesh_cluster_workspace_bytes(V, F)) carries the state from count through faces to emit.
 * events: NULL, or HOST array of hipEvent_t recorded between the stages (faces: [0] after the remap, [1] after the de-duplication; emit:
 * [0] after the means); a NULL entry is skipped.  Refused: sizes < 1, cell <= 0 or not finite, non-finite or reversed bounds, an index
 * >= 2^21 on some axis, M outside 1..V, V' > M, F' > F, a capacity (rows the output buffers hold) below V' or F'. */
long long cut3r_mesh_cluster_workspace_bytes(int V, int F);                   /* -1 on bad sizes */
int cut3r_mesh_cluster_count(const float* verts, int V, int F, double cell, const float* lo, const float* hi, void* workspace,
                             long long workspace_bytes, long long* total, void* stream);
int cut3r_mesh_cluster_faces(const int* faces, int V, int F, long long M, int passes, void* workspace, long long workspace_bytes,
                             long long* totals, void* const* events, void* stream);
int cut3r_mesh_cluster_emit(const float* verts, const unsigned char* colors, int V, int F, long long M, void* workspace,
                            long long workspace_bytes, float* out_verts, unsigned char* out_colors, int* out_faces, int* vertex_map,
                            int* face_map, long long Vout, long long Fout, long long cap_v, long long cap_f, void* const* events, void* stream);
/* Connected components (Open3D cluster_connected_triangles): two vertices are connected when a face holds both, and label(v) is the smallest
 * vertex index of v's component.  label_init sets labels [V] = scratch [V] = 0..V-1.  label_round is one round: a hook launch (per face,
 * integer atomicMin of the face's smallest label into the three vertices and into the three labels they carried, read from labels, written
 * to scratch) and a pointer-jumping launch (every vertex to the end of its chain; both arrays equal afterwards); *changed (device int) = 1
 * when a face saw two labels.  The HOST loops until *changed stays 0, at most V rounds: no kernel waits for another workgroup. */
int cut3r_mesh_label_init(int* labels, int* scratch, int V, void* stream);
int cut3r_mesh_label_round(const int* faces, int V, int F, int* labels, int* scratch, int* changed, void* stream);
/* Small-component removal (Open3D remove_triangles_by_mask on the cluster sizes).  A face belongs to the component of its first vertex, a
 * component's size is its number of faces (integer atomic adds).  Exactly one of min_faces, keep_largest is > 0 (the other 0): components
 * of size >= min_faces stay, or the first keep_largest in the order (size descending, label ascending).  Faces stay in input order;
 * vertices that no kept face references are dropped, the rest keep their order.  count writes totals [4] (device) = components, kept
 * components K, F', V'; emit writes out_verts, out_colors, out_faces, vertex_map [V], face_map [F'] as above and comps [K,2] int32 =
 * (label, size) of the kept components in that order.  Workspace: cut3r_mesh_components_workspace_bytes(V, F), untouched between the two.
 * Refused: sizes < 1, both or neither option, a negative option, counts out of range, a capacity below V', F' or K. */
long long cut3r_mesh_components_workspace_bytes(int V, int F);                /* -1 on bad sizes */
int cut3r_mesh_components_count(const int* faces, int V, int F, const int* labels, int min_faces, int keep_largest, void* workspace,
                                long long workspace_bytes, long long* totals, void* stream);
int cut3r_mesh_components_emit(const float* verts, const unsigned char* colors, int V, const int* faces, int F, void* workspace,
                               long long workspace_bytes, float* out_verts, unsigned char* out_colors, int* out_faces, int* vertex_map,
                               int* face_map, int* comps, long long Vout, long long Fout, long long K, long long cap_v, long long cap_f,
                               long long cap_k, void* stream);

/* ---- LPIPS of the rendering evaluation (csrc/lpips.hip) ---------------------------------------------------------------------------------
 * gaussian/utils/eval_utils.py:29,83,92 and :115,141,150: LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True).  fp32,
 * compiled without FMA contraction; tests/lpips_oracle.py restates every step and the maps are compared bit for bit.  Activations are
 * channels-last [n,H,W,C]; the n = 2B images of a call are the B first images followed by the B second images.  Every entry point refuses
 * (CUT3R_ERR_ARG, before any launch) null pointers, non-positive sizes and a shape whose output would be empty. */
/* eval_utils.py:29 normalize=True and the network's scaling layer: a, b [B,3,H,W] in [0,1] -> out [2B,H,W,3],
 * x = ((2 v - 1) - shift_c) / scale_c, shift (-.030, -.088, -.188), scale (.458, .448, .450), every step rounded, the division exact. */
int cut3r_lpips_input(const float* a, const float* b, int B, int H, int W, float* out, void* stream);
/* output size of a convolution along one axis, (in + 2 pad - k) / stride + 1; 0 when the arguments are not positive or nothing fits */
int cut3r_lpips_conv_out(int in, int k, int stride, int pad);
/* eval_utils.py:83,141 (the AlexNet `features` convolutions with their ReLU): x [n,H,W,Ci], w [KH,KW,Ci,Co], bias [Co] -> y [n,Ho,Wo,Co].
 * One output is acc = bias[co]; acc = fmaf(w[k,co], x[k], acc) over k = (ky KW + kx) Ci + ci ascending, a padded tap contributing
 * fmaf(w, 0, acc); then max(acc, 0).  impl 0: an implicit GEMM on v_mfma_f32_32x32x2_f32 (needs Co % 64 == 0), whose accumulation is
 * that chain, in 128-row tiles when those fill the chip and 64-row tiles otherwise (impl 2 / 3 force one); impl 1: the chain as fmaf on
 * the VALU.  The bits depend neither on n nor on impl.  Also refused: pad >= KH or KW, impl outside 0..3. */
int cut3r_lpips_conv(const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int Ci, int Co, int KH, int KW,
                     int stride, int pad, int impl, void* stream);
/* eval_utils.py:83,141 (the two 3x3 stride-2 max-pools of AlexNet `features`, no padding, floor): x [n,H,W,C] -> y [n,(H-3)/2+1,(W-3)/2+1,C];
 * H or W < 3 is refused. */
int cut3r_lpips_pool(const float* x, float* y, int n, int H, int W, int C, void* stream);
/* eval_utils.py:83,141 (one tap of the metric: unit-normalise over channels, squared difference, the 1x1 `lin` layer, spatial mean).
 * feat [2B,P,C] (C % 4 == 0), lin [C] -> v [B,P]: per pixel ss = fmaf(f_c, f_c, ss) over ascending c; n_c = f_c / sqrt(1e-8f + ss)
 * (norm 0, torchmetrics) or f_c / (sqrt(ss) + 1e-10f) (norm 1, the lpips package); d = n0_c - n1_c; v = fmaf(lin_c, d * d, v).  Then
 * score[b] (fp64, device) = (accumulate ? score[b] : 0) + sum_p v[b,p] / P, the sum in fp64 in a fixed order (no atomics). */
int cut3r_lpips_tail(const float* feat, const float* lin, int B, int P, int C, int norm, int accumulate, float* v, double* score,
                     void* stream);

/* ---- Focal length from the self-view pointmaps (csrc/calib.hip) ---------------------------------------------------------------------------
 * src/dust3r/post_process.py:12-64 estimate_focal_knowing_depth, both modes, without its final clip (one elementwise op of the caller).
 * pts fp32 [B,H,W,3] contiguous, pp fp32 [B,2], conf fp32 [B,H,W] or NULL (a pixel with conf < conf_min takes no part), focal fp32 [B] on
 * the device; pixel (row, col) has u = float(col) - ppx, v = float(row) - ppy.  fp32 per pixel, compiled without FMA contraction;
 * tests/focal_oracle.py restates both.  No floating-point atomics, no barrier across workgroups, no host synchronisation.  Refused
 * (CUT3R_ERR_ARG, before any launch): null pts / pp / focal / workspace, B < 1, H W < 1, 2 H W >= 2^31, a short or misaligned workspace. */
long long cut3r_focal_workspace_bytes(int B, int H, int W);                   /* -1 on bad sizes */
/* :38-55.  xz = x / z, yz = y / z (0 when not finite); a = xz u + yz v; b = xz xz + yz yz; f = float(double(sum a) / double(sum b)); then
 * `iters` times (the reference: 10) w = 1 / fmaxf(sqrtf(du du + dv dv), 1e-8f) with du = u - f xz, dv = v - f yz, and
 * f = float(double(sum fl32(w a)) / double(sum fl32(w b))).  fp64 sums in a fixed order: 16 workgroups per view over contiguous ranges of
 * ceil(HW / 16) pixels, 256 strided thread sums, a halving tree, the 16 partial pairs in ascending order (the file header).  iters + 2
 * launches; every workgroup re-adds the previous launch's partial pairs.  NaN for a view without a participating pixel or with sum b == 0. */
int cut3r_focal_weiszfeld(const float* pts, const float* conf, float conf_min, const float* pp, int B, int H, int W, int iters, float* focal,
                          void* workspace, long long workspace_bytes, void* stream);
/* :27-36.  The vote of rank (n - 1) / 2 (ascending) among the n non-NaN votes (u z) / x and (v z) / y of the participating pixels, which is
 * torch.nanmedian; +-inf votes take part; NaN when n == 0.  Radix select in four 8-bit passes over the order-preserving uint32 image of the
 * float: LDS histograms, integer atomicAdd into the view's 256-bin table of the pass, the next pass reads the chosen bin from it. */
int cut3r_focal_median(const float* pts, const float* conf, float conf_min, const float* pp, int B, int H, int W, float* focal,
                       void* workspace, long long workspace_bytes, void* stream);

/* ---- Multi-view depth consistency ahead of fusion and clouds (csrc/consistency.hip) ------------------------------------------------------
 * No reference counterpart: the geometric cross-check of MVSNet / Gipuma / COLMAP fusion with a free-space test.  depth [N,H,W] fp32 and
 * K [N,4] fp32 = fx fy cx cy on the device; ref [R] int32 the views to check, src [R,S] int32 their sources (-1: none), S <= 16; fwd, bwd
 * [R,S,12] fp64 (device) the rigid rows reference -> source and source -> reference.  One thread per reference pixel (u, v), the sources
 * in order, everything in fp64 in exactly this order (compiled without FMA contraction; tests/consistency_oracle.py restates it):
 *   a depth t is valid iff it is finite and 0 < t <= depth_max.  Invalid reference depth d: support = violation = 0, depth_avg = 0.
 *   x = (u - cx) d / fx, y = (v - cy) d / fy; X = ((F0 x + F1 y) + F2 d) + F3, Y, Z alike; Z <= z_min: no observation.
 *   us = fx_s X / Z + cx_s, vs alike; outside 0 <= us <= W - 1, 0 <= vs <= H - 1: no observation.
 *   x0 = floor(us), x1 = min(x0 + 1, W - 1), y alike; the taps t00 (y0,x0) t01 (y0,x1) t10 (y1,x0) t11 (y1,x1); one invalid: no observation.
 *   Z < t (1 - rel) for all four taps: violation += 1 (the source sees through the point), and this source gives no support.
 *   ax = us - x0, ay = vs - y0, ds = (t00 (1 - ax) + t01 ax)(1 - ay) + (t10 (1 - ax) + t11 ax) ay; (us, vs, ds) back-projected with the
 *   source's K, through bwd, projected with the reference's K -> (u2, v2, Z2); support += 1 and acc += Z2 (acc starts at d) iff
 *   Z2 > z_min, (u2 - u)^2 + (v2 - v)^2 < pix^2 and |Z2 - d| < rel d.
 *   support, violation [R,H,W] u8; depth_avg [R,H,W] fp32 = float(acc / (1 + support)), or NULL when not wanted.
 * No atomics: the same bits on every run.  Refused (CUT3R_ERR_ARG, before any launch): null pointers (depth_avg excepted), sizes <= 0,
 * S > 16, R > 65535, H W >= 2^31 / 16, depth_max or pix <= 0, rel outside (0, 1), z_min < 0, or a NaN among them.  A reference or source
 * index outside [0, N) reads nothing (all-zero outputs / no observation); the callers refuse such tables before the launch. */
int cut3r_depth_consistency(const float* depth, const float* K, int N, int H, int W, const int* ref, const int* src, int R, int S,
                            const double* fwd, const double* bwd, double depth_max, double pix, double rel, double z_min,
                            unsigned char* support, unsigned char* violation, float* depth_avg, void* stream);

/* ---- Diagnostic panels and frames of the Gaussian mapper (csrc/gs_panel.hip) ---------------------------------------------------------------
 * hislam2/gs_backend_per_frame.py:596-637 `viz` (its nine cells) as two launches without a host round trip; cut3r_slam_amd/gs_view.py
 * composes its frames with the same cell code.  All inputs device fp32, CHW, contiguous and FINITE (not checked); outputs uint8 HWC.
 * Compiled without FMA contraction; tests/gs_panel_oracle.py restates the arithmetic and every byte is compared.
 *   turbo cell   lo, hi = the map's fp32 min and max (apply_depth_colormap with near_plane = far_plane = None);
 *                den = fp32(double(hi) - double(lo) + 1e-10); q = clip(fp32(x - lo) / den, 0, 1), the division correctly rounded;
 *                idx = int(q * 255f) truncated; colour = TURBO_U8[idx] (csrc/turbo_u8.h: floor(T * 255 + 0.5) of matplotlib's table).
 *   colour cell  v fp32 -> floor(clamp(double(v), 0, 1) * 255 + 0.5) in fp64 (torchvision save_image of the reference's float64 panel).
 * ranges [8] uint32 (device) holds, for the four maps a, b, |a - b| and (alpha > 0.5 ? 1 : 0) in this order, the pair (~key(min), key(max)),
 * key(f) = the order-preserving image of the float (bits ^ 0x80000000 for f >= +0, ~bits below): the kernel reduces with integer maxima,
 * one atomicMax per value and workgroup, after a memset of the buffer on the stream (all zeros = nothing seen).  A NULL map leaves its
 * slots (and a NULL a or b those of |a - b|) at zero.  Refused: NULL ranges, all three maps NULL, n < 1, n >= 2^26. */
int cut3r_gs_panel_ranges(const float* a, const float* b, const float* alpha, long long n, unsigned int* ranges, void* stream);
/* out [3H,3W,3]:   gt image               | render                         | abs(gt - e) * 10, e_c = ((r0 A[0,c] + r1 A[1,c]) + r2 A[2,c]) + b_c
 *                  turbo(gt depth)        | turbo(render depth)            | turbo(abs(gt depth - render depth))
 *                  (render normal + 1) / 2 | (normal of render depth + 1) / 2 | turbo(alpha > 0.5)
 * ranges: cut3r_gs_panel_ranges(gt_depth, depth, alpha).  The normal of the render depth is gs_mapper.depth_to_normal:
 * p = ((x - cx) / fx, (y - cy) / fy, 1) d, n = cross(p(x+1,y) - p(x-1,y), p(x,y+1) - p(x,y-1)) / max(sqrt((nx nx + ny ny) + nz nz), 1e-12),
 * zero on the one-pixel border (byte 128); every product, sum, division and root rounded on its own.
 * Refused: a NULL pointer, H or W < 1, H W >= 2^26, fx or fy == 0. */
int cut3r_gs_panel(const float* gt, const float* render, const float* exposure_a, const float* exposure_b, const float* gt_depth,
                   const float* depth, const float* normal, const float* alpha, float fx, float fy, float cx, float cy, int H, int W,
                   const unsigned int* ranges, unsigned char* out, void* stream);
/* out [H,W,3] of one layer: 0 = rgb (src [3,H,W], colour cell), 1 = depth (src [H,W], turbo cell; its range is slot 0 of `ranges`, i.e.
 * cut3r_gs_panel_ranges(src, NULL, NULL), or with ranges == NULL the fixed lo, hi), 2 = normal (src [3,H,W], (n + 1) / 2 as a colour cell).
 * Refused: NULL src / out, a layer outside 0..2, H or W < 1, H W >= 2^26. */
int cut3r_gs_frame(const float* src, int layer, int H, int W, const unsigned int* ranges, float lo, float hi, unsigned char* out, void* stream);

/* Measurement aid of bench.py's roofline (no reference counterpart; not on the product path): a bare MFMA loop (v_mfma_f32_16x16x32_f16,
 * 16 independent accumulator chains per wave, 8 waves per workgroup, `grid` workgroups, `iters` x 16 MFMAs per wave, operands = 16-byte
 * chunks of data[nhalf] fp16, nhalf a power of two >= 32768) with s_memtime / s_memrealtime stamps around the loop.  stamps [grid,2] u64 =
 * (shader cycles, 100-MHz ticks) per workgroup; sink [grid*512] receives the accumulator sums.  FLOP = grid * 8 * iters * 16 * 16384. */
int cut3r_mfma_probe(const void* data, int nhalf, int iters, int grid, float* sink, unsigned long long* stamps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
