/*
 * ada_hip.h -- C ABI of libada_hip.so, the MI355X (gfx950) kernel library behind the
 * Amodal-Depth-Anything forward pass.
 *
 * The reference (zhyever/Amodal-Depth-Anything) has no FFI of its own: its lowest boundary is
 * the torch.nn / ATen call made by each L1 module.  Every entry point below
 * therefore names the reference call sites (file:line under /root/reference, DA2 =
 * src/models/amodalsynthdrive/depth_anything_v2) whose arithmetic it replaces.
 *
 * Conventions
 *  - plain C, raw device pointers, explicit sizes/strides; no torch types.
 *  - the caller owns every buffer (inputs, outputs, workspaces); the library allocates nothing.
 *    State kept by the library: a thread-local last-error string, a thread-local "last tile" code,
 *    and the process-global tuning switches of the ada_debug_* hooks at the end of this header
 *    (defaults = the shipped configuration; they select between kernels that all compute the same
 *    result, so a caller that never touches them sees a stateless library).
 *  - every launcher is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant,
 *    and returns 0 on success or a negative ADA_E* code; it never throws or exits.
 *  - "op" = the contraction-operand type the library was built for: IEEE fp16 by default
 *    (ada_operand_dtype() == ADA_DT_F16), bf16 with -DADA_OPERAND_BF16.  All accumulation,
 *    normalisation, softmax, activation and residual arithmetic is fp32.
 *  - activations of the DPT head are NHWC ("pixel rows"): row = (b*H + y)*W + x, ld = channels
 *    rounded up to a multiple of 64 (pad columns are zero).  "padded NHWC" additionally has a
 *    one-pixel zero border: [B, H+2, W+2, ld].
 */
#ifndef ADA_HIP_H
#define ADA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADA_ABI_VERSION 10   /* still 10: + ada_nearest_valid_workspace_bytes, ada_nearest_valid_fwd, ada_fill_gather_fwd, ada_push_pull_workspace_bytes, ada_push_pull_fwd (hole filling; five more exports, no signature changed, so a caller built against the earlier 10 runs unchanged).  Earlier, still 10: + ada_rank_filter_fwd, ada_extreme_filter_fwd (the rank filters; two more exports, no signature changed, so a caller built against the earlier 10 runs unchanged).  10: + ada_photo_prep_fwd, ada_mask_prep_fwd, ada_nearest_resize_fwd, ada_blend_ex (the amodal infer_image; exports only, no signature changed); later, still 10: + ada_depth_render_fwd (the rendering of infer.py:106-119; one more export, no signature changed, so a caller built against the earlier 10 runs unchanged).  History: 9: + ada_image_prep_fwd, ada_depth_resize_fwd (the raw model's infer_image; exports only, no signature changed).  History: 8 (round 6): the default-off experiment paths that lost are gone -- ada_igemm_args without ln_stats / ln_colsum / rowstat_out (EP_LNFOLD / EP_ROWSTATS) and the LayerNorm tail (ln_*), no ada_rowstats_finalize.  History: 6 (round 5): + ada_depth_stats_fwd, ada_token_diversity_fwd; 7: ada_igemm_args grows f8_from / f8_mid / f8_scales at its end and split_seg < 0 names the fp8 form of a split output (a zero-filled tail = off: every ABI-6 call means what it meant) */

/* status codes */
#define ADA_OK 0
#define ADA_EINVAL (-1)      /* bad argument (null pointer, negative size, misaligned ld ...) */
#define ADA_EUNSUPPORTED (-2) /* shape outside what the kernels implement */
#define ADA_ELAUNCH (-3)     /* HIP reported a launch failure */

/* dtypes */
#define ADA_DT_F32 0
#define ADA_DT_F16 1
#define ADA_DT_BF16 2

int ada_abi_version(void);
/* ADA_DT_F16 or ADA_DT_BF16: the operand type this build of the library contracts in. */
int ada_operand_dtype(void);
/* Text of the last error raised on the calling thread ("" if none). */
const char* ada_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM contraction with fused epilogue:   C[m, n] = sum_k A(m, k) * W[n, k]
 *
 * One MFMA kernel serves every dense contraction of the path:
 *   nn.Linear            DA2/dinov2_layers/attention.py:51,60 (qkv, proj); mlp.py:36,39 (fc1, fc2);
 *                        swiglu_ffn.py:30,33 (w12, w3)
 *   Conv2d 14x14 s14     DA2/dinov2_layers/patch_embed.py:66,76 after ada_patchify (a_mode PLAIN)
 *   Conv2d 1x1           DA2/dpt.py:172 (projects), DA2/util/blocks.py:146 (out_conv), dpt.py:149
 *   ConvTranspose2d k=s  DA2/dpt.py:88-100,173 (a_mode PLAIN + o_map SHUFFLE)
 *   Conv2d 3x3 s1/s2 p1  DA2/dpt.py:101-106,156,135,147; DA2/util/blocks.py:20-24,45-47 (a_mode CONV3)
 * with epilogues
 *   + bias                                  (every nn.Linear / Conv2d bias)
 *   GELU (exact erf)                        DA2/dinov2_layers/mlp.py:37
 *   * gamma + residual                      layer_scale.py:28 + block.py:105-106
 *   + residual                              DA2/util/blocks.py:80 (skip_add), dinov2.py:246 (pos_embed)
 *   ReLU on the operand copy                DA2/util/blocks.py:67,72 (activation before conv1/conv2)
 *   SiLU(x1)*x2                             swiglu_ffn.py:31-32 (columns interleaved by the packer)
 *   ReLU -> 1x1 conv (N -> 1) -> Sigmoid/ReLU   DA2/dpt.py:146-151 / RAW dpt.py:109-115 (tail)
 * ---------------------------------------------------------------------------------------- */

/* a_mode */
#define ADA_A_PLAIN 0 /* A(m, k) = A[m * lda + k] */
#define ADA_A_CONV3 1 /* 3x3 window gather from padded NHWC, k = (dy*3+dx)*lda + c */

/* output row maps: GEMM row m -> row of the output buffer */
#define ADA_MAP_PLAIN 0   /* row = m */
#define ADA_MAP_PAD 1     /* m=(b,y,x) in [B,Ho,Wo] -> interior of padded NHWC [B,Ho+2,Wo+2] */
#define ADA_MAP_TOKEN 2   /* m=(b,p) in [B,Np] -> token row b*(Np+1) + 1 + p (skips the cls row) */
#define ADA_MAP_SHUFFLE 3 /* ConvTranspose k=s: m=(b,y,x) in [B,Ho,Wo], n=(i,j,co) ->
                             padded NHWC [B, s*Ho+2, s*Wo+2], pixel (s*y+i, s*x+j), column co */

/* epilogue flags */
#define ADA_EP_BIAS 0x1
#define ADA_EP_GELU 0x2
#define ADA_EP_GAMMA 0x4     /* v *= gamma[n] (LayerScale) */
#define ADA_EP_RESIDUAL 0x8  /* v += res[res_row(m) * ldr + n] (fp32) */
#define ADA_EP_RELU_OP 0x10  /* ReLU applied to the operand-typed copy only */
#define ADA_EP_SWIGLU 0x20   /* columns come in (x1, x2) 32-wide groups: out = silu(x1) * x2 */
#define ADA_EP_TAIL 0x40     /* v = relu(v); d = sum_n v*tail_w[n] + tail_b; out_f32[m] = act(d) */
#define ADA_EP_RELU_F32 0x80 /* ReLU applied to the fp32 output as well */
/* (0x100, 0x200: ADA_EP_ROWSTATS / ADA_EP_LNFOLD of ABI <= 7 -- the LayerNorm folded into its consumer, a measured loss -- are gone; the bits stay unused) */

/* tail activations */
#define ADA_ACT_NONE 0
#define ADA_ACT_SIGMOID 1
#define ADA_ACT_RELU 2

typedef struct ada_igemm_args {
    int32_t M, N, K;        /* K = padded contraction length (multiple of 64); for CONV3, K = 9*lda */
    int32_t a_mode;
    const void* A;          /* op-typed */
    int64_t lda;            /* elements; multiple of 64 */
    /* CONV3 geometry: output grid [B, Ho, Wo]; input padded NHWC [B, Hp, Wp, lda]; stride 1 or 2 */
    int32_t Ho, Wo, Hp, Wp, stride;
    const void* W;          /* op-typed [N, K] row-major, K contiguous, zero padded */
    const float* bias;      /* [N] or NULL */
    const float* gamma;     /* [N] or NULL */
    const float* res;       /* fp32 residual or NULL */
    int64_t ldr;
    int32_t res_row_mod;    /* >0: res row = (m % res_row_mod) + res_row_off; 0: res row = out_f32 row */
    int32_t res_row_off;
    int32_t flags;          /* ADA_EP_* */
    float* out_f32;         /* fp32 output or NULL (may alias res) */
    int64_t ldo_f32;
    int32_t map_f32;        /* ADA_MAP_PLAIN / TOKEN */
    void* out_op;           /* op-typed output or NULL */
    int64_t ldo_op;
    int32_t map_op;         /* ADA_MAP_* */
    int32_t map_h, map_w;   /* Ho, Wo (PAD / SHUFFLE) or Np in map_h (TOKEN) */
    int32_t shuffle_s;      /* SHUFFLE: kernel = stride s; N = s*s*shuffle_c */
    int32_t shuffle_c;
    const float* tail_w;    /* TAIL: [N] fp32 */
    float tail_b;
    int32_t tail_act;
    int32_t split_seg;      /* > 0: split-precision op output -- out_op receives [hi | lo] in two column segments of
                               split_seg elements (hi = round(v), lo = round(v - hi)); 0 = plain;
                               < 0: the fp8 form of the same, seg = -split_seg: [hi: seg elements | lo8: seg bytes | hi8: seg bytes], see f8_from */
    int32_t a_dup_seg;      /* > 0: the A operand is such a split tensor: [hi | lo] segments of a_dup_seg elements per row (per tap of a
                               3x3 conv) and the contraction runs over THREE segments (hi, lo, hi -- the third re-reads the first) against
                               weights packed [w_hi | w_hi | w_lo]: x_hi w_hi + x_lo w_hi + x_hi w_lo.  K = 3 * a_dup_seg (x 9 for CONV3),
                               lda >= 2 * a_dup_seg.  0 = plain operand */
    int32_t tap_cols;       /* CONV3, > 0: sub-pixel convolution.  A stride-s transposed convolution (DA2/dpt.py:88-100 resize_layers[0/1]) followed,
                               with nothing in between, by a 3x3 convolution (DA2/dpt.py:153-159 input_projection[i][0]) is ONE 3x3 convolution
                               over the COARSE grid with s*s*Cout output columns: column block p = py*s + px (tap_cols = Cout columns each) is
                               output phase (py, px) and touches only the coarse taps its 3x3 fine window reaches -- 1, 2 or 4 of the 9.  The
                               weights are composed by the caller ([N, 9*lda] tap-major as for any CONV3, zero in the untouched blocks) and
                               tap_mask[p] (bit 3*(dy+1) + (dx+1)) names the touched taps; the kernel's k-loop for an N-tile walks the union of
                               its blocks' taps only: 36 C^2 MACs per coarse pixel instead of 160 C^2 for s = 4.  N / tap_cols <= 16.  0 = off */
    uint16_t tap_mask[16];
    int32_t a_wrap;         /* PLAIN, > 0: weight-only split precision.  The A row holds a_wrap operand-typed elements and the contraction runs over
                               K = 2 * a_wrap with the A walk starting over at k = a_wrap, against weights packed [w_hi | w_lo] (w_hi = round(w),
                               w_lo = round(w - w_hi)):  x w_hi + x w_lo  -- the weight's rounding error is gone, the activation's stays
                               (used where the activation is produced in the operand type anyway: attention output, SwiGLU hidden).  0 = off */
    int32_t bias_row_mod;   /* > 0: one bias vector per group of bias_row_mod consecutive rows: row m uses bias[(m / bias_row_mod) * N + n].  The
                               use_clstoken read-out (DA2/dpt.py:110-117,164-167: Linear(2D, D) on [patch | class token] + GELU) is a D -> D GEMM over
                               the patch tokens whose bias W_cls cls_b + b differs per image: one launch for the whole batch.  Operand-typed output
                               only (bias / GELU epilogues).  0 = one bias vector [N] */
    /* fp8 correction terms of a split-precision product (gfx950 v_mfma_scale_f32_16x16x128_f8f6f4, twice the fp16 matrix rate):
         x w  ~  x_hi w_hi  +  2^-10 x_lo8 w_hi8  +  x_hi8 w_lo8          (instead of three fp16 products, a_dup_seg)
       f8_from > 0: inside each period of the k-walk -- all K operand slots of a PLAIN operand, one tap (lda slots) of a CONV3 one -- the slots from
       f8_from on hold BYTES, two codes per slot: e5m2 for A, e4m3 for W, contracted 128 codes per k-step into the same fp32 accumulators.
       Slots [f8_from, f8_mid) use the scale pair in bits 0-15 of f8_scales (A byte, then W byte), [f8_mid, period) the pair in bits 16-31; a scale
       byte e multiplies its operand by 2^(e - 127) (E8M0).  The A layout [hi: seg slots | lo8: seg bytes | hi8: seg bytes] is what a producer writes
       for split_seg = -seg (lo8 = e5m2((v - hi) 2^10), hi8 = e5m2(v)); the weights are packed [w_hi | w_hi8 | w_lo8] with per-tensor power-of-two
       scales: K = 2 seg (x 9), f8_from = seg, f8_mid = 3 seg / 2, f8_scales = 117 | sb_hi << 8 | 127 << 16 | sb_lo << 24.  f8_from, f8_mid: multiples
       of 64.  Excludes a_dup_seg / a_wrap.  0 = off */
    int32_t f8_from, f8_mid;
    uint32_t f8_scales;
} ada_igemm_args;

int ada_igemm(const ada_igemm_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused scaled-dot-product attention, head_dim 64 (all of ViT-S/B/L/G):
 *   softmax(q k^T) v per (batch, head).  q must arrive pre-scaled by head_dim^-0.5 * log2(e) (folded into
 *   the qkv weights by the packer): the kernel evaluates the softmax in base 2, softmax_e(s) = softmax_2(s log2 e).  Replaces DA2/dinov2_layers/attention.py:53-59 (and the xformers
 *   memory_efficient_attention call at :76).  qkv is the packed output of the qkv linear:
 *   [B*N, 3*heads*64] with column = which*heads*64 + head*64 + d (attention.py:51 reshape).
 *   out: [B*N, heads*64] op-typed (the "transpose(1,2).reshape(B,N,C)" layout of :59).
 *   The N x N score matrix is never materialised: K/V tiles of 64 keys are staged through LDS,
 *   softmax runs online in fp32 registers.
 *   Score range: q k^T (log2 units, after the pre-scale) is tested for +-4096 with any placement over the key tiles -- every
 *   key, the first tile only, some query rows only, a maximum that climbs tile by tile (tests/test_gpu_attention_values.py);
 *   nothing upstream bounds it.  The shipped kernel keeps the running maximum in fp32.  The alternate kernel
 *   (ada_debug_set_attention_variant(3)) keeps it in the operand type and so has a hard limit the shipped one has not: the
 *   maximum is rounded to the operand type's grid (fp16: steps of 2 below 4096 and of 4 above, nothing beyond 65504) and P
 *   carries what the rounding leaves.
 * ---------------------------------------------------------------------------------------- */
int ada_attention_fwd(const void* qkv, void* out, int32_t batch, int32_t n_tokens, int32_t heads,
                      void* stream);
/* ABI 8: the same with a row stride for `out` (ld_out elements; 0 = heads * 64) and a split-precision output for the blocks whose linear layers run in split
 * precision -- the attention output feeds attn.proj (attention.py:60) and exists in the operand type only.  split_seg > 0: row = [hi | lo], lo = round(v - hi) at
 * column + split_seg;  split_seg < 0, seg = -split_seg: row = [hi: seg elements | lo8: seg bytes | hi8: seg bytes] (e5m2((v - hi) 2^10), e5m2(v)) -- the forms
 * ada_igemm reads through a_dup_seg / f8_from.  |split_seg| >= heads * 64, ld_out >= 2 |split_seg|.  0 = the plain row. */
int ada_attention_ex(const void* qkv, void* out, int32_t batch, int32_t n_tokens, int32_t heads, int64_t ld_out, int32_t split_seg,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension, eps inside the sqrt, biased variance, fp32 statistics:
 *   nn.LayerNorm(D, eps=1e-6)   DA2/dinov2.py:96,185 used at block.py:84,87 and dinov2.py:337-338
 *   channels-first LayerNorm    DA2/dpt.py:55-61 (on NHWC rows it is the same row-wise op)
 * in: fp32 [rows, ld_in]; normalises the first `dim` columns of each row.
 * Row selection: group_in > 0 treats the input as groups of `group_in` rows and skips the first
 * `skip` rows of each group (drops the cls token: dinov2.py:339-340); output rows are compacted.
 * Output (either may be NULL): op-typed with row map (PLAIN or PAD) and optional ReLU
 * (DA2/dpt.py:158), and/or fp32 plain.  split_seg > 0 writes the op-typed output in split precision
 * ([hi | lo] column segments, see ada_igemm_args.split_seg).
 * ---------------------------------------------------------------------------------------- */
int ada_layernorm_fwd(const float* in, int64_t ld_in, int32_t rows_out, int32_t dim,
                      int32_t group_in, int32_t skip,
                      const float* weight, const float* bias, float eps,
                      void* out_op, int64_t ld_op, int32_t map_op, int32_t map_h, int32_t map_w,
                      int32_t relu,
                      float* out_f32, int64_t ld_f32, int32_t split_seg, void* stream);

/* The same kernel with its two extensions (struct arguments; zero-initialise what is not used):
 *  - a SECOND operand-typed output of the same rows with the same statistics but its own gain / bias: the four tap LayerNorms of
 *    get_intermediate_layers (DA2/dinov2.py:337-340: shared final norm, cls token dropped) read the very rows the next block's norm1
 *    (block.py:84) reads, so one pass emits both -- rows are taken in groups of out2_group, the first out2_skip rows of a group are
 *    left out of the second output and the others compacted;
 *  - sub-pixel input (unshuffle_s = s > 0): `in` is the [coarse pixel, s*s*dim] fp32 output of a sub-pixel convolution
 *    (ada_igemm_args.tap_cols) and output row r is FINE pixel (b, Y, X) of the map_h x map_w grid, whose values are columns
 *    [(Y%s * s + X%s) * dim, +dim) of coarse pixel (b, Y/s, X/s) -- the channels-first LayerNorm + ReLU of input_projection
 *    (DA2/dpt.py:153-159) reads the merged convolution's output in place.  tap_bias [s*s*dim, 9] (optional) holds, per output column
 *    and coarse tap, the transposed convolution's bias as seen through the 3x3 filter; on the outermost ring of the fine grid the taps
 *    that fall outside the image are subtracted (zero padding applies to the transposed conv's OUTPUT, bias included). */
typedef struct ada_layernorm_args {
    const float* in;
    int64_t ld_in;
    int32_t rows_out, dim, group_in, skip;
    const float* weight;
    const float* bias;
    float eps;
    void* out_op;
    int64_t ld_op;
    int32_t map_op, map_h, map_w, relu;
    float* out_f32;
    int64_t ld_f32;
    int32_t split_seg;
    const float* weight2;
    const float* bias2;
    void* out2_op;
    int64_t ld2_op;
    int32_t out2_group, out2_skip, split_seg2;
    int32_t unshuffle_s;
    const float* tap_bias;
    int32_t identity;       /* 1: no normalisation, y = x (weight / bias may be NULL): with unshuffle_s the kernel is the re-layout pass behind a sub-pixel
                               convolution whose consumer is not a LayerNorm (raw head: resize_layers[i] + layerN_rn).  relu: 0 none, 1 both outputs,
                               2 the operand-typed output only (the fp32 copy is the pre-activation the ResidualConvUnit adds back, util/blocks.py:57-80) */
} ada_layernorm_args;
int ada_layernorm_ex(const ada_layernorm_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * 3x3 convolution of an align-corners bilinear up-sampling with the channel mixing moved in front of the resize:
 *   scratch.output_conv1( F.interpolate(refinenet1 output, x2, bilinear, align_corners=True) )      DA2/dpt.py:192-193, util/blocks.py:144-146
 * A 1x1 channel mix commutes with a per-channel resample, so
 *   conv3x3(resize(z))[Y, X, co] = b[co] + sum over the taps t = (dy, dx) whose position (Y + dy - 1, X + dx - 1) lies inside the fine grid of
 *                                  resize(W_t z)[Y + dy - 1, X + dx - 1, co]
 * in: [B * hi * wi, ld_in], fp32 or operand-typed (in_dtype = ADA_DT_F32 / the library's operand type), column t * channels + co = (W_t z)[co] on the COARSE grid (one ada_igemm with N = 9 * channels; the
 *     caller composes W_t with whatever 1x1 convolution precedes the resize -- refinenet1.out_conv -- and puts that convolution's bias, seen
 *     through W_t, into the GEMM's bias: a tap that falls into the zero padding then drops out whole, as it must).
 * out: fp32 [B * ho * wo, ld_out].  channels in {32, 64, 128}; an up-sampling is expected (the patch under an 8 x 16 tile must fit LDS).
 * A quarter of the 3x3 convolution's MACs on the 2x finer grid, and the up-sampled operand map is never written.
 * ---------------------------------------------------------------------------------------- */
int ada_tapsum_resize_fwd(const void* in, int32_t in_dtype, int64_t ld_in, int32_t batch, int32_t hi, int32_t wi, int32_t ho, int32_t wo, int32_t channels,
                          const float* bias, float* out, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patchify: the im2col half of the 14x14/stride-14 patch-embed convolutions
 * (DA2/dinov2_layers/patch_embed.py:76 for RGB, DA2/dinov2.py:239 for the guidance embed) with
 * the ImageNet normalisation of src/models/amodalsynthdrive/dav2.py:65 fused in.
 * x: fp32 NCHW [B,3,H,W]; guide: fp32 NCHW [B,Cg,H,W] or NULL (Cg = 0).
 * out: op-typed [B*(H/14)*(W/14), ld] with column (c*196 + dy*14 + dx), c over RGB then guide
 * channels; columns >= (3+Cg)*196 are written as zero.  mean/inv_std: [3] fp32 HOST pointers or NULL (raw
 * model, already normalised by the caller: infer.py:19).
 * split = 1 (split-precision embed): ld = 2 * segment and the row holds [hi | lo], hi = round_op(x),
 * lo = round_op(x - hi); with weights packed as [w_hi | w_hi | w_lo] the following GEMM evaluates the patch
 * embedding to ~fp32 accuracy on the fp16 matrix cores (3x the MACs of a layer that is 0.2 % of the model).
 * ---------------------------------------------------------------------------------------- */
int ada_patchify(const float* x, const float* guide, int32_t batch, int32_t cg, int32_t height,
                 int32_t width, const float* mean, const float* inv_std, void* out, int64_t ld,
                 int32_t split, void* stream);

/* Position table for a patch grid other than the native sq x sq one (DA2/dinov2.py:199-230): bicubic resample (ATen
 * upsample_bicubic2d semantics: A = -0.75, align_corners = False, the given scale factors, antialias off) of
 * pos[1:, :] viewed as [sq, sq, dim]; row 0 (cls) is copied.  pos: fp32 [1 + sq*sq, dim]; out: fp32 [1 + ph*pw, dim];
 * scale_h / scale_w: the scale_factor pair the reference passes ((ph + 0.1) / sq, (pw + 0.1) / sq).  Runs once per grid. */
int ada_pos_embed_resize(const float* pos, int32_t sq, int32_t dim, int32_t ph, int32_t pw, double scale_h,
                         double scale_w, float* out, void* stream);

/* cls row of the token matrix: tokens[b, 0, :] = cls + pos[0]  (DA2/dinov2.py:245-246). */
int ada_write_cls(float* tokens, int32_t batch, int32_t n_tokens, int32_t dim, const float* cls,
                  const float* pos0, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=True, on NHWC fp32 rows, with optional fused skip add:
 *   out(b,y,x,:) = bilinear(in)(b,y,x,:) [+ add(b,y,x,:)]
 * Replaces F.interpolate at DA2/util/blocks.py:144 and DA2/dpt.py:194, and the skip_add of
 * DA2/util/blocks.py:133.  Outputs (either may be NULL): fp32 plain [B*Ho*Wo, ld_f32]; op-typed
 * with row map PLAIN or PAD and optional ReLU (the activation opening the next ResidualConvUnit,
 * DA2/util/blocks.py:67).  split_seg > 0: split-precision op output as in ada_igemm_args.split_seg.
 * ---------------------------------------------------------------------------------------- */
int ada_bilinear_fwd(const float* in, int64_t ld_in, int32_t batch, int32_t hi, int32_t wi,
                     int32_t ho, int32_t wo, int32_t channels, const float* add, int64_t ld_add,
                     float* out_f32, int64_t ld_f32, void* out_op, int64_t ld_op, int32_t map_op,
                     int32_t relu, int32_t split_seg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused DPT tail: bilinear resize (align_corners=True) of the fp32 NHWC map `in` [B, hi, wi, >= cp channels] to [B, ho, wo],
 * 3x3 convolution (padding 1) to 32 channels + bias, ReLU, 1x1 convolution to one channel + tail_b, activation -- reference
 * DA2/dpt.py:194-195 (F.interpolate + scratch.output_conv2; raw model RAW/dpt.py:148-150) in one kernel; the up-sampled
 * map is never written to memory.  w: op-typed [32, 9 * cp] tap-major (the ada_igemm CONV3 packing), cp = channels padded to
 * a multiple of 64 (weights of pad channels zero; `in` rows must hold cp readable floats: ld_in >= cp).  out: fp32 [B, ho, wo].
 * Limits (ADA_EUNSUPPORTED otherwise; callers fall back to ada_bilinear_fwd + the EP_TAIL ada_igemm): cp is 64 or 128 (the weights of
 * every 64-channel pass stay in LDS), and the vertical scale is an up-sampling by at least 1.5 (a 10-row halo tile of the output must
 * lie within 8 source rows; the model's ratio is always 14 / 8).  Any horizontal scale.
 * ---------------------------------------------------------------------------------------- */
int ada_dpt_tail_fwd(const float* in, int64_t ld_in, int32_t batch, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                     int32_t cp, const void* w, const float* bias, const float* tail_w, float tail_b, int32_t tail_act,
                     float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depth evaluation sums.  Replaces the host-side numpy/torch evaluation of the reference:
 * the masked reductions behind src/util/metric.py:37-160 (abs_relative_difference, squared_relative_difference,
 * rmse_linear, rmse_log, log10, threshold_percentage = delta1/2/3, i_rmse, silog_rmse) and the normal-equation sums of
 * align_depth_least_square (src/util/alignment.py:7-54), all from ONE pass over the maps.
 *   pred, gt   fp32 [B, n_per_image];  mask uint8 [B, n_per_image] (non-zero = valid) or NULL (all valid)
 *   scale_shift fp32 [B, 2] or NULL: p = pred * scale + shift is what gets evaluated (the aligned prediction);
 *               clip_lo < clip_hi additionally clamps p to [clip_lo, clip_hi] (dataset depth range); like torch.clamp the clamp
 *               passes a NaN on, so a NaN prediction under the mask makes every sum that depends on p NaN for its image
 *   sums       fp64 [B, ADA_EVAL_NSUM] (overwritten), indexed by the ADA_EVAL_* constants; p, gt must be > 0 where valid
 *               for the log / ratio / inverse terms to be meaningful (as in the reference)
 * ---------------------------------------------------------------------------------------- */
#define ADA_EVAL_N 0          /* valid pixels */
#define ADA_EVAL_SUM_P 1      /* sum p */
#define ADA_EVAL_SUM_G 2      /* sum gt */
#define ADA_EVAL_SUM_PP 3     /* sum p*p */
#define ADA_EVAL_SUM_PG 4     /* sum p*gt */
#define ADA_EVAL_ABS_REL 5    /* sum |p-gt|/gt */
#define ADA_EVAL_SQ_REL 6     /* sum (p-gt)^2/gt */
#define ADA_EVAL_SQ 7         /* sum (p-gt)^2 */
#define ADA_EVAL_LOG_SQ 8     /* sum (ln p - ln gt)^2 */
#define ADA_EVAL_LOG 9        /* sum (ln p - ln gt) */
#define ADA_EVAL_LOG10_ABS 10 /* sum |log10 p - log10 gt| */
#define ADA_EVAL_D1 11        /* #{max(p/gt, gt/p) < 1.25} */
#define ADA_EVAL_D2 12        /* ... < 1.25^2 */
#define ADA_EVAL_D3 13        /* ... < 1.25^3 */
#define ADA_EVAL_INV_SQ 14    /* sum (1/p - 1/gt)^2 */
#define ADA_EVAL_NSUM 16
int ada_depth_eval_fwd(const float* pred, const float* gt, const uint8_t* mask, int32_t batch,
                       int64_t n_per_image, const float* scale_shift, float clip_lo, float clip_hi,
                       double* sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * The paper's evaluation protocol (reference: src/trainer/discriminative_trainer.py:496-613, src/scripts/pix2gestalt_eval.py:200-297): the
 * prediction is fitted onto the OBSERVATION over the VISIBLE mask, and the metrics are taken over the invisible region, raw and aligned.
 * Every map is [B, h, w] contiguous at the evaluation size; the prediction is fp32 [B, hp, wp] and is gathered inside both passes by ATen's
 * legacy nearest rule, per axis  src = min((int)floorf(dst * ((float)in / out)), in - 1)  (the identity for equal sizes).  Masks are uint8,
 * non-zero = inside.
 *   ada_protocol_fit_fwd   fit fp64 [B, ADA_FIT_NCOL] (overwritten), indexed by ADA_FIT_*: over visible != 0 the count, sum p, sum o, sum p p,
 *                          sum p o, min p, max p (+inf / -inf without a visible pixel); the counts of visible != 0 and of whole != 0 (the
 *                          difficulty bucket's ratio); scale and shift minimising sum (p scale + shift - o)^2, solved in fp64 from the normal
 *                          equations.  Two rank-deficient systems get numpy.linalg.lstsq's minimum-norm answer in closed form: no visible
 *                          pixel (0, 0); every visible p equal to c, i.e. min == max, (c m / (c c + 1), m / (c c + 1)) with m the mean o.
 *   ada_protocol_eval_fwd  sums fp64 [B, 2, ADA_EVAL_NSUM] (overwritten), the ADA_EVAL_* sums over region != 0 && valid != 0 (valid NULL:
 *                          every pixel valid) of g = gt + eps against  row 0: p = pred + eps;  row 1: p = (pred * scale) + shift + eps  with
 *                          scale / shift the fp32 roundings of the fit row's (the product is rounded before the sum, as in ada_blend_ex).  No
 *                          clamp: a negative p turns exactly the three log sums into NaN.
 * Neither uses atomics.  An image is cut into ceil(h w / ADA_PROTOCOL_CHUNK) chunks, each reduced by one workgroup in a fixed order, and the
 * chunk partials are added in index order: an image's result is bit-identical from run to run and alone or inside any batch.
 *   workspace  device memory, 8-byte aligned, at least  batch * ceil(h w / ADA_PROTOCOL_CHUNK) * ADA_PROTOCOL_WS_DOUBLES * 8  bytes (checked);
 *              contents are scratch, and the two calls may share it (they run in stream order).
 * ---------------------------------------------------------------------------------------- */
#define ADA_PROTOCOL_CHUNK 4096      /* pixels per chunk */
#define ADA_PROTOCOL_WS_DOUBLES 32   /* fp64 words of workspace per chunk */
#define ADA_FIT_N 0           /* visible pixels */
#define ADA_FIT_SUM_P 1       /* sum p */
#define ADA_FIT_SUM_O 2       /* sum o */
#define ADA_FIT_SUM_PP 3      /* sum p*p */
#define ADA_FIT_SUM_PO 4      /* sum p*o */
#define ADA_FIT_MIN_P 5
#define ADA_FIT_MAX_P 6
#define ADA_FIT_N_VISIBLE 7   /* #{visible != 0} */
#define ADA_FIT_N_WHOLE 8     /* #{whole != 0} */
#define ADA_FIT_SCALE 9
#define ADA_FIT_SHIFT 10
#define ADA_FIT_NCOL 12
int ada_protocol_fit_fwd(const float* pred, int32_t hp, int32_t wp, const float* observation, const uint8_t* visible, const uint8_t* whole,
                         int32_t batch, int32_t h, int32_t w, double* fit, void* workspace, int64_t workspace_bytes, void* stream);
int ada_protocol_eval_fwd(const float* pred, int32_t hp, int32_t wp, const float* gt, const uint8_t* region, const uint8_t* valid,
                          const double* fit, float eps, int32_t batch, int32_t h, int32_t w, double* sums, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-side glue of the two-model pipeline of infer.py (kept in HBM instead of bouncing through numpy):
 *   ada_minmax_fwd     per-image min / max of a [B, n] fp32 map -> minmax[B, 2]          (infer.py:22)
 *                      as torch's amin / amax: one NaN in an image makes both of its results NaN
 *   ada_normalize_fwd  norm = (d - min) / (max - min) and/or obs = norm * 2 - 1          (infer.py:22,92)
 *   ada_blend_fwd      out = mask > 0 ? amodal : base, then a 3x3 box blur (reflect-101 borders, = cv2.blur)
 *                      on the pixels whose 3x3 mask neighbourhood is mixed                (infer.py:30-44)
 * all tensors fp32, [B, H, W] contiguous; mask is 0/1 (anything > 0 counts as inside).
 * ---------------------------------------------------------------------------------------- */
int ada_minmax_fwd(const float* in, int32_t batch, int64_t n_per_image, float* minmax, void* stream);
int ada_normalize_fwd(const float* in, const float* minmax, int32_t batch, int64_t n_per_image, float* norm,
                      float* obs, void* stream);
int ada_blend_fwd(const float* amodal, const float* base, const float* mask, int32_t batch, int32_t height,
                  int32_t width, float* out, void* stream);

/* ada_blend_fwd with the alignment step of the reference's demo (app.py:214-216, 249-265: linear_regression_predict before median_filter_blend):
 *   scale_shift  DEVICE fp32 [B, 2] = (scale, shift) per image, or NULL.  The pasted value is amodal * scale + shift in fp32, the product rounded
 *                before the sum (torch's `slope * x + intercept`, app.py:263: no FMA); base, the paste rule and the border blur are ada_blend_fwd's.
 *                A NaN pair (an image whose fit had no support) gives NaN inside its mask and on the blurred border.
 *   NULL         launches the kernel of ada_blend_fwd itself: bit-identical to it. */
int ada_blend_ex(const float* amodal, const float* base, const float* mask, const float* scale_shift, int32_t batch, int32_t height,
                 int32_t width, float* out, void* stream);

/* Per-image moments of a sigmoid-head depth map (output of nn.Sigmoid(), reference DA2/dpt.py:146-151): sums[(b * chunks + c) * 2 + {0, 1}] =
 * (sum s, sum s (1 - s)) over chunk c of image b; the caller adds the chunk sums (fixed order, no atomics: bit-reproducible).  sum s(1-s) / sum s
 * is the factor by which the sigmoid compresses the head's logit error in mean|a - b| / mean|b| for this image: hip_ext/engine.py's precision
 * ladder re-runs the DPT head in split precision for the images where it is large (depth maps concentrated near 0).  No reference counterpart.
 * ABI 8: `act` (ADA_ACT_*) names the final activation of the head and with it the pair that plays this role -- the sensitivity of the metric to a logit
 * error of mean size eps is eps * sums[1] / sums[0]:  SIGMOID (sum s, sum s (1 - s));  RELU (sum out, number of positive outputs) -- a clipped pixel
 * carries no error, and a map that is mostly clipped with the rest just above the kink has a small denominator (RAW/dpt.py:109-115,182-184);  NONE
 * ('ssi' logits: sum |out|, number of outputs). */
int ada_depth_stats_fwd(const float* in, int32_t batch, int64_t n_per_image, int32_t chunks, int32_t act, float* sums, void* stream);
/* Token diversity of an encoder tap (operand-typed [batch * rows_per_image, ld], the first `dim` columns of a row): for image b and column chunk j
 * (64 columns; ceil(dim / 64) chunks)  sums[(b * chunks + j) * 2 + {0, 1}] = (sum over the chunk's columns of Var_rows, sum of E_rows[t^2]).  The caller adds the
 * chunks; sum Var / sum E[t^2] ~ 0.02 marks inputs whose patch tokens are all alike (constant images), where the head's operand rounding errors add
 * coherently: the second trigger of hip_ext/engine.py's precision ladder.  No reference counterpart. */
int ada_token_diversity_fwd(const void* tap, int64_t ld, int32_t batch, int32_t rows_per_image, int32_t dim, float* sums, void* stream);
/* The precision ladder's decision and paste on the device: from the three statistics blocks above, still on the device, the rung of every image of a
 * FIRST-rung run (hip_ext/ladder.py ladder_decide with ran = 1: the guard band plays no part) and the image's rows from the output of that rung.  Every
 * pointer is a DEVICE pointer; the launch sequence (two kernels) depends on no device value, so it can be captured into a HIP graph.  No reference
 * counterpart.
 *   stat_sums   fp32 [batch, chunks, 2], as ada_depth_stats_fwd writes it; read only when has_r
 *   stat_div    fp32 [batch, groups, 2] of the last tap, as ada_token_diversity_fwd writes it, or NULL (no tap-diversity trigger)
 *   stat_in     fp32 [batch, groups_in, 2] of the patchified input, or NULL
 *   decision    per image, in fp64, the pairs of a block added in index order starting from +0:
 *                 r       = has_r ? S1 / clamp(S0) : 0                      (S0, S1) = the sums of stat_sums
 *                 tap_div = V / clamp(E),  in_div likewise                  (V, E)   = the sums of stat_div / stat_in
 *                 flat    = (stat_div && tap_div < div) || (stat_in && in_div < div_in)
 *                 rung    = has3 && (flat || r > thr3) ? 3 : has2 && (flat || r > thr) ? 2 : 1
 *               clamp(x) = x < 1e-300 ? 1e-300 : x, torch's clamp_min: a NaN passes through it (and then compares false everywhere: rung 1 unless
 *               flat); `/` is the correctly rounded fp64 division.  thr / thr3 = +inf: no threshold on r.
 *   out         fp32 [batch, n_per_image]: the first rung's output, updated IN PLACE.  Rows of rung-1 images are not touched.
 *   src2, src3  fp32 [batch, n_per_image], the second / third rung's output for the WHOLE batch, either may be NULL; neither may alias out.  Image b's
 *               row is copied (as bits) from src2 where rung[b] == 2 and from src3 where rung[b] == 3.  Where that source is NULL the best available
 *               is taken -- rung 3 without src3: src2, else the row stays -- and the image counts as UNSERVED; rung[b] still names the rung it decided.
 *               16-byte accesses wherever a row of out and its source row are congruent mod 16, word accesses in front of and behind them.
 *   rung        int32 [batch], ratio fp64 [batch] (= r): overwritten
 *   counts      int64 [4], ADDED to: calls, images on rung >= 2, images on rung 3, unserved images.  The caller zeroes it once.
 * batch <= 65535. */
int ada_ladder_select_fwd(const float* stat_sums, int32_t chunks, const float* stat_div, int32_t groups, const float* stat_in, int32_t groups_in,
                          int32_t batch, double thr, double thr3, double div, double div_in, int32_t has2, int32_t has3, int32_t has_r,
                          float* out, const float* src2, const float* src3, int64_t n_per_image, int32_t* rung, double* ratio, int64_t* counts,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Image preparation and depth read-out of the raw model's infer_image / image2tensor (RAW/dpt.py:186-221), which the reference does on
 * the host with OpenCV and numpy (RAW/util/transform.py:5-158):
 *   ada_image_prep_fwd    cv2.cvtColor(BGR2RGB) / 255.0, cv2.resize(INTER_CUBIC) to ho x wo, (v - mean) / std, HWC -> CHW    (RAW/dpt.py:210-214)
 *     src      uint8 HWC [B][hi][wi][channels], BGR (channels = 3) or BGRA (4: alpha ignored, as cvtColor(BGR2RGB) does); pixels packed, rows
 *              row_pitch_bytes apart (>= wi * channels: a crop of a decoded frame is read in place), images image_stride_bytes apart
 *     out      fp32 NCHW [B, 3, ho, wo], RGB order.  mean / std: [3] fp32 HOST pointers, RGB order
 *     OpenCV's float path of INTER_CUBIC: scale_x = 1 / ((double)wo / wi); fx = (float)((dx + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx;
 *     taps sx - 1 .. sx + 2 clamped to the image (fx is kept at the borders); fp32 coefficients of cv2's interpolateCubic (A = -0.75);
 *     horizontal pass, then vertical (the same for y).  No antialiasing, and the result is NOT clamped: the overshoot of the cubic kernel
 *     at edges (below 0, above 1 before normalisation) is kept, as the reference keeps it.  Accumulation is fp32 (cv2: float64).
 *   ada_depth_resize_fwd  F.interpolate(depth[:, None], (ho, wo), mode="bilinear", align_corners=True)                        (RAW/dpt.py:192)
 *     in fp32 [B, hi, wi] -> out fp32 [B, ho, wo], both contiguous; ATen's arithmetic: scale = (in - 1) / (out - 1) in fp32 (0 when out == 1),
 *     src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), lambda = src - i0.  Any size in either direction (one channel: ada_bilinear_fwd
 *     needs channels % 4 == 0 and at most 2^24 output pixels).
 * Both: ho <= 262140, batch <= 65535.
 * ---------------------------------------------------------------------------------------- */
int ada_image_prep_fwd(const uint8_t* src, int32_t batch, int32_t hi, int32_t wi, int32_t channels, int64_t row_pitch_bytes,
                       int64_t image_stride_bytes, int32_t ho, int32_t wo, const float* mean, const float* std, float* out, void* stream);
int ada_depth_resize_fwd(const float* in, int32_t batch, int32_t hi, int32_t wi, int32_t ho, int32_t wo, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Host preparation and read-out of the two-model infer.py, which the reference does with OpenCV, torchvision and numpy (infer.py:17-18, 77, 83-91,
 * 113).  One thread per output pixel, a wave on 64 consecutive x of one output row; ho <= 262140, batch <= 65535.
 *   ada_photo_prep_fwd      one uint8 HWC photo -> the two network inputs, both fp32 [3, ho, wo], in ONE pass over the output grid; either may be NULL.
 *     src      uint8 [hi][wi][channels], BGR (3) or BGRA (4: alpha ignored); rows row_pitch_bytes apart (>= wi * channels), as ada_image_prep_fwd.
 *     CHANNEL ORDER: plane c of both outputs is byte c of a source pixel -- B, G, R for a cv2.imread photo.  The reference never converts BGR to RGB on
 *     this path (infer.py:17-18, 83) and feeds B, G, R planes to both networks (the raw model's own infer_image does convert: ada_image_prep_fwd).
 *     raw_out  cv2.resize(img, (wo, ho)) -- INTER_LINEAR on 8-bit pixels -- / 255                                              (infer.py:17-18)
 *              OpenCV's generic 8-bit path (imgproc/src/resize.cpp, HResizeLinear / VResizeLinear<uchar, int, short>), per axis:
 *                scale = 1.0 / ((double)n_out / n_in);  f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s;
 *                s < 0: s = 0, f = 0;  s >= n_in - 1: s = n_in - 1, f = 0;  second tap min(s + 1, n_in - 1);
 *                short coefficients a0 = rint((1.f - f) * 2048.f), a1 = rint(f * 2048.f) (fp32 products, half to even)
 *              horizontal, int32:  h = S[x0] * a0 + S[x1] * a1  on the source rows y0, y1
 *              vertical:           out = ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2)     (255 * 2048 >> 4 = 32640, 32640 * 2048 < 2^31)
 *              Exception, as in OpenCV: wi == 2 wo AND hi == 2 ho is the 2 x 2 area mean (a + b + c + d + 2) >> 2.
 *              The quotient is the correctly rounded fp32 v / 255.f.
 *     near_out torchvision Resize(NEAREST) of photo / 255 (infer.py:83-85) = ATen's nearest rule: scale = (float)n_in / n_out in fp32,
 *              src = min((int)floorf(dst * scale), n_in - 1).
 *   ada_mask_prep_fwd       uint8 masks [K][hi][wi] (rows row_pitch_bytes, masks image_stride_bytes apart; any non-zero value is inside) resized with
 *              the same ATen nearest rule -> out01 fp32 0 / 1 [K, 1, ho, wo] and, optionally, out_pm1 = 2 m - 1, the guide_mask of infer.py:86-91.
 *   ada_nearest_resize_fwd  fp32 [B, hi, wi] -> [B, ho, wo] with cv2.resize(INTER_NEAREST)'s rule (infer.py:77, 113):
 *              sx = min((int)floor(dx * ifx), wi - 1), ifx = 1.0 / ((double)wo / wi) in double; the same for y.
 * ---------------------------------------------------------------------------------------- */
int ada_photo_prep_fwd(const uint8_t* src, int32_t hi, int32_t wi, int32_t channels, int64_t row_pitch_bytes, int32_t ho, int32_t wo,
                       float* raw_out, float* near_out, void* stream);
int ada_mask_prep_fwd(const uint8_t* src, int32_t batch, int32_t hi, int32_t wi, int64_t row_pitch_bytes, int64_t image_stride_bytes,
                      int32_t ho, int32_t wo, float* out01, float* out_pm1, void* stream);
int ada_nearest_resize_fwd(const float* in, int32_t batch, int32_t hi, int32_t wi, int32_t ho, int32_t wo, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The rendering of infer.py:106-119 in ONE pass over the output grid [batch, ho, wo]: min-max normalisation (infer.py:22 / colorize_depth_maps), the
 * colour map, highlight_target (infer.py:46-57), cv2.resize(INTER_NEAREST) to the photo's size and the channel flip.  The library allocates nothing.
 *   depth     fp32 [batch, hi, wi];  mask  fp32 [batch, hi, wi] or NULL (no highlight);  both contiguous
 *   source    output pixel (dy, dx) shows source pixel (sy, sx) by ada_nearest_resize_fwd's rule (the same device function).  Nearest resize is a
 *             pure gather, so rendering the gathered pixel equals the reference's render-then-resize.
 *   normalise t = (d - lo) / span, every operation rounded to fp32 (no FMA, IEEE division), then clipped to [0, 1].
 *             minmax == NULL:  lo is the argument, span = (float)((double)hi_value - (double)lo)
 *             minmax != NULL:  DEVICE fp32 [batch, 2] (what ada_minmax_fwd writes): lo = minmax[b][0], span = minmax[b][1] - minmax[b][0] in fp32
 *             NaN stays NaN (span == 0 on a constant map: 0 / 0), +-inf clips.
 *   colour    idx = min((int)(t * 256.f), 255), rgb = lut[idx]; a NaN t is (0, 0, 0).  lut: DEVICE uint8 [256][3] in R, G, B order, the caller's.
 *             With lut[i] = (cmap(i)[:3] * 255).astype(uint8) this is (cmap(clip(x))[..., :3] * 255).astype(uint8) of a 256-entry matplotlib map, byte for byte.
 *   overlay   mask != NULL and alpha != 0: where the mask is 0 each byte becomes (uint8)((1.0 - alpha) * c + alpha * 200.0), in double, both products
 *             rounded before the sum, the result truncated.  alpha == 0 leaves the bytes alone.  alpha must lie in [0, 1].
 *   outline   mask != NULL: the tree's stand-in draw_mask_outline (src/util/image_util.py), bit for bit -- NOT cv2.findContours / drawContours, which
 *             there is no cv2 here to pin against.  inside = mask > 0;
 *               edge(v, u) = inside(v, u) && !(inside(v-1, u) && inside(v+1, u) && inside(v, u-1) && inside(v, u+1)), neighbours past the image taking the
 *               border pixel's value (a mask that fills the image has no edge);
 *               a pixel is painted outline_rgb (0xRRGGBB) when some in-image (v, u) with |v - sy| + |u - sx| <= thickness - 1 is an edge (the dilation
 *               is zero-padded).  thickness: 1..4 (the reference draws 2), checked whether or not a mask is given.
 *   out       uint8 [batch, ho, wo, 3] packed, R, G, B -- or B, G, R when bgr != 0 (infer.py:115-116); overlay and outline colours are R, G, B before the
 *             flip.  May be NULL.
 *   out_u16   uint16 [batch, ho, wo] = (uint16_t)(t * 65535.f), truncated, NaN -> 0; mask and outline do not apply (the 16-bit save of infer.py:107-108).
 *             May be NULL, but not both.
 * One thread per output pixel, or four with dword stores when wo % 4 == 0 and out / out_u16 are 4- / 8-byte aligned: same bytes either way.
 * ho <= 262140, batch <= 65535.
 * ---------------------------------------------------------------------------------------- */
int ada_depth_render_fwd(const float* depth, int32_t batch, int32_t hi, int32_t wi, const float* minmax, float lo, float hi_value,
                         const uint8_t* lut, const float* mask, int32_t thickness, uint32_t outline_rgb, double alpha,
                         int32_t ho, int32_t wo, int32_t bgr, uint8_t* out, uint16_t* out_u16, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact per-image quantiles, and the two maps that use them.  Additions under ABI 10: no existing signature or struct moves.
 *
 * ada_quantile_fwd replaces np.percentile(value[mask], vminp / vmaxp) of the reference's colorize() (src/scripts/colorize_depth.py:55-56, repeated in
 * four more scripts) and torch.quantile(depth_linear[valid_mask], [q, 1 - q]) of ScaleShiftDepthNormalizer (src/util/depth_transform.py:81-84): exact
 * order statistics of an fp32 map, selected by an 8-bit radix select on the floats' order-preserving keys (csrc/ada_quantile.hip), not sorted, not
 * read back.  The launch sequence (a clear of the workspace, four passes, one finish) depends on (batch, n) alone: capturable.
 *   x          fp32 [batch, n], contiguous; n < 2^31, batch <= 65535
 *   population of image b: the elements with valid[b][e] != 0 (valid: uint8 [batch, n] or NULL = all), with ADA_Q_EXCLUDE_VALUE those != exclude_value
 *              (compared in double, as ada_depth_colorize_fwd compares invalid_val; a NaN is not equal to it), with ADA_Q_POSITIVE_ONLY those > 0 (a NaN is not)
 *   q          HOST double [nq], 1 <= nq <= ADA_QUANTILE_MAX_Q, each in [0, 1] (a percentile p is p / 100.0)
 *   mode       s = the sorted population, cnt its size:
 *     ADA_Q_NUMPY  numpy's 'linear' on the values promoted to double: v = (cnt - 1) * q, j = floor(v), g = v - j, a = s[j], b = s[min(j + 1, cnt - 1)],
 *                  r = a + (b - a) * g, or b - (b - a) * (1 - g) where g >= 0.5; every operation in double, rounded on its own
 *     ADA_Q_TORCH  torch.quantile on an FMA-capable CPU build (every x86-64 with AVX2, every aarch64): r = fp32(q) * fp32(cnt - 1), lo = s[floor(r)], hi = s[ceil(r)], w = r - floor(r), d = hi - lo in fp32;
 *                  lo + w * d where w < 0.5, else hi - d * (1 - w), the product fused into the sum (ATen's lerp is an fmadd), 1 - w rounded on its own.
 *                  ATen's DEFAULT capability on a host without FMA rounds the product first and differs in the last bit in about 3 % of draws
 *   out        double [batch, nq];  out_f32  fp32 [batch, nq] or NULL: the same values rounded -- with nq = 2 the [batch, 2] range that
 *              ada_normalize_fwd, ada_depth_render_fwd (minmax) and ada_range_map_fwd read;  count  int64 [batch] or NULL: the population's size
 *   corners    a NaN inside the population makes every result of that image NaN (both references); an empty population gives NaN and count 0;
 *              -0 and +0 are equal values, which sign comes out is unspecified
 *   workspace  the caller's, 16-byte aligned, batch * ADA_QUANTILE_WS_BYTES_PER_IMAGE bytes; cleared by the call itself
 * Workgroups take ADA_QUANTILE_CHUNK elements of one image.  Only integer atomics: the same bits on every run.
 *
 * ada_range_map_fwd is the scale-and-shift of ScaleShiftDepthNormalizer.__call__ (src/util/depth_transform.py:87-94):
 *   out = ((d - lo) / (hi - lo)) * scale + shift, then with clip != 0 clamped to [clip_lo, clip_hi] (torch.clip: NaN stays NaN); lo = range[b][0],
 *   hi = range[b][1] from a DEVICE fp32 [batch, 2]; fp32 throughout, in this order, every operation rounded (no FMA, IEEE division).  lo == hi gives
 *   what IEEE gives (0 / 0 = NaN, x / 0 = +-inf): the reference does not guard it either.  d, out: fp32 [batch, n].
 *
 * ada_depth_colorize_fwd is colorize() itself (src/scripts/colorize_depth.py:18-84) below its percentiles, on the map promoted to double:
 *   t = (value - vmin) / (vmax - vmin) in double; vmin, vmax = range[b][0], range[b][1] from a DEVICE double [batch, 2] (ada_quantile_fwd's out), or
 *   the two HOST doubles when range == NULL;  t = value * 0 where vmin == vmax
 *   colour = lut[min((int)(t * 256), 255)], t < 0 -> lut[0], t >= 1 -> lut[255], a NaN t -> (0, 0, 0, 0): matplotlib's cmap(t, bytes=True) with
 *   lut = DEVICE uint8 [256][4] R, G, B, A = cmap(arange(256), bytes=True)
 *   invalid pixels get background_rgba (R | G << 8 | B << 16 | A << 24): invalid_mask[b][pixel] != 0 (uint8 [batch, h, w]) when given, else
 *   value == invalid_val, compared in double.  out: uint8 [batch, h, w, 4].
 * ---------------------------------------------------------------------------------------- */
#define ADA_Q_NUMPY 0
#define ADA_Q_TORCH 1
#define ADA_Q_EXCLUDE_VALUE 0x1
#define ADA_Q_POSITIVE_ONLY 0x2
#define ADA_QUANTILE_MAX_Q 4
#define ADA_QUANTILE_CHUNK 4096
#define ADA_QUANTILE_WS_BYTES_PER_IMAGE 33792   /* 4 passes x 8 ranks x 256 bins x 4 bytes + 1 KiB of rank state */
int ada_quantile_fwd(const float* x, const uint8_t* valid, int32_t batch, int64_t n_per_image, const double* q, int32_t nq, int32_t mode,
                     int32_t flags, double exclude_value, double* out, float* out_f32, int64_t* count, void* workspace, int64_t workspace_bytes,
                     void* stream);
int ada_range_map_fwd(const float* d, const float* range, int32_t batch, int64_t n_per_image, float scale, float shift, int32_t clip, float clip_lo,
                      float clip_hi, float* out, void* stream);
int ada_depth_colorize_fwd(const float* value, int32_t batch, int32_t h, int32_t w, const double* range, double vmin, double vmax,
                           const uint8_t* lut, const uint8_t* invalid_mask, double invalid_val, uint32_t background_rgba, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The ADIW pseudo-label generator (reference src/scripts/sam_pl_gen_dav2.py), which prepares every photo and mask with Pillow on the host
 * (Image.open(fp).convert('RGB').resize((518, 518)), lines 28, 93-98) and quantises the label with numpy (lines 115-121).  Additions under ABI 10.
 *   ada_pil_resize_u8_fwd   Pillow's ImagingResample for 8-bit pixels with filter BICUBIC (libImaging/Resample.c), and its NEAREST, byte for byte.
 *     src      uint8 HWC [batch][hi][wi][channels], channels 1 (L) or 3 (RGB); rows row_pitch_bytes apart, images image_stride_bytes apart, as
 *              ada_image_prep_fwd: a crop is read in place.
 *     filter   ADA_PIL_BICUBIC: per resized axis the caller passes DEVICE int32 tables, bounds [n_out][2] = (xmin, n) and kk [n_out][ksize], computed
 *              on the host in double (hip_ext/labels.py pil_coeffs) by Pillow's precompute_coeffs / normalize_coeffs_8bpc:
 *                scale = n_in / n_out;  fs = max(scale, 1.0);  support = 2.0 * fs;  ksize = (int)ceil(support) * 2 + 1;  ss = 1.0 / fs
 *                center = (xx + 0.5) * scale;  xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), n_in);  n = xmax - xmin
 *                w[x] = f((x + xmin - center + 0.5) * ss), x < n;  f(t) with a = -0.5:  |t| < 1: ((a + 2) t - (a + 3)) t t + 1;  |t| < 2: (((t - 5) t + 8) t - 4) a;  else 0
 *                the weights are divided by their sum (accumulated in index order; not when it is 0), then quantised as (int)(w * 2^22 + 0.5), or - 0.5
 *                for a negative w; entries past n are 0.  The support grows with the down-scale factor: 19 taps per axis for 2250 -> 518.
 *              The horizontal pass runs first, into the uint8 intermediate tmp [batch][hi][wo][channels] (the caller's workspace, tmp_bytes checked;
 *              needed only when both axes are resized), then the vertical pass.  Each pass:  acc = 2^21 + sum k[x] * pixel[xmin + x]  in int32 (Pillow's
 *              int), out = clamp(acc >> 22, 0, 255), the shift arithmetic (a negative sum clamps to 0).  The intermediate is ROUNDED TO uint8 between
 *              the passes, as Pillow rounds it: the passes are not fused at higher precision.  A pass whose n_in == n_out is skipped, as Pillow skips
 *              it (its tables may be NULL); with both skipped the pixels are copied.  The kernels clamp (xmin, n) to the axis.
 *              ADA_PIL_NEAREST (no tables, no tmp): per axis  src = min((int)floor((dst + 0.5) * ((double)n_in / n_out)), n_in - 1)  in double.
 *     outputs  any non-empty subset, none aliasing src:
 *                out_u8    HWC [batch][ho][wo][channels]: Pillow's bytes
 *                out_f32   planar [batch, channels, ho, wo]: v / 255.f, IEEE division = (float)((double)v / 255.0) for all 256 values -- np.array(im) / 255
 *                          cast to float32 (line 29-31).  Channel order kept: R, G, B planes for a convert('RGB') photo.
 *                out_mask  uint8 [batch][ho][wo] = v > 0 (lines 94, 98), channels == 1 only
 *   ada_label_combine_fwd   lines 115-117 and 121 in one launch.  whole, occ: fp32 [P, h, w], already min-max normalised; whole_mask: uint8 [P, h, w],
 *              non-zero = inside; scale_shift: DEVICE fp32 [P, 2].  No output may alias an input.
 *                v = whole_mask ? (whole * scale) + shift : occ   in fp32, the product rounded before the sum (no FMA), as in ada_blend_ex
 *                t = v * 65535.f
 *                ADA_LABEL_WRAP  numpy's astype(np.uint16) on x86-64, the reference's cast: NaN or |t| >= 2^31 gives 0, otherwise the low 16 bits of
 *                                (int32)trunc(t):  -3.7 -> 65533, 65536.0 -> 0, 65537.9 -> 1, 70000.5 -> 4464, NaN -> 0, 1e10 -> 0.  (The hardware's
 *                                conversion saturates; the rule is written out.)
 *                ADA_LABEL_CLIP  trunc after clamping t to [0, 65535]; NaN gives 0.
 *     out_u16       uint16 [P, ho, wo]: output pixel (dy, dx) shows source pixel (sy, sx) by the NEAREST rule above.  Nearest is a pure gather, so this is
 *                   the reference's quantise-then-resize.  NEAREST is what Image.fromarray(u16).resize((512, 512)) does under the reference's pinned
 *                   Pillow 10.0.1 (environment.yaml:227: modes with ';' default to NEAREST); Pillow 12 defaults to BICUBIC for "I;16".
 *     out_f32       optional fp32 [P, h, w]: v, the combined map before quantising
 *     out_of_range  optional int32 [P, ho] (overwritten): per label row, the gathered pixels with t outside [0, 65536) or NaN.  One wave owns a row and adds
 *                   its ballots in order; the caller sums the rows.  No atomics.
 * hi, ho <= 262140 (resize), batch / P <= 65535.
 * ---------------------------------------------------------------------------------------- */
#define ADA_PIL_NEAREST 0     /* Pillow's Image.NEAREST */
#define ADA_PIL_BICUBIC 3     /* Pillow's Image.BICUBIC */
#define ADA_LABEL_WRAP 0
#define ADA_LABEL_CLIP 1
int ada_pil_resize_u8_fwd(const uint8_t* src, int32_t batch, int32_t hi, int32_t wi, int32_t channels, int64_t row_pitch_bytes,
                          int64_t image_stride_bytes, int32_t ho, int32_t wo, int32_t filter, const int32_t* bounds_x, const int32_t* kk_x,
                          int32_t ksize_x, const int32_t* bounds_y, const int32_t* kk_y, int32_t ksize_y, uint8_t* tmp, int64_t tmp_bytes,
                          uint8_t* out_u8, float* out_f32, uint8_t* out_mask, void* stream);
int ada_label_combine_fwd(const float* whole, const float* occ, const uint8_t* whole_mask, const float* scale_shift, int32_t batch, int32_t h,
                          int32_t w, int32_t ho, int32_t wo, int32_t overflow, uint16_t* out_u16, float* out_f32, int32_t* out_of_range,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * The demo's mask front-end (reference app.py): connected components of a mask on the device, their statistics, the area filter of remove_small_noise
 * (app.py:283-293) and the prompt-point grid of get_points_from_components (app.py:77-99), which the reference does on the host with
 * cv2.connectedComponents / connectedComponentsWithStats.  Additions under ABI 10.  Integer arithmetic only: every result is exact and bit-reproducible.
 * The launch sequence of each call depends on the shapes alone (no host read, no flag loop, no cooperative launch): all four are legal inside a stream
 * capture.  The library allocates nothing.  h * w < 2^31, batch <= 65535, h and w down to 1.
 *   ada_mask_label_fwd       mask uint8 [batch][h][w], rows row_pitch_bytes apart (>= w), images image_stride_bytes apart, as ada_mask_prep_fwd: a crop is
 *     read in place; any non-zero byte is inside.  connectivity: 4 or 8 (anything else: ADA_EINVAL).
 *     labels     int32 [batch][h][w] packed: 0 = background, components numbered 1 .. n IN THE RASTER ORDER OF EACH COMPONENT'S FIRST PIXEL (row-major).
 *                That is scipy.ndimage.label's numbering.  OpenCV's documentation does not specify the numbering of connectedComponents, so nothing
 *                here claims label-for-label equality with cv2 -- only the same partition; what the reference derives from the labels (the kept
 *                pixels, the list of points up to the order of the components) depends on the partition alone.
 *     n_labels   int32 [batch] on the device: n per image
 *     workspace  the caller's, workspace_bytes >= 4 * batch * (2 * h * w + ceil(h * w / 1024)) (checked)
 *     Algorithm: a union-find over pixel indices whose links always point to a smaller-or-equal index (union by integer atomic min), so every pointer
 *     chase strictly decreases, every failed retry means some link decreased, no workgroup ever waits for another, and a component's root is its first
 *     raster pixel: the numbering is a prefix count over root flags.  32 x 32 tiles in LDS, one pass over the tile borders, resolve, count, number,
 *     paint: six launches (csrc/ada_masks.hip).
 *   ada_mask_stats_fwd       from a label map and a capacity max_labels >= 0:
 *     stats      int32 [batch][max_labels + 1][5] in cv2's column order (CC_STAT_LEFT, TOP, WIDTH, HEIGHT, AREA)
 *     sums       int64 [batch][max_labels + 1][2] = (sum of x, sum of y) over the component's pixels; centroid = sums / area, cv2's (x, y) order
 *     Row 0 is the background, as in connectedComponentsWithStats.  A row without pixels -- an empty background included -- is all zeros (this
 *     library's definition; cv2's row for an empty background is not pinned).  Pixels whose label exceeds max_labels (or is negative) are ignored: the
 *     caller detects the overflow from n_labels.  Runs of equal labels along a row are summed in registers and flushed with one set of integer atomics.
 *   ada_mask_keep_area_fwd   from a label map: keep = label != 0 && area(label) >= min_area (remove_small_noise's rule), exact for any number of components.
 *     out_u8     uint8 0 / 1 [batch][h][w], out_f32 fp32 0 / 1 [batch][h][w]: either may be NULL, not both
 *     workspace  the per-label areas, workspace_bytes >= 4 * batch * (h * w / 2 + 2) (checked): a grid of h x w pixels holds at most ceil(h * w / 2)
 *                components under either connectivity.  No capacity argument, no host read.
 *   ada_mask_grid_points_fwd from a label map and ada_mask_stats_fwd's stats (same max_labels):
 *     hit        int32 [batch][h][w] = label where area(label) >= small_component_thresh && (y - top) % grid_step == 0 && y < top + height - 1
 *                && (x - left) % grid_step == 0 && x < left + width - 1, else 0.  This is range(min_y, max_y, grid_step) x range(min_x, max_x, grid_step) of
 *                app.py:94-97, which EXCLUDES the last row and column of the bounding box: a large component one pixel wide yields no point.  grid_step >= 1.
 * ---------------------------------------------------------------------------------------- */
int ada_mask_label_fwd(const uint8_t* mask, int32_t batch, int32_t h, int32_t w, int64_t row_pitch_bytes, int64_t image_stride_bytes,
                       int32_t connectivity, int32_t* labels, int32_t* n_labels, void* workspace, int64_t workspace_bytes, void* stream);
int ada_mask_stats_fwd(const int32_t* labels, int32_t batch, int32_t h, int32_t w, int32_t max_labels, int32_t* stats, int64_t* sums, void* stream);
int ada_mask_keep_area_fwd(const int32_t* labels, int32_t batch, int32_t h, int32_t w, int32_t min_area, uint8_t* out_u8, float* out_f32,
                           void* workspace, int64_t workspace_bytes, void* stream);
int ada_mask_grid_points_fwd(const int32_t* labels, const int32_t* stats, int32_t batch, int32_t h, int32_t w, int32_t max_labels,
                             int32_t small_component_thresh, int32_t grid_step, int32_t* hit, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depth maps to geometry (reference src/models/amodalsynthdrive/zoedepth/utils/geometry.py, numpy on the host): the unprojection of depth_to_points,
 * the masked triangle list of create_triangles and a compaction of the vertices a triangle list uses.  Additions under ABI 10.  The launch sequence of
 * each call depends on the shapes alone (no host read, no flag loop, no cooperative launch, no workgroup waits for another): all three are legal inside
 * a stream capture.  The library allocates nothing.  Integer outputs are the same bits every run: no atomic decides a position.  h * w < 2^30,
 * batch <= 65535, h and w down to 1; anything else is ADA_EINVAL.
 *   The depth value z of a pixel, one rule for all three calls:  inverse == 0: z = (double)depth;  inverse == 1: z = 1 / (a * (double)depth + b), the
 *   product, the sum and the quotient each rounded once (a, b host doubles).  A vertex is VALID when z is finite and z > 0.
 *   ada_depth_points_fwd     depth fp32 [batch][h][w] packed.  camera: 21 HOST doubles, read before the call returns: Kinv[9] row-major (the inverse of
 *     the intrinsics, computed by the caller), R[9] row-major, t[3].  For the pixel in column x, row y, all in fp64, every product and sum rounded once
 *     and no FMA:
 *       p_i = ((z Kinv[i,0]) x + (z Kinv[i,1]) y) + (z Kinv[i,2])          q = (-p_0, -p_1, p_2)
 *       r_i = ((R[i,0] q_0 + R[i,1] q_1) + R[i,2] q_2) + t_i
 *     With R = I, t = 0 and a Kinv that has a zero in every row (any pinhole camera without skew) this is the reference's float64 result bit for bit;
 *     for a general pose it differs from numpy's stacked matmul by at most 2 gamma_4 (sum_j |R_ij| |q_j| + |t_i|), gamma_4 = 4u / (1 - 4u), u = 2^-53.
 *     A vertex whose z is not finite gets NaN in all three coordinates (the reference's inf * 0); a finite z <= 0 is unprojected as computed.
 *     out_f64  fp64 [batch][h][w][3], out_f32  fp32 [batch][h][w][3] = the fp64 result rounded once to nearest: either may be NULL, not both; 16-byte aligned
 *     valid    optional uint8 [batch][h][w]: 1 for a valid vertex, else 0
 *   ada_mesh_triangles_fwd   the candidates are create_triangles's, in its order: cells in raster order, each as (tl, bl, tr) then (br, tr, bl), vertex
 *     index = y * w + x.  A candidate is kept when each of its three vertices is inside the mask (mask NULL: every vertex is), is valid (depth NULL:
 *     every vertex is) and, with max_ratio > 0 (needs depth), z_max <= max_ratio * z_min over the three, the product one rounded fp64 multiply.
 *     mask       optional uint8 [batch][h][w], rows row_pitch_bytes apart (>= w), images image_stride_bytes apart, as ada_mask_label_fwd: a crop is
 *                read in place; any non-zero byte is inside
 *     depth      optional fp32 [batch][h][w] packed, with the z rule above
 *     triangles  int32 [batch][capacity][3]: the first min(count, capacity) kept triangles of each image; rows from count on are untouched
 *     count      int32 [batch] on the device: the true number, also when it exceeds capacity
 *     workspace  the caller's, workspace_bytes >= 4 * batch * max(1, ceil((h - 1) (w - 1) / ADA_GEOM_CHUNK)) (checked)
 *     h == 1 or w == 1: count = 0 (the reference returns an empty list without a mask and raises with one).
 *     Count, scan, scatter: three launches (csrc/ada_geometry.hip); the predicate is one device function used by the first and the third.
 *   ada_mesh_compact_fwd     from a triangle list [batch][capacity][3] with its count, and points [batch][h * w][3] of point_bytes 4 (fp32) or 8 (fp64):
 *     the vertices referenced by at least one of the first min(count, capacity) triangles, numbered 0 .. n - 1 in raster order.
 *     vertex_count  int32 [batch]: n, also when it exceeds vertex_capacity
 *     points_out    [batch][vertex_capacity][3], same type as points: vertex k of the new numbering, for k < min(n, vertex_capacity); rows from n on untouched
 *     colors / colors_out  optional uint8 [batch][h * w][3] -> [batch][vertex_capacity][3], gathered the same way (both or neither)
 *     triangles     rewritten in place to the new numbering (an index outside 0 .. h * w - 1 is left as it is)
 *     workspace     the caller's, workspace_bytes >= 4 * batch * (h * w + ceil(h * w / ADA_GEOM_CHUNK)) (checked)
 *     Clear, mark, count, scan, gather, remap: six launches.
 * ---------------------------------------------------------------------------------------- */
#define ADA_GEOM_WAVE 64            /* candidates per ballot */
#define ADA_GEOM_CHUNK 1024         /* cells / vertices per workgroup of the count and scatter passes */
#define ADA_GEOM_SCAN_BLOCK 1024    /* workgroup sums per step of the per-image scan */
int ada_depth_points_fwd(const float* depth, int32_t batch, int32_t h, int32_t w, const double* camera, int32_t inverse, double a, double b,
                         double* out_f64, float* out_f32, uint8_t* valid, void* stream);
int ada_mesh_triangles_fwd(const uint8_t* mask, int64_t row_pitch_bytes, int64_t image_stride_bytes, const float* depth, int32_t inverse, double a,
                           double b, double max_ratio, int32_t batch, int32_t h, int32_t w, int32_t* triangles, int32_t capacity, int32_t* count,
                           void* workspace, int64_t workspace_bytes, void* stream);
int ada_mesh_compact_fwd(int32_t* triangles, const int32_t* count, int32_t capacity, int32_t batch, int32_t h, int32_t w, const void* points,
                         int32_t point_bytes, const uint8_t* colors, void* points_out, uint8_t* colors_out, int32_t vertex_capacity,
                         int32_t* vertex_count, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Meshes seen from a camera: a z-buffer rasteriser for the meshes above (csrc/ada_raster.hip).  The reference hands its meshes to a third-party
 * renderer, so this arithmetic is the library's own; tests/_raster_ref.py restates it in numpy and the GPU suite compares bit for bit.  Additions under
 * ABI 10.  Neither call allocates or reads anything back; the launch sequence depends on the shapes alone: legal inside a stream capture.  The file is
 * built without floating-point contraction; "rounded" below means every product, sum and quotient is an IEEE fp64 operation of its own.
 *   ada_mesh_project_fwd     the vertex stage.  points [n_vertices][3] of point_bytes 4 (fp32, widened exactly) or 8 (fp64), in the reference's point
 *     convention (what ada_depth_points_fwd writes).  camera: 16 HOST doubles, read before the call returns: fx, fy, cx, cy, R[9] row-major, t[3].
 *       pose == 1:  q_i = ((R[i,0] p_x + R[i,1] p_y) + R[i,2] p_z) + t_i        pose == 0:  q = p exactly (R, t ignored)
 *       u = fx ((-q_x) / q_z) + cx     v = fy ((-q_y) / q_z) + cy               samples sit at integers: pixel (row i, column j) is (u, v) = (j, i)
 *     A vertex is VALID when q is finite, 2^-64 <= q_z <= 2^64 and |u|, |v| <= 16384 (the guard band).
 *     x, y   int32 [n_vertices]: rint(256 u), rint(256 v), round half to even; 0 for an invalid vertex
 *     w      fp64 [n_vertices]: 1 / q_z; 0 for an invalid vertex -- w == 0 IS the validity flag ada_mesh_raster_fwd reads
 *   ada_mesh_raster_fwd      clear, bin, walk, resolve: four launches.  triangles int32 [n_triangles][3] index the vertex records; a triangle is
 *     dropped when an index is outside [0, n_vertices), a vertex is invalid, or A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) is 0.  No clipping, no culling.
 *     At the sample (Sx, Sy) = (256 j, 256 i), in int64 (the guard band keeps every product below 2^47):
 *       e0 = (X2 - X1)(Sy - Y1) - (Y2 - Y1)(Sx - X1)    e1 = (X0 - X2)(Sy - Y2) - (Y0 - Y2)(Sx - X2)    e2 = A - e0 - e1;   A < 0: all four negated
 *     covered iff e0, e1, e2 >= 0 (edges inclusive).  w = w0 + ((double(e1) (w1 - w0) + double(e2) (w2 - w0)) / double(A)), rounded.
 *     The winner of a sample is the covering triangle with the largest float32(w) (round to nearest even), ties to the LOWEST triangle index: one
 *     64-bit unsigned atomic maximum of bits(float32(w)) << 32 | (0xFFFFFFFF - id).  Independent of arrival order: the same bytes every run.
 *     index   int32 [height][width]: the winner, -1 where nothing covers the sample
 *     depth   fp32 [height][width], from the winner's fp64 w rounded once: ADA_RASTER_OUT_W w; ADA_RASTER_OUT_Z 1 / w; ADA_RASTER_OUT_NORMALISED
 *             (w - b) / a (a != 0), the inverse of the z rule above; `fill` where index is -1
 *     colors / color  optional uint8 [n_vertices][3] -> [height][width][3], perspective-correct: n_i = double(e_i) w_i, den = (n0 + n1) + n2,
 *             channel = ((n0 c0 + n1 c1) + n2 c2) / den, out = min(255, floor(channel + 0.5)); fill_rgb (r | g << 8 | b << 16) where index is -1
 *     Work: a triangle whose screen-clipped box holds <= ADA_RASTER_SMALL_MAX samples is walked by its own thread; one of <= ADA_RASTER_WAVE_MAX by
 *     one wave in tiles of 8 x 8 samples; a larger one by a team of at least ADA_RASTER_WALK_SHARE of the walking launch's ADA_RASTER_WALK_BLOCKS
 *     workgroups in tiles of ADA_RASTER_TILE_W x ADA_RASTER_TILE_H; a tile with one edge function negative at its four corners is skipped.  The two
 *     lists are filled by one ballot per wave and one counter add; their order cannot reach the output.
 *     workspace  the caller's, 16-byte aligned, workspace_bytes >= 8 * (height * width rounded up to even) + 16 + 4 * n_triangles (checked)
 *     height * width < 2^30; n_triangles == 0 (and n_vertices == 0) is legal and gives the fills.
 * ---------------------------------------------------------------------------------------- */
#define ADA_RASTER_SMALL_MAX 16       /* samples in a box that the triangle's own thread walks */
#define ADA_RASTER_WAVE_MAX 4096      /* samples in a box that one wave walks */
#define ADA_RASTER_TILE_W 32          /* a workgroup's tile of a larger box */
#define ADA_RASTER_TILE_H 8
#define ADA_RASTER_WALK_BLOCKS 2048   /* workgroups of the walking launch */
#define ADA_RASTER_WALK_SHARE 16      /* workgroups that share one of the larger boxes, at least */
#define ADA_RASTER_OUT_W 0
#define ADA_RASTER_OUT_Z 1
#define ADA_RASTER_OUT_NORMALISED 2
int ada_mesh_project_fwd(const void* points, int32_t point_bytes, int32_t n_vertices, const double* camera, int32_t pose, int32_t* x, int32_t* y,
                         double* w, void* stream);
int ada_mesh_raster_fwd(const int32_t* x, const int32_t* y, const double* w, const uint8_t* colors, int32_t n_vertices, const int32_t* triangles,
                        int32_t n_triangles, int32_t height, int32_t width, int32_t mode, double a, double b, float fill, uint32_t fill_rgb,
                        float* depth, int32_t* index, uint8_t* color, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adaptive depth-map meshes: an error-bounded right-triangulated irregular network (RTIN: the binary tree of right isosceles triangles of
 * Lindstrom's and "martini"-style terrain meshes) in place of ada_mesh_triangles_fwd's two triangles per cell (csrc/ada_adaptive.hip).  The reference
 * has no such mesh: the arithmetic is the library's own, tests/_adaptive_ref.py restates it in numpy and the GPU suite compares bit for bit.  Additions
 * under ABI 10.  The mesh is conforming by construction (no T-junction, no crack, no skirt).  The launch sequence depends on the shapes and the flags
 * alone, nothing is read back or allocated: legal inside a stream capture.  The file is built without floating-point contraction.
 *   GRID.  A map of h x w vertices, h, w >= 2.  N is the smallest power of two with N >= max(h, w) - 1 (N <= ADA_ADAPT_MAX_N, else ADA_EUNSUPPORTED);
 *     the virtual grid is (N + 1) x (N + 1).  A vertex (i, j) = (row, column) with i >= h or j >= w is ABSENT.  A vertex's id in the output is i w + j,
 *     the ids of ada_mesh_triangles_fwd: ada_mesh_compact_fwd works on the result unchanged.
 *   TREE.  A triangle is (a, b, c), right angle at c, hypotenuse a b, m = (a + b) / 2.  Roots ((N, N), (0, 0), (N, 0)) then ((0, 0), (N, N), (0, N)).
 *     Children of (a, b, c): left (c, a, m), right (b, c, m); they keep the parent's winding, which with these roots is that of ada_mesh_triangles_fwd's
 *     (tl, bl, tr).  Heap index: roots 2 and 3, children 2 t and 2 t + 1.  Level 0 holds the roots; the leaves (legs of length 1) are level
 *     2 log2 N: 2 log2 N + 1 levels, 2 N^2 leaves.
 *   DISPARITY.  omega(v), fp64: inverse == 1: a * (double)depth + b, the product and the sum rounded once each (what ada_depth_points_fwd forms before
 *     its reciprocal); inverse == 0: 1.0 / (double)depth.  The error is measured on omega, not on z: a plane in space is linear in omega over the
 *     pixel grid, omega is what ada_mesh_raster_fwd interpolates, and with inverse == 1 it is linear in the network's output.
 *   KEEPABLE LEAF.  Its three vertices are present and pass the tests ada_mesh_triangles_fwd applies to a candidate's three vertices: inside the mask,
 *     valid (z finite and > 0, the z rule above), and with max_ratio > 0 z_max <= max_ratio * z_min.
 *   ERROR MAP.  E, fp64 per vertex, initially 0.  Triangles bottom-up by level; for a non-leaf T
 *       F(T) = +inf                                          if T's children are leaves and one of them is not keepable
 *       F(T) = max(|0.5 (omega_a + omega_b) - omega_m| / omega_m,   the sum, the product, the difference and the quotient each rounded once
 *                  E[m(left child)], E[m(right child)])             (the last two only when the children are not leaves)
 *       E[m(T)] = max(E[m(T)], F(T))
 *     over the up to two triangles that share m as hypotenuse midpoint: both sides of a hypotenuse split together.  +inf travels upwards through the
 *     child terms; the quotient is evaluated only where the child terms are finite (every vertex of T is then valid and omega_m finite and positive),
 *     so E holds no NaN.  E is monotone along the tree.  A triangle that touches an absent vertex has F = +inf.
 *   EMISSION for the tolerance tau = max_error (finite, >= 0).  A non-leaf T is a row iff (T is a root or E[m(parent)] > tau) and E[m(T)] <= tau.
 *     A leaf is a row iff (it is a root or E[m(parent)] > tau) and it is keepable.  no_max_error == 1: every keepable leaf (2 (h - 1) (w - 1) rows
 *     without a mask on a valid map).  A plane on a (2^k + 1)^2 map is 2 rows; a map whose sides are not 2^k + 1 refines along the image border
 *     because the absent vertices force it (a 12 x 19 plane: 82 rows) -- the price of one conforming root square.
 *   ORDER.  Ascending heap index; a row is (id(a), id(b), id(c)), int32.
 *   ada_mesh_adaptive_workspace_bytes   *bytes = what ada_mesh_adaptive_fwd asks for an h x w map (any batch: images run one after the other)
 *   ada_mesh_adaptive_fwd
 *     mask       optional uint8 [batch][h][w], rows row_pitch_bytes apart, images image_stride_bytes apart, as ada_mesh_triangles_fwd
 *     depth      fp32 [batch][h][w] packed
 *     triangles  int32 [batch][capacity][3]: the first min(count, capacity) rows of each image; rows from count on are untouched
 *     count      int32 [batch] on the device: the true number, also when it exceeds capacity (the overflow signal)
 *     error_out  optional fp64 [batch][h][w]: receives E.  error_ready == 1: it HOLDS E already, from an earlier call with the same depth, mask, inverse
 *                rule and max_ratio, and the error phase is skipped -- for callers who sweep the tolerance or size the output from a first count
 *     workspace  the caller's, 16-byte aligned, workspace_bytes >= ada_mesh_adaptive_workspace_bytes (checked)
 *     Work: E by a gather per midpoint vertex (each vertex is the midpoint of one level only), one launch per level while the level holds more than
 *     ADA_ADAPT_FOLD midpoints inside the image, the coarser levels in one workgroup; emission by one predicate and a count / scan / write
 *     compaction in heap order over the subtrees below the cells of ADA_ADAPT_CELL vertices' width that overlap the image, the levels above them
 *     walked by one workgroup.  No subtree wholly outside the image is launched over.  E is monotone along the tree, so a subtree whose root's
 *     parent is not split has no row and is left at once.  No atomic decides a position or a value (the one LDS add is an integer count): the same
 *     bytes every run.
 * ---------------------------------------------------------------------------------------- */
#define ADA_ADAPT_FOLD 1024           /* midpoints of a level at or below which the remaining levels run in one workgroup */
#define ADA_ADAPT_CELL 32             /* width of the cells whose two halves are the subtrees of the emission's workgroups */
#define ADA_ADAPT_MAX_N 16384         /* largest side of the virtual grid */
int ada_mesh_adaptive_workspace_bytes(int32_t h, int32_t w, int64_t* bytes);
int ada_mesh_adaptive_fwd(const uint8_t* mask, int64_t row_pitch_bytes, int64_t image_stride_bytes, const float* depth, int32_t inverse, double a,
                          double b, double max_ratio, double max_error, int32_t no_max_error, int32_t batch, int32_t h, int32_t w,
                          int32_t* triangles, int32_t capacity, int32_t* count, double* error_out, int32_t error_ready, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The edge metrics of the reference's evaluation (reference src/util/metric.py:181-328), which the reference computes on the host with
 * skimage.feature.canny and scipy.ndimage.distance_transform_edt after copying two full-size maps per sample.  Additions under ABI 10.  All maps are
 * packed [batch][h][w]; h * w < 2^31, batch <= 65535, h and w down to 1.  No atomics of their own (ada_canny_hysteresis_fwd runs ada_mask_label_fwd, whose
 * integer atomic-min union-find gives exact, reproducible labels), no host read, nothing allocated: every launch sequence depends on the shapes alone.  The arithmetic contract -- what is rounded where -- is DESIGN.md's "Edge metrics" section; csrc/ada_edges.hip is built without
 * floating-point contraction.
 *   ada_canny_fwd            replaces canny(depth, sigma=sigma, mask=None) of extract_edges (metric.py:215) up to the suppressed magnitude, on a FLOAT32
 *     image with mode 'constant', together with the pre-processing of metric.py:198-210:
 *     pre        0 identity; 1 to_log (metric.py:169-173): (d > 0) * log(max(d, eps32)); 2 extract_edges' default branch (metric.py:206-210):
 *                log((d > 0) * max(d, eps32)) / log(1.5), an fp32 division, -inf where d <= 0.  The logarithm is evaluated in fp64 and rounded once.
 *     weights    DEVICE fp64 [2 radius + 1], computed by the host as scipy's _gaussian_kernel1d does; radius = int(4 sigma + 0.5) <= ADA_CANNY_MAX_RADIUS
 *     Stages, each stored in fp32: Gaussian along axis 0 then axis 1 (zero outside the image; fp64 accumulation in scipy's symmetric order: centre tap,
 *     then (in[i - k] + in[i + k]) * w[k] from k = radius down to 1); division by (the same two passes over a map of ones, computed from the
 *     coordinates) + eps32; ndi.sobel along each axis with mode 'reflect' ([-1, 0, 1] along the axis, [1, 2, 1] along the other, fp64 accumulation);
 *     magnitude = sqrt(isobel * isobel + jsobel * jsobel) in three fp32 operations; skimage's bilinear non-maximum suppression: off the one-pixel
 *     border ring, magnitude >= low_threshold, weight and interpolation in fp64, kept when both interpolated neighbours are <= the magnitude.
 *     low_masked fp32: the kept magnitudes, 0 elsewhere.  pre_out / smoothed / isobel / jsobel / magnitude: optional fp32 stage maps (NULL: not written).
 *     One workgroup per 32 x 32 tile, halo radius + 2 in LDS: the image is read once.
 *   ada_canny_hysteresis_fwd replaces canny's double thresholding (ndi.label(low_mask, ones((3, 3))) and good_label[labels]): edges uint8 0 / 1 =
 *     pixels of the 8-connected components of low_masked > 0 that hold a pixel with low_masked >= high_threshold.  Labels come from
 *     ada_mask_label_fwd; a per-label byte is set by plain stores of one value, then gathered.
 *     workspace  workspace_bytes >= 4 batch h w + 4 batch + [ada_mask_label_fwd's] + batch * ceil4(h w / 2 + 2) + ceil4(batch h w)  (checked)
 *   ada_edt_fwd              replaces ndimage.distance_transform_edt(np.logical_not(edges)) (metric.py:242, 245): out fp64 = the Euclidean distance
 *     to the nearest non-zero pixel of edges (uint8), 0 on them.  Squared distances are exact integers (h, w <= 32767, else ADA_EUNSUPPORTED): a column
 *     pass (two scans), a row pass min over x' of (x - x')^2 + g(x')^2 with the row staged through LDS in chunks, one fp64 square root.  An image
 *     WITHOUT any edge pixel gives +inf everywhere; scipy's output for that input is an artefact of its implementation, not a documented value.
 *     workspace  workspace_bytes >= 4 batch h w  (checked)
 *   ada_edge_metric_fwd      the sums behind EdgeAcc / EdgeComp (metric.py:247-256): sums fp64 [batch][4] =
 *     ADA_EDGE_N_BDE, ADA_EDGE_SUM_DT  count and sum of d_target over pred_edges && valid && d_target < th_acc
 *     ADA_EDGE_N_GT,  ADA_EDGE_SUM_DP  count and sum of d_pred over gt_edges && valid
 *     valid      optional uint8 (NULL: every pixel).  workspace_bytes >= 8 * batch * ADA_EDGE_SUM_BLOCKS * 4  (checked)
 *   ada_soft_edge_fwd        the sums behind soft_edge_error (metric.py:317-328): sums fp64 [batch][2] = the number of valid pixels and the sum over
 *     them of min over the (2 radius + 1)^2 shifts of |shift(gt) - pred|, the shifted map 0 where it came from outside (shift_2d_replace with
 *     constant 0); difference and absolute value in fp32.  0 <= radius <= ADA_SOFT_EDGE_MAX_RADIUS.
 *     workspace_bytes >= 8 * batch * ADA_EDGE_SUM_BLOCKS * 2  (checked)
 *   Both reductions run in a fixed order (per-thread strided sums, a shuffle tree, ADA_EDGE_SUM_BLOCKS partial rows per image, one tree): the same bits
 *   every run.
 * ---------------------------------------------------------------------------------------- */
#define ADA_CANNY_MAX_RADIUS 16       /* sigma <= 4 */
#define ADA_SOFT_EDGE_MAX_RADIUS 8
#define ADA_EDGE_SUM_BLOCKS 256       /* partial rows per image of the two reductions */
#define ADA_EDGE_N_BDE 0
#define ADA_EDGE_SUM_DT 1
#define ADA_EDGE_N_GT 2
#define ADA_EDGE_SUM_DP 3
int ada_canny_fwd(const float* image, int32_t batch, int32_t h, int32_t w, int32_t pre, const double* weights, int32_t radius,
                  float low_threshold, float* low_masked, float* pre_out, float* smoothed, float* isobel, float* jsobel, float* magnitude,
                  void* stream);
int ada_canny_hysteresis_fwd(const float* low_masked, int32_t batch, int32_t h, int32_t w, float high_threshold, uint8_t* edges, void* workspace,
                             int64_t workspace_bytes, void* stream);
int ada_edt_fwd(const uint8_t* edges, int32_t batch, int32_t h, int32_t w, double* out, void* workspace, int64_t workspace_bytes, void* stream);
int ada_edge_metric_fwd(const uint8_t* pred_edges, const uint8_t* gt_edges, const uint8_t* valid, const double* d_target, const double* d_pred,
                        int32_t batch, int32_t h, int32_t w, double th_acc, double* sums, void* workspace, int64_t workspace_bytes, void* stream);
int ada_soft_edge_fwd(const float* pred, const float* gt, const uint8_t* valid, int32_t batch, int32_t h, int32_t w, int32_t radius, double* sums,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rank filters: the windowed order statistic of the VALID samples (additions under ABI 10).  Median, minimum (erosion) and maximum (dilation) are ranks of it;
 * opening and closing are compositions (hip_ext/masks.py).  The reference has no such operation on the device or off it: its median_filter_blend
 * (app.py:267, infer.py:30) runs cv2.blur, and its mask clean-up (app.py:207-211: cv2.erode, MORPH_CLOSE) runs on the host.
 *   INPUT.  x: fp32 (dtype ADA_DT_F32) or uint8 (ADA_DT_U8), packed [batch][h][w].  valid: optional uint8 of that shape, non-zero = the sample
 *     votes (NULL: every sample).  The window is kh x kw, both odd, radii rh = kh / 2 and rw = kw / 2.  h * w < 2^31, batch <= 65535, h and w down to 1.
 *   SAMPLES of output pixel (y, x): the positions (y + dy, x + dx), |dy| <= rh, |dx| <= rw, each axis mapped by the border rule
 *     ADA_BORDER_MIRROR   reflect-101: period 2 n - 2, the index reduced modulo the period, so a window wider than the image is legal; n == 1: index 0
 *                         (scipy's 'mirror', cv2's BORDER_REFLECT_101)
 *     ADA_BORDER_NEAREST  clamped into the image (scipy's 'nearest', cv2's BORDER_REPLICATE)
 *     ADA_BORDER_IGNORE   positions outside the image are dropped
 *     A mapped position contributes when valid is absent or non-zero there and, for fp32, the value is not NaN.  Mirrored or clamped duplicates count
 *     once each: the samples are a multiset of n values.
 *   RESULT.  n == 0: out = fill (converted to x's type; for uint8 an integer in 0 .. 255) and count = 0.  Otherwise the samples sorted ascending by IEEE
 *     comparison (+-inf order as numbers; -0 and +0 are equal and either may come out), s[0 .. n - 1], and out = s[r] with
 *     ADA_RANK_MIN     r = 0
 *     ADA_RANK_MAX     r = n - 1
 *     ADA_RANK_MEDIAN  r = n / 2              scipy's upper median: scipy.ndimage.median_filter when every sample votes
 *     0 <= rank <= 100 r = rank (n - 1) / 100 an integer percent; the quotient in integers, rounded down
 *     out is always one of the input values: no arithmetic touches a value.  count: optional int32 [batch][h][w] (NULL: not written), receives n.
 *   ada_rank_filter_fwd      any rank; kh * kw <= ADA_FILTER_MAX_WINDOW (9 x 9, 3 x 27, ...), else ADA_EINVAL before any launch.  One workgroup
 *     per tile of ADA_FILTER_TILE_H x ADA_FILTER_TILE_W outputs stages tile and halo into LDS once, as order-preserving 32-bit keys (an fp32's bits
 *     with the sign bit flipped, all bits flipped when negative; a uint8 as it is) with one key value marking invalid, NaN and dropped samples.
 *     Each thread then selects s[r] bit by bit, from the top: a bit stays set when at most r keys of the window lie below the candidate -- 32 passes
 *     (8 for uint8) over the window in LDS, no per-thread array, trip counts that depend on (kh, kw) alone.
 *   ada_extreme_filter_fwd   rank ADA_RANK_MIN or ADA_RANK_MAX only; kh, kw <= ADA_FILTER_MAX_EXTREME, else ADA_EINVAL before any launch.
 *     Separable: a row pass (tiles of ADA_FILTER_TILE_H x ADA_FILTER_TILE_W) writes per pixel the extreme key and the number of valid samples of its
 *     kw row neighbours, a column pass (tiles of ADA_FILTER_COL_TILE_H x ADA_FILTER_TILE_W) combines kh of them.  An invalid sample contributes the
 *     identity element; the extreme of extremes and the integer sum of counts are exact, so the result equals ada_rank_filter_fwd's.
 *     workspace  workspace_bytes >= 5 batch h w (a key and a one-byte count per pixel), 4-byte aligned  (checked)
 *   Both read nothing back, allocate nothing, use no atomics and launch one fixed grid derived from the shapes: legal inside a stream capture, the
 *   same bytes every run.  Offsets into the maps are 64-bit.
 * ---------------------------------------------------------------------------------------- */
#define ADA_DT_U8 3                    /* x / out of the rank filters: uint8 */
#define ADA_BORDER_MIRROR 0
#define ADA_BORDER_NEAREST 1
#define ADA_BORDER_IGNORE 2
#define ADA_RANK_MIN 101               /* ranks 0 .. 100 are integer percents */
#define ADA_RANK_MEDIAN 102
#define ADA_RANK_MAX 103
#define ADA_FILTER_MAX_WINDOW 81       /* kh * kw of ada_rank_filter_fwd */
#define ADA_FILTER_MAX_EXTREME 63      /* kh and kw of ada_extreme_filter_fwd */
#define ADA_FILTER_TILE_W 64           /* outputs per workgroup: ADA_FILTER_TILE_H rows of ADA_FILTER_TILE_W */
#define ADA_FILTER_TILE_H 4
#define ADA_FILTER_COL_TILE_H 16       /* rows per workgroup of the extremes' column pass */
int ada_rank_filter_fwd(const void* x, const uint8_t* valid, int32_t dtype, int32_t batch, int32_t h, int32_t w, int32_t kh, int32_t kw,
                        int32_t rank, int32_t border, double fill, void* out, int32_t* count, void* stream);
int ada_extreme_filter_fwd(const void* x, const uint8_t* valid, int32_t dtype, int32_t batch, int32_t h, int32_t w, int32_t kh, int32_t kw,
                           int32_t rank, int32_t border, double fill, void* out, int32_t* count, void* workspace, int64_t workspace_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Hole filling: a pixel without a sample gets a value from the pixels that have one (additions under ABI 10).  The rasteriser paints what no triangle
 * covers with a constant and the rank filters give a window without a valid sample a constant; these give every pixel a value.  The reference has no
 * such operation.  valid: uint8 [batch][h][w] packed, non-zero = the pixel has a sample; one mask for all channels of an image.  x / out: fp32
 * [batch][channels][h][w] packed.  batch, channels, h, w >= 1; h, w <= 32767 (else ADA_EUNSUPPORTED), batch <= 65535.
 *   ada_nearest_valid_fwd    the Euclidean feature transform.  index int32 [batch][h][w] = the flat position r * w + c of the valid pixel of the same
 *     image nearest in Euclidean distance; dist2 (optional, NULL: not written) int32 = the squared distance, an exact integer.  A valid pixel maps to
 *     itself, distance 0.  TIE RULE: among equally near valid pixels the smallest flat position.  An image without a valid pixel: index = -1 and
 *     dist2 = 0x7fffffff everywhere.  sqrt(dist2) is scipy.ndimage.distance_transform_edt(valid == 0); scipy's own index at a tie is an artefact of
 *     its implementation and is not followed.
 *     Work: a column pass (two scans) leaves per pixel the row of the nearest valid pixel of its column, the upper at equal |dy|; a row pass takes the
 *     lexicographic minimum over x' of ((x - x')^2 + g(x')^2, r(x') w + x') with the row's pairs staged through LDS ADA_INPAINT_CHUNK columns at a time.
 *     workspace  workspace_bytes >= ada_nearest_valid_workspace_bytes = 4 batch h w, 4-byte aligned  (checked)
 *   ada_fill_gather_fwd      out[b][c][p] = valid[b][p] ? x[b][c][p] : (0 <= index[b][p] < h w ? x[b][c][index[b][p]] : empty).  Values move as
 *     32-bit words: valid and copied pixels keep every bit.  index is ada_nearest_valid_fwd's; one outside the image counts as "none", never read.
 *   ada_push_pull_fwd        the smooth multi-resolution fill.  Level 0 is h x w, level l + 1 is ceil(h_l / 2) x ceil(w_l / 2), the top level L is 1 x 1.
 *     All in fp32, every product, sum and quotient rounded on its own (csrc/ada_inpaint.hip is built without floating-point contraction):
 *     LEVEL 0  v = valid ? x : +0, m = valid ? 1 : 0, by a select: the value under an invalid pixel, NaN and inf included, never reaches a result.
 *     PULL     coarse pixel (I, J) has the children (2 I + di, 2 J + dj), di, dj in {0, 1}; a child outside the level has m = 0.  n = the children
 *              with m = 1; m' = n > 0; v' = n > 0 ? (((s00 + s01) + s10) + s11) / n : +0 with s = m ? v : +0 and a correctly rounded division.
 *     TOP      a top pixel with m = 0 takes ``empty`` and counts as filled (an image without a valid pixel).
 *     PUSH     top down.  A pixel (i, j) with m = 1 keeps v.  One with m = 0: I = i >> 1, I2 = clamp(I + (i & 1 ? 1 : -1), 0, h_{l+1} - 1), J and J2
 *              likewise from j and w_{l+1}; v = (((9 a + 3 b) + 3 c) + d) * 0.0625 with a = V(I, J), b = V(I, J2), c = V(I2, J), d = V(I2, J2) of
 *              the already pushed level above -- bilinear with half-pixel centres and clamped borders.  Every level is then completely filled.
 *     out      level 0 after the push; valid pixels carry x bit for bit.
 *     workspace  the pyramid above level 0: workspace_bytes >= ada_push_pull_workspace_bytes = batch (4 channels + 1) sum over l >= 1 of h_l w_l,
 *                4-byte aligned (checked; 0 for a 1 x 1 image, where workspace may be NULL).  The result does not depend on what it held.
 *     Work: one launch per level up, one per level down; a thread owns one pixel of the written level and walks the channels.
 *   All of them read nothing back, allocate nothing, use no atomics and launch fixed grids derived from the shapes: legal inside a stream capture, the
 *   same bytes every run.  Offsets into the maps are 64-bit.
 * ---------------------------------------------------------------------------------------- */
#define ADA_INPAINT_CHUNK 1024         /* columns of a row staged per step of ada_nearest_valid_fwd's row pass */
int ada_nearest_valid_workspace_bytes(int32_t batch, int32_t h, int32_t w, int64_t* bytes);
int ada_nearest_valid_fwd(const uint8_t* valid, int32_t batch, int32_t h, int32_t w, int32_t* index, int32_t* dist2, void* workspace,
                          int64_t workspace_bytes, void* stream);
int ada_fill_gather_fwd(const float* x, const uint8_t* valid, const int32_t* index, int32_t batch, int32_t channels, int32_t h, int32_t w, float empty,
                        float* out, void* stream);
int ada_push_pull_workspace_bytes(int32_t batch, int32_t channels, int32_t h, int32_t w, int64_t* bytes);
int ada_push_pull_fwd(const float* x, const uint8_t* valid, int32_t batch, int32_t channels, int32_t h, int32_t w, float empty, float* out,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Membrane solve: the discrete harmonic extension of the known pixels of a map over a masked grid (additions under ABI 10).  The exact counterpart of
 * ada_push_pull_fwd, and with a source added back (minus / plus below) seamless cloning in its membrane form.  The reference has no such operation.
 *   PROBLEM.  Grid h x w, 4-neighbour graph, per image: domain (uint8 [batch][h][w], non-zero = the pixel is a node; NULL = every pixel) and known (uint8,
 *     non-zero = Dirichlet pixel; it counts only inside domain).  x fp32 [batch][channels][h][w] packed, one mask pair for the channels of an image.  The
 *     unknowns are U = domain and not known.  For every p in U
 *         sum over q in N4(p), q inside the image, q in domain, of (u_p - u_q) = 0,      u_q = d_q on a known q,
 *     with the data d = x, or d = x - minus (both widened to fp64 first) when minus is given.  An edge to a pixel outside the image or outside domain does
 *     not exist (natural boundary).  The matrix is a symmetric M-matrix, positive definite on every 4-connected component of domain that holds a known
 *     pixel.  A component without one is a pure Neumann problem with a zero right side: conjugate gradients leave it at the mean of its start values, and
 *     callers overwrite it (hip_ext.inpaint does, with ``empty``) or keep it out of domain.
 *   OUTPUT.  On U: u_p, or u_p + plus_p when plus is given, rounded to fp32 once (out) and / or as fp64 (out64).  On every other pixel, known pixels and
 *     pixels outside domain alike: x bit for bit, moved as a 32-bit word (out64: that float widened).  The value under a pixel that is not known, NaN and
 *     inf included, never reaches a result (selects).  minus and plus are read on known pixels and on U respectively, nowhere else.
 *   METHOD.  Conjugate gradients in fp64.  Per plane the workspace holds u, r, q, two direction buffers, one code byte per pixel of the image, three
 *     partial sums per tile and two slots of scalars (r.r, tol, frozen, steps).  A step is two launches of (tiles, channels, batch) workgroups, a
 *     workgroup per ADA_MEMBRANE_TILE_H x ADA_MEMBRANE_TILE_W tile: the first reduces the tiles' r.r and max |r|, forms p' = r + beta p into the other
 *     direction buffer, q = A p' and the tiles' p'.q; the second reduces p'.q and updates u, r and the partials.  Every workgroup reduces the partials
 *     for itself in one fixed order; no float atomics, no grid-wide barrier, no cooperative launch, no workgroup that waits for another.  Every sum has
 *     one order that depends on (h, w) alone: a plane's result is the same bytes from run to run, and alone or inside any batch.
 *   FREEZE.  A plane is frozen once max |r| of the recurrence is <= tol, once p'.A p' <= 0, or once r.r or alpha is not finite.  From then on the kernels
 *     leave its state as it is.  A NaN in a known pixel costs that plane its result (converged = 0) and nobody a hang: the launches are counted, not awaited.
 *   ada_membrane_begin_fwd    writes the codes, the start vector (d on known pixels; guess, fp32, on U, or 0 when guess is NULL), the start residual and
 *     the scalars.  tol >= 0 and finite, in the units of x.  Two launches.
 *   ada_membrane_iterate_fwd  exactly ``iterations`` steps for all planes, frozen ones idle: 2 iterations launches, one more when ``frozen`` (uint8
 *     [batch channels], optional) is given and receives the planes' flags.  begin -> iterate(a) -> iterate(b) -> end is begin -> iterate(a + b) -> end bit
 *     for bit: the state is the workspace's alone.
 *   ada_membrane_end_fwd      evaluates the TRUE residual b - A u from u itself, writes out and / or out64 (one of them is required), and per plane
 *     residual (fp64, its max norm), iterations (int32, the steps taken before the freeze) and converged (uint8, residual <= tol).  Two launches.  x must
 *     be begin's; the state is finished afterwards (begin starts the next solve).
 *   workspace  workspace_bytes >= ada_membrane_workspace_bytes = 40 batch channels h w + 24 batch channels tiles + 48 batch channels + batch h w rounded
 *     up to 8, tiles = ceil(h / TILE_H) ceil(w / TILE_W); 8-byte aligned (checked).  Every cell is written before it is read.
 *   Limits: batch, channels, h, w >= 1; h, w <= 32767, batch, channels <= 65535 (else ADA_EUNSUPPORTED).  A null pointer, a bad tol or count, a workspace
 *   that is too small: ADA_EINVAL before any launch.  Nothing is read back or allocated; the launch sequence depends on the arguments alone: legal inside
 *   a stream capture.  Offsets into the maps are 64-bit.
 * ---------------------------------------------------------------------------------------- */
#define ADA_MEMBRANE_TILE_H 16         /* rows of a workgroup's tile: one partial sum per tile and plane */
#define ADA_MEMBRANE_TILE_W 64         /* columns of a workgroup's tile */
int ada_membrane_workspace_bytes(int32_t batch, int32_t channels, int32_t h, int32_t w, int64_t* bytes);
int ada_membrane_begin_fwd(const float* x, const float* minus, const uint8_t* known, const uint8_t* domain, const float* guess, int32_t batch,
                           int32_t channels, int32_t h, int32_t w, double tol, void* workspace, int64_t workspace_bytes, void* stream);
int ada_membrane_iterate_fwd(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t iterations, uint8_t* frozen, void* workspace,
                             int64_t workspace_bytes, void* stream);
int ada_membrane_end_fwd(const float* x, const float* plus, int32_t batch, int32_t channels, int32_t h, int32_t w, float* out, double* out64,
                         double* residual, int32_t* iterations, uint8_t* converged, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tiled inference for inputs larger than the network's native 518 x 518 (the reference squashes every
 * input to 518 x 518, infer.py:17,84).  ada_tile_blend_fwd merges the per-tile predictions:
 *   tiles     fp32 [B, T, tile_h, tile_w]; tile t covers rows origin_y[t].. and columns origin_x[t].. of the full map
 *             (origin_* are DEVICE int32 [T]); every output pixel must be covered by at least one tile (one that is not comes out NaN)
 *   weight    separable feather min(i + 1, n - i, ramp) / ramp per axis: linear cross-fade over `ramp` pixels in overlaps
 *   out       fp32 [B, height, width] = sum_t w_t tile_t / sum_t w_t, both sums and the quotient in double, rounded once
 * ---------------------------------------------------------------------------------------- */
int ada_tile_blend_fwd(const float* tiles, int32_t batch, int32_t n_tiles, int32_t tile_h, int32_t tile_w,
                       const int32_t* origin_y, const int32_t* origin_x, int32_t height, int32_t width,
                       int32_t ramp, float* out, void* stream);

/* Hardware self-test used by the GPU test-suite: checks the MFMA / LDS-transpose fragment layouts the
 * kernels assume against a scalar computation on the device.  Returns 0 when they hold,
 * a positive bit mask of failed probes otherwise.  scratch: >= 1 MiB of device memory. */
int ada_selftest(void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tuning / diagnostic hooks.  Process-global switches (atomics) used by the test-suite (to run every tile
 * configuration and both main loops of ada_igemm against the same references), by tools/ (A/B
 * timing) and by bench.py (to report which kernel ran).  They never change results beyond fp32
 * summation order.  The environment variables ADA_IGEMM_TILE / _VARIANT / _GROUP and ADA_ATTN_VARIANT preset
 * the same switches once, at the first ada_igemm / ada_attention_fwd call.  One default and at most one alternate per
 * kernel family are built; what was measured and removed is recorded in DESIGN.md section 8 and profiles/.
 *   ada_debug_set_tile(cfg)      force the ada_igemm tile: 0 256x32, 1 128x64, 2 256x128, 3 256x256,
 *                                4 128x128; -1 = heuristic (default)
 *   ada_debug_set_variant(v)     main loop of the 256x256 tile: 0 = chosen by shape (default: the hand-scheduled 4-wave loop for
 *                                k-loops of >= 128 k-tiles, the single-barrier 8-wave loop otherwise); 4 = always the 8-wave loop;
 *                                16 = always the hand-scheduled 4-wave loop (generated assembly, csrc/ada_igemm_pipe4.inc)
 *   ada_debug_set_group(g)       force the column-group width of the tile order (0 = traffic model)
 *   ada_debug_last_tile()        tile code of the calling thread's most recent ada_igemm launch
 *                                (+200 when the hand-scheduled 4-wave main loop ran), -1 before the first launch
 *   ada_debug_set_timestamps(p)  device buffer of 8 x u64 per workgroup receiving s_memtime stamps
 *                                of the single-barrier loop, or NULL (default)
 *   ada_debug_set_attention_variant(v)  5 = 4-wave kernel with the softmax interleaved between its MFMAs (default),
 *                                3 = the 4-wave round-1 kernel (load, QK^T, softmax, PV in sequence)
 * ---------------------------------------------------------------------------------------- */
void ada_debug_set_tile(int cfg);
void ada_debug_set_variant(int v);
void ada_debug_set_group(int g);
int ada_debug_last_tile(void);
void ada_debug_set_timestamps(void* dev_buf);
void ada_debug_set_attention_variant(int v);
/* Saturation probe.  fp32 -> operand conversions clamp to the largest finite fp16 (+-65504) instead of overflowing to inf
 * (csrc/ada_common.h to_op); that is silent in the forward.  This adds, to the device counter *count (uint64, caller-zeroed), the
 * number of elements of an operand-typed buffer of n elements that sit AT the clamp (or are inf / NaN), so a caller can sweep the
 * activation buffers after a forward (hip_ext.engine.DepthEngine.saturation_report).  Asynchronous on `stream`; not on the hot path. */
int ada_debug_count_saturated(const void* buf, int64_t n, void* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Guided filter (He, Sun, Tang) and its fast form, guided joint up-sampling (additions under ABI 10): a map is fitted, window by window, as a linear
 * function of a guide image, and the fit is applied to the guide -- smoothing that keeps the guide's edges, and the way from depth at the network's size
 * to depth at the photo's size.  The reference has no such operation: it resizes with cv2's nearest rule (infer.py:77, 113).
 *   INPUT.  p: fp32 [batch][h][w] packed.  valid: optional uint8 of that shape (NULL: every sample).  A sample VOTES when valid is absent or non-zero
 *     there and p is not NaN; what lies under a sample that does not vote never reaches a result.  guide I: uint8 (ADA_DT_U8) or fp32 (ADA_DT_F32)
 *     [batch][gh][gw][channels] packed, channels C = 1 or 3, gh >= h and gw >= w.  radius r, 0 <= r <= ADA_GUIDED_MAX_RADIUS: the window of a pixel
 *     is the (2 r + 1)^2 positions around it that lie inside the image -- there is no other border rule.  eps > 0 and finite, in raw guide units
 *     (eps 255^2 for a uint8 guide and an eps meant for [0, 1]).  Sides <= 32767 (else ADA_EUNSUPPORTED), batch <= 65535.
 *   COEFFICIENT PASS, at the map's size (ada_guided_coeff_fwd).  The guide sample of map pixel (y, x) is I[((2 y + 1) gh) / (2 h)][((2 x + 1) gw) / (2 w)]
 *     (integer quotients): the identity for equal sizes, plain sub-sampling otherwise.  Over the n voting samples of a pixel's window, from the sums
 *     S1 = n, SI, SII = sum I I^T, Sp, SIp:  mI = SI / n, mp = Sp / n, Cov(I, I) = SII / n - mI mI^T, Cov(I, p) = SIp / n - mI mp,
 *         a = (Cov(I, I) + eps U)^-1 Cov(I, p)      (C = 1: a quotient; C = 3: an L D L^T solve, never the adjugate),      b = mp - a . mI.
 *     A window with n = 0 has no (a, b).  coeff fp64 [batch][h][w][C + 1] = (mean a_0 .. mean a_{C-1}, mean b) over the window's pixels that have one;
 *     covered uint8 [batch][h][w] = 1 where at least one has, else 0 and coeff = 0.
 *   APPLY PASS, at the guide's size H = gh, W = gw (ada_guided_apply_fwd).  Output pixel (Y, X) has the source coordinates
 *         sy = ((Y + 0.5) * h) / H - 0.5 clamped to [0, h - 1],  sx = ((X + 0.5) * w) / W - 0.5 clamped to [0, w - 1]      (fp64, in this order)
 *     y0 = floor(sy), y1 = min(y0 + 1, h - 1), fy = sy - y0, likewise x0, x1, fx.  The taps, in this order, are (y0, x0), (y0, x1), (y1, x0), (y1, x1) with
 *     the weights (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx.  A tap of weight 0 is never read (equal sizes give sy = Y exactly: the single tap).
 *     A tap of positive weight CONTRIBUTES when covered there.  c_j = sum over the contributing taps, in order, of weight * coeff_j; when a tap of
 *     positive weight does not contribute, c_j is divided by the sum (in order) of the contributing weights.  No contributing tap: out = fill.  Otherwise
 *         out = fp32( ((c_0 I_0 + c_1 I_1) + c_2 I_2) + c_C )       (C = 1: c_0 I_0 + c_1)  with I the guide at (Y, X).
 *   ARITHMETIC.  Every sum, product, quotient and the solve in fp64, each rounded on its own (csrc/ada_guided.hip is built without floating-point
 *     contraction); one rounding to fp32 at the very end.  The order of a window's sums is the kernels' own (rows of a column, then columns): against an
 *     fp64 restatement the fp32 results agree except at a rounding boundary.  The apply pass from given coeff / covered is reproduced bit for bit.
 *   WORK.  Coefficients: four launches, a thread per map pixel -- the column sums of the 5 (C = 1) or 14 (C = 3) moment planes, their row sums (a row's
 *     planes staged through LDS, ADA_GUIDED_TILE_W outputs per workgroup) with the solve, and the same two steps for the C + 2 planes (a, b, has).
 *     workspace  workspace_bytes >= ada_guided_workspace_bytes = 8 batch h w (moment planes + C + 2), 8-byte aligned (checked).  The result does
 *                not depend on what it held.
 *     Apply: one launch, a thread per ADA_GUIDED_APPLY_PX pixels of a row; vector loads and stores when W is a multiple of that and guide and out
 *     lie on 16-byte boundaries, the same values element by element otherwise.
 *   Refusals (ADA_EINVAL before any launch): a null pointer, r out of range, eps not finite and positive, C not 1 or 3, a guide dtype other than the
 *   two, a guide smaller than the map, a workspace that is too small.  All of them read nothing back, allocate nothing, use no atomics and launch fixed
 *   grids derived from the shapes: legal inside a stream capture, the same bytes every run.  Offsets into the maps are 64-bit.
 * ---------------------------------------------------------------------------------------- */
#define ADA_GUIDED_MAX_RADIUS 31
#define ADA_GUIDED_TILE_W 256          /* outputs of a row per workgroup of the row passes */
#define ADA_GUIDED_APPLY_PX 4          /* pixels of a row per thread of the apply pass */
int ada_guided_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t channels, int64_t* bytes);
int ada_guided_coeff_fwd(const float* p, const uint8_t* valid, const void* guide, int32_t guide_dtype, int32_t batch, int32_t h, int32_t w, int32_t gh,
                         int32_t gw, int32_t channels, int32_t radius, double eps, double* coeff, uint8_t* covered, void* workspace,
                         int64_t workspace_bytes, void* stream);
int ada_guided_apply_fwd(const double* coeff, const uint8_t* covered, const void* guide, int32_t guide_dtype, int32_t batch, int32_t h, int32_t w,
                         int32_t gh, int32_t gw, int32_t channels, float fill, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADA_HIP_H */
