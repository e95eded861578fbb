/* otvm_hip.h -- C ABI of libotvm_hip.so: the MI355X (gfx950) kernels behind the OTVM per-frame
 * inference path.
 *
 * The reference (Hongje/OTVM) has no FFI: its drop-in boundary is the Python nn.Module call
 * `EvalModel.forward` (reference models/alpha/model.py:391-512).  The product keeps that Python
 * surface (otvm_amd/alpha_model.py) and implements every device operation below it through this
 * C ABI -- plain pointers, sizes and a hipStream_t; no torch types.  Each entry point cites the
 * reference code whose device work it replaces.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless noted; `stream` is a hipStream_t passed as void*;
 *   - activations are NHWC fp32 with an explicit pixel stride `ld` (elements), so a tensor may be
 *     a channel slice of a wider buffer (this is how every torch.cat of the reference disappears);
 *   - channel counts of device tensors are padded to a multiple of 4 (zero weights on the pad);
 *   - every function returns 0 on success, non-zero on error; otvm_last_error() describes it.
 */
#ifndef OTVM_HIP_H
#define OTVM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTVM_ACT_NONE 0
#define OTVM_ACT_RELU 1
#define OTVM_ACT_LEAKY 2 /* negative slope 0.01 (nn.LeakyReLU default, FBA/models.py:305) */

/* Convolution arithmetic.  F32 and F16X3 accumulate in fp32 and meet the reference's 1e-3 fp32 contract:
 *   F32   : v_mfma_f32_32x32x2_f32, exact fp32 products (157 TFLOP/s peak);
 *   F16X3 : each fp32 operand split into fp16 hi+lo (22 significant bits), three
 *           v_mfma_f32_32x32x16_f16 passes hi*hi + hi*lo + lo*hi (833 TFLOP/s fp32-equivalent peak);
 *   F16   : (ABI 18) a LABELLED reduced-precision mode, never a default and not covered by the parity contract: operands rounded
 *           to fp16 once, ONE v_mfma_f32_32x32x16_f16 pass, fp32 accumulate -- in the implicit-GEMM and 3x3 patch kernels; the
 *           other f16x3 kernels (stems, 16-wide head tile, fused STM bottleneck, memory read) keep their three passes.  Takes
 *           the f16x3 weight arrays (w_hi / w_scale / w_frag / w_wfrag).                                                   */
#define OTVM_PREC_F32 0
#define OTVM_PREC_F16X3 1
#define OTVM_PREC_F16 2

const char* otvm_last_error(void);
#define OTVM_ABI_VERSION 21   /* 2: otvm_ppm_pool_ws_bytes(H, C); 3: otvm_conv_params.in_scale/in_shift/in_act;
                                 4: otvm_conv_params.splitk_ws; 5: otvm_preprocess_params.fg_u8/bg_u8/u8_rgb;
                                 6: otvm_conv_params.tune + otvm_conv2d_candidates;
                                 7: folded GroupNorm tables on otvm_gn_apply's residual and otvm_upsample_bilinear's input;
                                 8: otvm_memory_read_f16x3_partial / _combine / _partial_count; 9: otvm_ppm_head;
                                 10: otvm_finite_guard, otvm_clear;
                                 11: batch of images per launch (otvm_conv_params.batch ..., otvm_gn_*_b, otvm_upsample_bilinear_b,
                                     otvm_maxpool3x3s2_b);
                                 12: training forward (otvm_fba_head_train, otvm_upsample4_logits3, otvm_trimap_to_sm, otvm_loss_*);
                                 13: otvm_conv_params.w_wfrag + otvm_pack_wave_weight_f16x3 (one-wave 64x64 tile);
                                 14: otvm_ppm_conv_z / otvm_ppm_conv_add (the PPM branches' share of conv_up1.0 without upsampling);
                                 15: otvm_stm_bottleneck_f16x3 (one kernel per 1/4-resolution bottleneck of the STM encoders);
                                 19: ... and per 1/8-resolution identity bottleneck (Cin = 512, otvm_stm_bottleneck_params.tile);
                                 16: otvm_conv_params.gn_gamma ... gn_counter (the GroupNorm scale / shift table of the OUTPUT
                                     written by the conv's last workgroup instead of a separate otvm_gn_table launch);
                                 17: otvm_gram_f16 / otvm_gn_predict (GroupNorm statistics of a 1x1 convolution's output predicted
                                     from its input's Gram matrix: the normalisation moves into that convolution's epilogue);
                                 18: otvm_gram_params.diag / otvm_gn_predict_params.diag (conditioning + saturation diagnostics of the
                                     predicted statistics); implicit-GEMM tiles 32 + t with LDS-DMA weight stages and 64 + t = the same on
                                     v_mfma_f32_16x16x32_f16 (tune codes; no new entry points);
                                 20: otvm_matting_grad_conn / _ws_bytes / _params (Grad and Conn matting metrics);
                                 21: otvm_optflow_farneback / _ws_bytes / _params, otvm_matting_messddt (MESSDdt);
                                 (21, additive: the foreground outputs -- the entry points with _fgr in their names and the output
                                  kernel of otvm_fgr_params are NEW symbols only; no existing struct, prototype or result changed, so a
                                  caller built against the earlier 21 runs unchanged and the number stays;
                                  likewise otvm_trimap_apply_labels, the label pass of the keyframe corrections;
                                  likewise working-resolution matting: otvm_downsample_u8 / _trimap / _labels, otvm_guided_ws_bytes,
                                  otvm_guided_coeffs and otvm_guided_apply with their struct otvm_guided_params;
                                  likewise trimaps from masks: otvm_trimap_from_mask / _ws_bytes with otvm_mask_trimap_params;
                                  likewise the temporal stabilisation of alpha: otvm_luma_u8 and otvm_temporal_blend with
                                  otvm_temporal_params;
                                  likewise the patch conv with an upsampled source: otvm_conv2d_up and
                                  otvm_conv2d_accepts_upsampled_input with otvm_conv_up_params;
                                  likewise region-of-interest matting: otvm_trimap_bbox, otvm_roi_crop and otvm_roi_paste with
                                  otvm_roi_bbox_params, otvm_roi_crop_params and otvm_roi_paste_params;
                                  likewise the tracking window of region-of-interest matting: otvm_roi_track with
                                  otvm_roi_track_params, and otvm_roi_crop_at / otvm_roi_paste_at, which take the two structs above
                                  as they are plus a device pointer;
                                  likewise multi-subject matting: otvm_subjects_track, otvm_subjects_crop, otvm_subjects_bbox and
                                  otvm_subjects_resolve with their otvm_subjects_*_params;
                                  likewise video streams: otvm_yuv_to_rgb and otvm_rgb_to_yuv420 with otvm_yuv_to_rgb_params and
                                  otvm_rgb_to_yuv420_params;
                                  likewise masks of keyed footage: otvm_mask_from_chroma and otvm_mask_from_plate with
                                  otvm_mask_from_chroma_params and otvm_mask_from_plate_params) */
int otvm_abi_version(void);

/* ---------------------------------------------------------------- weights (load time) ----------
 * Pack an OIHW fp32 conv weight into the K-major layout the implicit-GEMM kernel reads:
 * w_packed[O_pad][K_pad], k = (ky*kw + kx)*I_pad + c, zero padded.  otvm_conv2d reads whole N tiles of
 * weight rows: O_pad must be O rounded up to a multiple of 128 (the same holds for w_hi / w_lo).
 *   ws != 0  : apply weight standardisation first (layers_WS.py:15-21: subtract per-filter mean,
 *              divide by sqrt(unbiased var + 1e-12) + 1e-5) -- done ONCE here instead of per forward.
 *   scale    : optional per-output-channel multiplier (BatchNorm eval fold gamma/sqrt(var+eps),
 *              torchvision Bottleneck inside STM.py:43-51,79-87), may be NULL.                    */
int otvm_pack_conv_weight(const float* w_oihw, int O, int I, int kh, int kw, int ws, const float* scale,
                          float* w_packed, int O_pad, int I_pad, int K_pad, void* stream);

/* f16x3, 3x3 stride-1 convolutions with I_pad % 32 == 0: weights in MFMA B-fragment order for the patch kernel
 * (conv_patch_f16x3.hip), [I_pad/32][9 taps][ceil(O/32)][2 k-steps][hi|lo][64 lanes][8 halfs].  w_scale as above. */
int64_t otvm_patch_weight_bytes_f16x3(int O, int I_pad);
int otvm_pack_patch_weight_f16x3(const float* w_packed, int O, int K_pad, int I_pad, void* w_frag, float* w_scale,
                                 void* stream);

/* f16x3, 7x7 stride-2 stems with few input channels (I_pad <= 64, O <= 64): weights in MFMA B-fragment order for the stem
 * kernel (conv_stem_f16x3.hip), [ceil(I_pad/8) channel groups][25 k-steps of two taps][2 n-tiles][hi|lo][64 lanes][8 halfs];
 * goes into otvm_conv_params.w_frag of such a layer.                                                              */
int64_t otvm_stem_weight_bytes_f16x3(int I_pad);
int otvm_pack_stem_weight_f16x3(const float* w_packed, int O, int K_pad, int I_pad, void* w_frag, float* w_scale,
                                void* stream);

/* Fold an eval-mode BatchNorm (eps 1e-5, running statistics; torchvision Bottleneck used by
 * STM.py:43-51,79-87) into a per-channel scale/bias: scale = gamma/sqrt(var+eps),
 * bias = beta - mean*scale.                                                                       */
int otvm_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int n,
                 float* scale, float* bias, void* stream);

/* ---------------------------------------------------------------- convolution ------------------
 * Implicit-GEMM convolution on the matrix cores (see OTVM_PREC_*), replaces every F.conv2d of
 * the path (180 per non-first frame).  out = act(conv(in') + bias + residual) where
 * in' = relu(in) if in_relu (STM.py:23-24 pre-activation ResBlock) else in.                       */
typedef struct {
    const float* in;  int H, W, Cin, in_ld;         /* Cin: padded channel count, multiple of 4 */
    const float* w;   int K_pad;                    /* packed weight from otvm_pack_conv_weight */
    const float* bias;                              /* [Cout] or NULL                           */
    const float* residual; int res_ld;              /* [Ho*Wo, Cout] view or NULL               */
    float* out;       int Ho, Wo, Cout, out_ld;
    int kh, kw, stride, pad, dil;
    int in_relu, act;
    int precision;                                  /* OTVM_PREC_F32 | OTVM_PREC_F16X3 | OTVM_PREC_F16 */
    const void* w_hi; const void* w_lo;             /* f16x3: split weights [O_pad][K_pad] fp16   */
    const float* w_scale;                           /* f16x3: per-filter power-of-two scale [Cout] */
    const void* w_frag;                             /* f16x3, optional: fragment-major weights for the 3x3 patch kernel
                                                       (otvm_pack_patch_weight_f16x3) or, for a 7x7 stride-2 layer, the
                                                       stem kernel (otvm_pack_stem_weight_f16x3); NULL = implicit GEMM only */
    double* gn_stats;                               /* optional: fused GroupNorm(32) statistics of the OUTPUT
                                                       (sum, sum of squares per group, [32][2] fp64, accumulated
                                                       atomically; Cout = 64, 128, 256, ... (32 groups of a power-of-two
                                                       number of channels), act == NONE, no residual) or NULL        */
    const float* in_scale; const float* in_shift;   /* optional fused normalisation of the INPUT (the GroupNorm apply of
                                                       the producing layer folded into this conv's staging):
                                                       in' = in_act(in * in_scale[c] + in_shift[c]) inside the image, zero
                                                       padding outside; tables of Cin floats from otvm_gn_table, or NULL.
                                                       Only layers for which otvm_conv2d_accepts_input_norm() returns 1 */
    int in_act;                                     /* OTVM_ACT_* applied after the input normalisation */
    int tune;                                       /* 0 = built-in heuristic; else a configuration code returned by
                                                       otvm_conv2d_candidates (which kernel / tile / K split runs the layer) */
    void* splitk_ws; int64_t splitk_ws_bytes;       /* optional workspace (f16x3): layers with too few output tiles to fill
                                                       the chip split K over up to 8 workgroups per tile and reduce the
                                                       partial tiles in a fixed order (deterministic); NULL = never split.
                                                       One workspace per stream that runs convs concurrently.          */
    /* ---- batch (ABI 11): the same layer applied to `batch` images in ONE launch (independent video sequences stepped
     * in lock-step share the weights; small maps cannot fill 256 CUs from one image).  Image b of a tensor lives `*_bs`
     * ELEMENTS behind image 0; every image is computed exactly as a batch-1 launch computes it (same tiles, same
     * summation order).  batch <= 1: a single image, the strides are ignored.                                      */
    int batch;
    int64_t in_bs, out_bs, res_bs;                  /* floats between consecutive images of in / out / residual        */
    int gn_bs;                                      /* doubles between the images' [32][2] statistics blocks (gn_stats) */
    int norm_bs;                                    /* floats between the images' in_scale / in_shift tables            */
    const void* w_wfrag;                            /* f16x3, optional (ABI 13): the split weights in MFMA B-fragment order for
                                                       the one-wave 64x64 tile (otvm_pack_wave_weight_f16x3); layers with
                                                       Cin % 32 == 0; NULL = that tile is never a candidate               */
    /* ---- ABI 16, optional, with gn_stats: the per-channel table otvm_gn_table would compute from the finished statistics
     * (scale[c] = rstd[g] gamma[c], shift[c] = beta[c] - mean[g] scale[c]; same arithmetic, same bits) is written by the
     * LAST workgroup of the launch to finish (each workgroup takes a ticket from *gn_counter after its statistics are in;
     * the counter re-arms itself to 0).  Consumers that normalise on the fly (in_scale / in_shift of the next conv, the
     * resampling kernels) then need no launch in between.  gn_counter: one zero-initialised unsigned per image.  Paths
     * that finish the statistics in a pass of their own (split K, exact fp32) launch the table kernel internally.      */
    const float* gn_gamma; const float* gn_beta;    /* GroupNorm weight / bias, Cout floats                              */
    float* gn_scale_out; float* gn_shift_out;       /* Cout floats each; image b's tables gn_tab_bs floats behind image 0 */
    unsigned* gn_counter;
    int gn_tab_bs;
    /* ---- ABI 17, 1x1 layers on the implicit-GEMM route (f16x3) only: a layer whose epilogue carries a PREDICTED
     * normalisation of its output (otvm_gn_predict writes w_scale / bias per frame and per image).                      */
    int ws_bs;                                      /* floats between the images' w_scale / bias arrays (0 = shared)      */
    const float* res_scale;                         /* optional, with residual: residual' = residual * res_scale[c] (the
                                                       GroupNorm scale of a raw identity-path tensor, otvm_gn_table; its shift
                                                       belongs into bias -- otvm_gn_predict_params.res_shift); Cout floats,
                                                       image b's table res_scale_bs floats behind image 0                 */
    int res_scale_bs;
    const float* in_res; int in_res_ld; int64_t in_res_bs;
                                                    /* optional, with in_scale, layers for which otvm_conv2d_accepts_input_residual()
                                                       returns 1 (3x3 patch kernel, <= 64 output channels): the input is the raw
                                                       input of a residual block's last GroupNorm whose apply pass is skipped,
                                                       in' = in_act(in * in_scale[c] + in_shift[c] + in_res) -- the arithmetic of
                                                       otvm_gn_apply with a residual; in_res = the block's identity, same shape   */
} otvm_conv_params;
int otvm_conv2d_accepts_input_residual(const otvm_conv_params* p);

/* ABI 17: the last 3x3 convolution of the FBA decoder / refinement (32 -> 16, LeakyReLU; FBA/models.py:383-388, 425-432) with
 * the head that follows it -- 1x1 conv 16 -> n_out, clamp / sigmoid, fba_fusion, softmax of the trimap-refinement logits; the
 * per-pixel arithmetic of otvm_fba_head below -- in the epilogue: the 16 hidden values never leave the registers.  p = the conv
 * (3x3, stride 1, dilation 1, Cin % 16 == 0, Cout == 16, f16x3, w_frag; p->out = the hidden state or NULL: not written);
 * image b of the head's tensors lives *_bs floats behind image 0 (p->batch > 1).                                            */
typedef struct otvm_head_params {
    const float* w; const float* b; int n_out;      /* 1x1 head: [n_out][16], [n_out]; n_out = 7 or 10                         */
    const float* img; int img_ld;                   /* composited RGB in [0,1]: 3 channels at pixel stride img_ld               */
    int64_t P;                                      /* pixels per plane of the planar outputs (= H * W of the conv)            */
    float* alpha_out; int alpha_stride;             /* fused alpha, element i at alpha_out[i * alpha_stride]                   */
    float* tri_out;                                 /* n_out == 10: [3][P] softmax of logits 7..9                              */
    float* sm; int sm_ld;                           /* optional (n_out == 10): p_unknown, p_fg, alpha -> sm[i * sm_ld + 3..5]   */
    int64_t img_bs, alpha_bs, tri_bs, sm_bs;
    const void* w16;                                /* optional: the conv's weights as B fragments of the 16-wide matrix-core tile
                                                       (otvm_pack_head16_weight_f16x3; Cin == 32): v_mfma_f32_16x16x32_f16 with
                                                       N = the 16 real output channels instead of a half-empty 32-wide tile   */
} otvm_head_params;
int otvm_conv2d_head(const otvm_conv_params* p, const otvm_head_params* h, void* stream);
/* The same launch, keeping the head's foreground estimate as well: fgr = planar [3][P] fp32 over the padded frame, R, G, B --
 * the clamped fused F of fba_fusion (FBA/models.py:281-284), the value the B update and the final alpha read; image b of a batch
 * at fgr + b * fgr_bs.  A compile-time form of the same two kernels (16-wide / 32-wide, chosen as above): alpha, trimap, sm and
 * the hidden state are bit-identical to the call without it; pixels outside the image are not written.                        */
int otvm_conv2d_head_fgr(const otvm_conv_params* p, const otvm_head_params* h, float* fgr, int64_t fgr_bs, void* stream);
int64_t otvm_head16_weight_bytes_f16x3(void);
/* w_packed = otvm_pack_conv_weight's output of a 3x3 layer with I_pad == 32 and 16 filters, w_scale = its split scale */
int otvm_pack_head16_weight_f16x3(const float* w_packed, int O, int K_pad, int I_pad, const float* w_scale, void* w16, void* stream);
int otvm_conv2d(const otvm_conv_params* p, void* stream);
/* The legal kernel configurations of a layer (f16x3): the patch kernel where the shape allows it, and the implicit-GEMM
 * tiles 256x256 ... 64x64, each alone or with the K range of every output tile shared by S = 2..8 workgroups
 * (deterministic fixed-order reduction through splitk_ws).  Writes up to max_n opaque codes to `out`, returns their
 * number; a code goes into otvm_conv_params.tune.  All configurations compute the same convolution (results differ
 * by fp32 summation order only); the host times them on the device once per layer shape and keeps the fastest.    */
int otvm_conv2d_candidates(const otvm_conv_params* p, int* out, int max_n);
/* 1 when otvm_conv2d would run the layer on a kernel that implements in_scale / in_shift -- f16x3: the 3x3 stride-1 patch
 * kernel, or (round 3) any implicit-GEMM tile on a layer with Cin % 32 == 0 and no in_relu -- else 0: the caller then applies
 * otvm_gn_apply as a separate pass.  Bit-identical to that two-pass route in the same configuration.                       */
int otvm_conv2d_accepts_input_norm(const otvm_conv_params* p);
/* 0 = no kernel takes it, 1 = the patch kernel would run this layer, 2 = an implicit-GEMM tile (which normalises every input
 * element once per tap: worth it for 1x1 layers, not for 3x3 layers with many channels -- the host's choice).  (ABI 16) */
int otvm_conv2d_input_norm_kind(const otvm_conv_params* p);

/* (21, additive: new symbols only.)  A 3x3 patch-kernel conv whose LEADING Cu input channels are the 2x bilinear upsampling
 * (align_corners = False) of a source-resolution tensor, interpolated while the conv stages its input patch: the 4x copy that
 * otvm_upsample_bilinear_b would write into channels [0, Cu) of the conv's input is never made.  Input channels [0, Cu) of the
 * weights meet the upsampled source, channels [Cu, p->Cin) the full-resolution view p->in, whose FIRST channel is input channel Cu
 * (p->in_ld / p->in_bs as usual; p->Cin stays the layer's whole padded channel count).  Each source element is normalised
 * (scale / shift / act: a GroupNorm table as otvm_upsample_bilinear_b takes it, or NULL) once, then blended with the arithmetic of
 * that kernel: the output -- and the fused GroupNorm sums -- equal, bit for bit, those of the pass followed by otvm_conv2d.
 * Taken by: f16x3 / f16, 3x3, stride 1, dilation 1, Cout <= 64 (the 64-filter and 32-filter patch tiles), p->H == 2 Hi and
 * p->W == 2 Wi, Cu % 16 == 0, no in_scale / in_relu / in_res on p, tune 0 or the patch kernel's code, 16-byte aligned views.  */
typedef struct otvm_conv_up_params {
    const float* src; int Hi, Wi, Cu, src_ld;       /* [Hi][Wi][Cu] at pixel stride src_ld                                    */
    int64_t src_bs;                                 /* floats between the images' sources (p->batch > 1)                      */
    const float* scale; const float* shift;         /* optional: src' = act(src * scale[c] + shift[c]), Cu floats each         */
    int act;                                        /* OTVM_ACT_* after the normalisation                                     */
    int norm_bs;                                    /* floats between the images' tables                                       */
    int tile_rows;                                  /* 0 = the tile otvm_conv2d picks for the map; 16 = the 16x32-pixel tile of the
                                                       <= 32-filter layers whatever the map size (same bits either way)        */
} otvm_conv_up_params;
int otvm_conv2d_up(const otvm_conv_params* p, const otvm_conv_up_params* u, void* stream);
/* 1 when otvm_conv2d_up takes (p, u), else 0 (wrong tile family, Cu % 16 != 0, a map that is not exactly 2x the source,
 * unaligned views, ...); launches nothing.                                                                                   */
int otvm_conv2d_accepts_upsampled_input(const otvm_conv_params* p, const otvm_conv_up_params* u);

/* f16x3: derive the split weights from a packed fp32 weight (see otvm_pack_conv_weight):
 * row o is scaled by 2^-e (|w| <= 1), w_hi = fp16(w), w_lo = fp16(w - w_hi), w_scale[o] = 2^e.
 * When I_pad % 32 == 0 (and taps <= 32) K is re-ordered channel-block major ([c/32][tap][c%32]) so
 * that the taps of one channel block are consecutive K chunks (input re-reads hit L1/L2).        */
int otvm_split_conv_weight_f16x3(const float* w_packed, int O, int O_pad, int K_pad, int taps, int I_pad,
                                 void* w_hi, void* w_lo, float* w_scale, void* stream);

/* f16x3, layers with I_pad % 32 == 0 (K in whole 32-channel chunks): the split weights w_hi / w_lo [O_pad][K_pad] (from
 * otvm_split_conv_weight_f16x3, K already in the kernel's chunk order) re-packed as MFMA B fragments
 * [O_pad/32][K_pad/32][2 k-steps][hi|lo][64 lanes][8 halfs] (1-KiB blocks, one coalesced load each) for the one-wave
 * 64x64 tile -- the small-map configuration whose operands bypass LDS; goes into otvm_conv_params.w_wfrag.           */
int64_t otvm_wave_weight_bytes_f16x3(int O_pad, int K_pad);
int otvm_pack_wave_weight_f16x3(const void* w_hi, const void* w_lo, int O_pad, int K_pad, void* w_wfrag, void* stream);

/* One torchvision Bottleneck of the STM encoders (stride 1, eval-mode BatchNorm folded: STM.py:43-51,79-87) as ONE launch:
 * t1 = relu(W1 x + b1), t2 = relu(W2 * t1 + b2), y = relu(W3 t2 + b3 + identity); the intermediates stay in LDS, x is read once
 * (with a one-pixel halo), y written once.
 *   1/4-resolution stage (planes = 64, y has 256 channels; csrc/bottleneck_f16x3.hip):
 *     Cin = 256: identity block (identity = x).   Cin = 64: the stage's first block -- the projection Wd x is folded into the
 *     last GEMM: w3f / s3 then belong to the concatenated filter [W3 | Wd] (K = 128) and b3 = b3 + bd.
 *   1/8-resolution stage (ABI 19; planes = 128, y has 512 channels; csrc/bottleneck128_f16x3.hip):
 *     Cin = 512: identity block (res3.1 - res3.3).  `tile` picks the pixel block of a workgroup: 0 = from the map size,
 *     1 = 8 x 16, 2 = 8 x 8, 3 = 4 x 8 (every tile computes the same values; fp32 summation orders are identical too).
 *   w1f / w2f / w3f: otvm_pack_wave_weight_f16x3 of the split weights (K-major [O_pad][K_pad] from otvm_split_conv_weight_f16x3);
 *   s*: their per-filter scales; b*: folded biases.  f16x3 arithmetic (OTVM_PREC_F16X3).                                  */
typedef struct {
    const float* x; int H, W, Cin, x_ld;            /* [H*W, Cin] view                                       */
    float* y; int y_ld;                             /* [H*W, 256 | 512] view                                 */
    const void* w1f; const void* w2f; const void* w3f;
    const float* s1; const float* s2; const float* s3;
    const float* b1; const float* b2; const float* b3;
    int batch; int64_t x_bs, y_bs;                  /* images per launch, floats between consecutive images  */
    int tile;                                       /* ABI 19: planes-128 blocks only, see above             */
} otvm_stm_bottleneck_params;
int otvm_stm_bottleneck_f16x3(const otvm_stm_bottleneck_params* p, void* stream);

/* ---------------------------------------------------------------- GroupNorm(32) ----------------
 * nn.GroupNorm(32, C, eps=1e-5, affine) (layers_WS.py:26-27, FBA/models.py:272-276), two passes:
 * stats accumulates per-group sum / sum-of-squares in fp64 (stats[32][2], must be zeroed before);
 * apply computes y = act((x-mean)*rstd*gamma + beta + residual).                                  */
int otvm_gn_stats(const float* x, int64_t P, int C, int ld, double* stats, void* stream);
/* per-channel scale / shift of the same normalisation (scale = rstd*gamma, shift = beta - mean*scale), for
 * otvm_conv_params.in_scale / in_shift: identical arithmetic to otvm_gn_apply's                                   */
int otvm_gn_table(const double* stats, int64_t P, int C, const float* gamma, const float* beta, float* scale,
                  float* shift, void* stream);
/* res_scale / res_shift (optional, tables from otvm_gn_table): the residual is itself a raw GroupNorm input whose apply
 * pass was skipped; it is normalised on the fly, residual' = res_act(residual * res_scale[c] + res_shift[c]).        */
int otvm_gn_apply(const float* x, int64_t P, int C, int ld, const double* stats, const float* gamma,
                  const float* beta, const float* residual, int res_ld, const float* res_scale, const float* res_shift,
                  int res_act, int act, float* out, int out_ld, void* stream);

/* Batched forms (ABI 11): the same normalisation applied to `batch` images in one launch -- per-image statistics
 * (GroupNorm is per sample), shared gamma / beta.  Image b of x / out / residual lives *_bs floats behind image 0, its
 * [32][2] statistics block stats_bs doubles, its scale / shift tables norm_bs floats.  batch = 1 == the calls above. */
int otvm_gn_stats_b(const float* x, int64_t P, int C, int ld, double* stats, int batch, int64_t x_bs, int stats_bs, void* stream);
int otvm_gn_table_b(const double* stats, int64_t P, int C, const float* gamma, const float* beta, float* scale, float* shift,
                    int batch, int stats_bs, int norm_bs, void* stream);
typedef struct {
    const float* x; int64_t P; int C, ld; const double* stats; const float* gamma; const float* beta;
    const float* residual; int res_ld; const float* res_scale; const float* res_shift; int res_act, act;
    float* out; int out_ld;
    int batch; int64_t x_bs, res_bs, out_bs; int stats_bs, norm_bs;
} otvm_gn_apply_params;
int otvm_gn_apply_b(const otvm_gn_apply_params* p, void* stream);

/* ---- GroupNorm statistics of a 1x1 convolution's output, PREDICTED from its input (ABI 17; csrc/gram.hip) ------------
 * FBA bottleneck tail (resnet_GN_WS.py:66-86): out = relu(GroupNorm(conv3(x')) + identity), x' = relu(GroupNorm(conv2 ...)).
 * y = W x' is linear, so the sums the GroupNorm of y needs follow from the input:  sum y = v_g . s,  sum y^2 = <G, M_g>  with
 * s = sum_p x'_p, G = sum_p x'_p x'_p^T (this call) and v_g = sum_{c in g} w_c, M_g = sum_{c in g} w_c w_c^T (per checkpoint).
 * otvm_gram_f16 : x = the RAW GroupNorm input of x' ([P][ld] fp32, C channels), in_scale / in_shift / in_act = its folded
 *                 normalisation (tables of otvm_gn_table; NULL = x is x' already).  Writes per pixel chunk k (nk =
 *                 otvm_gram_chunks(P, C, &pch) chunks of pch pixels) the block-upper-triangular partial Gram matrix
 *                 gpart[k][blk][bs*bs] (bs = otvm_gram_block(C); blocks (bi <= bj) row-major; otvm_gram_entries(C) floats per
 *                 chunk) and the partial channel sums spart[k][C].  passes = 1: operands rounded to fp16 (round to nearest;
 *                 the statistics average the rounding noise out), 3: the f16x3 split of the convolutions.
 * otvm_gn_predict: adds the partials in fp64, contracts them with Mp[32][entries] (fp32, group-major; off-diagonal blocks
 *                 carrying the factor 2 of the symmetric half) and v[32][C] (fp64), and writes  scale_eff[c] = wscale[c] * rstd_g * gamma[c],
 *                 bias_eff[c] = beta[c] - mean_g * rstd_g * gamma[c] (+ res_shift[c])  -- the values the consuming conv takes
 *                 as otvm_conv_params.w_scale / bias.  ws = batch * otvm_gn_predict_ws_bytes() of workspace (per-workgroup partial
 *                 sums, added in a fixed order by the last workgroup: deterministic), counter = zeroed uint32 per image (left
 *                 zeroed); stat_out (optional) receives (mean, rstd) per group.  Batched like otvm_gn_*_b.                     */
typedef struct otvm_gram_params {
    const float* x; int64_t P; int C, ld;
    const float* in_scale; const float* in_shift; int in_act;
    float* gpart; float* spart; int passes;
    int batch; int64_t x_bs; int norm_bs;            /* image b: x + b * x_bs, tables + b * norm_bs; partials are packed per image */
    unsigned* diag;                                  /* ABI 18, optional: the layer's two diagnostic words (see otvm_gn_predict_params);
                                                        this kernel sets bit 1 of diag[1] when an operand was clamped to +-65504   */
} otvm_gram_params;
int otvm_gram_block(int C);
int64_t otvm_gram_entries(int C);
int otvm_gram_chunks(int64_t P, int C, int* pch_out);
int otvm_gram_f16(const otvm_gram_params* p, void* stream);
typedef struct otvm_gn_predict_params {
    const float* gpart; const float* spart; int64_t P; int C, Cout;
    const float* Mp; const double* v; void* ws; unsigned* counter;
    const float* wscale; const float* gamma; const float* beta; const float* res_shift;
    float* scale_eff; float* bias_eff; float* stat_out;
    int batch, tab_bs, rs_bs;                        /* image b: tables + b * tab_bs floats, res_shift + b * rs_bs floats */
    unsigned* diag;                                  /* ABI 18, optional, two words the host clears and reads: diag[0] = running maximum
                                                        (atomicMax of float bits) of kappa = mean^2 / var over groups, images and
                                                        launches -- the factor by which the Gram matrix's rounding error reaches the
                                                        variance; diag[1] bit 0 = a statistic was not finite                         */
} otvm_gn_predict_params;
int64_t otvm_gn_predict_ws_bytes(void);
int otvm_gn_predict(const otvm_gn_predict_params* p, void* stream);

/* ---------------------------------------------------------------- pooling / resampling ---------*/
/* F.max_pool2d(3, 2, 1) (resnet_GN_WS.py:98, torchvision resnet maxpool in STM.py:47,83) */
int otvm_maxpool3x3s2(const float* in, int H, int W, int C, int ld, float* out, int out_ld, void* stream);
/* F.interpolate(mode='bilinear', align_corners=False) to (Ho,Wo); out = up(in) [+ add]
 * (FBA/models.py:358-376, STM.py:115) */
/* in_scale / in_shift (optional, tables from otvm_gn_table): the GroupNorm apply of the input folded into the resampling,
 * in' = in_act(in * in_scale[c] + in_shift[c]) per source pixel (FBA/models.py:364-376: GN + LeakyReLU, then interpolate). */
int otvm_upsample_bilinear(const float* in, int Hi, int Wi, int C, int in_ld, const float* in_scale, const float* in_shift,
                           int in_act, const float* add, int add_ld, float* out, int Ho, int Wo, int out_ld, void* stream);
/* batched forms (ABI 11): `batch` images per launch, image b lives *_bs floats behind image 0 (norm_bs: the tables) */
int otvm_maxpool3x3s2_b(const float* in, int H, int W, int C, int ld, float* out, int out_ld, int batch, int64_t in_bs,
                        int64_t out_bs, void* stream);
int otvm_upsample_bilinear_b(const float* in, int Hi, int Wi, int C, int in_ld, const float* in_scale, const float* in_shift,
                             int in_act, const float* add, int add_ld, float* out, int Ho, int Wo, int out_ld, int batch,
                             int64_t in_bs, int64_t add_bs, int64_t out_bs, int norm_bs, void* stream);
/* nn.AdaptiveAvgPool2d(s) for s in {1,2,3,6} in one launch (FBA/models.py:300-306);
 * out = 50 bins x C, bins ordered scale-major then row-major.
 * ws >= otvm_ppm_pool_ws_bytes(H, C): per-row sums of the 12 column bins (one pass over the map, then a
 * fixed-order reduction over the rows of every bin).                                                */
int64_t otvm_ppm_pool_ws_bytes(int H, int C);
int otvm_ppm_pool(const float* in, int H, int W, int C, int ld, float* out, void* ws, void* stream);

/* The four PPM heads behind the pooling (FBA/models.py:298-307: L.Conv2d(2048, 256, 1, bias) -> GroupNorm(32) ->
 * LeakyReLU on each pooled map) in one launch.  pooled = otvm_ppm_pool's output [50][C]; w[i] = packed fp32 weight of
 * branch i ([>= 256 rows][K_pad], weight standardisation already applied by otvm_pack_conv_weight), bias[i] optional;
 * out[i] = [s*s][out_ld] (s = 1, 2, 3, 6), normalised and activated -- ready for otvm_upsample_bilinear.           */
typedef struct otvm_ppm_head_params {
    const float* pooled; int C, K_pad, Cout;
    const float* w[4]; const float* bias[4]; const float* gamma[4]; const float* beta[4];
    float* out[4]; int out_ld, act;
} otvm_ppm_head_params;
int otvm_ppm_head(const otvm_ppm_head_params* p, void* stream);

/* The PPM branches' share of conv_up1.0 (FBA/models.py:358-365: 3x3 conv over cat[layer4, 4 upsampled PPM maps]) WITHOUT
 * materialising the upsampled maps: convolution and bilinear interpolation are linear, so
 *   otvm_ppm_conv_z  : Z[tap][j][o] = sum_c w_ppm[scale(j)][tap][c][o] * y_scale[j][c]  for the 50 pooled pixels j (otvm_ppm_head's
 *                      outputs y[4], pixel stride y_ld, 256 channels) and the 9 taps; w_ppm fp32 [4][9][256 c][256 o]; Z [9][50][256];
 *   otvm_ppm_conv_add: out[p][o] += sum_tap [p + tap inside HxW] sum_scale bilinear_up(Z[tap][scale])(p + tap)   (256 channels).
 * Identical to the reference's conv(cat(...)) restricted to the PPM channels up to fp32 summation order.                 */
int otvm_ppm_conv_z(const float* const* y, int y_ld, const float* w_ppm, float* Z, void* stream);
int otvm_ppm_conv_add(const float* Z, int H, int W, float* out, int out_ld, double* gn_stats, void* stream);
                                  /* gn_stats (optional, zeroed [32][2] fp64): GroupNorm(32) sums of the FINAL out, as otvm_conv_params.gn_stats */

/* ---------------------------------------------------------------- memory read (STM.py:140-163) -
 * mem[q, :] = sum_m softmax_m(K[m,:].Q[q,:] / sqrt(128)) V[m,:], m over T slots x hw positions.
 * Flash-style: one partial (max, sum, acc) per (query tile, slot), merged by a combine kernel;
 * the [T*hw, hw] probability matrix of the reference is never materialised.
 *   keys[t] : [hw,128] fp32, vals[t] : [hw,512] fp32 (device pointer tables live on the HOST)
 *   out     : [hw, 512] view with pixel stride out_ld (the first half of the 1024-ch m4 tensor)
 *   ws      : workspace >= otvm_memory_read_ws_bytes(hw, T) bytes                                 */
int64_t otvm_memory_read_ws_bytes(int hw, int T);
int otvm_memory_read(const float* q_key, int q_ld, const float* const* keys, const float* const* vals, int T,
                     int hw, float* out, int out_ld, void* ws, void* stream);

/* f16x3 variant (fp32-class accuracy on the f16 MFMA, see OTVM_PREC_F16X3).  The bank is this build's own
 * structure, so each slot is stored split (fp16 hi/lo) and in MFMA fragment order: otvm_bank_pack_f16x3
 * converts the fp32 key [hw,128] / value [hw,512] maps of a memorised frame (the KV_M_r4 conv outputs,
 * STM.py:201-228) into one packed slot of otvm_bank_slot_bytes_f16x3(hw) bytes; the read kernel streams
 * slots with coalesced 1-KiB wave loads directly into MFMA operands.  ws as otvm_memory_read.            */
int64_t otvm_bank_slot_bytes_f16x3(int hw);
int otvm_bank_pack_f16x3(const float* key, const float* val, int hw, void* slot, void* stream);
int otvm_memory_read_f16x3(const float* q_key, int q_ld, const void* const* slots, int T, int hw, float* out,
                           int out_ld, void* ws, void* stream);

/* The same read in two steps, for a caller that knows part of the bank earlier than the rest (the engine reads the slots
 * that are already resident on a side stream, under the previous frame's alpha network, and only the slot of the frame
 * just memorised on the critical path): the softmax over the memory axis is merged from per-chunk partials (running
 * max, sum, weighted value sum), so the bank may be visited in any grouping.  A workspace laid out for np_cap partials
 * holds np_cap * hw * (512 + 2) floats; a group of n slots writes otvm_memory_read_f16x3_partial_count(n, hw) partials
 * starting at part0 (*part_end = one past its last); combine merges partials [0, n_partials) into out.             */
int otvm_memory_read_f16x3_partial_count(int n_slots, int hw);
int otvm_memory_read_f16x3_partial(const float* q_key, int q_ld, const void* const* slots, int n_slots, int hw, void* ws,
                                   int np_cap, int part0, int* part_end, void* stream);
int otvm_memory_read_f16x3_combine(const void* ws, int np_cap, int n_partials, int hw, float* out, int out_ld, void* stream);

/* ---------------------------------------------------------------- frame glue --------------------
 * preprocess: alpha/model.py:380-389,408-414 + STM.py:53-57,89-93.  fg,bg: [3,H,W] fp32 BGR 0..255
 * planes; a: [H,W] in [0,1].  Writes the zero-padded 0..1 RGB composite and its normalised copies
 * into channel slices of the consumers' input buffers and the un-padded `scaled_imgs` [3,H,W].
 * Every destination (scaled_imgs, x11, sq, sm, d80) is optional: NULL = not written by this call.  */
typedef struct {
    const float* fg; const float* bg; const float* a;
    int H, W, Hp, Wp, lh, lw;
    float mean[3], std[3];        /* IMG_MEAN / IMG_STD                    */
    float mean_q[3], std_q[3];    /* trimap.model.Encoder_Q.mean / std     */
    float mean_m[3], std_m[3];    /* trimap.model.Encoder_M.mean / std     */
    float* scaled_imgs;           /* [3,H,W] planar RGB 0..1 (returned)    */
    float* x11; int x11_ld;       /* ch0-2 <- normalised                   */
    float* sq;  int sq_ld;        /* ch0-2 <- Encoder_Q normalised         */
    float* sm;  int sm_ld;        /* ch0-2 <- Encoder_M normalised         */
    float* d80; int d80_ld;       /* ch64-66 <- normalised, ch67-69 <- 0..1 */
    const unsigned char* fg_u8;   /* optional: decoded frames as uint8 [H,W,3] (interleaved, what an image decoder  */
    const unsigned char* bg_u8;   /* hands out); when set, fg / bg are ignored.  float(uint8) == the reference's     */
    int u8_rgb;                   /* .float() of the same pixels; u8_rgb != 0: channels are R,G,B instead of B,G,R   */
} otvm_preprocess_params;
int otvm_preprocess(const otvm_preprocess_params* p, void* stream);

/* pad a [3,H,W] one-hot/soft trimap to [3,Hp,Wp] (bg plane padded with 1, others 0;
 * alpha/model.py:410) */
int otvm_pad_trimap(const float* tri, int H, int W, float* out, int Hp, int Wp, int lh, int lw, void* stream);

/* STM decoder tail: x4 bilinear upsample of the [h4*w4,3] logits (ld) + softmax over the 3 classes
 * -> planar probs [3,Hp,Wp] (STM.py:136, alpha/model.py:440) */
int otvm_upsample4_softmax3(const float* logits, int h4, int w4, int ld, float* probs, void* stream);

/* User labels over the propagated trimap, between the STM decoder's softmax and the encoding (an extension of
 * alpha/model.py:425-443, where the reference takes a trimap on the first frame only and feeds every later frame the
 * propagated softmax as it is): wherever labels[y][x] is a class -- 0 bg, 1 unknown, 2 fg -- the three planes of
 * probs [3,Hp,Wp] at (lh + y, lw + x) become that class's exact one-hot (1.f / 0.f).  Every other label value (255 =
 * unlabelled by convention) and the padding border keep the bits they hold.  labels: uint8 [H,W].  One pass, 16-byte
 * stores (probs 16-byte aligned, Wp % 4 == 0); a group of four pixels without a label costs its four label bytes.       */
int otvm_trimap_apply_labels(float* probs, const uint8_t* labels, int H, int W, int Hp, int Wp, int lh, int lw, void* stream);

/* 8-channel trimap encoding (alpha/model.py:40-53, utils/utils.py:12-39): argmax class map, exact
 * Euclidean distance transform of the bg / fg classes on device (integer d^2), three Gaussians each,
 * plus the two soft channels.  probs: planar [3,Hp,Wp].  Writes x11 ch3-10 and d80 ch70-71.
 *   cls_override: optional u8 class map [Hp*Wp] used INSTEAD of the argmax (tests only), may be NULL
 *   cls_out     : u8 class map [Hp*Wp] (always written)
 *   ws          : workspace >= otvm_trimap_encode_ws_bytes(Hp,Wp)                                  */
int64_t otvm_trimap_encode_ws_bytes(int Hp, int Wp);
int otvm_trimap_encode(const float* probs, int Hp, int Wp, const uint8_t* cls_override, uint8_t* cls_out,
                       float* x11, int x11_ld, float* d80, int d80_ld, void* ws, void* stream);

/* FBA / refinement heads: 1x1 conv 16->7 (+3 trimap logits when n_out==10), clamp/sigmoid and
 * fba_fusion (FBA/models.py:279-288,383-388,425-432), softmax of the trimap logits
 * (alpha/model.py:460).  hid: [P,16] view (ld).  img: [P,3] view (0..1 RGB).
 *   alpha_out/alpha_stride : fused alpha written at alpha_out[p*alpha_stride]
 *   tri_out  : planar [3,P] softmax probs (n_out==10) or NULL
 *   sm       : Encoder_M input buffer; ch3 <- p_un, ch4 <- p_fg, ch5 <- alpha (n_out==10) or NULL */
int otvm_fba_head(const float* hid, int hid_ld, const float* w, const float* b, int n_out, const float* img,
                  int img_ld, int64_t P, float* alpha_out, int alpha_stride, float* tri_out, float* sm, int sm_ld,
                  void* stream);
/* ... keeping the clamped fused F as well: fgr planar [3][P], R, G, B (see the _fgr form of the fused layer above)     */
int otvm_fba_head_fgr(const float* hid, int hid_ld, const float* w, const float* b, int n_out, const float* img,
                      int img_ld, int64_t P, float* alpha_out, int alpha_stride, float* tri_out, float* sm, int sm_ld,
                      float* fgr, void* stream);

/* crop the padding and produce the returned tensors (alpha/model.py:495-508, eval.py:209):
 * alpha [H,W] fp32, alpha_u8 [H,W] = trunc(alpha*255) (may be NULL), trimap [3,H,W] (may be NULL) */
int otvm_crop_outputs(const float* alpha_p, const float* tri_p, int Hp, int Wp, int H, int W, int lh, int lw,
                      float* alpha, uint8_t* alpha_u8, float* tri, void* stream);

/* Foreground outputs of one frame in one pass: reads the padded alpha plane and the three padded F planes once and writes
 * whichever outputs are requested (NULL = not written).  All arithmetic is fp32, one IEEE operation per step (no contraction):
 *   fgr      [3,H,W] fp32, R, G, B : F cropped, unchanged
 *   rgba_u8  [H,W,4] : colour = q(F), A = q(alpha), q(v) = (uint8) min(max(trunc(v * 255.f), 0), 255) -- for alpha in [0,1] the
 *                      byte otvm_crop_outputs writes as alpha_u8.  Straight (not premultiplied) alpha
 *   comp_u8  [H,W,3] : bgf = (float)bg * (1.f / 255.f); c = (F * a) + (bgf * (1.f - a)); byte = q(c)
 * A non-finite operand (F, alpha, or the composite c) gives byte 0 (converting NaN to an integer is undefined in C; here it is
 * an explicit select).  bg_u8 = uint8 [H,W,3] of the frame's resolution, or NULL: the solid colour bg_color.  The three colour
 * bytes of rgba_u8 / comp_u8, bg_u8 and bg_color are in B, G, R order (u8_rgb == 0, as decoded frames are) or R, G, B
 * (u8_rgb != 0), as otvm_preprocess_params.u8_rgb has it.  No atomics: two calls give equal bits.                           */
typedef struct otvm_fgr_params {
    const float* alpha_p;         /* padded fused alpha [Hp*Wp] (needed for rgba_u8 / comp_u8)                    */
    const float* fgr_p;           /* padded F planes [3][Hp*Wp], R, G, B                                          */
    int Hp, Wp, H, W, lh, lw;     /* padded size, output size, top / left padding                                 */
    float* fgr;
    unsigned char* rgba_u8;
    unsigned char* comp_u8;
    const unsigned char* bg_u8;
    unsigned char bg_color[3];
    int u8_rgb;
} otvm_fgr_params;
int otvm_fgr_outputs(const otvm_fgr_params* p, void* stream);

/* ---------------------------------------------------------------- working-resolution matting ----
 * The network runs on a reduced copy of the frame (integer scale s = 2, 3, 4; working size h = ceil(H / s), w = ceil(W / s)) and
 * its outputs return to the frame's resolution through the colour-guide fast guided filter (He & Sun).  Everything below is
 * restated operation by operation in tests/guided_ref.py; the kernels use no atomics, so two calls give equal bits.
 *
 * Reductions (integer arithmetic):
 *   otvm_downsample_u8     uint8 [H,W,3] -> [h,w,3]: mean of the s x s block, clipped at the bottom / right edge to its n
 *                          source pixels: byte = (sum + n / 2) / n
 *   otvm_downsample_trimap planar one-hot float [3,H,W] (bg, unknown, fg) -> [3,h,w], conservative: fg only if plane 2 is 1.f
 *                          on every pixel of the block, bg only if plane 0 is; otherwise unknown (a block for which both hold
 *                          is not one-hot input: unknown).  The unknown band never shrinks
 *   otvm_downsample_labels uint8 [H,W] (0 bg, 1 unknown, 2 fg, else unlabelled) -> [h,w]: 255 if any pixel of the block is not
 *                          a class, the common class if all agree, otherwise 1 (unknown)                                    */
int otvm_downsample_u8(const uint8_t* src, int H, int W, int s, uint8_t* dst, void* stream);
int otvm_downsample_trimap(const float* src, int H, int W, int s, float* dst, void* stream);
int otvm_downsample_labels(const uint8_t* src, int H, int W, int s, uint8_t* dst, void* stream);

/* Guided filter.  otvm_guided_coeffs (working resolution): window (2r+1)^2, r = 1..4, clipped at the borders to its N pixels.
 * Each target is quantised once, P = (int)(min(max(p, 0), 1) * 65535.f + 0.5f), so the window sums of I_c, I_c I_d, P and
 * I_c P are exact 32-bit integers.  Per pixel in fp64, one IEEE operation per step:
 *   s_cd = (N sum(I_c I_d) - sum(I_c) sum(I_d)) / (N N 65025) [+ eps on the diagonal]
 *   p_c  = (N sum(I_c P) - sum(I_c) sum(P)) / (N N 255 65535)
 *   adjugate of the symmetric s: c00 = s11 s22 - s12 s12, c01 = s02 s12 - s01 s22, c02 = s01 s12 - s02 s11,
 *                                c11 = s00 s22 - s02 s02, c12 = s01 s02 - s00 s12, c22 = s00 s11 - s01 s01
 *   det = (s00 c00 + s01 c01) + s02 c02;  a_i = ((c_i0 p_0 + c_i1 p_1) + c_i2 p_2) / det
 *   b = (sum(P) / N) / 65535 - ((a_0 m_0 + a_1 m_1) + a_2 m_2),  m_c = (sum(I_c) / N) / 255
 * (a constant target gives a = 0 and b = P / 65535 exactly).  (a_0, a_1, a_2, b) is rounded to fp32 into ws [h,w,C,4]; coef
 * [h,w,C,4] receives its box mean over the same clipped window: fp64 sums of rows in ascending x, then of columns in ascending y,
 * divided by N, rounded to fp32.  ws: otvm_guided_ws_bytes(h, w, C) bytes, 16-byte aligned, no initialisation (it holds the
 * un-averaged coefficients afterwards); one ws serves one stream at a time.
 * otvm_guided_apply (full resolution, fp32, one IEEE operation per step): per pixel (X, Y) the mean coefficients are looked up
 * bilinearly with half-pixel centres -- t = 2X + 1 - s, x0 = floor(t / 2s), fx = (float)(t - 2s x0) / (float)(2s), x0 and x0 + 1
 * clamped to [0, w-1], rows alike; v = top + fy * (bot - top) with top = c00 + fx * (c01 - c00), bot = c10 + fx * (c11 - c10) --
 * then q = ((a_0 I_0 + a_1 I_1) + a_2 I_2) + b with I = (float)byte * (1.f / 255.f), clamped: q < 0 ? 0 : (q > 1 ? 1 : q); a NaN q
 * (non-finite coefficients: an eps too small for a constant guide region) gives 0 by an explicit select.
 * Target 0 goes to alpha [H,W] and alpha_u8 [H,W] = (uint8)(alpha * 255.f) (truncation, as otvm_crop_outputs; may be NULL),
 * targets 1..3 (C = 4: the F planes) to fgr [3,H,W].  RGBA / composite bytes: otvm_fgr_outputs on these with Hp = H, Wp = W,
 * lh = lw = 0.  The guide's three bytes are used in the order they are stored, in both calls.                            */
typedef struct otvm_guided_params {
    int H, W, s, h, w;            /* full size, scale (2, 3, 4), working size (ceil(H / s), ceil(W / s))                  */
    int r, C;                     /* window radius 1..4; targets: 1 (alpha) or 4 (alpha + F)                              */
    double eps;                   /* regulariser on the [0,1] scale, > 0                                                  */
    const uint8_t* guide_full;    /* uint8 [H,W,3]: the frame (apply)                                                     */
    const uint8_t* guide_work;    /* uint8 [h,w,3]: the working frame the network saw (coeffs)                            */
    const float* target[4];       /* C planes [h,w] fp32 (coeffs)                                                         */
    float* coef;                  /* [h,w,C,4] fp32, 16-byte aligned: written by coeffs, read by apply                    */
    float* alpha;                 /* outputs of apply                                                                     */
    uint8_t* alpha_u8;
    float* fgr;
} otvm_guided_params;
int64_t otvm_guided_ws_bytes(int h, int w, int C);      /* -1 for an empty image or C not in {1, 4} */
int otvm_guided_coeffs(const otvm_guided_params* p, void* ws, void* stream);
int otvm_guided_apply(const otvm_guided_params* p, void* stream);

/* first-frame trimap from a GT alpha (alpha/model.py:342-362): unknown = dilate(0<a<1) with a
 * (2r+1)^2 max filter, fg = (a==1), bg = (a==0); out planar one-hot [3,H,W]; ws >= H*W bytes      */
int otvm_trimap_from_alpha(const float* a, int H, int W, int r, float* out, void* ws, void* stream);

/* Trimap from a segmentation mask: exact erosion of the thresholded mask by Euclidean discs (an extension; the reference
 * derives trimaps from ground-truth alpha only, which gives a binary mask no unknown band).  Integers throughout.
 *   FG = (m >= hi), BG = (m <= lo) for the mask m, uint8 [H,W], 0 <= lo < hi <= 255;
 *   d_S(p) = min over the in-image pixels q not in S of |p - q|^2 (an exact integer; +inf when every pixel is in S).  Pixels
 *   outside the image belong to no set and seed nothing: a subject cut by the frame edge stays foreground up to the edge;
 *   fg = FG and d_FG > t_fg, bg = BG and d_BG > t_bg, everything else is unknown.  t = floor(r^2) for a band of r pixels,
 *   r = 0 ... 255; t = 0 gives the thresholded mask (unknown only where lo < m < hi).
 * Only the comparison with t matters, so with R = floor(sqrt(t)) the search is bounded: the vertical distance g to the nearest
 * non-member of the pixel's column, capped (any cap above R serves: 256 here), then per row the minimum over |dx| <= R of
 * g^2 + dx^2.  Two launches, no atomics (two calls give equal bits), nothing launched when an argument is refused.
 *   trimap : planar one-hot [3,H,W] (bg, unknown, fg), the layout of otvm_trimap_from_alpha's output, or NULL;
 *   labels : uint8 [H,W], 0 bg, 2 fg and band_label elsewhere -- 1 (unknown) or 255 (unlabelled: what
 *            otvm_trimap_apply_labels leaves alone, so a propagated trimap survives in the band) -- or NULL; one of the two
 *            outputs at least;
 *   ws     : otvm_trimap_from_mask_ws_bytes(H, W) bytes, 2-byte aligned, no initialisation; one ws serves one stream at a time.
 * New symbols only (additive, as the entries above): the ABI number stays.                                                   */
typedef struct otvm_mask_trimap_params {
    const uint8_t* mask;      /* [H,W] */
    int H, W, lo, hi;         /* 1 <= H, W < 16384; 0 <= lo < hi <= 255 */
    int t_fg, t_bg;           /* 0 .. 65025 */
    float* trimap;            /* planar one-hot [3,H,W] (bg, unknown, fg), or NULL */
    uint8_t* labels;          /* [H,W]: 0 bg, 2 fg, band_label elsewhere, or NULL */
    int band_label;           /* 1 (unknown) or 255 (unlabelled) */
} otvm_mask_trimap_params;
int64_t otvm_trimap_from_mask_ws_bytes(int H, int W);      /* -1 for bad sizes */
int otvm_trimap_from_mask(const otvm_mask_trimap_params* p, void* ws, void* stream);

/* one-hot of the argmax of a planar [3,H,W] trimap (alpha/model.py:356-362, returned tri_gt) */
int otvm_onehot_argmax3(const float* tri, int64_t P, float* out, void* stream);

/* ---------------------------------------------------------------- metrics ------
 * SAD / MSE / dtSSD partial sums of one frame (reference utils/tmp/metric.py:177-189,252-264) on 8-bit alphas
 * [n] = trunc(alpha*255) (eval.py:209); mask (unknown band) and the prev_* pointers may be NULL.  acc[5] (fp64,
 * caller-zeroed) accumulates  sum|p-t|m, sum(p-t)^2 m, sum m, sum((p-p')-(t-t'))^2 m', sum m'  -- integer-exact. */
int otvm_matting_metrics(const uint8_t* pred, const uint8_t* target, const uint8_t* mask, const uint8_t* prev_pred,
                         const uint8_t* prev_target, const uint8_t* prev_mask, int64_t n, double* acc, void* stream);
/* Grad and Conn of one frame (reference utils/tmp/metric.py:16-46,191-234) on the same 8-bit alphas and optional {0,1} mask
 * (NULL = all pixels).  acc[2] (fp64, caller-zeroed) accumulates  Grad = sum (|grad p| - |grad t|)^2 m  (9x9 Gaussian
 * derivative of sigma 1.4, replicate padding) and  Conn = sum |phi_p - phi_t| m  (10 thresholds, largest 4-connected
 * component of each, ties to the component with the smallest first raster index).  level_map (optional, uint8 [H,W])
 * receives each pixel's Conn level: k for t_k = float32 0.1 k, 10 for 1.0.  ws: otvm_matting_grad_conn_ws_bytes(H, W)
 * bytes of device memory, no initialisation needed; one ws serves one stream at a time.                            */
int otvm_matting_grad_conn(const uint8_t* pred, const uint8_t* target, const uint8_t* mask, int H, int W, double* acc,
                           uint8_t* level_map, void* ws, void* stream);
int64_t otvm_matting_grad_conn_ws_bytes(int H, int W);
/* host-side constants of the kernel above: cutoffs[10] = c_i (pred, target >= c_i <=> x/255.f >= t_i, i = 1..10),
 * levels[11] = t_k as float32, taps[18] = the L2-normalised 1-D Gaussian [9] and Gaussian-derivative [9] factors of hx.
 * Any pointer may be NULL.                                                                                           */
int otvm_matting_grad_conn_params(int* cutoffs, float* levels, double* taps);
/* Dense optical flow of two uint8 [H,W] frames: OpenCV's calcOpticalFlowFarneback(prev, next, None, 0.5, 5, 10, 2, 7, 1.5,
 * OPTFLOW_FARNEBACK_GAUSSIAN), the reference's calcOpticalFlow (utils/tmp/metric.py:48-53).  flow: float [H,W,2] = (dx, dy).
 * ws: otvm_optflow_farneback_ws_bytes(H, W) bytes of device memory, no initialisation; one ws serves one stream at a time.
 * Any H in 1..65535 and W >= 1; deterministic (no atomics).                                                          */
int otvm_optflow_farneback(const uint8_t* prev, const uint8_t* next, int H, int W, float* flow, void* ws, void* stream);
int64_t otvm_optflow_farneback_ws_bytes(int H, int W);
/* host-side constants for (H, W); returns the number of pyramid levels n (<= 6), in processing order (coarsest first):
 * levels[4n] = (k, width, height, GaussianBlur ksize), blur_taps[79n] = each level's float32 kernel (zero padded),
 * poly_taps[24] = g[0..7], xg[0..7], xxg[0..7] of FarnebackPolyExp(7, 1.5), poly_inv[4] = ig11, ig03, ig33, ig55,
 * win_taps[6] = the 11-tap flow window kernel, centre first.  Any pointer may be NULL; -1 for H or W < 1.             */
int otvm_optflow_farneback_params(int H, int W, int* levels, float* blur_taps, float* poly_taps, double* poly_inv, float* win_taps);
/* MESSDdt of one pair of frames (metric.py:266-302): the flow of (t0, t1) as above, rounded half to even, and the
 * reference's TRANSPOSED lookup -- pixel (r, c) of frame 1 is read at row clamp(c + dx, 0, H-1), column clamp(r + dy, 0, W-1).
 * acc[2] (fp64, caller-zeroed) accumulates  sum |(p0-t0)^2 m0 - (p1w-t1w)^2 m1w|  (0..255 integers: error * 255^2, exact)
 * and  sum m0.  Masks {0,1} or NULL (all pixels).  flow_out (optional, float [H,W,2]) receives the flow.
 * ws: otvm_optflow_farneback_ws_bytes(H, W).                                                                         */
int otvm_matting_messddt(const uint8_t* p0, const uint8_t* t0, const uint8_t* m0, const uint8_t* p1, const uint8_t* t1,
                         const uint8_t* m1, int H, int W, double* acc, float* flow_out, void* ws, void* stream);

/* ---------------------------------------------------------------- temporal stabilisation of alpha ----------
 * A causal, one-frame-state, motion-compensated recursive filter of alpha (an extension; the reference mattes every frame on
 * its own).  The defaults of otvm_amd/temporal.py are PLACEHOLDERS: there is no trained checkpoint here, the filter is checked
 * by definition and by property on synthetic clips, not by quality on real footage.  New symbols only (additive, as the
 * entries above): the ABI number stays.
 *
 * otvm_luma_u8: img uint8 [H,W,3] -> grey uint8 [H,W] = (B*1868 + G*9617 + R*4899 + 8192) >> 14 (integer: OpenCV's BGR2GRAY);
 * u8_rgb says which byte is R, as otvm_preprocess_params.u8_rgb does.  H in 1..65535, W >= 1.
 *
 * otvm_temporal_blend, per pixel (x, y), fp32, one IEEE operation per step, no atomics (two calls give equal bits):
 *   sx = (float)x + dx, sy = (float)y + dy with (dx, dy) = flow[y][x]: the flow from this frame to the previous one
 *        (otvm_optflow_farneback(prev = grey, next = grey_prev)).  ok = 0 <= sx <= W-1 && 0 <= sy <= H-1 (NaN and inf fail);
 *        when !ok nothing is gathered and w = 0.
 *   bilinear sample at (sx, sy): x0 = floorf(sx), fx = sx - x0, x1 = min(x0 + 1, W-1), likewise y;
 *        top = ((1-fx)*v00) + (fx*v01), bot = ((1-fx)*v10) + (fx*v11), v = ((1-fy)*top) + (fy*bot);
 *        taken of prev, giving sw, and of (float)grey_prev, giving gw.
 *   wc = max(0, 1 - |(float)grey - gw| * inv_tau_colour)     the photometric residual, which doubles as the occlusion test
 *   wa = max(0, 1 - |a - sw| * inv_tau_alpha)                a real change of alpha is not smoothed away
 *   gate = 1 without tri; otherwise with (t0, t1, t2) = tri[.][min(y / tri_scale, th-1)][min(x / tri_scale, tw-1)]
 *        gate = (t1 > t0 && t1 >= t2): numpy's first-max argmax equal to 1 (the unknown class), NaN gives 0
 *   w = ((strength*wc)*wa)*gate;  o = a + (w * (sw - a));  out = min(max(o, 0), 1) (-0.0 and NaN give +0.0);
 *   out_u8 = (uint8) trunc(out * 255.f), the byte otvm_crop_outputs writes.  A non-finite a gives out = a, byte 0.
 * prev == NULL is the first frame of a clip: w = 0 everywhere (out = the clamped alpha and its byte); grey, grey_prev, flow
 * and tri are not read.  (float)x is exact for W <= 2^24.                                                                */
typedef struct otvm_temporal_params {
    int H, W;                       /* H in 1..65535, W >= 1 */
    const float* alpha;             /* [H,W]: this frame's raw alpha */
    const float* prev;              /* [H,W]: the previous STABILISED alpha, every value in [0,1]; NULL = first frame */
    const uint8_t* grey;            /* [H,W]: this frame's luma */
    const uint8_t* grey_prev;       /* [H,W]: the previous frame's luma */
    const float* flow;              /* [H,W,2] = (dx, dy) */
    const float* tri;               /* planar [3,th,tw] (bg, unknown, fg) or NULL */
    int th, tw, tri_scale;
    float strength;                 /* in [0,1] */
    float inv_tau_colour, inv_tau_alpha;   /* positive, finite; reciprocals taken on the host in fp32 */
    float* out;                     /* [H,W]; must not alias prev */
    uint8_t* out_u8;                /* [H,W] or NULL */
} otvm_temporal_params;
int otvm_luma_u8(const uint8_t* img, int H, int W, int u8_rgb, uint8_t* grey, void* stream);
int otvm_temporal_blend(const otvm_temporal_params* p, void* stream);

/* ---------------------------------------------------------------- region-of-interest matting ----------
 * Run the network in a window round the subject (an extension; otvm_amd/roi.py, run_video_matte(roi=...)): the boxes of a class
 * map, the crop of a frame's inputs to a window and the paste of the window's results into the frame.  Checked by definition only:
 * the result is the matte of the cropped clip pasted back, NOT the full-frame matte.  All three run on the caller's stream, never
 * synchronise with the host, and launch nothing when an argument is refused (nonzero; otvm_last_error() starts with the function's
 * name).  Sizes are 1 .. 16383 a side.  New symbols only (additive, as the entries above): the ABI number stays.
 *
 * otvm_trimap_bbox: out[0..3] = y0, x0, y1, x1 (inclusive) of the UNKNOWN pixels, out[4..7] the same of the NON-BACKGROUND pixels;
 * an empty set gives (H, W, -1, -1).  Exactly one source:
 *   trimap float [3,H,W] (one-hot or probabilities): non-bg iff max(t1, t2) > t0; unknown iff non-bg and t1 >= t2 (a NaN fails the
 *          comparison it stands in);
 *   labels uint8 [H,W]: 1 is unknown, 1 or 2 non-bg, every other value (0, 255) neither.
 * out needs no initialisation: the call first stores the empty boxes, then reduces per wave and workgroup and merges with
 * integer min / max atomics, which do not depend on the order of arrival -- two calls give equal bits.  out may be slot t of a
 * [T,8] buffer: only its own 8 words are touched, and a clip is read back with one copy.                                      */
typedef struct otvm_roi_bbox_params {
    const float* trimap;            /* [3,H,W] or NULL */
    const uint8_t* labels;          /* [H,W] or NULL */
    int H, W;
    int32_t* out;                   /* 8 words */
} otvm_roi_bbox_params;
int otvm_trimap_bbox(const otvm_roi_bbox_params* p, void* stream);

/* otvm_roi_crop: the h x w window at origin (y0, x0) of an H x W frame, one launch, every pair optional (a destination without
 * its source is refused, and so is a call with no destination): frame uint8 [H,W,3] -> [h,w,3], trimap float [3,H,W] -> [3,h,w],
 * labels uint8 [H,W] -> [h,w].  Pure copies; nothing is assumed about the alignment of a window row (any x0, any W).        */
typedef struct otvm_roi_crop_params {
    int H, W, y0, x0, h, w;         /* 0 <= y0, y0 + h <= H, 0 <= x0, x0 + w <= W */
    const uint8_t* frame;    uint8_t* frame_out;
    const float* trimap;     float* trimap_out;
    const uint8_t* labels;   uint8_t* labels_out;
} otvm_roi_crop_params;
int otvm_roi_crop(const otvm_roi_crop_params* p, void* stream);

/* otvm_roi_paste: a window's results back at H x W in one pass; every output is optional (at least one), every element of a
 * requested output is written.  fp32, one IEEE operation per step, no atomics (two calls give equal bits).
 *   inside the window : alpha, trimap and fgr are the window's values, unchanged;
 *                       alpha_u8 = (uint8) min(max(trunc(a * 255.f), 0), 255), the byte otvm_crop_outputs writes; a non-finite
 *                       alpha gives byte 0, as in otvm_fgr_outputs;
 *   outside           : trimap = `outside` at that pixel, or (1, 0, 0) when outside is NULL; alpha = 1.f where outside's fg plane
 *                       is 1.f, else 0.f (byte 255 / 0); fgr = (float)byte * (1.f / 255.f) of the frame's pixel, stored R, G, B
 *                       (u8_rgb says which byte is R, as otvm_preprocess_params.u8_rgb does).
 * fgr needs win_fgr and frame.  RGBA / composite bytes: otvm_fgr_outputs on the pasted planes with Hp = H, Wp = W.           */
typedef struct otvm_roi_paste_params {
    int H, W, y0, x0, h, w;         /* as otvm_roi_crop_params */
    const float* win_alpha;         /* [h,w] */
    const float* win_trimap;        /* [3,h,w] */
    const float* win_fgr;           /* [3,h,w] R, G, B, or NULL */
    const uint8_t* frame;           /* [H,W,3], or NULL without fgr */
    int u8_rgb;
    const float* outside;           /* one-hot [3,H,W] or NULL: everything outside the window is background */
    float* alpha;                   /* [H,W] */
    uint8_t* alpha_u8;              /* [H,W] */
    float* trimap;                  /* [3,H,W] */
    float* fgr;                     /* [3,H,W] R, G, B */
} otvm_roi_paste_params;
int otvm_roi_paste(const otvm_roi_paste_params* p, void* stream);

/* The tracking window (run_video_matte(roi="track")): the window's SIZE is fixed for a clip, its ORIGIN lives on the device, one
 * (y0, x0) row per frame of an int32 [T,2] log, so that no frame waits for a read-back.  New symbols only; the structs above are
 * taken as they are.
 *
 * otvm_roi_track: one small launch, integer arithmetic, no atomics, ordinary stores (two calls give equal bits); writes out[0..1].
 *   box  : the eight words otvm_trimap_bbox wrote for the NEIGHBOURING frame; words 4 .. 7 (non-background) decide.
 *   prev : the neighbour's origin (two words, clamped into the frame as read), the box then being in the neighbour's WINDOW; or
 *          NULL: the box is in FRAME coordinates and the window is centred on it, (y0 + y1 + 1) / 2 - h / 2 clamped to the frame
 *          (an empty box: (0, 0)).
 *   With prev, each axis on its own: it HOLDS prev while the box keeps at least `hold` pixels from both window sides on that axis
 *   (a window side that is the frame's side always counts as held) and recentres on the box, clamped, otherwise; an empty box
 *   holds both.  hold >= 1.  otvm_amd/roi.py track_origin is the same policy on the host; the two are equal by test.           */
typedef struct otvm_roi_track_params {
    const int32_t* box;             /* 8 words */
    const int32_t* prev;            /* 2 words or NULL */
    int32_t* out;                   /* 2 words: row t of the log */
    int H, W, h, w, hold;
} otvm_roi_track_params;
int otvm_roi_track(const otvm_roi_track_params* p, void* stream);

/* otvm_roi_crop_at / otvm_roi_paste_at: otvm_roi_crop / otvm_roi_paste with the window's origin read by the kernel from `origin`,
 * two int32 words on the device (a row of the log); p->y0 and p->x0 are not looked at.  What the kernel reads is CLAMPED to
 * [0, H - h] x [0, W - w] before any address is formed from it: a stale or unwritten row cannot address outside the frame.
 * 1 <= h <= H and 1 <= w <= W; every other refusal as in the forms above.  The kernel bodies are those of the forms above.   */
int otvm_roi_crop_at(const otvm_roi_crop_params* p, const int32_t* origin, void* stream);
int otvm_roi_paste_at(const otvm_roi_paste_params* p, const int32_t* origin, void* stream);

/* ---------------------------------------------------------------- multi-subject matting ----------
 * One clip, S subjects (an extension; otvm_amd/subjects.py, run_video_matte_subjects): every subject is followed by a tracking
 * window of its own, the S windows share ONE size h x w and go through the network as one lock-step batch.  These are the tracking
 * window's glue launches over S subjects at once -- the launches of a step do not grow with S -- and the one new pass, the resolve,
 * which pastes the S windows into the frame and settles the pixels where they overlap.  Conventions as above: the caller's stream,
 * no host synchronisation, nothing launched when an argument is refused (nonzero; otvm_last_error() starts with the function's
 * name), sides 1 .. 16383, S = 1 .. OTVM_SUBJECTS_MAX.  Per-subject BUFFERS are fixed arrays of 8 pointers (entries s >= S are not
 * looked at); per-subject ROWS of int32 words are `base + s * stride` (stride in words, any sign), so that one [S,T,10] log --
 * words 0 .. 7 the boxes of a frame's output trimap in its window, words 8, 9 the window's origin -- is indexed as it lies.  An
 * origin read from device memory is CLAMPED to [0, H - h] x [0, W - w] before any address is formed from it.  Checked by definition
 * only, like the tracking window.  New symbols only (additive, as the entries above): the ABI number stays.                   */
#define OTVM_SUBJECTS_MAX 8

/* otvm_subjects_track: otvm_roi_track for S subjects in one launch of 2 S threads: thread (s, axis) applies that policy to
 * box_base + s * box_stride (8 words), prev_base + s * prev_stride (2 words; prev_base NULL: every subject centres on its box,
 * which is then in frame coordinates) and writes out_base + s * out_stride (2 words).  Bit-equal to S otvm_roi_track calls.   */
typedef struct otvm_subjects_track_params {
    int S;
    const int32_t* box_base;   int box_stride;
    const int32_t* prev_base;  int prev_stride;     /* prev_base NULL: a step with a source */
    int32_t* out_base;         int out_stride;
    int H, W, h, w, hold;
} otvm_subjects_track_params;
int otvm_subjects_track(const otvm_subjects_track_params* p, void* stream);

/* otvm_subjects_crop: the frame uint8 [H,W,3] -> S windows [h,w,3] at the S origins (origin_base + s * origin_stride, 2 words),
 * and / or S trimaps float [3,H,W] -> [3,h,w] at the same origins, in ONE launch.  Pure copies: for every s bit-equal to
 * otvm_roi_crop_at.  A destination set is given for all s < S or for none; one of the two at least.                          */
typedef struct otvm_subjects_crop_params {
    int S, H, W, h, w;
    const int32_t* origin_base;  int origin_stride;
    const uint8_t* frame;                            /* [H,W,3], or NULL without frame_out */
    uint8_t* frame_out[OTVM_SUBJECTS_MAX];           /* [h,w,3] each, or all NULL */
    const float* trimap[OTVM_SUBJECTS_MAX];          /* [3,H,W] each, or NULL without trimap_out */
    float* trimap_out[OTVM_SUBJECTS_MAX];            /* [3,h,w] each, or all NULL */
} otvm_subjects_crop_params;
int otvm_subjects_crop(const otvm_subjects_crop_params* p, void* stream);

/* otvm_subjects_bbox: otvm_trimap_bbox of S float trimaps [3,H,W] (H x W here is the maps' own size) into the 8 words at
 * out_base + s * out_stride: two launches whatever S is (the empty boxes, then the reduction with integer min / max atomics).
 * For every s bit-equal to otvm_trimap_bbox.                                                                                  */
typedef struct otvm_subjects_bbox_params {
    int S, H, W;
    const float* trimap[OTVM_SUBJECTS_MAX];
    int32_t* out_base;  int out_stride;
} otvm_subjects_bbox_params;
int otvm_subjects_bbox(const otvm_subjects_bbox_params* p, void* stream);

/* otvm_subjects_resolve: the S windows' results at H x W in ONE sweep.  Every output is optional (at least one), every element
 * of a requested output is written; fp32, one IEEE operation per step, no atomics (two calls give equal bits).  Per pixel:
 *   a_s      = the window's alpha where the pixel lies in subject s's window, 0.f elsewhere (everything outside a tracking
 *              window is background, as otvm_roi_paste_at with outside == NULL);
 *   sum      = ((a_0 + a_1) + a_2) + ... in subject order;
 *   normalise != 0 and sum > 1.f: a_s = a_s / sum (correctly rounded; a NaN sum fails the comparison: nothing is rescaled);
 *   alpha[s] = a_s; alpha_u8[s] = otvm_roi_paste's byte of it (a non-finite alpha gives 0);
 *   trimap[s]= the window's trimap inside the window, (1, 0, 0) outside; never rescaled;
 *   fgr[s]   = the window's F inside the window, (float)byte * (1.f / 255.f) of the frame's pixel outside, stored R, G, B;
 *   union    = fminf(sum, 1.f) of the UNNORMALISED sum, union_u8 its byte;
 *   owner    = the smallest s whose written a_s is largest and > 0.f, 255 when there is none.
 * With normalise == 0 every per-subject plane is bit-equal to otvm_roi_paste_at of that subject.  The rule of `normalise` is an
 * untuned PLACEHOLDER.  fgr needs win_fgr for every s < S and the frame.                                                       */
typedef struct otvm_subjects_resolve_params {
    int S, H, W, h, w;
    const int32_t* origin_base;  int origin_stride;
    const float* win_alpha[OTVM_SUBJECTS_MAX];       /* [h,w] each */
    const float* win_trimap[OTVM_SUBJECTS_MAX];      /* [3,h,w] each */
    const float* win_fgr[OTVM_SUBJECTS_MAX];         /* [3,h,w] R, G, B each, or NULL without fgr */
    const uint8_t* frame;                            /* [H,W,3], or NULL without fgr */
    int u8_rgb, normalise;
    float* alpha;                                    /* [S,H,W] */
    uint8_t* alpha_u8;                               /* [S,H,W] */
    float* trimap;                                   /* [S,3,H,W] */
    float* fgr;                                      /* [S,3,H,W] R, G, B */
    float* union_alpha;                              /* [H,W] */
    uint8_t* union_u8;                               /* [H,W] */
    uint8_t* owner;                                  /* [H,W] */
} otvm_subjects_resolve_params;
int otvm_subjects_resolve(const otvm_subjects_resolve_params* p, void* stream);

/* ---------------------------------------------------------------- video streams: YUV <-> RGB ----------
 * 8-bit YUV as a decoder or a Y4M stream holds it <-> the uint8 [H,W,3] frames the rest of this interface takes (an extension;
 * otvm_amd/yuv.py, python -m otvm_amd.y4m_cli).  Integer arithmetic throughout, no atomics: two calls give equal bits, and
 * tests/yuv_ref.py restates both kernels operation by operation.  Checked by definition only (bilinear chroma at the stated
 * siting, the matrix of the stated standard, round half up, clamp): within one code value of the float64 definition.  Both run on
 * the caller's stream, never synchronise with the host, and launch nothing when an argument is refused (nonzero;
 * otvm_last_error() starts with the function's name).  Sides are 1 .. 65535; every offset is formed in 64 bits.  Every plane has
 * its own pointer and its own row stride in bytes (>= the row's bytes), so a frame buffer is addressed where it lies.  New symbols
 * only (additive, as the entries above): the ABI number stays.
 *
 * Chroma sizes: cw = (W + 1) / 2, ch = (H + 1) / 2.  Layouts: 420P has u, v [ch,cw]; NV12 has one plane [ch,cw,2] = (U, V) given
 * as u (v is not looked at); 422P has u, v [H,cw]; 444P has u, v [H,W]; MONO has no chroma (U = V = 128; u, v not looked at).
 *
 * otvm_yuv_to_rgb.  Chroma at luma resolution is bilinear, weights in quarters per axis, indices clamped to the plane:
 *   horizontal, c = x >> 1 (420P, NV12, 422P):
 *     OTVM_YUV_SITING_CENTRE  even x: 3 C[c] + C[c-1],  odd x: 3 C[c] + C[c+1]
 *     OTVM_YUV_SITING_LEFT    even x: 4 C[c],           odd x: 2 C[c] + 2 C[c+1]
 *     444P: 4 C[x] (siting is not looked at beyond being a known value)
 *   vertical, r = y >> 1 (420P, NV12: always centre): even y: 3 row[r] + row[r-1], odd y: 3 row[r] + row[r+1]; otherwise 4 row[y].
 *   The product of the two is the integer u16 = 16 x chroma, NOT rounded; du = u16 - 2048, dv likewise.
 * Matrix, 20 fractional bits, one rounding, arithmetic shift, clamp to 0 .. 255, with yo = 16 (limited) or 0 (full):
 *     R = (CY (Y - yo) + RV dv           + 2^19) >> 20
 *     G = (CY (Y - yo) - GU du - GV dv   + 2^19) >> 20
 *     B = (CY (Y - yo) + BU du           + 2^19) >> 20
 *   (CY, RV, GU, GV, BU), the chroma ones carrying the 1/16:  BT.601 limited 1220945, 104597, 25675, 53279, 132201;
 *   BT.601 full 1048576, 91881, 22553, 46802, 116130;  BT.709 limited 1220945, 117489, 13975, 34925, 138438;
 *   BT.709 full 1048576, 103206, 12276, 30679, 121609.  Full range: CY = 2^20, so (v, 128, 128) gives R = G = B = v exactly.
 * rgb is [H,W,3] contiguous, stored R, G, B when u8_rgb != 0 and B, G, R otherwise.
 *
 * otvm_rgb_to_yuv420: img uint8 [H,W,3] (u8_rgb as above) -> planar y [H,W], u, v [ch,cw], chroma sited at the centre of its
 * 2 x 2 block ("C420jpeg").  With yo as above and co = 128:
 *     Y = ((YR R + YG G + YB B + 2^19) >> 20) + yo
 *     U = ((-UR sR - UG sG + CH sB + (co << 22) + 2^21) >> 22),  V = ((CH sR - VG sG - VB sB + (co << 22) + 2^21) >> 22), clamped
 *   where sR, sG, sB are the SUMS over the block's four pixels, coordinates clamped to the image (an odd edge counts the edge
 *   pixel twice): one integer expression, one rounding, no intermediate mean.  UG = CH - UR and VG = CH - VB, so the chroma rows
 *   sum to zero, and YR + YG + YB is the range's scale exactly (2^20 in full range): grey v gives (v, 128, 128) in full range.
 *   (YR, YG, YB, CH, UR, VB):  BT.601 limited 269262, 528618, 102662, 460551, 155423, 74897;
 *   BT.601 full 313524, 615514, 119538, 524288, 176932, 85262;  BT.709 limited 191455, 644068, 65019, 460551, 105533, 42230;
 *   BT.709 full 222927, 749942, 75707, 524288, 120138, 48074.                                                                   */
#define OTVM_YUV_420P 0
#define OTVM_YUV_NV12 1
#define OTVM_YUV_422P 2
#define OTVM_YUV_444P 3
#define OTVM_YUV_MONO 4
#define OTVM_YUV_BT601 0
#define OTVM_YUV_BT709 1
#define OTVM_YUV_LIMITED 0
#define OTVM_YUV_FULL 1
#define OTVM_YUV_SITING_LEFT 0
#define OTVM_YUV_SITING_CENTRE 1
typedef struct otvm_yuv_to_rgb_params {
    int H, W;
    int layout, matrix, range, siting;      /* OTVM_YUV_* */
    int y_stride, u_stride, v_stride;       /* bytes per row of each plane */
    int u8_rgb;
    const uint8_t* y;
    const uint8_t* u;                       /* NV12: the interleaved plane */
    const uint8_t* v;
    uint8_t* rgb;                           /* [H,W,3] */
} otvm_yuv_to_rgb_params;
int otvm_yuv_to_rgb(const otvm_yuv_to_rgb_params* p, void* stream);

typedef struct otvm_rgb_to_yuv420_params {
    int H, W;
    int matrix, range;                      /* OTVM_YUV_* */
    int y_stride, u_stride, v_stride;       /* bytes per row of each plane */
    int u8_rgb;
    const uint8_t* img;                     /* [H,W,3] */
    uint8_t* y;                             /* [H,W] */
    uint8_t* u;                             /* [ch,cw] */
    uint8_t* v;                             /* [ch,cw] */
} otvm_rgb_to_yuv420_params;
int otvm_rgb_to_yuv420(const otvm_rgb_to_yuv420_params* p, void* stream);

/* ---------------------------------------------------------------- masks of keyed footage --------
 * The mask otvm_trimap_from_mask takes, made from the frame itself: frame uint8 [H,W,3] -> mask uint8 [H,W], 255 = subject,
 * 0 = screen / plate, every element written.  Integer arithmetic throughout, no atomics: two calls give equal bits.  Both run on
 * the caller's stream, never synchronise with the host, and launch nothing when an argument is refused (nonzero;
 * otvm_last_error() starts with the function's name).  Sides are 1 .. 16383; every offset is formed in 64 bits.  Any base
 * address and any W is taken (four pixels move as dwords when W % 4 == 0 and frame and mask are 4-byte aligned, byte by byte
 * otherwise).  New symbols only (additive, as the entries above): the ABI number stays.
 *
 * otvm_mask_from_chroma: a hue-cone key that does not depend on brightness.  u8_rgb says which byte is R, as
 * otvm_preprocess_params.u8_rgb does.  Per pixel, with the chroma rows of otvm_rgb_to_yuv420's BT.601 full-range matrix
 * (CH, UR, VB) = (524288, 176932, 85262), UG = CH - UR, VG = CH - VB, applied to ONE pixel with 20 fractional bits:
 *     Cb = clamp((-UR R - UG G + CH B + (128 << 20) + 2^19) >> 20, 0, 255),  cb = Cb - 128
 *     Cr = clamp(( CH R - VG G - VB B + (128 << 20) + 2^19) >> 20, 0, 255),  cr = Cr - 128
 *     q  = (cb kb + cr kr) - |cb kr - cr kb|
 *   (kb, kr) are cb, cr of the key colour, computed by the caller by the same rule: -128 .. 127, refused when
 *   kb^2 + kr^2 < 16^2 (a grey key has no hue).  q is positive inside the 45 degree cone round the key's hue and grows with
 *   saturation.  With -2^20 <= qlo < qhi <= 2^20 (the caller's chroma thresholds times |K| = sqrt(kb^2 + kr^2), rounded):
 *     mask = 255 where q <= qlo, 0 where q >= qhi, 255 - ((q - qlo) 255) / (qhi - qlo) between them (floor division).
 *
 * otvm_mask_from_plate: a difference key against a clean plate, plate uint8 [H,W,3] in the frame's channel order (the
 * distance is symmetric in the channels, so the order itself is not asked for).  For pixel x and radius r in 0 .. 3
 *     d(x) = min over the plate pixels x' of the (2r+1)^2 neighbourhood of x, coordinates clamped to the image,
 *            of max_c |I_c(x) - P_c(x')|
 *   and with 0 <= lo < hi <= 255:
 *     mask = 0 where d <= lo, 255 where d >= hi, ((d - lo) 255) / (hi - lo) between them (floor division).               */
typedef struct otvm_mask_from_chroma_params {
    const uint8_t* frame;                   /* [H,W,3] */
    uint8_t* mask;                          /* [H,W] */
    int H, W;
    int u8_rgb;
    int kb, kr;                             /* the key colour's cb, cr */
    int qlo, qhi;
} otvm_mask_from_chroma_params;
int otvm_mask_from_chroma(const otvm_mask_from_chroma_params* p, void* stream);

typedef struct otvm_mask_from_plate_params {
    const uint8_t* frame;                   /* [H,W,3] */
    const uint8_t* plate;                   /* [H,W,3] */
    uint8_t* mask;                          /* [H,W] */
    int H, W;
    int radius;                             /* 0 .. 3 */
    int lo, hi;
} otvm_mask_from_plate_params;
int otvm_mask_from_plate(const otvm_mask_from_plate_params* p, void* stream);

/* ---------------------------------------------------------------- range guard / clear -----------
 * f16x3 splits fp32 operands into fp16 halves: |x| >= 65504 loses accuracy, >= 131008 becomes inf.
 * otvm_finite_guard scans an NHWC view [P, C] (ld) and stores min(*flag, tag) when any element fails |x| < limit
 * (NaN fails too); *flag is initialised to INT32_MAX by the caller and read by the host when it synchronises.  The
 * engine runs it on everything that survives a frame: the memorised key / value maps (STM.py:201-228), the hidden
 * state and the propagated trimap logits (alpha/model.py:432-471).                                               */
int otvm_finite_guard(const float* x, int64_t P, int C, int ld, float limit, int tag, int* flag, void* stream);
/* stream-ordered zero fill (hipMemsetAsync) -- the GroupNorm statistics arena is cleared once per frame           */
int otvm_clear(void* p, int64_t bytes, void* stream);

/* ---------------------------------------------------------------- training forward -------------
 * FullModel.forward of the reference's training class (models/alpha/model.py:189-312), FORWARD ONLY: the network runs on
 * the kernels above (B clips in lock-step, memory every frame); these entry points add what the losses need.
 * All tensors planar fp32; "N images" = batch x frames (x channels where noted); sums leave in fp64 accumulators that
 * the caller zeroes and divides by the element counts torch.mean / mse_loss / CrossEntropyLoss use.               */
/* the heads again with all outputs: out7 planar [7][P] = fused alpha, F, B (FBA/models.py:383-388,425-432);
 * logits_out planar [3][P] = the refinement's trimap logits (n_out == 10)                                           */
int otvm_fba_head_train(const float* hid, int hid_ld, const float* w, const float* b, int n_out, const float* img, int img_ld,
                        int64_t P, float* out7, float* logits_out, void* stream);
/* the STM decoder's logits, x4 bilinear (STM.py:136), WITHOUT the softmax: planar [3][Hp*Wp]                         */
int otvm_upsample4_logits3(const float* logits, int h4, int w4, int ld, float* logits_out, void* stream);
/* frame 0 of a training clip memorises the GROUND-TRUTH trimap (model.py:212, preds_trimap_refine[0] = tri[:,0]):
 * planar [3][P] -> the unknown / foreground channels of the Encoder_M input buffer                                   */
int otvm_trimap_to_sm(const float* tri, int64_t P, float* sm, int sm_ld, void* stream);
/* model.py:59-60: out = in.flip(channel) * s on planar [N][3][P]; model.py:42-44: trimask = (argmax == unknown), class map */
int otvm_scale_flip3(const float* in, int64_t N, int64_t P, float s, float* out, void* stream);
int otvm_trimask(const float* tri, int64_t N, int64_t P, float* mask, unsigned char* cls, const float* gts, float* vis, void* stream);
                                                    /* vis (optional): where(trimask, 128/255, gts), model.py:296-300 */
/* fba_single_image_loss, per-pixel part (model.py:117-150): writes cF, cB, comp [N][3][P], alpha_out [N][P]; acc5 += sums of |a - gt|,
 * |cF gt + cB (1-gt) - img|, |fgs a + bgs (1-a) - img|, |cF - fgs|, |cB - bgs|                                      */
int otvm_loss_fba_comp(const float* pred7, const float* gt, const float* trimask, const float* fgs, const float* bgs, const float* img,
                       int64_t N, int64_t P, float* cF, float* cB, float* comp, float* alpha_out, double* acc5, void* stream);
/* L1_grad (utils/loss_func.py:44-51): acc += | |grad x| - |grad y| | over planar [N][H][W]                            */
int otvm_loss_grad_l1(const float* x, const float* y, int64_t N, int H, int W, float eps, double* acc, void* stream);
/* exclusion_loss (loss_func.py:56-82), one pyramid level over images [B][S][3][H][W]: acc1[S][4] (zeroed) receives the
 * per-frame sums of |gx1|, |gy1|, |gx2|, |gy2|, acc2[B*S][2] (zeroed) the per-sample sums of the squared products       */
int otvm_loss_exclusion_level(const float* img1, const float* img2, int B, int S, int H, int W, float eps, double* acc1, double* acc2,
                              void* stream);
int otvm_avgpool2(const float* x, int64_t N, int H, int W, float* y, void* stream);
/* LapLoss (loss_func.py:95-155), one level: down = gauss(cur)[::2, ::2] for image and target (written), acc += weight *
 * | (cur_i - up(down_i)) - (cur_t - up(down_t)) |                                                                    */
int otvm_loss_lap_level(const float* cur_img, const float* cur_tgt, int64_t N, int H, int W, double weight, float* down_img,
                        float* down_tgt, double* acc, void* stream);
/* model.py:177-182: acc += ((x[b,t+1]-x[b,t]) - (y[b,t+1]-y[b,t]))^2 over planar [B][S][CP]                           */
int otvm_loss_temporal(const float* x, const float* y, int B, int S, int64_t CP, double* acc, void* stream);
/* nn.CrossEntropyLoss (model.py:286-290): acc += -log_softmax(logits)[cls] over planar logits [N][3][P], cls [N][P] u8 */
int otvm_loss_ce3(const float* logits, const unsigned char* cls, int64_t N, int64_t P, double* acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OTVM_HIP_H */
