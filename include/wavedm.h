/*
 * wavedm.h -- C ABI of libwavedm_hip.so: the MI355X (gfx950) implementation of WaveDM's sampling
 * hot path: 2-level Haar wavelet-packet DWT/IDWT, the wavelet-domain diffusion
 * UNet forward, and the per-step DDIM patch gather / scatter-mean / update.
 *
 * The reference has no FFI layer (it is pure Python on torch); each entry point
 * below names the reference function whose device work it replaces.  The reference-side binding
 * (ctypes) is shown in INTEGRATION.md and implemented in wavedm_amd/_lib.py.
 *
 * Conventions
 *   - every function returns 0 (WDM_OK) or a negative WDM_E* code and never throws;
 *     wdm_last_error() gives the message of the last failure on the calling thread;
 *   - the library never allocates device memory: the caller (torch) owns every buffer including
 *     the packed-weight buffer and the workspace, and passes raw device pointers;
 *   - all kernels are enqueued on the `stream` argument (a hipStream_t; pass torch's current
 *     stream); no call synchronises the device;
 *   - one wdm_handle per device, one wdm_unet per model; a handle/unet is not thread-safe,
 *     distinct handles are independent;
 *   - "NCHW f32" tensors are the reference's layout at the boundary; inside the UNet
 *     activations are NHWC (channels-last) in the model dtype (WDM_BF16 / WDM_F16: 2 bytes, WDM_F32 / WDM_F32X3: 4).
 */
#ifndef WAVEDM_H
#define WAVEDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WDM_ABI_VERSION 1

enum {
    WDM_OK = 0,
    WDM_EINVAL = -1,    /* bad argument / unsupported shape */
    WDM_ENOMEM = -2,    /* caller-provided buffer too small */
    WDM_EHIP = -3,      /* a HIP runtime call failed */
    WDM_ESTATE = -4,    /* call order violated (e.g. forward before all params loaded) */
    WDM_ENOTFOUND = -5  /* unknown parameter name */
};

/* WDM_F32X3: fp32 tensors exactly as WDM_F32 (same buffers, same elementwise kernels); only the contractions differ -- each product is three
 * bf16 MFMAs on operands split hi + lo in registers (~1e-5 end to end, several times the rate of the exact-fp32 MFMA chain).  UNet / block /
 * conv entry points take it; the HFRM and the trainer take WDM_F32 or WDM_BF16.
 * WDM_F16: the bf16 path on IEEE half operands -- fp16 tensors and packed weights, v_mfma_f32_16x16x32_f16 (the bf16 MFMA's rate), fp32 accumulators,
 * GroupNorm statistics, softmax and DDIM state exactly as in WDM_BF16.  Three more mantissa bits than bf16 (unit round-off 2^-11): the mode meant to
 * meet the 1e-3 parity bound at the bf16 mode's speed.  The price is range (|x| <= 65504): wdm_unet_load_param fails with WDM_EINVAL on a weight outside
 * it.  UNet / block / conv / layout entry points take it; the HFRM and the trainer do not. */
enum { WDM_F32 = 0, WDM_BF16 = 1, WDM_F32X3 = 2, WDM_F16 = 3 };

typedef struct wdm_handle wdm_handle;
typedef struct wdm_unet wdm_unet;

/* ---- library / handle ------------------------------------------------------------------- */
int wdm_abi_version(void);
const char* wdm_last_error(void);
int wdm_create(int device, wdm_handle** out);
int wdm_destroy(wdm_handle* h);

/* ---- Haar wavelet-packet transform ---------------------------------------------------------
 * Replaces WaveletTransform.forward, models/wavelet.py:37-49 (scale=2, transpose=True):
 *   fwd: x (B,3,H,W) NCHW f32  ->  y (B,48,H/4,W/4) NCHW f32, channel = subband*3 + rgb
 *   inv: y (B,48,h,w)          ->  x (B,3,4h,4w)
 * H and W must be multiples of 4. */
int wdm_dwt_fwd(wdm_handle* h, const float* x, float* y, int B, int H, int W, void* stream);
int wdm_dwt_inv(wdm_handle* h, const float* y, float* x, int B, int hh, int ww, void* stream);
/* The same transforms with the element-wise steps the reference runs around them folded in (no extra pass, no ATen kernel in the loop):
 *   wdm_dwt_fwd_affine:   y = DWT(scale * x + shift)            -- data_transform, 2x - 1 (restoration.py:8-9, ddm_wavelet.py:345-348)
 *   wdm_dwt_inv_compose:  coefficient channels [0, n_lo) are read from y_lo (B, lo_channels, h, w), the others from y_hi (B,48,h,w) -- the
 *                         torch.cat([x0[:, :pc], hf_wav[:, pc:]]) of restoration.py:114 -- and, if to_unit_range, the output is
 *                         clamp((x + 1) / 2, 0, 1) = inverse_data_transform (restoration.py:12-13).  n_lo = 0: y_lo may be NULL. */
int wdm_dwt_fwd_affine(wdm_handle* h, const float* x, float scale, float shift, float* y, int B, int H, int W, void* stream);
int wdm_dwt_inv_compose(wdm_handle* h, const float* y_lo, int lo_channels, int n_lo, const float* y_hi, float* x, int B, int hh, int ww,
                        int to_unit_range, void* stream);

/* wdm_ensemble_compose: N diffusion samples per image reduced to their mean image and per-pixel spread, fused with the compose + IDWT above (no
 * counterpart in the reference, which draws one sample).  All in fp32, in a fixed order, without atomics; everything is queued on `stream`.
 *   preds     (B * n_samples, lo_channels, hh, ww) : sample k of image i is row i * n_samples + k
 *   y_hi      (B, 48, hh, ww)                      : the bands that are not predicted; may be NULL when n_lo == 48
 *   mean_img  (B, 3, 4hh, 4ww)
 *   std_img   same shape, or NULL
 *   mean_coef (B, n_lo, hh, ww), or NULL
 * mean coefficient = (((p_0 + p_1) + p_2) + ...) / (float)n_samples, samples added in ascending order, the last step a division.
 * mean_img = what wdm_dwt_inv_compose makes of [mean_coef[:, :n_lo] | y_hi[:, n_lo:]] (n_samples == 1: its bits).
 * std_img  = the unbiased (n_samples - 1) standard deviation over the samples of the UNCLAMPED pixel (IDWT(compose(p_k, y_hi)) + 1) / 2, in two passes
 *            (the mean first, then the squared deviations, added in ascending order); only the n_lo predicted bands enter the deviations.  Without
 *            to_unit_range the factor 1/2 is dropped.  n_samples == 1 with std_img is WDM_EINVAL.
 * An image's result does not depend on the batch around it.  Limits, else WDM_EINVAL and nothing is launched: 1 <= n_samples <= 256; n_lo a multiple of 3
 * in [3, 48], n_lo <= lo_channels; B * n_samples <= 65535.  Element offsets are 64-bit. */
int wdm_ensemble_compose(wdm_handle* h, const float* preds, int lo_channels, int n_lo, int n_samples, const float* y_hi, float* mean_img,
                         float* std_img, float* mean_coef, int B, int hh, int ww, int to_unit_range, void* stream);

/* ---- layout helpers at the UNet boundary ---------------------------------------------------
 * A "patch list" is n triples (img, hi, wi) of int32 on the DEVICE: patch k is the p x p window
 * at (hi, wi) of image `img` of a (NIMG, C, H, W) NCHW f32 tensor.  It restates the reference's
 * `corners` list (models/ddm_wavelet.py:419) with an explicit image index so that B independent
 * 64x64 crops (corners = [(0,0)] each) and one stitched image (45 corners) use the same kernels.
 *
 * wdm_pack_channels: gather `nch` channels of src (NIMG, nch, H, W) NCHW f32 for every patch into
 * channels [c_off, c_off+nch) of the NHWC UNet input x96 (n, p, p, 96) of dtype `dtype`.
 * Replaces crop()+cat at models/ddm_wavelet.py:467-478 (channel order [x_cond 0:48 | x_t 48:51 |
 * x_other 51:96]). */
int wdm_pack_channels(wdm_handle* h, const float* src, int nch, int H, int W, const int32_t* patches, int n,
                      int p, void* x96, int c_total, int c_off, int dtype, void* stream);

/* wdm_ddim_update: scatter-add of the predicted noise patches into the full image in patch-list
 * order, division by the overlap count, and the eta=0 DDIM update; replaces
 * models/ddm_wavelet.py:485-502.
 *   eps      (n, 3, p, p) NCHW f32 : UNet output per patch
 *   x_t      (NIMG, 3, H, W)       : current sample;  x0_out / x_next_out same shape
 *   coefficients (host floats, computed by the caller in fp32 like utils/sampling.py:10-13):
 *     sqrt_1m_at = sqrt(1-abar_t), sqrt_at = sqrt(abar_t), sqrt_at_next, c2 = sqrt(1-abar_next)
 *   x0 = (x_t - eps*sqrt_1m_at)/sqrt_at ;  x_next = sqrt_at_next*x0 + c2*eps
 * Pixels covered by no patch get eps = 0/0 = NaN exactly like the reference's division.
 * This and the three 3-channel names below are the `_c` entry points further down at channels = 3: the same kernels, the same bits.  With a patch list
 * they therefore refuse nimg > 65535 (the image is a launch-grid dimension there) with WDM_EINVAL; patches == NULL, the element-wise identity form,
 * has no such limit. */
int wdm_ddim_update(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, const float* x_t,
                    int nimg, int H, int W, float sqrt_1m_at, float sqrt_at, float sqrt_at_next, float c2,
                    float* x0_out, float* x_next_out, void* stream);

/* wdm_ddim_update_eta: the same scatter-mean and x0, with the stochastic term of models/ddm_wavelet.py:500-502 (eta != 0; the reference's
 * own callers pass eta = 0, ddm_wavelet.py:302):  c1 = eta*sqrt((1 - at/at_next)(1 - at_next)/(1 - at)), c2 = sqrt((1 - at_next) - c1^2) -- both
 * computed by the caller in fp32 --  x_next = sqrt_at_next*x0 + c1*noise + c2*eps, summed left to right like the reference's expression.
 *   noise (NIMG, 3, H, W) f32 : the caller's randn_like(x) draw of this step */
int wdm_ddim_update_eta(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, const float* x_t,
                        int nimg, int H, int W, float sqrt_1m_at, float sqrt_at, float sqrt_at_next, float c1, float c2,
                        const float* noise, float* x0_out, float* x_next_out, void* stream);

/* Patch-sharded single image (no reference counterpart -- its eval is single-GPU): every rank runs the UNet
 * on ITS patches only.  wdm_patch_accumulate writes the rank's partial sums (NIMG*3*H*W floats) followed by its partial overlap
 * counts (same size) into acc_cnt, the caller all-reduces (sum) that ONE buffer over RCCL, and wdm_ddim_from_sums divides and
 * applies the DDIM update of wdm_ddim_update on every rank.  n = 0 writes zeros. */
int wdm_patch_accumulate(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, int nimg, int H, int W,
                         float* acc_cnt, void* stream);
int wdm_ddim_from_sums(wdm_handle* h, const float* acc_cnt, const float* x_t, int nimg, int H, int W, float sqrt_1m_at,
                       float sqrt_at, float sqrt_at_next, float c2, float* x0_out, float* x_next_out, void* stream);

/* The four entry points above for ANY number of prediction channels (`channels` = model.pred_channels: 12 = the whole coarse level, 48 = every band
 * diffused): eps (n, channels, p, p), x_t / x0_out / x_next_out / noise (NIMG, channels, H, W), acc_cnt 2 * NIMG*channels*H*W floats (sums | counts).
 * A pixel's covering patches are searched within its image's span of the patch list only, once for up to four channels; each channel's sum runs in
 * patch-list order in fp32 like the reference's sequential "+=".  With a patch list, nimg and channels are launch-grid dimensions: more than 65535 of either,
 * or H * W beyond 2^31 - 257, is WDM_EINVAL.  patches == NULL is the element-wise identity form (n == nimg, p == H == W) and has no such limit. */
int wdm_ddim_update_c(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, int channels, const float* x_t,
                      int nimg, int H, int W, float sqrt_1m_at, float sqrt_at, float sqrt_at_next, float c2,
                      float* x0_out, float* x_next_out, void* stream);
int wdm_ddim_update_eta_c(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, int channels, const float* x_t,
                          int nimg, int H, int W, float sqrt_1m_at, float sqrt_at, float sqrt_at_next, float c1, float c2,
                          const float* noise, float* x0_out, float* x_next_out, void* stream);
int wdm_patch_accumulate_c(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, int channels, int nimg, int H, int W,
                           float* acc_cnt, void* stream);
int wdm_ddim_from_sums_c(wdm_handle* h, const float* acc_cnt, const float* x_t, int channels, int nimg, int H, int W, float sqrt_1m_at,
                         float sqrt_at, float sqrt_at_next, float c2, float* x0_out, float* x_next_out, void* stream);

/* ---- images of DIFFERENT sizes in one call: the ragged layout -----------------
 * A ragged C-channel tensor of nimg images is ONE flat f32 buffer: image i occupies the contiguous elements
 * [C * pix_off[i], C * pix_off[i+1]) as a plain (C, H_i, W_i) NCHW block, pix_off = the prefix sum of H_i * W_i.  One set of tables therefore serves
 * x_cond (48 channels), x_t / x0 / x_next (pred_channels) and x_other; every W_i is a multiple of 4, so every block starts 16-byte aligned for every C.
 * Device tables (read-only, built by the caller -- wavedm_amd.sampling.RaggedLayout validates them; the library checks only what the host can see):
 *   img_tab  int32[nimg][4]  : H_i, W_i, patch_lo_i, patch_hi_i -- [patch_lo, patch_hi) is image i's slice of the patch list, which must be image-major
 *                              (all of image 0's triples, then image 1's, ...), every window inside its image;
 *   blk_tab  int32[nimg + 1] : the first 256-pixel block of image i, blocks counted per image (ceil(H_i W_i / 256) each); blk_tab[nimg] = nblk, all blocks;
 *   pix_off  int64[nimg + 1] : the pixel offsets above.
 * wdm_pack_channels_ragged: wdm_pack_channels with `src` ragged (nch channels); p <= 128 and nch <= 48 (one workgroup per patch row).
 * wdm_ddim_update_ragged:   wdm_ddim_update_c (eta = 0) with x_t / x0_out / x_next_out ragged (`channels` channels); eps (n, channels, p, p) as before.
 * Per image both return the bits of the plain entry points on that image alone (wdm_ddim_update's at channels = 3): the same sums in patch-list order,
 * the same expression, 0/0 = NaN where no patch covers a pixel.  Bad arguments: WDM_EINVAL, nothing launched. */
int wdm_pack_channels_ragged(wdm_handle* h, const float* src, int nch, const int32_t* img_tab, const int64_t* pix_off, int nimg,
                             const int32_t* patches, int n, int p, void* x96, int c_total, int c_off, int dtype, void* stream);
int wdm_ddim_update_ragged(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, int channels, const float* x_t,
                           const int32_t* img_tab, const int32_t* blk_tab, const int64_t* pix_off, int nimg, int nblk, float sqrt_1m_at,
                           float sqrt_at, float sqrt_at_next, float c2, float* x0_out, float* x_next_out, void* stream);

/* ---- DPM-Solver++(2M) multistep update (no reference counterpart, whose only integrator is the DDIM step) ----------------
 * The scatter-mean of wdm_ddim_update_c, wdm_ddim_from_sums_c and wdm_ddim_update_ragged followed by the second-order multistep rule for the
 * probability-flow ODE instead of the DDIM step:
 *   x0     = (x_t - eps*sqrt_1m_at)/sqrt_at                    -- the expression, and for the same inputs the bits, of the DDIM entry points
 *   x_next = fma(cp, x0_prev, fma(c0, x0, cx * x_t))           -- three roundings, the same in all three entry points
 *   x0_prev : the previous step's x0_out, the shape of x_t; may not alias x0_out or x_next_out
 *   cx, c0, cp : host floats (wavedm_amd.sampling.solver_coefficients): cx = sigma_next/sigma_t, c0 = g (1 + 1/(2r)), cp = -g/(2r),
 *                g = alpha_next (1 - exp(-h)), h the step's log-SNR gap and r the ratio of the previous gap to it.
 * Argument order, patch-list rules, 0/0 = NaN on uncovered pixels, refusals (WDM_EINVAL, nothing launched) and grid limits are those of the DDIM
 * sibling; a null x0_prev is WDM_EINVAL.  The sharded pair is wdm_patch_accumulate_c, unchanged, then wdm_multistep_from_sums_c.
 * Additions to the ABI: WDM_ABI_VERSION stays 1. */
int wdm_multistep_update_c(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, int channels, const float* x_t,
                           const float* x0_prev, int nimg, int H, int W, float sqrt_1m_at, float sqrt_at, float cx, float c0, float cp,
                           float* x0_out, float* x_next_out, void* stream);
int wdm_multistep_from_sums_c(wdm_handle* h, const float* acc_cnt, const float* x_t, const float* x0_prev, int channels, int nimg, int H, int W,
                              float sqrt_1m_at, float sqrt_at, float cx, float c0, float cp, float* x0_out, float* x_next_out, void* stream);
int wdm_multistep_update_ragged(wdm_handle* h, const float* eps, const int32_t* patches, int n, int p, int channels, const float* x_t,
                                const float* x0_prev, const int32_t* img_tab, const int32_t* blk_tab, const int64_t* pix_off, int nimg, int nblk,
                                float sqrt_1m_at, float sqrt_at, float cx, float c0, float cp, float* x0_out, float* x_next_out, void* stream);

/* NCHW f32 (B,C,H,W) -> NHWC dtype (B,H,W,C) and back (used by the drop-in model(x, t) call). */
int wdm_nchw_to_nhwc(wdm_handle* h, const float* src, void* dst, int B, int C, int H, int W, int dtype,
                     void* stream);
int wdm_nhwc_to_nchw(wdm_handle* h, const void* src, float* dst, int B, int C, int H, int W, int dtype,
                     void* stream);

/* ---- UNet ----------------------------------------------------------------------------------
 * Replaces DiffusionUNet.__init__/forward, models/unet.py:197-307, 346-395 (use_window and
 * wavelet_in_unet off, as in configs/raindrop_wavelet.yml). */
typedef struct wdm_unet_config {
    int ch;                  /* model.ch */
    int n_levels;            /* len(model.ch_mult), <= 8 */
    int ch_mult[8];
    int num_res_blocks;
    int n_attn_res;          /* len(model.attn_resolutions), <= 8 */
    int attn_resolutions[8];
    int in_channels;         /* UNet input channels (96 for raindrop_wavelet.yml, unet.py:212); any width >= 1: conv_in is zero-padded to a multiple of 32 */
    int out_ch;              /* 3 (12 / 48 with data.use_window / data.wavelet_in_unet) */
    int resolution;          /* data.image_size */
    int resamp_with_conv;    /* must be 1 */
    int dtype;               /* WDM_BF16 (throughput), WDM_F16 (throughput, fp16 operands), WDM_F32 (exact parity mode) or WDM_F32X3 (fast parity mode) */
} wdm_unet_config;

int wdm_unet_create(wdm_handle* h, const wdm_unet_config* cfg, wdm_unet** out);
int wdm_unet_destroy(wdm_unet* u);

/* state_dict enumeration: names/shapes are exactly the reference's state_dict keys */
int wdm_unet_num_params(const wdm_unet* u);
int wdm_unet_param_info(const wdm_unet* u, int i, const char** name, int* ndim, int64_t shape[4]);

/* packed weights live in ONE caller-allocated device buffer (so a rank-0 RCCL broadcast of that
 * buffer is the whole weight distribution step) */
size_t wdm_unet_packed_bytes(const wdm_unet* u);
int wdm_unet_set_packed(wdm_unet* u, void* packed, size_t bytes);
/* repack one fp32 parameter (device pointer, reference layout: conv OIHW, Linear [out,in]) into
 * the packed buffer, converting to the model dtype */
int wdm_unet_load_param(wdm_unet* u, const char* name, const float* dev_src, int64_t numel, void* stream);
/* mark the packed buffer as complete without per-parameter loads (after a broadcast) */
int wdm_unet_mark_loaded(wdm_unet* u);

size_t wdm_unet_workspace_bytes(const wdm_unet* u, int B);
/* x96: (B, R, R, in_channels) NHWC in the model dtype; t: n_t device floats, n_t in {1, B};
 * eps_out: (B, out_ch, R, R) NCHW f32 */
int wdm_unet_forward(wdm_unet* u, const void* x96, const float* t, int n_t, int B, float* eps_out,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The timestep-dependent part of the network -- sinusoidal embedding, temb MLP and every ResnetBlock's temb_proj (models/unet.py:10-28, 225-230,
 * 354-357, 125) -- depends on t alone.  A sampler knows its whole timestep sequence up front (models/ddm_wavelet.py:296-297): wdm_unet_temb_table
 * computes the rows for all n timesteps in four launches, temb_out[n][wdm_unet_temb_rows(u)] (f32, device), and wdm_unet_forward_temb runs one UNet
 * call from one row of it (shared by the B images) -- the same bits as wdm_unet_forward with that timestep, four launches fewer per call.
 * The table is a function of the weights: rebuild it after a weight update.  workspace: the forward workspace serves. */
int wdm_unet_temb_rows(const wdm_unet* u);
int wdm_unet_temb_table(wdm_unet* u, const float* t, int n, float* temb_out, void* workspace, size_t workspace_bytes, void* stream);
int wdm_unet_forward_temb(wdm_unet* u, const void* x96, const float* temb_row, int B, float* eps_out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Taps on the forward (unit tests): wdm_unet_forward_taps IS wdm_unet_forward -- the same launches on the same arena -- and copies every layer's output to a caller
 * buffer right behind the launch that produced it (device to device, on `stream`, before the arena reuses the memory).  The layers are listed by
 * wdm_unet_num_taps / wdm_unet_tap_info in executor order under their state_dict prefixes: conv_in, down.L.block.B, down.L.attn.B, down.L.downsample, mid.block_1,
 * mid.attn_1, mid.block_2, up.L.block.B, up.L.attn.B, up.L.upsample.  C, H, W: the output's shape; kind: WDM_UNET_TAP_*; in0: the tap the layer reads (-1: the
 * network's input); in1: for a ResnetBlock of the up path the tap of its skip connection, the second half of the concat [in0 | in1], else -1.
 *   taps[i]     : device pointer to (B, H, W, C) NHWC in the model dtype, or NULL to skip the layer; the array itself is a host array and may be NULL
 *   nrm_taps[i] : likewise; receives act(GroupNorm_consumer(output)), the normalised copy the producing conv wrote for its consumer, where it wrote one, and is
 *                 left untouched where it wrote none
 * With both arrays NULL nothing is added to wdm_unet_forward: the same launches, the same bits.  Arguments, workspace and refusals as wdm_unet_forward.
 * Additions to the ABI: WDM_ABI_VERSION stays 1. */
enum { WDM_UNET_TAP_RESBLOCK = 0, WDM_UNET_TAP_ATTN = 1, WDM_UNET_TAP_CONV_IN = 2, WDM_UNET_TAP_DOWN = 3, WDM_UNET_TAP_UP = 4 };
int wdm_unet_num_taps(const wdm_unet* u);
int wdm_unet_tap_info(const wdm_unet* u, int i, const char** name, int* C, int* H, int* W, int* kind, int* in0, int* in1);
int wdm_unet_forward_taps(wdm_unet* u, const void* x96, const float* t, int n_t, int B, float* eps_out, void* const* taps, void* const* nrm_taps,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-block entry points (unit parity tests; same code the UNet executor runs) -----------
 * Weights are given in the reference layout as fp32 device pointers and packed on the fly into
 * `scratch`; x / y are NCHW f32 at this test boundary.  See wavedm_amd/csrc/api.hip. */
typedef struct wdm_resblock_params {  /* ResnetBlock, models/unet.py:81-138 */
    int cin, cout;
    const float *norm1_w, *norm1_b, *conv1_w, *conv1_b, *temb_w, *temb_b;
    const float *norm2_w, *norm2_b, *conv2_w, *conv2_b, *nin_w, *nin_b; /* nin_* NULL if cin==cout */
} wdm_resblock_params;
typedef struct wdm_attn_params {      /* AttnBlock, models/unet.py:141-193 */
    int c;
    const float *norm_w, *norm_b, *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *proj_w, *proj_b;
} wdm_attn_params;

/* x may be the channel concat of two tensors (x0: c0 channels, x1: c1 channels, c1 may be 0) */
int wdm_resblock_forward(wdm_handle* h, const wdm_resblock_params* p, const float* x0, int c0, const float* x1,
                         int c1, const float* temb /* (n_t, 512) raw temb, SiLU applied inside */, int n_t,
                         int temb_ch, int B, int H, int W, float* y, int dtype, void* scratch,
                         size_t scratch_bytes, void* stream);
int wdm_attn_forward(wdm_handle* h, const wdm_attn_params* p, const float* x, int B, int H, int W, float* y,
                     int dtype, void* scratch, size_t scratch_bytes, void* stream);
/* mode: 0 = conv3x3 s1 p1, 1 = Downsample (pad(0,1,0,1) + conv3x3 s2), 2 = Upsample (nearest x2 +
 * conv3x3 p1), 3 = conv1x1 */
int wdm_conv_forward(wdm_handle* h, const float* w, const float* b, int cin, int cout, int mode, const float* x,
                     int B, int H, int W, float* y, int dtype, void* scratch, size_t scratch_bytes,
                     void* stream);
/* timestep embedding + temb MLP (unet.py:10-28, 354-357): t (n_t) -> temb (n_t, 4*ch) */
int wdm_temb_forward(wdm_handle* h, const float* t, int n_t, int ch, const float* w0, const float* b0,
                     const float* w1, const float* b1, float* temb_out, void* scratch, size_t scratch_bytes,
                     void* stream);

/* ---- operators of the optional `data.global_attn` model (DiffusionUNet_Global / Attn_Global, models/unet.py:397-636) ----
 * The ResnetBlocks, AttnBlocks and 3x3 / 1x1 convolutions of that model run on the block entry points above (wavedm_amd/unet_global.py);
 * these are the operators only it has, as plain fp32 NCHW kernels (wavedm_amd/csrc/global_attn.hip).
 * wdm_conv2d_direct: torch.nn.Conv2d(Cin, Cout, k, stride, pad, groups) (weight [Cout][Cin/groups][k][k]) or, transposed != 0,
 *   torch.nn.ConvTranspose2d(Cin, Cout, k, stride, pad) (weight [Cin][Cout][k][k]) -- unet.py:407-424 (q, k, v), :522, :567.
 * wdm_groupnorm: GroupNorm(32, eps) [+ SiLU] (unet.py:36-37; Attn_Global applies norm_patch to both inputs, :433-434).
 * wdm_cross_attention: q (B,C,Nq), k and v (B,C,Nk), any Nk >= 1 -> out (B,C,Nq), softmax(C^-0.5 q^T k) over the keys (unet.py:438-455).
 * wdm_upsample_add: y = x + nearest_upsample(hp, scale) (unet.py:459-462). */
int wdm_conv2d_direct(wdm_handle* h, const float* x, const float* w, const float* bias, int B, int Cin, int H, int W, int Cout, int k,
                      int stride, int pad, int groups, int transposed, float* y, void* stream);
int wdm_groupnorm(wdm_handle* h, const float* x, const float* gamma, const float* beta, int B, int C, int H, int W, float eps, int silu,
                  float* y, void* stream);
int wdm_cross_attention(wdm_handle* h, const float* q, const float* k, const float* v, int B, int C, int Nq, int Nk, float* out,
                        void* stream);
int wdm_upsample_add(wdm_handle* h, const float* x, const float* hp, int B, int C, int H, int W, int scale, float* y, void* stream);

/* ---- HFRM -------------------------------------------------------------------
 * Replaces HFRM.__init__/forward, models/arch.py:206-253 (the module restoration.py:94 runs once per image to
 * produce the 45 "other" wavelet channels).  Same protocol as the UNet object: enumerate the state_dict keys,
 * give one caller-allocated buffer, load fp32 parameters, finalize (packs the GEMM weights, folds beta/gamma),
 * forward on NCHW f32 images whose H and W are multiples of 16. */
typedef struct wdm_hfrm wdm_hfrm;
typedef struct wdm_hfrm_config {
    int in_channel;          /* 3 */
    int dim;                 /* 32 */
    int mid_blk_num;         /* 6 */
    int n_enc;               /* 4 */
    int enc_blk_nums[8];     /* 2,2,2,4 (models/ddm_wavelet.py:139) */
    int n_dec;               /* 4 */
    int dec_blk_nums[8];     /* 2,2,2,2 */
    int dtype;
} wdm_hfrm_config;
int wdm_hfrm_create(wdm_handle* h, const wdm_hfrm_config* cfg, wdm_hfrm** out);
int wdm_hfrm_destroy(wdm_hfrm* m);
int wdm_hfrm_num_params(const wdm_hfrm* m);
int wdm_hfrm_param_info(const wdm_hfrm* m, int i, const char** name, int* ndim, int64_t shape[4]);
size_t wdm_hfrm_packed_bytes(const wdm_hfrm* m);
int wdm_hfrm_set_packed(wdm_hfrm* m, void* packed, size_t bytes);
int wdm_hfrm_load_param(wdm_hfrm* m, const char* name, const float* dev_src, int64_t numel, void* stream);
int wdm_hfrm_finalize(wdm_hfrm* m, void* stream);
size_t wdm_hfrm_workspace_bytes(const wdm_hfrm* m, int B, int H, int W);
int wdm_hfrm_forward(wdm_hfrm* m, const float* x, int B, int H, int W, float* y, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Local channel-attention pooling: the reference's test-time local converter (models/arch.py:46-130, replace_layers + Local_Base.convert
 * with fast_imp=False).  Every ChannelAttn pools over a sliding window instead of the whole map; at level l (maps of H/2^l x W/2^l, l = 0 ..
 * n_enc) the window is kh_l = (train_h >> l) * base_h / train_h by kw_l likewise (integer divisions: what the converting forward at the
 * training size freezes).  A map the window covers (kh_l >= h and kw_l >= w) is pooled globally, exactly as without the mode; otherwise
 * P[i][j] = mean of rows [r0, r0 + k1) x columns [c0, c0 + k2), k1 = min(h, kh_l), k2 = min(w, kw_l), r0 = clamp(i - (k1 - 1) / 2, 0, h - k1),
 * c0 = clamp(j - (k2 - 1) / 2, 0, w - k2), and the block scales every pixel by chan_conv(P) at that pixel.
 *   wdm_hfrm_set_local: all four zero -> global pooling (the default).  WDM_EINVAL for a non-positive size, a training size that is no
 *   multiple of 2^n_enc, or a window that is empty at some level.  Takes effect at the next wdm_hfrm_workspace_bytes / wdm_hfrm_forward (the
 *   local mode needs more workspace); no re-finalize needed.  In the local mode wdm_hfrm_forward refuses a workspace below wdm_hfrm_workspace_bytes
 *   with WDM_ENOMEM before its first launch (in the global mode, as before, at the first allocation that does not fit).
 *   wdm_hfrm_local_kernel: the frozen (kh_l, kw_l) of a level, 0 and 0 in global mode.
 *   wdm_hfrm_local_pool: the windowed mean alone, for tests: x (B, H, W, d) NHWC in dtype (WDM_F32: d % 4 == 0, WDM_BF16: d % 8 == 0) ->
 *   compact_out (B, H - k1 + 1, W - k2 + 1, d), same dtype, the mean of every k1 x k2 window (k1 = min(H, kh), k2 = min(W, kw)); fp32 sums in
 *   a fixed order (no atomics).  Allocates its own scratch and waits for the stream. */
int wdm_hfrm_set_local(wdm_hfrm* m, int base_h, int base_w, int train_h, int train_w);
int wdm_hfrm_local_kernel(const wdm_hfrm* m, int level, int* kh, int* kw);
int wdm_hfrm_local_pool(wdm_handle* h, const void* x, int B, int H, int W, int d, int kh, int kw, int dtype, void* compact_out, void* stream);
/* Pictures beyond the conv kernel's launch range.  Every 1x1 / 2x2 convolution of the HFRM is a GEMM on a kernel that addresses its operands through
 * buffer descriptors with 32-bit offsets: an input below 4 294 901 760 bytes, an output or residual below 4 026 531 840.  A GEMM with an operand beyond that
 * runs as several launches over consecutive row ranges -- each the largest multiple of 256 rows whose operands all stay below the limit, the last one the
 * remainder -- with the bits of a single launch; the closing 3x3 conv_out then runs on a direct kernel without extents (fp32 accumulation in another order
 * than the MFMA form).  A picture within the range takes the launches it always took.  wdm_hfrm_forward refuses more than 2^27 pixels per image (the bound up to
 * which every index of the path is checked) with WDM_EINVAL before its first launch; below that the workspace decides.
 *   wdm_hfrm_set_max_launch_bytes: lowers both limits to `bytes` (never raises them), for tests and diagnosis; 0 restores the kernels' own.  WDM_EINVAL
 *   for a negative value or one that does not hold a 256-row tile of the model's widest GEMM operand.  Takes effect at the next forward.
 *   wdm_hfrm_chunk_rows: host only -- the rows per launch of a GEMM of M rows, cin -> cout channels, under the current limit (M itself: one launch).
 *   wdm_hfrm_conv_out: the direct conv_out alone, for tests: x (B, H, W, cin) NHWC and res (B, H, W, cout) NHWC in dtype (WDM_F32 or WDM_BF16), w (cout, cin,
 *   3, 3) and bias fp32 (w is rounded to dtype as the packed copy is) -> y (B, cout, H, W) f32 = conv3x3(x, pad 1) + bias + res.  cin = 32, cout = 3.  Waits
 *   for the stream. */
int wdm_hfrm_set_max_launch_bytes(wdm_hfrm* m, int64_t bytes);
int wdm_hfrm_chunk_rows(const wdm_hfrm* m, int64_t M, int cin, int cout, int has_res, int64_t* rows);
int wdm_hfrm_conv_out(wdm_handle* h, const void* x, const void* res, const float* w, const float* bias, int B, int H, int W, int cin, int cout, int dtype,
                      float* y, void* stream);
/* One stage of a created, finalized HFRM on its own (unit tests): the very members wdm_hfrm_forward runs (run_block, gemm_rows, the same launches), on the caller's
 * tensors, so a per-stage reference cannot drift from the model.  Waits for the stream -- not a building block of a forward.
 *   kind WDM_HFRM_STAGE_BLOCK:    index = the block's position in registration order (encoders, decoders, mid_blks); x, y (B, H, W, d) NHWC in the model dtype
 *        WDM_HFRM_STAGE_DOWN:     downs[index]: x (B, H, W, d) -> y (B, H/2, W/2, 2d); H and W even
 *        WDM_HFRM_STAGE_UP:       ups[index] + PixelShuffle + skip: x (B, H, W, d), skip and y (B, 2H, 2W, d/2)
 *        WDM_HFRM_STAGE_CONV_IN:  x (B, in_channel, H, W) NCHW f32 -> y (B, H, W, dim) NHWC in the model dtype
 *        WDM_HFRM_STAGE_CONV_OUT: the MFMA form: x (B, H, W, dim) NHWC, the residual (B, H, W, in_channel) NHWC as `skip`, both in the model dtype -> y (B, in_channel,
 *                                 H, W) NCHW f32; H and W multiples of 8 -- the smallest tile of the conv kernel it runs on is 8 x 8 pixels and its dispatcher
 *                                 refuses any other map (every map wdm_hfrm_forward gives it is a multiple of 16); for other sizes there is wdm_hfrm_conv_out
 * Any other H, W >= 1.  Honours wdm_hfrm_set_local (a block pools at its level's window) and wdm_hfrm_set_max_launch_bytes.  All tensors 16-byte aligned, the
 * workspace 256-byte aligned and at least wdm_hfrm_stage_workspace_bytes (0 on a bad kind, index or shape), else WDM_ENOMEM before the first launch.
 * Additions to the ABI: WDM_ABI_VERSION stays 1. */
enum { WDM_HFRM_STAGE_BLOCK = 0, WDM_HFRM_STAGE_DOWN = 1, WDM_HFRM_STAGE_UP = 2, WDM_HFRM_STAGE_CONV_IN = 3, WDM_HFRM_STAGE_CONV_OUT = 4 };
size_t wdm_hfrm_stage_workspace_bytes(const wdm_hfrm* m, int kind, int index, int B, int H, int W);
int wdm_hfrm_stage_forward(wdm_hfrm* m, int kind, int index, const void* x, const void* skip, int B, int H, int W, void* y, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- output side of DiffusiveRestoration.restore ---------------------------------
 * wdm_image_sqdiff: a, b (B,3,H,W) f32 on the device -> sums[B][2] (device, fp64):
 *   [0] = sum over 3 channels and pixels of (clamp01(a) - clamp01(b))^2   -> torchPSNR, utils/metrics.py:7-11
 *   [1] = sum over pixels of (Y(a) - Y(b))^2, Y = (24.966 c0 + 128.553 c1 + 65.481 c2 + 16)/255
 *                                                                          -> calculate_psnr_in_GPU(.., True), :30-51
 * wdm_to_u8_hwc: (B,C,H,W) f32 -> (B,H,W,C) u8 with torchvision.utils.save_image's rounding
 *   (x*255 + 0.5, clamp to [0,255], truncate), replacing utils/logging.py:9-12's device->host float copy. */
int wdm_image_sqdiff(wdm_handle* h, const float* a, const float* b, int B, int H, int W, double* sums, void* stream);
int wdm_to_u8_hwc(wdm_handle* h, const float* x, int B, int C, int H, int W, uint8_t* y, void* stream);

/* ---- input side of DiffusiveRestoration.restore_folder: photographs at their own size ----------------
 * wdm_image_ingest: src (B,H,W,3) u8 HWC -> dst (B,3,Hp,Wp) f32 NCHW in [0,1], value (float)u8 / 255.0f as a correctly rounded division (the bits of
 *   torch.from_numpy(a).float().div(255)); rows H..Hp-1 and columns W..Wp-1 are filled by symmetric extension that is total for any pad length: the source
 *   row of output row y is s = y mod 2H, s >= H -> 2H-1-s, columns likewise (numpy.pad(mode="symmetric"): [0 1 2] -> [0 1 2 2 1 0 0 1 2 ...]).
 *   1 <= H <= Hp, 1 <= W <= Wp, B >= 1, Wp a multiple of 4, dst 16-byte aligned (else WDM_EINVAL); 64-bit element offsets.
 * wdm_to_u8_hwc_crop: x (B,C,Hp,Wp) f32 -> y (B,H,W,C) u8 from the top-left H x W window, wdm_to_u8_hwc's rounding (its bits when H == Hp and W == Wp). */
int wdm_image_ingest(wdm_handle* h, const uint8_t* src, int B, int H, int W, float* dst, int Hp, int Wp, void* stream);
int wdm_to_u8_hwc_crop(wdm_handle* h, const float* x, int B, int C, int Hp, int Wp, int H, int W, uint8_t* y, void* stream);

/* ---- orientations of whole fp32 pictures: the HFRM's test-time self-ensemble (csrc/imageio.hip) ----------------
 * Orientation code o in 0 .. 7, data.augment's (the comment above wdm_data_draw_oriented): O_o(t) = o & 1: t.flip(-1), then o & 2: t.flip(-2), then o & 4: t.transpose(-1, -2).
 * Its inverse D_o undoes the steps in reverse order: transpose if o & 4, then flip(-2) if o & 2, then flip(-1) if o & 1 -- the same map for every code but the
 * two quarter turns 5 and 6, which are each other's inverse.
 * wdm_image_orient: x (B,C,H,W) f32 NCHW -> y = O_o(x), (B,C,H,W) without bit 2 and (B,C,W,H) with it; a copy: the bits of x.
 * wdm_image_deorient_accumulate: H and W are ACC's; y is (B,C,H,W) without bit 2 of o and (B,C,W,H) with it (what wdm_image_orient wrote for these H, W, o).
 *   first != 0: acc = D_o(y) * scale;  first == 0: acc = (acc + D_o(y)) * scale -- fp32, the sum rounded once, then the product; 0 < scale <= 1, and 1.0f
 *   leaves the bits alone.  The mean of K members in ascending order is K calls, first on the first, scale = 1/K on the last, 1.0f before; no atomics, and
 *   every element of acc is written by one thread.
 * Both: any B, C, H, W >= 1 within a grid of 2^31 - 1 tiles of 64 x 64; 64-bit element offsets; pointers 4-byte aligned, and 16-byte accesses on a side whose
 * rows are a multiple of 4 long when both pointers are 16-byte aligned.  x and y (y and acc) must not overlap.  o outside 0 .. 7, a size below 1, a misaligned
 * or null pointer, a scale outside (0, 1]: WDM_EINVAL, nothing is launched.  Queued on `stream`; no host synchronisation. */
int wdm_image_orient(wdm_handle* h, const float* x, int B, int C, int H, int W, int o, float* y, void* stream);
int wdm_image_deorient_accumulate(wdm_handle* h, const float* y, int B, int C, int H, int W, int o, int first, float scale, float* acc, void* stream);

/* ---- training data resident in HBM (wavedm_amd/device_data.py: DeviceImageStore; csrc/device_data.hip) ----------------
 * The store: N (input, ground truth) pairs as uint8 HWC in one flat device buffer `pixels` without padding; `offsets` (N,2) int64 = byte offset of pair i's
 * input and ground truth, `sizes` (N,2) int32 = H, W of pair i (both images of a pair).  Read-only for every call here.
 * wdm_data_draw: the (img, row, col) int32 triples of the n_items * patch_n samples of a step whose first item has global number g0.  Item G = g0 + j lies in
 *   epoch E = G / N at position G % N and takes image perms[(E - perm_epoch0) * N + G % N] (`perms`: n_perm permutations of N int32, epochs perm_epoch0 ...; the
 *   items' epochs must lie inside, else WDM_EINVAL).  Crop q of item G: u = G * patch_n + q as a 64-bit number, Philox4x32-10 (csrc/dropout.h) with key
 *   (data_seed low word, high word) at counter (u low, u high, 0x43524F50, 0) gives words w0, w1: row = (w0 * (H - p + 1)) >> 32, col = (w1 * (W - p + 1)) >> 32
 *   in 64-bit arithmetic.  p == 0: whole images, row = col = 0.  Images smaller than p are the caller's to refuse (the store does).
 * wdm_train_sample_gather: triples (n) -> x0 (n, 48 + pred_channels + 48 - other_channels_begin, p/4, p/4) f32 NCHW =
 *   [DWT(2 in - 1) | DWT(2 gt - 1)[:pred_channels] | DWT(2 gt - 1)[other_channels_begin:]] of each p x p crop, in = u8 / 255 correctly rounded (wdm_image_ingest's
 *   rule), the transform wdm_dwt_fwd's arithmetic: the bits of assemble_training_sample (model.use_gt_in_train) on the same crops cut on the host.  crops01
 *   (optional, 16-byte aligned): (n, 6, p, p) f32 = [in | gt] in [0,1].  p a multiple of 4; 1 <= pred_channels <= 48; 0 <= other_channels_begin <= 48; n >= 1 and
 *   within the launch grid; else WDM_EINVAL and nothing is launched.  64-bit element offsets (a store may exceed 4 GB); no load wider than a byte from an
 *   address that is not a multiple of its width.
 *   CONTRACT: the kernel cannot check a triple against its image.  0 <= img < N, 0 <= row <= H - p, 0 <= col <= W - p are the caller's to guarantee
 *   (wdm_data_draw's triples do); so is the truth of the tables.
 * wdm_store_gather_images: images idx[k * idx_stride] (k < n) of a store whose images all measure H x W -> inp, gt (n,3,H,W) f32 NCHW in [0,1] (u8 / 255,
 *   to_tensor's bits): the HFRM trainer's batch.  idx may be the first column of a triple buffer (idx_stride 3).
 * All three are queued on `stream`; no launch argument depends on a device result; no host synchronisation. */
int wdm_data_draw(wdm_handle* h, const int32_t* sizes, int64_t n_images, const int32_t* perms, int64_t perm_epoch0, int n_perm, int64_t g0, int n_items,
                  int patch_n, int p, int64_t data_seed, int32_t* triples, void* stream);
int wdm_train_sample_gather(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const int32_t* triples, int n, int p,
                            int pred_channels, int other_channels_begin, float* x0, float* crops01, void* stream);
int wdm_store_gather_images(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* idx, int idx_stride, int n, int H, int W, float* inp,
                            float* gt, void* stream);

/* ---- orientations of those crops and images (data.augment) ----------------
 * Orientation code o in 0 .. 7 on a square crop or a whole image t (.., H, W), in this order: o & 1: t = t.flip(-1) (mirror left-right); o & 2: t = t.flip(-2)
 * (mirror top-bottom); o & 4: t = t.transpose(-1, -2) -- the eight symmetries of the square, each once.  The input and the ground truth of a sample take the same o.
 * orient_mask in 0 .. 7 (else WDM_EINVAL): 0 none, 1 hflip, 3 flips, 7 d4.
 * wdm_data_draw_oriented: wdm_data_draw's arguments, checks and triples (same values, same layout), and orient[j * patch_n + q] = (w2 >> 29) & orient_mask, w2 =
 *   word 2 of the crop counter that gives row and col.  With p == 0 (whole images; the triples take no Philox word) the same counter is evaluated, u = G * patch_n + q.
 *   Whether bit 2 suits the images (whole images must be square) is the caller's to decide through orient_mask.
 * wdm_train_sample_gather_oriented: wdm_train_sample_gather's arguments, checks and outputs, each sample's crop oriented by orient[sample] first: x0 and crops01
 *   are the bits of assemble_training_sample on the host-cut crops after the three torch operations above.  One launch serves samples of different codes.
 *   CONTRACT: like the triples, the codes cannot be checked against anything on the device; values outside 0 .. 7 are the caller's responsibility.  The kernel
 *   uses orient[sample] & 7, so no value can address outside the crop.
 * wdm_store_gather_images_oriented: wdm_store_gather_images's outputs with image k oriented by orient[k] & orient_mask.  orient_mask & 4 needs H == W (a transposed
 *   H x W image is W x H and would not fit the batch), else WDM_EINVAL; with it cleared, no device value can transpose.
 * Every WDM_EINVAL launches nothing.  Queued on `stream`; no launch argument depends on a device result; no host synchronisation. */
int wdm_data_draw_oriented(wdm_handle* h, const int32_t* sizes, int64_t n_images, const int32_t* perms, int64_t perm_epoch0, int n_perm, int64_t g0, int n_items,
                           int patch_n, int p, int64_t data_seed, int orient_mask, int32_t* triples, int32_t* orient, void* stream);
int wdm_train_sample_gather_oriented(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const int32_t* triples,
                                     const int32_t* orient, int n, int p, int pred_channels, int other_channels_begin, float* x0, float* crops01, void* stream);
int wdm_store_gather_images_oriented(wdm_handle* h, const uint8_t* pixels, const int64_t* offsets, const int32_t* idx, int idx_stride, const int32_t* orient,
                                     int orient_mask, int n, int H, int W, float* inp, float* gt, void* stream);

/* wdm_image_ssim: a, b (B images each, layout by `kind`) on the device -> out[B] (device, fp64): SSIM of each pair as calculate_ssim defines it
 * (utils/metrics.py:82-149; Y conversion :152-255) -- 11x11 Gaussian window (sigma 1.5) over the valid (H-10) x (W-10) region, C1 = (0.01*255)^2,
 * C2 = (0.03*255)^2, moments and map in fp64, the map's mean.
 *   kind WDM_IMG_F32_NCHW: (B,3,H,W) f32 in [0,1], taken as clamp(x*255, 0, 255) in f32 (models/restoration.py:144);
 *        WDM_IMG_U8_HWC:   (B,H,W,3) u8;   WDM_IMG_F32_HWC: (B,H,W,3) f32 already on [0,255], taken as is.
 *   y_only 1: to_y_channel's Y (float32 steps as the reference; weights [24.966, 128.553, 65.481] on the channels in storage order, as
 *             wdm_image_sqdiff's Y) -> calculate_ssim(.., test_y_channel=True);  0: mean of the three per-channel SSIMs.
 * H, W >= 11 (else WDM_EINVAL), 1 <= B <= 65535.  `scratch` holds per-tile partial sums: at least the byte count the size query returns for
 * (B, H, W), else WDM_ENOMEM.  Fixed reduction order, no atomics: an image's value does not depend on the batch around it; identical inputs
 * give exactly 1.0.  Queued on `stream`, no host synchronisation. */
enum { WDM_IMG_F32_NCHW = 0, WDM_IMG_U8_HWC = 1, WDM_IMG_F32_HWC = 2 };
size_t wdm_image_ssim_scratch_bytes(int B, int H, int W);
int wdm_image_ssim(wdm_handle* h, const void* a, const void* b, int kind, int y_only, int B, int H, int W, double* out, void* scratch,
                   size_t scratch_bytes, void* stream);

/* ---- training step: backward primitives, test entry points --------------------------
 * wdm_conv_backward: autograd of one convolution of models/unet.py (mode as wdm_conv_forward: 0 conv3x3 s1 p1, 1 Downsample,
 * 2 Upsample, 3 conv1x1).  x (B,cin,H,W), dy (B,cout,Ho,Wo), w OIHW f32 -> dx (B,cin,H,W) (optional), dw OIHW f32, db (cout) (optional). */
int wdm_conv_backward(wdm_handle* h, const float* w, int cin, int cout, int mode, const float* x, const float* dy, int B,
                      int H, int W, float* dx, float* dw, float* db, int dtype, void* scratch, size_t scratch_bytes,
                      void* stream);

/* wdm_gn_act_backward: autograd of GroupNorm(32, 1e-6)(+SiLU) (unet.py:31-37) over a channel concat [C0 | C - C0] of x (B,C,H,W);
 * dy (B,C,H,W) -> dx (B,C,H,W), dgamma (C), dbeta (C). */
int wdm_gn_act_backward(wdm_handle* h, const float* x, int C0, int C, const float* gamma, const float* beta, const float* dy,
                        int silu, int B, int H, int W, float* dx, float* dgamma, float* dbeta, int dtype, void* scratch,
                        size_t scratch_bytes, void* stream);

/* Dropout of the training step (model.dropout; csrc/dropout.h).  No mask is stored: the kernels draw it from Philox4x32-10 with key = seed and
 * counter = (e >> 3 low, e >> 3 high, layer, step) for the element index e = ((b H W) + pixel) C + c; element e takes 16-bit lane e & 7 of the call's
 * 128 bits and is kept iff lane >= round(65536 p); kept elements are scaled by 65536 / (65536 - round(65536 p)).  layer = the ResnetBlock's position in
 * wdm_trainer_param_info order (down, mid, up); step = the optimizer step being computed.
 * wdm_dropout_mask: the factor (0 or the scale) of every element of a (B, C, H, W) tensor, fp32 NCHW (C a multiple of 8), from the device function the
 * training kernels call.
 * wdm_gn_act_dropout: y = factor * silu(GroupNorm(32, 1e-6)(x)) of one (B, C, H, W) tensor and its autograd, dy -> dx, dgamma, dbeta, on the kernels the
 * training step launches for a ResnetBlock's norm2 (dtype: WDM_F32 or WDM_BF16).  p outside [0, 1) is WDM_EINVAL in all three. */
int wdm_dropout_mask(wdm_handle* h, float p, int64_t seed, int64_t step, int layer, int B, int H, int W, int C, float* factor_nchw,
                     void* stream);
int wdm_gn_act_dropout(wdm_handle* h, const float* x, int C, const float* gamma, const float* beta, const float* dy, int B, int H, int W,
                       float p, int64_t seed, int64_t step, int layer, float* y, float* dx, float* dgamma, float* dbeta, int dtype,
                       void* scratch, size_t scratch_bytes, void* stream);

/* ---- training step object -----------------------------------------------------------
 * Replaces the body of DenoisingDiffusion_Wavelet.train's inner loop (models/ddm_wavelet.py:259-272) for the raindrop_wavelet.yml
 * branch: noise_estimation_loss (:108-124) forward + backward, torch.optim.Adam step (utils/optimize.py:5-8) and EMAHelper.update
 * (:48-53).  Parameters, gradients, Adam moments and the EMA shadow are five caller-allocated flat fp32 DEVICE buffers sharing one
 * layout (wdm_trainer_param_info gives name, shape and float offset of every state_dict entry; the temb_proj layers sit at the end as
 * one [rows][4ch] matrix).  A data-parallel job all-reduces the gradient buffer between _step and _adam_ema.
 *   x0 (B, in_channels, R, R) f32: [x_cond | x_tar | x_other] in the wavelet domain; e (B, out_ch, R, R) noise; t (B) timesteps as
 *   float; sqrt_a / sqrt_1ma (B): sqrt(abar_t), sqrt(1 - abar_t) (device); c_t0: first channel of x_tar.
 *   loss (device float) = mean_b sum (e - out)^2; out_nchw (optional): the network output. */
typedef struct wdm_trainer wdm_trainer;
int wdm_trainer_create(wdm_handle* h, const wdm_unet_config* cfg, wdm_trainer** out);
int wdm_trainer_destroy(wdm_trainer* t);
int wdm_trainer_num_params(const wdm_trainer* t);
int64_t wdm_trainer_num_floats(const wdm_trainer* t);
int wdm_trainer_param_info(const wdm_trainer* t, int i, const char** name, int* ndim, int64_t shape[4], int64_t* offset);
int wdm_trainer_set_buffers(wdm_trainer* t, float* params, float* grads, float* m, float* v, float* ema);
/* training.use_mse (ddm_wavelet.py:263-266): back-propagate mse_loss = mean_b sum (x_tar - x0_pred)^2 instead of the noise-space loss
 * (default 0).  *loss of wdm_trainer_step stays the noise-space value either way. */
int wdm_trainer_set_objective(wdm_trainer* t, int use_mse);
/* model.dropout: state of the handle, read by the next wdm_trainer_step calls.  step = the optimizer step those calls compute (the trainer's count + 1);
 * p = 0 (the default) launches exactly the kernels of a model without dropout. */
int wdm_trainer_set_dropout(wdm_trainer* t, float p, int64_t seed, int64_t step);
int wdm_trainer_step(wdm_trainer* t, const float* x0, const float* tt, const float* sqrt_a, const float* sqrt_1ma, const float* e,
                     int B, int c_t0, float* loss, float* out_nchw, void* workspace, size_t workspace_bytes, void* stream);
/* One stage of the training step on its own (a test entry: it waits for the stream): the forward and then the backward of the stage through the very
 * members and graph ops wdm_trainer_step chains, on the caller's tensors, with every conv's weights packed from the parameter buffer as a step packs them.
 * Activations and their gradients are NHWC in the trainer's dtype; the map H x W is the caller's (not cfg.resolution).  A stage writes only its own entries
 * of the gradient buffer and only its own rows of d_temb_all.  `dx0_set` / `dx1_set`: the gradient buffer already holds a later consumer's gradient, and the
 * stage adds to it as the step does from the second consumer on.
 *   RESBLOCK index = the block's position among the ResnetBlocks in wdm_trainer_param_info order (also its dropout layer): x0 (B, H, W, cin - c1), x1
 *            (B, H, W, c1) the skip half of a concat (c1 = 0: none), temb_all (B, temb_rows) f32, dy -> y (B, H, W, cout), dx0, dx1, the block's rows of
 *            d_temb_all (B, temb_rows), its gradient entries.  Dropout as set by wdm_trainer_set_dropout.
 *   ATTN     index = the AttnBlock's position: x0, dy -> y, dx0 (B, H, W, c); H x W a token count the trainer's attention takes.
 *   CONV     index = the conv's position among the 4-d weights: conv_in (no dx0), a Downsample (y on H/2 x W/2) or an Upsample (y on 2H x 2W).
 *   TEMB     t (B), d_temb_all (B, temb_rows) -> temb_all, the gradients of temb.dense.0 / .1 and of every temb_proj weight and bias.
 *   INPUT    x0 (B, in_channels, H, W) NCHW f32, e (B, out_ch, H, W), sa, s1m (B), c_t0 -> x96 (B, H, W, in_channels) the built input, y conv_in's output;
 *            with dy also conv_in's gradients.  No dx.
 *   HEAD     x0 = h (B, H, W, ch), e, and sa / s1m under use_mse -> out_nchw (optional), loss, dx0, the gradients of norm_out and conv_out.
 * Tensors 16-byte aligned; the workspace 256-byte aligned and at least wdm_trainer_stage_workspace_bytes (0 on a bad kind, index or shape), all checked
 * before the first launch. */
enum { WDM_TRAINER_STAGE_RESBLOCK = 0, WDM_TRAINER_STAGE_ATTN = 1, WDM_TRAINER_STAGE_CONV = 2, WDM_TRAINER_STAGE_TEMB = 3, WDM_TRAINER_STAGE_INPUT = 4,
       WDM_TRAINER_STAGE_HEAD = 5 };
typedef struct wdm_trainer_stage_io {
    const void *x0, *x1, *dy;
    float *temb_all, *d_temb_all;
    const float *t, *e, *sa, *s1m;
    void *y, *x96, *dx0, *dx1;
    float *out_nchw, *loss;
    int c1, c_t0, dx0_set, dx1_set;
} wdm_trainer_stage_io;
size_t wdm_trainer_stage_workspace_bytes(const wdm_trainer* t, int kind, int index, int B, int H, int W);
int wdm_trainer_stage(wdm_trainer* t, int kind, int index, const wdm_trainer_stage_io* io, int B, int H, int W, void* workspace, size_t workspace_bytes,
                      void* stream);
int wdm_trainer_adam_ema(wdm_trainer* t, int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                         float ema_mu, void* stream);
/* The other optimizers utils/optimize.py:5-14 can build, as torch 2.10's single-tensor rules, each with the EMA update in the same pass over the flat
 * buffers (fp32, no atomics).  g is the gradient, g += weight_decay * p first (the reference's SGD call passes no weight decay: its callers pass 0):
 *   WDM_OPT_ADAM     state0 exp_avg, state1 exp_avg_sq                              the rule of wdm_trainer_adam_ema
 *   WDM_OPT_AMSGRAD  state0 exp_avg, state1 exp_avg_sq, state2 max_exp_avg_sq       vmax = max(vmax, v);
 *                    p -= lr / (1 - beta1^step) * m / (sqrt(vmax) / sqrt(1 - beta2^step) + eps)
 *   WDM_OPT_RMSPROP  state0 square_avg          s = beta2 s + (1 - beta2) g^2;  p -= lr g / (sqrt(s) + eps)     (beta2 = RMSprop's alpha; momentum 0, not centered)
 *   WDM_OPT_SGD      state0 momentum_buffer     buf = g at step 1, beta1 buf + g afterwards;  p -= lr buf       (beta1 = the momentum; dampening 0, no Nesterov)
 * Arguments a rule does not use are ignored; its state buffers are required.  The hyper-parameters are doubles: 1 - beta, the bias corrections and
 * lr / (1 - beta1^step) are formed from them as torch forms them from Python floats, then rounded to fp32 once.
 * wdm_trainer_set_optimizer selects the rule of a trainer and hands over its state buffers (wdm_trainer_num_floats floats each; WDM_OPT_ADAM, the default,
 * replaces m / v of wdm_trainer_set_buffers); wdm_trainer_optim_step applies it to the trainer's parameters, gradients and EMA shadow.
 * wdm_optim_step applies one step to caller-owned buffers of n >= 0 floats: 16-byte accesses where every buffer shares one misalignment from a 16-byte
 * boundary, scalar ends (and scalar throughout where they do not); ema may be NULL. */
enum { WDM_OPT_ADAM = 0, WDM_OPT_AMSGRAD = 1, WDM_OPT_RMSPROP = 2, WDM_OPT_SGD = 3 };
int wdm_trainer_set_optimizer(wdm_trainer* t, int rule, float* state0, float* state1, float* state2);
int wdm_trainer_optim_step(wdm_trainer* t, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                           double ema_mu, void* stream);
int wdm_optim_step(wdm_handle* h, int rule, float* params, const float* grads, float* state0, float* state1, float* state2, float* ema,
                   int64_t n, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, double ema_mu,
                   void* stream);
/* ---- guard of the training step: global gradient-norm clipping and non-finite skip (no counterpart in the reference's loop) ----
 * wdm_grad_guard takes the 2-norm of a flat fp32 buffer of n >= 0 floats (any alignment) on the device and writes a record of four words:
 *   norm           sqrt(sum g^2) -- every square and the whole sum in fp64 (a square of an fp32 is exact there), rounded to fp32 once.  One gradient of 1e30 gives
 *                  1e30, where an fp32 sum of squares gives infinity.  Two launches whose shape follows n alone, fixed summation order, no atomics: the same
 *                  buffer gives the same bits.
 *   coef           torch.nn.utils.clip_grad_norm_'s factor in fp32, min(1, max_norm / (norm + 1e-6f)); exactly 1.0f when max_norm <= 0 (clipping off).  A
 *                  non-finite norm gives what that arithmetic gives (NaN from NaN, 0 from infinity), as clip_grad_norm_(error_if_nonfinite=False) does.
 *   skip           skip_nonfinite && some gradient is NaN or infinite (the fp64 sum cannot overflow, so it is non-finite exactly then)
 *   skipped_total  += skip: the caller zeroes the record once, before its first step
 * scratch: wdm_grad_guard_scratch_bytes bytes, 8-byte aligned, only live between the two launches.  The gradient buffer is read only.  WDM_EINVAL: a null
 * pointer, n < 0, NaN max_norm, scratch too small.
 * The _guarded steps are wdm_optim_step (all four rules, plain Adam too), wdm_trainer_optim_step and wdm_hfrm_trainer_adam behind such a record, which they read
 * on the device -- nothing returns to the host and no launch argument depends on it.  skip != 0: the kernel returns before its first store; parameters, every
 * state buffer and the EMA shadow keep their bits.  Otherwise g = grad * coef is formed first, as a product of its own (torch scales .grad in place before the
 * optimizer sees it, so weight decay is added to the scaled gradient), and the rule's arithmetic follows unchanged: coef == 1 gives the bits of the unguarded
 * entry.  `step` is the caller's count of CALLS and advances over a skipped step too (bias corrections, dropout counters, checkpoints and lr schedules count
 * calls).  WDM_OPT_SGD: a step 1 that may be skipped needs a zeroed momentum buffer -- the skipped kernel leaves it untouched and step 2 forms beta1 * 0 + g, the
 * buffer step 1 would have created. */
typedef struct wdm_grad_record {
    float norm, coef;
    int32_t skip, skipped_total;
} wdm_grad_record;
size_t wdm_grad_guard_scratch_bytes(void);
int wdm_grad_guard(wdm_handle* h, const float* grads, int64_t n, float max_norm, int skip_nonfinite, wdm_grad_record* record, void* scratch,
                   size_t scratch_bytes, void* stream);
int wdm_optim_step_guarded(wdm_handle* h, int rule, float* params, const float* grads, float* state0, float* state1, float* state2, float* ema,
                           int64_t n, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay, double ema_mu,
                           const wdm_grad_record* record, void* stream);
int wdm_trainer_optim_step_guarded(wdm_trainer* t, int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                                   double ema_mu, const wdm_grad_record* record, void* stream);
/* Gradient buckets for a data-parallel all-reduce that overlaps the backward (the reference wraps the model in DistributedDataParallel, ddm_wavelet.py:168,
 * which all-reduces 25 MB buckets while the backward runs).  The parameters sit in the flat buffers in forward order and the backward runs in reverse, so the
 * gradient buffer fills from its end: with n events set (hipEvent_t handles owned by the caller; n = 0 switches the feature off) every following
 * wdm_trainer_step cuts the filled range into at most n buckets of about equal size and records event k on the step's stream behind the last launch that
 * writes bucket k.  wdm_trainer_grad_buckets returns the bounds of the last step in float elements of the gradient buffer, descending:
 * bucket k = [bounds[k + 1], bounds[k]), 0 <= k < *n_buckets <= n (bounds needs room for n + 1 values).  What lies outside [bounds[n_buckets], bounds[0]) --
 * the timestep-embedding MLP and the temb_proj matrix -- is final only when the whole step is. */
int wdm_trainer_set_grad_events(wdm_trainer* t, void* const* events, int n);
int wdm_trainer_grad_buckets(const wdm_trainer* t, int64_t* bounds, int max_bounds, int* n_buckets);

/* ---- HFRM training step -------------------------------------------------------------------------------
 * Replaces the body of train_hfrm.py's loop (train_hfrm.py:240-268): HFRM forward, the back-propagated loss
 * 2 * mean|255 out - 255 target| = 510 * mean|out - target| (the perceptual terms are commented out there) and its backward, and
 * torch.optim.Adam with no EMA.  cfg->dtype = WDM_F32 only (the type of the parameters and the optimizer state), the reference's HFRM widths
 * (dim 32, in_channel 3, <= 4 levels).
 * Parameters, gradients and the Adam moments are four caller-allocated flat fp32 DEVICE buffers of wdm_hfrm_trainer_num_floats floats sharing one
 * layout: wdm_hfrm_trainer_param_info gives name, shape and float offset of every state_dict entry, in the reference's registration order.
 *   x (B, 3, H, W) NCHW f32, H and W multiples of 16; pass exactly one of target (B, 3, H, W) -- the reference loss, *loss (device float) is
 *   written -- or dy (B, 3, H, W), an upstream gradient of the output (the loss is not computed, loss may be NULL).  The step writes every entry of
 *   the gradient buffer (not accumulated); out (optional, B x 3 x H x W) receives the forward output.  Deterministic: no float atomics.
 *   wdm_hfrm_trainer_workspace_bytes: the exact workspace of a step at (B, H, W) (a dry run of the step's allocations); 0 on a bad shape.  The step
 *   checks workspace_bytes against that figure before its first launch (WDM_ENOMEM, "workspace too small").
 *   wdm_hfrm_trainer_set_precision: the storage type of activations and activation gradients.  WDM_F32 (the state after create): exact fp32.
 *   WDM_BF16: mixed precision -- activations, saved tensors and activation gradients in bf16 (round to nearest even), the 1x1 / downs GEMMs and their
 *   weight gradients on the bf16 MFMA path with fp32 accumulation; parameters, gradients, Adam moments, partial sums, the loss and all other arithmetic
 *   stay fp32, so the four buffers, their layout and wdm_hfrm_trainer_adam are the same in both modes.  No loss scaling (bf16 has fp32's exponent
 *   range); WDM_F16 is refused for that reason, anything else is WDM_EINVAL.  Legal between steps; workspace_bytes and step follow the setting. */
typedef struct wdm_hfrm_trainer wdm_hfrm_trainer;
int wdm_hfrm_trainer_create(wdm_handle* h, const wdm_hfrm_config* cfg, wdm_hfrm_trainer** out);
int wdm_hfrm_trainer_destroy(wdm_hfrm_trainer* t);
int wdm_hfrm_trainer_num_params(const wdm_hfrm_trainer* t);
int64_t wdm_hfrm_trainer_num_floats(const wdm_hfrm_trainer* t);
int wdm_hfrm_trainer_param_info(const wdm_hfrm_trainer* t, int i, const char** name, int* ndim, int64_t shape[4], int64_t* offset);
int wdm_hfrm_trainer_set_buffers(wdm_hfrm_trainer* t, float* params, float* grads, float* m, float* v);
int wdm_hfrm_trainer_set_precision(wdm_hfrm_trainer* t, int act_dtype);
size_t wdm_hfrm_trainer_workspace_bytes(const wdm_hfrm_trainer* t, int B, int H, int W);
int wdm_hfrm_trainer_step(wdm_hfrm_trainer* t, const float* x, const float* target, const float* dy, int B, int H, int W, float* loss, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* One stage of the training step on its own (unit tests), the trainer's counterpart of wdm_hfrm_stage_forward: the forward and then the backward of one stage, through
 * the very members wdm_hfrm_trainer_step chains (fwd_block / bwd_block, down_fwd / down_bwd, up_fwd / up_bwd, conv_in_fwd / conv_in_wgrad, conv_out_fwd / conv_out_bwd),
 * on the caller's tensors, with the weights packed from the parameter buffer as a step packs them.  Activations and their gradients are NHWC in the trainer's current
 * storage type (wdm_hfrm_trainer_set_precision: f32 or bf16); kinds and indices as wdm_hfrm_stage_forward.
 *   WDM_HFRM_STAGE_BLOCK:    x, y, dy, dx (B, H, W, d); every gradient entry of the block is written
 *   WDM_HFRM_STAGE_DOWN:     x (B, H, W, d) -> y (B, H/2, W/2, 2d); dy like y; dx (B, H, W, d) holds on entry the gradient that arrived over the skip connection and on
 *                            return that gradient plus the adjoint of the gather (unshuffle2_kernel's add form); downs[index] weight and bias; H and W even
 *   WDM_HFRM_STAGE_UP:       x (B, H, W, d), skip (B, 2H, 2W, d/2) -> y like skip; dy like y -> dx (B, H, W, d); ups[index] weight.  The gradient of skip is dy itself:
 *                            no kernel runs for it and none is returned
 *   WDM_HFRM_STAGE_CONV_IN:  x (B, 3, H, W) NCHW f32 -> y (B, H, W, 32); dy like y; there is no dx (may be NULL); conv_in weight and bias
 *   WDM_HFRM_STAGE_CONV_OUT: x (B, H, W, 32), skip = the image (B, 3, H, W) NCHW f32 -> y (B, 3, H, W) NCHW f32; dy NCHW f32 -> dx (B, H, W, 32); conv_out weight and
 *                            bias; H and W multiples of 8 -- the smallest tile of the conv kernel its forward runs on is 8 x 8 pixels
 * Any other H, W >= 1.  Only the stage's own entries of the gradient buffer are written, everything else stays untouched.  All tensors 16-byte aligned; the workspace
 * 256-byte aligned and at least wdm_hfrm_trainer_stage_workspace_bytes (0 on a bad kind, index or shape), checked before the first launch (WDM_ENOMEM).  Waits for the
 * stream -- a test entry, not a building block.  Additions to the ABI: WDM_ABI_VERSION stays 1. */
size_t wdm_hfrm_trainer_stage_workspace_bytes(const wdm_hfrm_trainer* t, int kind, int index, int B, int H, int W);
int wdm_hfrm_trainer_stage(wdm_hfrm_trainer* t, int kind, int index, const void* x, const void* skip, const void* dy, int B, int H, int W, void* y, void* dx,
                           void* workspace, size_t workspace_bytes, void* stream);
/* the betas are doubles: torch forms 1 - beta and the bias corrections from the Python floats (an fp32 0.999 puts 1 - beta2 1.3e-5 off) */
int wdm_hfrm_trainer_adam(wdm_hfrm_trainer* t, int64_t step, float lr, double beta1, double beta2, float eps, float weight_decay, void* stream);
/* ... behind the record of wdm_grad_guard over the trainer's gradient buffer (see there) */
int wdm_hfrm_trainer_adam_guarded(wdm_hfrm_trainer* t, int64_t step, float lr, double beta1, double beta2, float eps, float weight_decay,
                                  const wdm_grad_record* record, void* stream);

/* ---- live kernel timing (bench.py roofline leg) ----------------------------------------------
 * While enabled, every convolution launch is bracketed by two HIP events on its own stream and
 * tagged with its algorithmic flops (2*M*N*K) and bytes (input + weights + output once).
 * wdm_prof_report synchronises those events, aggregates per kernel configuration and clears. */
typedef struct wdm_prof_entry {
    char kernel[96];
    long long launches;
    double total_ms, total_flops, total_bytes;
} wdm_prof_entry;
int wdm_prof_enable(int on);
int wdm_prof_report(wdm_prof_entry* out, int max_entries, int* n_entries);

/* ---- experiment switches ------------------------------------------------------------------------
 * The WDM_* environment variables (alternative kernels kept for A/B runs; defaults are the measured best) are read once, at
 * first use -- no launch path calls getenv.  A harness that changes them inside a running process calls this to have them read again.
 * (No counterpart in the reference: csrc/common.h EnvCfg.) */
int wdm_env_refresh(void);

/* ---- concurrent streams -------------------------------------------------------------------------
 * A caller that keeps n independent forward calls in flight on n HIP streams (wavedm_amd/sampling.py: chunks of independent crops) says so here: the tile
 * choices that follow the workgroup count of ONE launch ("256-column tiles where they still fill the chip") then count n launches side by side.  Those
 * alternatives write the same bits, so this changes speed only.  n = 1 (default): one launch owns the chip.  (No counterpart in the reference.)
 *
 * HAZARD, measured and not root-caused (EXPERIMENTS.md, round 3 "chunks of independent crops on separate HIP streams"): with four chunks on four streams the
 * sampler gains 0 ... +5 % when every pass takes streams it has not used before, and LOSES 35 % (126 -> 83 img/s, every box) when the same four stream
 * objects carry pass after pass -- also on every eighth pass of a caller that draws from a pool of 32.  GPU_MAX_HW_QUEUES = 1 / 2 are worse still, so the
 * mapping of streams onto the hardware queues is involved; what exactly is not understood.  The library itself creates no streams and keeps no per-stream
 * state (each call's scratch is the caller's workspace), so nothing here depends on which stream a call arrives on: the effect is in the runtime's queue
 * assignment.  Until it is understood, run ONE stream per device (the default everywhere in wavedm_amd; sampling.ddim_sample(streams=) is opt-in) and do
 * not cache side streams across passes. */
int wdm_set_concurrent_streams(int n);

#ifdef __cplusplus
}
#endif
#endif /* WAVEDM_H */
