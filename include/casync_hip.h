/*
 * casync_hip.h -- C ABI of libcasync_hip.so, the MI355X (gfx950) engine for the
 * CASync lip-sync U-Net per-frame inference forward.
 *
 * The reference has no FFI: its boundary for this path is the Python call
 *     predictions = self.net(batch_tensor, hubert_tensor)
 * (reference image_infer_v1/tools/frame_synthesizer/infer_api.py:259-260) on an
 * nn.Module built by Model(6, "hubert") / load_state_dict / eval()
 * (infer_api.py:41-43; module/unet.py:273-345).  This library is what a
 * binding for that call binds: plain pointers and sizes, explicit stream, int
 * status codes, no C++ exceptions, no torch types.  calipsync_amd/unet.py is
 * the ctypes host that keeps the reference's Model.forward(x, audio_feat)
 * signature on top of it (INTEGRATION.md shows the stub).
 *
 * All device pointers are fp32, 16-byte aligned.  Tensors at the boundary are
 * the reference's own layouts (NCHW, contiguous); internally the engine works
 * in NHWC.  A handle is bound to one device and is not thread-safe: one
 * caller / one stream at a time (the reference has one caller at a time,
 * infer_api.py:259 under inference.py:80 or a worker thread).
 */
#ifndef CASYNC_HIP_H
#define CASYNC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct casync_engine* casync_handle;
typedef void* casync_stream;          /* a hipStream_t (NULL = default stream) */

/* status codes (0 = ok, negative = error; never throws) */
enum {
  CASYNC_OK = 0,
  CASYNC_ERR_ARG = -1,        /* null pointer / bad size / unsupported shape   */
  CASYNC_ERR_HIP = -2,        /* a HIP runtime call failed (see last_error)    */
  CASYNC_ERR_STATE = -3,      /* weights not loaded / workspace too small      */
  CASYNC_ERR_NO_DEVICE = -4   /* no gfx950 device visible                      */
};

/* ---- introspection (callable without a GPU) --------------------------- */
/* Bumped on every change of a prototype, struct layout or the packed-weight layout; the ctypes
 * host (calipsync_amd/_lib.py) refuses a library whose version differs from the one it binds.   */
#define CASYNC_ABI_VERSION 13  /* 12: S3FD face detector handle (casync_s3fd_*, casync_op_s3fd_*); 13: its bf16 precision
                                * (casync_s3fd_create_ex, _precision, _workspace_bytes_ex, casync_op_s3fd16_*).  The face-pipeline
                                * operators at the end of this file (casync_op_resize_linear_u8, _face_crops192, _s3fd_candidates,
                                * _landmarks_finalize), casync_op_s3fd_nms, casync_op_clip_gather / _compose, casync_op_jpeg_*, casync_op_jpeg420_*, casync_op_jpegdec_* and casync_op_mjpegdec_* were added under 13: new symbols only, no prototype or layout changed */
int         casync_abi_version(void);
const char* casync_last_error(void);           /* thread-local message         */

/* Packed-weight layout.  The host folds eval-mode BatchNorm into the conv /
 * linear weights (replaces nn.BatchNorm2d/1d + bias adds, module/unet.py:18,
 * 28,32,163,168,174,228,230,260,301,310,311) and writes each folded tensor at
 * the offset this table names.  Offsets/sizes are in floats.               */
int         casync_packed_count(void);
const char* casync_packed_name(int i);
int64_t     casync_packed_offset(int i);
int64_t     casync_packed_size(int i);
int64_t     casync_packed_total(void);          /* floats in the whole buffer  */

/* Audio encoder of a handle (reference Model(6, mode), module/unet.py:281-284), fixed at creation.
 * The entries without a mode argument mean CASYNC_AUDIO_HUBERT.                                  */
enum {
  CASYNC_AUDIO_HUBERT = 0,    /* AudioConvHubert: audio [B,32,32,32], 582-key state_dict       */
  CASYNC_AUDIO_WENET = 1      /* AudioConvWenet:  audio [B,256,16,32], 577 keys (no bn7)       */
};
/* The packed layout of one audio mode (wenet: no audio_model.bn7.s/.t, conv1 / conv2 take 256
 * channels, conv3.w is 256 x 9 x 256).  An unknown mode answers 0 / NULL / -1.                   */
int         casync_packed_count_m(int audio_mode);
const char* casync_packed_name_m(int audio_mode, int i);
int64_t     casync_packed_offset_m(int audio_mode, int i);
int64_t     casync_packed_size_m(int audio_mode, int i);
int64_t     casync_packed_total_m(int audio_mode);

/* Workspace (activations, NHWC fp32) needed for a batch of B frames.        */
int64_t     casync_workspace_bytes(int batch);               /* fp32 engine            */
int64_t     casync_workspace_bytes_dt(int batch, int dtype); /* 0 = fp32, 1 = bf16     */
/* ... for THIS handle (its dtype, audio mode and options: the arena is smaller when the fused kernels
 * are on, which is the default).  Any arena at least this large is accepted by casync_forward.  */
int64_t     casync_workspace_bytes_h(casync_handle h, int batch);

/* ---- tuning options ---------------------------------------------------- */
/* Every switch of the engine by name (the CASYNC_<NAME> environment variables, lower case without
 * the prefix: "lanes", "trunk_lanes", "overlap", "gemm_streamk", "fuse_ir", "fuse_q", ... -- DESIGN.md
 * lists them).  The environment is read ONCE per process; casync_create copies the process defaults
 * into the handle.  h != NULL changes that handle only; h == NULL changes the process defaults, which
 * the casync_op_* single-operator calls and handles created later use.  No counterpart in the
 * reference (it has no tuning surface).                                                         */
int  casync_set_option(casync_handle h, const char* name, int value);
int  casync_get_option(casync_handle h, const char* name, int* value);

/* ---- engine life cycle ------------------------------------------------- */
/* Replaces Model(6,"hubert").to(device) (infer_api.py:41).                   */
int  casync_create(int device_id, casync_handle* out);
/* dtype = activation storage type inside the engine: 0 = fp32 (parity path, < 1e-3 vs
 * the reference), 1 = bf16 activations + bf16 matrix-core operands with fp32 accumulate
 * (BASELINE configs[2]; ~1e-2 vs the reference, reported separately).  The boundary
 * tensors stay fp32 either way.                                                  */
int  casync_create_ex(int device_id, int dtype, casync_handle* out);
/* Model(6, "wenet") as well: audio_mode = CASYNC_AUDIO_HUBERT | CASYNC_AUDIO_WENET.  The handle's
 * packed layout is casync_packed_*_m(audio_mode).                                                */
int  casync_create_mode(int device_id, int dtype, int audio_mode, casync_handle* out);
void casync_destroy(casync_handle h);

/* Replaces net.load_state_dict(...) (infer_api.py:42): the packed, BN-folded
 * buffer of casync_packed_total_m(mode) floats.  _host copies from host memory into
 * an engine-owned device buffer; _device adopts a caller-owned device buffer
 * (e.g. the tensor an RCCL broadcast just filled) without copying -- the
 * caller keeps it alive for the life of the handle.                          */
int  casync_load_weights_host(casync_handle h, const float* packed, int64_t n_floats);
int  casync_load_weights_device(casync_handle h, const float* packed_dev, int64_t n_floats);

/* Replaces Model.forward(x, audio_feat) (module/unet.py:314-345).
 *   x_dev     [B,6,160,160]  NCHW fp32   (reference crop ch0-2, masked crop ch3-5)
 *   audio_dev [B,32,32,32]   NCHW fp32   (HuBERT window; CASYNC_AUDIO_HUBERT handle)
 *             [B,256,16,32]  NCHW fp32   (WeNet window, CASYNC_AUDIO_WENET handle: the reference
 *                                         dataset's reshape, dataset/dataset.py:173-174)
 *   out_dev   [B,3,160,160]  NCHW fp32   in (0,1)
 * Enqueues on `stream`, no host synchronisation, no allocation.             */
int  casync_forward(casync_handle h, const float* x_dev, const float* audio_dev,
                    float* out_dev, int batch, void* workspace_dev,
                    int64_t workspace_bytes, casync_stream stream);

/* Same forward, but the HuBERT windows are gathered on the device: `features_dev` is the whole
 * [n_steps, 2, 1024] fp32 feature array of the clip (uploaded once), frame_idx_dev[b] the video
 * frame index of batch entry b; entry b sees features[idx-8 : idx+8], zero-padded past both
 * ends, reshaped to (32,32,32) -- exactly FrameSynthesizer._get_audio_features
 * (infer_api.py:99-145), without the B x 128 KB host windows and their H2D copy.
 * HuBERT handles only: a CASYNC_AUDIO_WENET handle returns CASYNC_ERR_ARG (the reference has no
 * inference-side WeNet window builder).                                                     */
int  casync_forward_windows(casync_handle h, const float* x_dev, const float* features_dev,
                            int n_steps, const int32_t* frame_idx_dev, float* out_dev, int batch,
                            void* workspace_dev, int64_t workspace_bytes, casync_stream stream);

/* Debug taps: copy a named NHWC intermediate of the LAST forward (same batch,
 * same workspace) into dst_dev; returns its per-frame float count or <0.
 * Names: x1 x2 x3 x4 x5 a tx kx fuse u1 u2 u3 u4 att0..att3 audio_conv1..5
 * (audio_conv1 / audio_conv2 of a wenet handle are 16x32 frames of 256 channels)  */
int64_t casync_tap(casync_handle h, const char* name, int batch, void* workspace_dev,
                   void* dst_dev, int64_t dst_elems, casync_stream stream);  /* dst: engine dtype */

/* Per-kernel timing of one forward (HIP events around every launch on
 * `stream`; synchronises).  Writes up to `cap` entries; returns the count.  */
typedef struct {
  char  name[48];     /* plan step, e.g. "up4.conv.double_conv.0.fused"      */
  char  kernel[64];   /* HIP kernel instance as rocprofv3 names it           */
  float ms;           /* event-pair time minus the calibrated cost of an empty pair (clamped at 0) */
  float ms_raw;       /* the event-pair time as measured                     */
  double flops;       /* algorithmic flops of this launch                   */
  double bytes;       /* algorithmic bytes (inputs read once + outputs)     */
} casync_kernel_time;
int  casync_profile_forward(casync_handle h, const float* x_dev, const float* audio_dev,
                            float* out_dev, int batch, void* workspace_dev,
                            int64_t workspace_bytes, casync_stream stream,
                            casync_kernel_time* out, int cap);

/* ---- single operators (used by the parity tests and micro-benchmarks) ---- */
/* Activation storage type of the casync_op_* calls made by this thread afterwards:
 * 0 = fp32 (default), 1 = bf16 (activation / weight pointers are then bf16; bias,
 * scales and all arithmetic stay fp32).                                        */
int casync_op_set_dtype(int dtype);
/* 1x1 conv / linear as GEMM on NHWC rows: C[M,N] = epi(A[M,K] * W[N,K]^T).
 * Replaces nn.Conv2d(k=1)/nn.Linear + folded BN + LeakyReLU (+ residual)
 * (module/unet.py:17-20,31-33,201-204,227-229,256-259).
 * epilogue: v = acc + bias[n]; v += pre_scale[n]*pre_res[m,n]; v = lrelu(v) if
 * act; v += post_res[m,n]; v = lrelu(v*aff_s[n]+aff_t[n]) if aff_s.         */
int casync_op_pw_gemm(const void* a, int lda, const void* w, const float* bias,
                      void* c, int ldc, int m, int n, int k, int act,
                      const void* pre_res, int ld_pre, const float* pre_scale,
                      const void* post_res, int ld_post,
                      const float* aff_s, const float* aff_t, casync_stream stream);
/* Diagnostic (tools/experiments/gemm_timeline.py): the casync_op_pw_gemm calls this thread makes next
 * write 8 timestamp words per workgroup into dev_words (NULL = off).  Never used by the engine.  */
int casync_debug_gemm_stamps(void* dev_words);
/* Same for the fused inverted-residual kernel (fp32): 5 words per workgroup (first 4096 workgroups) = shader
 * cycles of wave 0 in prologue / P1 / P2 / P3 / epilogue.  tools/experiments/ir_timeline.py.              */
int casync_debug_ir_stamps(void* dev_words);
/* nn.Conv2d(k=3, bias) + folded BN + LeakyReLU of the audio encoder (conv3: stride 2 pad 1, conv5: stride 2
 * pad 3; module/unet.py:161-168) as an implicit GEMM: in [B,H,W,cin] NHWC, w [cout][(ky,kx,cin)],
 * out [B,Ho,Wo,cout].  cin % (128 B / elem) == 0, cout % 64 == 0. */
int casync_op_conv3x3(const void* in, const void* w, const float* bias, void* out, int batch, int h, int w_,
                      int cin, int cout, int stride, int pad, int act, casync_stream stream);
/* The same with the strides of the two axes apart and a choice of activation: act 0 = none,
 * 1 = LeakyReLU(0.01), 2 = ReLU (AudioConvWenet conv3: stride (1,2) pad 1, conv5: stride 2 pad 3,
 * each + BN + ReLU; module/unet.py:119-133).  Ho = (h+2pad-3)/stride_h+1, Wo = (w+2pad-3)/stride_w+1. */
int casync_op_conv3x3_ex(const void* in, const void* w, const float* bias, void* out, int batch, int h, int w_,
                         int cin, int cout, int stride_h, int stride_w, int pad, int act, casync_stream stream);

/* What that convolution executes (host only, no device needed).  In fp32 its GEMM rows are position-major -- output positions
 * sorted by which of their nine taps lie inside the image, frames innermost -- and each 64-row tile walks only the taps
 * that some row of it has (option conv_skip, default 1; results are bit-identical with 0).  ktile_groups_full: (output
 * tile, tap) pairs with all nine taps; ktile_groups_run: the pairs walked at the current process options and dtype.
 * Audio conv5 (16x16, stride 2, pad 3) at batch 32: run / full = 0.649; bf16 launches keep frame-major rows and run == full.
 * Additive to ABI 13. */
int casync_conv3x3_plan(int batch, int h, int w_, int cin, int cout, int stride_h, int stride_w, int pad,
                        int64_t* ktile_groups_full, int64_t* ktile_groups_run);

/* Depthwise 3x3, pad 1, stride 1|2, + bias + LeakyReLU on NHWC.
 * Replaces nn.Conv2d(groups=C,k=3)+BN+LeakyReLU (module/unet.py:21-30).
 * w is tap-major [9][C].                                                    */
int casync_op_dw3x3(const void* in, const float* w, const float* bias, void* out,
                    int batch, int h, int wdt, int c, int stride, casync_stream stream);
/* The same depthwise 3x3 (pad 1, stride 1) + bias + LeakyReLU behind an Up block's first expand conv whose two
 * input-channel halves were computed apart (engine plan `skip_early`, fp32): the conv's input is
 * LeakyReLU(pre + up(g)), pre = W1b . skip + b at h x wdt, g = W1a . lo at (h/2) x (wdt/2), up = bilinear x2 with
 * align_corners=True.  Replaces nn.Upsample + torch.cat + the expand conv's LeakyReLU + Conv2d(groups=C,k=3)+BN+
 * LeakyReLU (module/unet.py:90-97, 17-30).  pre [B,h,wdt,c] NHWC, g [B,h/2,wdt/2,ldg] (first c columns used),
 * w tap-major [9][C], out [B,h,wdt,c].  h, wdt even, c % 4 == 0, frames the LDS-slab plan takes (10..40).     */
int casync_op_dw3x3_ups(const float* pre, const float* g, int ldg, const float* w, const float* bias, float* out,
                        int batch, int h, int wdt, int c, casync_stream stream);
/* Debug (tests/kernel_ledger.py): casync_debug_launch_log clears this thread's launch log and switches recording on
 * (on != 0) or off; while it is on, every kernel launch of the thread adds its kernel to the log once.  With it off a
 * launch does nothing more than before.  casync_debug_launched writes the logged kernels' short names
 * ("pw_gemm_kernel<__bf16, 128, 128, 2, 2>", the keys of tools/kernel_resources.py and of the profile rows), one per
 * line, NUL-terminated, into buf; returns their count, CASYNC_ERR_ARG when buf is too small.  Never used by the engine. */
int casync_debug_launch_log(int on);
int casync_debug_launched(char* buf, int cap);
/* Expand 1x1 conv + BN + LeakyReLU + depthwise 3x3 (pad 1, stride 1|2) + BN + LeakyReLU in one kernel, fp32, for the
 * inverted residuals below 32x32 (module/unet.py:17-30): the GEMM's output tile is whole frames, the depthwise conv
 * runs on it in LDS.  a [frames*hw*hw, lda], w1 [cexp][cin], b1 [cexp], wd [9][cexp] tap-major, bd [cexp],
 * d [frames*ho*ho, ldd].  hw in {10, 16, 20} (stride 2 only at 20), cin % 32 == 0, cexp % 64 == 0.           */
int casync_op_pw_dw(const void* a, int lda, const void* w1, const float* b1, const float* wd, const float* bd,
                    void* d, int ldd, int frames, int hw, int stride, int cin, int cexp, const void* ups, int ld_ups,
                    casync_stream stream);
/* The same on rectangular frames (AudioConvWenet's 16x32 blocks: module/unet.py:119-133), stride 1, one whole frame per
 * tile: a [frames*h*w, lda], d [frames*h*w, ldd], in the storage type of casync_op_set_dtype (w1 too; b1, wd, bd
 * fp32).  h x w = 16 x 32; fp32: cin % 16 == 0, cexp % 32 == 0; bf16: cin % 32 == 0, cexp % 64 == 0.               */
int casync_op_pw_dw_rect(const void* a, int lda, const void* w1, const float* b1, const float* wd, const float* bd,
                         void* d, int ldd, int frames, int h, int w, int cin, int cexp, casync_stream stream);
/* 1x1 conv + bias + [bilinear x2 upsample (align_corners=True) of a low-resolution tensor] + LeakyReLU:
 * c[m, :] = act(a[m, :] . w^T + bias + up2x(ups)[m, :]), rows m = pixels (b, y, x) of h x w frames, ups
 * [B*(h/2)*(w/2), ld_ups].  An Up block's expand conv (module/unet.py:90-96 + 17-20) with the upsample commuted behind
 * the conv: W1 . cat(up(lo), skip) = up(W1a . lo) + W1b . skip; `ups` = W1a . lo, a = skip, w = W1b.  casync_op_pw_dw
 * takes the same optional addend (ups may be NULL there).                                                   */
int casync_op_pw_gemm_ups(const void* a, int lda, const void* w, const float* bias, void* c, int ldc, int m, int n,
                          int k, int act, const void* ups, int ld_ups, int h, int w_, casync_stream stream);
/* Whole inverted-residual block in one kernel (expanded tensor stays in LDS); the
 * high-resolution stages use it.  Replaces InvertedResidual.forward
 * (module/unet.py:16-40) with BN folded: w1 [2cin][cin], wd [9][2cin], w2 [cout][2cin]
 * (w1/w2 in the op dtype, the rest fp32).
 * Returns CASYNC_ERR_ARG if (cin, cout, stride) has no instance.              */
int casync_op_ir_fused(const void* in, int ld_in, const void* w1, const float* b1,
                       const float* wd, const float* bd, const void* w2, const float* b2,
                       void* out, int ld_out, int batch, int h, int w, int cin, int cout,
                       int stride, int res, casync_stream stream);
/* Decoder variant: the block input is cat([bilinear_x2(lo)[0:c_lo], in[c_lo:cin]]) with the
 * upsample (align_corners=True) computed while loading -- Up.forward's interpolate + cat +
 * first InvertedResidual (module/unet.py:90-97) in one kernel.  lo: [B,h/2,w/2,ld_lo].     */
int casync_op_ir_fused_up(const void* lo, int ld_lo, int c_lo, const void* in, int ld_in,
                          const void* w1, const float* b1, const float* wd, const float* bd,
                          const void* w2, const float* b2, void* out, int ld_out, int batch,
                          int h, int w, int cin, int cout, casync_stream stream);
/* The same block with the upsample COMMUTED behind the expand conv (fp32 only): bilinear interpolation is linear
 * per channel and the 1x1 conv linear per pixel, so W1 . cat(up(lo), skip) = up(W1a . lo) + W1b . skip.
 * g = W1a . lo [B,h/2,w/2,ld_g >= 2*cin] (no bias), in = the skip half [B,h,w,ld_in >= cin/2], w1b [2*cin][cin/2];
 * cin is the block's logical input width (64 / 128).  Same result as casync_op_ir_fused_up up to fp32 rounding. */
int casync_op_ir_fused_upg(const float* g, int ld_g, const float* in, int ld_in, const float* w1b,
                           const float* b1, const float* wd, const float* bd, const float* w2,
                           const float* b2, float* out, int ld_out, int batch, int h, int w, int cin,
                           int cout, casync_stream stream);
/* Bilinear x2, align_corners=True (module/unet.py:86-87,91), NHWC, writing
 * into a wider row (ldc) so the concat with the skip is free.               */
int casync_op_upsample2x(const void* in, void* out, int ldc, int batch, int h, int wdt,
                         int c, casync_stream stream);
/* Cross attention core (module/unet.py:212-217): per frame
 * out = gamma * (softmax_j(Q K^T) V) + res, 100 face x 100 audio positions.  */
int casync_op_cross_attention(const void* q, int ldq, const void* k, int ldk,
                              const void* v, int ldv, const void* res, int ld_res,
                              const float* gamma_dev, void* out, int ld_out,
                              int batch, casync_stream stream);
/* FrameSynthesizer._get_audio_features (infer_api.py:99-145) alone, on the device: the gather casync_forward_windows
 * starts with, as an operator.  features_dev [n_steps,2,1024] fp32, frame_idx_dev [batch] int32 (any value: negative,
 * past the end).  nhwc = 0: windows_dev is the reference's own return value, [batch,32,32,32] fp32 (window row r of
 * features[idx-8 : idx+8] = channels 2r, 2r+1; all zeros where the reference falls back to its default window);
 * nhwc = 1: the engine's image [batch,1024,32] in the storage type of casync_op_set_dtype (what the first audio
 * kernel reads).  Bit-exact against the reference's own output (tests/golden/frame_windows.npz).                    */
int casync_op_audio_windows(const float* features_dev, int n_steps, const int32_t* frame_idx_dev, void* windows_dev,
                            int batch, int nhwc, casync_stream stream);
/* Tensor glue of FrameSynthesizer.process_batch around the model call, on the device:
 * crop_to_input: resized 168x168 BGR crops (uint8 HWC) -> the [B,6,160,160] fp32 model input
 *   (inner [4:164,4:164], masked copy with the black rectangle (5,5,150,145), HWC->CHW, /255,
 *   concat) -- infer_api.py:238-245;  pred_to_u8: pred*255 -> uint8 HWC [B,160,160,3]
 *   (truncation) -- infer_api.py:265-266.  Bit-exact; cv2.resize / blending stay on the host. */
int casync_op_crop_to_input(const uint8_t* crops168_dev, float* x_dev, int batch, casync_stream stream);
int casync_op_pred_to_u8(const float* pred_dev, uint8_t* out_dev, int batch, casync_stream stream);
/* The image arithmetic of FrameSynthesizer.process_batch on ragged per-frame regions (infer_api.py:234-235 and
 * 263-346).  The host slices every frame's crop box img[ymin:ymax, xmin:xmax] (infer_api.py:206-234) into ONE
 * byte buffer `regions` (h x w x 3 uint8 each, contiguous) and describes frame b in geom[b*12 .. b*12+11]
 * (int32): { region byte offset, h, w, width (xmax-xmin BEFORE the clamps: side of the synthesised square),
 * valid (1 when (width,width) == (h,w), else the frame is returned unchanged: infer_api.py:320-324), byte offset in
 * `synth`, byte offset in the two mask buffers, kind of the optional frame mask (-1 = none, 0 = float32 in [0,1],
 * 1 = uint8 standing for value / 255 -- what infer_api.py:68-70 computes on the host), its height, its width, and the
 * low / high 32 bits of its device address (masks live in allocations of their own, so a clip's masks can stay resident
 * on the device across batches instead of being uploaded with every batch) }.  pts: [B][33][2] int32 = the contour points already shifted / scaled / truncated
 * (infer_api.py:281-289).
 *   casync_frame_prepare: cv2.resize(region, (168,168)) -> crops168 [B,168,168,3] u8, and (x_dev != NULL) the
 *     [B,6,160,160] model input of casync_op_crop_to_input.
 *   casync_frame_paste_back: crop[4:164,4:164] = uint8(pred*255); cv2.resize to (width,width); cv2.fillPoly; area-
 *     scaled cv2.dilate; float64 blend with the original region (and the optional float mask, resized) -> out_regions
 *     (same layout as `regions`).  synth / mask_a / mask_b / area are scratch (sizes: sum of width*width*3, 2 x
 *     mask_bytes = sum of h*w, B int32).
 * OpenCV's arithmetic is restated from its published sources (resize.cpp, drawing.cpp, morph.cpp); cv2 is not
 * available in the build image, so parity with the real library is UNPINNED; parity with the CPU restatement
 * (oracle/frame_ops_oracle.py) is bit-exact.                                                                    */
int casync_frame_prepare(const uint8_t* regions_dev, const int32_t* geom_dev, int batch, uint8_t* crops168_dev,
                         float* x_dev, casync_stream stream);
int casync_frame_paste_back(const uint8_t* regions_dev, const int32_t* geom_dev, const int32_t* pts_dev,
                            const uint8_t* crops168_dev, const float* pred_dev, int batch,
                            int max_h, int max_w, int max_width, int64_t mask_bytes, uint8_t* synth_dev,
                            uint8_t* mask_a_dev, uint8_t* mask_b_dev, int32_t* area_dev, uint8_t* out_regions_dev,
                            casync_stream stream);
/* NCHW <-> NHWC helpers */
int casync_op_nchw_to_nhwc(const float* in, void* out, int batch, int c, int hw,
                           casync_stream stream);
/* inc block straight from the NCHW face crop (module/unet.py:58-67,290)      */
int casync_op_inc(const float* x_nchw, const float* packed_inc, void* out, int ldc,
                  int batch, casync_stream stream);
/* OutConv + outc_bn + sigmoid -> NCHW (module/unet.py:100-106,342-344)       */
int casync_op_outc(const void* in, int ld_in, const float* w, const float* b,
                   float* out_nchw, int batch, casync_stream stream);

/* ---- HuBERT feature extractor (ABI 8) ---------------------------------- */
/* transformers HubertModel (hubert-large: hidden 1024, 16 heads, FFN 4096, stable layer norm,
 * exact GELU, eps 1e-5) with any number of layers, fp32, batch 1 in the reference
 * (image_infer_v1/utils/hubert_extractor.py:19-58: model(batch).last_hidden_state).  Its own handle,
 * packed layout and workspace; forwards take the same cross-handle gate as casync_forward.        */
typedef struct casync_hubert* casync_hubert_handle;
/* Packed layout of a model with `layers` encoder layers (1..48; else 0 / NULL / -1).  Tensors start
 * on 256-B boundaries.  Conv weights are [cout][tap][cin]; pos.w is [group][tap][n][c] with the
 * weight norm folded; layer<l>.qkv.w stacks q, k, v projections ([3072][1024]) with q (rows and
 * bias) pre-scaled by 1/8; linear weights are torch's [out][in].                                  */
int         casync_hubert_packed_count(int layers);
const char* casync_hubert_packed_name(int layers, int i);
int64_t     casync_hubert_packed_offset(int layers, int i);
int64_t     casync_hubert_packed_size(int layers, int i);
int64_t     casync_hubert_packed_total(int layers);
/* tokens of a waveform of `samples` samples (0 below one receptive field, 400 samples)           */
int64_t     casync_hubert_tokens(int64_t samples);
/* workspace of a forward of `batch` waveforms of `samples` samples (0 when there is no token)    */
int64_t     casync_hubert_workspace_bytes(int batch, int64_t samples);
int  casync_hubert_create(int device_id, int layers, casync_hubert_handle* out);
void casync_hubert_destroy(casync_hubert_handle h);
/* casync_hubert_packed_total(layers) floats; _device adopts a caller-owned, 256-B aligned buffer */
int  casync_hubert_load_weights_host(casync_hubert_handle h, const float* packed, int64_t n_floats);
int  casync_hubert_load_weights_device(casync_hubert_handle h, const float* packed_dev, int64_t n_floats);
/* wave_dev [batch, samples] (already normalised), out_dev [batch, T, 1024] = last_hidden_state.
 * Enqueues on `stream`, no host synchronisation, no allocation.                                 */
int  casync_hubert_forward(casync_hubert_handle h, const float* wave_dev, int batch, int64_t samples, float* out_dev,
                           void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
/* Debug: the same forward, stopped at `stage` and that intermediate written to out_dev:
 * 1 = feature-encoder output [batch, T, 512], 2 = input to layer 0 (after the positional conv)
 * [batch, T, 1024], 3 = hidden states after n_layers layers, before the final LayerNorm.          */
int  casync_hubert_forward_tap(casync_hubert_handle h, const float* wave_dev, int batch, int64_t samples, int stage,
                               int n_layers, float* out_dev, void* workspace_dev, int64_t workspace_bytes,
                               casync_stream stream);
/* single operators (tests): conv0 + LayerNorm + GELU -> [batch*T0, 512]; LayerNorm over 512 / 1024
 * columns (+ GELU); out = x + GELU(posconv(x) + b) over [batch, T, 1024]; attention from the fused
 * [batch*T, 3072] q|k|v buffer -> [batch*T, 1024]; GEMM with overlapping A rows (lda may be < K),
 * act 0 or 3 (GELU), bias and post-residual [m, ld_post].                                        */
int  casync_op_hubert_conv0(const float* wave, int batch, int samples, const float* w, const float* b, const float* g,
                            const float* be, float* out, casync_stream stream);
int  casync_op_hubert_layernorm(const float* in, int ldi, float* out, int ldo, int rows, int cols, const float* g,
                                const float* b, float eps, int gelu, casync_stream stream);
int  casync_op_hubert_posconv(const float* x, const float* w_packed, const float* bias, float* out, int batch, int T,
                              casync_stream stream);
int  casync_op_hubert_attention(const float* qkv, float* out, int batch, int T, casync_stream stream);
int  casync_op_rows_gemm(const float* a, int lda, const float* w, const float* bias, float* c, int ldc, int m, int n,
                         int k, int act, const float* post_res, int ld_post, casync_stream stream);

/* ---- HuBERT, bf16 precision (ABI 10) ------------------------------------- */
/* dtype 0 = fp32 (casync_hubert_create), 1 = bf16: bf16 GEMM operands (from a bf16 image of the packed
 * weights made at load), bf16 activations between the kernels, fp32 sums and an fp32 residual stream;
 * conv0, feature projection and positional conv keep their fp32 arithmetic.  Waveform in and
 * last_hidden_state (and the debug taps) out stay fp32; forward / forward_tap serve both.          */
int  casync_hubert_create_ex(int device_id, int layers, int dtype, casync_hubert_handle* out);
/* workspace of a forward on THIS handle (the bf16 arena differs from the fp32 one)                */
int64_t casync_hubert_workspace_bytes_h(casync_hubert_handle h, int batch, int64_t samples);
/* single operators of the bf16 handle (tests); pointers declared void* are bf16.  conv0 -> bf16;
 * layernorm512: bf16 in, bf16 out with GELU (out_f32 0, gelu 1) or fp32 out (out_f32 1, gelu 0);
 * layernorm1024: v = h (+ delta when given; h = v when store_h), out = LayerNorm(v) as bf16 or fp32;
 * gelu: exact GELU in place over n bf16 (n % 8 == 0); widen: bf16 -> fp32; attention from the fused bf16
 * [batch*T, 3072] q|k|v buffer -> bf16 [batch*T, 1024]; rows_gemm_bf16: C = A W^T + bias, A rows may
 * overlap (lda < K), K % 64 == 0, N % 64 == 0.                                                     */
int  casync_op_hubert16_conv0(const float* wave, int batch, int samples, const float* w, const float* b, const float* g,
                              const float* be, void* out, casync_stream stream);
int  casync_op_hubert16_layernorm512(const void* in, int ldi, void* out, int ldo, int rows, const float* g, const float* b,
                                     float eps, int out_f32, int gelu, casync_stream stream);
int  casync_op_hubert16_layernorm1024(float* h, int ldh, const void* delta, int ldd, int store_h, void* out, int ldo,
                                      int rows, const float* g, const float* b, float eps, int out_f32,
                                      casync_stream stream);
int  casync_op_hubert16_gelu(void* x, int64_t n, casync_stream stream);
int  casync_op_hubert16_widen(const void* in, float* out, int64_t n, casync_stream stream);
int  casync_op_hubert16_attention(const void* qkv, void* out, int batch, int T, casync_stream stream);
int  casync_op_rows_gemm_bf16(const void* a, int lda, const void* w, const float* bias, void* c, int ldc, int m, int n,
                              int k, casync_stream stream);

/* ---- PFLD_GhostOne landmark network (ABI 11) ------------------------------ */
/* PFLD_GhostOne(width_factor=0.5, input_size=192, landmark_number=110), the network behind the reference's
 * LipDetector (utils/lip_detector/lip_detector.py:23-26,100-106; tools/pfld_mobileone.py:12-133), fp32, with every
 * MobileOneBlock folded on the host to one conv + bias (base_module.py:329-400).  Its own handle, packed layout and
 * workspace; forwards take the same cross-handle gate as casync_forward and casync_hubert_forward.               */
typedef struct casync_pfld* casync_pfld_handle;
/* Packed layout (floats; tensors start on 256-B boundaries): conv1.w [(ky,kx,ci)=27][32], conv2.w [9][32]; per
 * bottleneck <b> in conv3_1 .. conv6 and ghost module g1 / g2: <b>.g?.pw.w [ceil16(cin)][np] and .pw.b [np],
 * .dw.w [9][np], .dw.b [np] with np = ceil16(cout/2), zero-padded (the fp32 MFMA granule); <b>.dw.w [9][hid] of
 * the stride-2 bottlenecks; conv7.w [(ky,kx,ci)=72][16]; conv8.w [(y,x,c)=2304][64]; conv_out.w [256][220].   */
int         casync_pfld_packed_count(void);
const char* casync_pfld_packed_name(int i);
int64_t     casync_pfld_packed_offset(int i);
int64_t     casync_pfld_packed_size(int i);
int64_t     casync_pfld_packed_total(void);
int64_t     casync_pfld_workspace_bytes(int batch);           /* 0 for a batch outside 1..4096 */
/* Replaces PFLDInference().cuda() / load_state_dict / eval() (lip_detector.py:23-26). */
int  casync_pfld_create(int device_id, casync_pfld_handle* out);
void casync_pfld_destroy(casync_pfld_handle h);
int  casync_pfld_load_weights_host(casync_pfld_handle h, const float* packed, int64_t n_floats);
int  casync_pfld_load_weights_device(casync_pfld_handle h, const float* packed_dev, int64_t n_floats);
/* Replaces self.pfld_backbone(input_img) (lip_detector.py:105; pfld_mobileone.py:99-133): x_dev [B,3,192,192] NCHW
 * fp32 in [0,1] -> out_dev [B,220].  _u8 takes what cv2.resize hands over, [B,192,192,3] uint8 BGR HWC, and divides
 * by 255 itself (lip_detector.py:100-102): bit-equal to casync_pfld_forward on float(u8) / 255.  Enqueues on
 * `stream`, no host synchronisation, no allocation, no atomics: frame i of a batch has the bits of that frame alone. */
int  casync_pfld_forward(casync_pfld_handle h, const float* x_dev, int batch, float* out_dev, void* workspace_dev,
                         int64_t workspace_bytes, casync_stream stream);
int  casync_pfld_forward_u8(casync_pfld_handle h, const uint8_t* crops_dev, int batch, float* out_dev,
                            void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
/* Debug: the same forward stopped at `stage`, that intermediate written NHWC to out_dev: 0 conv1, 1 conv2 [B,96,96,32],
 * 2-4 conv3_1..3 [B,48,48,40], 5-7 conv4_1..3 [B,24,24,48], 8-11 conv5_1..4 [B,12,12,72], 12 conv6 [B,12,12,8],
 * 13 conv7 [B,12,12,16], 14 conv8 (x5) [B,64], 15 conv_out [B,220] (pfld_mobileone.py:100-130).  in_dev is float NCHW, or
 * uint8 HWC when input_u8.                                                                                            */
int  casync_pfld_forward_tap(casync_pfld_handle h, const void* in_dev, int input_u8, int batch, int stage, float* out_dev,
                             void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
/* single operators (tests), one per kernel family, all NHWC fp32:
 * stem: conv1 (dense 3x3 s2 p1, 3 -> 32, ReLU) + conv2 (depthwise 3x3, ReLU) of an h x w input (pfld_mobileone.py:
 *   100-101) -> out [B,ho,wo,32], ho = (h-1)/2+1; sums [B][tiles of 8x8][32] = per-tile channel sums of out;
 *   conv1_out (optional) [B,ho,wo,32].
 * ghost: GhostOneModule.forward (base_module.py:117-121) with folded blocks: out[.., 0:half] = act(pw(in)),
 *   out[.., half:2 half] = act(dw3x3(out[.., 0:half])), act = ReLU or none; in [B,h,w,ld_in], cin % 4 == 0,
 *   half <= 128; sums (optional, half <= 64) [B][tiles of 6x6][2 half].
 * dw_s2: the linear stride-2 depthwise 3x3, pad 1, of GhostOneBottleneck (base_module.py:136-145): in [B,h,w,c]
 *   -> out [B,(h-1)/2+1,(w-1)/2+1,ld_out], w [9][c].
 * head: AvgPool2d of the four stages from their per-tile sums (sums[j]: [B][tiles[j]][32|40|48|72], mean = sum /
 *   counts[j]), conv7, conv8, cat, conv_out (pfld_mobileone.py:102,108,114,121,125-131): x6 [B,12,12,8] -> out
 *   [B, ld_out >= 220].  sums / tiles / counts are HOST arrays of four.                                        */
int  casync_op_pfld_stem(const void* x, int input_u8, const float* w1, const float* b1, const float* w2, const float* b2,
                         float* out, float* sums, float* conv1_out, int batch, int h, int w, casync_stream stream);
int  casync_op_pfld_ghost(const float* in, int ld_in, const float* wp, const float* bp, const float* wd, const float* bd,
                          float* out, int ld_out, float* sums, int batch, int h, int w, int cin, int half, int act,
                          casync_stream stream);
int  casync_op_pfld_dw_s2(const float* in, const float* w, const float* bias, float* out, int ld_out, int batch, int h,
                          int w_, int c, casync_stream stream);
int  casync_op_pfld_head(const float* const* sums, const int* tiles, const int* counts, const float* x6, const float* w7,
                         const float* b7, const float* w8, const float* wo, const float* bo, float* out, int ld_out,
                         int batch, casync_stream stream);

/* ---- S3FD face detector (ABI 12) ------------------------------------------ */
/* S3FDNet, the network behind the reference's S3FDFaceDetector (utils/lip_detector/tools/detect_face.py:19-22;
 * tools/s3fd/nets.py:28-107), fp32, on equal-sized frames of any H x W the reference itself can run.  The handle replaces
 * S3FDNet.forward up to its call of Detect.forward (nets.py:109-171) plus PriorBox.forward and decode (box_utils.py:41-59,
 * 195-217); Detect.forward's threshold / NMS and everything behind it stay on the host (calipsync_amd/facedet.py).  Its own
 * handle, packed layout and workspace; forwards take the same cross-handle gate as the other three handles.            */
typedef struct casync_s3fd* casync_s3fd_handle;
/* Packed layout (floats; tensors start on 256-B boundaries): conv1_1.w [(ky,kx,ci)=27][64]; the dense 3x3 convs conv1_2 ..
 * conv5_3, conv6_2, conv7_2 (extras 1, 3) as <name>.w [cout][(ky,kx,cin)]; fc6.w [1024][(ky,kx,512)]; the 1x1 convs fc7,
 * conv6_1, conv7_1 (extras 0, 2) as [cout][cin]; every <name>.b [cout]; head<k>.w [8][(ky,kx,cin)] = loc[k] (rows 0-3) over
 * conf[k] (rows 4-7; two zero rows for k >= 1), with the L2Norm weight of sources 0-2 folded into the cin axis, head<k>.b [8]. */
int         casync_s3fd_packed_count(void);
const char* casync_s3fd_packed_name(int i);
int64_t     casync_s3fd_packed_offset(int i);
int64_t     casync_s3fd_packed_size(int i);
int64_t     casync_s3fd_packed_total(void);
/* Priors of an h x w frame (nets.py:155-166: the six maps' pixels, in order; 0 for a size the handle refuses) and the size
 * of source map k (0..5).                                                                                              */
int64_t     casync_s3fd_priors(int h, int w);
int         casync_s3fd_map_size(int h, int w, int k, int* map_h, int* map_w);
/* 0 for a shape the handle refuses: batch outside 1..65536, a frame whose pooled size reaches 0 (the reference raises
 * there too), a side above 8192, one frame whose conv1 output alone reaches 2 GiB.  No operand of one launch reaches 2 GiB:
 * a larger batch is walked in sub-batches inside the forward, and the workspace is that of one sub-batch.               */
int64_t     casync_s3fd_workspace_bytes(int batch, int h, int w);
/* Replaces S3FDNet(device).to(device) / load_state_dict / eval() (main.py:20-23). */
int  casync_s3fd_create(int device_id, casync_s3fd_handle* out);
void casync_s3fd_destroy(casync_s3fd_handle h);
int  casync_s3fd_load_weights_host(casync_s3fd_handle h, const float* packed, int64_t n_floats);
int  casync_s3fd_load_weights_device(casync_s3fd_handle h, const float* packed_dev, int64_t n_floats);
/* x_dev [B,3,H,W] NCHW fp32 as main.py:36-42 hands it over (channel c of the image as given minus (123, 117, 104)[c]) ->
 * det_dev [B,P,5] = (face probability, x1, y1, x2, y2) of EVERY prior, normalised coordinates, no threshold: softmax(conf)
 * [..., 1] (nets.py:170) and decode(loc, priors, [0.1, 0.2]) (box_utils.py:151).  _u8 takes the frames themselves,
 * [B,H,W,3] uint8, and subtracts the mean on the device: bit-equal to the float form.  batch 0 does nothing.  Enqueues
 * on `stream`, no host synchronisation, no allocation, no atomics: frame i of a batch has the bits of that frame alone. */
int  casync_s3fd_forward(casync_s3fd_handle h, const float* x_dev, int batch, int H, int W, float* det_dev,
                         void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
int  casync_s3fd_forward_u8(casync_s3fd_handle h, const uint8_t* frames_dev, int batch, int H, int W, float* det_dev,
                            void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
/* Debug: the same forward stopped at `stage`, that intermediate written NHWC to out_dev, each after its ReLU and before the
 * pool: 0 conv1_2 [B,H,W,64], 1 conv2_2, 2 conv3_3, 3 conv4_3, 4 conv5_3 (nets.py:115-131), 5 fc6, 6 fc7, 7 conv6_2,
 * 8 conv7_2 (nets.py:135-138); 9 loc [B,P,4], 10 the conf logits [B,P,2] after conf[0]'s max-out (nets.py:141-162),
 * 11 det [B,P,5].  in_dev is float NCHW, or uint8 HWC when input_u8.                                                */
int  casync_s3fd_forward_tap(casync_s3fd_handle h, const void* in_dev, int input_u8, int batch, int H, int W, int stage,
                             float* out_dev, void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
/* single operators (tests), one per kernel, all NHWC fp32:
 * stem: vgg[0-1], Conv2d(3, 64, 3, 1, 1) + ReLU (nets.py:35-36), x float NCHW or uint8 HWC (the mean subtracted here:
 *   main.py:38-41); w [(ky,kx,ci)=27][64] -> out [B,h,w,64].
 * maxpool: nn.MaxPool2d(2, 2[, ceil_mode=True]) (nets.py:39,45,53,61,69): in [B,h,w,c] -> out [B,h/2,w/2,c] or
 *   [B,(h+1)/2,(w+1)/2,c]; c % 4 == 0.
 * im2col_dil: the [B h w][(ky,kx,c)] matrix of a 3x3 conv with padding = dilation (vgg[30], fc6: nets.py:71), zero where a
 *   tap falls outside.
 * relu: in place over n floats (n % 4 == 0): nets.py:72,74,136 behind the GEMMs without a ReLU epilogue.
 * l2norm: L2Norm.forward without the weight (nets.py:21-23): out[r,:] = in[r,:] / (sqrt(sum in[r,:]^2) + 1e-10).
 * head: loc[k] and conf[k] of one source (nets.py:141-153): in [B,h,w,c], w [8][(ky,kx,c)], bias [8] -> loc [B,priors,4] and
 *   conf [B,priors,2] at priors first_prior + y w + x; maxout: conf = (max of rows 4-6, row 7) (nets.py:144-145), else rows
 *   4 and 5.
 * decode: PriorBox.forward (box_utils.py:195-212) + decode (box_utils.py:54-58) + softmax(conf)[..., 1] (nets.py:170) of an
 *   H x W frame's priors: loc [B,P,4], conf [B,P,2] -> det [B,P,5].                                                   */
int  casync_op_s3fd_stem(const void* x, int input_u8, const float* w, const float* bias, float* out, int batch, int h, int w_,
                         casync_stream stream);
int  casync_op_s3fd_maxpool(const float* in, float* out, int batch, int h, int w_, int c, int ceil_mode, casync_stream stream);
int  casync_op_s3fd_im2col_dil(const float* in, float* out, int batch, int h, int w_, int c, int dilation, casync_stream stream);
int  casync_op_s3fd_relu(float* x, int64_t n, casync_stream stream);
int  casync_op_s3fd_l2norm(const float* in, float* out, int64_t rows, int c, casync_stream stream);
int  casync_op_s3fd_head(const float* in, const float* w, const float* bias, float* loc, float* conf, int batch, int h, int w_,
                         int c, int priors, int first_prior, int maxout, casync_stream stream);
int  casync_op_s3fd_decode(const float* loc, const float* conf, float* det, int batch, int H, int W, casync_stream stream);

/* ---- S3FD, bf16 precision (ABI 13) ----------------------------------------- */
/* A second precision of the handle, chosen at creation: precision 0 is the fp32 handle above (casync_s3fd_create is the _ex
 * form with 0), 1 runs the network on bf16 activations; any other value is refused before any device call.  Precision 1:
 * conv1_1 in fp32 from the fp32 weights with a bf16 store; conv1_2 .. conv5_3, fc6 (on its dilated im2col matrix), fc7 and
 * the four extras with bf16 operands from a bf16 image of the packed buffer made on the device at load_weights_*, fp32
 * accumulation, bias and ReLU, bf16 out; pooling and im2col on bf16 (exact); L2Norm with an fp32 sum of squares and a true
 * division, bf16 out; the heads from bf16 activations with their fp32 weights, fp32 loc / conf logits; priors, decode and
 * score as in the fp32 handle.  The packed layout is the same.  forward, forward_u8, forward_tap and load_weights_* serve
 * both precisions: frames in and det [B,P,5] fp32 out as above, every tap of a bf16 stage widened to fp32.  Same forward
 * properties (no allocation, synchronisation or atomics; frame i of a batch has the bits of that frame alone; sub-batches
 * by the 2 GiB rule on the bf16 byte sizes).  _precision: 0 or 1 (-1 for a null handle).  _workspace_bytes_ex: the
 * workspace of one precision (0 for an unknown precision or a refused shape); casync_s3fd_workspace_bytes is precision 0. */
int     casync_s3fd_create_ex(int device_id, int precision, casync_s3fd_handle* out);
int     casync_s3fd_precision(casync_s3fd_handle h);
int64_t casync_s3fd_workspace_bytes_ex(int precision, int batch, int h, int w);
/* single operators (tests), one per kernel of the bf16 precision; in / out named void* are bf16 NHWC, c % 8 == 0, weights,
 * bias, loc and conf fp32 as in the casync_op_s3fd_* entries of the same name:
 * stem: fp32 arithmetic as casync_op_s3fd_stem (x float NCHW or uint8 HWC, the two forms bit-equal) -> out [B,h,w,64] bf16.
 * maxpool, im2col_dil, relu (n % 8 == 0): the bf16 forms of the fp32 entries, exact on bf16 values.
 * widen: bf16 -> fp32 over n values (n % 8 == 0), the taps of the bf16 stages.
 * l2norm: bf16 rows in, fp32 sum of squares, out[r,:] = bf16(in[r,:] / (sqrt(sum) + 1e-10)).
 * head: casync_op_s3fd_head from bf16 activations: fp32 weights and sums, fp32 loc / conf.                           */
int  casync_op_s3fd16_stem(const void* x, int input_u8, const float* w, const float* bias, void* out, int batch, int h, int w_,
                           casync_stream stream);
int  casync_op_s3fd16_maxpool(const void* in, void* out, int batch, int h, int w_, int c, int ceil_mode, casync_stream stream);
int  casync_op_s3fd16_im2col_dil(const void* in, void* out, int batch, int h, int w_, int c, int dilation, casync_stream stream);
int  casync_op_s3fd16_relu(void* x, int64_t n, casync_stream stream);
int  casync_op_s3fd16_widen(const void* in, float* out, int64_t n, casync_stream stream);
int  casync_op_s3fd16_l2norm(const void* in, void* out, int64_t rows, int c, casync_stream stream);
int  casync_op_s3fd16_head(const void* in, const float* w, const float* bias, float* loc, float* conf, int batch, int h, int w_,
                           int c, int priors, int first_prior, int maxout, casync_stream stream);

/* ---- face pipeline between S3FD and PFLD (additive to ABI 13) ---------------- */
/* The pixel and row work that joins the two face networks, so frames resident on the device reach int32 landmarks without
 * a pixel crossing the host.  Every entry checks its arguments before any device call (CASYNC_ERR_ARG and a message
 * otherwise), launches on `stream` and returns without synchronising; none allocates or uses atomics.
 *
 * resize_linear_u8: cv2.resize(INTER_LINEAR) on uint8 (S3FD.detect_faces, tools/s3fd/main.py:34), as restated from OpenCV
 *   4.x's resize.cpp: src [batch,sh,sw,3] -> dst [batch,dh,dw,3], both HWC.  scale_x / scale_y are source per destination,
 *   passed in as cv2 derives them: (double)1 / ((double)dst / src) for cv2.resize(src, dsize), 1 / f for cv2.resize(src, (0, 0),
 *   fx=f, fy=f) with dsize = (round-half-even(sw f), round-half-even(sh f)).  Equal sizes copy; (sw, sh) == (2 dw, 2 dh) is the
 *   INTER_AREA mean (a + b + c + d + 2) >> 2 that cv::resize switches to; otherwise fx = (float)((d + 0.5) scale - 0.5), floor,
 *   the two border clamps on columns, rows clipped with their weights kept, coefficients cvRound(c 2048),
 *   (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2.  batch 1..65535, sides 1..32767, scales in (0, 32768].
 * face_crops192: LipDetector's crop and cv2.resize(crop, (192, 192)) (lip_detector.py:46-80) without the crop: frames
 *   [n_frames,H,W,3] uint8 on the device; geom [n_crops][5] int32 = {frame, x1, y1, w, h} in HOST memory, read before the call
 *   returns.  Record i names a virtual h x w image whose pixel (y, x) is frames[frame, y1 + y, x1 + x] inside the frame and 0
 *   outside (x1, y1 may be negative, the window may miss the frame altogether); crops192[i] [192,192,3] is resize_linear_u8 of
 *   it, the identity (192) and 2x (384) cases included.  w < 1, h < 1, a side above 32767, |x1| or |y1| above 2^24, or frame
 *   outside [0, n_frames) is refused, with the record's index, before anything is launched.
 * s3fd_candidates: Detect.forward's selection (box_utils.py:150-156) on the device: det [batch,P,5] -> rows [batch,cap,5],
 *   rows[b, :min(counts[b], cap)] = the rows of det[b] whose score det[b,:,0] > thresh, in prior order; counts[b] is the number
 *   of such rows even beyond cap; rows past it are not written.  A NaN score fails the comparison.  1 <= cap <= P.
 * landmarks_finalize: lip_detector.py:106-114: y [n,220] (casync_pfld_forward's output) and mean_face [220] on the device,
 *   geom [n][5] in HOST memory as above (frame is ignored) -> out [n,110,2] int32 = (int32)((y + mean) * {w, h} + {x1, y1}),
 *   float32 with every operation rounded on its own, truncated toward zero.  Specified for finite results within int32.   */
int  casync_op_resize_linear_u8(const uint8_t* src, int batch, int sh, int sw, uint8_t* dst, int dh, int dw, double scale_x,
                                double scale_y, casync_stream stream);
int  casync_op_face_crops192(const uint8_t* frames, int n_frames, int H, int W, const int32_t* geom, int n_crops, uint8_t* crops192,
                             casync_stream stream);
int  casync_op_s3fd_candidates(const float* det, int batch, int P, float thresh, int cap, int32_t* counts, float* rows,
                               casync_stream stream);
int  casync_op_landmarks_finalize(const float* y, const float* mean_face, const int32_t* geom, int n, int32_t* out,
                                  casync_stream stream);

/* ---- S3FD's two NMS passes on the device (additive to ABI 13: a new symbol, nothing else changed) ---------------- */
/* What the reference runs on the host behind the network, on the rows casync_op_s3fd_candidates wrote: Detect.forward's nms
 * (box_utils.py:62-173), S3FD.detect_faces' walk, scaling and rows (main.py:45-58) and Girshick's nms_ (box_utils.py:7-38).
 * rows [batch,cap,5] float32 = (score, x1, y1, x2, y2) in prior order and counts [batch] int32, both on the device; per frame
 * b with n = counts[b]:
 *   n > cap:  status[b] = -1 and nothing else of the frame is written (the caller takes that frame's dense rows to the host);
 *   stage 1 (float32): area = (x2 - x1) * (y2 - y1); rows are visited by descending score, among equal scores the higher row
 *     index first (the stable ascending argsort popped from its end); the first surviving row i is kept and a later row j
 *     survives iff inter / ((area[j] - inter) + area[i]) <= 0.3f with inter = max(min(x2) - max(x1), 0) * max(min(y2) -
 *     max(y1), 0) (a NaN from 0 / 0 drops the row); at most 750 rows are kept.  detect_out [batch,750,5] float32 and detect_n
 *     [batch] int32 (both null, or both given) receive the kept rows (score, box) and their number: Detect.forward's output
 *     for the face class; rows behind detect_n[b] are not written.  (nms_top_k = 5000 cannot bite at cap <= 1024.)
 *   stage 2: the leading kept rows with score > conf_th (float32; behind the kept rows the reference's array holds zeros); if
 *     all 750 pass, status[b] = -2 (the reference's IndexError).  Else pt = box * (width, height, width, height) in float32,
 *     widened with the score to float64; areas = (x2 - x1) * (y2 - y1); visited by descending score, among equal scores the
 *     higher index first (argsort(kind="stable")[::-1]; the reference's default argsort leaves ties open); j survives iff
 *     inter / ((areas[i] + areas[j]) - inter) <= 0.1.  faces[b, :status[b]] float64 = (x1, y1, x2, y2, score) in keep order,
 *     status[b] = their number (0 for a frame without candidates); faces [batch,750,5], rows behind status[b] not written.
 * Every operation is the IEEE one of its type, so the result equals calipsync_amd.facedet's numpy restatement bit for bit
 * (finite boxes, no NaN score).  One 256-lane workgroup per frame, static LDS only, no atomics, no allocation, no
 * synchronisation.  batch 1..65535, cap 1..1024, width and height >= 1.                                                   */
int  casync_op_s3fd_nms(const float* rows, const int32_t* counts, int batch, int cap, int width, int height, float conf_th,
                        int32_t* status, double* faces, float* detect_out, int32_t* detect_n, casync_stream stream);

/* ---- a clip resident on the device (additive to ABI 13: two new symbols, nothing else changed) ---------------- */
/* The byte moves between the stored frames of a clip, frames [n_frames,H,W,3] uint8 on the device, and the packed `regions`
 * layout of casync_frame_prepare / casync_frame_paste_back, so that a batch of the frame loop needs no pixel from the host.
 * rec [batch][8] int32 in HOST memory, read before the call returns:
 *   { frame, y0, x0, h, w, valid, region byte offset, 0 }
 * frame indexes `frames`; (y0, x0, h, w) is the crop box img[y0:y0+h, x0:x0+w] (frame_loop.crop_box); region byte offset is
 * word 0 of the frame's geometry record, where its h x w x 3 bytes lie in `regions` (any alignment, gaps allowed).
 *   clip_gather:  regions[offset .. offset + h w 3) = frames[frame, y0:y0+h, x0:x0+w] for every record, whatever `valid` says.
 *   clip_compose: out [batch,H,W,3]; out[b] = frames[rec[b].frame], and where rec[b].valid the box is replaced by the h x w x 3
 *     bytes of out_regions at the record's offset.  out_regions may be NULL when no record is valid (the plain fetch of stored
 *     frames).  out must not overlap frames.  An output byte has one writer: a byte inside a valid box comes from out_regions only.
 * Refused with CASYNC_ERR_ARG before anything is launched or touched: a null pointer, H or W < 1, batch < 0 (batch 0 returns
 * 0), frame outside [0, n_frames), a box with h or w < 1 or not inside the frame, an offset < 0 or offset + h w 3 >
 * regions_bytes, a valid record with out_regions NULL.  clip_compose checks the box and the offset of valid records only.
 * One wave per row, 16-byte accesses where source and destination are 16-byte aligned together and narrower ones elsewhere
 * (no vector crosses a box edge); byte offsets are 64-bit.  No LDS, no atomics, no allocation, no synchronisation.            */
int  casync_op_clip_gather(const uint8_t* frames, int n_frames, int H, int W, const int32_t* rec, int batch, uint8_t* regions,
                           int64_t regions_bytes, casync_stream stream);
int  casync_op_clip_compose(const uint8_t* frames, int n_frames, int H, int W, const int32_t* rec, int batch,
                            const uint8_t* out_regions, int64_t regions_bytes, uint8_t* out, casync_stream stream);

/* ---- baseline JPEG of finished frames (additive to ABI 13: three new symbols, nothing else changed) ---------------- */
/* uint8 BGR frames [batch,H,W,3] on the device -> `batch` complete JFIF files in one contiguous device buffer.  The stream:
 * SOI, APP0 (JFIF 1.1, density 1 x 1), DQT 0 and 1 (8-bit, zigzag), SOF0 (4:4:4, tables 0, 1, 1), the four Annex K DHT, DRI (one
 * restart interval per row of 8 x 8 blocks), SOS: 629 bytes for any size and quality; then the scan, every block row padded
 * with 1-bits and closed by RSTn (n counts rows from 0, modulo 8), the last one by EOI.  The arithmetic is libjpeg's integer
 * baseline path (16-bit fixed-point colour, accurate integer DCT, round-half-away quantisation by 8 Q), so the bytes are those
 * of libjpeg-turbo for quality q, no subsampling and one restart interval per block row (calipsync_amd/jpeg.py holds the numpy
 * twin; tests/golden/jpeg_cases.npz the recorded bytes).
 *   jpeg_header:          HOST ONLY.  Writes the 629 header bytes to out (host memory, cap >= 629) and returns their number.
 *   jpeg_workspace_bytes: the scratch a batch needs: the row lengths, then one slot of slot_bytes per block row of every frame.
 *     slot_bytes 0 = the default, twice the raw bytes of a block row: 2 * 8 * 3 * 8 * ceil(W / 8).
 *   jpeg_encode:          scratch (4-byte aligned, scratch_bytes >= jpeg_workspace_bytes), out [out_cap], offsets int64 [batch + 1]
 *     and status int32 [batch] are device memory.  out[offsets[i] .. offsets[i+1]) is frame i's complete file when status[i] == 0.
 *     status 1: a block row outgrew its slot (uniform noise at quality 100 is about 1.4 x its raw size; the worst case of a block
 *     is far larger); status 2: the frame would pass out_cap.  A failed frame contributes zero bytes (offsets[i+1] == offsets[i]),
 *     the frames behind it follow on; no frame writes outside its slots or past out[offsets[batch]].  The two quantisation tables
 *     and the header are computed on the host and travel as kernel arguments.
 * Refused with a negative status before anything is launched: H or W outside 1..65535, quality outside 1..100, batch < 0,
 * slot_bytes < 0, out_cap < 0, a null or misaligned pointer, a scratch that is too small.  batch 0 returns 0 and touches nothing.
 * One wave per block row (colour, DCT and quantisation in registers, the code bits through a 32 KB LDS buffer), one workgroup
 * for the prefix over rows and frames, one workgroup per row for the compaction.  The output is a pure function of the input:
 * no global atomics, one writer per byte.  No allocation, no synchronisation.                                            */
int     casync_op_jpeg_header(int H, int W, int quality, uint8_t* out, int cap);
int64_t casync_op_jpeg_workspace_bytes(int batch, int H, int W, int64_t slot_bytes);
int     casync_op_jpeg_encode(const uint8_t* frames_bgr, int batch, int H, int W, int quality, int64_t slot_bytes, uint8_t* scratch,
                              int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int32_t* status,
                              casync_stream stream);

/* ---- 4:2:0 baseline JPEG of finished frames (additive to ABI 13: three new symbols, nothing else changed) ---------- */
/* The casync_op_jpeg_* trio with chroma at half resolution both ways, what libjpeg writes by default: the same argument lists,
 * status codes, buffer contracts and refusals, where a "row" is a row of 16 x 16 MCUs, ceil(H / 16) of them.  The stream: the
 * same 629 header bytes but for SOF0 (Y samples 2 x 2: component 1 is 0x22, components 2 and 3 stay 0x11) and DRI (ceil(W / 16),
 * one restart interval per MCU row); then the scan, every MCU row padded with 1-bits and closed by RSTn (n counts MCU rows from
 * 0, modulo 8), the last one by EOI.  One MCU is Y(2r,2c), Y(2r,2c+1), Y(2r+1,2c), Y(2r+1,2c+1), Cb(r,c), Cr(r,c); the three DC
 * predictors restart at 0 at the head of every MCU row.
 *   Y:      the last column and row repeated up to 8 ceil(W / 8) x 8 ceil(H / 8), then level-shifted.  A Y block of an MCU past
 *           those (block column >= ceil(W / 8) or block row >= ceil(H / 8)) is a dummy: its AC coefficients are zero and its DC
 *           is that of the Y block before it in the same MCU, so it codes as DC difference 0 and EOB.
 *   Cb, Cr: the full-resolution plane of the 16-bit fixed-point colour conversion is padded on the right to 16 ceil(W / 16)
 *           columns by repeating the last column, and at the bottom by one repeated row when H is odd; every output sample is
 *           (a + b + c + d + bias) >> 2 over its 2 x 2 inputs, bias 1 in even output columns and 2 in odd ones; the last
 *           downsampled row is then repeated up to 8 ceil(H / 16) rows; then the level shift.
 * DCT, quantisation (luma table for Y, chroma table for Cb and Cr), Huffman tables, padding and byte stuffing are those of the
 * 4:4:4 stream, so the bytes are those of libjpeg-turbo for quality q, 2 x 2 chroma subsampling and one restart interval per
 * MCU row (calipsync_amd/jpeg.py encode_jpeg_host(..., subsampling="4:2:0") is the numpy twin; tests/golden/jpeg420_cases.npz
 * holds the recorded bytes).
 *   jpeg420_header:          HOST ONLY.  Writes the 629 header bytes to out (host memory, cap >= 629) and returns their number.
 *   jpeg420_workspace_bytes: the row lengths, then one slot of slot_bytes per MCU row of every frame.  slot_bytes 0 = the default,
 *     twice the raw bytes of the samples an MCU row codes: 2 * 384 * ceil(W / 16).
 *   jpeg420_encode:          as jpeg_encode.  status 1: an MCU row outgrew its slot; status 2: the frame would pass out_cap.
 * One wave per MCU row (two lanes per MCU, 32 MCUs at a time: colour, downsampling, DCT and quantisation in registers, 24 KB of
 * coefficients and 8 KB of code bits in LDS; a dummy block runs no DCT), then the same plan and pack stages.  The output is a
 * pure function of the input: no global atomics, one writer per byte.  No allocation, no synchronisation.                   */
int     casync_op_jpeg420_header(int H, int W, int quality, uint8_t* out, int cap);
int64_t casync_op_jpeg420_workspace_bytes(int batch, int H, int W, int64_t slot_bytes);
int     casync_op_jpeg420_encode(const uint8_t* frames_bgr, int batch, int H, int W, int quality, int64_t slot_bytes, uint8_t* scratch,
                                 int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* offsets, int32_t* status,
                                 casync_stream stream);

/* ---- baseline JPEG files -> frames (additive to ABI 13: two new symbols, nothing else changed) -------------------- */
/* `batch` baseline JPEG files of one size -> uint8 BGR frames [batch,H,W,3] on the device, byte for byte what libjpeg's default
 * integer path decodes (islow inverse DCT: 13 constant bits, columns first, descaled by 11 and 18 bits, +128, clamp; 4:2:0 chroma
 * through h2v2 fancy upsampling of the real ceil(H/2) x ceil(W/2) plane with its edge rows and columns repeated; 16-bit
 * fixed-point YCbCr -> RGB).  calipsync_amd/jpeg.py decode_jpeg_host is the numpy twin, parse_jpeg reads the headers and
 * plan_decode builds what this call takes; tests/golden/jpeg_decode_cases.npz holds recorded files and pixels.  The subset: SOF0,
 * 8 bits, three components sampled 1x1 / 1x1 / 1x1 or 2x2 / 1x1 / 1x1, one interleaved scan, 8-bit quantisation tables, Huffman
 * tables 0 and 1 of any contents, any restart interval.
 *   data [data_bytes], DEVICE, 4-byte aligned: per file its scan (the entropy-coded bytes, RSTn markers included), its segment
 *     list and its table block, each on a 4-byte boundary.
 *       segment list: int32 start [nseg] | end [nseg] | first subsequence [nseg + 1]; start / end are byte offsets relative to the
 *         scan of each restart segment, markers excluded; segment j has max(1, ceil(8 (end - start) / chunk_bits)) subsequences.
 *       table block, 3720 bytes: quantisation uint16 [3][64] per component in natural order | uint8 DC table (0 / 1) of each
 *         component, 0 | uint8 AC table of each, 0 | Huffman tables DC 0, DC 1, AC 0, AC 1 of 832 bytes: uint16 lut [256] on the
 *         next 8 bits (length << 8 | symbol, 0: a longer code) | int32 maxcode [8] of lengths 9..16 (-1: none) | int32 valoff [8]
 *         (index of the length's first symbol - its first code) | uint8 symbols [256].
 *   rec [batch][16] int32 in HOST memory, read before the call returns:
 *     { scan byte offset in data, scan bytes, sampling (0: 4:4:4, 2: 4:2:0), restart interval in MCUs (0: none), segments,
 *       segment list byte offset, table block byte offset, subsequences, index of its first subsequence among the batch's,
 *       status decided on the host (0; otherwise the frame gets that status, no subsequences and no work), 0 ... }
 *   subsampling: 2 sizes the scratch for 4:2:0 files only (a 4:4:4 record without a status is then refused), 0 for either.  chunk_bits: a multiple of 32 in 32..2^30.  A frame has
 *     at most 2^17 subsequences: the plan runs at most as many rounds as a frame has subsequences and a round sweeps them all, so
 *     this bounds the time one workgroup can be kept busy by a file that never synchronises (a record above it is refused; the
 *     caller takes a longer chunk_bits or the host path, as calipsync_amd/jpeg.py plan_decode does).
 *   jpegdec_workspace_bytes: 64 bytes per subsequence, then per frame its int16 coefficients [blocks][64] and its sample planes.
 *   status [batch] int32, DEVICE: 0, or the code of the first restart segment that breaks a rule -- 1: an invalid Huffman code, a
 *     DC category above 11 or a run past coefficient 63 ahead of the segment's last block; 2: the segment's bytes end before its
 *     last block; 3: they hold more blocks than its MCUs.  A frame with a non-zero status has unspecified pixels inside its own
 *     slot of `out`; nothing outside its slot and its scratch is written.
 * Refused with CASYNC_ERR_ARG before anything is launched or touched: a null pointer, a misaligned buffer, H or W outside
 * 1..65535, a record whose offsets leave data, whose segment count is not the geometry's, which has more than 2^17 subsequences, or whose subsequences do not follow the
 * previous record's, a scratch smaller than jpegdec_workspace_bytes says.  The contents of data are never trusted: every value
 * read from a segment list or a table is clamped or masked, bits past a segment's end read as zero, a segment writes at most the
 * blocks its MCUs have, and every loop is bounded by the bits of its subsequence.
 * Four kernels per 64 frames: the entropy plan (one workgroup per frame: the entry state of every subsequence by a fixed-point
 * iteration from guessed states, which ends after at most as many rounds as the longest segment has subsequences with the serial
 * decoder's states; then block offsets, DC predictors and the status by a segmented prefix sum), the coefficient write (one lane
 * per subsequence), the inverse DCT (one lane per block) and upsampling + colour (one lane per four pixels).  The output is a pure
 * function of the input: no global atomics.  One hipMemsetAsync of the coefficients; no allocation, no synchronisation.        */
int64_t casync_op_jpegdec_workspace_bytes(int batch, int H, int W, int subsampling, int64_t total_subsequences);
int     casync_op_jpegdec_decode(const uint8_t* data, int64_t data_bytes, const int32_t* rec, int batch, int H, int W, int subsampling,
                                 int chunk_bits, uint8_t* scratch, int64_t scratch_bytes, uint8_t* out, int32_t* status,
                                 casync_stream stream);

/* ---- Motion-JPEG files -> frames (additive to ABI 13: two new symbols, nothing else changed) ----------------------- */
/* casync_op_jpegdec_decode's wider sibling (csrc/jpeg_dec_mjpeg.hip; what the two share is csrc/jpeg_dec_common.h): the same
 * data, segment lists, table blocks, records, status codes, refusals and four stages, with the sampling word of a record taking
 *   0: 4:4:4, an MCU of 8 x 8 pixels, slots Y Cb Cr;          1: 4:2:2 (2x1 / 1x1 / 1x1), 16 x 8, slots Y Y Cb Cr;
 *   2: 4:2:0, 16 x 16, slots Y Y Y Y Cb Cr;                    3: grayscale, one component, a scan of single 8 x 8 blocks,
 * and any other value refused.  One call decodes a batch whose records mix the four; the scratch is sized for the largest of them,
 * so there is no `subsampling` argument.  4:2:2 chroma goes through libjpeg's h2v1 fancy upsampling of the real ceil(W/2)
 * columns (out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2, the first and last column copied, no
 * vertical filter); a grayscale file's Y is written to B, G and R; its table block holds component 0's quantisation table and
 * table selectors, the rest zero.  A file that leaves out Huffman tables (the MJPG convention) is the host's business: its table
 * block carries the Annex K table of the class and id the scan names (calipsync_amd/jpeg.py parse_jpeg(subset="mjpeg")).
 * calipsync_amd/jpeg.py decode_jpeg_host(subset="mjpeg") is the numpy twin; tests/golden/mjpeg_decode_cases.npz holds recorded
 * files and Pillow's pixels.  4:4:4 and 4:2:0 records give the bytes casync_op_jpegdec_decode gives.                        */
int64_t casync_op_mjpegdec_workspace_bytes(int batch, int H, int W, int64_t total_subsequences);
int     casync_op_mjpegdec_decode(const uint8_t* data, int64_t data_bytes, const int32_t* rec, int batch, int H, int W, int chunk_bits,
                                  uint8_t* scratch, int64_t scratch_bytes, uint8_t* out, int32_t* status, casync_stream stream);

/* ---- SyncNet_color, the lip-sync judge (additive to ABI 13: new symbols, nothing else changed) --------------------- */
/* The reference's SyncNet_color (module/syncnet.py:155-246) in eval mode, fp32: a face encoder of 17 conv + BatchNorm (+ x)
 * + ReLU blocks on [batch,3,160,160] NCHW in [0,1] (BGR: the layout of the U-Net's output), an audio encoder of 14 such
 * blocks on [batch,32,32,32] (mode CASYNC_AUDIO_HUBERT) or [batch,256,16,32] (CASYNC_AUDIO_WENET), each ending in [batch,512,
 * 3,3]; then view(batch, -1) in NCHW order (index c * 9 + y * 3 + x), x / max(|x|_2, 1e-12) and LeakyReLU(0.01).  BatchNorm
 * is folded into the convs on the host (calipsync_amd/syncnet.py).  Packed tensors per block, `face.<i>` / `audio.<i>`:
 *   .w  [cout][(ky,kx,cin)] (face.0: [(ky,kx,cin) = 147][32]),  .b  [cout].
 * Activations are NHWC.  face.0 (7x7) has a kernel of its own, face.1 (5x5, stride 2) and the 27 3x3 blocks run on one implicit-GEMM
 * kernel that sums K in chunks of 32 (one fma chain over K = 4608 leaves several times the reference's own float32 error), the
 * two 1x1 blocks on the data-parallel ring GEMM followed by a ReLU pass (the pointwise GEMM has no ReLU epilogue and may split K
 * at small M): no stream-K, no K split, no atomics, no sum across frames, so frame i of a batch has the bits of that frame
 * forwarded alone.  A batch above 256 frames runs in passes of 256.
 *   sync_workspace_bytes: 0 for a mode other than the two or a batch outside 1..65536.
 *   sync_forward: audio_emb_dev and face_emb_dev [batch,4608] fp32, 16-byte aligned; workspace 256-byte aligned.  Enqueues on
 *     `stream`, does not synchronise.  batch 0 returns 0.
 *   sync_forward_tap: stage 0..16 = face.0..face.16, 17..30 = audio.0..audio.13: that block's output in the reference's NCHW
 *     order into out_dev; the other encoder's input may be NULL.
 * Single operators (the kernel ledger's entries), all fp32, 16-byte aligned, enqueue and return:
 *   sync_stem7:   x [batch,3,h,w] NCHW, w [147][32], bias [32] -> out [batch,h,w,32] = relu(conv7x7 pad 3 + bias).
 *   sync_conv5:   in [batch,h,w,32] NHWC, w [64][(ky,kx,c) = 800], bias [64] -> out [batch,ho,wo,64], 5x5, stride 2, pad 1, ReLU;
 *                 ho = (h - 3) / 2 + 1, h and w >= 3.
 *   sync_conv3:   in [batch,h,w,cin] NHWC, w [cout][(ky,kx,c) = 9 cin], bias [cout], res NULL or [batch,ho,wo,cout] -> out [batch,ho,
 *                 wo,cout] = relu(conv3x3 + bias + res); cin a multiple of 32, cout of 64, strides 1..8, pad 0..8.
 *   sync_relu:    ReLU in place, n a multiple of 4.
 *   sync_to_nchw: in [batch,hw,c] -> out [batch,c,hw].
 *   sync_embed:   in [batch,9,512] NHWC -> out [batch,4608] as above; the norm is summed in float64 in a fixed order.
 *   sync_curve:   face_emb, audio_emb [n,d] (d a multiple of 4) -> sim [2 max_shift + 1, n], sim[s + max_shift, i] =
 *                 dot(face_i, audio_(i+s)) / max(|face_i| |audio_(i+s)|, 1e-8), sums in float64, one wave per pair;
 *                 0 where i + s is outside [0, n).  n >= 1, 0 <= max_shift <= 4096.                                         */
typedef struct casync_sync* casync_sync_handle;
int         casync_sync_packed_count(int mode);
const char* casync_sync_packed_name(int mode, int i);
int64_t     casync_sync_packed_offset(int mode, int i);
int64_t     casync_sync_packed_size(int mode, int i);
int64_t     casync_sync_packed_total(int mode);
int64_t     casync_sync_workspace_bytes(int mode, int batch);
int  casync_sync_create(int device_id, int mode, casync_sync_handle* out);
void casync_sync_destroy(casync_sync_handle h);
int  casync_sync_load_weights_host(casync_sync_handle h, const float* packed, int64_t n_floats);
int  casync_sync_load_weights_device(casync_sync_handle h, const float* packed_dev, int64_t n_floats);
int  casync_sync_forward(casync_sync_handle h, const float* face_dev, const float* audio_dev, int batch, float* audio_emb_dev,
                         float* face_emb_dev, void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
int  casync_sync_forward_tap(casync_sync_handle h, const float* face_dev, const float* audio_dev, int batch, int stage,
                             float* out_dev, void* workspace_dev, int64_t workspace_bytes, casync_stream stream);
int  casync_op_sync_stem7(const float* x, const float* w, const float* bias, float* out, int batch, int h, int w_, casync_stream stream);
int  casync_op_sync_conv5(const float* in, const float* w, const float* bias, float* out, int batch, int h, int w_, casync_stream stream);
int  casync_op_sync_conv3(const float* in, const float* w, const float* bias, const float* res, float* out, int batch, int h, int w_,
                          int cin, int cout, int stride_h, int stride_w, int pad, casync_stream stream);
int  casync_op_sync_relu(float* x, int64_t n, casync_stream stream);
int  casync_op_sync_to_nchw(const float* in, float* out, int batch, int hw, int c, casync_stream stream);
int  casync_op_sync_embed(const float* in, float* out, int batch, casync_stream stream);
int  casync_op_sync_curve(const float* face_emb, const float* audio_emb, int n, int d, int max_shift, float* sim, casync_stream stream);

/* ---- SyncNet_color, bf16 precision (additive to ABI 13) ---------------------- */
/* A second precision of the handle above, chosen at creation: precision 0 is the fp32 handle (casync_sync_create is the _ex
 * form with 0), 1 runs the network on bf16 activations; any other value is refused before any device call.  The three entries
 * are spelled casync_syncnet_*: the set of casync_sync_* names is closed.  Precision 1:
 *   face.0 (7x7) in fp32 from the fp32 weights on the fp32 NCHW input, one rounding to bf16 on the NHWC store; the audio window
 *   rounded once to bf16 NHWC; every other block with bf16 operands (the weights from a bf16 image, round to nearest even, of
 *   the packed buffer, made on the device at load_weights_*), fp32 accumulation over K in one fixed order, + the fp32 bias, +
 *   the residual (bf16, widened) in fp32 before the ReLU, one rounding to bf16 on the store; the last block of each encoder
 *   (face.16, audio.13) stores its fp32 sum unrounded and the embedding is computed from it as in the fp32 handle (float64
 *   norm in a fixed order, LeakyReLU).  No K split, no atomics, no sum across frames: frame i of a batch has the bits of that
 *   frame forwarded alone, whatever tile it lies in.  A batch above 256 frames runs in passes of 256.
 * The packed layout is the same fp32 buffer.  casync_sync_load_weights_host / _device, casync_sync_forward, casync_sync_forward_tap
 * and casync_sync_destroy take a handle of either precision: fp32 inputs, fp32 embeddings [batch,4608], every tap of a bf16
 * stage widened to fp32 NCHW; the same forward gate.  _precision: 0 or 1 (-1 for a null handle).  _workspace_bytes_ex: the
 * workspace of one precision (0 for an unknown precision or mode or a batch outside 1..65536); precision 1 needs half of
 * precision 0.
 * Single operators (the kernel ledger's entries), one per kernel of the bf16 precision; pointers named void* are bf16, NHWC,
 * 16-byte aligned; weights of the convs bf16 [cout][(ky,kx,c)], bias fp32:
 *   sync16_stem7:   casync_op_sync_stem7's arithmetic (x, w, bias fp32) -> out [batch,h,w,32] bf16.
 *   sync16_conv5:   in [batch,h,w,32], w [64][800] -> out [batch,ho,wo,64] bf16 = relu(conv5x5 stride 2 pad 1 + bias).
 *   sync16_conv3:   in [batch,h,w,cin], w [cout][9 cin], res NULL or [batch,ho,wo,cout] bf16 -> out bf16 = relu(conv3x3 + bias + res);
 *                   cin a multiple of 32, cout of 64, strides 1..8, pad 0..8; tile = 64 or 16 output channels per workgroup (the
 *                   handle takes 16 where 64 would make fewer than 64 workgroups); both tiles return the same bits.
 *   sync16_conv1:   in [batch,h,w,cin], w [cout][cin] -> out [batch,h,w,cout] FP32 = relu(conv1x1 + bias), not rounded.
 *   sync16_to_nchw: in [batch,hw,c] bf16 -> out [batch,c,hw] fp32.                                                         */
int     casync_syncnet_create_ex(int device_id, int mode, int precision, casync_sync_handle* out);
int     casync_syncnet_precision(casync_sync_handle h);
int64_t casync_syncnet_workspace_bytes_ex(int mode, int precision, int batch);
int  casync_op_sync16_stem7(const float* x, const float* w, const float* bias, void* out, int batch, int h, int w_, casync_stream stream);
int  casync_op_sync16_conv5(const void* in, const void* w, const float* bias, void* out, int batch, int h, int w_, casync_stream stream);
int  casync_op_sync16_conv3(const void* in, const void* w, const float* bias, const void* res, void* out, int batch, int h, int w_,
                            int cin, int cout, int stride_h, int stride_w, int pad, int tile, casync_stream stream);
int  casync_op_sync16_conv1(const void* in, const void* w, const float* bias, float* out, int batch, int h, int w_, int cin, int cout,
                            casync_stream stream);
int  casync_op_sync16_to_nchw(const void* in, float* out, int batch, int hw, int c, casync_stream stream);

/* ---- the audio front end: WAV bytes -> the normalised 16 kHz waveform (additive to ABI 13: four new symbols) ------- */
/* What stands between a RIFF PCM file of any rate and casync_hubert_forward, on the device (calipsync_amd/audio.py frontend_host is
 * the numpy twin; tests/golden/audio_resample_cases.npz holds recorded cases):
 *   decode:    little-endian PCM of `width` bytes: u8 (v - 128) / 128, i16 v / 2^15, i24 v / 2^23, i32 v / 2^31, each an fp32 value.
 *   downmix:   mono 0 ("mean"): the `channels` samples of a frame summed in channel order in fp32, divided once by channels;
 *              mono 1 ("first"): channel 0.
 *   resample:  y[k] = sum_i x[i] taps[k down + half - i up], half = (n_taps - 1) / 2, zeros outside both arrays, summed over
 *              ascending i in one fp32 fma chain.  With the taps of audio.py resample_taps(rate) this is scipy.signal.resample_poly(x,
 *              up, down) at its defaults.  up == down copies: y = x, taps_dev may be NULL.
 *   normalise: out = (x - (float)mean) * (float)((var + 1e-7)^-1/2), mean and the population variance of the n samples summed in
 *              float64, per block over a fixed span and then over the blocks: no atomics, the bits repeat from call to call.
 *   audio_out_samples:        HOST ONLY.  ceil(n up / down) for up / down = 16000 / rate in lowest terms; -1 for n < 0 or rate < 1.
 *   audio_workspace_bytes:    what audio_normalize needs for n_out samples (-1 for n_out < 1).
 *   audio_resample:           pcm [frames * channels * width] bytes, taps_dev [n_taps] fp32 and out [n_out] fp32 are DEVICE memory;
 *     n_out must be ceil(frames up / down).  pcm needs no alignment (16-byte loads are used where a frame never straddles one).
 *   audio_normalize:          x [n] -> out [n] (out may be x); workspace 8-byte aligned, audio_workspace_bytes long.  When it
 *     has run, the workspace starts with float64 mean, float64 variance.
 * Refused with CASYNC_ERR_ARG before anything is launched: a null pointer, width outside 1..4, channels outside 1..16, mono
 * other than 0 / 1, up or down < 1, frames < 1, an even n_taps, an n_out other than the formula's, a ratio whose outputs reach
 * further than the kernel's input tile (down / up above about 15).  Enqueue on `stream`; no allocation, no synchronisation.   */
int64_t casync_audio_out_samples(int64_t n, int rate);
int64_t casync_op_audio_workspace_bytes(int64_t n_out);
int     casync_op_audio_resample(const uint8_t* pcm, int width, int channels, int64_t frames, int mono, int up, int down,
                                 const float* taps_dev, int64_t n_taps, float* out, int64_t n_out, casync_stream stream);
int     casync_op_audio_normalize(const float* x, int64_t n, void* workspace, float* out, casync_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* CASYNC_HIP_H */
