/*
 * casync_ploss.h -- the trainer's loss with its gradient (libcasync_hip.so, additive to ABI 13: new symbols only, nothing of
 * casync_hip.h changed; CASYNC_ABI_VERSION stays 13).  Plain C99.
 *
 * The reference's step (step2_train_unet.py:12-36,107-112) computes
 *   loss_perceptual = mean((F(preds) - F(labels).detach())^2)   over B 256 (H/4) (W/4) values,
 *   loss_pixel      = mean(|preds - labels|)                    over B 3 H W values,
 *   loss            = loss_pixel + 0.1 loss_perceptual,
 * F = torchvision's vgg19().features up to and including index 14: Conv(3,64) ReLU Conv(64,64) ReLU MaxPool(2,2) Conv(64,128) ReLU
 * Conv(128,128) ReLU MaxPool(2,2) Conv(128,256) ReLU Conv(256,256) ReLU Conv(256,256); 3x3, padding 1, bias; floor pools; no
 * ReLU behind the last conv; no input normalisation.  preds and labels are fp32 NCHW [B,3,H,W], H, W >= 4.
 * The handle computes the three values and d loss / d preds.  The VGG is frozen: the gradients of its weights (which the
 * reference accumulates and never reads) are NOT computed, and no gradient reaches labels.
 *
 * Activations are fp32 NHWC.  The six convs behind conv1_1 run on the ring implicit-GEMM kernel (data-parallel tiles), a conv of
 * more than 64 input channels as one launch per slice of 64 whose partial outputs are summed as a fixed tree (that kernel sums
 * K = 9 cin products in one fp32 chain: K stays 576); their backward-data passes run the same way on weights transformed once
 * at load.  The features of image i are
 * the same bits at any batch.  Every entry that takes a stream enqueues on `stream`, allocates nothing and synchronises
 * nothing (the convs run on frame-major rows: no position table is built).  Pointers are device pointers unless said otherwise.
 */
#ifndef CASYNC_PLOSS_H
#define CASYNC_PLOSS_H

#include "casync_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct casync_ploss* casync_ploss_handle;

/* The packed weight buffer (floats; every tensor starts 256-B aligned):
 *   conv1_1.w [(ky,kx,cin)=27][64], conv1_1.b [64], then for conv1_2, conv2_1, conv2_2, conv3_1, conv3_2, conv3_3:
 *   <name>.w [cout][ky][kx][cin], <name>.b [cout].                                                                          */
int         casync_ploss_packed_count(void);
const char* casync_ploss_packed_name(int i);
int64_t     casync_ploss_packed_offset(int i);
int64_t     casync_ploss_packed_size(int i);
int64_t     casync_ploss_packed_total(void);

int  casync_ploss_create(int device_id, casync_ploss_handle* out);
void casync_ploss_destroy(casync_ploss_handle h);
/* Both loads also build the six backward matrices ([cin][2-ky][2-kx][cout], casync_op_ploss_weight_transform) and the channel
 * slices of both directions' matrices (casync_op_ploss_split) in a buffer of the handle's own and wait for them: a load allocates and synchronises, a forward or backward never does.  A device buffer
 * stays the caller's and must outlive the handle's use of it.                                                             */
int  casync_ploss_load_weights_host(casync_ploss_handle h, const float* packed, int64_t n_floats);
int  casync_ploss_load_weights_device(casync_ploss_handle h, const float* packed_dev, int64_t n_floats);

/* Bytes of `saved` and of `scratch` for a batch; 0 for a shape the handle refuses.  Both grow with the batch.
 *
 * `saved` is an OUTPUT of forward and an INPUT of backward: the prediction's post-ReLU activations a1_1, a1_2 [B,H,W,64],
 * a2_1, a2_2 [B,H/2,W/2,128], a3_1, a3_2 [B,H/4,W/4,256] and d = F(pred) - F(label) [B,H/4,W/4,256], in that order, each on a
 * 256-B boundary.  forward writes every byte of them (padding between them is never read); backward only reads.  forward
 * with saved == NULL keeps nothing (the no-grad form) and runs in `scratch` alone.
 * `scratch` is scratch in the sense of the workspace contract: no result depends on what it held before the call, and
 * nothing in it needs to survive the call.  256-B aligned, like `saved`.                                                    */
int64_t casync_ploss_saved_bytes(int batch, int H, int W);
int64_t casync_ploss_scratch_bytes(int batch, int H, int W);

/* losses_dev[3] = { w_pix * pixel + w_perc * perceptual, pixel, perceptual } (fp32).  The two sums are taken in float64 in an
 * order that depends on the shape alone (per-workgroup partial sums in scratch, one finishing workgroup): the same call twice
 * gives the same bits.  With w_pix == 0 the pixel kernel is not launched and pixel is 0.
 * CASYNC_ERR_ARG before anything runs: a null handle or pointer, weights not loaded, batch < 1, H or W < 4, a batch whose
 * largest activation ([B,H,W,64] fp32) reaches 2 GiB.  CASYNC_ERR_STATE: saved or scratch too small.                       */
int casync_ploss_forward(casync_ploss_handle h, const float* pred, const float* label, int batch, int H, int W, float w_pix, float w_perc,
                         float* losses_dev, void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes, casync_stream stream);

/* grad_pred [B,3,H,W] = s * ( w_perc * (2 / N_feat) * dF^T(d) + w_pix * sign(pred - label) / N_pix ), s = *grad_out_dev (a device
 * scalar: no host synchronisation), sign(0) = 0, N_feat = B 256 (H/4) (W/4), N_pix = B 3 H W.  `saved` as the forward of the
 * same pred, label and shape left it; the chain carries the unscaled d, the two scale factors meet in the last kernel, and s is
 * the last factor (a power of two scales the bits exactly).  With w_pix == 0 pred and label are not read (they may be NULL).   */
int casync_ploss_backward(casync_ploss_handle h, const float* pred, const float* label, const float* grad_out_dev, float* grad_pred, int batch,
                          int H, int W, float w_pix, float w_perc, const void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes,
                          casync_stream stream);

/* One intermediate, NHWC.  Forward stages: 0 conv1_1, 1 conv1_2, 2 pool1, 3 conv2_1, 4 conv2_2, 5 pool2, 6 conv3_1, 7 conv3_2
 * (all behind their ReLU), 8 conv3_3 -- each [2B, ...]: the prediction's B images, then the label's -- and 9 d [B,H/4,W/4,256].
 * Backward stages, the gradient leaving each step (= entering the next): 0 conv3_3^T(d), 1 masked by a3_2, 2 conv3_2^T, 3 masked
 * by a3_1, 4 conv3_1^T [B,H/4,W/4,128], 5 pool2 + ReLU adjoint [B,H/2,W/2,128], 6 conv2_2^T, 7 masked by a2_1, 8 conv2_1^T
 * [B,H/2,W/2,64], 9 pool1 + ReLU adjoint [B,H,W,64], 10 conv1_2^T, 11 masked by a1_1, 12 grad_pred [B,3,H,W] (NCHW).
 * casync_ploss_tap_floats: the floats of `out` (0 for a refused shape or stage); out is 16-B aligned.                        */
int64_t casync_ploss_tap_floats(int backward, int batch, int H, int W, int stage);
int casync_ploss_forward_tap(casync_ploss_handle h, const float* pred, const float* label, int batch, int H, int W, int stage, float* out,
                             void* scratch, int64_t scratch_bytes, casync_stream stream);
int casync_ploss_backward_tap(casync_ploss_handle h, const float* pred, const float* label, const float* grad_out_dev, int batch, int H, int W,
                              float w_pix, float w_perc, const void* saved, int64_t saved_bytes, int stage, float* out, void* scratch,
                              int64_t scratch_bytes, casync_stream stream);

/* ---- the kernels alone.  NHWC tensors are 16-B aligned, C % 4 == 0; a tensor of 2 GiB or more is refused (CASYNC_ERR_ARG). ---- */
/* x [B,3,H,W] NCHW, w [(ky,kx,cin)=27][64], bias [64] -> out [B,H,W,64] = ReLU(conv + bias), one fmaf chain over (ky, kx, cin) */
int casync_op_ploss_stem(const float* x, const float* w, const float* bias, float* out, int batch, int H, int W, casync_stream stream);
/* in [B,H,W,C] -> out [B,H/2,W/2,C]: 2x2 / 2 max, an odd last row / column dropped; H, W >= 2 */
int casync_op_ploss_pool(const float* in, float* out, int batch, int H, int W, int C, casync_stream stream);
/* w [cout][ky][kx][cin] -> out [cin][2-ky][2-kx][cout]; twice (with cout and cin exchanged) is the identity */
int casync_op_ploss_weight_transform(const float* w, float* out, int cout, int cin, casync_stream stream);
/* in [rows][c] -> out [c / 64][rows][64]: the 64-channel slices of an activation or of a weight matrix; c % 64 == 0 */
int casync_op_ploss_split(const float* in, float* out, int64_t rows, int c, casync_stream stream);
/* partials [g][n] (g = 2 or 4), rows of c -> out [n] = ((p0 + p1) [+ (p2 + p3)]) + bias[column], then ReLU where relu != 0; bias may be
 * NULL; every sum rounded on its own */
int casync_op_ploss_combine(const float* partials, int g, const float* bias, float* out, int64_t n, int c, int relu, casync_stream stream);
/* g[i] = a[i] > 0 ? g[i] : 0, in place, n % 4 == 0 */
int casync_op_ploss_relu_bwd(float* g, const float* a, int64_t n, casync_stream stream);
/* g_pool [B,H/2,W/2,C], a [B,H,W,C] (the pool's post-ReLU input) -> g [B,H,W,C]: of each window the first maximum in row-major
 * order (torch's > rule) receives g_pool if that maximum is positive; everything else, a dropped row / column included, is 0 */
int casync_op_ploss_pool_bwd(const float* g_pool, const float* a, float* g, int batch, int H, int W, int C, casync_stream stream);
/* g1 [B,H,W,64], w as casync_op_ploss_stem's -> grad_pred [B,3,H,W] = *grad_out_dev * (perc_scale * conv^T(g1) + pix_scale *
 * sign(pred - label)), each product and sum rounded on its own; pred == label == NULL: no pixel term */
int casync_op_ploss_stem_bwd(const float* g1, const float* w, const float* pred, const float* label, const float* grad_out_dev, float* grad_pred,
                             int batch, int H, int W, float perc_scale, float pix_scale, casync_stream stream);
/* casync_ploss_partials(items): the float64 partial sums a reduction over `items` lane items writes (1024 at the most): items
 * = n / 4 for sqdiff, n for absdiff.  Host only. */
int casync_ploss_partials(int64_t items);
/* d[i] = fp[i] - fl[i], partials[k] = workgroup k's sum of d^2 (float64); n % 4 == 0 */
int casync_op_ploss_sqdiff(const float* fp, const float* fl, float* d, int64_t n, double* partials, casync_stream stream);
/* partials[k] = workgroup k's sum of |pred - label| (float64) */
int casync_op_ploss_absdiff(const float* pred, const float* label, int64_t n, double* partials, casync_stream stream);
/* perceptual = fp32(sum(partials_sq) / count_sq), pixel = fp32(sum(partials_abs) / count_abs) (0 with n_abs == 0),
 * losses_dev[3] = { w_pix * pixel + w_perc * perceptual, pixel, perceptual }; one workgroup, a fixed order */
int casync_op_ploss_finish(const double* partials_sq, int n_sq, int64_t count_sq, const double* partials_abs, int n_abs, int64_t count_abs,
                           float w_pix, float w_perc, float* losses_dev, casync_stream stream);

#ifdef __cplusplus
}
#endif

#endif /* CASYNC_PLOSS_H */
