/*
 * casync_train.h -- the trainer's batches from a clip resident on the device (libcasync_hip.so, additive to ABI 13: one new
 * symbol, nothing of casync_hip.h changed; CASYNC_ABI_VERSION stays 13).  Plain C99.
 *
 * The reference builds a training sample in MyDataset.__getitem__ / process_img (dataset/dataset.py:73-178): two cv2.imread of
 * full frames, two landmark files, two crops resized to 168 x 168, a slice, a black rectangle, / 255.  With the clip's frames
 * stored on the device once (frames [n_frames,H,W,3] uint8, the store of casync_op_clip_gather) a batch is one call here.
 */
#ifndef CASYNC_TRAIN_H
#define CASYNC_TRAIN_H

#include "casync_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rec [batch][12] int32 in HOST memory, read before the call returns:
 *   { t, y0, x0, h, w, r, ry0, rx0, rh, rw, 0, 0 }
 * t and r index `frames`: the target and the reference frame of the sample (they may be the same frame).  (y0, x0, h, w) is the
 * target's region frame[y0:y0+h, x0:x0+w], (ry0, rx0, rh, rw) the reference's; each is the dataset's box img[ymin:ymax, xmin:xmax]
 * already cut to the frame as numpy slicing cuts it, so h != w where the square ran past the bottom or the right edge.
 *   crop168 = cv2.resize(region, (168, 168)): 8-bit INTER_LINEAR with its exact-2x INTER_AREA branch, the arithmetic of
 *     casync_frame_prepare applied to a region of any h x w;
 *   real = crop168[4:164, 4:164]; masked = real with x in [5, 154], y in [5, 149] black (cv2.rectangle (5, 5, 150, 145), filled);
 *   real_ex = the same crop of the reference region.
 *   img_concat [batch,6,160,160] = cat(real_ex, masked), img_real [batch,3,160,160] = real: fp32 CHW in the stored channel order,
 *     every value float(u8) / 255.0f, an IEEE fp32 division.
 * Refused with CASYNC_ERR_ARG before anything is launched or written: a null pointer, H or W < 1, batch < 0 (batch 0 returns 0),
 * a frame index outside [0, n_frames), a box with h or w < 1 or not inside the frame.
 * One kernel over the records (64 to a launch, as kernel arguments): the regions are read straight from `frames`, every output
 * element is written once by one lane, with 16-byte stores where img_concat and img_real are both 16-byte aligned and 4-byte
 * stores otherwise; frame byte offsets are 64-bit.  Enqueues on `stream`; no upload, no allocation, no workspace, no
 * synchronisation, no LDS, no atomics.                                                                                     */
int  casync_op_train_batch(const uint8_t* frames, int n_frames, int H, int W, const int32_t* rec, int batch, float* img_concat,
                           float* img_real, casync_stream stream);

#ifdef __cplusplus
}
#endif

#endif /* CASYNC_TRAIN_H */
