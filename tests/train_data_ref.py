"""A numpy restatement of what the reference's ``MyDataset.__getitem__`` / ``process_img`` compute for one training sample
(dataset/dataset.py:73-146), composed from ``oracle.frame_ops_oracle.resize_linear_u8`` (the cv2.resize restatement the frame
kernels are held to).  It is written from the reference's text independently of calipsync_amd/train_data.py: numpy slicing does
the cutting, a slice assignment draws the rectangle.

  frames:   t = min(idx, n_img - 1); the reference item ex is shown as frame min(ex, n_img - 1)                  :137, :144
  region:   lms int32; xmin = lms[1][0], ymin = lms[52][1], xmax = lms[31][0], width = xmax - xmin, ymax = ymin + width;
            img[ymin:ymax, xmin:xmax]                                                                          :82-90
  crops:    cv2.resize(region, (168, 168), cv2.INTER_AREA): the third positional argument of cv2.resize is dst, so this is
            the default INTER_LINEAR (as at infer_api.py:235); [4:164, 4:164]; cv2.rectangle(.., (5, 5, 150, 145), 0, -1)
            blackens x in [5, 154], y in [5, 149]                                                              :91-98
  tensors:  HWC -> CHW, float32, / 255.0; img_concat = cat(real_ex, masked), img_real = real                  :123-134

cv2 is absent here, so the reading of the two cv2 calls is as unpinned against the real library as the frame loop's.
Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

from oracle.frame_ops_oracle import resize_linear_u8


def train_features(t: int, seed: int = 5) -> np.ndarray:
    """The [t, 2, 1024] fp32 features behind tests/golden/train_windows.npz: 2 hashed bits per value, (v - 2) / 2 in [-1, 0.5],
    exact arithmetic only.  Few levels so that six windows stored in full compress to a small file; 4096 random bits a step
    still tell any two rows, channels or columns apart."""
    from calipsync_amd import recipe
    bits = recipe._bits(seed, 0x747261, t * 2048, lane=t)
    v = (bits >> np.uint64(62)).astype(np.int64) - 2
    return (v.astype(np.float32) / np.float32(2)).reshape(t, 2, 1024)


def frames_of(idx: int, ex: int, n_img: int):
    """(target frame, reference frame) of item idx with reference item ex"""
    return min(idx, n_img - 1), min(ex, n_img - 1)


def region(img: np.ndarray, lms) -> np.ndarray:
    lms = np.array(np.asarray(lms, dtype=np.float32), dtype=np.int32)
    xmin, ymin, xmax = lms[1][0], lms[52][1], lms[31][0]
    width = xmax - xmin
    ymax = ymin + width
    return img[ymin:ymax, xmin:xmax]


def real_of(crop: np.ndarray) -> np.ndarray:
    """region or box cut -> the inner 160 x 160 x 3 of its 168 x 168 resize"""
    return resize_linear_u8(crop, (168, 168))[4:164, 4:164].copy()


def tensors(real: np.ndarray, real_ex: np.ndarray):
    """(img_concat [6,160,160], img_real [3,160,160]) float32 of the two inner crops"""
    masked = real.copy()
    masked[5:150, 5:155] = 0                                   # cv2.rectangle (x, y, w, h) = (5, 5, 150, 145), filled
    chw = lambda a: a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return np.concatenate([chw(real_ex), chw(masked)], axis=0), chw(real)


def sample(frames, landmarks, idx: int, ex: int):
    """One item from a clip's frames [n,H,W,3] and per-frame landmarks"""
    t, r = frames_of(idx, ex, len(frames))
    return tensors(real_of(region(frames[t], landmarks[t])), real_of(region(frames[r], landmarks[r])))


def sample_boxes(frames, t: int, box, r: int, rbox):
    """One kernel record {t, y0, x0, h, w, r, ry0, rx0, rh, rw}: the boxes are already inside the frame"""
    (y0, x0, h, w), (ry0, rx0, rh, rw) = box, rbox
    return tensors(real_of(frames[t][y0:y0 + h, x0:x0 + w]), real_of(frames[r][ry0:ry0 + rh, rx0:rx0 + rw]))


def batch(frames, landmarks, items, refs):
    pairs = [sample(frames, landmarks, int(i), int(e)) for i, e in zip(items, refs)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
