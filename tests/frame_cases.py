"""Named batches that reach every branch of the frame kernels (csrc/frame_ops.hip), with the expected result of every
stage from the CPU restatement (oracle/frame_ops_oracle.py, oracle/frame_loop_oracle.py).  Nothing here touches the GPU
side: tests/test_frame_cases.py checks on any machine that each case reaches the branch it is named for,
tests/kernel_ledger.py (frame_ops) runs the batches through casync_frame_prepare / casync_frame_paste_back and holds
every stage to these expectations bit for bit.

A batch is what the C ABI takes, frame by frame: the crop region (h x w x 3 uint8), `width` (the side of the synthesised
square), `valid` (width == h == w), the 33 contour points, the model's prediction and the optional frame mask.  No model
runs: `pred` is part of the case and carries values on the truncation edges of uint8(pred * 255).

  sizes          every synth branch (width 168 identity, 84 INTER_AREA, general), widths 1..701 side by side (ragged
                 launch guards, odd byte offsets), a dilation radius of 53 (width 701) over a fill that leaves the corners to cover
  polygons       contours a landmark file can hold and an arc cannot: points far outside, both stages of clipLine, no fill
                 edge at all, even-odd holes, 32 crossings on a row, 16.16 fixed point at |x| = 30000, every line octant
  masks          the frame mask's three resampling branches, float32 and uint8
  invalid_all    no valid frame: the synth launch is skipped
  invalid_mixed  invalid frames first, last and between valid ones
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from oracle import frame_loop_oracle
from oracle import frame_ops_oracle as fo

NPTS = 33
NAMES = ("sizes", "polygons", "masks", "invalid_all", "invalid_mixed")
SIZES_WIDTHS = (84, 1, 701, 2, 337, 3, 168, 85, 336, 83, 169, 167)      # the smallest beside the largest
POLY_W = 101
MASK_W = 48
# (mask h, mask w) against a MASK_W x MASK_W region, by the branch of the blend's resample
MASK_SHAPES = (("same", (48, 48)), ("double", (96, 96)), ("double_h_only", (96, 48)), ("up", (20, 27)), ("down", (131, 77)),
               ("one", (1, 1)), ("same_h", (48, 31)))


class Batch(NamedTuple):
    name: str
    labels: Tuple[str, ...]                   # one per frame
    regions: List[np.ndarray]                 # h x w x 3 uint8
    width: Tuple[int, ...]
    valid: Tuple[bool, ...]
    pts: np.ndarray                           # [B,33,2] int32
    pred: np.ndarray                          # [B,3,160,160] float32 in [0,1]
    masks: List[Optional[np.ndarray]]         # float32 in [0,1], uint8 (standing for value / 255), or None
    # expected, per stage (lists hold None for an invalid frame)
    crops168: np.ndarray                      # [B,168,168,3] uint8
    x: np.ndarray                             # [B,6,160,160] float32
    synth: List[Optional[np.ndarray]]         # width x width x 3 uint8
    fill: List[Optional[np.ndarray]]          # h x w uint8 (fillPoly)
    area: Tuple[int, ...]                     # 0 for an invalid frame
    e: Tuple[int, ...]
    rows: List[Optional[np.ndarray]]          # the fill after the row pass of the dilation
    final: List[Optional[np.ndarray]]         # the dilated mask
    out: List[np.ndarray]                     # the blended region (the region itself for an invalid frame)

    def frame(self, label):
        return self.labels.index(label)


# ------------------------------------------------------------------ inputs
def _pad33(vertices) -> np.ndarray:
    """a contour of 33 points from fewer vertices: the last one repeated (zero-length edges)"""
    v = [tuple(p) for p in vertices]
    assert 1 <= len(v) <= NPTS
    return np.array(v + [v[-1]] * (NPTS - len(v)), dtype=np.int32)


def _ellipse(w: int, radius: float) -> np.ndarray:
    t = np.arange(NPTS) * (2 * np.pi / NPTS)
    return np.stack([w / 2 + radius * w * np.cos(t), w / 2 + 0.9 * radius * w * np.sin(t)], 1).astype(np.int32)


def _pred(rng, b: int) -> np.ndarray:
    """random predictions; the head of every frame holds 0, 1, every k / 255 and the float just below it"""
    pred = rng.random((b, 3, 160, 160), dtype=np.float32)
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    edge = np.concatenate([[np.float32(0.0), np.float32(1.0)], k, np.nextafter(k[1:], np.float32(0.0))]).astype(np.float32)
    flat = pred.reshape(b, -1)
    for i in range(b):
        flat[i, :edge.size] = np.roll(edge, 7 * i)
        flat[i, 25600 + 160 * 80:25600 + 160 * 80 + edge.size] = edge[::-1]     # (and away from the crop's corner)
    return pred


def _regions(rng, shapes):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def polygon_frames(rng):
    """[(label, [33,2] int32)] of the `polygons` batch, for a POLY_W x POLY_W region"""
    w = POLY_W
    c = w // 2
    t = np.arange(NPTS) * (2 * np.pi / NPTS)
    arc = np.stack([40 * np.cos(t), 70 * np.sin(t)], 1)
    out = [("far_right", (arc + (350, c)).astype(np.int32)),
           ("far_left", (arc + (-350, c)).astype(np.int32)),
           ("enclosing", _pad33([(-50, -50), (150, -60), (160, 150), (-40, 155)]))]
    # beyond every corner and every side; edges that need the y stage of clipLine and then the x stage (first end:
    # (-30,-10)->(60,50), (135,120)->(50,60); second end: (60,50)->(131,-25), (50,60)->(-22,128)), edges that cut a
    # corner with both ends outside, an edge straight across, and one that misses the region past its corner codes
    out.append(("corner_cutting", _pad33([(-30, -10), (60, 50), (131, -25), (140, 50), (90, 112), (135, 120), (50, 60), (-22, 128),
                                          (-40, 50), (30, -15), (70, -40), (-20, 30), (130, 70), (110, 108), (-30, 10), (10, -30)])))
    xs = rng.integers(-15, 71, NPTS)
    xs[5], xs[20] = -15, 70                                   # the drawn segment: clipped on the left, ends inside on the right
    out.append(("collinear", np.stack([xs, np.full(NPTS, 40)], 1).astype(np.int32)))
    out.append(("identical", _pad33([(37, 61)])))
    out.append(("two_edges", np.array([(20, 20)] * 31 + [(80, 70), (30, 70)], dtype=np.int32)))
    star = [(c + 46 * np.sin(4 * np.pi * k / 5), c - 46 * np.cos(4 * np.pi * k / 5)) for k in range(5)]       # {5/2}
    out.append(("star", _pad33(np.array(star).astype(np.int32))))
    out.append(("zigzag", np.array([(3 + 3 * i, 10 if i % 2 == 0 else 90) for i in range(32)] + [(3, 95)], dtype=np.int32)))
    out.append(("large", _pad33([(-30000, -30011), (30100, 30090), (29000, -31000), (40, 70), (-29500, 30500), (60, -30000)])))
    angles = [(20, 10), (20, 60), (50, 90), (60, 30), (95, 22), (70, 15), (45, 40), (40, 5)]   # vertical, 45 deg, steep, shallow, ...
    out.append(("angles_cw", _pad33(angles)))
    out.append(("angles_ccw", _pad33(angles[::-1])))
    for k in range(3):
        out.append((f"random{k}", rng.integers(-20, w + 20, (NPTS, 2)).astype(np.int32)))
    return out


def _mask(rng, kind: str, shape) -> np.ndarray:
    """a frame mask holding the values 0, 1 and 255 (uint8) / 0, 1/255 and 1 (float32)"""
    m = rng.integers(0, 256, shape, dtype=np.uint8)
    flat = m.reshape(-1)
    special = np.array([255, 0, 1], dtype=np.uint8)[:max(1, min(3, flat.size))]
    flat[:special.size] = special
    if flat.size >= 6:
        flat[-3:] = special[::-1]
    if kind == "u8":
        return m
    return (m.astype(np.float32) / np.float32(255.0)).astype(np.float32)


# ------------------------------------------------------------------ expectations
def row_maximum(mask: np.ndarray, e: int) -> np.ndarray:
    """maximum over [x - e, x + e] clipped to the row (the row pass of the separable dilation)"""
    padded = np.pad(mask, ((0, 0), (e, e)))                  # zeros never raise a maximum of uint8
    return np.lib.stride_tricks.sliding_window_view(padded, 2 * e + 1, axis=1).max(axis=2)


def float_mask(mask: Optional[np.ndarray]) -> Optional[np.ndarray]:
    """the float32 mask the reference holds for a uint8 image (infer_api.py:68-70)"""
    if mask is None or mask.dtype != np.uint8:
        return mask
    return mask.astype(np.float32) / 255.0


def _expect(name, labels, regions, width, valid, pts, pred, masks) -> Batch:
    b = len(regions)
    crops = np.stack([fo.resize_linear_u8(r, (168, 168)) for r in regions])
    x = frame_loop_oracle.crops_to_model_input(crops)
    patch = frame_loop_oracle.predictions_to_uint8(pred)
    synth, fill, area, es, rows, final, out = [], [], [], [], [], [], []
    for i in range(b):
        if not valid[i]:
            for lst in (synth, fill, rows, final):
                lst.append(None)
            area.append(0)
            es.append(fo.expand_pixels(0))
            out.append(regions[i].copy())
            continue
        crop = crops[i].copy()
        crop[4:164, 4:164] = patch[i]
        synth.append(fo.resize_linear_u8(crop, (width[i], width[i])))
        fill.append(fo.fill_poly(regions[i].shape[:2], pts[i]))
        area.append(int(np.sum(fill[i] > 0)))
        es.append(fo.expand_pixels(area[i]))
        rows.append(row_maximum(fill[i], es[i]))
        final.append(fo.dilate_square(fill[i], es[i]))
        blended = regions[i].copy()
        blended[...] = fo.blend_region(regions[i], synth[i], final[i], float_mask(masks[i]))    # float64 -> uint8: truncation
        out.append(blended)
    return Batch(name, tuple(labels), regions, tuple(int(v) for v in width), tuple(bool(v) for v in valid), pts, pred, masks,
                 crops, x, synth, fill, tuple(area), tuple(es), rows, final, out)


def _sizes() -> Batch:
    rng = np.random.default_rng(7101)
    ws = SIZES_WIDTHS
    pts = np.stack([_ellipse(w, 0.55) for w in ws])
    return _expect("sizes", [f"w{w}" for w in ws], _regions(rng, [(w, w) for w in ws]), ws, [True] * len(ws), pts, _pred(rng, len(ws)),
                   [None] * len(ws))


def _polygons() -> Batch:
    rng = np.random.default_rng(7102)
    frames = polygon_frames(rng)
    b = len(frames)
    return _expect("polygons", [f[0] for f in frames], _regions(rng, [(POLY_W, POLY_W)] * b), [POLY_W] * b, [True] * b,
                   np.stack([f[1] for f in frames]), _pred(rng, b), [None] * b)


def _masks() -> Batch:
    rng = np.random.default_rng(7103)
    labels, masks = [], []
    for kind in ("f32", "u8"):
        for rel, shape in MASK_SHAPES:
            labels.append(f"{kind}_{rel}")
            masks.append(_mask(rng, kind, shape))
    labels.append("none")
    masks.append(None)
    b = len(labels)
    pts = np.stack([_ellipse(MASK_W, 0.3)] * b)
    return _expect("masks", labels, _regions(rng, [(MASK_W, MASK_W)] * b), [MASK_W] * b, [True] * b, pts, _pred(rng, b), masks)


def _invalid(mixed: bool) -> Batch:
    rng = np.random.default_rng(7105 if mixed else 7104)
    # (h, w, width): boxes clamped at one border, at the other, and at both
    frames = [("invalid0", 30, 41, 41, None), ("invalid1", 50, 37, 50, "u8"), ("invalid2", 40, 44, 45, "f32")]
    if mixed:
        frames = [frames[0], ("valid0", 57, 57, 57, None), frames[1], ("valid1", 64, 64, 64, "u8"), ("valid2", 1, 1, 1, None), frames[2]]
    shapes = [(h, w) for _, h, w, _, _ in frames]
    pts = np.stack([_ellipse(min(h, w), 0.4) for h, w in shapes])
    masks = [None if kind is None else _mask(rng, kind, (24, 30)) for *_, kind in frames]
    return _expect("invalid_mixed" if mixed else "invalid_all", [f[0] for f in frames], _regions(rng, shapes), [f[3] for f in frames],
                   [f[1] == f[2] == f[3] for f in frames], pts, _pred(rng, len(frames)), masks)


@functools.lru_cache(maxsize=None)
def batch(name: str) -> Batch:
    """the named batch with its expectations (built once per process; treat it as read-only)"""
    if name == "sizes":
        return _sizes()
    if name == "polygons":
        return _polygons()
    if name == "masks":
        return _masks()
    if name in ("invalid_all", "invalid_mixed"):
        return _invalid(name == "invalid_mixed")
    raise KeyError(name)
