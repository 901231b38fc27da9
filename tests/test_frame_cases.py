"""The batches of tests/frame_cases.py reach the branches of csrc/frame_ops.hip they are named for (no GPU): each claim is
checked from the case's inputs and the oracle's outputs alone, so a case that quietly stops testing its branch fails here
on any machine.  tests/kernel_ledger.py (frame_ops) runs the same batches on the device."""
from fractions import Fraction

import numpy as np
import pytest

import frame_cases as fc
from oracle import frame_ops_oracle as fo


@pytest.fixture(scope="module", params=fc.NAMES)
def batch(request):
    return fc.batch(request.param)


def test_every_stage_has_its_shape_and_dtype(batch):
    b = len(batch.regions)
    assert b == len(batch.labels) == len(batch.width) == len(batch.valid) == len(batch.masks) == len(set(batch.labels))
    assert batch.pts.shape == (b, 33, 2) and batch.pts.dtype == np.int32
    assert batch.pred.shape == (b, 3, 160, 160) and batch.pred.dtype == np.float32
    assert batch.pred.min() == 0.0 and batch.pred.max() == 1.0
    assert batch.crops168.shape == (b, 168, 168, 3) and batch.crops168.dtype == np.uint8
    assert batch.x.shape == (b, 6, 160, 160) and batch.x.dtype == np.float32
    assert len(batch.area) == len(batch.e) == b
    for i, r in enumerate(batch.regions):
        h, w = r.shape[:2]
        assert r.dtype == np.uint8 and r.shape == (h, w, 3) and h > 0 and w > 0
        assert batch.valid[i] == (batch.width[i] == h == w)
        assert batch.out[i].shape == r.shape and batch.out[i].dtype == np.uint8
        m = batch.masks[i]
        assert m is None or (m.ndim == 2 and m.dtype in (np.float32, np.uint8))
        if m is not None and m.dtype == np.float32:
            assert 0.0 <= m.min() and m.max() <= 1.0
        if not batch.valid[i]:
            assert batch.synth[i] is batch.fill[i] is batch.rows[i] is batch.final[i] is None and batch.area[i] == 0
            assert np.array_equal(batch.out[i], r)
            continue
        assert batch.synth[i].shape == (w, w, 3) and batch.synth[i].dtype == np.uint8
        for stage in (batch.fill[i], batch.rows[i], batch.final[i]):
            assert stage.shape == (h, w) and stage.dtype == np.uint8 and set(np.unique(stage)) <= {0, 255}
        assert batch.area[i] == int((batch.fill[i] > 0).sum()) and batch.e[i] == fo.expand_pixels(batch.area[i]) >= 1
        assert (batch.rows[i] >= batch.fill[i]).all() and (batch.final[i] >= batch.rows[i]).all()


def test_pred_sits_on_the_truncation_edges():
    pred = fc.batch("sizes").pred[3].reshape(-1)
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    for v in (np.float32(0.0), np.float32(1.0), *k, *np.nextafter(k[1:], np.float32(0.0))):
        assert (pred == v).any(), v
    u8 = np.array(np.nextafter(k[1:], np.float32(0.0)) * 255, dtype=np.uint8)
    assert (u8 == np.arange(255)).all()        # the float below k / 255 truncates to k - 1 for every k


def test_sizes_reach_the_three_synth_branches_and_the_ragged_guards():
    s = fc.batch("sizes")
    assert all(s.valid) and sorted(s.width) == [1, 2, 3, 83, 84, 85, 167, 168, 169, 336, 337, 701]
    assert 84 in s.width and 168 in s.width                                     # INTER_AREA, identity
    i = s.width.index(1)
    assert 701 in (s.width[i - 1], s.width[i + 1])                              # the smallest beside the largest
    assert sum(r.size for r in s.regions[:i + 1]) % 2 == 1                      # the next region starts at an odd byte
    i = s.e.index(max(s.e))
    assert s.e[i] == 53 and s.width[i] == 701                                   # the widest window of the dilation ...
    assert (s.fill[i] == 0).any() and (s.final[i] != s.rows[i]).any() and (s.rows[i] != s.fill[i]).any()   # ... has zeros to cover
    assert np.array_equal(s.synth[s.width.index(168)][4:164, 4:164].transpose(2, 0, 1),
                          np.array(s.pred[s.width.index(168)] * 255, dtype=np.uint8))   # identity: the patch itself


def test_masks_stand_in_the_stated_relation_to_the_region():
    m = fc.batch("masks")
    h = w = fc.MASK_W
    assert all(r.shape == (h, w, 3) for r in m.regions) and h % 2 == 0
    for kind, dtype in (("f32", np.float32), ("u8", np.uint8)):
        shape = {rel: m.masks[m.frame(f"{kind}_{rel}")].shape for rel, _ in fc.MASK_SHAPES}
        assert all(m.masks[m.frame(f"{kind}_{rel}")].dtype == dtype for rel, _ in fc.MASK_SHAPES)
        assert shape["same"] == (h, w)
        assert shape["double"] == (2 * h, 2 * w)
        assert shape["double_h_only"] == (2 * h, w)
        assert shape["up"][0] < h and shape["up"][1] < w and shape["up"] != (1, 1)
        assert shape["down"][0] > h and shape["down"][1] > w and shape["down"] != (2 * h, 2 * w)
        assert shape["one"] == (1, 1)
        assert shape["same_h"][0] == h and shape["same_h"][1] != w
        big = m.masks[m.frame(f"{kind}_same")]
        assert {0, 1, 255} <= set(np.unique(big if kind == "u8" else np.rint(big * 255).astype(int)))
    assert m.masks[m.frame("none")] is None
    assert all(a > 0 for a in m.area)
    differ = [int((m.out[i] != m.out[m.frame("none")]).sum()) for i in range(len(m.out) - 1)]
    assert all(d > 0 for d in differ)                                           # every mask shows in the blend


def _outside_y_then_x(w, h, p1, p2):
    """clipLine's first end: outside in y, not rejected, and outside in x where the edge meets that border row (by a whole
    pixel, so the truncation cannot decide it)"""
    (x1, y1), (x2, y2) = p1, p2
    right, bottom = w - 1, h - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if not (c1 & 12) or (c1 & c2):
        return False
    a = 0 if c1 < 8 else bottom
    x = x1 + Fraction((a - y1) * (x2 - x1), y2 - y1)
    return x <= -1 or x >= right + 1


def test_polygons_reach_what_they_claim():
    p = fc.batch("polygons")
    w = h = fc.POLY_W
    assert all(r.shape == (h, w, 3) for r in p.regions) and w % 2 == 1
    for label in ("far_right", "far_left"):
        i = p.frame(label)
        assert not p.fill[i].any() and p.area[i] == 0 and p.e[i] == 1 and np.array_equal(p.out[i], p.regions[i])
    assert (p.pts[p.frame("far_right"), :, 0] > 2 * w).all() and (p.pts[p.frame("far_left"), :, 0] < -w).all()
    i = p.frame("enclosing")
    q = p.pts[i]
    assert (p.fill[i] == 255).all()
    assert all(x < 0 or x >= w or y < 0 or y >= h for x, y in q)
    # corner cutting: vertices beyond all four sides and all four corners; both stages of clipLine for a first end
    i = p.frame("corner_cutting")
    q = [tuple(int(v) for v in pt) for pt in p.pts[i]]
    assert all(x < 0 or x >= w or y < 0 or y >= h for x, y in q if (x, y) not in ((60, 50), (50, 60)))
    codes = {(x < 0) + (x >= w) * 2 + (y < 0) * 4 + (y >= h) * 8 for x, y in q}
    assert {1, 2, 4, 8, 5, 6, 9, 10} <= codes
    edges = list(zip([q[-1]] + q[:-1], q))
    two_stage = [e for e in edges if _outside_y_then_x(w, h, *e)]
    assert two_stage and all(fo._clip_line(w, h, *e[0], *e[1])[0] for e in two_stage)      # ... and the x stage brings it in
    assert any(_outside_y_then_x(w, h, e[1], e[0]) for e in edges if not _outside_y_then_x(w, h, *e))   # a second end too
    outside_both = [e for e in edges if all(x < 0 or x >= w or y < 0 or y >= h for x, y in e)]
    assert any(fo._clip_line(w, h, *a, *b)[0] for a, b in outside_both)         # both ends outside, drawn all the same
    assert 0 < p.area[i] < w * h
    # no fill edge: lines only
    i = p.frame("collinear")
    assert len(set(p.pts[i, :, 1])) == 1 and len(set(p.pts[i, :, 0])) > 2
    ys, xs = np.nonzero(p.fill[i])
    assert set(ys) == {int(p.pts[i, 0, 1])} and (np.diff(xs) == 1).all()
    assert xs[0] == 0 and p.pts[i, :, 0].min() < 0 and xs[-1] == p.pts[i, :, 0].max() < w - 1
    i = p.frame("identical")
    assert len({tuple(pt) for pt in p.pts[i]}) == 1 and p.area[i] == 1
    i = p.frame("two_edges")
    q = p.pts[i]
    assert len({tuple(pt) for pt in q}) == 3
    assert sum(int(a[1] != b[1]) for a, b in zip(np.roll(q, 1, axis=0), q)) == 2
    assert p.area[i] > 500                                                      # two edges are enough to fill
    i = p.frame("star")
    assert p.fill[i][h // 2, w // 2] == 0 and p.fill[i][h // 2 - 30, w // 2] == 255      # the even-odd hole, an arm
    i = p.frame("zigzag")
    q = p.pts[i]
    active = [sum(int(min(a[1], b[1]) <= y < max(a[1], b[1])) for a, b in zip(np.roll(q, 1, axis=0), q)) for y in range(h)]
    assert max(active) >= 16 and max(active) <= 33
    i = p.frame("large")
    assert np.abs(p.pts[i]).max() >= 2 ** 14 and (p.pts[i] >= 2 ** 14).any() and (p.pts[i] <= -2 ** 14).any()
    assert 0 < p.area[i] < w * h
    cw, ccw = p.frame("angles_cw"), p.frame("angles_ccw")
    assert np.array_equal(p.pts[cw][:8], p.pts[ccw][:8][::-1])
    steps = {(int(b[0] - a[0]), int(b[1] - a[1])) for a, b in zip(np.roll(p.pts[cw], 1, axis=0), p.pts[cw])} - {(0, 0)}
    assert any(dx == 0 for dx, dy in steps) and any(abs(dx) == abs(dy) for dx, dy in steps)
    assert any(abs(dy) > abs(dx) > 0 for dx, dy in steps) and any(abs(dx) > abs(dy) > 0 for dx, dy in steps)
    assert any(dx < 0 for dx, dy in steps) and any(dx > 0 for dx, dy in steps)
    assert sum(label.startswith("random") for label in p.labels) >= 3


def _spans(q, y):
    """the even-odd spans (xa, xb) of row y in exact arithmetic: the crossings of the edges with y0 <= y < y1, in pairs"""
    xs = sorted(a[0] + Fraction((y - a[1]) * (b[0] - a[0]), b[1] - a[1])
                for a, b in zip([q[-1]] + q[:-1], q) if min(a[1], b[1]) <= y < max(a[1], b[1]))
    return list(zip(xs[0::2], xs[1::2]))


def test_polygons_reach_the_span_clamps_and_every_arm_of_the_line_iterator():
    """Counted over the whole batch from `pts` alone.  A span counts only where it is decided by two whole pixels: the 16.16
    slope of an edge is truncated, which moves a crossing by less than (y - y0) / 65536 < 1 pixel at these coordinates."""
    p = fc.batch("polygons")
    w = h = fc.POLY_W
    left = right = out_left = out_right = rejected = vertical_major = right_to_left = 0
    for pts in p.pts:
        q = [tuple(int(v) for v in pt) for pt in pts]
        if sum(a[1] != b[1] for a, b in zip([q[-1]] + q[:-1], q)) >= 2:      # with fewer edges nothing is filled
            for y in range(h):
                for xa, xb in _spans(q, y):
                    left += xa <= -2 and xb >= 2                             # `if (x1 < 0) x1 = 0` decides pixels
                    right += xb >= w + 1 and xa <= w - 3                     # `if (x2 >= w) x2 = w - 1`
                    out_left += xb <= -2                                     # `x2 >= 0` fails
                    out_right += xa >= w + 1                                 # `x1 < w` fails
        for a, b in zip([q[-1]] + q[:-1], q):
            if all(0 <= x < w and 0 <= y < h for x, y in (a, b)):
                x1, y1, x2, y2 = *a, *b
            else:
                ok, x1, y1, x2, y2 = fo._clip_line(w, h, *a, *b)
                rejected += not ok
                if not ok:
                    continue
            vertical_major += abs(y2 - y1) > abs(x2 - x1)
            right_to_left += x2 < x1
    assert left >= 100 and right >= 100 and out_left >= 50 and out_right >= 50, (left, right, out_left, out_right)
    assert rejected >= 50 and vertical_major >= 50 and right_to_left >= 50, (rejected, vertical_major, right_to_left)
    # the insertion sort has work to do: a row of the star whose crossings do not come in edge order
    q = [tuple(int(v) for v in pt) for pt in p.pts[p.frame("star")]]
    rows = [[a[0] + Fraction((y - a[1]) * (b[0] - a[0]), b[1] - a[1]) for a, b in zip([q[-1]] + q[:-1], q)
             if min(a[1], b[1]) <= y < max(a[1], b[1])] for y in range(h)]
    assert any(len(r) >= 4 and r != sorted(r) for r in rows)


def test_invalid_batches():
    a, m = fc.batch("invalid_all"), fc.batch("invalid_mixed")
    assert not any(a.valid) and all(r.shape[0] != r.shape[1] for r in a.regions)
    assert max(w * v for w, v in zip(a.width, a.valid)) == 0                    # max_width: the synth launch is skipped
    assert not m.valid[0] and not m.valid[-1] and any(m.valid) and 1 in [w for w, v in zip(m.width, m.valid) if v]
    assert any(not np.array_equal(o, r) for o, r in zip(m.out, m.regions))


def test_row_maximum_is_the_row_pass_of_the_dilation():
    rng = np.random.default_rng(3)
    mask = (rng.random((9, 14)) > 0.9).astype(np.uint8) * 255
    for e in (1, 4, 20):
        brute = np.array([[mask[y, max(0, x - e):x + e + 1].max() for x in range(14)] for y in range(9)])
        assert np.array_equal(fc.row_maximum(mask, e), brute)
        assert np.array_equal(fc.row_maximum(fc.row_maximum(mask, e).T, e).T, fo.dilate_square(mask, e))
