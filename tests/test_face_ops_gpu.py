"""-m gpu: the four operators of csrc/face_ops.hip, bit for bit against the oracle's resize_linear_u8 (and numpy for the row
operators), every output in a sentinel-padded buffer that must stay untouched past the end.  The cases and expected values
are in tests/face_cases.py."""
import numpy as np
import pytest

import face_cases as fc
from calipsync_amd import facedet, recipe

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", list(fc.RESIZE_CASES))
def test_resize_is_the_oracles(name, batch):
    got, want, fence = fc.run_resize(name, batch)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = int((got != want).sum())
    print(f"{name} x{batch}: {want.shape}, {bad} of {want.size} bytes differ")
    assert bad == 0 and fence


def test_the_quarter_scale_of_a_replicated_frame_is_the_frame():
    """what tests/test_face_pipeline_gpu.py feeds the detector: fx=0.25 of the recipe frames replicated 4x"""
    import torch
    from calipsync_amd import face_ops
    frames = recipe.make_s3fd_inputs(2)
    big = np.repeat(np.repeat(frames, 4, 1), 4, 2)
    got = face_ops.resize_frames_u8(torch.from_numpy(big).to("cuda:0"), fx=0.25)
    assert np.array_equal(got.cpu().numpy(), frames)


def test_half_scale_on_an_odd_side_is_refused():
    import torch
    from calipsync_amd import face_ops
    with pytest.raises(ValueError, match="not pinned"):
        face_ops.resize_frames_u8(torch.zeros((1, 9, 8, 3), dtype=torch.uint8, device="cuda:0"), fx=0.5)
    even = torch.from_numpy(fc.image(10, 8, "half")[None]).to("cuda:0")
    assert np.array_equal(face_ops.resize_frames_u8(even, fx=0.5)[0].cpu().numpy(), fc.expected_resize(fc.image(10, 8, "half"), (4, 5)))


# ---------------------------------------------------------------------------------------------- crops
@pytest.mark.parametrize("which", ["one", "kinds", "many"])
def test_crops_are_the_oracles_resize_of_the_virtual_crop(which):
    got, want, fence = fc.run_crops(which)
    assert got.shape == want.shape
    per_crop = (got != want).reshape(len(want), -1).sum(axis=1)
    print(f"{which}: {len(want)} crops, differing bytes per crop {per_crop.tolist()}")
    assert not per_crop.any() and fence
    if which == "kinds":
        table = fc.crop_table(which)
        assert len({int(t[0]) for t in table}) == 3                    # crops of different frames in one call
        assert not want[9].any() and want[0].all()                     # the one wholly outside is black, the one inside has no padding


def test_a_bad_record_raises_with_the_librarys_message():
    import torch
    from calipsync_amd import face_ops
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="crop 1 names frame 1 of 1"):
        face_ops.face_crops192(frames, [[0, 0, 0, 4, 4], [1, 0, 0, 4, 4]])
    with pytest.raises(RuntimeError, match="crop 0 is 0 x 4"):
        face_ops.face_crops192(frames, [[0, 0, 0, 0, 4]])


# ---------------------------------------------------------------------------------------------- candidates
@pytest.fixture(scope="module")
def recipe_det():
    """the recipe detector's dense det of three 77 x 93 frames, P = 596: computed once, never changed"""
    eng = facedet.S3FDEngine(recipe.make_s3fd_state_dict(), "cuda:0")
    det = eng.forward_u8(recipe.make_s3fd_inputs(3)).cpu().numpy()
    eng.close()
    assert det.shape == (3, 596, 5)
    det.setflags(write=False)
    return det


@pytest.mark.parametrize("thresh", [0.05, 0.5])
def test_candidates_are_numpys_mask_select_in_prior_order(recipe_det, thresh):
    for det in (recipe_det, recipe_det[1:2]):                          # batches of 3 and 1
        ok, counts = fc.candidates_match(det, thresh, 596)
        print(f"thresh {thresh}: counts {counts.tolist()}")
        assert ok
    assert thresh > 0.05 or counts.min() >= 2


def test_candidates_with_a_cap_below_the_count_an_empty_frame_and_a_nan(recipe_det):
    _, full = fc.candidates_match(recipe_det, 0.05, 596)
    cap = int(full.min()) // 2
    assert cap >= 1
    ok, counts = fc.candidates_match(recipe_det, 0.05, cap)
    assert ok and (counts > cap).all() and np.array_equal(counts, full)          # counted past the cap, written up to it
    det = recipe_det.copy()
    det[1, :, 0] = 0.04                                                # an all-below frame between two others
    first = int(np.flatnonzero(det[0, :, 0] > 0.05)[0])
    det[0, first, 0] = np.nan                                          # a NaN score fails the comparison
    det[2, 300, 0] = np.float32(0.05)                                  # equality is not above
    ok, counts = fc.candidates_match(det, 0.05, 596)
    assert ok and counts[1] == 0 and counts[0] == full[0] - 1


# ---------------------------------------------------------------------------------------------- finalize
@pytest.mark.parametrize("n", [1, 3, 70])
def test_finalize_is_landmarks_from_crops_arithmetic(n):
    got, want, fence = fc.run_finalize(n)
    assert got.shape == want.shape == (n, 110, 2) and got.dtype == np.int32
    assert np.array_equal(got, want) and fence
    assert (want < 0).any() and (want > 0).any()
