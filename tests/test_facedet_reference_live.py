"""Re-runs the reference's S3FDNet on the recipe and compares it with tests/golden/s3fd_b2.npz, and holds tests/s3fd_ref.py to
it; skipped where the reference tree is not mounted (it never is on the GPU machine)."""
import os
import sys

import numpy as np
import pytest
import torch

import s3fd_ref
from calipsync_amd import facedet, recipe
from conftest import GOLDEN

REF = os.environ.get("CASYNC_REFERENCE", "/root/reference")
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "utils", "lip_detector", "tools", "s3fd")), reason="reference tree not mounted")


@pytest.fixture(scope="module")
def net():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REF, "utils", "lip_detector"))
    try:
        from tools.s3fd.nets import S3FDNet          # (nets.py and box_utils.py import torch and numpy only)
    finally:
        sys.path.pop(0)
    n = S3FDNet("cpu").eval()
    n.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_s3fd_state_dict().items()}, strict=True)
    return n


@pytest.fixture(scope="module")
def x():
    u8 = recipe.make_s3fd_inputs(2)
    return torch.from_numpy((u8.astype(np.float32) - facedet.IMG_MEAN).transpose(0, 3, 1, 2).copy())


def test_reference_reproduces_the_fixtures_detect_output(net, x):
    fx = np.load(os.path.join(GOLDEN, "s3fd_b2.npz"))
    with torch.no_grad():
        y = net(x).numpy()
    kept = fx["detect32"][:, 1, :, 0] > 0
    assert np.array_equal(y[:, 1, :, 0] > 0, kept)                                    # the same rows survive
    assert np.abs(y - fx["detect32"]).max() <= 4 * float(fx["ref_err.det"])         # (another thread count may sum in another order)


def test_the_restatement_equals_the_fixture_in_float64(x):
    fx = np.load(os.path.join(GOLDEN, "s3fd_b2.npz"))
    taps = s3fd_ref.network(recipe.make_s3fd_state_dict(), x, torch.float64)
    assert taps["maps"] == facedet.map_sizes(77, 93)
    assert np.abs(taps["loc"].numpy() - fx["loc64"]).max() <= 1e-11 and np.abs(taps["conf"].numpy() - fx["conf64"]).max() <= 1e-11
    assert np.abs(s3fd_ref.dense(taps, 77, 93).numpy() - fx["det64"]).max() <= 1e-12
