"""Re-runs the reference's PFLD_GhostOne on the recipe and compares it with tests/golden/pfld_b3.npz; skipped where the
reference tree is not mounted (it never is on the GPU machine)."""
import os
import sys

import numpy as np
import pytest
import torch

from calipsync_amd import landmarks, recipe
from conftest import GOLDEN

REF = os.environ.get("CASYNC_REFERENCE", "/root/reference")
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "utils", "lip_detector", "tools")), reason="reference tree not mounted")


@pytest.fixture(scope="module")
def net():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REF, "utils", "lip_detector"))
    try:
        from tools.pfld_mobileone import PFLD_GhostOne
    finally:
        sys.path.pop(0)
    n = PFLD_GhostOne().eval()
    n.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in recipe.make_pfld_state_dict().items()}, strict=True)
    return n


def test_reference_reproduces_the_fixture(net):
    fx = np.load(os.path.join(GOLDEN, "pfld_b3.npz"))
    x = torch.from_numpy((np.asarray(recipe.make_pfld_inputs(3), dtype=np.float32) / 255.0).transpose(0, 3, 1, 2).copy())
    with torch.no_grad():
        y32 = net(x).numpy()
        y64 = net.double()(x.double()).numpy()
        net.float()
    assert np.abs(y64 - fx["out64"]).max() <= 1e-12
    assert np.abs(y32 - fx["out32"]).max() <= 4 * float(fx["ref_err.out"])   # (another thread count may sum in another order)


def test_our_fold_equals_the_reference_reparameterize(net):
    sd = recipe.make_pfld_state_dict()
    ours = landmarks.fold(sd, dtype=np.float64)
    for p, *_ in landmarks.blocks():
        m = net.get_submodule(p)
        k, b = m._get_kernel_bias()
        assert np.abs(ours[f"{p}.w"] - k.detach().numpy()).max() <= 2e-6, p
        assert np.abs(ours[f"{p}.b"] - b.detach().numpy()).max() <= 2e-6, p
