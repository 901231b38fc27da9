"""Re-runs the reference's SyncNet_color on the recipe and compares it with tests/golden/syncnet_*.npz and with the restatement;
skipped where the reference tree is not mounted (it never is on the GPU machine)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import syncnet_ref
from calipsync_amd import recipe, syncnet
from conftest import GOLDEN

REF = os.environ.get("CASYNC_REFERENCE", "/root/reference")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "module", "syncnet.py")), reason="reference tree not mounted")


@pytest.fixture(scope="module")
def ref_class():
    """module/syncnet.py imports cv2 at its head; neither the constructor nor forward uses it: an attribute-less stand-in"""
    sys.dont_write_bytecode = True
    asked = []

    class NoCv2(types.ModuleType):
        def __getattr__(self, name):
            if not name.startswith("__"):
                asked.append(name)
            raise AttributeError(name)

    had = sys.modules.get("cv2")
    if had is None:
        sys.modules["cv2"] = NoCv2("cv2")
    sys.path.insert(0, REF)
    try:
        from module.syncnet import SyncNet_color
    finally:
        sys.path.pop(0)
    yield SyncNet_color
    if had is None:
        sys.modules.pop("cv2", None)
    assert not asked, asked


@pytest.mark.parametrize("mode,batch", [("hubert", 3), ("wenet", 2)])
def test_reference_reproduces_the_fixture_and_the_restatement(ref_class, mode, batch):
    fx = np.load(os.path.join(GOLDEN, f"syncnet_{mode}_b{batch}.npz"))
    sd = recipe.make_syncnet_state_dict(mode)
    net = ref_class(mode).eval()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    x, a = (torch.from_numpy(v) for v in recipe.make_syncnet_inputs(batch, mode))
    with torch.no_grad():
        a32, f32 = (t.numpy() for t in net(x, a))
        a64, f64 = (t.numpy() for t in net.double()(x.double(), a.double()))
    assert np.abs(a64 - fx["audio_emb64"]).max() <= 1e-12 and np.abs(f64 - fx["face_emb64"]).max() <= 1e-12
    assert np.abs(a32 - fx["audio_emb32"]).max() <= 4 * float(fx["ref_err.audio_emb"])   # (another thread count may sum in another order)
    assert np.abs(f32 - fx["face_emb32"]).max() <= 4 * float(fx["ref_err.face_emb"])
    ra, rf, _ = syncnet_ref.forward(syncnet.fold(sd, mode, dtype=np.float64), x.double(), a.double(), mode)
    assert np.abs(ra.numpy() - a64).max() <= 1e-12 and np.abs(rf.numpy() - f64).max() <= 1e-12
    assert list(net.state_dict()) == [k for k, _ in syncnet.manifest(mode)]
