"""Cross-checks against what the reference itself computed, recorded by ``tests/golden/make_reference_checks.py``
(``tests/golden/reference_checks.npz``; the script runs the reference's own code, the suite only reads the data).
They guard the pin itself: the committed golden output still is what the reference computes on the inputs the
recipe regenerates, and the oracle tracks the reference on inputs and batch sizes the fixture does not contain."""
import hashlib
import os
import random

import numpy as np
import pytest
import torch

from calipsync_amd import recipe
from conftest import sample_indices
from oracle import unet_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "reference_checks.npz"))


def _sha(a: np.ndarray) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def _inputs_sha(x: np.ndarray, a: np.ndarray) -> bytes:
    return _sha(np.concatenate([x.reshape(-1), a.reshape(-1)]))


def test_committed_golden_output_is_reproducible(ref, golden, recipe_sd):
    from calipsync_amd import arch
    h = hashlib.sha256()
    for k, _s, _d, _r in arch.manifest():
        h.update(np.ascontiguousarray(recipe_sd[k]).tobytes())
    x, a = recipe.make_inputs(2)
    # the reference's re-run was fed what the recipe regenerates today, and so was the committed fixture
    assert h.digest() == ref["repro.weights_sha256"].tobytes() == golden["weights_sha256"].tobytes()
    assert _inputs_sha(x, a) == ref["repro.inputs_sha256"].tobytes()
    # the reference's re-run reproduced the committed output bit for bit
    assert _sha(golden["out.full"]) == ref["repro.out_sha256"].tobytes()


@pytest.mark.parametrize("batch,seed", [(1, 11), (3, 12)])
def test_oracle_tracks_the_reference_off_fixture(ref, recipe_sd, batch, seed):
    x, a = recipe.make_inputs(batch, seed=seed)
    assert _inputs_sha(x, a) == ref[f"off.b{batch}s{seed}.inputs_sha256"].tobytes()
    got = unet_oracle.forward(unet_oracle.to_torch(recipe_sd), torch.from_numpy(x), torch.from_numpy(a)).numpy()
    name = f"off.b{batch}s{seed}.out"
    assert tuple(ref[f"{name}.shape"]) == got.shape == (batch, 3, 160, 160)
    flat = got.reshape(-1)
    assert np.abs(flat[sample_indices(flat.size)] - ref[f"{name}.samples"]).max() <= 1e-5
    # the whole tensor, through its statistics (make_golden.py's convention for tensors stored as samples): the bounds
    # |d| <= 1e-5 per pixel implies on them (outputs lie in (0, 1), so |got + ref| <= 2 in the sum of squares)
    s, f64 = ref[f"{name}.stats"], flat.astype(np.float64)
    assert abs(f64.sum() - s[0]) <= 1e-5 * f64.size and abs(np.abs(f64).sum() - s[1]) <= 1e-5 * f64.size
    assert abs((f64 * f64).sum() - s[2]) <= 2e-5 * f64.size
    assert abs(f64.min() - s[3]) <= 1e-5 and abs(f64.max() - s[4]) <= 1e-5


def test_reference_state_dict_keys_match_the_manifest(ref):
    from calipsync_amd import arch
    ours = [(e[0], tuple(e[1])) for e in arch.manifest()]
    dims = iter(ref["state_dict.dims"].tolist())
    theirs = [(str(k), tuple(next(dims) for _ in range(n))) for k, n in zip(ref["state_dict.keys"], ref["state_dict.ndim"])]
    assert ours == theirs


# ---- rows f2 / f3-walk: the reference's frame-loop methods (FrameSynthesizer._get_audio_features /
#      _generate_frame_sequence), as recorded by tests/golden/make_reference_checks.py ----
def test_committed_window_fixture_is_reproducible_and_oracle_tracks_off_fixture(ref):
    from frame_data import golden_features
    from oracle import frame_loop_oracle
    fx = np.load(os.path.join(GOLDEN, "frame_windows.npz"))
    assert [bytes(d) for d in ref["win.T17.window_sha256"]] == [d.tobytes() for d in fx["T17.window_sha256"]]
    for t, seed in ((23, 5), (9, 6), (3, 7)):                                   # clips the fixture does not hold
        feats = golden_features(t, seed=seed)
        assert _sha(feats) == ref[f"win.T{t}s{seed}.features_sha256"].tobytes()
        idx = list(range(-2 * t - 3, 2 * t + 12))
        got = frame_loop_oracle.get_audio_features(feats, idx)
        assert got.dtype == np.float32 and got.shape == (len(idx), 32, 32, 32)
        assert [_sha(w) for w in got] == [bytes(d) for d in ref[f"win.T{t}s{seed}.window_sha256"]]


def test_committed_walk_fixture_is_reproducible_and_product_tracks_off_fixture(ref):
    from calipsync_amd.frame_walk import PingPongWalk
    fx = np.load(os.path.join(GOLDEN, "frame_walk.npz"))
    assert ref["walk.F37.mixed.s2.frames"].tolist() == fx["F37.mixed.s2.frames"].tolist()
    for total, seed in ((4, 9), (11, 10), (211, 11)):                           # off-fixture clips and seeds
        sizes = [random.Random(seed).choice([1, 2, 7, 8, 8, 64]) for _ in range(40)]
        assert sizes == ref[f"walk.F{total}.s{seed}.sizes"].tolist()
        frames = iter(ref[f"walk.F{total}.s{seed}.frames"].tolist())
        want = [[next(frames) for _ in range(n)] for n in sizes]
        walk = PingPongWalk(total, random.Random(seed))
        assert [walk.take(n) for n in sizes] == want
