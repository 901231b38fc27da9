"""The packed layouts of the four handles behind one PackedLayout (csrc/handle.h): bit for bit what they were before the
handles shared it (tests/golden/packed_layouts.json: count, total and a sha256 over "name:offset:size" lines, recorded from
the library before the change), the accessors' answers out of range, and _lib.pack_named / unpack_named.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

from calipsync_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_layouts.json")
LAYOUTS = {
    "unet_hubert": lambda: _lib.packed_layout("hubert"),
    "unet_wenet": lambda: _lib.packed_layout("wenet"),
    "hubert_1": lambda: _lib.hubert_layout(1),
    "hubert_2": lambda: _lib.hubert_layout(2),
    "hubert_24": lambda: _lib.hubert_layout(24),
    "hubert_48": lambda: _lib.hubert_layout(48),
    "pfld": _lib.pfld_layout,
    "s3fd": _lib.s3fd_layout,
}


@pytest.fixture(scope="module")
def lib():
    from calipsync_amd import build
    build.build()            # cross-compiles for gfx950 without a GPU
    return _lib.load()


def test_the_fixture_names_every_layout():
    assert set(json.load(open(GOLDEN))) == set(LAYOUTS)


@pytest.mark.parametrize("key", sorted(LAYOUTS))
def test_layout_is_what_it_was(lib, key):
    want = json.load(open(GOLDEN))[key]
    items, total = LAYOUTS[key]()
    digest = hashlib.sha256("".join(f"{n}:{o}:{s}\n" for n, o, s in items).encode()).hexdigest()
    assert {"count": len(items), "total": int(total), "sha256": digest} == want


def test_unet_accessors_without_a_mode_are_the_hubert_layout(lib):
    items = [(lib.casync_packed_name(i).decode(), lib.casync_packed_offset(i), lib.casync_packed_size(i))
             for i in range(lib.casync_packed_count())]
    assert (items, lib.casync_packed_total()) == _lib.packed_layout("hubert")


def test_hubert_has_no_layout_outside_1_to_48_layers(lib):
    assert lib.casync_hubert_packed_count(0) == 0 and lib.casync_hubert_packed_count(49) == 0
    for layers in (0, 49):
        with pytest.raises(ValueError, match=f"no packed layout for {layers} layers"):
            _lib.hubert_layout(layers)


@pytest.mark.parametrize("prefix,args", [("", ()), ("hubert_", (2,)), ("pfld_", ()), ("s3fd_", ())])
def test_accessors_out_of_range(lib, prefix, args):
    count = getattr(lib, f"casync_{prefix}packed_count")(*args)
    assert count > 0
    for i in (-1, count):
        assert getattr(lib, f"casync_{prefix}packed_name")(*args, i) is None
        assert getattr(lib, f"casync_{prefix}packed_offset")(*args, i) == -1
        assert getattr(lib, f"casync_{prefix}packed_size")(*args, i) == -1
    assert getattr(lib, f"casync_{prefix}packed_name")(*args, count - 1) is not None


def test_unet_mode_accessors_out_of_range(lib):
    for mode in (0, 1):
        count = lib.casync_packed_count_m(mode)
        for i in (-1, count):
            assert lib.casync_packed_name_m(mode, i) is None
            assert lib.casync_packed_offset_m(mode, i) == -1 and lib.casync_packed_size_m(mode, i) == -1
    assert lib.casync_packed_count_m(2) == 0 and lib.casync_packed_name_m(2, 0) is None
    assert lib.casync_packed_offset_m(2, 0) == -1 and lib.casync_packed_size_m(2, 0) == -1 and lib.casync_packed_total_m(2) == -1


# ---------------------------------------------------------------------------------------------- pack_named / unpack_named
SYNTHETIC = ([("a.w", 0, 6), ("a.b", 64, 3), ("z", 128, 1)], 192)


def _named():
    return {"a.w": np.arange(6, dtype=np.float32).reshape(2, 3) + 1, "a.b": np.array([7, 8, 9], np.float32),
            "z": np.array([0.5], np.float32)}


def test_pack_named_round_trips_through_unpack_named():
    buf = _lib.pack_named(_named(), SYNTHETIC)
    assert buf.shape == (192,) and buf.dtype == np.float32
    back = _lib.unpack_named(buf, SYNTHETIC)
    assert list(back) == ["a.w", "a.b", "z"]
    for name, a in _named().items():
        assert np.array_equal(back[name], a.reshape(-1)), name
    used = np.zeros(192, bool)
    for _, off, size in SYNTHETIC[0]:
        used[off:off + size] = True
    assert not buf[~used].any()          # the padding between tensors stays zero


def test_pack_named_names_the_tensor_of_the_wrong_size():
    named = _named()
    named["a.b"] = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match=r"packed tensor a\.b: 4 floats, the engine expects 3"):
        _lib.pack_named(named, SYNTHETIC)


def test_pack_named_refuses_a_leftover_name():
    named = _named()
    named["stray"] = np.zeros(1, np.float32)
    with pytest.raises(ValueError, match=r"tensors the engine layout does not name: \['stray'\]"):
        _lib.pack_named(named, SYNTHETIC)
