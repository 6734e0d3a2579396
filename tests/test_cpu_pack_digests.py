"""Every packed weight blob, byte for byte (CPU only): length and sha256 of what nqa_pack_vgg_weights writes in all eight
modes, and nqa_pack_conv_split for five layer shapes, against tests/golden/pack_digests.json -- recorded by
tools/pack_digests.py from the library as it was BEFORE the packers and the blob layout moved into csrc/nqa_weights.hip.
The inputs (tools/pack_digests.py): the stand-in weights; the same with an all-zero layer and layers scaled past both
clamps of weight_scale_exp; random layers for the single-layer packer.  The golden file is never written here."""
import ctypes as C
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("pack_digests", os.path.join(ROOT, "tools", "pack_digests.py"))
pack_digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pack_digests)

GUARD, FILL = 4096, 0xA5


@pytest.fixture(scope="module")
def lib():
    from nerf_qa_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "pack_digests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def vgg_inputs():
    return pack_digests.vgg_inputs()


def test_golden_covers_every_case(golden):
    assert set(golden) == {"synth", "edge", "conv_split"}
    assert set(golden["synth"]) == set(golden["edge"]) == set(pack_digests.MODES)
    assert len(golden["conv_split"]) == len(pack_digests.CONV_SPLIT_SHAPES)


@pytest.mark.parametrize("mode", pack_digests.MODES)
@pytest.mark.parametrize("name", ["synth", "edge"])
def test_vgg_blob_digest(name, mode, vgg_inputs, golden, lib):
    from nerf_qa_amd import ops
    assert pack_digests.digest(ops.pack_vgg_weights(vgg_inputs[name], mode).numpy()) == golden[name][mode]


def test_conv_split_blob_digests(golden, lib):
    from nerf_qa_amd import ops
    got = [pack_digests.digest(ops.pack_conv_split(w).numpy()) for w in pack_digests.conv_split_inputs()]
    assert got == golden["conv_split"]


def _guarded(nbytes):
    assert nbytes > 0
    return np.full(nbytes + GUARD, FILL, np.uint8)


def _check_guarded(buf, nbytes, want):
    assert (buf[nbytes:] == FILL).all(), "the packer wrote past the size it reports"
    assert nbytes == want["bytes"] and hashlib.sha256(buf[:nbytes].tobytes()).hexdigest() == want["sha256"]


@pytest.mark.parametrize("mode", pack_digests.MODES)
def test_vgg_pack_stays_inside_its_size(mode, vgg_inputs, golden, lib):
    """nqa_pack_vgg_weights straight into a buffer with 4096 bytes of 0xA5 behind nqa_packed_weights_bytes: those stay,
    and what lies before them is the recorded blob (so every byte of it was written, none left as 0xA5)."""
    from nerf_qa_amd import _lib
    p = _lib.prec_id(mode)
    convs = vgg_inputs["synth"]
    nbytes = lib.nqa_packed_weights_bytes(p)
    buf = _guarded(nbytes)
    wp = (C.c_void_p * len(convs))(*[w.ctypes.data for w, _ in convs])
    bp = (C.c_void_p * len(convs))(*[b.ctypes.data for _, b in convs])
    assert lib.nqa_pack_vgg_weights(wp, bp, p, buf.ctypes.data) == 0
    _check_guarded(buf, nbytes, golden["synth"][mode])


def test_conv_split_pack_stays_inside_its_size(golden, lib):
    for w, want in zip(pack_digests.conv_split_inputs(), golden["conv_split"]):
        cout, cin = w.shape[:2]
        nbytes = lib.nqa_packed_conv_split_bytes(cout, cin)
        buf = _guarded(nbytes)
        assert lib.nqa_pack_conv_split(w.ctypes.data, cout, cin, buf.ctypes.data) == 0
        _check_guarded(buf, nbytes, want)
