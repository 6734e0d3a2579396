#!/usr/bin/env python3
"""Byte length and sha256 of every packed weight blob the host packers produce, as JSON (CPU only, no GPU is used).

    python tools/pack_digests.py > digests.json          (NQA_LIB=... selects another build of the library)

tests/golden/pack_digests.json is this tool's output for a library built from the commit BEFORE the packers moved to
csrc/nqa_weights.hip; tests/test_cpu_pack_digests.py holds the tree's own library to it.  The blob format is part of
what the kernels compute: record the file again only together with a deliberate change of the format.

    synth        ops.pack_vgg_weights(synth.vgg16_weights(1234), mode), all eight modes
    edge         the same weights with layer 3 all zero (weight_scale_exp's k = 0 path), layer 5 times 1e8 (its lower
                 clamp, k = -8) and layer 8 times 1e-9 (its upper clamp, k = 24)
    conv_split   ops.pack_conv_split of five random layers, (cout, cin) as in CONV_SPLIT_SHAPES
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("f32", "bf16", "f16", "f32s", "f32m", "f32m2", "f32m4", "f16w")
CONV_SPLIT_SHAPES = ((64, 64), (64, 128), (128, 128), (256, 512), (512, 512))  # (cout, cin), drawn in this order


def vgg_inputs() -> dict:
    """{"synth" | "edge": 13 (weight, bias) pairs}"""
    from nerf_qa_amd import synth
    convs = synth.vgg16_weights(1234)
    edge = [(w.copy(), b) for w, b in convs]
    edge[3][0][...] = 0
    edge[5][0][...] *= np.float32(1e8)
    edge[8][0][...] *= np.float32(1e-9)
    return {"synth": convs, "edge": edge}


def conv_split_inputs() -> list:
    rng = np.random.default_rng(5)
    return [rng.standard_normal((cout, cin, 3, 3)).astype(np.float32) * 0.02 for cout, cin in CONV_SPLIT_SHAPES]


def digest(blob) -> dict:
    """blob: numpy uint8 array"""
    return {"bytes": int(blob.nbytes), "sha256": hashlib.sha256(blob.tobytes()).hexdigest()}


def digests() -> dict:
    from nerf_qa_amd import ops
    out = {name: {m: digest(ops.pack_vgg_weights(convs, m).numpy()) for m in MODES}
           for name, convs in vgg_inputs().items()}
    out["conv_split"] = [digest(ops.pack_conv_split(w).numpy()) for w in conv_split_inputs()]
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    json.dump(digests(), sys.stdout, indent=1)
    sys.stdout.write("\n")
