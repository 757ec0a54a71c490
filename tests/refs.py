"""Test-side names of the checkers and of the public-API binding (see oracle/bindings.py and linne_amd/api.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bindings import (MAX_CH, MAX_LAYERS, MAX_PARAMS, ORACLE_SO, PRESET_LAYERS, REF_SO, ChannelTap, EncodeParameter,  # noqa: E402,F401
                      FrameTap, Oracle, Reference, fnv1a64, oracle_available, reference_available)
from linne_amd.api import (LinneApi, _planar_ptrs, _RefDecoderConfig, _RefEncodeParameter, _RefEncoderConfig,  # noqa: E402,F401
                           _RefHeader)


import hashlib  # noqa: E402
import json  # noqa: E402

import numpy as np  # noqa: E402

ANSWERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_answers.json")


def digest(data):
    """length and sha256 of bytes, or of an array's int32 samples in C order"""
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.int32).tobytes()
    data = bytes(data)
    return {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def _tag(data):
    return digest(data)["sha256"][:20]


def encode_key(x, bits, rate, block, preset, ms, af_iters=0, learning=0):
    x = np.asarray(x)
    return f"encode_whole/{x.shape[0]}x{x.shape[1]}/{_tag(x)}/bits{bits}/rate{rate}/block{block}/m{preset}/ms{int(bool(ms))}/a{af_iters}/l{int(learning)}"


def blocks_key(x, bits, rate, block, preset, ms, lens):
    x = np.asarray(x)
    return f"encode_blocks/{x.shape[0]}x{x.shape[1]}/{_tag(x)}/bits{bits}/rate{rate}/block{block}/m{preset}/ms{int(bool(ms))}/lens{_tag(np.asarray(lens, dtype=np.int32))}"


def decode_key(stream):
    return f"decode_whole/{_tag(stream)}"


def cli_key(args, data):
    return f"cli {' '.join(args)}/{_tag(data)}"


class Recorded:
    """one answer of the real reference as tests/golden/make_reference_golden.py recorded it (length + sha256): it compares
    equal to the bytes (or the int32 samples) the reference gave, and to nothing else"""

    def __init__(self, key, rec):
        self.key, self.rec = key, {"bytes": rec["bytes"], "sha256": rec["sha256"]}

    def __eq__(self, other):
        if isinstance(other, Recorded):
            return self.rec == other.rec
        if not isinstance(other, (bytes, bytearray, memoryview, np.ndarray)):
            return NotImplemented
        return digest(other) == self.rec

    __hash__ = None

    def __repr__(self):
        return f"<the reference's answer to {self.key}: {self.rec['bytes']} bytes, sha256 {self.rec['sha256'][:16]}...>"


class RecordedReference:
    """the real reference's answers for the tests' inputs, recorded from oracle/_ref by tests/golden/make_reference_golden.py into
    tests/golden/reference_answers.json: the tests need neither the reference's sources nor a build of them.  An input the
    recording does not hold is an error (rerun the script where oracle/_ref is built), never a skip."""

    def __init__(self, path=ANSWERS):
        with open(path) as f:
            self.answers = json.load(f)

    def _get(self, key):
        if key not in self.answers:
            raise KeyError(f"no recorded reference answer for {key} (tests/golden/make_reference_golden.py records them)")
        return self.answers[key]

    def encode_whole(self, x, bits, rate, block, preset, ms, af_iters=0, learning=0):
        key = encode_key(x, bits, rate, block, preset, ms, af_iters, learning)
        return Recorded(key, self._get(key))

    def encode_block_lengths(self, x, bits, rate, block, preset, ms, lens):
        """header + one EncodeBlock call per entry of `lens` (any length up to the block size)"""
        key = blocks_key(x, bits, rate, block, preset, ms, lens)
        return Recorded(key, self._get(key))

    def decode_whole(self, stream):
        """(return code, decoded samples) of DecodeWhole with the CRC check on"""
        key = decode_key(stream)
        rec = self._get(key)
        return rec["ret"], Recorded(key, rec["pcm"])

    def cli(self, args, data):
        """the bytes the reference's command line tool writes for `args` (-e -m N: encode, -d: decode) and the input file's bytes"""
        key = cli_key(args, data)
        return Recorded(key, self._get(key))
