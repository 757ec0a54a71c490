"""The reference for mixing the channels of windows of resident .lnn streams (tests/test_stream_mix_cpu.py, tests/test_gpu_stream_mix.py):
what LINNEAmd_MixWindowsDevice must write, from numpy int64 on the oracle's decode of the same bytes, never from the library under test.
Stated once, here; tests/test_stream_mix_cpu.py holds it to hand-written values."""
import numpy as np

FORMATS = ("s32", "s16", "s24", "f32")
ELEMENT_BYTES = {"s32": 4, "s16": 2, "s24": 3, "f32": 4}


def mixed_values(v, matrix, shift=0, clip_bits=0):
    """steps 1 to 3 of include/linne_amd.h LINNEAmd_MixWindowsDevice on the frames v (C, n) int32 -> (y int64 (Co, n), clipped?).
    matrix: (Co, >= C) integers within int16, of which the first C columns count"""
    v = np.asarray(v)
    assert v.dtype == np.int32 and v.ndim == 2
    C = v.shape[0]
    m = np.asarray(matrix, dtype=np.int64)[:, :C]
    assert m.ndim == 2 and 1 <= m.shape[0] <= 8 and m.shape[1] == C and m.min(initial=0) >= -32768 and m.max(initial=0) <= 32767
    assert 0 <= shift <= 31 and (clip_bits == 0 or 2 <= clip_bits <= 32)
    acc = m @ v.astype(np.int64)                                 # |a product| <= 2^46, eight of them 2^49: int64 holds it
    y = (acc + (1 << (shift - 1))) >> shift if shift else acc   # (numpy's >> on int64 is arithmetic)
    B = clip_bits or 32
    c = np.clip(y, -(1 << (B - 1)), (1 << (B - 1)) - 1)
    return c, bool((c != y).any())


def expected_mix(full, first, n, matrix, shift=0, clip_bits=0, fmt="s32", bits=16):
    """window [first, first + n) of the decoded stream `full` (C, ns) int32 through the matrix, in the format fmt -> (the elements
    (Co, n): int32, int16, uint8 (Co, n, 3) little-endian, or float32; saturated: step 3 or the format's range clipped an element).
    bits: the stream's bits_per_sample, the float format's scale where clip_bits is 0"""
    assert fmt in FORMATS
    y, sat = mixed_values(np.ascontiguousarray(np.asarray(full)[:, first:first + n], dtype=np.int32), matrix, shift, clip_bits)
    if fmt == "s32":
        return y.astype(np.int32), sat
    if fmt == "f32":
        Bf = clip_bits or bits
        return y.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -(Bf - 1)), sat
    top = 32767 if fmt == "s16" else 8388607
    c = np.clip(y, -top - 1, top)
    sat = sat or bool((c != y).any())
    if fmt == "s16":
        return c.astype(np.int16), sat
    u = (c & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8), sat


def random_matrix(rng, Co, C, garbage=True):
    """(8, 8) int16: random coefficients with the extremes among them in the (Co, C) corner, garbage (or zeros) elsewhere"""
    m = rng.integers(-32768, 32768, size=(8, 8)).astype(np.int16) if garbage else np.zeros((8, 8), dtype=np.int16)
    core = rng.integers(-32768, 32768, size=(Co, C))
    flat = core.reshape(-1)
    for at, x in zip(rng.permutation(flat.size), (32767, -32767, -32768, 0, 1, -1)):         # (a matrix of one or two entries has the first of them)
        flat[at] = x
    m[:Co, :C] = core
    return m
