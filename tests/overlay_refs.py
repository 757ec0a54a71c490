"""The reference for overlaying windows of several resident .lnn streams (tests/test_stream_overlay_cpu.py,
tests/test_gpu_stream_overlay.py): what LINNEAmd_OverlayWindowsDevice must write, from numpy int64 and Python integers on the oracle's
decode of the same bytes, never from the library under test.  Stated once, here; tests/test_stream_overlay_cpu.py holds it to
hand-written values."""
import numpy as np

from mix_refs import ELEMENT_BYTES, FORMATS  # noqa: F401  (the formats are the mix call's)

UNIT = 1 << 32


def gains(gain_q32, step_q32, n):
    """g(i) = (gain_q32 + step_q32 * i) >> 32 for i < n, the floor, in Python integers -> int64 (n,); every one must fit int16"""
    g = [(int(gain_q32) + int(step_q32) * i) >> 32 for i in range(n)] if n <= 4096 else None
    if g is None:                                               # long ramps: the same in int64 -- the ends fit int16, so nothing wraps
        assert -(1 << 63) <= int(gain_q32) + int(step_q32) * (n - 1) < 1 << 63 and -(1 << 63) <= int(step_q32) * (n - 1) < 1 << 63
        g = (np.int64(gain_q32) + np.int64(step_q32) * np.arange(n, dtype=np.int64)) >> np.int64(32)
    g = np.asarray(g, dtype=np.int64)
    assert n == 0 or (-32768 <= g[0] <= 32767 and -32768 <= g[-1] <= 32767), "a gain end outside int16"
    return g


def as_pair(gain):
    """a source's gain as overlay_windows takes it: an int, a constant gain, or a (gain_q32, step_q32) pair -> the pair"""
    return (int(gain) * UNIT, 0) if isinstance(gain, (int, np.integer)) else (int(gain[0]), int(gain[1]))


def overlaid_values(num_samples, sources, shift=0, clip_bits=0):
    """steps 1 to 3 of include/linne_amd.h LINNEAmd_OverlayWindowsDevice.  sources: (full, first, n, at, gain), full the decoded stream
    (C, ns) int32 -> (y int64 (C, num_samples), clipped?)"""
    assert 1 <= len(sources) <= 64 and 0 <= shift <= 31 and (clip_bits == 0 or 2 <= clip_bits <= 32)
    C = np.asarray(sources[0][0]).shape[0]
    acc = np.zeros((C, num_samples), dtype=np.int64)
    for full, first, n, at, gain in sources:
        full = np.asarray(full)
        assert full.dtype == np.int32 and full.shape[0] == C and n >= 1 and 0 <= first and first + n <= full.shape[1] and 0 <= at and at + n <= num_samples
        acc[:, at:at + n] += gains(*as_pair(gain), n)[None, :] * full[:, first:first + n].astype(np.int64)      # |a product| <= 2^46, 64 of them 2^52
    y = (acc + (1 << (shift - 1))) >> shift if shift else acc
    B = clip_bits or 32
    c = np.clip(y, -(1 << (B - 1)), (1 << (B - 1)) - 1)
    return c, bool((c != y).any())


def expected_overlay(num_samples, sources, shift=0, clip_bits=0, fmt="s32", bits=16):
    """the output in the format fmt -> (the elements (C, num_samples): int32, int16, uint8 (C, n, 3) little-endian, or float32;
    saturated: step 3 or the format's range clipped an element).  bits: the bits_per_sample of the first source's stream, the float
    format's scale where clip_bits is 0"""
    assert fmt in FORMATS
    y, sat = overlaid_values(num_samples, sources, shift, clip_bits)
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


def fade_ref(g0, g1, n):
    """what linne_amd.fade promises, stated apart from it: a pair whose gain is g0 at sample 0 and g1 at sample n"""
    span = (g1 - g0) * UNIT
    step = span // n if span >= 0 else -((-span) // n)
    return g0 * UNIT + UNIT // 2, step
