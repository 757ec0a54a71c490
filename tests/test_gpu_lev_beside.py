"""The long layer's order-128 Levinson launch beside the short-trial lag kernels (LINNE_AMD_LEV_BESIDE; lnn_forms.h lev_beside): the
solver on the chunk's sibling stream, the small-LDS k_autocorr_sub beside it, the riding trials dealt over the two blocks of the trial-1
launch.  Stereo at -m 7 with LINNE_AMD_HIST=1 (small batches then take the lanes = jobs lag kernels), music from tests/signals, the
smallest shapes where this can go wrong.  With the form forced off and on in fresh contexts every output must be equal bit for bit --
same products, same adds, same order -- and a second call in the same context must repeat the first (nothing left in flight)."""
import numpy as np
import pytest

import linne_amd
from signals import music, music_frames

pytestmark = pytest.mark.gpu

NCH, BITS, PRESET = 2, 16, 7


def case_partial_block():
    """17 frames of 10 240 samples: 136 jobs, the last 64-job block holds 8"""
    return 10240, music_frames(17, NCH, 10240, BITS, seed=601), None


def case_shortest_block():
    """16 frames of 4096 samples: 32 samples per finest unit, the shortest block hist_takes"""
    return 4096, music_frames(16, NCH, 4096, BITS, seed=602), None


def case_ragged_tail():
    """9 frames, the last of 9280 samples: its lags come from the general kernel on the sibling stream the solver shares"""
    frames = music_frames(9, NCH, 10240, BITS, seed=603)
    frames[-1, :, 9280:] = 0
    return 10240, frames, np.array([10240] * 8 + [9280], dtype=np.uint32)


def case_silent_frame():
    """a frame of silence among music: zero problems in the lanes of a wave"""
    frames = music_frames(9, NCH, 10240, BITS, seed=604)
    frames[4] = 0
    return 10240, frames, None


CASES = {"partial_block": case_partial_block, "shortest_block": case_shortest_block, "ragged_tail": case_ragged_tail, "silent_frame": case_silent_frame}


def encode(ctx_env, beside, block, frames, ns, calls=1, **env):
    outs = []
    with ctx_env({"LINNE_AMD_HIST": "1", "LINNE_AMD_LEV_BESIDE": beside, **env}) as ctx:
        shape = ctx.shape(NCH, BITS, block, PRESET, True)
        for _ in range(calls):
            res, prm, st = ctx.encode_frames_host(shape, frames, ns)
            outs.append((res, prm, st, ctx.last_fallback_count()))
    return outs


def same(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("residual", "parameters", "statistics")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {name} differ"
    assert a[3] == b[3], f"{what}: fallback count {a[3]} vs {b[3]}"


@pytest.mark.parametrize("name", list(CASES))
def test_beside_equals_serial_bit_for_bit(ctx_env, oracle, name):
    block, frames, ns = CASES[name]()
    (off,) = encode(ctx_env, "0", block, frames, ns)
    on1, on2 = encode(ctx_env, "1", block, frames, ns, calls=2)
    same(off, on1, "LEV_BESIDE=0 against =1")
    same(on1, on2, "two calls of one context")
    (inline,) = encode(ctx_env, "2", block, frames, ns)           # the measuring form: the same launches, the solver on the chunk's own stream
    same(off, inline, "LEV_BESIDE=0 against =2")
    if name == "silent_frame":
        assert not off[0][4].any() and not on1[0][4].any()
    if name == "partial_block":
        # the packed blocks against the oracle's EncodeBlock bytes: its stream behind the 30-byte header
        shape = linne_amd.Shape(NCH, BITS, block, PRESET, 1)
        blocks, _ = linne_amd.pack_frames(shape, frames, on1[0], on1[1], on1[2], None, 0.0, 2)
        x = np.ascontiguousarray(frames.transpose(1, 0, 2).reshape(NCH, -1))
        want = oracle.encode_whole(x, BITS, 44100, block, PRESET, True)
        assert b"".join(bytes(b) for b in blocks) == want[30:], "packed blocks differ from the oracle's"


def test_two_halves_each_with_a_sibling(ctx_env):
    """LINNE_AMD_STREAMS=2 forks a call of 1024 frames into two chunks on two compute streams (lnn_call_split: 512 frames per stream when
    the count is forced): stream slot 1 takes the second sibling stream, created by the first chunk that sends its solver there, and
    the second pair of events.  1023 frames of 4096 samples and a ragged one, so that one half also has the general lag kernel on its
    sibling; the frames are 32 music frames repeated at 32 levels."""
    block, F = 4096, 1024
    base = music_frames(32, NCH, block, BITS, seed=605)
    frames = np.concatenate([base // (1 + g) for g in range(F // 32)]).astype(np.int32)
    frames[-1, :, 3000:] = 0
    ns = np.array([block] * (F - 1) + [3000], dtype=np.uint32)
    (off,) = encode(ctx_env, "0", block, frames, ns, LINNE_AMD_STREAMS="2")
    on1, on2 = encode(ctx_env, "1", block, frames, ns, calls=2, LINNE_AMD_STREAMS="2")
    same(off, on1, "two streams: LEV_BESIDE=0 against =1")
    same(on1, on2, "two streams: two calls of one context")
