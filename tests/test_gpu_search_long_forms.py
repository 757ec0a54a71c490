"""k_search_long's two grid forms -- (jobs, tiles) blocks and one block per job that walks the job's tiles -- give the same encode.

Each case encodes one batch twice, with LINNE_AMD_SEARCH_JOB=0 and =1, and asserts that residual, parameters and statistics are
equal word for word, that the count of exact fallbacks is equal, that the forced form is the one that ran (kind 25 was launched
and LINNEAmd_GetLastSearchLongForm names the form), and that every frame equals the oracle's hot path.  A batch is a handful of
distinct frames -- music, a frame of silence, a frame of a constant (both take the exact fallback) -- tiled over the frame count,
all full 10 240-sample frames except one ragged tail (which stays with k_fir2<2>).  The cases: -m 7 (128-tap long layer, four
regularisers) and -m 3 (64 taps, two), stereo at two batch sizes above SEARCH_JOB_MIN jobs per launch (lnn_k_search.h), the
threshold from which the per-job form is chosen when nothing is forced, and mono batches of one frame below it (4 and 2 jobs).
One stream, so that a launch sees the whole batch.
"""
import ctypes

import numpy as np
import pytest

import linne_amd
from signals import music_frames

NCH, BITS, BLOCK = 2, 16, 10240
NBASE = 6                       # music frames; base NBASE is silence, NBASE + 1 a constant
TAIL = 5000                     # the last frame's length
SEARCH_JOB_MIN = 8              # lnn_k_search.h


def build_batch(F, seed, NCH=NCH):
    """([F][C][BLOCK] int32, lengths, base index of every frame): bases cycle with period NBASE + 2, the last frame is ragged"""
    bases = np.zeros((NBASE + 2, NCH, BLOCK), dtype=np.int32)
    bases[:NBASE] = music_frames(NBASE, NCH, BLOCK, BITS, seed=seed)
    bases[NBASE + 1] = 1000
    bmap = np.arange(F) % (NBASE + 2)
    ns = np.full(F, BLOCK, dtype=np.uint32)
    ns[-1] = TAIL
    frames = bases[bmap]
    frames[-1, :, TAIL:] = 0
    return np.ascontiguousarray(frames), ns, bmap


def oracle_runs(oracle, frames, ns, bmap, preset, NCH=NCH):
    """the oracle's hot path once per distinct (base, length): {key: (tap, residual)}"""
    out = {}
    for f in range(len(ns)):
        key = (int(bmap[f]), int(ns[f]))
        if key in out:
            continue
        enc = oracle.encoder(NCH, BITS, 44100, BLOCK, preset, NCH == 2)
        out[key] = enc.hotpath(frames[f][:, :int(ns[f])])
        enc.close()
    return out


def jobs_of(F, preset, NCH=NCH):
    return F * NCH * linne_amd.PRESET_NUM_REGULARS[preset]


def test_inputs_and_oracle_on_the_host(oracle):
    """the builder and the oracle side of the comparison, without a GPU: the batch has its silent, constant and ragged frames, and
    the oracle encodes each distinct frame"""
    frames, ns, bmap = build_batch(11, seed=5)
    assert frames.shape == (11, NCH, BLOCK) and int(ns[-1]) == TAIL and (ns[:-1] == BLOCK).all()
    assert not frames[NBASE].any() and (frames[NBASE + 1] == 1000).all() and not frames[-1, :, TAIL:].any()
    runs = oracle_runs(oracle, frames, ns, bmap, 7)
    assert len(runs) == NBASE + 2 + 1                       # the ragged frame is a key of its own
    for (b, n), (tap, res) in runs.items():
        assert res.shape == (NCH, n)
    mono = build_batch(1, seed=5, NCH=1)
    assert mono[0].shape == (1, 1, BLOCK) and len(oracle_runs(oracle, *mono, 7, NCH=1)) == 1
    assert jobs_of(1, 7, 1) < SEARCH_JOB_MIN <= jobs_of(1, 7) and jobs_of(1, 3, 1) < SEARCH_JOB_MIN <= jobs_of(40, 3)


def _encode(ctx_env, env, preset, frames, ns):
    from test_gpu_batch_forms import scratch_for
    nch = frames.shape[1]
    with ctx_env(env, scratch_bytes=scratch_for(nch, BITS, BLOCK, preset, nch == 2, len(ns))) as c:
        shape = c.shape(nch, BITS, BLOCK, preset, nch == 2)
        c.enable_timing(True)
        res, prm, st = c.encode_frames_host(shape, frames, ns)
        fn = linne_amd.lib.LINNEAmd_GetLastSearchLongForm
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
        return res, prm, st, c.last_launches(25), int(fn(c.h)), c.last_fallback_count(), c.last_min_margin()


@pytest.mark.gpu
@pytest.mark.parametrize("preset,F,nch", [(7, 40, 2), (7, 1100, 2), (3, 40, 2), (3, 2200, 2), (7, 1, 1), (3, 1, 1)])
def test_both_forms_give_the_same_encode_and_the_oracles(ctx_env, oracle, preset, F, nch):
    from test_gpu_parity import _check_taps
    frames, ns, bmap = build_batch(F, seed=100 + preset, NCH=nch)
    if F == 1:
        ns[0] = BLOCK                                       # below the threshold: one full mono frame (a ragged one is not k_search_long's)
        frames = build_batch(2, seed=100 + preset, NCH=nch)[0][:1]
    big = jobs_of(F, preset, nch) >= SEARCH_JOB_MIN
    got = {}
    for form in (0, 1):
        got[form] = _encode(ctx_env, {"LINNE_AMD_SEARCH_JOB": str(form), "LINNE_AMD_STREAMS": "1"}, preset, frames, ns)
        res, prm, st, launches, ran, fallbacks, margin = got[form]
        print(f"-m {preset}, {F} frames of {nch} channels, form {form}: {launches} launches of kind 25, form {ran} ran, {fallbacks} exact fallbacks, min margin {margin:.6e}")
        assert launches >= 1, "k_search_long was not launched"
        assert ran == form, f"form {form} was forced, form {ran} ran"
    auto = _encode(ctx_env, {"LINNE_AMD_STREAMS": "1"}, preset, frames, ns)
    assert auto[4] == (1 if big else 0), f"{jobs_of(F, preset, nch)} jobs: the rule chose form {auto[4]}"
    for name, k in (("residual", 0), ("parameters", 1)):
        assert np.array_equal(got[0][k], got[1][k]), f"{name} differ between the forms"
        assert np.array_equal(got[0][k], auto[k]), f"{name} differ between the forced and the chosen form"
    assert np.array_equal(got[0][2], got[1][2], equal_nan=True) and np.array_equal(got[0][2], auto[2], equal_nan=True), "statistics differ between the forms"
    assert got[0][5] == got[1][5] == auto[5], f"exact fallbacks: {got[0][5]} / {got[1][5]} / {auto[5]}"
    if F > 1:
        assert got[0][5] > 0, "the silent and the constant frames were to take the exact fallback"
    runs = oracle_runs(oracle, frames, ns, bmap, preset, NCH=nch)
    res, prm, st = got[1][:3]
    for f in range(F):
        n = int(ns[f])
        tap, ores = runs[(int(bmap[f]), n)]
        assert np.array_equal(res[f][:, :n], ores), f"frame {f}: residual differs from the oracle"
        assert not res[f][:, n:].any(), f"frame {f}: residual behind its end"
        _check_taps(tap, prm[f], st[f], preset, nch, f"frame {f}")
