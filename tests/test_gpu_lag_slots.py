"""The long layer's lanes = jobs lag kernels at the smallest shapes at which they do real work, against the oracle, frame by frame.

k_autocorr_hist<P, TT> deals the PT + 1 lags of a trial over its waves: every wave but the last owns HIST_LPW lags, the last one what is
left (8 of 129 at order 128, 2 of 65 at order 64) and runs a tile loop of its own with that many chains.  A lag dropped or doubled where
one wave's lags end and the next one's begin -- lag J0 of each wave, the last lag of the last wave -- changes the coefficients of the
layer, and with them the residual of every frame it touches: the cases below compare parameters, statistics and residual of EVERY frame
with the oracle's, and assert the launch counts the rules give (lnn_forms.h), so that a moved threshold fails the case instead of
letting it test other kernels.

Shapes, from hist_takes (lnn_forms.h) and AcCfg (every trial u = 1 .. min(P, 128) present): the analysis length must be a multiple of
16 << (NT - 1) and hold 32 samples per finest unit.  A 128-tap layer has NT = 8 trials: multiples of 2048 of at least 128 x 32 = 4096,
so 4096 samples is the smallest frame; a 64-tap layer NT = 7: multiples of 1024 of at least 64 x 32 = 2048.  The kernels are launched
from 12 288 jobs on; each case has a few more, and a job count that is no multiple of 64: the last block of a run is partial.

Blocks of these kernels never mix frame lengths under the rules as they stand -- the rows are cut into runs of one length class, and a
batch with more runs than RowRuns holds switches the kernels off -- so the block-uniform early return is reached through its other
term: a block whose length class the kernels do not take (case "ragged": frames of 1000 samples, which stay with the general kernel).
Case "two_lengths" has two classes the kernels DO take (2048 and 4096 samples in blocks of 4096, a 64-tap layer): two runs with
different tile counts, each ending in a partial block.

Material: the bench's synthetic recipe (tests/signals.py music) at three levels, one all-zero frame, one frame of full-scale white noise.
"""
import os

import numpy as np
import pytest

import linne_amd
from signals import music
from test_gpu_batch_forms import OracleBatch, check_encode, hist_takes, scratch_for

pytestmark = pytest.mark.gpu

NB = 11                                 # distinct base frames
KINDS = (3, 21, 22, 23)                 # the general long-layer lag kernel, k_autocorr_hist<P,0>, <P,1>, k_autocorr_sub (include/linne_amd.h)
HIST_MIN_JOBS = 12288                   # lnn_forms.h: cf->hist


def bases(nch, bits, block, seed):
    """[NB][C][block]: 0 all zero, 1 full-scale white noise, the others music at 1, 1/3 and 3x (clipped) level"""
    hi, lo = (1 << (bits - 1)) - 1, -(1 << (bits - 1))
    out = np.zeros((NB, nch, block), dtype=np.int32)
    out[1] = np.random.default_rng(seed).integers(lo, hi + 1, size=(nch, block)).astype(np.int32)
    for b in range(2, NB):
        x = music(nch, block, bits, seed=seed * 100 + b).astype(np.int64)
        if b % 3 == 1:
            x = np.trunc(x / 3.0).astype(np.int64)
        elif b % 3 == 2:
            x = np.clip(3 * x, lo, hi)
        out[b] = x
    return out


def make_batch(F, nch, bits, block, preset, seed, short=0, nshort=0):
    """F frames drawn from the bases by a seeded map (the first NB frames: every base once); nshort of them, at random places,
    `short` samples long"""
    rng = np.random.default_rng(seed)
    bs = bases(nch, bits, block, seed)
    bmap = rng.integers(0, NB, size=F)
    bmap[:NB] = np.arange(NB)
    ns = np.full(F, block, dtype=np.uint32)
    if nshort:
        ns[rng.choice(np.arange(NB, F), size=nshort, replace=False)] = short
    frames = bs[bmap]
    for f in np.flatnonzero(ns < block):
        frames[f, :, int(ns[f]):] = 0
    return {"frames": np.ascontiguousarray(frames), "ns": ns, "bases": bs, "bmap": bmap, "nch": nch, "bits": bits, "block": block, "preset": preset}


# name: (preset, bits, block, F, short, nshort, expected launches)
#   p128_min     -m 5 (4 / 128 / 16 taps, one regulariser): 6 203 stereo frames of 4096 samples, J = 12 406 = 193 x 64 + 54; every frame the
#                kernels': no general launch
#   p64_min      -m 3 (4 / 64 / 8, two regularisers): 3 101 stereo frames of 2048 samples, J = 12 404 = 193 x 64 + 52
#   ragged       -m 5, 6 203 frames of which 300 hold 1000 samples: their 600 jobs' blocks return early, the general kernel has them;
#                the full frames' run is 11 806 jobs = 184 x 64 + 30
#   two_lengths  -m 3, blocks of 4096: 3 077 frames (J = 12 308) of which 1 000 hold 2048 samples: runs of 4 000 = 62 x 64 + 32 and
#                8 308 = 129 x 64 + 52 jobs, 2 and 4 tiles of 16 positions per finest unit
CASES = {
    "p128_min": (5, 16, 4096, 6203, 0, 0, {3: 0, 21: 1, 22: 1, 23: 1}),
    "p64_min": (3, 16, 2048, 3101, 0, 0, {3: 0, 21: 1, 22: 0, 23: 1}),
    "ragged": (5, 16, 4096, 6203, 1000, 300, {3: 1, 21: 1, 22: 1, 23: 1}),
    "two_lengths": (3, 16, 4096, 3077, 2048, 1000, {3: 0, 21: 1, 22: 0, 23: 1}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_lag_kernels_at_their_smallest_shapes(ctx_env, oracle, name):
    for v in os.environ:
        assert not v.startswith("LINNE_AMD_"), f"{v} is set: these cases run the rules as they stand"
    preset, bits, block, F, short, nshort, want = CASES[name]
    nch, ms = 2, True
    R = linne_amd.PRESET_NUM_REGULARS[preset]
    J = F * nch * R
    assert HIST_MIN_JOBS <= J < HIST_MIN_JOBS + 128 and J % 64 != 0, f"J = {J}: just past the threshold, the last block partial"
    batch = make_batch(F, nch, bits, block, preset, seed=1000 + preset, short=short, nshort=nshort)
    taken = np.array([hist_takes(int(n), preset, block, 1) for n in batch["ns"]])
    assert taken[batch["ns"] == block].all(), "full frames are the kernels'"
    smallest = min(n for n in range(8, block + 1, 8) if hist_takes(n, preset, block, 1))
    assert smallest == (short if name == "two_lengths" else block), f"{smallest}: the smallest length the kernels take is in the batch"
    if short:
        assert taken[batch["ns"] == short].all() if want[3] == 0 else not taken[batch["ns"] == short].any()
        for n in (block, short):
            rows = int((batch["ns"] == n).sum()) * nch * R
            assert rows % 64 != 0, f"the run of {n}-sample frames ends in a partial block"
    ob = OracleBatch(oracle, batch, ms)
    with ctx_env({}, scratch_bytes=scratch_for(nch, bits, block, preset, ms, F)) as c:
        shape = c.shape(nch, bits, block, preset, ms)
        c.enable_timing(True)
        res, prm, st = c.encode_frames_host(shape, batch["frames"], batch["ns"])
        ran = {k: c.last_launches(k) for k in KINDS}
    print(f"{name}: J = {J}, launches {ran}, {len(np.unique(ob.key))} oracle runs")
    check_encode(ob, batch, res, prm, st, name)
    assert ran == want, f"{name}: launches {want} expected, {ran} ran"
