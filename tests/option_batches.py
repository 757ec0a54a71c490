"""What tests/test_option_batches_cpu.py and tests/test_gpu_option_batches.py share: the batches that hold -a N and -l to the oracle
frame by frame at job counts past the 64- and 256-job launch rules, as plain data, the oracle's answers for them, and what
lnn_forms_query says the library does with them.  Nothing here touches a GPU.

A case is one encode call of F frames: the mixed material of test_gpu_batch_forms.base_frames (silence, chirps, noise, music at three
levels) spread over the frames by a seeded map, 40 frames at random places (22 of case 4's 45) cut to the lengths of ragged_pool (1, 3, 7, a
layer's order - 1 / + 0 / + 1, block / 2 + 1, ...: at most 15 lengths + the block), and bases 0 .. 4 planted at fixed places so
that silence -- the zero problems of -a, the channel-frames that leave the trainer at once -- stands beside music in every call,
full and ragged.  Frame counts make the channel-frame count CF no multiple of 64 and put it on the side of 64 and 256 the case is
for (the final pass of -a N has one job per channel-frame: lnn_forms.h lev_wave J <= 64, sel_wave J <= 256, k_autocorr_wide
F x C x R <= 64).

   1  -a 2     2 ch MS 16-bit, block 1024, -m 7 (R = 4, 128 taps)   F = 161, CF = 322   final pass above 256 jobs: k_levinson_lds, k_select, k_autocorr2;
                                                                                        two blocks of k_af_best / k_af_init / k_af_finish, six of k_af_pivot / k_af_solve
   2  -a 1     3 ch, 24-bit, every other frame loud, block 1024, -m 3  F = 111, CF = 333   af_Rstride = maxP^2 = 4096 far beyond four channel-frames; k_prep_slow rows in front of -a
   3  -l       2 ch MS 16-bit, block 512, -m 4 (R = 4)              F = 141, CF = 282   tr_job through best[]; k_tr_init over two blocks; silence beside music in one trainer loop
   4  -a 1 -l  2 ch MS 16-bit, block 1024, -m 5                     F = 45,  CF = 90    64 < jobs <= 256 in the final pass (k_levinson_lds with k_select_wave); trainer behind it (best == NULL)
   5  -a 1 -l  1 ch 16-bit, block 1024, -m 0 (layers 2 / 32)        F = 301, CF = 301   L = 2 in the trainer's kernels; the smallest maxP
   6  -a 2     case 1's batch, an arena for ceil(F / 3) + 1 frames: chunks of 54 / 54 / 53 frames
   7  -l       case 3's batch, an arena for ceil(F / 3) + 1 frames: chunks of 47 / 47 / 47 frames (141 = 3 x 47: lnn_call_split evens
               the chunks out, so only case 6 has a smaller last chunk)

There is no eighth case: lnn_call_split keeps a call on one stream unless it has 512 frames per stream, whether LINNE_AMD_STREAMS
is given or not, so LINNE_AMD_STREAMS=2 does not cut a call of 161 frames in two (test_option_batches_cpu asserts it).

The arena of cases 6 and 7 is sized from the scratch bytes per frame WITH the option set.  LINNEAmd_ScratchBytesPerFrame knows the
shape only; lnn_forms_query reports the figure the encode call itself uses (frame_scratch_bytes with -a / -l), so that is asked.
"""
import ctypes as C

import numpy as np

import linne_amd
from test_forms_cpu import CALL_FIELDS, CHUNK_FIELDS, LAYER_FIELDS      # (its import declares lnn_forms_query's argument types)
from test_gpu_batch_forms import OracleBatch, make_batch

lib = linne_amd.lib

NRAGGED = 40
HUGE = 1 << 42
PLANTED = [0, 1, 2, 3, 4, 0, 0, 5, 0]       # bases at fixed places: silence four times (twice on ragged frames), chirps, noise, music


def _case(af, learn, nch, bits, block, preset, ms, F, seed, loud=False, thirds=False, side=(), sel_wave=None):
    return {"af": af, "learn": learn, "nch": nch, "bits": bits, "block": block, "preset": preset, "ms": ms, "F": F, "seed": seed, "loud": loud,
            "thirds": thirds, "side": side, "sel_wave": sel_wave}


# side: CF against the two thresholds of the final pass, as (threshold, "above" | "at most"); sel_wave: what the final pass of the
# whole call must choose (None: no final pass)
CASES = {
    1: _case(2, 0, 2, 16, 1024, 7, True, 161, 101, side=((64, "above"), (256, "above")), sel_wave=0),
    2: _case(1, 0, 3, 24, 1024, 3, False, 111, 102, loud=True, side=((64, "above"), (256, "above")), sel_wave=0),
    3: _case(0, 1, 2, 16, 512, 4, True, 141, 103, side=((64, "above"), (256, "above"))),
    4: _case(1, 1, 2, 16, 1024, 5, True, 45, 104, side=((64, "above"), (256, "at most")), sel_wave=1),
    5: _case(1, 1, 1, 16, 1024, 0, False, 301, 105, side=((64, "above"), (256, "above")), sel_wave=0),
}
CASES[6] = dict(CASES[1], thirds=True)
CASES[7] = dict(CASES[3], thirds=True)
NAMES = {1: "a2-m7-322cf", 2: "a1-m3-24bit-333cf", 3: "l-m4-282cf", 4: "a1-l-m5-90cf", 5: "a1-l-m0-mono-301cf", 6: "a2-m7-three-chunks", 7: "l-m4-three-chunks"}

_BATCHES = {}
CACHE = {}          # the oracle's answers by (shape, settings, length, content), over all cases (OracleBatch's cache)
_ANSWERS = {}


def batch_of(n):
    """the batch of case n (cases 6 and 7: the batch of 1 and 3), built once and left unchanged"""
    c = CASES[n]
    key = (c["nch"], c["bits"], c["block"], c["preset"], c["F"], c["seed"])
    if key not in _BATCHES:
        b = make_batch(c["F"], c["nch"], c["bits"], c["block"], c["preset"], c["seed"], loud_every_other=c["loud"], nragged=min(NRAGGED, c["F"] // 2))
        rng = np.random.default_rng(c["seed"] + 7)
        ragged, full = np.flatnonzero(b["ns"] < c["block"]), np.flatnonzero(b["ns"] == c["block"])
        where = np.concatenate([rng.choice(full, size=len(PLANTED) - 2, replace=False), rng.choice(ragged[b["ns"][ragged] > 128], size=2, replace=False)])
        for f, base in zip(where, PLANTED):
            b["bmap"][f] = base
            b["frames"][f] = b["bases"][base]
            b["frames"][f, :, int(b["ns"][f]):] = 0
        for a in (b["frames"], b["ns"], b["bmap"], b["bases"]):
            a.setflags(write=False)
        _BATCHES[key] = b
    return _BATCHES[key]


def answers(oracle, n, on):
    """the oracle's answers for case n's batch with the case's options (on) or without any (not on), as an OracleBatch"""
    c = CASES[n]
    af, learn = (c["af"], c["learn"]) if on else (0, 0)
    key = (id(batch_of(n)), af, learn)
    if key not in _ANSWERS:
        _ANSWERS[key] = OracleBatch(oracle, batch_of(n), c["ms"], cache=CACHE, af=af, learn=learn)
    return _ANSWERS[key]


def shape_of(n):
    c = CASES[n]
    return linne_amd.Shape(c["nch"], c["bits"], c["block"], c["preset"], int(c["ms"]))


def forms(n, on=True, arena=HUGE, streams=2):
    """lnn_forms_query for case n's call on a context with `streams` compute sub-streams and a side stream (what a context creates
    by default): the call record with ["chunks"] -- per chunk the search passes' record and, with -a N, the final pass's under
    ["final_pass"] --, each with ["layers"]"""
    c = CASES[n]
    af, learn = (c["af"], c["learn"]) if on else (0, 0)
    shape, ns = shape_of(n), np.ascontiguousarray(batch_of(n)["ns"], dtype=np.uint32)
    out = np.zeros(1 << 16, dtype=np.int64)
    got = lib.lnn_forms_query(0, C.byref(shape), ns.ctypes.data, len(ns), arena, streams, 1, af, learn, 1, out.ctypes.data, out.size)
    assert got > 0, "lnn_forms_query refused the call"
    call = dict(zip(CALL_FIELDS, (int(v) for v in out[:16])))
    call["chunks"], at = [], 48
    while at < got:
        rec = dict(zip(CHUNK_FIELDS, (int(v) for v in out[at:at + 16])))
        at += 16
        rec["layers"] = []
        for _ in range(call["L"]):
            rec["layers"].append(dict(zip(LAYER_FIELDS, (int(v) for v in out[at:at + 24]))))
            at += 24
        if rec["final"]:
            call["chunks"][-1]["final_pass"] = rec
        else:
            call["chunks"].append(rec)
    assert at == got and len(call["chunks"]) == call["nchunks"]
    return call


def per_frame(n, on=True):
    """scratch bytes per frame of case n's call, with its options set or without"""
    return forms(n, on)["per_frame"]


def arena_for(n):
    """cases 6 and 7: room for ceil(F / 3) + 1 frames (+ the arena's fixed 64 KiB and one alignment step); the others: the whole
    call in one chunk"""
    c = CASES[n]
    per = per_frame(n)
    if c["thirds"]:
        return per * ((c["F"] + 2) // 3 + 1) + 65536 + 256
    return int(per * c["F"] * 1.02) + (256 << 20)


def long_layer(preset):
    Ls = linne_amd.PRESET_LAYERS[preset]
    return Ls.index(max(Ls))


def final_forms_expected(CF):
    """the final pass of a chunk of CF channel-frames, from the rules as lnn_forms.h states them: (lev_wave, sel_wave)"""
    return int(CF <= 64), int(CF <= 256)
