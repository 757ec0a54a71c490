"""The large-batch kernel forms against the oracle, on every preset family, at the batch sizes that pick them BY THEMSELVES (-m gpu).

EncodeFramesDevice and DecodeFramesDevice choose their kernel forms by batch size (lnn_device.hip, the rules at the chunk loop and
in DecodeFramesDevice).  Each case below builds one batch that the rules send through the forms it names, with nothing forced, and
checks it on both sides against the oracle, frame by frame:

* encode: the product's residual, parameters and statistics of EVERY frame equal the oracle's hot path of that frame
  (libs/linne_encoder/src/linne_encoder.c:594-752), and the residual behind a ragged frame's end is zero;
* decode: the oracle's own residual and parameters, tiled over the whole batch, decode to the oracle's own synthesis (which is the
  input), and the sentinel behind a ragged frame's end stays; then the product's own encode output decodes to the input as well;
* the forms ran: the launch counts of the call (include/linne_amd.h, LINNEAmd_GetLastTimingMs) are those the rules give for the
  batch.  A moved threshold fails the case instead of letting it test something else.

A batch is B = 97 distinct base frames of mixed material (music, music at a third and at three times its level, chirps, white noise,
one silent frame) spread over the frames by a seeded random map, so that neighbouring rows of a block hold different content and
the unit counts and best regularisers differ between the lanes of a wave; about 200 frames at random places are ragged, with
lengths from a small pool.  The oracle runs once per distinct (base, length).  Frame counts are chosen so that the channel-frame
count is not a multiple of 64 (and of 8 or 4 where the channel count allows): the last block of every row kernel is partial.
"""
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import linne_amd
from signals import music, waveform
from test_gpu_parity import _check_taps, _params_from_tap

pytestmark = pytest.mark.gpu

B = 97                          # distinct base frames per case (a prime: the map from frames to bases has no period)
NRAGGED = 200
SENTINEL = -123456
GIB = 1 << 30


# ---------------------------------------------------------------------------------------------------------------------------------
# host restatements of the class rules the launch decisions go by (lnn_device.hip make_class, lnn_dev_common.h hist_takes /
# search_long_takes, the k_fwd_loss / k_last_layer tests at the chunk loop): used to build batches whose forms have work to do

def analysis_length(n, preset, block):
    na = ((n + 7) // 8) * 8                                     # linne_encoder.c:652-654
    na = max(na, max(linne_amd.PRESET_LAYERS[preset]))
    return min(na, block)


def trial_count(P, na):
    return sum(1 for u in (1 << k for k in range(8)) if u <= min(P, 128) and P % u == 0 and na % u == 0)


def all_trials(P):
    return sum(1 for u in (1 << k for k in range(8)) if u <= min(P, 128))


def hist_takes(n, preset, block, layer):
    P, na = linne_amd.PRESET_LAYERS[preset][layer], analysis_length(n, preset, block)
    nt = all_trials(P)
    return P >= 64 and trial_count(P, na) == nt and na % (16 << (nt - 1)) == 0 and (na >> (nt - 1)) >= 32 and block % 4 == 0


def search_long_takes(n, preset, block, layer):
    Ls, na = linne_amd.PRESET_LAYERS[preset], analysis_length(n, preset, block)
    P = Ls[layer]
    return 0 < layer < len(Ls) - 1 and P in (64, 128) and trial_count(P, na) == all_trials(P) and na % 2048 == 0


def last_layer_keeps(n, preset, block):
    """k_fwd_loss takes the frame (analysis length a multiple of 4 x the last layer's order) and every trial of the last layer is
    present: a ragged frame that fails this turns k_last_layer off for its whole chunk"""
    Ls, na = linne_amd.PRESET_LAYERS[preset], analysis_length(n, preset, block)
    return na % (4 * Ls[-1]) == 0 and trial_count(Ls[-1], na) == all_trials(Ls[-1])


def ragged_pool(preset, block, keep_last_layer=False):
    """1, a few samples, a layer's order -1 / +0 / +1, block / 2 + 1, block - 3 and a few more; at most 15 lengths + the block"""
    Ls = linne_amd.PRESET_LAYERS[preset]
    cand = [1, 3, 7, Ls[0] + 1, Ls[1] - 1, Ls[1], Ls[1] + 1, block // 2 + 1, block - 3, 777, block // 2, 3 * block // 4 - 8, 2 * Ls[1] + 1, 1000, 63, 127]
    pool = []
    for n in cand:
        if 0 < n < block and n not in pool and (not keep_last_layer or last_layer_keeps(n, preset, block)):
            pool.append(n)
    return np.array(pool[:15], dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# batches

def base_frames(nch, bits, block, seed):
    """[B][C][block]: 0 silence, 1-2 chirp (full and a third), 3-4 white noise, the rest 'music' at 1, 1/3 and 3x (clipped) level.
    Returns the bases and the indices of the loud (3x) ones."""
    hi, lo = (1 << (bits - 1)) - 1, -(1 << (bits - 1))
    out = np.zeros((B, nch, block), dtype=np.int32)
    loud = []
    chirp = waveform("chirp", nch, block, bits, seed=seed)
    out[1], out[2] = chirp, np.trunc(chirp / 3.0).astype(np.int32)
    out[3] = waveform("white_noise", nch, block, bits, seed=seed + 1)
    out[4] = waveform("white_noise", nch, block, bits, seed=seed + 2) // 8
    for b in range(5, B):
        x = music(nch, block, bits, seed=seed * 1000 + b).astype(np.int64)
        k = b % 3
        if k == 1:
            x = np.trunc(x / 3.0).astype(np.int64)
        elif k == 2:
            x = np.clip(3 * x, lo, hi)
            loud.append(b)
        out[b] = x
    return out, np.array(loud)


def make_batch(F, nch, bits, block, preset, seed, keep_last_layer=False, loud_every_other=False, nragged=NRAGGED):
    rng = np.random.default_rng(seed)
    bases, loud = base_frames(nch, bits, block, seed)
    bmap = rng.integers(0, B, size=F)
    if loud_every_other:
        bmap[1::2] = rng.choice(loud, size=len(bmap[1::2]))
    ns = np.full(F, block, dtype=np.uint32)
    pool = ragged_pool(preset, block, keep_last_layer)
    where = rng.choice(F, size=nragged, replace=False)
    ns[where] = rng.choice(pool, size=nragged)
    ns[where[:len(pool)]] = pool                                # every length of the pool occurs
    assert len(set(ns.tolist())) <= 16, "an encode call takes up to 16 distinct frame lengths"
    frames = bases[bmap]
    for f in np.flatnonzero(ns < block):
        frames[f, :, int(ns[f]):] = 0
    return {"frames": np.ascontiguousarray(frames), "ns": ns, "bases": bases, "bmap": bmap, "nch": nch, "bits": bits, "block": block, "preset": preset}


class OracleBatch:
    """the oracle's hot path for every distinct (base, length) of a batch, and its own synthesis of its output; .key[f] indexes
    the per-key arrays for frame f"""

    def __init__(self, oracle, batch, ms, cache=None, af=0, learn=0):
        """cache: a dict that keeps the oracle's answers by (shape, settings, length, content) over many batches; af, learn: the
        oracle's -a N / -l settings"""
        nch, bits, block, preset = batch["nch"], batch["bits"], batch["block"], batch["preset"]
        pairs = np.stack([batch["bmap"], batch["ns"].astype(np.int64)], axis=1)
        keys, self.key = np.unique(pairs, axis=0, return_inverse=True)
        self.key = self.key.reshape(-1)
        K = len(keys)
        self.res = np.zeros((K, nch, block), dtype=np.int32)
        self.dec = np.full((K, nch, block), SENTINEL, dtype=np.int32)
        self.prm = np.zeros((K, nch, linne_amd.PARAM_WORDS), dtype=np.int32)
        self.r0, self.loss, self.tail = (np.zeros((K, nch)) for _ in range(3))
        self.best = np.zeros((K, nch), dtype=np.int64)
        self.taps = [None] * K

        def one(k):
            b, n = int(keys[k][0]), int(keys[k][1])
            x = batch["bases"][b][:, :n]
            ck = (nch, bits, block, preset, bool(ms), af, learn, n, hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest())
            if cache is not None and ck in cache:
                return (k, n) + cache[ck]
            enc = oracle.encoder(nch, bits, 44100, block, preset, ms, af_iters=af)
            oracle.L.oracle_encoder_set_learning(enc.h, learn)
            tap, r = enc.hotpath(x)
            enc.close()
            d = oracle.decode_hotpath([tap.ch[ch] for ch in range(nch)], r, bits, block, preset, ms)
            assert np.array_equal(d, x), f"base {b}, n = {n}: the oracle's own round trip"
            if cache is not None:
                cache[ck] = (tap, r, d)
            return k, n, tap, r, d

        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            for k, n, tap, r, d in ex.map(one, range(K)):
                self.taps[k] = tap
                self.res[k, :, :n] = r
                self.dec[k, :, :n] = d
                self.prm[k] = _params_from_tap(tap, preset, nch)
                for ch in range(nch):
                    t = tap.ch[ch]
                    self.r0[k, ch], self.best[k, ch], self.loss[k, ch], self.tail[k, ch] = t.est_r0, t.best_pass, t.pass_loss[t.best_pass], t.parcor_tail


def param_words(preset):
    """the words of a parameter record the oracle defines (_check_taps's)"""
    Ls = linne_amd.PRESET_LAYERS[preset]
    w = np.zeros(linne_amd.PARAM_WORDS, dtype=bool)
    w[0:4] = True
    w[4:4 + len(Ls)] = True
    w[7:7 + len(Ls)] = True
    w[10:10 + sum(Ls)] = True
    return w


def _first(bad, k=8):
    return [int(f) for f in np.flatnonzero(bad)[:k]]


def check_encode(ob, batch, res, prm, st, where):
    """every frame of the product's encode output against the oracle; on a difference _check_taps names the first field"""
    preset, nch, ns = batch["preset"], batch["nch"], batch["ns"]
    block = batch["block"]
    key = ob.key
    behind = np.zeros(res.shape[0], dtype=bool)
    for f in np.flatnonzero(ns < block):
        behind[f] = res[f, :, int(ns[f]):].any()
    assert not behind.any(), f"{where}: residual behind the end of {int(behind.sum())} ragged frames (first {_first(behind)})"
    w = param_words(preset)
    bad_p = np.zeros(len(ns), dtype=bool)
    bad_s = np.zeros(len(ns), dtype=bool)
    bad_r = np.zeros(len(ns), dtype=bool)
    for a in range(0, len(ns), 2048):                           # (in slices: the expected residual of a whole batch is large)
        sl = slice(a, min(a + 2048, len(ns)))
        k = key[sl]
        bad_r[sl] = (res[sl] != ob.res[k]).any(axis=(1, 2))
        bad_p[sl] = (prm[sl][:, :, w] != ob.prm[k][:, :, w]).any(axis=(1, 2))
        r0 = st[sl][:, :, linne_amd.ST_R0]
        ok = ((r0 == ob.r0[k]) | (np.isnan(r0) & np.isnan(ob.r0[k])))
        ok &= st[sl][:, :, linne_amd.ST_BEST].astype(np.int64) == ob.best[k]
        ok &= st[sl][:, :, linne_amd.ST_LOSS] == ob.loss[k]
        ok &= st[sl][:, :, linne_amd.ST_TAIL] == ob.tail[k]
        bad_s[sl] = ~ok.all(axis=1)
    bad = bad_p | bad_s | bad_r
    if bad.any():
        f = int(np.flatnonzero(bad)[0])
        head = (f"{where}: the product's encode differs from the oracle in {int(bad.sum())} of {len(ns)} frames (parameters {int(bad_p.sum())}, "
                f"statistics {int(bad_s.sum())}, residual {int(bad_r.sum())}; first {_first(bad)}, their lengths {[int(ns[g]) for g in _first(bad)]})")
        _check_taps(ob.taps[key[f]], prm[f], st[f], preset, nch, f"{head}; frame {f} n={int(ns[f])}")
        pytest.fail(f"{head}; frame {f}: residual")


def check_variety(batch, prm, st, R):
    """the batch did vary between lanes: more than one unit count in some layer, more than one best regulariser when R > 1"""
    nl = len(linne_amd.PRESET_LAYERS[batch["preset"]])
    units = prm[:, :, 4:4 + nl]
    assert any(len(np.unique(units[:, :, l])) > 1 for l in range(nl)), "every frame chose the same unit counts: the divergent-lane paths went untested"
    if R > 1:
        assert len(np.unique(st[:, :, linne_amd.ST_BEST])) > 1, "every frame chose the same regulariser"


def marked(x, ns, block):
    y = x.copy()
    for f in np.flatnonzero(ns < block):
        y[f, :, int(ns[f]):] = SENTINEL
    return y


def check_decode(dec, want, ns, block, where):
    if np.array_equal(dec, want):
        return
    own = np.zeros(len(ns), dtype=bool)
    tail = np.zeros(len(ns), dtype=bool)
    for f in range(len(ns)):
        n = int(ns[f])
        own[f] = not np.array_equal(dec[f, :, :n], want[f, :, :n])
        tail[f] = not np.array_equal(dec[f, :, n:], want[f, :, n:])
    pytest.fail(f"{where}: {int(own.sum())} frames decode to other samples (first {_first(own)}, lengths {[int(ns[g]) for g in _first(own)]}); "
                f"{int(tail.sum())} frames had samples behind their end written (first {_first(tail)})")


ENCODE_KINDS = (1, 3, 13, 18, 20, 21, 22, 23, 25)
DECODE_KINDS = (11, 12, 30, 31, 32, 33, 34, 35, 36)


def run_case(ctx_env, oracle, batch, ms, env, scratch, enc_kinds, dec_kinds):
    """encode (nothing forced) -> every frame against the oracle; decode of the oracle's output -> the oracle's synthesis; decode of
    the product's output -> the input; the launch counts of both calls as the rules give them for this batch"""
    for v in os.environ:
        assert not v.startswith("LINNE_AMD_"), f"{v} is set: these cases run the rules as they stand"
    nch, bits, block, preset = batch["nch"], batch["bits"], batch["block"], batch["preset"]
    frames, ns = batch["frames"], batch["ns"]
    ob = OracleBatch(oracle, batch, ms)
    with ctx_env(env, scratch_bytes=scratch) as c:
        shape = c.shape(nch, bits, block, preset, ms)
        c.enable_timing(True)
        res, prm, st = c.encode_frames_host(shape, frames, ns)
        enc = {k: c.last_launches(k) for k in ENCODE_KINDS}
        dec_o = c.decode_frames_host(shape, marked(ob.res[ob.key], ns, block), ob.prm[ob.key], ns)
        dec = {k: c.last_launches(k) for k in DECODE_KINDS}
        dec_p = c.decode_frames_host(shape, marked(res, ns, block), prm, ns)
    print(f"encode launches {enc}; decode launches {dec}; {len(np.unique(ob.key))} oracle runs")
    check_encode(ob, batch, res, prm, st, "encode")
    check_variety(batch, prm, st, linne_amd.PRESET_NUM_REGULARS[preset])
    want = ob.dec[ob.key]
    for f in np.flatnonzero(ns < block):
        want[f, :, int(ns[f]):] = SENTINEL
    check_decode(dec_o, want, ns, block, "decode of the oracle's residual and parameters")
    check_decode(dec_p, marked(frames, ns, block), ns, block, "decode of the product's own encode output")
    # last: which forms ran (the values above are checked first, so that a wrong result is reported as such)
    for k, v in enc_kinds.items():
        assert enc[k] == v, f"encode: {v} launches of kind {k} expected, {enc[k]} ran ({enc})"
    for k, v in dec_kinds.items():
        assert dec[k] == v, f"decode: {v} launches of kind {k} expected, {dec[k]} ran ({dec})"
    return res, prm, st, ob


def scratch_for(nch, bits, block, preset, ms, frames):
    """an arena that holds the whole call in one chunk per stream"""
    per = int(linne_amd.lib.LINNEAmd_ScratchBytesPerFrame(__import__("ctypes").byref(linne_amd.Shape(nch, bits, block, preset, int(ms)))))
    assert per > 0
    return int(per * frames * 1.02) + (256 << 20)


# kinds (include/linne_amd.h): 1 k_prep (one span per chunk), 3 the long layer's general lag kernel, 13 k_stats / k_stats_rows,
# 18 the last layer's certified search (k_fir_small; absent when k_last_layer takes the chunk), 20 k_fwd_loss_mw / k_fwd_loss /
# k_last_layer, 21 / 22 / 23 k_autocorr_hist<P, 0> / <P, 1> / k_autocorr_sub, 25 k_search_long; decode: 33 k_synth_rows<1|3|7> (a long
# layer), 36 k_synth_rows<0> / k_synth_rows8 (a short layer), 35 k_synth_l0_de, 34 k_deemph_lr, 12 k_ms_to_lr, 11 / 30 / 31 / 32 the
# other forms.  Every case runs k_stats_rows (kind 13: F x C >= 1024, far past) and the throughput decode (F x C >= 1536).
NO_OTHER_DECODE = {11: 0, 12: 0, 30: 0, 31: 0, 32: 0, 34: 0}


def test_preset2_mono_the_once_red_batch(ctx_env, oracle):
    """20 557 mono 16-bit frames of 1024 samples at -m 2 (layers 4 / 64 / 8, one regulariser): the batch of the once-red run of
    test_decode_throughput_forms_at_the_batch_sizes_that_pick_them[2-1-16].  J = 20 557: k_autocorr_hist<64, 0> and k_autocorr_sub<64>
    are launched (J >= 12 288) and the general lag kernel serves, beside them, the rows they do not take -- at 1024 samples every row
    (hist_takes needs an analysis length of 2048 for P = 64) --, no k_fwd_loss (J < 24 576), k_fir_small for the short layers.
    Decode: CF = 20 557 >= 20 480 picks k_synth_rows8<8> for the last layer (kind 36; 77 channel-frames past the threshold: this is
    that batch), k_synth_rows<3> for the long one, k_synth_l0_de<false> with 13 rows in its last block (20 557 = 64 x 321 + 13)."""
    F, nch, bits, block, preset, ms = 20557, 1, 16, 1024, 2, False
    batch = make_batch(F, nch, bits, block, preset, seed=21)
    run_case(ctx_env, oracle, batch, ms, {}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 1, 3: 1, 13: 1, 18: 1, 20: 0, 21: 1, 22: 0, 23: 1, 25: 0},
             {33: 1, 35: 1, 36: 1, **NO_OTHER_DECODE})


def test_preset3_8bit_stereo_fwd_loss_mw(ctx_env, oracle):
    """6 203 stereo 8-bit frames of 2048 samples, MS, at -m 3 (layers 4 / 64 / 8, two regularisers): J = 24 812.  k_fwd_loss_mw<8> for the
    last layer (kind 20 with the certified search, kind 18, beside it: 24 576 <= J < 65 536 picks the five-wave form, 40 000 jobs short
    of the one-wave form), k_autocorr_hist<64> / k_autocorr_sub<64> with work to do (an analysis length of 2048 samples: full frames),
    the general lag kernel beside them for the ragged frames, k_search_long<64> for the full frames.  Decode: CF = 12 406 < 20 480 keeps
    four channel-frames per wave for the short layer (k_synth_rows<0>), k_synth_rows<3>, k_synth_l0_de<true> (MS -> LR fused)."""
    F, nch, bits, block, preset, ms = 6203, 2, 8, 2048, 3, True
    batch = make_batch(F, nch, bits, block, preset, seed=31)
    assert sum(hist_takes(int(n), preset, block, 1) for n in batch["ns"]) > F // 2
    assert sum(search_long_takes(int(n), preset, block, 1) for n in batch["ns"]) > F // 2
    run_case(ctx_env, oracle, batch, ms, {}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 1, 3: 1, 13: 1, 18: 1, 20: 1, 21: 1, 22: 0, 23: 1, 25: 1},
             {33: 1, 35: 1, 36: 1, **NO_OTHER_DECODE})


def test_preset4_last_layer_eight_taps_on_two_streams(ctx_env, oracle):
    """12 301 stereo 16-bit frames of 1024 samples, MS, at -m 4 (layers 4 / 64 / 8, four regularisers): J = 98 408, cut by default into
    two chunks of 6 151 / 6 150 frames over the two compute streams (each >= 32 768 jobs), and each chunk of >= 49 152 jobs whose frames
    all keep every trial of the last layer goes to k_last_layer<8> (kind 20, no kind 18).  The ragged lengths are chosen to keep every
    trial.  Decode: CF = 24 602 >= 20 480: k_synth_rows8<8>, k_synth_rows<3>, k_synth_l0_de<true>."""
    F, nch, bits, block, preset, ms = 12301, 2, 16, 1024, 4, True
    batch = make_batch(F, nch, bits, block, preset, seed=41, keep_last_layer=True)
    assert all(last_layer_keeps(int(n), preset, block) for n in batch["ns"])
    run_case(ctx_env, oracle, batch, ms, {}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 2, 3: 2, 13: 1, 18: 0, 20: 2, 21: 2, 22: 0, 23: 2, 25: 0},
             {33: 1, 35: 1, 36: 1, **NO_OTHER_DECODE})


def test_preset5_loud_24bit_long_frames(ctx_env, oracle):
    """6 203 stereo 24-bit frames of 4096 samples, MS, at -m 5 (layers 4 / 128 / 16, one regulariser), every other frame loud: J = 12 406.
    k_autocorr_hist<128, 0 / 1> and k_autocorr_sub<128> with work to do (full frames: an analysis length of 4096), k_search_long<128>
    (a multiple of the 2048-sample tile), no k_fwd_loss (J < 24 576), and k_prep_slow over dozens of blocks: the pre-emphasis sums of
    loud 24-bit rows are not exact integers (k_prep lists them; k_prep_slow shares kind 1 with it, so the batch's loudness is asserted
    instead: thousands of its rows fail k_prep's exact-sum test).  Decode: CF = 12 406: k_synth_rows<0> for the 16-tap layer, k_synth_rows<7>, k_synth_l0_de<true>."""
    F, nch, bits, block, preset, ms = 6203, 2, 24, 4096, 5, True
    batch = make_batch(F, nch, bits, block, preset, seed=51, loud_every_other=True)
    x = batch["frames"].astype(np.int64)
    side = x[:, 1] - x[:, 0]                                    # MS as the encoder forms it (linne_encoder.c: ms_conversion)
    mid = x[:, 0] + (side >> 1)
    loud = sum(int(((y * y).sum(axis=1) >= (1 << 53)).sum()) for y in (mid, side))        # k_prep's test: sum x^2 < 2^53 or not exact
    assert loud >= 64 * 24, f"{loud} channel-frames for k_prep_slow: fewer than its dozens of blocks"
    assert sum(hist_takes(int(n), preset, block, 1) for n in batch["ns"]) > F // 2
    run_case(ctx_env, oracle, batch, ms, {}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 1, 3: 1, 13: 1, 18: 1, 20: 0, 21: 1, 22: 1, 23: 1, 25: 1},
             {33: 1, 35: 1, 36: 1, **NO_OTHER_DECODE})


def test_preset7_eight_channels_fwd_loss_mw(ctx_env, oracle):
    """1 603 frames of eight 24-bit channels of 1024 samples, MS, at -m 7 (layers 4 / 128 / 16, four regularisers): J = 51 296, one stream
    (a half would hold fewer than 32 768 jobs).  k_fwd_loss_mw<16> (kind 20 beside kind 18: J < 65 536, 14 000 jobs short of the one-wave
    form), k_autocorr_hist<128> launched (taking no row at 1024 samples).  Decode: CF = 12 824 < 20 480: k_synth_rows<0>, k_synth_rows<7>,
    k_synth_l0_de<true> over eight channels."""
    F, nch, bits, block, preset, ms = 1603, 8, 24, 1024, 7, True
    batch = make_batch(F, nch, bits, block, preset, seed=71)
    run_case(ctx_env, oracle, batch, ms, {}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 1, 3: 1, 13: 1, 18: 1, 20: 1, 21: 1, 22: 1, 23: 1, 25: 0},
             {33: 1, 35: 1, 36: 1, **NO_OTHER_DECODE})


def test_preset7_fwd_loss_one_wave_per_64_jobs(ctx_env, oracle):
    """9 001 stereo 16-bit frames of 1024 samples, MS, at -m 7: J = 72 008.  k_fwd_loss<16> -- one wave per 64 jobs -- is what a chunk of
    65 536 <= J < 81 920 jobs takes on one stream (kind 20 beside kind 18; 6 472 jobs past the five-wave form's limit, 9 912 short of
    k_last_layer's).  LINNE_AMD_STREAMS=1 keeps the call in one chunk: by default it would be cut into two halves of 36 004 jobs, which
    take k_fwd_loss_mw.  Decode: CF = 18 002 < 20 480: k_synth_rows<0>, k_synth_rows<7>, k_synth_l0_de<true>."""
    F, nch, bits, block, preset, ms = 9001, 2, 16, 1024, 7, True
    batch = make_batch(F, nch, bits, block, preset, seed=72)
    run_case(ctx_env, oracle, batch, ms, {"LINNE_AMD_STREAMS": "1"}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 1, 3: 1, 13: 1, 18: 1, 20: 1, 21: 1, 22: 1, 23: 1, 25: 0},
             {33: 1, 35: 1, 36: 1, **NO_OTHER_DECODE})


def test_preset7_last_layer_sixteen_taps_on_two_streams(ctx_env, oracle):
    """12 301 stereo 16-bit frames of 1024 samples, MS, at -m 7: two chunks of >= 49 152 jobs over the two compute streams, each taken
    whole by k_last_layer<16> (kind 20, no kind 18); ragged lengths that keep every trial.  Decode: CF = 24 602: k_synth_rows8<16>,
    k_synth_rows<7>, k_synth_l0_de<true>."""
    F, nch, bits, block, preset, ms = 12301, 2, 16, 1024, 7, True
    batch = make_batch(F, nch, bits, block, preset, seed=73, keep_last_layer=True)
    assert all(last_layer_keeps(int(n), preset, block) for n in batch["ns"])
    run_case(ctx_env, oracle, batch, ms, {}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 2, 3: 2, 13: 1, 18: 0, 20: 2, 21: 2, 22: 2, 23: 2, 25: 0},
             {33: 1, 35: 1, 36: 1, **NO_OTHER_DECODE})


def test_preset1_three_channels_general_lag_kernels(ctx_env, oracle):
    """7 001 frames of three 16-bit channels of 1024 samples, no MS, at -m 1 (layers 2 / 32, two regularisers): J = 42 006, one stream.
    A 32-tap long layer has no lanes = jobs form: the general lag kernels over a grid of 21 003 channel-frames, no k_fwd_loss (its
    forms take last layers of <= 16 taps).  Decode: CF = 21 003: k_synth_rows<1> for the 32-tap layer, k_synth_l0_de<false> for layer 0
    (two taps: no k_synth_rows8 is left to run) over three channels."""
    F, nch, bits, block, preset, ms = 7001, 3, 16, 1024, 1, False
    batch = make_batch(F, nch, bits, block, preset, seed=11)
    run_case(ctx_env, oracle, batch, ms, {}, scratch_for(nch, bits, block, preset, ms, F),
             {1: 1, 3: 1, 13: 1, 18: 1, 20: 0, 21: 0, 22: 0, 23: 0, 25: 0},
             {33: 1, 35: 1, 36: 0, **NO_OTHER_DECODE})


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole-stream path's narrow staging: <= 16-bit PCM travels as int16, 17-24-bit PCM as packed 3-byte samples (lnn_api.c
# fill_frames); only through them do k_stats_rows<*, 1 | 2> and k_prep's narrow loads run

def default_group_frames(num_frames, nch, block, regs):
    """lnn_api.c default_group for an encode: frames per staging slot (one device call each)"""
    want = (30720 + nch * regs - 1) // (nch * regs)
    cap = GIB // (nch * block * 4) + 1
    n = max(256, min(want, cap))
    if n >= num_frames:
        return num_frames
    ngroups = num_frames // n
    return (num_frames + ngroups - 1) // ngroups


@pytest.mark.parametrize("bits", [16, 24])
def test_whole_stream_narrow_staging_at_large_groups(product, oracle, bits):
    """EncodeWhole of one stereo stream of 6 203 frames of 1024 samples + a 555-sample tail at -m 0 (cheap for the oracle): one group of
    12 408 jobs (>= 12 288) staged as int16 (16-bit) or as packed 3-byte samples (24-bit).  The .lnn bytes equal the oracle's and
    DecodeWhole restores the input."""
    for v in os.environ:
        assert not v.startswith("LINNE_AMD_"), v
    nch, block, preset = 2, 1024, 0
    F = 6204
    x = music(nch, (F - 1) * block + 555, bits, seed=600 + bits)
    x[:, 3 * block:4 * block] = np.clip(3 * x[:, 3 * block:4 * block].astype(np.int64), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    g = default_group_frames(F, nch, block, linne_amd.PRESET_NUM_REGULARS[preset])
    assert g == F and g * nch * linne_amd.PRESET_NUM_REGULARS[preset] >= 12288
    mine = product.encode_whole(x, bits, 44100, block, preset, True)
    assert mine == oracle.encode_whole(x, bits, 44100, block, preset, True)
    ret, dec = product.decode_whole(mine)
    assert ret == 0 and np.array_equal(dec, x)
