"""Every trial mean the search kernels hand to k_select / k_select_wave, against the oracle's mean of the same trial (-m gpu).

The certified unit-count search rests on one premise: each mean of the kernels' order-free sums lies within
rel * m_ref + slack of the reference's ordered mean (tests/search_means.py has the formulas; tests/test_search_means_cpu.py shows
that the interval holds a correct evaluation and reports a wrong one).  The other GPU tests see only the argmin, and on music the
runner-up is per cent away: a kernel that is off by 1e-6 passes them all.  Here LINNEAmd_SetSearchCapture records what the selection
kernels decided from, and per (frame, channel, regulariser pass, layer, trial):

  searches the certificate decided, and the certified side of those it refused
      the captured mean lies in the interval, rel and slack computed here from the oracle's na, np, max |input| and coefficient norms;
      the captured max |input| equals the oracle's bit for bit; the captured coefficient norm is within np 2^-52 relative of it (the
      kernels add the np magnitudes in other orders: lnn_k_search.h), hence the device's slack is no smaller than the oracle's less
      that rounding; the captured rel is the formula's
  searches the exact chains decided (k_fir2<0> after a refusal or under LINNE_AMD_EXACT=1, k_last_layer)
      the captured ordered mean equals the oracle's mean bit for bit; every search of a silent frame is one of these
  bookkeeping
      one record per trial the reference evaluates and none else; the argmin of the captured means is the oracle's winner of that
      pass and, for the winning pass, the unit count in the parameter record; with the capture off the call gives the same residual,
      parameters, statistics, fallback count, margin and launches

tests/search_means.py lists the cases and what each has to show through LINNEAmd_GetLastTimingLaunches (kinds 25, 5, 15, 18, 20, 7, 6)
and LINNEAmd_GetLastSearchLongForm: k_search_long<128> and <64> in their three forms, k_fir2<2> on ragged frames (a job_off run
between two lengths k_search_long takes), short blocks, with and without the fused forward, k_fir_small<2 / 4 / 8 / 16> as layer 0
and as the last layer, k_last_layer, both selection kernels, 8 / 16 / 24-bit material, 1 / 2 / 8 channels, odd unit lengths (3001
samples: units of 47), two chunks, two streams, and lengths that alternate in the caller's order.  The last test prints the smallest
bound / |m_gpu - m_ref| seen per kernel form (DESIGN.md section 6 quotes it); nothing is asserted on it beyond the bound.
"""
import ctypes

import numpy as np
import pytest

import linne_amd
import search_means as sm
from linne_amd import CAP_HOW, CAP_HSUM, CAP_MEAN, CAP_ORDERED, CAP_REL, CAP_SLACK, CAP_UNITS, CAP_XMAX

pytestmark = pytest.mark.gpu

KINDS = (1, 5, 6, 7, 15, 18, 20, 25)
_cache, _headroom = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _encode(ctx_env, sig, env, frames, ns, arena, capture):
    from test_gpu_batch_forms import scratch_for
    full = scratch_for(sig["nch"], sig["bits"], sig["block"], sig["preset"], sig["ms"], len(ns))
    with ctx_env(env, scratch_bytes=full if arena is None else int((full - (256 << 20)) * arena)) as c:
        shape = c.shape(sig["nch"], sig["bits"], sig["block"], sig["preset"], sig["ms"])
        c.enable_timing(True)
        c.set_search_capture(capture)
        res, prm, st = c.encode_frames_host(shape, frames, ns)
        fn = linne_amd.lib.LINNEAmd_GetLastSearchLongForm
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
        tele = {"launches": {k: c.last_launches(k) for k in KINDS}, "form": int(fn(c.h)), "fallbacks": c.last_fallback_count(), "margin": c.last_min_margin()}
        cap = c.last_search_capture(shape, len(ns)) if capture else None
        if not capture:
            assert int(linne_amd.lib.LINNEAmd_GetLastSearchCapture(c.h, None, 0)) == 0, "records without the capture"
        return res, prm, st, tele, cap


def _label(sig, env, exp, tele, l, s):
    """the kernel that produced the certified means of layer l for a frame of analysis length s["n"] (lnn_device.hip's launch rules)"""
    layers = linne_amd.PRESET_LAYERS[sig["preset"]]
    P, last = layers[l], l + 1 == len(layers)
    spec = env.get("LINNE_AMD_SPECULATE", "1") != "0" and not last
    if l == 0:
        return f"k_fir_small<{P}> layer 0"
    if last:
        return f"k_fir_small<{P}> last layer" if P <= 16 else f"k_fir2<2> last layer, {P} taps"
    full = len(s["units"]) == min(P, 128).bit_length()
    if spec and P in (64, 128) and full and s["n"] % 2048 == 0:
        form = "one pass" if env.get("LINNE_AMD_SEARCH_TWO", "1") == "0" else ("two passes, per job" if tele["form"] == 1 else "two passes, (jobs, tiles)")
        return f"k_search_long<{P}> {form}"
    return f"k_fir2<2> {P} taps" + (", fused forward" if spec else "")


@pytest.mark.parametrize("case", sm.CASES, ids=sm.CASE_IDS)
def test_captured_trial_means_against_the_oracles(ctx_env, oracle, case):
    name, sig, F, lens, env, exp = case
    frames, ns, bmap = sm.build_batch(sig, F, lens)
    _, silent, constant = sm.bases_of(sig)
    res, prm, st, tele, cap = _encode(ctx_env, sig, env, frames, ns, exp.get("arena"), True)
    layers, R, C = linne_amd.PRESET_LAYERS[sig["preset"]], linne_amd.PRESET_NUM_REGULARS[sig["preset"]], sig["nch"]
    print(f"{name}: launches {tele['launches']}, k_search_long form {tele['form']}, {tele['fallbacks']} exact fallbacks, min margin {tele['margin']:.3e}")

    # ---- the forms this case is here for did run
    for k in exp["kinds"]:
        assert tele["launches"][k] >= 1, f"kind {k} was not launched: {tele['launches']}"
    for k in exp.get("absent", ()):
        assert tele["launches"][k] <= 0, f"kind {k} was launched: {tele['launches']}"
    if "form" in exp:
        assert tele["form"] == exp["form"], f"k_search_long form {tele['form']}, expected {exp['form']}"
    chunks = tele["launches"][1]
    assert chunks >= exp.get("chunks", 1), f"{chunks} chunk(s)"
    if "chunks" not in exp:
        assert chunks == 1
    jobs = -(-F // chunks) * C * R                           # (chunks are of equal size: lnn_device.hip)
    assert (jobs <= 256) == (exp["decider"] == "wave"), f"{jobs} jobs per chunk: not the selection kernel this case is for"

    # ---- the capture changes nothing
    r0, p0, s0, t0, _ = _encode(ctx_env, sig, env, frames, ns, exp.get("arena"), False)
    assert np.array_equal(r0, res) and np.array_equal(p0, prm) and np.array_equal(s0, st, equal_nan=True), "the capture changed the encode"
    assert t0 == tele, f"the capture changed the telemetry: {t0} / {tele}"

    # ---- per trial against the oracle
    runs = sm.oracle_searches(oracle, sig, frames, ns, bmap, _cache)
    nrec, how_count, flagged_const = 0, {0: 0, 1: 0, 2: 0}, {}
    for f in range(F):
        tap, ores, tr = runs[(int(bmap[f]), int(ns[f]))]
        assert np.array_equal(res[f][:, :int(ns[f])], ores), f"frame {f}: residual differs from the oracle"
        for ch in range(C):
            for r in range(R):
                for l, P in enumerate(layers):
                    s, rec, where = tr[ch][r][l], cap[f, ch, r, l], f"{name}: frame {f} (base {bmap[f]}, n {ns[f]}) channel {ch} pass {r} layer {l}"
                    nt = len(s["units"])
                    nrec += nt
                    assert np.array_equal(rec[:nt, CAP_UNITS], s["units"]), f"{where}: trials {rec[:, CAP_UNITS]}, the oracle's {s['units']}"
                    assert np.isnan(rec[nt:]).all(), f"{where}: a record beyond the last trial"
                    how = rec[:nt, CAP_HOW]
                    assert (how == how[0]).all() and how[0] in (0.0, 1.0, 2.0), f"{where}: decided by {how}"
                    how = int(how[0])
                    how_count[how] += 1
                    if "how" in exp:
                        assert how == exp["how"], f"{where}: decided by {how}"
                    if l + 1 == len(layers) and "last_how" in exp:
                        assert how == exp["last_how"], f"{where}: decided by {how}"
                    if int(bmap[f]) == silent:
                        assert how != 0, f"{where}: a search of a silent frame was certified"
                    if int(bmap[f]) == constant and how != 0:
                        flagged_const[f] = flagged_const.get(f, 0) + 1
                    if how in (0, 1):
                        m = rec[:nt, CAP_MEAN]
                        bad = sm.violations(m, s)
                        assert not bad, f"{where}: certified means outside the interval: (trial, |m_gpu - m_ref|, bound) {bad}; gpu {m}, oracle {s['mean']}"
                        assert np.array_equal(_bits(rec[:nt, CAP_XMAX]), _bits(s["xmax"])), f"{where}: max |x| {rec[:nt, CAP_XMAX]} / {s['xmax']}"
                        np_ = P / s["units"].astype(np.float64)
                        assert (np.abs(rec[:nt, CAP_HSUM] - s["hmax"]) <= np_ * 2.0 ** -52 * s["hmax"]).all(), f"{where}: coefficient norms {rec[:nt, CAP_HSUM]} / {s['hmax']}"
                        assert (rec[:nt, CAP_REL] == sm.rel_of(s["n"])).all(), f"{where}: rel {rec[:nt, CAP_REL]}"
                        want = np.array([sm.slack_of(a, x, h) for a, x, h in zip(np_, s["xmax"], s["hmax"])])
                        assert (rec[:nt, CAP_SLACK] >= want * (1.0 - np_ * 2.0 ** -52 - 2.0 ** -50)).all(), f"{where}: slack {rec[:nt, CAP_SLACK]} below the oracle-derived {want}"
                        lab = _label(sig, env, exp, tele, l, s)
                        _headroom[lab] = min(_headroom.get(lab, np.inf), sm.headroom(m, s))
                    else:
                        assert np.isnan(rec[:nt, :CAP_HOW]).all(), f"{where}: certified-side words on k_last_layer's path"
                    if how == 0:
                        assert np.isnan(rec[:nt, CAP_ORDERED]).all(), f"{where}: an ordered mean on a certified search"
                        decided = rec[:nt, CAP_MEAN]
                    else:
                        assert np.array_equal(_bits(rec[:nt, CAP_ORDERED]), _bits(s["mean"])), f"{where}: ordered means {rec[:nt, CAP_ORDERED]}, the oracle's {s['mean']}"
                        decided = rec[:nt, CAP_ORDERED]
                    win = int(s["units"][int(np.argmin(decided))])            # (np.argmin: the first minimum = strict < from the left)
                    assert win == int(s["units"][int(np.argmin(s["mean"]))]), f"{where}: the captured means choose {win} units"
                    if r == int(tap.ch[ch].best_pass):
                        assert win == int(prm[f, ch, linne_amd.PRM_UNITS + l]) == int(tap.ch[ch].num_units[l]), f"{where}: {win} units, the record has {prm[f, ch, linne_amd.PRM_UNITS + l]}"
    assert int(np.count_nonzero(~np.isnan(cap[..., CAP_UNITS]))) == nrec, "records that belong to no trial of the reference"
    if constant is not None:
        nconst = int(np.count_nonzero(bmap == constant))
        assert len(flagged_const) == nconst, f"constant frames with a flagged search: {sorted(flagged_const)} of {nconst}"
    assert tele["fallbacks"] == how_count[1], f"{how_count[1]} searches took the exact fallback, the call counted {tele['fallbacks']}"
    print(f"{name}: {nrec} trial records; searches decided by the certificate / the exact fallback / k_last_layer: {how_count[0]} / {how_count[1]} / {how_count[2]}")


def test_headroom_per_kernel_form():
    """printed, not asserted: the smallest bound / |m_gpu - m_ref| per kernel form over the cases above"""
    for lab in sorted(_headroom):
        print(f"headroom {lab:50s} {_headroom[lab]:10.1f}")
