"""The interval the certified unit-count search is held to, checked without a GPU (tests/search_means.py states it).

3a  The reference's own ordered means lie inside the interval around an independent, effectively exact evaluation of the same trials
    (terms in longdouble from the oracle's layer inputs and coefficients, summed by math.fsum) -- on every input of
    tests/test_gpu_search_means.py, before a GPU sees them.  This is the half of the argument that does not depend on any kernel: the
    interval is wide enough for a correct evaluation.
3b  It is narrow enough to catch a wrong one: the comparison routine reports the oracle's means with one term left out of one trial,
    with the coefficients of two adjacent units swapped for 8 samples, and scaled by 1 + 1e-9 -- stand-ins for a search kernel that
    drops a sample at a tile seam, reads a neighbouring unit's coefficients, or sums a little too much -- on every search of every
    music input.
"""
import numpy as np
import pytest

import search_means as sm

_cache = {}
SIGNALS = {}
for _name, _sig, _F, _lens, _env, _exp in sm.CASES:
    SIGNALS.setdefault(sm.sig_key(_sig), (_sig, []))[1].append((_F, _lens))


def _inputs(oracle, sig, batches):
    """every distinct (frame, length) the GPU cases of this signal use -> {(base, n): (tap, residual, searches)} with layer data"""
    out = {}
    for F, lens in batches:
        frames, ns, bmap = sm.build_batch(sig, F, lens)
        out.update(sm.oracle_searches(oracle, sig, frames, ns, bmap, _cache, with_data=True))
    return out


def _searches(runs):
    for (base, n), (tap, res, tr) in sorted(runs.items()):
        for ch, passes in enumerate(tr):
            for ps, layers in enumerate(passes):
                for l, s in enumerate(layers):
                    yield (base, n, ch, ps, l), s


@pytest.mark.parametrize("key", list(SIGNALS), ids=[f"m{dict(k)['preset']}_{dict(k)['nch']}ch_{dict(k)['bits']}bit_{dict(k)['block']}" for k in SIGNALS])
def test_the_reference_means_lie_inside_the_interval_around_the_exact_ones(oracle, key):
    sig, batches = SIGNALS[key]
    runs = _inputs(oracle, sig, batches)
    nsearch, worst = 0, np.inf
    for where, s in _searches(runs):
        exact = sm.exact_means(s)
        # the tap's own bookkeeping, recomputed: the interval's inputs are what the test thinks they are
        assert s["xmax"][0] == np.max(np.abs(s["input"])) and len(s["input"]) == s["n"]
        for t, u in enumerate(s["units"]):
            hm = max(np.sum(np.abs(s["coef"][t][un * (s["P"] // u):(un + 1) * (s["P"] // u)])) for un in range(u))
            assert abs(hm - s["hmax"][t]) <= s["P"] * 2.0 ** -52 * hm
        bad = sm.violations(s["mean"], s, ref_means=exact)
        assert not bad, f"{where}: the reference's mean lies outside the interval around the exact one: (trial, |diff|, bound) {bad}"
        d = np.abs(s["mean"].astype(np.longdouble) - exact)
        b = sm.bounds_of(s, exact)
        if (d > 0).any():
            worst = min(worst, float(np.min(b[d > 0] / d[d > 0])))
        nsearch += 1
    print(f"{nsearch} searches, smallest bound / |m_oracle - m_exact| = {worst:.1f}")
    assert nsearch


def _perturbed(s, which):
    """the oracle's means of one search with one of the three faults"""
    m = s["mean"].copy()
    n, P = s["n"], s["P"]
    if which == "dropped term":                 # the largest term of the one-unit trial is missing from its sum
        terms = sm.exact_terms(s["input"], s["coef"][0], 1)
        m[0] -= float(np.max(terms)) / n
    elif which == "neighbour's coefficients":   # the two-unit trial: the first 8 samples of unit 1 take unit 0's coefficients
        t = 1
        assert s["units"][t] == 2
        h = s["coef"][t]
        good = sm.exact_terms(s["input"], h, 2)
        wrong = sm.exact_terms(s["input"], np.concatenate([h[:P // 2], h[:P // 2]]), 2)
        k = slice(n // 2, n // 2 + 8)
        m[t] += float(np.sum(wrong[k] - good[k])) / n
    else:
        m = m * (1.0 + 1e-9)
    return m


@pytest.mark.parametrize("which", ["dropped term", "neighbour's coefficients", "scaled by 1 + 1e-9"])
def test_the_comparison_reports_a_perturbed_mean(oracle, which):
    """on every search of every music input of the two 16-bit stereo signals (-m 7 and -m 3) the fault is reported; the silent and the
    constant frames are left out (their means are zero or nearly so: there is nothing to perturb)"""
    hit = 0
    for sig in (sm.SIG7, sm.SIG3):
        frames, ns, bmap = sm.build_batch(sig, 7, sm.MIX)
        music = {k: v for k, v in sm.oracle_searches(oracle, sig, frames, ns, bmap, _cache, with_data=True).items() if k[0] < sig["nmusic"]}
        assert len(music) >= 4
        for where, s in _searches(music):
            assert not sm.violations(s["mean"], s), f"{where}: the unperturbed means are reported"
            bad = sm.violations(_perturbed(s, which), s)
            assert bad, f"{where}: '{which}' was not reported"
            hit += 1
    print(f"'{which}': reported on {hit} of {hit} searches")
