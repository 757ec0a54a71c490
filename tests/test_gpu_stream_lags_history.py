"""GPU test that a lag_windows call's answer does not depend on the calls its context served before it (tests/lag_history.py holds the
scenarios, written as tests/stream_history.py writes its lists): every lags step is held to lag_refs on the oracle's decode, element
for element, on ONE context per scenario, among measure, quiet, mix, resample, overlay and relate calls."""
import numpy as np
import pytest

import lag_history as lh
from lag_refs import expected_lags
from stream_history import material

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mat(oracle):
    return material(oracle)


def run(mat, steps):
    import torch
    import linne_amd
    ctx = linne_amd.Context(0)
    dev = {name: torch.from_numpy(np.frombuffer(mat.data[name], dtype=np.uint8).copy()).cuda() for name in lh.NAMES}
    idx = dict(zip(lh.NAMES, ctx.index_streams([dev[name] for name in lh.NAMES])))
    try:
        for k, s in enumerate(steps):
            where = (k, s["call"], s["note"])
            if s["call"] == "lags":
                got = ctx.lag_windows([(dev[a], idx[a], fa, n, dev[b], idx[b], fb, lf, L, pairs) for a, fa, n, b, fb, lf, L, pairs in s["probes"]], group_frames=s["gf"])
                for i, (t, (a, fa, n, b, fb, lf, L, pairs)) in enumerate(zip(got, s["probes"])):
                    want, a_sq = expected_lags(mat.full[a], fa, n, mat.full[b], fb, lf, L, pairs)
                    assert np.array_equal(t.cpu(), want), where + (i,)
                    assert np.array_equal(t.a_sq.cpu().numpy().view(np.uint64), a_sq), where + (i,)
                continue
            wins = [(dev[name], idx[name], first, n) for name, first, n in s["wins"]]
            if s["call"] == "measure":
                ctx.measure_windows(wins, bucket_samples=441, group_frames=s["gf"])
            elif s["call"] == "quiet":
                ctx.quiet_windows(wins, 40, group_frames=s["gf"])
            elif s["call"] == "relate":
                ctx.relate_windows(wins, bucket_samples=7, group_frames=s["gf"])
            elif s["call"] == "mix":
                for w, (name, _, _) in zip(wins, s["wins"]):          # (a matrix has its stream's channel count)
                    m, shift = linne_amd.downmix_matrix(lh.CHANNELS[name])
                    ctx.mix_windows([w], m, shift=shift, group_frames=s["gf"])
            elif s["call"] == "resample":
                ctx.resample_windows([(d, x, first // 2, n // 2) for d, x, first, n in wins], 3, 2, group_frames=s["gf"])
            elif s["call"] == "overlay":
                ctx.overlay_windows([(2000, [(d, x, first, n, 7 * j, 1 + j) for j, (d, x, first, n) in enumerate(wins)])], group_frames=s["gf"])
            else:
                raise AssertionError(s["call"])
    finally:
        for x in idx.values():
            x.close()
        ctx.close()


def test_lags_between_its_siblings(mat):
    steps = lh.scenario_between()
    assert [s["call"] for s in steps[1::2]] == lh.SIBLINGS and all(s["call"] == "lags" for s in steps[0::2])
    run(mat, steps)


def test_large_small_large(mat):
    run(mat, lh.scenario_large_small_large())
