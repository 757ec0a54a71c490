"""GPU test that a project_windows call's answer does not depend on the calls its context served before it (tests/project_history.py
holds the scenarios, written as tests/stream_history.py writes its lists): every project step is held to project_refs on the oracle's
decode, element for element, on ONE context per scenario, among measure, quiet, mix, resample, overlay and lag calls."""
import numpy as np
import pytest

import project_history as ph
from project_refs import expected_project
from stream_history import material

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mat(oracle):
    return material(oracle)


def run(mat, steps):
    import torch
    import linne_amd
    ctx = linne_amd.Context(0)
    bases = ph.bases()
    dev = {name: torch.from_numpy(np.frombuffer(mat.data[name], dtype=np.uint8).copy()).cuda() for name in ph.NAMES}
    idx = dict(zip(ph.NAMES, ctx.index_streams([dev[name] for name in ph.NAMES])))
    try:
        for k, s in enumerate(steps):
            where = (k, s["call"], s["note"])
            if s["call"] == "project":
                b, hop, before, shift, clip, f32, rows_first = s["spec"]
                groups = {}
                for name, first, n in s["wins"]:
                    groups.setdefault((ph.CHANNELS[name], n), []).append((name, first, n))
                for members in groups.values():
                    got, sat = ctx.project_windows([(dev[name], idx[name], first, n) for name, first, n in members], bases[b], hop, before=before, shift=shift, clip_bits=clip,
                                                   dtype=torch.float32 if f32 else torch.int32, float_exp=31 if f32 else 0, rows_first=rows_first, group_frames=s["gf"], return_saturated=True)
                    got = got.cpu().numpy()
                    for i, (name, first, n) in enumerate(members):
                        want, wsat = expected_project(mat.full[name], first, n, bases[b], hop, before, shift, clip, f32, 31 if f32 else 0)
                        assert np.array_equal(got[i].view(np.uint32), np.ascontiguousarray(want.transpose(0, 2, 1) if rows_first else want).view(np.uint32)) and sat[i] == wsat, where + (name, first, n)
                continue
            if s["call"] == "lags":
                ctx.lag_windows([(dev[a], idx[a], fa, n, dev[b], idx[b], fb, lf, L, pairs) for a, fa, n, b, fb, lf, L, pairs in s["probes"]], group_frames=s["gf"])
                continue
            wins = [(dev[name], idx[name], first, n) for name, first, n in s["wins"]]
            if s["call"] == "measure":
                ctx.measure_windows(wins, bucket_samples=441, group_frames=s["gf"])
            elif s["call"] == "quiet":
                ctx.quiet_windows(wins, 40, group_frames=s["gf"])
            elif s["call"] == "mix":
                for w, (name, _, _) in zip(wins, s["wins"]):          # (a matrix has its stream's channel count)
                    m, shift = linne_amd.downmix_matrix(ph.CHANNELS[name])
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


def test_project_between_its_siblings(mat):
    steps = ph.scenario_between()
    assert [s["call"] for s in steps[1::2]] == ph.SIBLINGS and all(s["call"] == "project" for s in steps[0::2])
    run(mat, steps)


def test_large_small_large(mat):
    run(mat, ph.scenario_large_small_large())
