"""The rule that sends the long layer's order-128 Levinson launch to the chunk's sibling stream beside the short-trial lag kernels
(lnn_forms.h: LnnLayerForms.lev_beside), asked without a GPU through lnn_forms_query.  The expected values are worked out from the
rule as lnn_forms.h states it: the lanes = jobs lag kernels run in the layer, its order is 128, a sibling stream exists, and the
chunk has at least LNN_LEV_BESIDE_MIN = 32 768 jobs; LINNE_AMD_LEV_BESIDE=0/1 replaces the size term."""
import pytest

import test_forms_cpu as tf
from test_forms_cpu import no_knobs  # noqa: F401  (autouse: no LINNE_AMD_* knob leaks in from the environment)

MAXT = tf.MAXT
LAYER_FIELDS = tf.LAYER_FIELDS[:21] + ["lev_beside", "lev_carrier", "carrier_ride"]
MIN_JOBS = 32768


@pytest.fixture(autouse=True)
def layer_fields(monkeypatch):
    monkeypatch.setattr(tf, "LAYER_FIELDS", LAYER_FIELDS)


def long_layer(preset, S, lengths, **kw):
    return [c["layers"][1] for c in tf.encode_forms(preset, S, lengths, **kw)["chunks"]]


def on(layer):
    """the whole of the form: the flag, the launch list (trial 0 bare, the riders with trial 1) and the rider trial index"""
    assert (layer["lev_beside"], layer["lev_carrier"], layer["lev_ride"], layer["carrier_ride"], layer["nlev"]) == (1, 1, MAXT, 4, 4), layer
    return True


def off(layer, nlev=4, ride=4):
    carrier = 0 if ride < MAXT else MAXT        # (MAXT: no trial rides, no launch carries any)
    assert (layer["lev_beside"], layer["lev_carrier"], layer["lev_ride"], layer["carrier_ride"], layer["nlev"]) == (0, carrier, ride, ride, nlev), layer
    return True


def test_on_from_32768_jobs():
    F = MIN_JOBS // 8                    # -m 7 stereo: 8 jobs per frame
    for f, want in ((F - 1, off), (F, on), (F + 1, on)):
        (layer,) = long_layer(7, 10240, [10240] * f)
        assert layer["hist_layer"] == 1 and want(layer), f


def test_each_half_of_a_two_stream_call_is_asked_on_its_own(monkeypatch):
    """two streams: 8192 frames are halves of 32 768 jobs, both on; one frame fewer and the call keeps one stream (lnn_call_split), a
    single chunk of 65 528 jobs, on; forced onto two streams, 4096 + 4095 frames are a half at the threshold and a half below it"""
    assert [l["lev_beside"] for l in long_layer(7, 10240, [10240] * 8192, streams=2)] == [1, 1]
    assert [l["lev_beside"] for l in long_layer(7, 10240, [10240] * 8191, streams=2)] == [1]
    monkeypatch.setenv("LINNE_AMD_STREAMS", "2")
    assert [l["lev_beside"] for l in long_layer(7, 10240, [10240] * 8191, streams=-1)] == [1, 0]


def test_off_for_a_layer_of_order_64(monkeypatch):
    """-m 2: layers 4 / 64 / 8, two jobs per stereo frame; an order-64 solver block is 67 KB and needs no help -- not even the knob turns it on"""
    (layer,) = long_layer(2, 10240, [10240] * (2 * MIN_JOBS // 2))
    assert layer["hist_layer"] == 1 and layer["lev_beside"] == 0 and layer["lev_carrier"] == 0
    monkeypatch.setenv("LINNE_AMD_LEV_BESIDE", "1")
    (layer,) = long_layer(2, 10240, [10240] * (2 * MIN_JOBS // 2))
    assert layer["lev_beside"] == 0 and layer["lev_carrier"] == 0


def test_needs_the_lanes_are_jobs_lag_kernels_not_every_frame_theirs(monkeypatch):
    """the condition chosen is hist_layer, not hist_all: a ragged tail's lags come from the general kernel on the same sibling stream,
    in front of the solver, so the chunk keeps the form; without the lanes = jobs kernels (LINNE_AMD_HIST=0) there is nothing to run beside"""
    F = MIN_JOBS // 8
    (layer,) = long_layer(7, 10240, [10240] * F + [9280])
    assert (layer["hist_layer"], layer["hist_all"], layer["beside"]) == (1, 0, 1) and on(layer)
    monkeypatch.setenv("LINNE_AMD_HIST", "0")
    (layer,) = long_layer(7, 10240, [10240] * F)
    assert layer["hist_layer"] == 0 and off(layer)


def test_needs_a_sibling_stream():
    (layer,) = long_layer(7, 10240, [10240] * (MIN_JOBS // 8), side=0)
    assert off(layer)


def test_knob_forces_both_ways(monkeypatch):
    F = MIN_JOBS // 8
    monkeypatch.setenv("LINNE_AMD_LEV_BESIDE", "0")
    assert off(long_layer(7, 10240, [10240] * (4 * F))[0])
    monkeypatch.setenv("LINNE_AMD_LEV_BESIDE", "1")
    monkeypatch.setenv("LINNE_AMD_HIST", "1")
    assert on(long_layer(7, 10240, [10240] * 17)[0]), "136 jobs"
    assert on(long_layer(7, 4096, [4096] * 16)[0])
    layer = long_layer(7, 10240, [10240] * 8)[0]
    assert layer["lev_wave"] == 1 and layer["lev_beside"] == 0, "64 jobs: a wave per problem, one launch"
    monkeypatch.setenv("LINNE_AMD_LEV_RIDE", "0")
    assert off(long_layer(7, 10240, [10240] * 17)[0], nlev=MAXT, ride=MAXT), "no riders to move: a launch per trial as before"


def test_the_other_layers_never_take_it(monkeypatch):
    monkeypatch.setenv("LINNE_AMD_LEV_BESIDE", "1")
    monkeypatch.setenv("LINNE_AMD_HIST", "1")
    c = tf.encode_forms(7, 10240, [10240] * 17)["chunks"][0]
    assert [l["lev_beside"] for l in c["layers"]] == [0, 1, 0] and [l["lev_carrier"] for l in c["layers"]] == [0, 1, 0]
    fin = tf.encode_forms(7, 10240, [10240] * 17, af=1)["chunks"][1]
    assert fin["final"] == 1 and [l["lev_beside"] for l in fin["layers"]] == [0, 0, 0], "the final pass of -a N runs the general kernels"


def test_a_forced_two_stream_call_has_the_form_in_both_halves(monkeypatch):
    """the shape tests/test_gpu_lev_beside.py runs on two streams: 1023 frames of 4096 samples and a ragged one, LINNE_AMD_STREAMS=2"""
    for name, v in (("STREAMS", "2"), ("HIST", "1"), ("LEV_BESIDE", "1")):
        monkeypatch.setenv("LINNE_AMD_" + name, v)
    call = tf.encode_forms(7, 4096, [4096] * 1023 + [3000], streams=-1)
    assert (call["nsub"], call["use_sub"], call["nchunks"]) == (2, 1, 2)
    assert [on(c["layers"][1]) for c in call["chunks"]] == [True, True]
    assert [c["layers"][1]["beside"] for c in call["chunks"]] == [0, 1], "the ragged frame sorts into the second half"
