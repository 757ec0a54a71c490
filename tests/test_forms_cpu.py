"""The launch rules of linne_amd/csrc/lnn_forms.h, asked without a GPU through lnn_forms_query / lnn_classes_replay (test exports of
liblinne_amd.so, like lnn_preset_info): every size boundary as the value below it and the values one frame either side, the class
tests of the lanes = jobs kernels on a ragged tail, every forcing knob, and the class bookkeeping of tests/call_history.py's
scenarios through the real code.  Stereo, presets 2 (layers 4 / 64 / 8, one regulariser: 2 jobs per frame) and 7 (4 / 128 / 16,
four regularisers: 8 jobs per frame), blocks of 2048 and 10240 samples.  The expected values are worked out from the rules as
lnn_forms.h states them, never read back from the code."""
import ctypes as C

import numpy as np
import pytest

import call_history as ch
import linne_amd

lib = linne_amd.lib
lib.lnn_forms_query.restype = C.c_int64
lib.lnn_forms_query.argtypes = [C.c_int, C.POINTER(linne_amd.Shape), C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                C.c_int, C.c_void_p, C.c_uint64]
lib.lnn_classes_replay.restype = C.c_int64
lib.lnn_classes_replay.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]

CALL_FIELDS = ["branch", "nlen", "na_max", "prod_ok", "nsub", "use_sub", "chunk", "part_bytes", "nchunks", "stats_rows", "per_frame", "L",
               "streams_forced", "_13", "_14", "_15"]
CHUNK_FIELDS = ["f0", "Fc", "J", "final", "fwd_loss_on", "fuse_cfg", "fuse_all", "last_layer_all", "prep_defer", "hist", "chain_sum", "chain_sum_wave",
                "cascade_walk", "runs_mixed", "nruns", "present"]
LAYER_FIELDS = ["fir_spec", "hist_layer", "hist_all", "beside", "lev_wave", "nlev", "lev_ride", "last_layer", "long_any", "long_all", "search_form",
                "fir_small", "sel_wave", "fwd_loss", "fwd_loss_mw", "forward", "forward_walk", "nleft", "left_first", "left_frames", "long_mask",
                "_21", "_22", "_23"]
MAXCLS, MAXT = 16, 8
BRANCH = ["first", "reuse", "append", "restart by shape", "restart by overflow"]       # lnn_forms.h LNN_CLS_*
DEC_LAYERS, DEC_WAVE, DEC_PIPE = 0, 1, 2
DL_FUSED_L0, DL_ROWS, DL_ROWS8, DL_SMALL, DL_BIG, DL_GENERAL = range(6)
HUGE = 1 << 42          # an arena that never cuts a call into chunks
ONE = 0                 # a context without compute sub-streams (LINNE_AMD_STREAMS=1 when it was created)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    import os
    for v in list(os.environ):
        if v.startswith("LINNE_AMD_") and v != "LINNE_AMD_LIB":
            monkeypatch.delenv(v)


def encode_forms(preset, S, lengths, arena=HUGE, streams=ONE, side=1, af=0, learn=0):
    """the call record, with ["chunks"]: chunk records, each with ["layers"]"""
    shape = linne_amd.Shape(2, 16, S, preset, 1)
    ns = np.ascontiguousarray(lengths, dtype=np.uint32)
    out = np.zeros(1 << 16, dtype=np.int64)
    n = lib.lnn_forms_query(0, C.byref(shape), ns.ctypes.data, len(ns), arena, streams, side, af, learn, 1, out.ctypes.data, out.size)
    assert n > 0, "lnn_forms_query refused the call"
    call = dict(zip(CALL_FIELDS, (int(v) for v in out[:16])))
    call["lens"] = [int(v) for v in out[16:16 + call["nlen"]]]
    call["slots"] = [int(v) for v in out[32:32 + call["nlen"]]]
    call["chunks"], at = [], 48
    while at < n:
        c = dict(zip(CHUNK_FIELDS, (int(v) for v in out[at:at + 16])))
        at += 16
        c["layers"] = []
        for _ in range(call["L"]):
            c["layers"].append(dict(zip(LAYER_FIELDS, (int(v) for v in out[at:at + 24]))))
            at += 24
        call["chunks"].append(c)
    assert at == n
    return call


def one_chunk(preset, S, F, **kw):
    call = encode_forms(preset, S, [S] * F, **kw)
    assert call["nchunks"] == 1 and call["chunks"][0]["Fc"] == F
    return call["chunks"][0]


def decode_forms(preset, S, F, aligned=1):
    shape = linne_amd.Shape(2, 16, S, preset, 1)
    out = np.zeros(64, dtype=np.int64)
    n = lib.lnn_forms_query(1, C.byref(shape), None, F, 0, 0, 0, 0, 0, aligned, out.ctypes.data, out.size)
    nl = len(linne_amd.PRESET_LAYERS[preset])
    assert n == 2 + 5 * nl
    return {"call": int(out[0]), "ms_separate": int(out[1]),
            "layers": [dict(zip(["form", "nch", "pb", "de", "ms_fold"], (int(v) for v in out[2 + 5 * l:7 + 5 * l]))) for l in range(nl)]}


JOBS = {2: 2, 7: 8}     # jobs per stereo frame


def frames_for(preset, jobs):
    assert jobs % JOBS[preset] == 0
    return jobs // JOBS[preset]


# ---------------------------------------------------------------------------------------------------------------------------------
# encode: size boundaries

@pytest.mark.parametrize("preset,S", [(7, 2048), (2, 10240)])
def test_fwd_loss_from_24576_jobs(preset, S):
    F = frames_for(preset, 24576)
    for f, want in ((F - 1, 0), (F, 1), (F + 1, 1)):
        c = one_chunk(preset, S, f)
        assert (c["fwd_loss_on"], c["fuse_cfg"], c["fuse_all"]) == (want,) * 3, f
        assert c["chain_sum"] == 1 - want and c["layers"][-1]["fwd_loss"] == want and c["layers"][-1]["forward"] == 1 - want, f


@pytest.mark.parametrize("preset,S", [(7, 10240), (2, 2048)])
def test_autocorr_hist_from_12288_jobs(preset, S):
    F = frames_for(preset, 12288)
    for f, want in ((F - 1, 0), (F, 1), (F + 1, 1)):
        c = one_chunk(preset, S, f)
        assert c["hist"] == want and [l["hist_layer"] for l in c["layers"]] == [0, want, 0], f
        assert [l["hist_all"] for l in c["layers"]] == [0, want, 0] and c["layers"][1]["beside"] == 0, "full frames are all k_autocorr_hist's"


def test_autocorr_hist_leaves_short_blocks_to_the_general_kernel():
    """2048 samples in 128 units are 16 per unit, less than a weight tile: at -m 7 no frame of a 2048-sample block is k_autocorr_hist's,
    and the general kernel runs beside it on the side stream (on the chunk's own stream when there is none)"""
    c = one_chunk(7, 2048, 1536)
    assert c["hist"] == 1 and c["layers"][1]["hist_layer"] == 1 and c["layers"][1]["hist_all"] == 0 and c["layers"][1]["beside"] == 1
    assert one_chunk(7, 2048, 1536, side=0)["layers"][1]["beside"] == 0


def test_autocorr_hist_is_off_when_runs_are_mixed(monkeypatch):
    monkeypatch.setenv("LINNE_AMD_SORT", "0")
    monkeypatch.setenv("LINNE_AMD_HIST", "1")
    c = encode_forms(7, 2048, [2048, 777] * 9)["chunks"][0]
    assert c["runs_mixed"] == 1 and c["nruns"] == 1 and c["hist"] == 0
    c = encode_forms(7, 2048, [2048, 777] * 8)["chunks"][0]
    assert c["runs_mixed"] == 0 and c["nruns"] == 16 and c["hist"] == 1, "sixteen runs still fit"
    monkeypatch.setenv("LINNE_AMD_SORT", "1")
    c = encode_forms(7, 2048, [2048, 777] * 9)["chunks"][0]
    assert c["runs_mixed"] == 0 and c["nruns"] == 2 and c["hist"] == 1


PAIRS = [(2, 2048), (2, 10240), (7, 2048), (7, 10240)]


@pytest.mark.parametrize("preset,S", PAIRS)
def test_last_layer_from_81920_jobs_alone(preset, S):
    F = frames_for(preset, 81920)
    for f, want in ((F - 1, 0), (F, 1), (F + 1, 1)):
        c = one_chunk(preset, S, f)
        last = c["layers"][-1]
        assert c["last_layer_all"] == want and last["last_layer"] == want, f
        assert last["fwd_loss"] == 1 - want and c["fuse_all"] == 1 and last["forward"] == 0, f
        assert [l["last_layer"] for l in c["layers"][:-1]] == [0, 0]


def test_last_layer_from_49152_jobs_with_sub_streams():
    """two streams: the halves of 12 287 frames are 6 144 and 6 143 frames, 49 152 and 49 144 jobs"""
    for F, want in ((12286, [0, 0]), (12287, [1, 0]), (12288, [1, 1])):
        call = encode_forms(7, 2048, [2048] * F, streams=2)
        assert call["nsub"] == 2 and call["use_sub"] == 1 and call["nchunks"] == 2
        assert [c["last_layer_all"] for c in call["chunks"]] == want, F
        assert [c["J"] for c in call["chunks"]] == [8 * ((F + 1) // 2), 8 * (F - (F + 1) // 2)]


@pytest.mark.parametrize("preset,below,above", [(7, 32, 33), (2, 128, 129)])
def test_last_layer_2_from_257_jobs(monkeypatch, preset, below, above):
    """(stereo job counts are even: 256 and the first count above it)"""
    monkeypatch.setenv("LINNE_AMD_LAST_LAYER", "2")
    monkeypatch.setenv("LINNE_AMD_FWD_LOSS", "1")
    assert one_chunk(preset, 2048, below)["J"] == 256 and one_chunk(preset, 2048, below)["last_layer_all"] == 0
    assert one_chunk(preset, 2048, above)["last_layer_all"] == 1
    monkeypatch.setenv("LINNE_AMD_LAST_LAYER", "1")
    assert one_chunk(preset, 2048, above)["last_layer_all"] == 0


@pytest.mark.parametrize("preset,S", PAIRS)
def test_fwd_loss_mw_below_65536_jobs(preset, S):
    F = frames_for(preset, 65536)
    for f, want in ((F - 1, 1), (F, 0), (F + 1, 0)):
        last = one_chunk(preset, S, f)["layers"][-1]
        assert last["fwd_loss"] == 1 and last["fwd_loss_mw"] == want, f


def test_statistics_rows_form_from_1024_channel_frames():
    for preset in (2, 7):
        for S in (2048, 10240):
            assert [encode_forms(preset, S, [S] * F)["stats_rows"] for F in (511, 512, 513)] == [0, 1, 1]
    assert encode_forms(7, 2050, [2050] * 512)["stats_rows"] == 0, "rows that are no whole 16-byte groups"
    assert encode_forms(0, 2048, [2048] * 512)["stats_rows"] == 1, "a layer 0 of two taps"


@pytest.mark.parametrize("preset", [2, 7])
def test_small_batch_wave_forms(preset):
    """Levinson wave up to 64 jobs, select wave up to 256, chain-sum wave up to 1024"""
    for jobs, field, per_layer in ((64, "lev_wave", True), (256, "sel_wave", True), (1024, "chain_sum_wave", False)):
        F = frames_for(preset, jobs)
        for f, want in ((F - 1, 1), (F, 1), (F + 1, 0)):
            c = one_chunk(preset, 10240, f)
            if per_layer:
                assert [l[field] for l in c["layers"]] == [want] * 3, (field, f)
            else:
                assert c["chain_sum"] == 1 and c[field] == want, (field, f)


def test_levinson_launch_list():
    """beyond 64 jobs: the trials of a 128-tap layer need 64 x (2 x 128 + 3) doubles of LDS for the one-unit trial (132 608 bytes of 163 840); three problem sets
    of order 8 (16 units, trial 4: 3 x 9 728 bytes) are the first that fit beside it: trials 0 .. 3 are launched, the rest ride"""
    c = one_chunk(7, 2048, 9)
    lds = lambda n: 8 * 64 * (2 * n + 3)
    assert [t for t in range(1, 8) if lds(128) + 3 * lds(128 >> t) <= 160 * 1024][0] == 4
    assert (c["layers"][1]["lev_wave"], c["layers"][1]["nlev"], c["layers"][1]["lev_ride"]) == (0, 4, 4)
    assert (c["layers"][0]["nlev"], c["layers"][0]["lev_ride"]) == (1, 1), "a four-tap layer: everything rides with the one-unit trial"


@pytest.mark.parametrize("preset,S", PAIRS)
def test_cascade_grid_from_1024_channel_frames(preset, S):
    assert [one_chunk(preset, S, f)["cascade_walk"] for f in (511, 512, 513)] == [0, 1, 1]


@pytest.mark.parametrize("preset,S", PAIRS)
def test_forward_pass_walks_tiles_from_4096_jobs(preset, S):
    F = frames_for(preset, 4096)
    for f, want in ((F - 1, 0), (F, 1), (F + 1, 1)):
        c = one_chunk(preset, S, f)
        assert [l["forward_walk"] for l in c["layers"]] == [want, want, 0], "the last layer's search writes no one-unit forward: its pass has every job"


def test_per_job_search_from_8_jobs():
    assert [one_chunk(2, 2048, F)["layers"][1]["search_form"] for F in (3, 4, 5)] == [1, 2, 2]
    c = one_chunk(7, 2048, 1)
    assert c["J"] == 8 and c["layers"][1]["search_form"] == 2 and c["layers"][1]["long_any"] == 1 and c["layers"][1]["long_all"] == 1


def test_two_streams_by_default_need_1024_frames_and_32768_jobs_per_half(monkeypatch):
    for preset, F in ((7, 8192), (2, 32768)):                   # halves of 32 768 jobs
        assert [encode_forms(preset, 2048, [2048] * f, streams=2)["nsub"] for f in (F - 1, F, F + 1)] == [1, 2, 2]
    call = encode_forms(7, 2048, [2048] * 8191, streams=2)
    assert call["use_sub"] == 0 and call["nchunks"] == 1
    monkeypatch.setenv("LINNE_AMD_STREAMS", "2")                # forced: only the 512 frames per stream remain
    got = [encode_forms(7, 2048, [2048] * f, streams=-1) for f in (1023, 1024, 1025)]
    assert [g["nsub"] for g in got] == [1, 2, 2] and [g["streams_forced"] for g in got] == [1, 1, 1]
    assert [g["use_sub"] for g in got] == [1, 1, 1], "a forced stream count forks even a single chunk off the caller's stream"
    monkeypatch.setenv("LINNE_AMD_STREAMS", "1")
    assert encode_forms(7, 2048, [2048] * 8192, streams=-1)["use_sub"] == 0


def test_chunks_are_even_and_a_multiple_of_the_stream_count():
    call = encode_forms(2, 2048, [2048] * 39 + [777], arena=0)
    per = call["per_frame"]
    assert per == lib.LINNEAmd_ScratchBytesPerFrame(C.byref(linne_amd.Shape(2, 16, 2048, 2, 1)))
    call = encode_forms(2, 2048, [2048] * 39 + [777], arena=5 * per + 65536 + 256)
    assert (call["chunk"], call["nchunks"]) == (5, 8) and [c["Fc"] for c in call["chunks"]] == [5] * 8
    call = encode_forms(2, 2048, [2048] * 41, arena=6 * per + 65536 + 256)
    assert (call["chunk"], call["nchunks"]) == (6, 7), "41 frames in 7 chunks of 6 (the last holds 5)"
    assert [c["Fc"] for c in call["chunks"]] == [6] * 6 + [5]


@pytest.mark.parametrize("preset", [2, 7])
def test_autocorr_wide_up_to_64_rows(preset):
    F = frames_for(preset, 64)
    assert [encode_forms(preset, 2048, [2048] * f)["prod_ok"] for f in (F - 1, F, F + 1)] == [0b111, 0b111, 0b101]


# ---------------------------------------------------------------------------------------------------------------------------------
# encode: a ragged tail the lanes = jobs kernels do not take

@pytest.mark.parametrize("tail_first", [False, True])
def test_ragged_tail_fails_every_class_test(tail_first):
    """777 samples: an analysis length of 784 = 16 x 49.  Not whole 2048-sample tiles (k_search_long), five of eight trials of the
    128-tap layer (k_autocorr_hist), not a multiple of 4 x 16 (k_fwd_loss)"""
    F = 3100
    ns = [777] + [10240] * F if tail_first else [10240] * F + [777]
    call = encode_forms(7, 10240, ns)
    c = call["chunks"][0]
    assert call["lens"] == ([777, 10240] if tail_first else [10240, 777]) and call["slots"] == [0, 1] and c["present"] == 0b11
    assert c["J"] == 8 * (F + 1) >= 24576 and (c["fwd_loss_on"], c["fuse_cfg"], c["fuse_all"], c["chain_sum"]) == (1, 1, 0, 1)
    assert c["layers"][2]["fwd_loss"] == 1 and c["layers"][2]["forward"] == 1, "k_fwd_loss for the frames it takes, the two-kernel form for the tail"
    long = c["layers"][1]
    assert (c["hist"], long["hist_layer"], long["hist_all"], long["beside"]) == (1, 1, 0, 1)
    assert (long["long_any"], long["long_all"]) == (1, 0)
    assert (long["nleft"], long["left_first"], long["left_frames"]) == (1, 0 if tail_first else F, 1), "the sorted chunk: one run, where the tail's class lies"
    assert long["long_mask"] == (0b10 if tail_first else 0b01)
    full = encode_forms(7, 10240, [10240] * (F + 1))["chunks"][0]
    assert (full["fuse_all"], full["layers"][1]["hist_all"], full["layers"][1]["long_all"], full["layers"][1]["nleft"]) == (1, 1, 1, 0)


def test_unsorted_tails_leave_one_run_each(monkeypatch):
    monkeypatch.setenv("LINNE_AMD_SORT", "0")
    ns = [2048, 2048, 777, 2048, 1001, 1001, 2048]
    long = encode_forms(7, 2048, ns)["chunks"][0]["layers"][1]
    assert (long["long_any"], long["long_all"], long["nleft"], long["left_first"], long["left_frames"]) == (1, 0, 2, 2, 3)


def test_a_tail_k_fwd_loss_does_not_take_turns_k_last_layer_off():
    """k_last_layer takes a chunk whole or not at all.  At -m 2 the last layer has 8 taps: a 1056-sample tail (33 x 32) is
    k_fwd_loss's and the chunk keeps k_last_layer; a 1016-sample tail (8 x 127, no multiple of 4 x 8) is not, and the chunk loses it.
    The rule's other class term, every trial of the last layer present, cannot fail on its own: an analysis length that is a
    multiple of 4 x P divides by every unit count up to P, so no frame reaches it without failing k_fwd_loss's test first."""
    F = frames_for(2, 81920)
    assert encode_forms(2, 2048, [2048] * F + [1056])["chunks"][0]["last_layer_all"] == 1
    c = encode_forms(2, 2048, [2048] * F + [1016])["chunks"][0]
    assert (c["fuse_cfg"], c["fuse_all"], c["last_layer_all"]) == (1, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# encode: every forcing knob overrides its rule

def test_forcing_knobs(monkeypatch):
    big, small = frames_for(7, 81920), 5
    def chunk(F, **env):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv("LINNE_AMD_" + k, v)
            return one_chunk(7, 10240, F)
    assert chunk(big, HIST="0")["hist"] == 0 and chunk(small, HIST="1")["hist"] == 1
    assert chunk(big, FWD_LOSS="0")["fwd_loss_on"] == 0 and chunk(small, FWD_LOSS="1")["fuse_all"] == 1
    assert chunk(big, LAST_LAYER="0")["last_layer_all"] == 0 and chunk(big, EXACT="1")["last_layer_all"] == 0 and chunk(big)["last_layer_all"] == 1
    assert chunk(small, FWD_LOSS="1")["layers"][2]["fwd_loss_mw"] == 1 and chunk(small, FWD_LOSS="1", FWD_LOSS_MW="0")["layers"][2]["fwd_loss_mw"] == 0
    assert chunk(1)["layers"][1]["lev_wave"] == 1 and chunk(1, LEV_WAVE="0")["layers"][1]["lev_wave"] == 0
    assert (chunk(9, LEV_RIDE="0")["layers"][1]["nlev"], chunk(9, LEV_RIDE="0")["layers"][1]["lev_ride"]) == (MAXT, MAXT), "72 jobs: a launch per trial, none rides"
    assert [chunk(small, **e)["layers"][1]["search_form"] for e in ({}, {"SEARCH_JOB": "0"}, {"SEARCH_TWO": "0"}, {"SEARCH_TWO": "0", "SEARCH_JOB": "1"})] == [2, 1, 0, 0]
    assert chunk(1, SEARCH_JOB="1")["layers"][1]["search_form"] == 2
    assert chunk(small, SEARCH_LONG="0")["layers"][1]["long_any"] == 0
    spec0 = chunk(small, SPECULATE="0")
    assert [l["fir_spec"] for l in chunk(small)["layers"]] == [1, 1, 0] and [l["fir_spec"] for l in spec0["layers"]] == [0, 0, 0]
    assert spec0["layers"][1]["long_any"] == 0, "k_search_long writes the one-unit forward: not without it"
    assert [l["fir_small"] for l in chunk(small)["layers"]] == [1, 0, 1] and [l["fir_small"] for l in chunk(small, FIR_SMALL="0")["layers"]] == [0, 0, 0]
    assert chunk(small)["prep_defer"] == 1 and chunk(small, PREP_DEFER="0")["prep_defer"] == 0 and chunk(small, PREP_GENERAL="1")["prep_defer"] == 0
    with monkeypatch.context() as m:
        m.setenv("LINNE_AMD_STATS_ROWS", "1")
        assert encode_forms(7, 2048, [2048])["stats_rows"] == 1
        m.setenv("LINNE_AMD_STATS_ROWS", "0")
        assert encode_forms(7, 2048, [2048] * 600)["stats_rows"] == 0
        m.delenv("LINNE_AMD_STATS_ROWS")
        m.setenv("LINNE_AMD_WIDE", "0")
        m.setenv("LINNE_AMD_L0_PRODUCTS", "0")
        assert encode_forms(7, 2048, [2048])["prod_ok"] == 0


def test_final_pass_of_af_is_the_same_rules_with_one_job_per_channel_frame():
    F = frames_for(7, 81920)
    call = encode_forms(7, 2048, [2048] * F, af=1)
    main, fin = call["chunks"]
    assert (main["final"], fin["final"]) == (0, 1) and fin["J"] == 2 * F and main["J"] == 8 * F
    assert main["last_layer_all"] == 0 and main["fuse_all"] == 1, "-a N keeps k_last_layer off: the final pass needs the search passes' winners"
    assert (fin["hist"], fin["fwd_loss_on"], fin["fuse_cfg"], fin["chain_sum"]) == (0, 0, 0, 0)
    assert [l["fir_spec"] for l in fin["layers"]] == [0, 0, 0] and [l["long_any"] for l in fin["layers"]] == [0, 0, 0]
    assert [l["forward"] for l in fin["layers"]] == [1, 1, 0], "no output of the last layer: only its parameters"
    assert [l["fir_small"] for l in fin["layers"]] == [1, 0, 1]
    small = encode_forms(7, 2048, [2048] * 16, af=1)["chunks"][1]
    assert small["J"] == 32 and [l["lev_wave"] for l in small["layers"]] == [1, 1, 1], "32 jobs in the final pass of a chunk of 128"
    assert one_chunk(7, 2048, F, learn=1)["last_layer_all"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# decode

def test_decode_pipe_below_1536_channel_frames():
    assert [decode_forms(7, 2048, F)["call"] for F in (767, 768, 769)] == [DEC_PIPE, DEC_LAYERS, DEC_LAYERS]
    assert [decode_forms(2, 2048, F, aligned=0)["call"] for F in (767, 3071, 3072, 3073)] == [DEC_PIPE, DEC_PIPE, DEC_LAYERS, DEC_LAYERS]
    d = decode_forms(7, 2048, 767)
    assert d["ms_separate"] == 1, "the one-launch forms leave MS -> LR to k_ms_to_lr"
    lanes = decode_forms(2, 2048, 3072, aligned=0)
    assert [l["form"] for l in lanes["layers"]] == [DL_SMALL, DL_BIG, DL_SMALL] and [l["pb"] for l in lanes["layers"]] == [4, 64, 8] and lanes["ms_separate"] == 1


@pytest.mark.parametrize("preset,S,nch,pb", [(7, 10240, 7, 16), (2, 2048, 3, 8)])
def test_decode_rows8_from_20480_channel_frames(preset, S, nch, pb):
    for F, form, want_pb in ((10239, DL_ROWS, 0), (10240, DL_ROWS8, pb), (10241, DL_ROWS8, pb)):
        d = decode_forms(preset, S, F)
        assert d["call"] == DEC_LAYERS and d["ms_separate"] == 0
        assert d["layers"][0] == {"form": DL_FUSED_L0, "nch": 0, "pb": 0, "de": 1, "ms_fold": 1}
        assert d["layers"][1] == {"form": DL_ROWS, "nch": nch, "pb": 0, "de": 0, "ms_fold": 0}
        assert d["layers"][2] == {"form": form, "nch": 0, "pb": want_pb, "de": 0, "ms_fold": 0}, F


def test_decode_knobs(monkeypatch):
    for F in (40, 30000):
        for name, call in (("wave", DEC_WAVE), ("pipe", DEC_PIPE), ("lanes", DEC_LAYERS), ("rows", DEC_LAYERS)):
            monkeypatch.setenv("LINNE_AMD_DECODE_KERNEL", name)
            d = decode_forms(7, 2048, F)
            assert d["call"] == call, (name, F)
            if name == "lanes":
                assert [l["form"] for l in d["layers"]] == [DL_SMALL, DL_BIG, DL_SMALL] and [l["pb"] for l in d["layers"]] == [4, 128, 16] and d["ms_separate"] == 1
            if name == "rows":
                assert [l["form"] for l in d["layers"]] == [DL_FUSED_L0, DL_ROWS, DL_ROWS8 if F >= 10240 else DL_ROWS]
    monkeypatch.setenv("LINNE_AMD_DECODE_KERNEL", "rows")
    for F, rows8, form in ((40, "1", DL_ROWS8), (30000, "0", DL_ROWS)):
        monkeypatch.setenv("LINNE_AMD_DECODE_ROWS8", rows8)
        assert decode_forms(7, 2048, F)["layers"][2]["form"] == form
        monkeypatch.setenv("LINNE_AMD_DECODE_FUSED", "0")
        l0 = decode_forms(7, 2048, F)["layers"][0]
        assert l0 == {"form": form, "nch": 0, "pb": 4, "de": 1, "ms_fold": 1}, "layer 0 by rows, the de-emphasis and MS -> LR behind it"
        monkeypatch.setenv("LINNE_AMD_DECODE_FUSED", "1")
        assert decode_forms(7, 2048, F)["layers"][0]["form"] == DL_FUSED_L0


# ---------------------------------------------------------------------------------------------------------------------------------
# the class bookkeeping over a list of calls, against the Python restatement

def replay(calls):
    shapes = (linne_amd.Shape * len(calls))(*[linne_amd.Shape(s[0], s[1], s[2], s[3], int(s[4])) for s, _ in calls])
    lengths = np.concatenate([np.asarray(ns, dtype=np.uint32) for _, ns in calls])
    counts = np.array([len(ns) for _, ns in calls], dtype=np.uint32)
    out = np.zeros(len(calls) * (2 + MAXCLS), dtype=np.int64)
    n = lib.lnn_classes_replay(shapes, lengths.ctypes.data, counts.ctypes.data, len(calls), out.ctypes.data, out.size)
    assert n == out.size
    rec = out.reshape(len(calls), 2 + MAXCLS)
    return [(BRANCH[int(r[0])], [int(v) for v in r[2:2 + int(r[1])]]) for r in rec]


@pytest.mark.parametrize("scenario,branches", [(ch.scenario1, ch.S1_BRANCHES), (ch.scenario2, ch.S2_BRANCHES), (ch.scenario3, ch.S3_BRANCHES),
                                               (ch.scenario6, ["first"] + ["reuse"] * 11)])
def test_class_bookkeeping_takes_the_scenarios_branches(scenario, branches):
    calls = ch.calls_of([s for s in scenario() if s.get("op", "encode") == "encode"])
    got = replay(calls)
    assert [b for b, _ in got] == branches
    assert got == ch.replay_classes(calls), "branches and resident lengths in slot order, call after call"


def test_class_sort_is_stable_and_slots_follow_first_appearance():
    call = encode_forms(7, 2048, [777, 2048, 777, 1001, 2048])
    assert call["lens"] == [777, 2048, 1001] and call["slots"] == [0, 1, 2] and call["na_max"] == 2048 and call["branch"] == 0
    assert call["chunks"][0]["nruns"] == 3 and call["chunks"][0]["present"] == 0b111
