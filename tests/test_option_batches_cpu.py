"""The premises of tests/test_gpu_option_batches.py, without a GPU: the batches of tests/option_batches.py are what their cases say --
the option changes what the oracle answers, the oracle's answers vary between the lanes, silence yields zero problems beside live
ones, the channel-frame counts lie where the launch rules flip, and the library's own rules (lnn_forms_query) cut and serve the
calls as the cases are written for.  The oracle's round trip of every (base, length) pair is asserted where its answers are
computed (test_gpu_batch_forms.OracleBatch)."""
import ctypes as C

import numpy as np
import pytest

import linne_amd
import option_batches as ob
from test_gpu_batch_forms import param_words

ALL = sorted(ob.CASES)
BASIC = [n for n in ALL if not ob.CASES[n]["thirds"]]


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    import os
    for v in list(os.environ):
        if v.startswith("LINNE_AMD_") and v != "LINNE_AMD_LIB":
            monkeypatch.delenv(v)


def pairs(n, ans):
    """per oracle run of the batch: (base, length)"""
    b = ob.batch_of(n)
    out = np.zeros((len(ans.taps), 2), dtype=np.int64)
    out[ans.key] = np.stack([b["bmap"], b["ns"].astype(np.int64)], axis=1)
    return out


@pytest.mark.parametrize("n", ALL, ids=[ob.NAMES[n] for n in ALL])
def test_size_premises(n):
    c, b = ob.CASES[n], ob.batch_of(n)
    CF = c["F"] * c["nch"]
    assert CF % 64 != 0 and CF % 256 != 0 and CF > 64
    for threshold, side in c["side"]:
        assert (CF > threshold) if side == "above" else (CF <= threshold), (CF, threshold, side)
    assert b["frames"].shape == (c["F"], c["nch"], c["block"]) and 512 <= c["block"] <= 1024
    lengths = set(b["ns"].tolist())
    assert len(lengths) <= 16 and c["block"] in lengths
    Ls = linne_amd.PRESET_LAYERS[c["preset"]]
    assert {1, 3, 7, Ls[1] - 1, Ls[1], Ls[1] + 1, c["block"] // 2 + 1} <= lengths
    ragged = int((b["ns"] < c["block"]).sum())
    assert ragged == min(40, c["F"] // 2) and ragged >= 22
    silent = np.flatnonzero(b["bmap"] == 0)
    assert (b["ns"][silent] == c["block"]).any() and (b["ns"][silent] < c["block"]).any(), "silence on full and on ragged frames"
    assert not b["frames"][silent].any()
    assert {1, 2, 3, 4} <= set(b["bmap"].tolist()), "chirps and noise"
    assert sum(1 for base in set(b["bmap"].tolist()) if base >= 5) >= 20, "music"
    # the blocks the -a / -l kernels are launched with (lnn_device.hip run_af, run_train, run_final_pass)
    if n in (1, 2, 3, 5):
        assert (CF + 255) // 256 == 2 and CF % 256 != 0, "two blocks of the 256-thread kernels, the second partial"
    if n == 1:
        assert (CF + 63) // 64 == 6 and CF % 64 != 0, "one problem per channel-frame would already be six blocks of 64, the last partial"


@pytest.mark.parametrize("n", BASIC, ids=[ob.NAMES[n] for n in BASIC])
def test_the_option_changes_the_oracles_answer(oracle, n):
    c = ob.CASES[n]
    on, off = ob.answers(oracle, n, True), ob.answers(oracle, n, False)
    pr = pairs(n, on)
    assert np.array_equal(pr, pairs(n, off))
    w = param_words(c["preset"])
    loud = pr[:, 0] != 0
    changed = (on.prm[:, :, w] != off.prm[:, :, w]).any(axis=(1, 2))
    print(f"case {n}: the option changes {int((changed & loud).sum())} of {int(loud.sum())} non-silent (base, length) pairs")
    assert 2 * int((changed & loud).sum()) >= int(loud.sum())
    assert not changed[~loud].any(), "silence: zeros with the option and without"


@pytest.mark.parametrize("n", BASIC, ids=[ob.NAMES[n] for n in BASIC])
def test_the_oracles_answers_vary(oracle, n):
    c = ob.CASES[n]
    on = ob.answers(oracle, n, True)
    Ls = linne_amd.PRESET_LAYERS[c["preset"]]
    units = on.prm[:, :, 4:4 + len(Ls)]
    for l in range(len(Ls)):
        assert len(np.unique(units[:, :, l])) > 1, f"layer {l}: one unit count everywhere"
    ll = ob.long_layer(c["preset"])
    print(f"case {n}: unit counts of the long layer {np.unique(units[:, :, ll]).tolist()}")
    assert (units[:, :, ll] == 1).any(), "no frame keeps one unit in the long layer"
    assert (units[:, :, ll] > 1).any(), "no multi-unit problem: no job contributes several entries to the problem list"
    if linne_amd.PRESET_NUM_REGULARS[c["preset"]] > 1:
        assert len(np.unique(on.best)) > 1, "one best regulariser everywhere"


@pytest.mark.parametrize("n", BASIC, ids=[ob.NAMES[n] for n in BASIC])
def test_silence_is_a_zero_problem_beside_live_ones(oracle, n):
    c = ob.CASES[n]
    on = ob.answers(oracle, n, True)
    pr = pairs(n, on)
    ncoef = sum(linne_amd.PRESET_LAYERS[c["preset"]])
    coef = on.prm[:, :, 10:10 + ncoef]
    silent = pr[:, 0] == 0
    assert silent.sum() >= 2 and not coef[silent].any(), "the silent base: every coefficient zero"
    assert coef[~silent].any(axis=(1, 2)).sum() >= (~silent).sum() // 2, "in a call where the others are not"


def test_loud_24bit_rows_go_to_k_prep_slow():
    """case 2: channel-frames whose sum of squares reaches 2^53 fail k_prep's exact-sum test (no MS: the channels as they are)"""
    x = ob.batch_of(2)["frames"].astype(np.int64)
    rows = int(((x * x).sum(axis=2) >= (1 << 53)).sum())
    assert rows >= 64, f"{rows} channel-frames for k_prep_slow"


@pytest.mark.parametrize("n", ALL, ids=[ob.NAMES[n] for n in ALL])
def test_chunks_and_final_pass_forms(n):
    """the call as the library's rules cut and serve it.  Expected values from the rules as lnn_forms.h states them: the final pass has
    one job per channel-frame; lev_wave up to 64 jobs, sel_wave up to 256; k_autocorr_wide for a call of at most 64 rows"""
    c = ob.CASES[n]
    F, nch = c["F"], c["nch"]
    R = linne_amd.PRESET_NUM_REGULARS[c["preset"]]
    call = ob.forms(n, arena=ob.arena_for(n))
    assert ob.per_frame(n, on=False) == lib_per_frame(n) < call["per_frame"], "the options need scratch of their own"
    if c["thirds"]:
        third = (F + 2) // 3
        assert call["chunk"] == third and [k["Fc"] for k in call["chunks"]] == [third, third, F - 2 * third]
        assert call["chunks"][-1]["Fc"] <= third and (n != 6 or call["chunks"][-1]["Fc"] < third)
    else:
        assert call["nchunks"] == 1 and call["chunks"][0]["Fc"] == F
    assert call["nsub"] == 1 and call["use_sub"] == 0
    ll = ob.long_layer(c["preset"])
    assert not (call["prod_ok"] >> ll) & 1, "k_autocorr2 for the long layer"
    for k in call["chunks"]:
        assert k["J"] == k["Fc"] * nch * R and k["last_layer_all"] == 0 and k["hist"] == 0
        assert ("final_pass" in k) == bool(c["af"])
        if c["af"]:
            fin = k["final_pass"]
            assert fin["J"] == k["Fc"] * nch
            lev, sel = ob.final_forms_expected(fin["J"])
            assert [l["lev_wave"] for l in fin["layers"]] == [lev] * call["L"] and [l["sel_wave"] for l in fin["layers"]] == [sel] * call["L"]
            assert lev == 0, "every case's final pass runs k_levinson_lds"
            if not c["thirds"]:
                assert sel == c["sel_wave"]
    if n == 6:
        assert [k["final_pass"]["J"] for k in call["chunks"]] == [108, 108, 106]


def lib_per_frame(n):
    shape = ob.shape_of(n)
    return int(linne_amd.lib.LINNEAmd_ScratchBytesPerFrame(C.byref(shape)))


def test_two_streams_do_not_cut_a_call_of_case_1s_size(monkeypatch):
    """why there is no eighth case: with LINNE_AMD_STREAMS=2 given when the context is created, lnn_call_split still asks for 512 frames
    per stream; the 161 frames stay one chunk (forked off the caller's stream, which changes no kernel form)"""
    monkeypatch.setenv("LINNE_AMD_STREAMS", "2")
    call = ob.forms(1, streams=-1)
    assert (call["streams_forced"], call["nsub"], call["nchunks"]) == (1, 1, 1)
