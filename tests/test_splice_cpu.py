"""CPU tests (-m "not gpu") of cutting and joining streams (include/linne_amd.h LINNEAmd_SpliceStreamsDevice):
1. the premise -- a stream that keeps untouched blocks byte for byte and holds re-encoded edge blocks of fewer samples is a valid
   .lnn stream -- against the real reference's recorded answers (tests/golden/splice_answers.json, written from oracle/_ref by
   tests/golden/make_splice_golden.py), and against the reference itself where it is built;
2. which fragment lengths the reference's encoder takes at all;
3. the host's plan (linne_amd/csrc/lnn_splice.h, through the exported lnn_splice_plan) against a numpy restatement of the contract;
4. the boundary: symbols, struct layout, Python entry points, argument errors that need no device."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import linne_amd
import splice_cases as sc
from refs import Reference, digest, reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, INSUFFICIENT_BUFFER, CORRUPTION = sc.OK, sc.INVALID_ARGUMENT, sc.INSUFFICIENT_BUFFER, sc.CORRUPTION


@pytest.fixture(scope="module")
def answers():
    with open(os.path.join(ROOT, "tests", "golden", "splice_answers.json")) as f:
        return json.load(f)


# ---- 1. the premise ----
@pytest.mark.parametrize("preset", sc.PREMISE_PRESETS)
@pytest.mark.parametrize("case", ["trim", "join"])
def test_premise_the_reference_decodes_a_spliced_stream(answers, oracle, case, preset):
    name = f"{case}/m{preset}"
    cuts = sc.premise_cases(preset)[name]
    data, want = sc.splice_with(oracle, cuts, preset)            # the oracle's streams and fragment blocks, spliced in numpy
    rec = answers[f"premise/{name}"]
    # the reference wrote the same bytes (so the oracle's encode_whole(fragment)[30:] is the reference's), decoded them with the CRC
    # check on, returned OK and the cuts' samples
    assert digest(data) == rec["stream"]
    assert rec["ret"] == OK and rec["pcm"] == digest(want)
    ret, pcm, _ = oracle.decode_whole(data)
    assert ret == OK and np.array_equal(pcm, want)
    if case == "trim":                                          # the stream is what the issue describes
        off, first, size, typ, nsmp = sc.blocks_of(data)
        assert nsmp == [548, 1024, 1024, 1024, 880] and sc.header_fields(data)["num_samples"] == 4500
        src = oracle.encode_whole(cuts[0][0], 16, 44100, 1024, preset, True)
        so, _, ss, _, _ = sc.blocks_of(src)
        assert data[off[1]:off[4]] == src[so[2]:so[4] + ss[4] + 6]
    if reference_available():                                   # the real reference itself, where it is built
        ref = Reference()
        rdata, _ = sc.splice_with(ref, cuts, preset)
        rret, rpcm = ref.decode_whole(rdata)
        assert rdata == data and rret == OK and np.array_equal(np.stack(rpcm), want)


# ---- 2. the fragments the reference encodes at all ----
def test_fragment_lengths_the_reference_takes(answers, oracle):
    good = {p: [n for n in sc.FRAGMENT_LENGTHS if answers[f"fragment/m{p}/n{n}"]["good"]] for p in sc.PREMISE_PRESETS}
    assert any(n <= 33 for n in good[0]), good
    assert 129 in good[7] and 256 in good[7], good
    for p in sc.PREMISE_PRESETS:
        for n in sc.FRAGMENT_LENGTHS:
            rec = answers[f"fragment/m{p}/n{n}"]
            # the rule the header states: an edge block of no more samples than the preset's largest layer is outside the contract
            assert rec["good"] == (n > sc.MAX_ORDER[p]), (p, n, rec["how"])
            if rec["good"]:
                assert digest(oracle.encode_whole(sc.fragment_pcm(n, p), 16, 44100, sc.PREMISE_BLOCK, p, True)[sc.HEADER:]) == rec["block"]


# ---- 3. the planner ----
def tables(nsmp, sizes):
    """block tables of a made-up stream: the blocks' sample counts and size fields"""
    off, first, at = [], [0], sc.HEADER
    for n, s in zip(nsmp, sizes):
        off.append(at)
        first.append(first[-1] + n)
        at += s + 6
    return off, first, list(sizes), [0] * len(nsmp), list(nsmp)


A = sc.PlanStream(tables([1024] * 8 + [500], [901, 17, 1200, 5, 777, 4100, 333, 64, 222]), 8 * 1024 + 500)        # a ragged last block
B = sc.PlanStream(tables([1024] * 4, [400, 401, 402, 403]), 4096)
MONO = sc.PlanStream(tables([1024] * 4, [400, 401, 402, 403]), 4096, channels=1, ms=0)
M7 = sc.PlanStream(tables([1024] * 4, [400, 401, 402, 403]), 4096, preset=7)
DAMAGED = sc.PlanStream(tables([1024] * 8, [300] * 8), 8192, fail_block=5, fail_code=CORRUPTION)
SHORT = sc.PlanStream(tables([1024] * 2, [300] * 2), 4096)                                                             # its blocks end before its header's count
STREAMS = [A, B, MONO, M7, DAMAGED, SHORT]
BIG = 1 << 40

PLAN_CASES = {
    "inside one block": [([(0, 1100, 500)], BIG, 0)],
    "on block boundaries": [([(0, 1024, 3072)], BIG, 0)],
    "one whole block": [([(0, 2048, 1024)], BIG, 0)],
    "head and tail fragments": [([(0, 1500, 4500)], BIG, 0)],
    "head fragment only": [([(0, 1500, 548 + 2048)], BIG, 0)],
    "tail fragment only": [([(0, 1024, 1024 + 100)], BIG, 0)],
    "the ragged last block whole": [([(0, 7 * 1024, 1024 + 500)], BIG, 0), ([(0, 8 * 1024, 500)], BIG, 0)],
    "the whole stream": [([(0, 0, 8 * 1024 + 500)], BIG, 0)],
    "zero-sample cuts between others": [([(0, 0, 0), (0, 100, 900), (1, 512, 0), (1, 1024, 2048), (0, 8692, 0)], BIG, 0)],
    "a join": [([(0, 700, 3000), (1, 2048, 2000), (0, 0, 1024)], BIG, 0)],
    "many outputs": [([(0, 1500, 4500)], BIG, 0), ([(1, 0, 4096)], BIG, 0), ([(0, 100, 200)], BIG, 0)],
    "mismatched shapes": [([(0, 0, 1024), (2, 0, 1024)], BIG, 0), ([(1, 0, 1024), (3, 0, 1024)], BIG, 0), ([(1, 0, 1024)], BIG, 0)],
    "a range past the end": [([(1, 4000, 97)], BIG, 0), ([(1, 4097, 0)], BIG, 0), ([(1, 4096, 0), (1, 0, 4096)], BIG, 0), ([(1, 0, 2 ** 64 - 1)], BIG, 0)],
    "beyond the blocks": [([(5, 1024, 2048)], BIG, 0), ([(5, 0, 2048)], BIG, 0)],
    "no cuts, no samples, too many": [([], BIG, 0), ([(0, 5, 0), (1, 7, 0)], BIG, 0), ([(-1, 0, 10)], BIG, 0), ([(0, 0, 100)], BIG, sc.WHY["align"]),
                                      ([(0, 0, 100)], BIG, sc.WHY["null"])],
    "damage": [([(4, 0, 4096)], BIG, 0), ([(4, 0, 5 * 1024)], BIG, 0), ([(4, 0, 5 * 1024 + 1)], BIG, 0), ([(4, 6200, 300)], BIG, 0),
               ([(1, 0, 1024), (4, 7000, 1000), (0, 0, 1024)], BIG, 0), ([(4, 0, 8193)], BIG, 0)],
    "short fragments": [([(0, 1000, 1024)], BIG, 0), ([(0, 1024 - 32, 1024 + 32)], BIG, 0), ([(0, 1024 - 33, 1024 + 33 + 33)], BIG, 0), ([(3, 0, 128)], BIG, 0),
                        ([(3, 0, 129)], BIG, 0), ([(0, 8 * 1024 + 490, 10)], BIG, 0)],
}


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_against_the_numpy_restatement(name):
    outputs = PLAN_CASES[name]
    frag_bytes = [211 + 37 * i for i in range(16)]
    got = sc.library_plan(linne_amd.lib, STREAMS, outputs, frag_bytes)
    want = sc.numpy_plan(STREAMS, outputs, frag_bytes)
    assert got == want
    # and, at every output's needed size: one byte less does not fit, the size itself and one more do
    for k, (cuts, _, why0) in enumerate(outputs):
        if want[0][k]["result"] != OK:
            continue
        need = want[0][k]["bytes"]
        for cap, code in ((need - 1, INSUFFICIENT_BUFFER), (need, OK), (need + 1, OK)):
            trial = list(outputs)
            trial[k] = (cuts, cap, why0)
            g, w = sc.library_plan(linne_amd.lib, STREAMS, trial, frag_bytes), sc.numpy_plan(STREAMS, trial, frag_bytes)
            assert g == w and g[0][k]["result"] == code and g[0][k]["bytes"] == need
            assert [o["result"] for o in g[0][:k] + g[0][k + 1:]] == [o["result"] for o in want[0][:k] + want[0][k + 1:]]


def test_plan_facts():
    """what the cases above must have hit, said outright"""
    plan = lambda outputs: sc.library_plan(linne_amd.lib, STREAMS, outputs, [100] * 8)
    outs, pieces = plan(PLAN_CASES["on block boundaries"])
    assert (outs[0]["encoded_blocks"], outs[0]["copied_blocks"], len(pieces)) == (0, 3, 1)
    assert pieces[0][2:7] == (0, 3, A.tables[0][1], A.tables[0][4], A.tables[0][4] - A.tables[0][1]) and outs[0]["bytes"] == 30 + 17 + 1200 + 5 + 18
    outs, pieces = plan(PLAN_CASES["inside one block"])
    assert (outs[0]["encoded_blocks"], outs[0]["copied_blocks"]) == (1, 0) and pieces[0][2:6] == (1, 1, 1100, 1600) and outs[0]["bytes"] == 130
    outs, pieces = plan(PLAN_CASES["the ragged last block whole"])
    assert [(o["encoded_blocks"], o["copied_blocks"], o["total_samples"]) for o in outs] == [(0, 2, 1524), (0, 1, 500)]
    outs, pieces = plan(PLAN_CASES["head and tail fragments"])
    assert [p[2:6] for p in pieces] == [(1, 1, 1500, 2048), (0, 3, A.tables[0][2], A.tables[0][5]), (1, 1, 5120, 6000)]
    outs, pieces = plan(PLAN_CASES["zero-sample cuts between others"])
    assert outs[0]["result"] == OK and outs[0]["total_samples"] == 2948 and [p[1] for p in pieces] == [1, 3]
    assert [o["why"] for o in plan(PLAN_CASES["mismatched shapes"])[0]] == [sc.WHY["shape"], sc.WHY["shape"], 0]
    assert [o["why"] for o in plan(PLAN_CASES["a range past the end"])[0]] == [sc.WHY["range"], sc.WHY["range"], 0, sc.WHY["range"]]
    assert [o["result"] for o in plan(PLAN_CASES["damage"])[0]] == [OK, OK, CORRUPTION, CORRUPTION, CORRUPTION, INVALID_ARGUMENT]
    assert [o["why"] for o in plan(PLAN_CASES["short fragments"])[0]] == [sc.WHY["short_fragment"]] * 2 + [0, sc.WHY["short_fragment"], 0, sc.WHY["short_fragment"]]
    many = [([(0, 0, 8 * 1024 + 500)] * 500000, BIG, 0)]          # 500000 * 8692 > 2^32 - 1
    assert plan(many)[0][0]["why"] == sc.WHY["total"]


# ---- 4. the boundary ----
def test_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("LINNEAmd_SpliceStreamsDevice", "LINNEAmd_GetLastSpliceCount"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in linne_amd.AMD_SYMBOLS, name
        assert hasattr(linne_amd.lib, name), name
    assert re.search(r"struct\s+LINNEAmdCut\s*\{", src) and re.search(r"struct\s+LINNEAmdSplice\s*\{", src)
    assert hasattr(linne_amd.lib, "lnn_splice_plan")


def test_struct_layouts():
    assert [(f[0], getattr(linne_amd.Cut, f[0]).offset) for f in linne_amd.Cut._fields_] == [("index", 0), ("d_stream", 8), ("first_sample", 16), ("num_samples", 24)]
    assert C.sizeof(linne_amd.Cut) == 32
    S = linne_amd.Splice
    assert [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [("cuts", 0), ("num_cuts", 8), ("d_out", 16), ("capacity", 24), ("out_bytes", 32),
                                                                    ("copied_blocks", 40), ("encoded_blocks", 44), ("result", 48)]
    assert C.sizeof(S) == 56


def test_python_entry_points():
    p = inspect.signature(linne_amd.Context.splice_streams).parameters
    assert list(p)[:2] == ["self", "splices"] and (p["group_frames"].default, p["return_codes"].default) == (0, False)
    assert list(inspect.signature(linne_amd.Context.last_splice_count).parameters) == ["self", "which"]


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_SpliceStreamsDevice
    s = (linne_amd.Splice * 2)()
    for i in range(2):
        s[i].result, s[i].out_bytes = -1, 77
    assert f(None, s, 2, 0) == INVALID_ARGUMENT and f(None, None, 0, 0) == INVALID_ARGUMENT
    assert linne_amd.lib.LINNEAmd_GetLastSpliceCount(None, 0) == -1
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    assert f(C.addressof(blank), None, 3, 0) == INVALID_ARGUMENT
    assert f(C.addressof(blank), None, 0, 0) == OK and f(C.addressof(blank), s, 0, 0) == OK
    assert [(s[i].result, s[i].out_bytes) for i in range(2)] == [(-1, 77)] * 2
    assert [linne_amd.lib.LINNEAmd_GetLastSpliceCount(C.addressof(blank), w) for w in range(6)] == [0] * 6
    assert linne_amd.lib.LINNEAmd_GetLastSpliceCount(C.addressof(blank), 6) == -1 and linne_amd.lib.LINNEAmd_GetLastSpliceCount(C.addressof(blank), -1) == -1
