"""CPU tests (-m "not gpu") of repairing damaged streams (include/linne_amd.h LINNEAmd_RepairStreamsDevice):
1. the premise -- what the numpy restatement of the contract (tests/repair_cases.py) makes of every damaged stream of the case table
   decodes under the real reference with the CRC check on, to the kept blocks' samples with zeros in the gaps -- against the
   reference's recorded answers (tests/golden/repair_answers.json, written from oracle/_ref by tests/golden/make_repair_golden.py),
   and against the reference itself where it is built;
2. the host's plan (linne_amd/csrc/lnn_repair.h, through the exported lnn_repair_plan) against the restatement, on the case table
   and on random block tables;
3. the boundary: symbols, struct layouts, Python entry points, argument errors that need no device."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import linne_amd
import repair_cases as rc
import splice_cases as sc
from refs import Reference, digest, reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, INSUFFICIENT_BUFFER = rc.OK, rc.INVALID_ARGUMENT, rc.INSUFFICIENT_BUFFER


@pytest.fixture(scope="module")
def answers():
    with open(os.path.join(ROOT, "tests", "golden", "repair_answers.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases(oracle):
    return rc.build_cases(oracle)


# ---- 1. the premise ----
def test_premise_the_reference_decodes_every_repaired_stream(answers, cases, oracle):
    assert sorted(cases) == sorted(answers)
    ref = Reference() if reference_available() else None
    for name, (data, clean) in cases.items():
        rec = answers[name]
        assert digest(data) == rec["stream"], name               # the oracle wrote the reference's stream
        got = rc.repair(data)
        if name.endswith("/n"):
            assert got is None and rec["repaired"] is None
            continue
        out, report = got
        want = rc.expected_pcm(oracle, data, out)
        assert digest(out) == rec["repaired"] and rec["ret"] == OK and rec["pcm"] == digest(want), name
        ret, pcm, _ = oracle.decode_whole(out)
        assert ret == OK and np.array_equal(pcm, want), name
        assert sc.header_fields(out) == sc.header_fields(data) and sum(sc.blocks_of(out)[4]) == sc.header_fields(data)["num_samples"], name
        if ref is not None:                                     # the real reference itself, where it is built
            rret, rpcm = ref.decode_whole(out)
            assert rret == OK and np.array_equal(np.stack(rpcm), want), name


def test_every_case_has_the_gaps_the_table_means(cases):
    """the gap lists, said outright (first sample, samples) -- and for one gap the samples are the original's with that range zero"""
    S, tail = rc.BLOCK, rc.SAMPLES - 11 * rc.BLOCK
    one = {"a": [], "b": [(5 * S, S)], "c/huge": [(5 * S, S)], "c/7": [(5 * S, S)], "d": [(5 * S, S)], "e": [(5 * S, S)], "f": [(5 * S, 0)],
           "g/middle": [(9 * S, 2 * S + tail)], "g/boundary": [(10 * S, S + tail)], "h": [(0, S)], "i": [(11 * S, tail)], "j": [(5 * S, 2 * S)]}
    for name in rc.SOURCES:
        x = rc.source_pcm(name)
        for case, want in one.items():
            data, clean = cases[f"{name}/{case}"]
            out, report = rc.repair(data)
            assert [(g["first_sample"], g["num_samples"]) for g in report["gaps"]] == want and report["exact"] == 1, (name, case)
            assert report["fill_blocks"] == sum(-(-n // S) for _, n in want) and report["lost_samples"] == sum(n for _, n in want)
            assert report["kept_blocks"] == 12 - sum(-(-n // S) for _, n in want), (name, case)
            if case in ("a", "f"):
                assert out == clean, (name, case)               # junk between sound blocks is dropped
        out, report = rc.repair(cases[f"{name}/k"][0])          # two gaps: placed by estimate
        assert report["exact"] == 0 and report["num_gaps"] == 2 and report["lost_samples"] == 2 * S and report["kept_blocks"] == 10
        assert report["gaps"][0]["first_sample"] == 3 * S and sum(g["num_samples"] for g in report["gaps"]) == 2 * S
        assert report["gaps"][1]["first_sample"] == 3 * S + report["gaps"][0]["num_samples"] + 4 * S
    for preset in sc.PREMISE_PRESETS:
        out, report = rc.repair(cases[f"trim/m{preset}/l"][0])
        assert [(g["first_sample"], g["num_samples"], g["fill_blocks"]) for g in report["gaps"]] == [(0, 548, 1)] and report["exact"] == 1
    out, report = rc.repair(cases["mono/m0/m/intact"][0])       # the embedded block is skipped: the chain goes on behind the RAW block
    assert out == cases["mono/m0/m/intact"][0] and report["num_gaps"] == 0 and report["kept_blocks"] == 12
    out, report = rc.repair(cases["mono/m0/m/broken"][0])       # the documented limit: inside a lost stretch it is kept
    assert report["kept_blocks"] == 12 and report["num_gaps"] == 2 and report["lost_samples"] == S - 100 and report["exact"] == 0


def test_one_gap_is_the_original_with_that_range_zero(cases, oracle):
    for name in ("mono/m7", "stereo/m0/ms"):
        x = rc.source_pcm(name)
        for case in ("b", "e", "g/middle", "g/boundary", "h", "i", "j"):
            out, report = rc.repair(cases[f"{name}/{case}"][0])
            g = report["gaps"][0]
            want = x.copy()
            want[:, g["first_sample"]:g["first_sample"] + g["num_samples"]] = 0
            ret, pcm, _ = oracle.decode_whole(out)
            assert ret == OK and np.array_equal(pcm, want), (name, case)


# ---- 2. the planner ----
def library_plan(kept, N, S, stream_bytes, capacity):
    """lnn_repair_plan -> (output layout as [(fill, src, dst, bytes)], fill bytes, report)"""
    u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64).reshape(-1)
    head, blocks = u64([N, S, stream_bytes, capacity]), u64([list(k) for k in kept] or [[0, 0, 0]])
    out_rec = np.zeros(9, np.uint64)
    cap = len(kept) + 2
    gap_rec, run_rec = np.zeros(6 * cap, np.uint64), np.zeros(4 * (2 * cap + 1), np.uint64)
    fill_cap = 11 * (N // min(S, 65535) + cap + 1)
    fill = np.zeros(fill_cap, np.uint8)
    f = linne_amd.lib.lnn_repair_plan
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    assert f(head.ctypes.data, blocks.ctypes.data, len(kept), out_rec.ctypes.data, gap_rec.ctypes.data, cap, run_rec.ctypes.data, 2 * cap + 1, fill.ctypes.data, fill_cap) == 0
    result, nbytes, kept_blocks, fill_blocks, ngaps, lost, exact, nruns, nfill = (int(v) for v in out_rec)
    assert ngaps <= cap and nruns <= 2 * cap + 1 and nfill <= fill_cap
    gaps = [dict(zip(("first_sample", "num_samples", "src_offset", "src_bytes", "fill_blocks", "fill_at"), (int(v) for v in gap_rec[6 * i:6 * i + 6]))) for i in range(ngaps)]
    runs = [tuple(int(v) for v in run_rec[4 * i:4 * i + 4]) for i in range(nruns)]
    report = {"out_bytes": nbytes, "result": result, "kept_blocks": kept_blocks, "fill_blocks": fill_blocks, "num_gaps": ngaps, "lost_samples": lost, "exact": exact}
    return runs, bytes(fill[:nfill]), gaps, report


def restated_plan(kept, N, S, stream_bytes, capacity):
    """the same from tests/repair_cases.py: the output as pieces of the source and fill bytes, in order"""
    gaps, exact, layout = rc.plan(kept, N, S, stream_bytes)
    F = min(S, 65535)
    pieces, fill = [], b""
    for item in layout:
        if item[0] == "src":
            if pieces and pieces[-1][0] == 0 and pieces[-1][1] + pieces[-1][2] == item[1]:
                pieces[-1] = (0, pieces[-1][1], pieces[-1][2] + item[2] - item[1])
            else:
                pieces.append((0, item[1], item[2] - item[1]))
        else:
            blocks = b"".join(rc.silent_block(min(F, item[1] - k)) for k in range(0, item[1], F))
            pieces.append((1, len(fill), len(blocks)))
            fill += blocks
    runs, dst = [], 0
    for f, src, n in pieces:
        runs.append((f, src, dst, n))
        dst += n
    report = {"out_bytes": dst, "result": OK, "kept_blocks": len(kept), "fill_blocks": sum(g["fill_blocks"] for g in gaps), "num_gaps": len(gaps),
              "lost_samples": N - sum(n for _, _, n in kept), "exact": exact}
    if dst > capacity or dst > 2 ** 32 - 1:
        report["result"] = INSUFFICIENT_BUFFER
        return [], b"", gaps, report
    return runs, fill, gaps, report


def check_plan(kept, N, S, stream_bytes):
    want = restated_plan(kept, N, S, stream_bytes, 1 << 40)
    got = library_plan(kept, N, S, stream_bytes, 1 << 40)
    keys = ("first_sample", "num_samples", "src_offset", "src_bytes", "fill_blocks")
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3]
    assert [{k: g[k] for k in keys} for g in got[2]] == [{k: g[k] for k in keys} for g in want[2]]
    need = want[3]["out_bytes"]
    for cap, code in ((need - 1, INSUFFICIENT_BUFFER), (need, OK), (need + 1, OK)):      # the verdict on the capacity
        runs, fill, _, report = library_plan(kept, N, S, stream_bytes, cap)
        assert (report["result"], report["out_bytes"]) == (code, need) and (code == OK or (runs == [] and fill == b""))
    return want


def test_plan_against_the_restatement_on_every_case(cases):
    for name, (data, _) in cases.items():
        if name.endswith("/n"):
            continue
        h = sc.header_fields(data)
        kept = rc.salvage_chain(bytes(data), h)
        runs, fill, gaps, report = check_plan(kept, h["num_samples"], h["num_samples_per_block"], len(data))
        out, rep = rc.repair(data)
        assert b"".join((fill if f else data)[src:src + n] for f, src, _, n in runs) == out, name
        assert {k: rep[k] for k in report} == report, name


def test_plan_on_random_block_tables():
    rng = np.random.default_rng(2026)
    seen = {"zero trailing": 0, "big S": 0, "five gaps": 0, "no blocks": 0, "no gap": 0}
    for trial in range(300):
        S = int(rng.choice([256, 1024, 4096, 70000, 200000]))
        nb, ngaps = int(rng.integers(0, 41)), int(rng.integers(0, 6))
        holes = set(rng.choice(nb + 1, size=min(ngaps, nb + 1), replace=False).tolist()) if ngaps else set()
        kept, at, samples = [], 30, 0
        for r in range(nb):
            if r in holes:
                at += int(rng.integers(1, 5000))
            size, n = int(rng.integers(5, 3000)), int(rng.integers(1, S + 1))
            kept.append((at, size, n))
            at += size + 6
            samples += n
        tail_bytes = int(rng.integers(0, 3000)) if nb in holes else 0
        lost = int(rng.integers(1, 3 * S)) if (holes or rng.integers(0, 2)) else 0
        want = check_plan(kept, samples + lost, S, at + tail_bytes)
        seen["zero trailing"] += bool(want[2]) and want[2][-1]["src_bytes"] == 0
        seen["big S"] += S > 65535 and want[3]["fill_blocks"] > 0
        seen["five gaps"] += want[3]["num_gaps"] >= 5
        seen["no blocks"] += nb == 0
        seen["no gap"] += want[3]["num_gaps"] == 0
    assert all(seen.values()), seen


def test_plan_facts():
    """what the random tables must agree with, said outright"""
    blk = lambda off, size, n: (off, size, n)
    # a truncation exactly behind a block: one trailing gap of 0 bytes gets everything
    runs, fill, gaps, report = library_plan([blk(30, 94, 1024)], 3000, 1024, 130, 1 << 40)
    assert gaps[0]["src_bytes"] == 0 and (gaps[0]["first_sample"], gaps[0]["num_samples"], gaps[0]["fill_blocks"]) == (1024, 1976, 2) and report["exact"] == 1
    assert runs == [(0, 0, 0, 130), (1, 0, 130, 22)] and fill == rc.silent_block(1024) + rc.silent_block(952)
    # S above 65535: a fill block holds at most 65535 samples
    runs, fill, gaps, report = library_plan([], 200000, 100000, 30, 1 << 40)
    assert report["fill_blocks"] == 4 and fill == rc.silent_block(65535) * 3 + rc.silent_block(200000 - 3 * 65535) and report["kept_blocks"] == 0
    # two gaps share by their bytes, the remainder to the last; the header and a first block at byte 30 are one run
    kept = [blk(30, 94, 1000), blk(230, 94, 1000), blk(630, 94, 1000)]
    runs, fill, gaps, report = library_plan(kept, 3100, 1024, 730, 1 << 40)
    assert [(g["src_bytes"], g["num_samples"]) for g in gaps] == [(100, 25), (300, 75)] and report["exact"] == 0
    assert runs[0] == (0, 0, 0, 130) and [r[0] for r in runs] == [0, 1, 0, 1, 0]
    # an undamaged stream: one run, its bytes up to the last block's end
    runs, fill, gaps, report = library_plan([blk(30, 94, 1000), blk(130, 94, 1000)], 2000, 1024, 999, 1 << 40)
    assert runs == [(0, 0, 0, 230)] and gaps == [] and report["exact"] == 1 and report["out_bytes"] == 230


# ---- 3. the boundary ----
def test_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("LINNEAmd_RepairStreamsDevice", "LINNEAmd_GetLastRepairGaps", "LINNEAmd_GetLastRepairCount"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in linne_amd.AMD_SYMBOLS, name
        assert hasattr(linne_amd.lib, name), name
    assert re.search(r"struct\s+LINNEAmdRepair\s*\{", src) and re.search(r"struct\s+LINNEAmdGap\s*\{", src)
    assert hasattr(linne_amd.lib, "lnn_repair_plan")


def test_struct_layouts():
    G, R = linne_amd.Gap, linne_amd.Repair
    assert [(f[0], getattr(G, f[0]).offset) for f in G._fields_] == [("first_sample", 0), ("num_samples", 8), ("src_offset", 16), ("src_bytes", 24),
                                                                    ("fill_blocks", 32), ("reserved", 36)]
    assert C.sizeof(G) == 40
    assert [(f[0], getattr(R, f[0]).offset) for f in R._fields_] == [("d_stream", 0), ("stream_bytes", 8), ("d_out", 16), ("capacity", 24), ("out_bytes", 32),
                                                                    ("lost_samples", 40), ("kept_blocks", 48), ("fill_blocks", 52), ("num_gaps", 56), ("exact", 60),
                                                                    ("result", 64)]
    assert C.sizeof(R) == 72


def test_python_entry_points():
    p = inspect.signature(linne_amd.Context.repair_streams).parameters
    assert list(p) == ["self", "streams", "return_codes"] and p["return_codes"].default is False
    assert list(inspect.signature(linne_amd.Context.last_repair_count).parameters) == ["self", "which"]


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_RepairStreamsDevice
    s = (linne_amd.Repair * 2)()
    for i in range(2):
        s[i].result, s[i].out_bytes = -1, 77
    assert f(None, s, 2) == INVALID_ARGUMENT and f(None, None, 0) == INVALID_ARGUMENT
    assert linne_amd.lib.LINNEAmd_GetLastRepairCount(None, 0) == -1
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    assert f(C.addressof(blank), None, 3) == INVALID_ARGUMENT
    assert f(C.addressof(blank), None, 0) == OK and f(C.addressof(blank), s, 0) == OK
    assert [(s[i].result, s[i].out_bytes) for i in range(2)] == [(-1, 77)] * 2
    assert [linne_amd.lib.LINNEAmd_GetLastRepairCount(C.addressof(blank), w) for w in range(7)] == [0] * 7
    assert linne_amd.lib.LINNEAmd_GetLastRepairCount(C.addressof(blank), 7) == -1 and linne_amd.lib.LINNEAmd_GetLastRepairCount(C.addressof(blank), -1) == -1
    gaps, n = C.POINTER(linne_amd.Gap)(), C.c_uint32(5)
    assert linne_amd.lib.LINNEAmd_GetLastRepairGaps(C.addressof(blank), 0, C.byref(gaps), C.byref(n)) == INVALID_ARGUMENT
    assert linne_amd.lib.LINNEAmd_GetLastRepairGaps(None, 0, C.byref(gaps), C.byref(n)) == INVALID_ARGUMENT
