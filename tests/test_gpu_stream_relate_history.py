"""The relate call's answers do not depend on the calls the context served before, nor the other windows calls' on it (-m gpu).

The relate call's accumulators lie in the context's scratch where the measure, digest, quiet and histogram calls keep theirs, behind
every pass's buffers: a record that the preset did not zero, or a region sized for another call, would show as a sum or a count that
depends on the call before.  On one fresh context the relate call runs before and after each of the six other windows consumers,
large, then small, then large again, and behind failing calls; every answer -- the siblings' too -- is held to its reference for that
call alone (relate_refs.expected_relate on the oracle's decode; tests/stream_refs.py and test_stream_histogram_cpu for the siblings),
through the C entry point, on tables that lie in one buffer of sentinels which is compared whole.  The material, the steps and the
runner are those of tests/stream_history.py, tests/test_gpu_stream_history.py and tests/test_gpu_stream_histogram_history.py."""
import numpy as np
import pytest

import linne_amd
import stream_history as sh
from relate_refs import expected_relate
from test_gpu_stream_histogram_history import hstep, run_histogram
from test_gpu_stream_history import SENT64, Dev, hold, last_error, mat, windows_array  # noqa: F401  (mat is a fixture)

pytestmark = pytest.mark.gpu

BUCKETS = [0, 441, 7, 1, 300, 64, 256]                          # cycled through the windows of a step from the step's own offset
GAP = 2


def rstep(wins, k=0, gf=0, note="", **kw):
    s = {"call": "relate", "wins": list(wins), "gf": gf, "note": note, "specs": [BUCKETS[(k + i) % len(BUCKETS)] for i in range(len(wins))]}
    s.update(kw)
    return s


def run_relate(c, dev, s, mat):
    """the step's call through its C entry point; asserts its codes and every word of the buffer its tables lie in"""
    import torch
    W = len(s["wins"])
    codes = s.get("codes") or [sh.OK] * W
    w = windows_array(dev, s)
    offs, at, sizes = [], GAP, []
    for (name, first, n), b in zip(s["wins"], s["specs"]):
        nch, nb = dev.x[name].header["num_channels"], (1 if b == 0 else -(-n // b))
        offs.append(at)
        sizes.append(4 * (nch * (nch + 1) // 2) * nb)
        at += sizes[-1] + GAP
    buf = torch.full((at,), SENT64, dtype=torch.int64, device="cuda")
    sp = (linne_amd.RelateSpec * W)()
    for j, ((name, first, n), b) in enumerate(zip(s["wins"], s["specs"])):
        sp[j].bucket_samples, sp[j].d_out, sp[j].pair_stride = b, buf.data_ptr() + 8 * offs[j], (1 if b == 0 else -(-n // b))
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_RelateWindowsDevice(c.h, w, sp, W, s["gf"])
    text = last_error(c)
    if "raises" in s:
        assert ret == s["raises"] and text and not text.startswith("window "), (ret, text)
        return
    assert [w[j].result for j in range(W)] == codes, ([w[j].result for j in range(W)], text)
    bad = [j for j in range(W) if codes[j] != sh.OK]
    assert ret == (codes[bad[0]] if bad else sh.OK), (ret, text)
    assert text.startswith(f"window {bad[0]}: ") if bad else text == "", text
    want = np.full(at, SENT64, dtype=np.int64)
    for j, ((name, first, n), b) in enumerate(zip(s["wins"], s["specs"])):
        if codes[j] == sh.OK:
            want[offs[j]:offs[j] + sizes[j]] = np.ascontiguousarray(expected_relate(mat.full[name], first, n, b)).view(np.int64).reshape(-1)
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        where = [j for j in range(W) if not np.array_equal(got[offs[j]:offs[j] + sizes[j]], want[offs[j]:offs[j] + sizes[j]])]
        raise AssertionError(f"the tables of windows {where} of {s['wins']} differ from the reference" if where else "a sentinel around the tables was overwritten")


def runner(s, mat):
    if s["call"] == "relate":
        return lambda c_, dev_, s=s: run_relate(c_, dev_, s, mat)
    if s["call"] == "histogram":
        return lambda c_, dev_, s=s: run_histogram(c_, dev_, s, mat)
    return None


def run_steps(ctx_env, mat, steps, tag, names=None):
    with ctx_env({}) as c:
        dev = Dev(c, mat, names)
        for i, s in enumerate(steps):
            hold(ctx_env, mat, c, dev, s, f"{tag}, step {i}", run=runner(s, mat))
            if "raises" not in s and not s.get("codes"):
                assert last_error(c) == ""
        dev.close()


def windows_of(k):
    """an anchor over whole blocks of the largest shape and sh.SPANS on four of the smaller streams, rotated from call to call"""
    return [("loud", 1024, (9 - k % 3) * 1024 - 24)] + [(sh.SMALL_STREAMS[(k + i) % 5], a, n) for i, (a, n) in enumerate(sh.SPANS)]


def test_before_and_after_every_other_consumer(ctx_env, mat):
    steps = [rstep(windows_of(0), k=0, note="the context's first call")]
    for k, call in enumerate(sh.CONSUMERS + ["histogram"], 1):
        sibling = hstep(windows_of(2 * k), k=k) if call == "histogram" else sh.step(call, windows_of(2 * k), k=k)
        sibling["note"] = "behind the relate call: its accumulators or samples where the relate records lay"
        steps.append(sibling)
        steps.append(rstep(windows_of(2 * k + 1), k=3 * k, gf=k % 2, note=f"behind {call}: its records where that call's accumulators or scratch lay"))
    run_steps(ctx_env, mat, steps, "relate between the siblings")


def test_large_then_small_then_large_again(ctx_env, mat):
    name = "mixed"
    r = sh.largest_block(mat, name)
    first = mat.tables(name)[1][r]
    whole, small = [(name, 0, sh.num_samples(name))], [(name, first + 70, 64)]
    steps = [rstep(whole, specs=[0], note="grows the scratch: samples of the whole stream, the slots of one long bucket"),
             rstep(small, specs=[7], note="its records begin inside the whole-stream call's samples"),
             rstep(whole, specs=[441], gf=1, note="many passes in one scratch, its records where the small call's lay"),
             rstep(small, specs=[7], note="the same 64 samples again: the same answer"),
             rstep(whole, specs=[0], note="and the whole stream as at first")]
    rng = np.random.default_rng(12)
    wins = []
    for i in range(64):
        nm = sh.NAMES[i % 6]
        a = int(rng.integers(0, sh.num_samples(nm) - 900))
        wins.append((nm, a, int(rng.integers(1, 900))))
    steps += [rstep(wins, k=1, note="64 windows of every shape: long lists, records of every window"),
              rstep([(name, first + 5, 150)], k=3, note="one window: its records inside the 64 windows' samples"),
              rstep(wins, k=4, note="the 64 windows with other bucket lengths")]
    run_steps(ctx_env, mat, steps, "large, small, large")


def test_a_good_call_behind_a_failing_one(ctx_env, mat):
    bl = mat.tables("loud")
    k, r = mat.crc_block, mat.rice_block
    good = [("mixed", 100, 900), ("three", 300, 1000)]
    after = [("loud", 2000, 3000), ("mixed", 500, 2000), ("three", 0, 1500)]
    steps = [rstep([good[0], ("loud/rice", bl[1][r] + 10, 700), ("loud/rice", bl[1][r - 1] + 10, 700), good[1]], k=1, codes=[sh.OK, sh.NG, sh.OK, sh.OK],
                   note="a window over a block whose Rice codes do not end where they should: its fail word is set on the device, its records are not committed"),
             rstep(after, k=2, note="a good call behind it"),
             rstep([("loud/crc", bl[1][k] + 3, 600), good[0], ("loud/crc", 0, bl[1][k] - 24), ("loud", 1, sh.num_samples("loud"))], k=2,
                   codes=[sh.CORRUPTION, sh.OK, sh.OK, sh.INVALID_ARGUMENT], note="windows refused on the host, the others run"),
             rstep(after, k=5, gf=2, note="a good call behind it"),
             rstep([(nm, 0, 50) for nm in mat.tiny], k=3, raises=sh.NG, note="65 stream shapes: the call is refused as a whole"),
             rstep(after, k=0, note="a good call behind it"),
             sh.step("measure", after, k=1, note="and a sibling behind that")]
    with ctx_env({}) as c:
        dev = Dev(c, mat).need(mat.tiny)
        for i, s in enumerate(steps):
            hold(ctx_env, mat, c, dev, s, f"behind failures, step {i}", run=runner(s, mat))
        assert last_error(c) == ""
        dev.close()
