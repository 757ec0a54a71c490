"""The answers of the calls on resident .lnn streams do not depend on the calls the context served before (-m gpu).

Every scenario of tests/stream_history.py runs its steps in order on ONE fresh context, and every step's answer is held to its
reference -- the oracle's bytes and decode, the block walk of index_cases, the restatements of repair_cases and splice_cases, numpy,
Python integers and zlib.crc32 (tests/stream_refs.py) -- never to another run of the library.  The windows calls are made through
the C entry points on tables that lie in one buffer of sentinels, a sentinel record in front of, between and behind them, and the
whole buffer is compared.  What is pinned is what a LINNEAmdContext carries from call to call: the pinned and device lists, the
scratch with the consumers' accumulators behind it, the scan's and the splice's buffers, and the flags a wrapping call sets
("What the resident calls share").

When a step differs from its reference, the same call is made once more, alone, on a second fresh context, and the failure says
whether that one agrees with the reference: if it does, the history is to blame."""
from types import SimpleNamespace

import numpy as np
import pytest

import linne_amd
import stream_consumers as sc
import stream_history as sh
from stream_consumers import last_error, to_device

pytestmark = pytest.mark.gpu

SENT32 = -123456789
SENT64 = 0x5A5A5A5A5A5A5A5A
KINDS = range(max(sc.KIND.values()) + 1)     # every kernel kind of include/linne_amd.h


@pytest.fixture(scope="module")
def mat(oracle):
    return sh.material(oracle)


def as_bytes(t):
    return bytes(t.cpu().numpy())


class Dev:
    """the material on the device as one context sees it: the streams' bytes and the indexes that context built"""

    def __init__(self, c, mat, names=None):
        self.c, self.mat, self.t, self.x = c, mat, {}, {}
        self.need(sh.NAMES + ["loud/crc", "loud/rice"] if names is None else names)

    def need(self, names):
        new = [n for n in dict.fromkeys(names) if n not in self.x]
        if new:
            for n in new:
                self.t[n] = to_device(self.mat.data[n])
            for n, x in zip(new, self.c.index_streams([self.t[n] for n in new])):
                self.x[n] = x
        return self

    def close(self):
        for x in self.x.values():
            x.close()


def windows_array(dev, s):
    W = len(s["wins"])
    w = (linne_amd.Window * W)()
    for j, (name, first, n) in enumerate(s["wins"]):
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].d_pcm, w[j].pcm_stride, w[j].result = dev.x[name].h, dev.t[name].data_ptr(), first, n, None, 0, -1
    return w


def channels(dev, name):
    return dev.x[name].header["num_channels"]


def run_windows(c, dev, s, mat):
    """the step's call through its C entry point; asserts its codes, its answers and every byte of the buffer its tables lie in"""
    import torch
    codes = s.get("codes") or [sh.OK] * len(s["wins"])
    if "raises" in s:
        want = [None] * len(s["wins"])
    elif s["call"] in sh.LATER:                                  # (their references are the consumer table's, in want_buffer)
        want = [True if code == sh.OK else None for code in codes]
    else:
        want = sh.expected(s, mat)
    W, gf, lib = len(s["wins"]), s["gf"], linne_amd.lib
    w = windows_array(dev, s)
    nch = [channels(dev, name) for name, _, _ in s["wins"]]
    ns = [n for _, _, n in s["wins"]]
    answers = None
    if s["call"] == "place":
        offs, at = [], 3
        for C, n in zip(nch, ns):
            offs.append(at)
            at += C * n + 3
        buf = torch.full((at,), SENT32, dtype=torch.int32, device="cuda")
        for j in range(W):
            w[j].d_pcm, w[j].pcm_stride = buf.data_ptr() + 4 * offs[j], ns[j]
        torch.cuda.synchronize()
        ret = lib.LINNEAmd_DecodeWindowsDevice(c.h, w, W, gf)
        wbuf = np.full(at, SENT32, dtype=np.int32)
        for j in range(W):
            if want[j] is not None:
                wbuf[offs[j]:offs[j] + nch[j] * ns[j]] = want[j].reshape(-1)
        got = buf.cpu().numpy()
    elif s["call"] == "compare":
        pcms = [torch.from_numpy(np.ascontiguousarray(sh.held_pcm(s, j, mat)) if codes[j] == sh.OK else np.zeros((nch[j], ns[j]), np.int32)).cuda() for j in range(W)]
        diffs = (linne_amd.Diff * W)()
        for j in range(W):
            w[j].d_pcm, w[j].pcm_stride = pcms[j].data_ptr(), ns[j]
            diffs[j].num_differing, diffs[j].first_sample, diffs[j].first_channel = 99, 98, 97
        torch.cuda.synchronize()
        ret = lib.LINNEAmd_CompareWindowsDevice(c.h, w, None, diffs, W, gf)
        answers = [(int(d.num_differing), int(d.first_sample), int(d.first_channel)) for d in diffs]
        want_answers = [(99, 98, 97) if v is None else v for v in want]
        got = wbuf = None
    elif s["call"] in ("measure", "digest"):
        measure = s["call"] == "measure"
        words, dtype = (4, linne_amd.MEASURE_DTYPE) if measure else (2, linne_amd.DIGEST_DTYPE)
        nbs = [1 if b == 0 else -(-n // b) for n, b in zip(ns, s["buckets"])]
        offs, at = [], 1
        for C, nb in zip(nch, nbs):
            offs.append(at)
            at += (C if measure else 1) * nb + 1
        buf = torch.full((at, words), SENT64, dtype=torch.int64, device="cuda")
        sp = ((linne_amd.MeasureSpec if measure else linne_amd.DigestSpec) * W)()
        for j in range(W):
            sp[j].bucket_samples, sp[j].d_out = s["buckets"][j], buf.data_ptr() + 8 * words * offs[j]
            if measure:
                sp[j].channel_stride = nbs[j]
        torch.cuda.synchronize()
        ret = (lib.LINNEAmd_MeasureWindowsDevice if measure else lib.LINNEAmd_DigestWindowsDevice)(c.h, w, sp, W, gf)
        wbuf = np.full((at, words), SENT64, dtype=np.int64).view(dtype).reshape(at)
        for j in range(W):
            if want[j] is None:
                continue
            if measure:
                for ch, row in enumerate(want[j]):
                    for k, r in enumerate(row):
                        wbuf[offs[j] + ch * nbs[j] + k] = r
            else:
                for k, (crc, nbytes) in enumerate(want[j]):
                    wbuf[offs[j] + k] = (crc, 0, nbytes)
        got = buf.cpu().numpy().view(dtype).reshape(at)
    elif s["call"] in sh.LATER:
        # the bucket consumers' scaffold (stream_consumers.raw_call), the rows of a table adjacent and two sentinel words around it
        c_, fields = sc.CONSUMERS[s["call"]], [(f[0], f[1], int(f[2]), f[3]) if s["call"] == "histogram" else (f,) for f in s["specs"]]
        items = [(dev.t[name], dev.x[name], first, n, C, *f, None) for (name, first, n), C, f in zip(s["wins"], nch, fields)]
        tracks = [SimpleNamespace(full=mat.full[name]) for name, _, _ in s["wins"]]
        ret, results, got, offs, nbs = sc.raw_call(c_, c, items, gf, pad=0, gap=2)
        for j in range(W):
            w[j].result = results[j]
        wbuf = sc.want_buffer(c_, len(got), items, tracks, codes, offs, nbs, pad=0)
    else:
        offs, at = [], 1
        for cap in s["caps"]:
            offs.append(at)
            at += cap + 1
        buf = torch.full((at, 2), SENT64, dtype=torch.int64, device="cuda")
        sp, an = (linne_amd.QuietSpec * W)(), (linne_amd.Quiet * W)()
        for j in range(W):
            sp[j].threshold, sp[j].min_samples, sp[j].capacity, sp[j].d_out = s["thr"][j], s["mins"][j], s["caps"][j], buf.data_ptr() + 16 * offs[j]
            an[j].num_runs = an[j].quiet_samples = an[j].lead_samples = an[j].trail_samples = SENT64
        torch.cuda.synchronize()
        ret = lib.LINNEAmd_QuietWindowsDevice(c.h, w, sp, an, W, gf)
        answers = [(int(a.num_runs), int(a.quiet_samples), int(a.lead_samples), int(a.trail_samples)) for a in an]
        want_answers = [(SENT64,) * 4 if v is None else tuple(v[1:]) for v in want]
        wbuf = np.full((at, 2), SENT64, dtype=np.int64)
        for j in range(W):
            for k, r in enumerate(want[j][0] if want[j] is not None else []):
                wbuf[offs[j] + k] = r
        got = buf.cpu().numpy()
    text = last_error(c)
    if "raises" in s:
        assert ret == s["raises"] and text and not text.startswith("window "), (ret, text)
        return
    assert [w[j].result for j in range(W)] == codes, ([w[j].result for j in range(W)], text)
    bad = [j for j in range(W) if codes[j] != sh.OK]
    assert ret == (codes[bad[0]] if bad else sh.OK), (ret, text)
    assert text.startswith(f"window {bad[0]}: ") if bad else text == "", text
    if answers is not None:
        assert answers == want_answers, [j for j in range(W) if answers[j] != want_answers[j]]
    if wbuf is not None and got.tobytes() != wbuf.tobytes():
        where = [j for j in range(W) if want[j] is not None and got[offs[j]:(offs[j + 1] if j + 1 < W else len(got)) - 1].tobytes() != wbuf[offs[j]:(offs[j + 1] if j + 1 < W else len(got)) - 1].tobytes()]
        raise AssertionError(f"the tables of windows {where} of {s['wins']} differ from the reference" if where else "a sentinel around the tables was overwritten")


def run_other(c, dev, s, mat, memo):
    """the other resident calls of scenario (d)"""
    call = s["call"]
    if call == "set_verify":
        c.set_verify(s["on"])
    elif call == "index_streams":
        dev.need(n for n in s["streams"])
        got, codes = c.index_streams([dev.t[n] for n in s["streams"]], return_codes=True)
        tables = []
        for n, x, code in zip(s["streams"], got, codes):
            wcode, nb, want, failure = sh.expected_index(mat, n)
            assert code == wcode == sh.OK and x.num_blocks == nb, n
            t = [[int(v) for v in a] for a in x.blocks()]
            assert t == [list(a) for a in want], n
            assert x.failure() == failure, n
            tables.append((t, x.failure()))
            x.close()
        assert memo.setdefault(tuple(s["streams"]), tables) == tables          # the same streams later: the same indexes
        assert last_error(c) == ""
    elif call == "repair_streams":
        got, codes = c.repair_streams(s["streams"], return_codes=True)
        for i, (data, (stream, report), code) in enumerate(zip(s["streams"], got, codes)):
            out, rep = sh.expected_repair(data)
            assert code == sh.OK and as_bytes(stream) == out and report == rep, i
        assert last_error(c) == ""
    elif call == "encode_streams":
        got = c.encode_streams([(mat.pcm[n],) + (sh.SPEC[n][1], sh.RATE) + sh.SPEC[n][2:5] for n in s["tracks"]])
        for n, t in zip(s["tracks"], got):
            assert as_bytes(t) == mat.data[n], n
        assert last_error(c) == ""
    elif call == "splice_streams":
        splices = [[(dev.t[n], dev.x[n], lo, k) for n, lo, k in cuts] for cuts in s["cuts"]]
        if "raises" in s:
            with pytest.raises(linne_amd.LinneAmdError) as e:
                c.splice_streams(splices)
            assert e.value.code == s["raises"] and e.value.codes == [s["raises"]] * len(splices)
            return
        got = c.splice_streams(splices)
        for i, (cuts, t) in enumerate(zip(s["cuts"], got)):
            data, copied, encoded, pcm = sh.expected_splice(mat, cuts)
            assert as_bytes(t) == data and c.last_splice_blocks[i] == (copied, encoded), i
            ret, back = mat.oracle.decode_whole(data)[:2]
            assert ret == sh.OK and np.array_equal(back, pcm), i
        assert last_error(c) == ""
    else:
        run_windows(c, dev, s, mat)


def differs(check):
    """the failure's text if the check fails, else None"""
    try:
        check()
    except (AssertionError, pytest.fail.Exception) as e:
        return str(e) or repr(e)
    return None


def hold(ctx_env, mat, c, dev, s, where, run=None):
    run = run or (lambda c_, dev_: run_windows(c_, dev_, s, mat))
    bad = differs(lambda: run(c, dev))
    if bad:
        with ctx_env({}) as c2:
            dev2 = Dev(c2, mat, list(dev.x))
            again = differs(lambda: run(c2, dev2))
            dev2.close()
        pytest.fail(f"{where} ({s['call']}; {s['note']}): {bad}\nthe same call alone on a fresh context " +
                    (f"differs from its reference too ({again}): the history is not (alone) to blame" if again
                     else "AGREES with its reference: the calls before this one are to blame"))


def run_list(ctx_env, mat, steps, tag, c=None, dev=None):
    if c is not None:
        for i, s in enumerate(steps):
            hold(ctx_env, mat, c, dev, s, f"{tag}, step {i}")
        return
    with ctx_env({}) as c:
        dev = Dev(c, mat)
        run_list(ctx_env, mat, steps, tag, c, dev)
        dev.close()


def test_every_ordered_pair_of_consumers(ctx_env, mat):
    """scenario (a): 26 windows calls on one context, every ordered pair of place, compare, measure, digest and quiet adjacent once,
    consecutive calls on other streams with other buckets, thresholds and min_samples"""
    run_list(ctx_env, mat, sh.scenario_a(), "pairs")


@pytest.mark.parametrize("name", [f"b/{x}" for x in sh.ACCUMULATING] + [f"b/many/{x}" for x in sh.ACCUMULATING])
def test_large_then_small_then_large_again(ctx_env, mat, name):
    """scenario (b): a whole stream, 64 samples through another consumer, the whole stream in one-block passes, the 64 samples again;
    64 windows of every shape, then one window"""
    run_list(ctx_env, mat, sh.scenario_b(mat)[name], name)


@pytest.mark.parametrize("call", sh.LATER)
def test_before_and_after_every_other_consumer(ctx_env, mat, call):
    """histogram, then relate: before and after every consumer that came before it, on one context"""
    with ctx_env({}) as c:
        dev = Dev(c, mat)
        for i, s in enumerate(sh.scenario_between(call)):
            hold(ctx_env, mat, c, dev, s, f"{call} between the siblings, step {i}")
            assert last_error(c) == ""
        dev.close()


@pytest.mark.parametrize("call", sh.LATER)
def test_large_then_small_then_large_again_later(ctx_env, mat, call):
    with ctx_env({}) as c:
        dev = Dev(c, mat)
        for i, s in enumerate(sh.scenario_large_small_large(mat, call)):
            hold(ctx_env, mat, c, dev, s, f"{call} large, small, large, step {i}")
            assert last_error(c) == ""
        dev.close()


@pytest.mark.parametrize("call", sh.LATER)
def test_a_good_call_behind_a_failing_one(ctx_env, mat, call):
    with ctx_env({}) as c:
        dev = Dev(c, mat).need(mat.tiny)
        for i, s in enumerate(sh.scenario_behind_failures(mat, call)):
            hold(ctx_env, mat, c, dev, s, f"{call} behind failures, step {i}")
        assert last_error(c) == ""
        dev.close()


def test_after_failures(ctx_env, mat):
    """scenario (c): a window over a Rice-damaged block, windows that reach an index's fail_block, a window beyond the stream, a quiet
    table one record too small, a call of 65 stream shapes -- the good windows beside each, and behind each one good call of every
    consumer, with no error text left"""
    with ctx_env({}) as c:
        dev = Dev(c, mat).need(mat.tiny)
        for i, (fail, good) in enumerate(sh.scenario_c(mat)):
            hold(ctx_env, mat, c, dev, fail, f"failure {i}")
            for j, s in enumerate(good):
                hold(ctx_env, mat, c, dev, s, f"behind failure {i} ({fail['note']}), good call {j}")
                assert last_error(c) == ""
        dev.close()


def test_the_other_resident_calls_in_between(ctx_env, mat):
    """scenario (d): index 16 streams, repair one, index one, splice, repair three, encode verified and not, a refused splice, a good
    one, every windows consumer, index the 16 again.  With timing on, every call behind the refused splice makes the launches, kind
    by kind, that the same call makes alone on a fresh context"""
    memo = {}
    with ctx_env({}) as c:
        c.enable_timing(True)
        dev = Dev(c, mat).need(sh.SIXTEEN)
        for i, s in enumerate(sh.scenario_d(mat)):
            run = lambda c_, dev_, s=s, m=memo: run_other(c_, dev_, s, mat, m if c_ is c else {})      # noqa: E731
            hold(ctx_env, mat, c, dev, s, f"in between, step {i}", run)
            if s.get("count"):
                mine = [c.last_launches(k) for k in KINDS]
                with ctx_env({}) as c2:
                    c2.enable_timing(True)
                    dev2 = Dev(c2, mat).need(sh.SIXTEEN)
                    run_other(c2, dev2, s, mat, {})
                    alone = [c2.last_launches(k) for k in KINDS]
                    dev2.close()
                assert sum(alone) > 0 and mine == alone, (i, s["call"], {k: (a, b) for k, (a, b) in enumerate(zip(mine, alone)) if a != b})
        dev.close()


def test_an_index_outlives_the_scratch_it_was_built_beside(ctx_env, mat):
    """scenario (e): the indexes first, then all of scenario (b)'s growth on the same context, then the old indexes in a call of
    every consumer"""
    with ctx_env({}) as c:
        dev = Dev(c, mat)
        for name, steps in sh.scenario_b(mat).items():
            run_list(ctx_env, mat, steps, f"growth {name}", c, dev)
        run_list(ctx_env, mat, sh.scenario_e(), "old indexes", c, dev)
        dev.close()


def test_two_contexts_calls_alternating(ctx_env, mat):
    """scenario (f): two contexts of the device, A's call k followed by B's call k on other streams, from one thread"""
    list_a, list_b = sh.scenario_f()
    with ctx_env({}) as a, ctx_env({}) as b:
        dev_a, dev_b = Dev(a, mat), Dev(b, mat)
        for k, (sa, sb) in enumerate(zip(list_a, list_b)):
            hold(ctx_env, mat, a, dev_a, sa, f"context A, call {k}")
            hold(ctx_env, mat, b, dev_b, sb, f"context B, call {k}")
        dev_a.close()
        dev_b.close()
