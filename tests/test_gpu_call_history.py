"""A context's answers do not depend on the calls before it (-m gpu).

Every scenario of tests/call_history.py runs its steps in order on ONE context (or one API handle), and every step's output is held
bit for bit to the oracle's answer for that step's input alone -- residual, parameter record and statistics of every frame, the way
test_gpu_batch_forms.check_encode does it; streams to oracle.encode_whole / decode_whole; the one-handle sequence to the bytes the
real reference wrote for the same sequence (tests/golden/reference_answers.json).  What is pinned is the state a LINNEAmdContext
carries from call to call: the resident class tables and their cumulative offsets (build_classes), the pinned metadata ring, the
buffers that grow, the modes that stay set, the per-call knobs, and LINNEEncoder.parcor_state.

When a step differs from the oracle, the same call is made once more on a fresh context and the failure says whether that one
agrees with the oracle: if it does, the history is to blame.
"""
import numpy as np
import pytest

import call_history as ch
import linne_amd
from refs import digest
from test_gpu_batch_forms import check_decode, check_encode, marked

pytestmark = pytest.mark.gpu


held = ch.held      # (the oracle's answers of a step as test_gpu_batch_forms.OracleBatch, the batch), cached over the module


def call(c, step, monkeypatch):
    """the step's setters, then its encode call under its knobs"""
    for name, value in step["set"]:
        getattr(c, name)(value)
    with monkeypatch.context() as m:
        for k, v in step["env"].items():
            m.setenv(k, v)
        return c.encode_frames_host(c.shape(*step["shape"]), ch.frames_of(step), step["ns"])


def differs(check):
    """the failure's text if the check fails, else None"""
    try:
        check()
    except (AssertionError, pytest.fail.Exception) as e:
        return str(e)
    return None


def on_a_fresh_context(ctx_env, oracle, monkeypatch, step):
    with ctx_env({}) as c:
        c.set_af_iterations(step["af"])
        c.set_learning(bool(step["learn"]))
        out = call(c, dict(step, set=()), monkeypatch)
    ob, batch = held(oracle, step)
    bad = differs(lambda: check_encode(ob, batch, *out, "fresh"))
    return ("the same call on a fresh context differs from the oracle too: the history is not (alone) to blame" if bad
            else "the same call on a fresh context AGREES with the oracle: the calls before this one are to blame")


def hold(ctx_env, oracle, monkeypatch, step, out, where):
    ob, batch = held(oracle, step)
    bad = differs(lambda: check_encode(ob, batch, *out, where))
    if bad:
        pytest.fail(f"{bad}\n{where}: {on_a_fresh_context(ctx_env, oracle, monkeypatch, step)}")


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def run(ctx_env, oracle, monkeypatch, steps, tag):
    outs = []
    with ctx_env({}) as c:
        for i, s in enumerate(steps):
            out = call(c, s, monkeypatch)
            hold(ctx_env, oracle, monkeypatch, s, out, f"{tag}, step {i} ({s['name']})")
            outs.append(out)
    return outs


def test_class_table_grows_call_after_call(ctx_env, oracle, monkeypatch):
    """scenario 1: {2048}, {2048, 777}, {2048, 1001, 129}, {2048}, {777}, {1001, 777} tail first, at 2 channels, 16 bits, -m 7, MS:
    classes appended by earlier calls serve later ones, earlier classes survive every re-upload of the tables"""
    run(ctx_env, oracle, monkeypatch, ch.scenario1(), "table grows")


def test_table_overflow_and_restart(ctx_env, oracle, monkeypatch):
    """scenario 2: 10 lengths, 10 others (the table starts over), three + three of them (appended), 16 in one call (starts over),
    the first call again (its answer again), a call that finds everything"""
    steps = ch.scenario2()
    outs = run(ctx_env, oracle, monkeypatch, steps, "table overflows")
    assert same(outs[4], outs[0]), "E repeats A's frames and must give A's answer"


def test_shape_changes(ctx_env, oracle, monkeypatch):
    """scenario 3: bits, MS, preset (same layers), block, then every field at once, twice, then the first shape again"""
    run(ctx_env, oracle, monkeypatch, ch.scenario3(), "shape changes")


def test_modes_switched_on_and_off(ctx_env, oracle, monkeypatch):
    """scenario 4: -a 1, -l, the search capture and the timing, each switched on for one call and off again; the calls with a mode
    on are held to the oracle with the same setting, the plain calls between them all give the first one's answer"""
    steps = ch.scenario4()
    outs = run(ctx_env, oracle, monkeypatch, steps, "modes")
    plain = [o for s, o in zip(steps, outs) if s["name"] == "plain"]
    assert len(plain) == 5
    for i, o in enumerate(plain[1:]):
        assert same(o, plain[0]), f"plain call {i + 1} differs from the first"


def test_kernel_forms_take_turns(ctx_env, oracle, monkeypatch):
    """scenario 5: a one-frame, a 40-frame and a one-frame call, then default / hist + fwd_loss + stats_rows / default on loud 24-bit
    material (k_prep_slow's row list) / prep_general on quiet material / unsorted alternating lengths / default, over one arena"""
    run(ctx_env, oracle, monkeypatch, ch.scenario5(), "forms take turns")


def test_more_calls_in_flight_than_the_ring_has_slots(ctx_env, oracle, monkeypatch):
    """scenario 6: 12 encode_frames and 3 decode_frames calls on device tensors, back to back on a context with its own stream, one
    synchronize() at the end.  Context.encode_frames / decode_frames only enqueue (they drain torch's stream, on which nothing is
    pending here, never the context's), every call has its own tensors and its own length list; only the first call waits for
    the device (it uploads the class tables of all four lengths).  The last call is larger than the fourteen before it: the class
    index buffer grows (ensure_buf) while they are queued."""
    import torch
    steps = ch.scenario6()
    frames = [ch.frames_of(s) for s in steps]
    obs = [held(oracle, s) for s in steps]
    tens = []
    for s, x, (ob, batch) in zip(steps, frames, obs):
        F, nch, block = x.shape
        if s["op"] == "encode":
            tens.append((torch.from_numpy(x).cuda(), (torch.zeros((F, nch, block), dtype=torch.int32, device="cuda"),
                                                       torch.zeros((F, nch, linne_amd.PARAM_WORDS), dtype=torch.int32, device="cuda"),
                                                       torch.zeros((F, nch, linne_amd.STAT_WORDS), dtype=torch.float64, device="cuda"))))
        else:
            tens.append((torch.from_numpy(marked(ob.res[ob.key], s["ns"], block)).cuda(), torch.from_numpy(np.ascontiguousarray(ob.prm[ob.key])).cuda()))
    torch.cuda.synchronize()
    with ctx_env({}) as c:
        shape = c.shape(*ch.S1)
        for s, t in zip(steps, tens):
            if s["op"] == "encode":
                c.encode_frames(shape, t[0], s["ns"], out=t[1])
            else:
                c.decode_frames(shape, t[0], t[1], s["ns"])
        c.synchronize()
        got = [tuple(o.cpu().numpy() for o in t[1]) if s["op"] == "encode" else t[0].cpu().numpy() for s, t in zip(steps, tens)]
    for i, (s, x, (ob, batch), g) in enumerate(zip(steps, frames, obs, got)):
        where = f"in flight, call {i} ({s['op']})"
        if s["op"] == "encode":
            hold(ctx_env, oracle, monkeypatch, s, g, where)
        else:
            bad = differs(lambda: check_decode(g, marked(x, s["ns"], ch.S1[2]), s["ns"], ch.S1[2], where))
            if bad:
                with ctx_env({}) as c2:
                    alone = c2.decode_frames_host(c2.shape(*ch.S1), marked(ob.res[ob.key], s["ns"], ch.S1[2]), ob.prm[ob.key], s["ns"])
                ok = np.array_equal(alone, marked(x, s["ns"], ch.S1[2]))
                pytest.fail(f"{bad}\n{where}: the same call alone on a fresh context {'AGREES with the oracle: the calls around it are to blame' if ok else 'differs too'}")


def test_entry_points_mixed_on_one_context(ctx_env, oracle, monkeypatch):
    """scenario 7: encode_frames_host, decode_frames_host of another shape, rice_plan + rice_emit, encode_stream, index_stream +
    decode_stream of 100 samples, of the whole stream (its scratch grows), of the 100 samples again, decode_windows over two streams,
    and the first call again, which must give the first answer"""
    import torch
    s7 = ch.scenario7()
    first, dstep = s7["first"], s7["decode"]
    (xa, *argsa), (xb, *argsb) = ch.stream_inputs()
    want_a, want_b = oracle.encode_whole(xa, *argsa), oracle.encode_whole(xb, *argsb)
    with ctx_env({}) as c:
        out1 = call(c, first, monkeypatch)
        hold(ctx_env, oracle, monkeypatch, first, out1, "mixed, encode_frames_host")
        ob, _ = held(oracle, dstep)
        block = dstep["shape"][2]
        dec = c.decode_frames_host(c.shape(*dstep["shape"]), marked(ob.res[ob.key], dstep["ns"], block), ob.prm[ob.key], dstep["ns"])
        check_decode(dec, marked(ch.frames_of(dstep), dstep["ns"], block), dstep["ns"], block, "mixed, decode_frames_host")
        # the Rice stage over the oracle's residual of the first step, against the oracle's coder
        ob1, _ = held(oracle, first)
        res, ns, shape = np.ascontiguousarray(ob1.res[ob1.key]), first["ns"], c.shape(*first["shape"])
        d_res = torch.from_numpy(res).cuda()
        plan = c.rice_plan(shape, d_res, ns)
        packed, offsets = c.rice_emit(shape, d_res, plan)
        c.synchronize()
        plan, packed, off = plan.cpu().numpy(), packed.cpu().numpy(), offsets.cpu().numpy().view(np.uint32)
        NB = linne_amd.RICE_PLAN_NBITS
        nbits = plan[:, :, NB:NB + 4].copy().view(np.uint32)[:, :, 0]
        emitted = 0
        for f in range(res.shape[0]):
            for chn in range(res.shape[1]):
                if plan[f, chn, 1]:
                    continue                                      # (left to the host's search)
                code, bits = oracle.rice_encode(res[f, chn, :int(ns[f])])
                cf = f * res.shape[1] + chn
                assert int(nbits[f, chn]) == bits and off[cf] != 0xFFFFFFFF, f"mixed, rice_plan: frame {f} ch {chn}"
                assert np.array_equal(packed[int(off[cf]):int(off[cf]) + len(code)], np.frombuffer(code, dtype=np.uint8)), f"mixed, rice_emit: frame {f} ch {chn}"
                emitted += 1
        assert emitted >= 4, "the device planned hardly any code: the step tested nothing"
        # streams
        sa = c.encode_stream(xa, *argsa)
        assert bytes(sa.cpu().numpy()) == want_a, "mixed, encode_stream differs from the oracle's stream"
        ia = c.index_stream(sa)
        small = lambda: c.decode_stream(sa, 1500, 100, index=ia).cpu().numpy()      # noqa: E731
        assert np.array_equal(small(), xa[:, 1500:1600]), "mixed, decode_stream of 100 samples"
        assert np.array_equal(c.decode_stream(sa, index=ia).cpu().numpy(), xa), "mixed, decode_stream of the whole stream"
        assert np.array_equal(small(), xa[:, 1500:1600]), "mixed, decode_stream of the 100 samples again"
        sb = torch.from_numpy(np.frombuffer(want_b, dtype=np.uint8).copy()).cuda()
        ib = c.index_stream(sb)
        wins = [(sa, ia, 1000, 2100, xa), (sb, ib, 2000, 3000, xb), (sa, ia, 0, None, xa), (sb, ib, xb.shape[1] - 50, 50, xb), (sa, ia, 7 * 1024 - 5, 305, xa)]
        pcm = c.decode_windows([w[:4] for w in wins])
        for i, ((_, _, a, n, x), p) in enumerate(zip(wins, pcm)):
            assert np.array_equal(p.cpu().numpy(), x[:, a:(a + n if n is not None else None)]), f"mixed, decode_windows: window {i}"
        ia.close()
        ib.close()
        out9 = call(c, first, monkeypatch)
        hold(ctx_env, oracle, monkeypatch, first, out9, "mixed, the first call again")
        assert same(out9, out1)


def test_after_a_refused_call(ctx_env, oracle, monkeypatch):
    """scenario 8: a length of 0, a length above the block, 17 distinct lengths, preset 8, a block not longer than a layer's order,
    MS with one channel -- each raises LinneAmdError with its LINNEApiResult, and the good calls right after it, of the same shape
    and of another, give the oracle's answer"""
    with ctx_env({}) as c:
        for g in ch.good8(6):
            hold(ctx_env, oracle, monkeypatch, g, call(c, g, monkeypatch), "before any refusal")
        for i, (name, shape, ns, code) in enumerate(ch.scenario8()):
            x = np.full((len(ns), shape[0], shape[2]), 100, dtype=np.int32)
            with pytest.raises(linne_amd.LinneAmdError) as e:
                c.encode_frames_host(c.shape(*shape), x, np.array(ns, dtype=np.uint32))
            assert e.value.code == code, f"{name}: {e.value} (code {e.value.code}, {code} documented)"
            for g in ch.good8(i):
                hold(ctx_env, oracle, monkeypatch, g, call(c, g, monkeypatch), f"after '{name}', {g['shape']}")


def test_one_handle_many_streams(product, oracle, reference):
    """scenario 9: EncodeWhole (16-bit stereo), SetEncodeParameter to 24-bit mono, EncodeWhole, back, five EncodeBlock calls,
    EncodeWhole on ONE LINNEEncoder handle: the bytes the real reference wrote doing the same on one of its handles (recorded); the
    block that opens streams 1, 2 and 3 is COMPRESS with the Q2 value the stream before it left on the handle and RAW without it
    (test_call_history_cpu.py).  Then all four streams, formats alternating, through ONE LINNEDecoder handle: the inputs"""
    xs = ch.handle_inputs()
    streams = ch.handle_sequence(product)
    fmt = [ch.STEREO9, ch.MONO9, None, ch.STEREO9]
    for i, (x, s) in enumerate(zip(xs, streams)):
        rec = reference.answers[ch.handle_key(i, x)]
        if digest(s) != {"bytes": rec["bytes"], "sha256": rec["sha256"]}:
            alone = ""
            if fmt[i]:
                nch, bits, rate, block, preset, ms = fmt[i]
                fresh = product.encode_whole(x, bits, rate, block, preset, ms)
                agrees = fresh == oracle.encode_whole(x, bits, rate, block, preset, ms)
                alone = (f"; a fresh handle's EncodeWhole of it {'AGREES with' if agrees else 'differs from'} the oracle's fresh encode and "
                         f"{'equals' if fresh == s else 'differs from'} the used handle's bytes")
            pytest.fail(f"stream {i} of the one-handle sequence: {len(s)} bytes, block types {ch.block_types(s)}; the reference wrote "
                        f"{rec['bytes']} bytes, block types {rec['block_types']}{alone}")
    for i, (ret, pcm) in zip(ch.DECODE_ORDER9, ch.decode_through_one_handle(product, streams)):
        assert ret == 0 and np.array_equal(pcm, xs[i]), f"one decoder handle: stream {i} (return {ret})"
