"""The scenarios of tests/call_history.py are what they claim to be, checked without a GPU: the class-table branches they are
written for are taken at the intended steps (by a replay of build_classes' bookkeeping), the refused length list has 17 lengths,
every oracle answer decodes to its input again, the plain steps of the mode scenario have one answer, and the reference's recorded
answers for the one-handle sequence are all there."""
import time

import numpy as np

import call_history as ch


def test_scenario1_appends_then_reuses():
    steps = ch.scenario1()
    got = ch.replay_classes(ch.calls_of(steps))
    assert [b for b, _ in got] == ch.S1_BRANCHES
    assert [ch.set_of(s["ns"]) for s in steps] == [{2048}, {2048, 777}, {2048, 1001, 129}, {2048}, {777}, {1001, 777}]
    assert got[-1][1] == [2048, 777, 1001, 129], "classes keep the slot they were appended at"
    assert ch.distinct(steps[5]["ns"])[0] == 1001 and steps[5]["ns"][0] != ch.S1[2], "the last call opens with a tail"
    assert ((1001 + 7) // 8 * 8) // 16 % 2 == 1, "1001 has odd unit lengths (quirk Q1)"
    for s in steps:
        assert min(s["ns"]) >= 129, "above the longest layer's order"


def test_scenario2_overflows_and_starts_over():
    steps = ch.scenario2()
    got = ch.replay_classes(ch.calls_of(steps))
    assert [b for b, _ in got] == ch.S2_BRANCHES
    A, B, C, D, E, F = (ch.distinct(s["ns"]) for s in steps)
    assert len(A) == len(B) == 10 and not set(A) & set(B) and len(A) + len(B) > ch.MAXCLS
    assert got[1][1] == B, "B's lengths replace A's"
    assert len(set(C) & set(A)) == 3 and len(set(C) & set(B)) == 3 and got[2][1] == B + C[:3], "three of A's are appended behind B's"
    assert len(D) == ch.MAXCLS and 0 < len(set(D) & set(got[2][1])) < ch.MAXCLS and got[3][1] == D
    assert E == A and got[4][1] == A
    assert np.array_equal(ch.frames_of(steps[4]), ch.frames_of(steps[0])), "E repeats A's frames exactly"
    assert set(F) <= set(A)
    assert min(min(s["ns"]) for s in steps) >= 129


def test_scenario3_changes_one_field_at_a_time_then_all():
    steps = ch.scenario3()
    assert [b for b, _ in ch.replay_classes(ch.calls_of(steps))] == ch.S3_BRANCHES
    shapes = [s["shape"] for s in steps]
    for a, b in zip(shapes[:5], shapes[1:5]):
        assert sum(x != y for x, y in zip(a, b)) == 1, (a, b)
    for a, b, k in zip(shapes[4:7], shapes[5:8], (2, 4, 4)):
        assert sum(x != y for x, y in zip(a, b)) >= k, (a, b)
    assert shapes[0] == shapes[-1] and all(777 in ch.set_of(s["ns"]) for s in steps)


def test_scenario6_wraps_the_ring_with_slots_of_one_layout():
    steps = ch.scenario6()
    ops = [s["op"] for s in steps]
    assert ops.count("encode") == 12 and ops.count("decode") == 3 and len(steps) > ch.META
    assert [len(s["ns"]) for s in steps] == [ch.F6] * (len(steps) - 1) + [ch.F6_LAST], "the last call makes d_clsidx grow with 14 calls queued"
    assert steps[-1]["op"] == "encode" and ch.set_of(steps[-1]["ns"][:8]) == {ch.S1[2]} and ch.set_of(steps[-1]["ns"]) == set(ch.POOL6)
    for i in range(ch.META, len(steps)):
        assert ops[i] == ops[i - ch.META], "a slot is taken again by a call of the same kind"
        assert not np.array_equal(steps[i]["ns"], steps[i - ch.META]["ns"]), "and holds other lengths then"
    got = ch.replay_classes(ch.calls_of([s for s in steps if s["op"] == "encode"]))
    assert [b for b, _ in got] == ["first"] + ["reuse"] * 11, "only the first call waits for the device (to upload the tables)"


def test_scenario8_refused_lists():
    cases = {name: (shape, ns, code) for name, shape, ns, code in ch.scenario8()}
    assert len(cases) == 6
    shape, ns, code = cases["17 distinct lengths"]
    assert len(set(ns)) == 17 == ch.MAXCLS + 1 and all(0 < n <= shape[2] for n in ns)
    assert 0 in cases["a length of 0"][1] and max(cases["a length above the block"][1]) == ch.S8[2] + 1
    assert cases["preset 8"][0][3] == 8 and cases["MS with one channel"][0][0] == 1 and cases["MS with one channel"][0][4]
    assert cases["a block not longer than a layer's order"][0][2] <= 64


def test_scenario5_loud_then_quiet():
    steps = ch.scenario5()
    loud = [i for i, s in enumerate(steps) if s["kind"] == "loud"]
    assert len(loud) == 1 and steps[loud[0] + 1]["kind"] == "quiet"
    assert ch.inexact_rows(steps[loud[0]]) >= 6 and ch.inexact_rows(steps[loud[0] + 1]) == 0
    assert [len(s["ns"]) for s in steps[:3]] == [1, 40, 1]
    assert not steps[0]["env"] and not steps[3]["env"] and not steps[-1]["env"]


def test_every_oracle_answer_round_trips_and_the_plain_steps_agree(oracle):
    """OracleBatch decodes every answer with the oracle's own synthesis as it computes it; the CPU time of all of them is printed"""
    t0, w0 = time.process_time(), time.time()
    for k, make in ch.ENCODE_SCENARIOS.items():
        for s in make():
            a, _ = ch.held(oracle, s)
            x = ch.frames_of(s)
            for f, n in enumerate(s["ns"]):
                assert np.array_equal(a.dec[a.key[f], :, :int(n)], x[f, :, :int(n)]), (k, s["name"], f)
    for s in list(ch.scenario7().values()) + [g for i in range(7) for g in ch.good8(i)]:
        ch.held(oracle, s)
    plain = [s for s in ch.scenario4() if s["name"] == "plain"]
    assert len(plain) == 5
    first, _ = ch.held(oracle, plain[0])
    for s in plain[1:]:
        a, _ = ch.held(oracle, s)
        assert np.array_equal(a.res[a.key], first.res[first.key]) and np.array_equal(ch.frames_of(s), ch.frames_of(plain[0]))
    modes = {s["name"]: s for s in ch.scenario4() if s["name"] != "plain"}
    base, _ = ch.held(oracle, modes["capture on"])
    for name in ("-a 1", "-l"):
        a, _ = ch.held(oracle, modes[name])
        assert not np.array_equal(a.res[a.key], base.res[base.key]), f"{name} changes nothing on this input: the step would test nothing"
    for x, bits, rate, block, preset, ms in ch.stream_inputs():
        stream = oracle.encode_whole(x, bits, rate, block, preset, ms)
        ret, dec, _ = oracle.decode_whole(stream)
        assert ret == 0 and np.array_equal(dec, x)
    types = ch.block_types(oracle.encode_whole(*ch.stream_inputs()[0]))
    assert {0, 1, 2} <= set(types), types
    print(f"{len(ch.CACHE)} oracle runs, {time.process_time() - t0:.1f} s of CPU time, {time.time() - w0:.1f} s of wall time")


def test_the_recorded_handle_sequence_is_complete_and_depends_on_the_carried_value(oracle, reference):
    """the reference's four streams off one handle are recorded, each with COMPRESS, SILENT and RAW blocks; the block that opens
    streams 1, 2 and 3 -- the first one after each SetEncodeParameter, the first EncodeBlock call, the first block of the last
    EncodeWhole -- is COMPRESS off the used handle and RAW off a fresh one (the oracle's): an encoder that drops the carried Q2
    value at any of these points writes other bytes.  For stream 3, whose format is stream 2's, the oracle itself shows both: one
    oracle handle fed stream 2's blocks and then this block writes it COMPRESS, a fresh one RAW."""
    xs = ch.handle_inputs()
    assert len(xs) == 4 and sum(ch.BLOCKS9) == xs[2].shape[1]
    recs = []
    for i, x in enumerate(xs):
        rec = reference.answers.get(ch.handle_key(i, x))
        assert rec and rec["bytes"] > 30 and len(rec["sha256"]) == 64, f"stream {i} of the one-handle sequence is not recorded"
        assert set(rec["block_types"]) == {0, 1, 2}, f"stream {i}: COMPRESS, SILENT and RAW blocks"
        assert rec["block_types"][-1] == 0, f"stream {i} ends with a COMPRESS block: the next stream finds its value carried"
        recs.append(rec)
    for i in (1, 2, 3):
        nch, bits, rate, block, preset, ms = ch.FORMAT9[i]
        fresh = ch.block_types(oracle.encode_whole(xs[i][:, :block], bits, rate, block, preset, ms))
        assert recs[i]["block_types"][0] == 0 and fresh == [2], f"stream {i}: its first block is {recs[i]['block_types'][0]} off the used handle, {fresh} off a fresh one"
    nch, bits, rate, block, preset, ms = ch.STEREO9
    e = oracle.encoder(nch, bits, rate, block, preset, ms)
    prog = 0
    for n in ch.BLOCKS9:
        e.encode_block(xs[2][:, prog:prog + n])
        prog += n
    carried = e.encode_block(xs[3][:, :block])[0]
    e.close()
    assert carried[8] == 0, "one oracle handle over stream 2's blocks, then the first block of stream 3: COMPRESS"
    assert sorted(set(ch.DECODE_ORDER9)) == [0, 1, 2, 3]
    for a, b in zip(ch.DECODE_ORDER9, ch.DECODE_ORDER9[1:]):
        assert xs[a].shape[0] != xs[b].shape[0], "the decoder handle alternates between the formats"
