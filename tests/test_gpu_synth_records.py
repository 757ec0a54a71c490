"""Every decode path on parameter records no encoder writes (tests/synth_records.py: any power-of-two unit count in every layer,
any shift >= 1, any int8 coefficient, any pre-emphasis state, cascades that wrap int32), bit for bit against the oracle's PCM,
which tests/test_synth_records_cpu.py and the hash check below hold to the real reference decoder's recorded answers
(tests/golden/synth_records.json).  Every case of the table is compared on every path and in every synthesis form; none is
skipped."""
import json
import os

import numpy as np
import pytest

import synth_records as sr
from test_gpu_parity import _force_decode_form
from test_synth_records_cpu import GOLDEN, _generator

pytestmark = pytest.mark.gpu

SHAPE_IDS = [s.name for s in sr.SHAPES]
SENTINEL = -123456


@pytest.fixture(scope="module")
def material(oracle):
    """per shape, computed once and never written to: the cases, their streams and the expected PCM (the oracle's synthesis of every
    record, checked here against the recorded reference answer for the stream of all cases)"""
    gen = _generator()
    with open(os.path.join(GOLDEN, "synth_records.json")) as f:
        gold = json.load(f)
    out = {}
    for shape, cases in sr.table().items():
        pcm = [sr.expected_pcm(shape, c) for c in cases]
        whole = np.concatenate(pcm + [np.zeros((shape.nch, sr.CLOSING_SAMPLES), dtype=np.int32)], axis=1)
        assert gen.fnv_planes(whole) == gold["shapes"][shape.name]["stream"]["fnv"], f"{shape.name}: the oracle's PCM is not the recorded reference's"
        for a in pcm + [whole]:
            a.setflags(write=False)
        out[shape] = {"cases": cases, "pcm": pcm, "whole": whole, "stream": sr.case_stream(shape, cases), "first": sr.case_offsets(cases)}
    return out


@pytest.mark.parametrize("kernel", ["wave", "lanes", "pipe", "rows", "rows4", "rows_nf", None])
@pytest.mark.parametrize("shape", sr.SHAPES, ids=SHAPE_IDS)
def test_frames_of_the_table_in_one_batch(ctx, material, monkeypatch, shape, kernel):
    """DecodeFramesHost on the whole table of a shape in one batch: frames of four lengths and every unit count side by side in a
    wave and in a 64-row block, in each synthesis form and in the one the batch-size rule picks; what lies behind a frame's n stays"""
    if kernel:
        _force_decode_form(monkeypatch, kernel)
    m = material[shape]
    cases = m["cases"]
    assert len(cases) <= 64
    res = np.stack([c.residual for c in cases])
    prm = np.stack([c.record for c in cases])
    ns = np.array([c.n for c in cases], dtype=np.uint32)
    for f, c in enumerate(cases):
        res[f, :, c.n:] = SENTINEL
    ctx.enable_timing(True)
    try:
        dec = ctx.decode_frames_host(ctx.shape(shape.nch, shape.bits, shape.block, shape.preset, shape.ms), res, prm, ns)
        ran = {k: ctx.last_launches(k) for k in (11, 30, 31, 32, 33, 34, 35, 36)}
    finally:
        ctx.enable_timing(False)
    compared = 0
    for f, c in enumerate(cases):
        assert np.array_equal(dec[f, :, :c.n], m["pcm"][f]), f"{c.name} (frame {f}, n = {c.n}): {_first_difference(dec[f, :, :c.n], m['pcm'][f])}"
        assert np.all(dec[f, :, c.n:] == SENTINEL), f"{c.name}: samples behind the frame's end were written"
        compared += 1
    assert compared == len(cases)
    # last: the form that was asked for ran (include/linne_amd.h LINNE_AMD_T_SYNTH*).  The throughput form moves samples in groups
    # of four, so a block of 1023 takes the lanes kernels under it
    rows = shape.block % 4 == 0
    fused = {33, 35} | ({36} if len(sr.PRESET_LAYERS[shape.preset]) == 3 else set())          # (36: a short layer behind the long one)
    want = {"wave": {11}, "pipe": {32}, None: {32}, "lanes": {30, 31}, "rows": fused if rows else {30, 31}, "rows4": fused if rows else {30, 31},
            "rows_nf": {33, 34, 36} if rows else {30, 31}}[kernel]
    assert {k for k, v in ran.items() if v} == want, f"launches by kind: {ran}"


def _first_difference(got, want):
    ch, s = np.argwhere(got != want)[0]
    return f"{int((got != want).sum())} samples differ, the first at channel {ch} sample {s}: {got[ch, s]} for {want[ch, s]}"


@pytest.mark.parametrize("shape", sr.SHAPES, ids=SHAPE_IDS)
def test_decode_whole_of_the_tables_streams(product, material, monkeypatch, shape):
    """LINNEDecoder_DecodeWhole with the CRC check on: Rice decoding on the device and on the host, groups of two blocks and the
    default, the lanes form, the throughput form and the batch-size rule's choice -- the reference's PCM every time"""
    m = material[shape]
    calls = 0
    for kernel in (None, "lanes", "rows"):
        with monkeypatch.context() as mp:
            if kernel:
                _force_decode_form(mp, kernel)
            for mode in ("1", "0"):
                mp.setenv("LINNE_AMD_DECODE_STREAM", mode)
                for group in ("2", None):
                    if group:
                        mp.setenv("LINNE_AMD_GROUP", group)
                    else:
                        mp.delenv("LINNE_AMD_GROUP", raising=False)
                    ret, dec = product.decode_whole(m["stream"], check_crc=1)
                    where = f"kernel {kernel}, LINNE_AMD_DECODE_STREAM={mode}, LINNE_AMD_GROUP={group}"
                    assert ret == 0, f"{where}: DecodeWhole -> {ret}"
                    assert np.array_equal(dec, m["whole"]), f"{where}: {_first_difference(dec, m['whole'])}"
                    calls += 1
    assert calls == 12


@pytest.mark.parametrize("shape", [s for s in sr.SHAPES if s.bits == 16 and "growth" in s.families], ids=lambda s: s.name)
def test_decode_whole_takes_the_int32_way_back_on_data(product, material, monkeypatch, shape):
    """a 16-bit stream whose samples leave the int16 range (the growth family's blocks alone): DecodeWhole succeeds and delivers the
    int32 samples -- the way back that only LINNE_AMD_DEBUG_NO_PCM16 reached"""
    assert "LINNE_AMD_DEBUG_NO_PCM16" not in os.environ
    m = material[shape]
    picks = [f for f, c in enumerate(m["cases"]) if c.family == "growth"]
    assert len(picks) == 4
    stream = sr.case_stream(shape, [m["cases"][f] for f in picks])
    want = np.concatenate([m["pcm"][f] for f in picks] + [np.zeros((shape.nch, sr.CLOSING_SAMPLES), dtype=np.int32)], axis=1)
    for f in picks:
        assert np.abs(m["pcm"][f].astype(np.int64)).max() > 32767
    for mode in ("1", "0"):
        monkeypatch.setenv("LINNE_AMD_DECODE_STREAM", mode)
        for group in ("2", None):
            if group:
                monkeypatch.setenv("LINNE_AMD_GROUP", group)
            else:
                monkeypatch.delenv("LINNE_AMD_GROUP", raising=False)
            ret, dec = product.decode_whole(stream, check_crc=1)
            assert ret == 0, f"LINNE_AMD_DECODE_STREAM={mode}, LINNE_AMD_GROUP={group}: DecodeWhole -> {ret}"
            assert np.array_equal(dec, want), f"LINNE_AMD_DECODE_STREAM={mode}, LINNE_AMD_GROUP={group}: {_first_difference(dec, want)}"


@pytest.mark.parametrize("shape", sr.SHAPES, ids=SHAPE_IDS)
def test_decode_stream_of_the_tables_streams(ctx, material, shape):
    """the resident path, whose parameters the DEVICE parses: the whole stream, and one range that starts and ends inside blocks"""
    m = material[shape]
    got = ctx.decode_stream(m["stream"]).cpu().numpy()
    assert got.shape == m["whole"].shape
    for f, c in enumerate(m["cases"]):
        a, b = int(m["first"][f]), int(m["first"][f + 1])
        assert np.array_equal(got[:, a:b], m["pcm"][f]), f"{c.name}: {_first_difference(got[:, a:b], m['pcm'][f])}"
    assert not got[:, int(m["first"][-1]):].any()
    lo, hi = int(m["first"][3]) + 77, int(m["first"][len(m["cases"]) - 2]) + 101
    got = ctx.decode_stream(m["stream"], lo, hi - lo).cpu().numpy()
    assert np.array_equal(got, m["whole"][:, lo:hi]), _first_difference(got, m["whole"][:, lo:hi])


def _tail_window(m, shape):
    """a window wholly inside the samples no layer synthesises: the frame of 1000 samples with 128 units in every layer"""
    f = next(f for f, c in enumerate(m["cases"]) if c.name.endswith("units/all128/n1000"))
    nl = len(sr.PRESET_LAYERS[shape.preset])
    assert (m["cases"][f].record[:, sr.PRM_UNITS:sr.PRM_UNITS + nl] == 128).all() and m["cases"][f].n == 1000
    return int(m["first"][f]) + 128 * (1000 // 128) + 20, 60          # inside [896, 1000) of the frame


@pytest.mark.parametrize("pair", [(0, 3), (1, 2), (4, 5)], ids=lambda p: f"{SHAPE_IDS[p[0]]}+{SHAPE_IDS[p[1]]}")
def test_decode_windows_over_two_of_the_tables_streams(ctx, material, pair):
    """ten windows over two streams in one call: inside one block, across block edges, across many blocks, wholly inside a frame's
    unsynthesised tail, and across the growth family's blocks where the shape has them"""
    import torch
    shapes = [sr.SHAPES[i] for i in pair]
    ms = [material[s] for s in shapes]
    streams = [torch.from_numpy(np.frombuffer(m["stream"], dtype=np.uint8).copy()).to("cuda:0") for m in ms]
    indexes = [ctx.index_stream(t) for t in streams]
    try:
        windows = []
        for k, (shape, m) in enumerate(zip(shapes, ms)):
            first, total = m["first"], m["whole"].shape[1]
            ranges = [_tail_window(m, shape), (int(first[5]) + 9, 200), (int(first[7]) - 13, 3000), (int(first[len(first) // 2]) - 1, 2),
                      (total - 700, 700)]
            grow = [f for f, c in enumerate(m["cases"]) if c.family == "growth"]
            if grow:
                ranges[1] = (int(first[grow[0]]) + 500, int(first[grow[-1]]) + 300 - int(first[grow[0]]) - 500)
            windows += [(k, lo, n) for lo, n in ranges]
        assert len(windows) >= 8
        got = ctx.decode_windows([(streams[k], indexes[k], lo, n) for k, lo, n in windows])
        for (k, lo, n), g in zip(windows, got):
            want = ms[k]["whole"][:, lo:lo + n]
            g = g.cpu().numpy()
            assert g.shape == want.shape and np.array_equal(g, want), f"{shapes[k].name} [{lo}, {lo + n}): {_first_difference(g, want)}"
    finally:
        for ix in indexes:
            ix.close()
