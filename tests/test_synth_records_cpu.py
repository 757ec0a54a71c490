"""The case table of tests/synth_records.py -- COMPRESS blocks with parameter records no encoder writes -- on the CPU: the test-side
block writer and the oracle (oracle/linne_oracle.c) are held to the REAL reference decoder's recorded answers
(tests/golden/synth_records.json, from tests/golden/make_synth_records_golden.py: the reference under ASan + UBSan), and the
table's premises are checked: what each family claims to reach, it reaches.  No case is skipped anywhere."""
import importlib.util
import json
import os

import numpy as np
import pytest

import synth_records as sr
from refs import PRESET_LAYERS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_synth_records_golden", os.path.join(GOLDEN, "make_synth_records_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "synth_records.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def expected(oracle):
    """{shape: [pcm [C][n] per case]}: the oracle's synthesis of every record, computed once"""
    return {shape: [sr.expected_pcm(shape, c) for c in cases] for shape, cases in sr.table().items()}


def test_the_recording_covers_the_table_and_nothing_is_undefined(gold):
    import hashlib
    assert gold["seed"] == sr.SEED
    assert set(gold["shapes"]) == {s.name for s in sr.SHAPES}
    for shape, cases in sr.table().items():
        g = gold["shapes"][shape.name]
        assert list(g["cases"]) == [c.name for c in cases], f"{shape.name}: the recording is of another table"
        for rec in [g["stream"]] + list(g["cases"].values()):
            assert rec["defined"] is True and rec["ret"] == 0
        assert hashlib.sha256(sr.case_stream(shape, cases)).hexdigest() == g["stream"]["sha256"], f"{shape.name}: the writer's bytes changed"
        for c in cases:
            assert sr.defined(c.record, c.n, shape.preset), c.name


@pytest.mark.parametrize("shape", sr.SHAPES, ids=[s.name for s in sr.SHAPES])
def test_oracle_decodes_every_case_to_the_references_pcm(oracle, gold, expected, shape):
    """oracle.decode_whole of the writer's streams (CRC check on) -> OK and the recorded reference PCM, case by case and for the
    stream of all cases; oracle.decode_hotpath of the records themselves gives the same samples"""
    gen = _generator()
    cases = sr.table()[shape]
    g = gold["shapes"][shape.name]
    compared = 0
    for c, want in zip(cases, expected[shape]):
        stream = sr.case_stream(shape, [c])
        ret, pcm, _ = oracle.decode_whole(stream)
        assert ret == 0, f"{c.name}: oracle.decode_whole -> {ret}"
        assert pcm.shape == (shape.nch, c.n + sr.CLOSING_SAMPLES)
        assert gen.fnv_planes(pcm) == g["cases"][c.name]["fnv"], f"{c.name}: the oracle's PCM is not the reference's"
        assert np.array_equal(pcm[:, :c.n], want) and not pcm[:, c.n:].any(), f"{c.name}: decode_hotpath of the record differs from decode_whole of its block"
        compared += 1
    assert compared == len(cases) == len(g["cases"])
    ret, pcm, _ = oracle.decode_whole(sr.case_stream(shape, cases))
    assert ret == 0 and gen.fnv_planes(pcm) == g["stream"]["fnv"]
    assert np.array_equal(pcm[:, :-sr.CLOSING_SAMPLES], np.concatenate(expected[shape], axis=1))


def test_every_huffman_symbol_occurs():
    seen = set()
    for shape, cases in sr.table().items():
        seen |= sr.symbols(shape, cases)
    assert seen == set(range(256))


def test_the_units_family_reaches_what_it_claims():
    for shape, cases in sr.table().items():
        layers = PRESET_LAYERS[shape.preset]
        lens = set()
        for l, P in enumerate(layers):
            units = [(int(c.record[ch, sr.PRM_UNITS + l]), c.n) for c in cases if c.family == "units" for ch in range(shape.nch)]
            assert {u for u, _ in units} == {1 << k for k in range(8)}, f"{shape.name} layer {l}"
            assert any(u > P for u, _ in units) or P == 128, f"{shape.name} layer {l}: no unit count above the order"
            assert any(n % u for u, n in units) and any(n % u == 0 and u > 1 for u, n in units), f"{shape.name} layer {l}"
            assert any(n % u and (n // u) % 16 for u, n in units), f"{shape.name} layer {l}: no unit edge inside a 16-sample tile"
            lens |= {n for _, n in units}
        assert lens == set(sr.lengths(shape.block))
        tails = [c for c in cases if c.family == "units" and all(c.n % int(c.record[ch, sr.PRM_UNITS + l]) for ch in range(shape.nch) for l in range(len(layers)))]
        assert len(tails) >= 3, f"{shape.name}: no frame with a tail that no layer synthesises"


def test_the_shift_coefficient_and_preemphasis_families_reach_what_they_claim():
    for shape, cases in sr.table().items():
        if "shift" not in shape.families:
            continue
        layers = PRESET_LAYERS[shape.preset]
        total = sum(layers)
        for l in range(len(layers)):
            assert {int(c.record[0, sr.PRM_RSHIFT + l]) for c in cases if c.family == "shift"} == set(range(1, 16)), f"{shape.name} layer {l}"
        coefs = [c.record[:, sr.PRM_COEF:sr.PRM_COEF + total] for c in cases if c.family == "coef"]
        assert any((k == 127).all() for k in coefs) and any((k == -128).all() for k in coefs)
        assert any((k[:, 0::2] == 127).all() and (k[:, 1::2] == -128).all() for k in coefs)
        for stage in range(2):
            assert {int(c.record[ch, sr.PRM_PCOEF + stage]) for c in cases if c.family == "preem" for ch in range(shape.nch)} == set(range(16))
            prevs = {int(c.record[ch, sr.PRM_PREV + stage]) for c in cases if c.family == "preem" for ch in range(shape.nch)}
            assert prevs == {-(1 << shape.bits), (1 << shape.bits) - 1}, f"{shape.name}: the ends of the {shape.bits + 1}-bit zig-zag range"
    assert sum(1 for s in sr.SHAPES if s.nch == 8) == 1 and any(s.nch == 1 for s in sr.SHAPES) and any(s.nch == 3 and s.ms for s in sr.SHAPES)
    assert {s.preset for s in sr.SHAPES} == {0, 4, 7} and {s.bits for s in sr.SHAPES} == {16, 24} and {s.block for s in sr.SHAPES} == {1024, 1023}
    assert {(s.nch, s.ms) for s in sr.SHAPES} >= {(1, False), (2, True), (2, False), (3, True), (8, False)}


def test_the_growth_family_wraps_and_leaves_the_sample_formats(expected):
    """on the expected PCM and the cascade in unbounded integers (synth_plain, which must agree with the oracle): in every shape
    with the family some case holds samples beyond 2^24 that no wrap produced, some case wrapped, every case leaves the int16
    range, and no residual is larger than 2^20"""
    for shape, cases in sr.table().items():
        if "growth" not in shape.families:
            continue
        beyond24_unwrapped = wrapped_cases = 0
        for c, want in zip(cases, expected[shape]):
            assert np.abs(c.residual.astype(np.int64)).max() <= 1 << 20
            if c.family != "growth":
                continue
            pcm, peak, wrapped = sr.synth_plain(shape, c)
            assert np.array_equal(pcm, want), f"{c.name}: the cascade in plain integers differs from the oracle's"
            big = np.abs(want.astype(np.int64)).max()
            assert big > 32767, f"{c.name}: the decoded samples stay inside int16"
            assert big > 1 << 24, f"{c.name}: no sample beyond 2^24"
            beyond24_unwrapped += (not wrapped) and peak < 1 << 31
            wrapped_cases += bool(wrapped)
        assert beyond24_unwrapped >= 1, f"{shape.name}: every growth case wrapped"
        assert wrapped_cases >= 2, f"{shape.name}: too few growth cases wrap"


def test_the_plain_integer_cascade_agrees_on_the_tail_cases(expected):
    """the frames whose tail no layer synthesises, in plain integers straight from linne_lpc_synthesize.c:14-15 and :27"""
    checked = 0
    for shape, cases in sr.table().items():
        for c, want in zip(cases, expected[shape]):
            if c.family == "units" and "/all" in c.name and shape.nch <= 3:
                pcm, _, _ = sr.synth_plain(shape, c)
                assert np.array_equal(pcm, want), c.name
                checked += 1
    assert checked >= 15
