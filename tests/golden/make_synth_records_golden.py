#!/usr/bin/env python3
"""Generates tests/golden/synth_records.json: what the REAL reference decoder makes of the case table of tests/synth_records.py --
COMPRESS blocks with parameter records no encoder writes.  Every case's one-block stream, and every shape's stream of all its
cases, is decoded by oracle/_ref/ref_decode_san in a child process: the reference decoder built with AddressSanitizer + UBSan
(oracle/Makefile; CPU only).  Recorded per stream: the result code, an FNV-1a-64 of the decoded planes, `defined` (no sanitizer
report), and the sha256 of the stream's bytes, which ties the answer to the table that was decoded.

The table is meant to lie wholly inside what the reference decodes with defined behaviour (synth_records.defined).  A case that
comes back undefined or not OK makes this script FAIL: tighten the rule or the table, the tests skip nothing.

    python tests/golden/make_synth_records_golden.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def fnv_planes(pcm):
    """FNV-1a-64 over the int32 planes, little-endian bytes, channel after channel (what oracle/ref_decode_san.c prints)"""
    import numpy as np
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(pcm, dtype="<i4").tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def reference_answer(san, stream, tmp):
    with open(tmp, "wb") as f:
        f.write(stream)
    r = subprocess.run([san, tmp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    rec = {"sha256": hashlib.sha256(stream).hexdigest()}
    if r.returncode != 0 or not r.stdout.startswith("ret "):
        why = ([l for l in r.stderr.strip().splitlines() if "ERROR" in l or "runtime error" in l] or ["crash"])[0][:200]
        return dict(rec, defined=False, why=why)
    parts = r.stdout.split()
    return dict(rec, defined=True, ret=int(parts[1]), fnv=parts[3])


def main():
    import synth_records as sr
    san = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "ref_decode_san")
    assert os.path.exists(san), "build oracle/_ref first (make -C oracle ref)"
    out = {"seed": sr.SEED, "shapes": {}}
    bad = []
    fd, tmp = tempfile.mkstemp(suffix=".lnn")
    os.close(fd)
    try:
        for shape, cases in sr.table().items():
            entry = {"stream": reference_answer(san, sr.case_stream(shape, cases), tmp), "cases": {}}
            for c in cases:
                entry["cases"][c.name] = reference_answer(san, sr.case_stream(shape, [c]), tmp)
            out["shapes"][shape.name] = entry
            for name, rec in [(shape.name, entry["stream"])] + list(entry["cases"].items()):
                if not rec["defined"] or rec["ret"] != 0:
                    bad.append((name, rec))
    finally:
        os.remove(tmp)
    for name, rec in bad:
        print(f"NOT DEFINED AND OK: {name}: {rec}", file=sys.stderr)
    if bad:
        sys.exit(f"{len(bad)} streams of the table are undefined or refused by the reference: nothing written")
    path = os.path.join(HERE, "synth_records.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    ncases = sum(len(e["cases"]) for e in out["shapes"].values())
    size = os.path.getsize(path)
    assert size < 1 << 20, f"{path}: {size} bytes, above the limit for a committed file"
    print(f"{ncases} cases in {len(out['shapes'])} shapes, all decoded OK with defined behaviour; {size} bytes")


if __name__ == "__main__":
    main()
