"""Records the real reference's answers for tests/test_splice_cpu.py into tests/golden/splice_answers.json (as
make_reference_golden.py does for its own file):
  premise/<case>      a spliced stream assembled in numpy (tests/splice_cases.py) from the reference's own streams and its own fragment
                      encodings: length + sha256 of the stream, the return code of the reference's DecodeWhole (CRC check on) and
                      length + sha256 of the samples it returns;
  fragment/m<p>/n<n>  whether the reference's EncodeWhole of a fragment of n samples round-trips through its DecodeWhole, and the
                      length + sha256 of the block it writes.  Every fragment runs in a process of its own: the reference is free to
                      crash on lengths outside its contract, which is recorded as such.
Needs oracle/_ref (built by oracle/Makefile where the reference's sources are); no GPU.
Run from the repository root after build():  python tests/golden/make_splice_golden.py"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import numpy as np  # noqa: E402

import splice_cases as sc  # noqa: E402
from refs import REF_SO, Reference, digest, reference_available  # noqa: E402

ANSWERS = os.path.join(HERE, "splice_answers.json")


def fragment(n, preset):
    """runs in a child: prints the fragment's record as JSON"""
    ref = Reference()
    x = sc.fragment_pcm(n, preset)
    stream = ref.encode_whole(x, 16, 44100, sc.PREMISE_BLOCK, preset, True)
    ret, pcm = ref.decode_whole(stream)
    good = ret == 0 and np.array_equal(np.stack(pcm), x)
    print(json.dumps({"good": bool(good), "how": "round trip" if good else f"DecodeWhole -> {ret} or other samples", "block": digest(stream[sc.HEADER:])}))


def main():
    if not reference_available():
        sys.exit(f"{REF_SO} not built: run build() where the reference's sources are")
    ref = Reference()
    answers = {}
    for preset in sc.PREMISE_PRESETS:
        for name, cuts in sc.premise_cases(preset).items():
            data, _ = sc.splice_with(ref, cuts, preset)
            ret, pcm = ref.decode_whole(data)
            answers[f"premise/{name}"] = {"stream": digest(data), "ret": int(ret), "pcm": digest(np.stack(pcm))}
        for n in sc.FRAGMENT_LENGTHS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fragment", str(n), str(preset)], stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL, text=True)
            if r.returncode == 0:
                rec = json.loads(r.stdout.strip().splitlines()[-1])
            else:
                rec = {"good": False, "how": f"EncodeWhole ended the process with status {r.returncode}", "block": None}
            answers[f"fragment/m{preset}/n{n}"] = rec
    with open(ANSWERS, "w") as f:
        json.dump(dict(sorted(answers.items())), f, indent=0)
        f.write("\n")
    print(f"{len(answers)} answers -> {os.path.relpath(ANSWERS, ROOT)}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--fragment":
        fragment(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
