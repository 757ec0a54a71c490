"""Records the real reference's answers for tests/test_repair_cpu.py into tests/golden/repair_answers.json (as make_splice_golden.py
does for its own file): for every case of tests/repair_cases.py, built from the reference's own streams, length + sha256 of the
damaged stream, of the stream the numpy restatement of the repair contract makes of it, the return code of the reference's DecodeWhole
(CRC check on) on that and length + sha256 of the samples it returns.  Digests only.
Needs oracle/_ref (built by oracle/Makefile where the reference's sources are); no GPU.
Run from the repository root after build():  python tests/golden/make_repair_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import numpy as np  # noqa: E402

import repair_cases as rc  # noqa: E402
from refs import REF_SO, Reference, digest, reference_available  # noqa: E402

ANSWERS = os.path.join(HERE, "repair_answers.json")


def main():
    if not reference_available():
        sys.exit(f"{REF_SO} not built: run build() where the reference's sources are")
    ref = Reference()
    answers = {}
    for name, (data, _) in rc.build_cases(ref).items():
        got = rc.repair(data)
        if got is None:
            answers[name] = {"stream": digest(data), "repaired": None}
            continue
        out, report = got
        ret, pcm = ref.decode_whole(out)
        answers[name] = {"stream": digest(data), "repaired": digest(out), "ret": int(ret), "pcm": digest(np.stack(pcm)),
                         "gaps": [[g["first_sample"], g["num_samples"]] for g in report["gaps"]], "exact": report["exact"]}
    with open(ANSWERS, "w") as f:
        json.dump(dict(sorted(answers.items())), f, indent=0)
        f.write("\n")
    print(f"{len(answers)} answers -> {os.path.relpath(ANSWERS, ROOT)}")


if __name__ == "__main__":
    main()
