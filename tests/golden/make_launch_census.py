"""Records which kernels an encode and a decode call launch, case by case, as tests/golden/launch_census.json.

    python tests/golden/make_launch_census.py            (on the GPU box, at the commit whose launches are the reference)

Each case is one encode_frames and one decode_frames call on a fresh context: stereo, 2048-sample blocks, noise.  What is kept per
case: the launch count of every timing kind (include/linne_amd.h, 1 ... 55) after each of the two calls, the form of the call's last
k_search_long launch and the count of exact fallbacks.  tests/test_gpu_launch_census.py runs the same cases (CASES, run_case) and
requires the same counts: a change of the host's launch code that is meant to leave the launches alone is held to that here.
Output values are not recorded: the parity tests compare those.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "launch_census.json")
KINDS = range(1, 56)
NCH, BITS, BLOCK = 2, 16, 2048


def _case(name, preset, lengths, env=None, af=0, learn=False, scratch_frames=0):
    return {"name": name, "preset": preset, "lengths": list(lengths), "env": dict(env or {}), "af": af, "learn": learn,
            "scratch_frames": scratch_frames}


def _tail(F, tail):
    return [BLOCK] * (F - 1) + [tail]


_HIST_FWD = {"LINNE_AMD_HIST": "1", "LINNE_AMD_FWD_LOSS": "1"}
CASES = []
for _m in (0, 2, 7):
    CASES += [_case(f"m{_m}_f1", _m, [BLOCK]), _case(f"m{_m}_f5_tail1001", _m, _tail(5, 1001)), _case(f"m{_m}_f40_tail777", _m, _tail(40, 777))]
CASES += [
    _case("m7_f40_hist_fwdloss", 7, _tail(40, 777), _HIST_FWD),
    _case("m7_f40_hist_fwdloss_lastlayer2", 7, _tail(40, 777), {**_HIST_FWD, "LINNE_AMD_LAST_LAYER": "2"}),
    _case("m7_f40_search_job0", 7, _tail(40, 777), {"LINNE_AMD_SEARCH_JOB": "0"}),
    _case("m7_f40_search_two0", 7, _tail(40, 777), {"LINNE_AMD_SEARCH_TWO": "0"}),
    _case("m7_f40_speculate0", 7, _tail(40, 777), {"LINNE_AMD_SPECULATE": "0"}),
    _case("m7_f40_fir_small0", 7, _tail(40, 777), {"LINNE_AMD_FIR_SMALL": "0"}),
    _case("m7_f1_lev_wave0", 7, [BLOCK], {"LINNE_AMD_LEV_WAVE": "0"}),
    _case("m7_f18_sort0_mixed_runs", 7, [BLOCK, 777] * 9, {"LINNE_AMD_SORT": "0"}),
    _case("m7_f40_exact", 7, _tail(40, 777), {"LINNE_AMD_EXACT": "1"}),
    _case("m7_f8_af1", 7, _tail(8, 777), af=1),
    _case("m7_f8_learning", 7, _tail(8, 777), learn=True),
    _case("m2_f40_arena_of_five_frames", 2, _tail(40, 777), scratch_frames=5),
    _case("m0_f1100_streams2", 0, _tail(1100, 777), {"LINNE_AMD_STREAMS": "2"}),
    _case("decode_wave", 7, _tail(40, 777), {"LINNE_AMD_DECODE_KERNEL": "wave"}),
    _case("decode_lanes", 7, _tail(40, 777), {"LINNE_AMD_DECODE_KERNEL": "lanes"}),
    _case("decode_pipe", 7, _tail(40, 777), {"LINNE_AMD_DECODE_KERNEL": "pipe"}),
    _case("decode_rows", 7, _tail(40, 777), {"LINNE_AMD_DECODE_KERNEL": "rows"}),
    _case("decode_fused0", 7, _tail(40, 777), {"LINNE_AMD_DECODE_FUSED": "0"}),
    _case("decode_rows8", 7, _tail(40, 777), {"LINNE_AMD_DECODE_ROWS8": "1"}),
    # (80 channel-frames take the pipe form by themselves; with the rows form asked for, the two knobs have something to select)
    _case("decode_rows_fused0", 7, _tail(40, 777), {"LINNE_AMD_DECODE_KERNEL": "rows", "LINNE_AMD_DECODE_FUSED": "0"}),
    _case("decode_rows_rows8", 7, _tail(40, 777), {"LINNE_AMD_DECODE_KERNEL": "rows", "LINNE_AMD_DECODE_ROWS8": "1"}),
]
CASE_NAMES = [c["name"] for c in CASES]

_noise = {}


def noise_frames(F):
    """[F][C][BLOCK] of Gaussian noise (tests/signals.py); the first frames of one long draw, so every case shares it"""
    from signals import waveform
    if "x" not in _noise:
        _noise["x"] = waveform("gauss_noise", NCH, 1100 * BLOCK, BITS, seed=5).reshape(NCH, 1100, BLOCK).transpose(1, 0, 2)
    return np.ascontiguousarray(_noise["x"][:F])


def run_case(case, setenv):
    """the census of one case; setenv(name, value) sets the case's knobs BEFORE the context is created (the caller restores them)"""
    import torch
    import linne_amd
    for k, v in case["env"].items():
        setenv(k, v)
    lengths = np.array(case["lengths"], dtype=np.uint32)
    F = len(lengths)
    frames = noise_frames(F).copy()
    for f in range(F):
        frames[f, :, int(lengths[f]):] = 0
    scratch = 0
    shape = linne_amd.Shape(NCH, BITS, BLOCK, case["preset"], 1)
    if case["scratch_frames"]:
        per = int(linne_amd.lib.LINNEAmd_ScratchBytesPerFrame(ctypes.byref(shape)))
        scratch = case["scratch_frames"] * per + 65536 + 256
    c = linne_amd.Context(0, scratch_bytes=scratch, use_torch_stream=False)
    try:
        c.enable_timing(True)
        if case["af"]:
            c.set_af_iterations(case["af"])
        if case["learn"]:
            c.set_learning(True)
        pcm = torch.from_numpy(frames).to("cuda:0")
        res, prm, _ = c.encode_frames(shape, pcm, lengths)
        c.synchronize()
        enc = {str(k): c.last_launches(k) for k in KINDS if c.last_launches(k)}
        form = int(linne_amd.lib.LINNEAmd_GetLastSearchLongForm(ctypes.c_void_p(c.h)))
        fallback = c.last_fallback_count()
        c.decode_frames(shape, res, prm, lengths)
        c.synchronize()
        dec = {str(k): c.last_launches(k) for k in KINDS if c.last_launches(k)}
    finally:
        c.close()
    return {"encode": enc, "search_long_form": form, "fallbacks": fallback, "decode": dec}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, os.path.dirname(HERE))
    out = {}
    for case in CASES:
        saved = {k: os.environ.get(k) for k in case["env"]}
        try:
            out[case["name"]] = run_case(case, os.environ.__setitem__)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        print(case["name"], json.dumps(out[case["name"]]), flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
