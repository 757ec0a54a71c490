"""-a N and -l against the oracle, frame by frame, in batches past the 64- and 256-job launch rules (-m gpu).

The cases are those of tests/option_batches.py (its docstring has the table and why there is no two-stream case);
tests/test_option_batches_cpu.py proves their premises without a GPU.  Each case runs on a fresh context with the option set through
set_af_iterations / set_learning, nothing forced by the environment, and is checked values first, forms last:

1. the product's residual, oracle-defined parameter words, r0, best regulariser, loss and Q2 tail of EVERY frame equal the oracle's
   with the same -a N / -l (test_gpu_batch_forms.check_encode: bit for bit, no tolerance), and the residual behind a ragged frame's
   end is zero;
2. the product's output, with sentinels behind ragged ends, decodes to the input;
3. with the option switched off again on the same context the same batch gives the plain oracle's answer: the refinement buffers,
   job_reg and af_best leave nothing behind;
4. kind 26 (the real final pass of -a N) and kind 27 (the trainer) have one span per chunk where the option is on and none where it
   is off; kind 1 (k_prep) counts the chunks;
5. the final pass of -a N ran the forms the case is for: lnn_forms_query with the case's options says, for the case's channel-frame
   count, lev_wave = 0 (k_levinson_lds with its riders), sel_wave as the case states it, no k_autocorr_wide for the long layer.  A
   moved threshold fails here instead of letting the case test something else.

Cases 6 and 7 run case 1's and case 3's batch in an arena for ceil(F / 3) + 1 frames, sized with the scratch bytes per frame of the
call WITH its option (option_batches.arena_for): three chunks, and every frame must also equal the one-chunk result.
"""
import os
import time

import numpy as np
import pytest

import linne_amd
import option_batches as ob
from test_gpu_batch_forms import check_decode, check_encode, check_variety, marked

pytestmark = pytest.mark.gpu

ALL = sorted(ob.CASES)
KINDS = (1, 26, 27)
_ONE_CHUNK = {}         # the product's output of a case that ran in one chunk, for the chunked case of the same batch


def encode_with_options(ctx_env, n):
    """case n on a fresh context: (output with the option, launches, decode of that output, output with the option off again, launches, seconds)"""
    c, b = ob.CASES[n], ob.batch_of(n)
    frames, ns = b["frames"], b["ns"]
    with ctx_env({}, scratch_bytes=ob.arena_for(n)) as ctx:
        shape = ctx.shape(c["nch"], c["bits"], c["block"], c["preset"], c["ms"])
        ctx.enable_timing(True)
        ctx.set_af_iterations(c["af"])
        ctx.set_learning(bool(c["learn"]))
        t0 = time.perf_counter()
        out = ctx.encode_frames_host(shape, frames, ns)
        seconds = time.perf_counter() - t0
        launches = {k: ctx.last_launches(k) for k in KINDS}
        dec = ctx.decode_frames_host(shape, marked(out[0], ns, c["block"]), out[1], ns)
        ctx.set_af_iterations(0)
        ctx.set_learning(False)
        plain = ctx.encode_frames_host(shape, frames, ns)
        launches_plain = {k: ctx.last_launches(k) for k in KINDS}
    return out, launches, dec, plain, launches_plain, seconds


def one_chunk_result(ctx_env, n):
    """what the one-chunk case of n's batch gave (case 1 for 6, case 3 for 7); computed here when that case has not run in this session"""
    base = {6: 1, 7: 3}[n]
    if base not in _ONE_CHUNK:
        _ONE_CHUNK[base] = encode_with_options(ctx_env, base)[0]
    return _ONE_CHUNK[base]


@pytest.mark.parametrize("n", ALL, ids=[ob.NAMES[n] for n in ALL])
def test_option_batch_against_the_oracle(ctx_env, oracle, n):
    for v in os.environ:
        assert not v.startswith("LINNE_AMD_") or v == "LINNE_AMD_LIB", f"{v} is set: these cases run the rules as they stand"
    c, b = ob.CASES[n], ob.batch_of(n)
    ns, block = b["ns"], c["block"]
    on, off = ob.answers(oracle, n, True), ob.answers(oracle, n, False)
    out, launches, dec, plain, launches_plain, seconds = encode_with_options(ctx_env, n)
    print(f"case {n} ({ob.NAMES[n]}): encode with the option {seconds:.2f} s; launches {launches}, option off {launches_plain}")
    if not c["thirds"]:
        _ONE_CHUNK[n] = out
    # 1. the oracle with the same option
    check_encode(on, b, *out, f"case {n}, -a {c['af']}{' -l' if c['learn'] else ''}")
    check_variety(b, out[1], out[2], linne_amd.PRESET_NUM_REGULARS[c["preset"]])
    if c["thirds"]:
        one = one_chunk_result(ctx_env, n)
        for name, x, y in zip(("residual", "parameters", "statistics"), out, one):
            eq = (x == y) | (np.isnan(x) & np.isnan(y)) if x.dtype.kind == "f" else (x == y)
            differ = np.flatnonzero(~eq.all(axis=(1, 2)))
            assert len(differ) == 0, f"case {n}: the {name} of frames {differ[:8].tolist()} differ between three chunks and one"
    # 2. decode
    check_decode(dec, marked(b["frames"], ns, block), ns, block, f"case {n}: decode of the product's own encode output")
    # 3. the option off again on the same context
    check_encode(off, b, *plain, f"case {n}, the option switched off again on the same context")
    # 4. launch counts
    call = ob.forms(n, arena=ob.arena_for(n))
    nchunks = 3 if c["thirds"] else 1
    assert call["nchunks"] == nchunks
    assert launches == {1: nchunks, 26: nchunks if c["af"] else 0, 27: nchunks if c["learn"] else 0}, launches
    assert launches_plain == {1: ob.forms(n, on=False, arena=ob.arena_for(n))["nchunks"], 26: 0, 27: 0}, launches_plain
    # 5. the forms of the final pass
    ll = ob.long_layer(c["preset"])
    assert not (call["prod_ok"] >> ll) & 1, "k_autocorr_wide would serve the long layer"
    for k in call["chunks"]:
        assert ("final_pass" in k) == bool(c["af"])
        if c["af"]:
            fin = k["final_pass"]
            assert fin["J"] == k["Fc"] * c["nch"]
            lev, sel = ob.final_forms_expected(fin["J"])
            assert [l["lev_wave"] for l in fin["layers"]] == [lev] * call["L"] and lev == 0, "the final pass is for k_levinson_lds"
            assert [l["sel_wave"] for l in fin["layers"]] == [sel] * call["L"]
            assert c["thirds"] or sel == c["sel_wave"], "the final pass on the other side of 256 jobs"
