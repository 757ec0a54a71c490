"""Records the real reference's answers for the inputs of the tests that compare with it (the `reference` fixture,
tests/refs.py RecordedReference) into tests/golden/reference_answers.json: length + sha256 of every stream the reference
library (oracle/_ref/liblinne_ref.so) and its command line tool (oracle/_ref/linne_ref) write, and of the samples its
decoder returns.  Needs oracle/_ref (built by oracle/Makefile where the reference's sources are); no GPU.
Run from the repository root after build():  python tests/golden/make_reference_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import call_history as ch  # noqa: E402
import test_gpu_parity as gp  # noqa: E402
import test_oracle_cpu as oc  # noqa: E402
from refs import ANSWERS, REF_SO, Reference, blocks_key, cli_key, decode_key, digest, encode_key, reference_available  # noqa: E402
from signals import LONG_STREAMS, WAVEFORMS, long_stream_args, music, waveform  # noqa: E402

REF_CLI = os.path.join(ROOT, "oracle", "_ref", "linne_ref")


def params(fn):
    """the argument values of a test's @pytest.mark.parametrize"""
    for m in fn.pytestmark:
        if m.name == "parametrize":
            return list(m.args[1])
    raise LookupError(fn.__name__)


def main():
    if not (reference_available() and os.path.exists(REF_CLI)):
        sys.exit(f"{REF_SO} / {REF_CLI} not built: run build() where the reference's sources are")
    ref = Reference()
    answers = {}

    def encode(x, bits, rate, block, preset, ms, af_iters=0, learning=0):
        stream = ref.encode_whole(x, bits, rate, block, preset, ms, af_iters=af_iters, learning=learning)
        answers[encode_key(x, bits, rate, block, preset, ms, af_iters, learning)] = digest(stream)
        return stream

    def decode(stream):
        ret, pcm = ref.decode_whole(stream)
        answers[decode_key(stream)] = {"ret": int(ret), "pcm": digest(pcm)}

    # test_oracle_cpu.py
    for kind in WAVEFORMS:
        for nch, bits, preset in oc.REFERENCE_LIBRARY_CONFIGS:
            encode(waveform(kind, nch, 4096, bits, seed=nch + bits), bits, 8000, 1024, preset, nch >= 2)
    for _, x in oc.block_type_sequences():
        encode(x, 16, 44100, 1024, 7, True)

    # test_gpu_parity.py
    x = music(2, 3 * 10240 + 2000, 16, seed=11)                                       # test_lnn_bytes_music_with_tail
    decode(encode(x, 16, 44100, 10240, 7, True))
    x, lens = gp.many_block_lengths()                                                   # test_decode_whole_of_a_stream_with_many_...
    stream = gp.stream_of_blocks(ref, x, 16, 44100, 4096, 7, True, lens)
    answers[blocks_key(x, 16, 44100, 4096, 7, True, lens)] = digest(stream)
    decode(stream)
    encode(gp.emission_input(4096), 16, 44100, 4096, 7, True)                           # test_whole_stream_with_and_without_device_emission
    for nch, bits, block, preset, total in params(gp.test_odd_block_sizes):
        encode(music(nch, total, bits, seed=block), bits, 44100, block, preset, nch >= 2)
    for nch, bits, block, preset, total, af in params(gp.test_auxiliary_function_iterations):
        encode(music(nch, total, bits, seed=block + af), bits, 44100, block, preset, nch >= 2, af_iters=af)
    for kind in params(gp.test_auxiliary_function_on_degenerate_signals):
        encode(waveform(kind, 2, 4096, 16, seed=1), 16, 44100, 1024, 7, True, af_iters=2)
    for nch, bits, block, preset, total, af in params(gp.test_network_trainer):
        encode(music(nch, total, bits, seed=block + af), bits, 44100, block, preset, nch >= 2, af_iters=af, learning=1)
    for kind in params(gp.test_network_trainer_on_degenerate_signals):
        encode(waveform(kind, 1, 1024, 16, seed=1), 16, 44100, 512, 4, False, learning=1)

    # test_gpu_rice_oracle.py test_long_block_streams, test_oracle_cpu.py test_oracle_equals_reference_at_long_blocks
    for cfg in LONG_STREAMS:
        decode(encode(*long_stream_args(*cfg)))

    # test_gpu_call_history.py test_one_handle_many_streams: the four streams ONE encoder handle of the reference writes in turn
    # (call_history.handle_sequence), and its own decoder handle's round trip of them
    xs, streams = ch.handle_inputs(), ch.handle_sequence(ref)
    for i, (x, stream) in enumerate(zip(xs, streams)):
        answers[ch.handle_key(i, x)] = dict(digest(stream), block_types=ch.block_types(stream))
    for i, (ret, pcm) in zip(ch.DECODE_ORDER9, ch.decode_through_one_handle(ref, streams)):
        assert ret == 0 and (pcm == xs[i]).all(), f"the reference's own round trip of stream {i}"

    # test_own_cli_matches_the_reference_cli: the reference CLI's .lnn of each WAV, and its WAV of each such .lnn
    with tempfile.TemporaryDirectory() as tmp:
        for wav, mode in (("ref_16bit_2ch.wav", "7"), ("ref_16bit_2ch.wav", "5"), ("ref_a.wav", "5")):
            src, lnn, back = os.path.join(HERE, wav), os.path.join(tmp, "o.lnn"), os.path.join(tmp, "o.wav")
            subprocess.run([REF_CLI, "-e", "-m", mode, src, lnn], check=True, stdout=subprocess.DEVNULL)
            subprocess.run([REF_CLI, "-d", lnn, back], check=True, stdout=subprocess.DEVNULL)
            data, enc, dec = (open(p, "rb").read() for p in (src, lnn, back))
            answers[cli_key(["-e", "-m", mode], data)] = digest(enc)
            answers[cli_key(["-d"], enc)] = digest(dec)

    with open(ANSWERS, "w") as f:
        json.dump(dict(sorted(answers.items())), f, indent=0)
        f.write("\n")
    print(f"{len(answers)} answers -> {os.path.relpath(ANSWERS, ROOT)}")


if __name__ == "__main__":
    main()
