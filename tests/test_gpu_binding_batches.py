"""GPU tests of what the Python forms of the batch calls that write new resident streams add to the C entry points
(Context.encode_streams, splice_streams, repair_streams): every output at its default room in one allocation, the items whose result
is INSUFFICIENT_BUFFER once more, together, at their exact sizes in another allocation, and then one result, one text and one list of
codes for both calls.  The C calls themselves are held to their contracts in tests/test_gpu_stream_batch_encode.py,
tests/test_gpu_splice.py and tests/test_gpu_repair.py; here every item is held to the same Python form on that item alone.

Inputs that need the second call by themselves: a stream of a non-empty track is at least 30 header bytes and 11 block-head bytes, and
the default room is 2 * C * N * ceil(bits / 8) + 30, so a track with C * N * ceil(bits / 8) <= 5 never fits (the oracle's streams of
the three below take 71 to 74 bytes)."""
import numpy as np
import pytest

import linne_amd
from signals import music
from stream_refs import blocks

pytestmark = pytest.mark.gpu

OK, INSUFFICIENT_BUFFER = 0, 3
RATE, BLOCK, PRESET = 44100, 1024, 0
REFUSED = 2                                  # the place of the track whose header is refused
TINY, ORDINARY = (0, 3, 5), (1, 4)


def as_bytes(t):
    return bytes(t.cpu().numpy())


def room(pcm, bits):
    return 2 * pcm.shape[0] * pcm.shape[1] * ((bits + 7) // 8) + 30


@pytest.fixture(scope="module")
def batch(ctx):
    """(tracks, the states given, encode_stream's (bytes, new state) per track -- the LinneAmdError of the refused one)"""
    import torch
    rng = np.random.default_rng(3)
    noise = torch.from_numpy(rng.integers(-32768, 32768, size=(2, 3000)).astype(np.int16)).cuda()
    mono = torch.from_numpy(music(1, 1500, 16, seed=5).astype(np.int16)).cuda()
    tiny = [rng.integers(-100, 100, size=(1, n)).astype(np.int32) for n in (1, 3)] + [rng.integers(-9000, 9000, size=(1, 2)).astype(np.int32)]
    tracks = [(tiny[0], 8, RATE, BLOCK, PRESET, False), (noise, 16, RATE, BLOCK, PRESET, False), (music(2, 500, 16, seed=6), 16, RATE, 32, PRESET, False),
              (tiny[1], 8, RATE, BLOCK, PRESET, False), (mono, 16, RATE, BLOCK, PRESET, False), (tiny[2], 16, RATE, BLOCK, PRESET, False)]
    states = [0.0, 0.25, 0.5, -0.25, 0.125, 0.0]
    single = []
    for i, (t, st) in enumerate(zip(tracks, states)):
        if i == REFUSED:
            with pytest.raises(linne_amd.LinneAmdError) as e:
                ctx.encode_stream(*t, parcor_state=st)
            single.append(e.value)
        else:
            s, new = ctx.encode_stream(*t, parcor_state=st)
            single.append((as_bytes(s), new))
    for i in TINY:
        assert len(single[i][0]) > room(tracks[i][0], tracks[i][1]) and len(single[i][0]) >= 41, i      # never fits its default room
    for i in ORDINARY:
        assert len(single[i][0]) <= room(tracks[i][0], tracks[i][1]), i
    assert single[REFUSED].code not in (OK, INSUFFICIENT_BUFFER)
    return tracks, states, single


def test_encode_streams_encodes_again_at_the_exact_size(ctx, batch):
    tracks, states, single = batch
    refused = single[REFUSED].code
    streams, new, codes = ctx.encode_streams(tracks, group_frames=0, parcor_states=states, return_codes=True)
    # the second call held the three tiny tracks: mono 8-bit twice and mono 16-bit, two shapes of the first call's three
    assert ctx.last_stream_batch_count(0) == 2
    assert codes == [refused if i == REFUSED else OK for i in range(6)]
    for i in range(6):
        if i == REFUSED:
            assert streams[i] is None and new[i] == states[i]          # (a failing track's state is left alone)
        else:
            assert (as_bytes(streams[i]), new[i]) == single[i], f"track {i}"
            assert streams[i].data_ptr() % 4 == 0
    # the first call's streams lie in another allocation than the second call's, which has not touched them
    first, second = ({streams[i].untyped_storage().data_ptr() for i in which} for which in (ORDINARY, TINY))
    assert len(first) == 1 and len(second) == 1 and first != second
    # without return_codes: the first failing track's code, every track's code
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.encode_streams(tracks, group_frames=0, parcor_states=states)
    assert e.value.code == refused and e.value.codes == codes and len(e.value.codes) == 6
    assert f"track {REFUSED} failed" in str(e.value)
    # without states, and verified
    assert [None if s is None else as_bytes(s) for s in ctx.encode_streams(tracks, return_codes=True)[0]] == \
        [None if s is None else as_bytes(s) for s in ctx.encode_streams(tracks, parcor_states=[0.0] * 6, return_codes=True)[0]]
    ctx.set_verify(True)
    try:
        vstreams, vnew, vcodes = ctx.encode_streams(tracks, group_frames=0, parcor_states=states, return_codes=True)
    finally:
        ctx.set_verify(False)
    assert vcodes == codes and vnew == new
    assert [None if s is None else as_bytes(s) for s in vstreams] == [None if s is None else as_bytes(s) for s in streams]


def test_encode_streams_all_fit_and_none(ctx, batch):
    tracks, states, single = batch
    streams, new = ctx.encode_streams([tracks[i] for i in ORDINARY], parcor_states=[states[i] for i in ORDINARY])
    assert [(as_bytes(s), st) for s, st in zip(streams, new)] == [single[i] for i in ORDINARY]
    streams, new = ctx.encode_streams([tracks[i] for i in TINY], parcor_states=[states[i] for i in TINY])      # every track once more
    assert [(as_bytes(s), st) for s, st in zip(streams, new)] == [single[i] for i in TINY]
    assert ctx.encode_streams([], parcor_states=[], return_codes=True) == ([], [], [])


@pytest.fixture(scope="module")
def sources(ctx):
    """two streams of five blocks and a tail on the device, with their indexes"""
    out = []
    for nch, seed in ((2, 21), (1, 22)):
        x = music(nch, 5 * BLOCK + 300, 16, seed=seed)
        t = ctx.encode_stream(x, 16, RATE, BLOCK, 4, nch == 2).clone()
        out.append((t, ctx.index_stream(t), x.shape[1]))
    yield out
    for _, index, _ in out:
        index.close()


def test_splice_streams_failing_output_among_good_ones(ctx, sources):
    """Two good outputs and one whose cut reaches past its stream's end, each held to the call on that output alone.  The second call
    cannot be reached with natural inputs: an output's default room is a bound on its size.  That pass is the one
    test_encode_streams_encodes_again_at_the_exact_size proves."""
    (a, ia, na), (b, ib, nb) = sources
    splices = [[(a, ia, 100, 3 * BLOCK), (a, ia, 4 * BLOCK, None)], [(b, ib, 100, nb)], [(b, ib, BLOCK, 2 * BLOCK), (b, ib, 37, 0), (b, ib, 0, None)]]
    single = []
    for cuts in splices:
        s, c = ctx.splice_streams([cuts], return_codes=True)
        single.append((None if s[0] is None else as_bytes(s[0]), c[0], ctx.last_splice_blocks[0]))
    assert [c for _, c, _ in single] == [OK, single[1][1], OK] and single[1][1] not in (OK, INSUFFICIENT_BUFFER) and single[1][0] is None
    for gf in (0, 3):
        streams, codes = ctx.splice_streams(splices, group_frames=gf, return_codes=True)
        assert [(None if s is None else as_bytes(s), c, n) for s, c, n in zip(streams, codes, ctx.last_splice_blocks)] == single, gf
        assert len({s.untyped_storage().data_ptr() for s in streams if s is not None}) == 1 and all(s.data_ptr() % 4 == 0 for s in streams if s is not None)
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.splice_streams(splices)
    assert e.value.code == single[1][1] and e.value.codes == codes and "splice 1: " in str(e.value)
    assert ctx.last_splice_blocks == [n for _, _, n in single]          # set for a call that raises, too
    assert ctx.splice_streams([]) == [] and ctx.splice_streams([], return_codes=True) == ([], [])


def test_repair_streams_failing_stream_among_good_ones(ctx, sources):
    """Two streams that repair -- one with a block lost, one sound -- and one shorter than a header, each held to the call on that
    stream alone.  The second call cannot be reached with natural inputs: a stream's default room is a bound on its repaired size.
    That pass is the one test_encode_streams_encodes_again_at_the_exact_size proves."""
    (a, _, _), (b, _, _) = sources
    broken = bytearray(as_bytes(a))
    off, size = blocks(bytes(broken))[2][:2]
    broken[off + size - 2] ^= 0x10                                      # block 2 fails its CRC
    streams = [bytes(broken), as_bytes(b)[:17], b]
    single = []
    for s in streams:
        got, c = ctx.repair_streams([s], return_codes=True)
        single.append((None if got[0][0] is None else as_bytes(got[0][0]), got[0][1], c[0]))
    assert [c for _, _, c in single] == [OK, single[1][2], OK] and single[1][2] not in (OK, INSUFFICIENT_BUFFER) and single[1][0] is None
    assert single[0][1]["num_gaps"] == 1 == len(single[0][1]["gaps"]) and single[2][1]["num_gaps"] == 0 and single[2][0] == as_bytes(b)
    got, codes = ctx.repair_streams(streams, return_codes=True)
    assert [(None if s is None else as_bytes(s), report, c) for (s, report), c in zip(got, codes)] == single
    assert len({s.untyped_storage().data_ptr() for s, _ in got if s is not None}) == 1
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.repair_streams(streams)
    assert e.value.code == single[1][2] and e.value.codes == codes and "repair 1: " in str(e.value)
    assert ctx.repair_streams([]) == [] and ctx.repair_streams([], return_codes=True) == ([], [])
