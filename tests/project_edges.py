"""The windows of the plane-count tests (tests/test_gpu_stream_project.py test 7, tests/test_stream_project_cpu.py): streams whose decode
is chosen -- values at the edges of the rule by which lnn_k_project.h cuts a tile's samples into 2, 3 or 4 planes --, the windows that
put such a value where a scan of the tile's values could miss it, and, from the decoded samples alone, the plane count every tile of
every window must choose.  Nothing here touches a GPU or the library under test.

Every thread of the kernel ORs v ^ (v >> 31) over the values it reads of the tile and compares its OR with 2^15 and 2^23.  A threshold that
is off by one shows only where such an OR is the edge value itself, which depends on how the threads share the values: 32768 and -32769
are therefore planted a second time amid zeros, where the OR is the value however they are shared, and the 4-plane edges lie
in a stream that is zeros but for them."""
import numpy as np

import synth_records as sr
from project_refs import INT32_MAX, INT32_MIN, project_length, sample_planes
from refs import PRESET_LAYERS
from signals import music

S = 1024
P1, P2, P3 = 8001, 20001, 36003             # odd multiples of 3: a frame of one sample reads them at hop 3 and skips them at hop 2
QUIET = 9000                                # zeros on either side of P3
PLANTS = {"planted16": (16, [(0, P1, 32767), (1, P1, -32768)]),
          "planted24": (24, [(0, P1, 32768), (1, P1, -32769), (0, P2, (1 << 23) - 1), (1, P2, -(1 << 23)), (0, P3, 32768), (1, P3, -32769)])}
Q1, Q2 = 9003, 21003
CRAFTED = [(0, Q1, 1 << 23), (1, Q1, -(1 << 23) - 1), (0, Q2, INT32_MAX), (1, Q2, INT32_MIN)]
CRAFTED_SHAPE = sr.SHAPES[2]                # 2 channels, 16 bits, blocks of 1023, no mid/side
CRAFTED_BLOCKS = 32
WIDE_AT = [(0, 1035), (1, 1036), (0, 2045), (1, 2045)]      # both ends of a long run of 4-plane values in the relate tests' "wide values" stream
# (basis, hop, shift): the one-sample basis [[1], [-1], [32767], [-32768]] and a random 19 x 70 one, under both of the kernel's scans
COMBOS = (("one", 1, 1, 0), ("one", 1, 3, 0), ("one", 1, 2, 0), ("b70", 70, 7, 12), ("b70", 70, 70, 12), ("b70", 70, 75, 12))
# name: (frames, the frame that holds the value, its sample (None: the frame's last; "gap": behind the frame), the tile)
PLACEMENTS = {"first": (128, 64, 0, 1), "last": (128, 63, None, 0), "ragged": (101, 100, None, 1), "short": (10, 9, None, 0), "short first": (10, 0, 0, 0), "gap": (128, 70, "gap", 1)}
EVERYWHERE = {("span", k) for k in ("first", "last", "ragged")} | {("frames", k) for k in ("first", "last", "ragged", "gap")}


def planted_signal(name):
    """-> (bits, int32 (2, 46 blocks)): quiet music (below 2^13: 2 planes), zeros around P3, a last block of full-scale noise (which the
    encoder stores RAW), and the values of PLANTS[name]"""
    bits, plants = PLANTS[name]
    x = music(2, 46 * S, 16, seed=70 + bits).astype(np.int32) >> 3
    assert np.abs(x).max() < 1 << 13
    x[:, P3 - QUIET:P3 + QUIET] = 0
    x[:, 45 * S:] = np.random.default_rng(bits).integers(-(1 << (bits - 1)), 1 << (bits - 1), (2, S))
    for ch, p, v in plants:
        x[ch, p] = v
    return bits, np.ascontiguousarray(x)


def crafted_stream():
    """-> (the bytes, the decode they must have): COMPRESS blocks of a record no encoder writes -- every coefficient and both
    pre-emphasis stages zero, so that the cascade adds (1 >> 1) = 0 to every sample and the decode is the residual itself
    (synth_records.synth_plain) -- whose residual is zeros but for 2^23, -2^23 - 1, INT32_MAX and INT32_MIN"""
    sh = CRAFTED_SHAPE
    nl = len(PRESET_LAYERS[sh.preset])
    rec = np.zeros((sh.nch, sr.PARAM_WORDS), dtype=np.int32)
    rec[:, sr.PRM_UNITS:sr.PRM_UNITS + nl] = 1
    rec[:, sr.PRM_RSHIFT:sr.PRM_RSHIFT + nl] = 1
    assert sr.defined(rec, sh.block, sh.preset) and (sh.nch, sh.ms) == (2, False)
    x = np.zeros((sh.nch, CRAFTED_BLOCKS * sh.block + sr.CLOSING_SAMPLES), dtype=np.int32)
    for ch, p, v in CRAFTED:
        x[ch, p] = v
    parts = [x[:, k * sh.block:(k + 1) * sh.block] for k in range(CRAFTED_BLOCKS)]
    return sr.write_stream([rec] * CRAFTED_BLOCKS, parts, [sh.block] * CRAFTED_BLOCKS, sh.nch, sh.bits, sh.block, sh.preset, sh.ms), x


def planes_of(x):
    """project_refs.sample_planes over an array"""
    x = np.asarray(x, dtype=np.int64)
    m = x ^ (x >> 31)
    return 2 + (m >= 1 << 15) + (m >= 1 << 23)


def tile_planes(row, first, n, H, N, before):
    """the kernel's rule from the decoded samples: per tile of 64 frames of a window of channel `row`, (the plane count its widest read
    value needs, the positions that hold a value of that count, every position read, the OR of v ^ (v >> 31) over them).  A sample no
    frame reads -- in the gap of a hop beyond the frame, off the stream -- counts for nothing (off the stream lie zeros: 2 planes)"""
    row = np.asarray(row, dtype=np.int64)
    out = []
    for f0 in range(0, n, 64):
        cnt = min(64, n - f0)
        pos = np.unique(((first + f0 + np.arange(cnt))[:, None] * H - before + np.arange(N)[None, :]).reshape(-1))
        pos = pos[(pos >= 0) & (pos < row.shape[0])]
        pl = planes_of(row[pos])
        top = int(pl.max()) if pos.size else 2
        assert not pos.size or top == max(sample_planes(int(v)) for v in (row[pos].max(), row[pos].min()))
        out.append((top, pos[pl == top].tolist(), pos, int(np.bitwise_or.reduce(row[pos] ^ (row[pos] >> 31))) if pos.size else 0))
    return out


def window_at(p, H, N, f, s):
    """(first, before) of the window whose frame f, counted from its first, has stream sample p as its sample s (s >= N: in the gap
    behind the frame), or None: (first + f) * H - before + s == p with before < N"""
    for before in range(N):
        q = p - s + before - f * H
        if q >= 0 and q % H == 0:
            return q // H, before
    return None


def window_for(full, ch, p, v, N, H, placement):
    """the window of PLACEMENTS[placement] for the value v at sample p of channel ch -> None where the stream has no such window, else
    (first, n, before, whether the premise holds): the value's tile needs the value's plane count and the value is the only one of
    that count it reads (of 2 planes: one of them); in the gap, no tile reads it and its tile needs fewer planes"""
    n, f, s, tile = PLACEMENTS[placement]
    at = next((w for w in (window_at(p, H, N, f, g) for g in (range(N, H) if s == "gap" else [N - 1 if s is None else s])) if w), None)
    if at is None or at[0] + n > project_length(full.shape[1], H):
        return None
    first, before = at
    tiles = tile_planes(full[ch], first, n, H, N, before)
    top, widest, pos, _ = tiles[tile]
    need = sample_planes(v)
    if s == "gap":
        assert all(p not in tl[2] for tl in tiles) and (first + f) * H - before + N <= p < (first + f + 1) * H - before
        return first, n, before, need == 2 or top < need
    assert (first + f) * H - before + (N - 1 if s is None else s) == p and (f == tile * 64 if s == 0 else f == min(n, tile * 64 + 64) - 1)
    return first, n, before, top == need and (widest == [p] if need > 2 else p in widest)


def edge_windows(decodes, found=()):
    """decodes: name -> the decode (C, n) of the streams of PLANTS and of "crafted" (and of those `found` names) -> (windows, counts):
    windows are dicts of stream, ch, p, v, basis, N, hop, shift, first, n, before, placement, scan ("span": H <= N, "frames": H > N),
    must; counts the (plane count, scan) of every tile of every channel of every window.  A chosen value's premise is asserted; a found
    one (found: (stream, ch, p)) gives a window only where its premise holds"""
    targets = [(name, ch, p, v, True) for name, (_, plants) in PLANTS.items() for ch, p, v in plants] + [("crafted", ch, p, v, True) for ch, p, v in CRAFTED]
    targets += [(name, ch, p, int(decodes[name][ch, p]), False) for name, ch, p in found]
    windows, counts = [], set()
    for name, ch, p, v, must in targets:
        full = decodes[name]
        assert int(full[ch, p]) == v
        for basis, N, H, shift in COMBOS:
            scan = "span" if H <= N else "frames"
            for placement in PLACEMENTS:
                if (placement == "gap") and H <= N:
                    continue
                w = window_for(full, ch, p, v, N, H, placement)
                if w is None:
                    continue
                first, n, before, ok = w
                assert ok or not must, (name, ch, p, v, N, H, placement)
                if not ok:
                    continue
                per_channel = [tile_planes(full[c], first, n, H, N, before) for c in range(full.shape[0])]
                counts |= {(tl[0], scan) for tiles in per_channel for tl in tiles}
                windows.append(dict(stream=name, ch=ch, p=p, v=v, basis=basis, N=N, hop=H, shift=shift, first=first, n=n, before=before, placement=placement, scan=scan, must=must,
                                    bare=per_channel[ch][PLACEMENTS[placement][3]][3] == (v ^ (v >> 31)) and placement != "gap"))
    return windows, counts


def assert_coverage(windows, counts):
    """what the issue asks to occur: every plane count under both scans; every chosen value at the tile's first frame's first sample,
    its last frame's last sample, in a ragged last tile (under both scans) and in the gap; each threshold's two edge values in a tile
    whose OR is the value itself; a found 4-plane value among narrower ones under both scans"""
    assert counts >= {(P, scan) for P in (2, 3, 4) for scan in ("span", "frames")}, counts
    chosen = {w["v"] for w in windows if w["must"]}
    assert chosen == {32767, -32768, 32768, -32769, (1 << 23) - 1, -(1 << 23), 1 << 23, -(1 << 23) - 1, INT32_MAX, INT32_MIN}
    for v in chosen:
        got = {(w["scan"], w["placement"]) for w in windows if w["must"] and w["v"] == v}
        assert got >= EVERYWHERE, (v, sorted(EVERYWHERE - got))
    for v in (32768, -32769, 1 << 23, -(1 << 23) - 1):
        got = {(w["scan"], w["placement"]) for w in windows if w["v"] == v and w["bare"]}
        assert got >= {k for k in EVERYWHERE if k[1] != "gap"}, (v, got)
    assert {w["scan"] for w in windows if not w["must"]} == {"span", "frames"} and all(sample_planes(w["v"]) == 4 for w in windows if not w["must"])
