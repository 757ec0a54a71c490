"""GPU tests of LINNEAmd_ProjectWindowsDevice at sample positions up to 2^32 - 1, with images and tables that lie more than 2^32 words
from their bases, at its documented bound of 2^40 products a window, and with more tiles than one launch may have.  The streams are
tests/far_streams.py's two of 2^32 - 1 samples (an island of sound across 2^31, one 70000 samples before the end); every expected row
is far_streams.far_project's, which cuts the frames that touch an island from the virtual decode, never allocates such a stream, and
which tests/test_far_streams_cpu.py holds to project_refs.expected_project at reduced scale.  Every other frame reads zeros alone and
must be zeros.  No expected value comes from the library under test; every word between sentinels must equal the reference's.  Where a
table is too large to copy whole (the bound's 1 GiB, the 16 GiB of the far strides) the test says what is compared on the device and
what on the host."""
import ctypes as C
import time

import numpy as np
import pytest

import far_streams as fs
import linne_amd
from far_streams import A_START as A, B_START as B, ISLAND_SAMPLES as LA, N32, SHAPES
from project_refs import project_length
from stream_consumers import KIND, last_error, to_device
from test_gpu_stream_far import FarTrack
from test_gpu_stream_project import SENTINEL, item, random_basis, raw_project, strides

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NG = 0, 1, 7
HALF = 1 << 31
NAMES = tuple(SHAPES)
MAX_TILES = 0xFFFFFF


@pytest.fixture(scope="module")
def made(oracle):
    return {name: fs.full_scale(oracle, name) for name in NAMES}


def tracks(c, made):
    devs = [to_device(made[name][0]) for name in NAMES]
    return {name: FarTrack(name, made[name][1], dev, x) for name, dev, x in zip(NAMES, devs, c.index_streams(devs))}


@pytest.fixture(scope="module")
def far(ctx, made):
    out = tracks(ctx, made)
    yield out
    for t in out.values():
        t.index.close()


def reference(it):
    return fs.far_project(it["t"].pcm, it["first"], it["n"], it["basis"], it["hop"], it["before"], it["shift"], it["clip"], it["f32"], it["fexp"])


def want_words(items, offs, size, refs):
    """sentinels but the windows' elements: zeros, and the reference's rows at the frames that touch an island"""
    buf = np.full(size, SENTINEL, dtype=np.uint32)
    for it, off, (idx, rows, _) in zip(items, offs, refs):
        cs, fst, rs = strides(it)
        K = it["basis"].shape[0]
        c, f, k = np.meshgrid(np.arange(it["t"].nch), np.arange(it["n"]), np.arange(K), indexing="ij")
        buf[off + c * cs + f * fst + k * rs] = 0
        c, f, k = np.meshgrid(np.arange(it["t"].nch), idx, np.arange(K), indexing="ij")
        buf[off + c * cs + f * fst + k * rs] = np.ascontiguousarray(rows).view(np.uint32)
    return buf


def held(c, items, group_frames=(0, 2)):
    """the call at every group_frames: the codes, every word of the buffer and the saturated words are the reference's -> the references"""
    refs = [reference(it) for it in items]
    for gf in group_frames:
        ret, codes, buf, offs, sats = raw_project(c, items, gf)
        assert ret == OK and codes == [OK] * len(items), (gf, codes, last_error(c))
        want = want_words(items, offs, len(buf), refs)
        bad = np.flatnonzero(buf != want)
        if bad.size:
            j = max(k for k in range(len(offs)) if offs[k] <= bad[0]) if bad[0] >= offs[0] else -1
            it = items[j]
            raise AssertionError(f"group_frames {gf}: word {bad[0]} (window {j} begins at {offs[j]}: {it['t'].name} N {it['basis'].shape[1]} K {it['basis'].shape[0]} H {it['hop']} "
                                 f"first {it['first']} n {it['n']} before {it['before']} {it['order']}) is {int(buf[bad[0]]):#x}, not {int(want[bad[0]]):#x}; {bad.size} words differ")
        assert sats == [int(r[2]) for r in refs], (gf, sats)
    return refs


def call(c, wins, group_frames=0):
    """LINNEAmd_ProjectWindowsDevice on windows that name their own memory: dicts of t, first, n, basis, hop, before, shift, clip, f32,
    fexp, ptr (the table's address) and cs, fs, rs (its strides in elements) -> (ret, codes, saturated words (7: left as it was))"""
    import torch
    W = len(wins)
    w, sp = (linne_amd.Window * W)(), (linne_amd.ProjectSpec * W)()
    for j, q in enumerate(wins):
        t, basis = q["t"], q["basis"]
        assert basis.dtype == np.int16 and basis.flags["C_CONTIGUOUS"]
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].result, w[j].d_pcm, w[j].pcm_stride = t.index.h, t.dev.data_ptr(), q["first"], q["n"], -1, q["ptr"], 0
        sp[j].frame_len, sp[j].hop, sp[j].num_rows, sp[j].before, sp[j].shift, sp[j].clip_bits = basis.shape[1], q["hop"], basis.shape[0], q.get("before", 0), q.get("shift", 0), q.get("clip", 0)
        sp[j].format, sp[j].float_exp = (linne_amd.PCM_F32 if q.get("f32") else linne_amd.PCM_S32), q.get("fexp", 0)
        sp[j].channel_stride, sp[j].frame_stride, sp[j].row_stride, sp[j].saturated, sp[j].reserved = q["cs"], q["fs"], q["rs"], 7, 0
        sp[j].basis = basis.ctypes.data_as(C.POINTER(C.c_int16))
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_ProjectWindowsDevice(c.h, w, sp, W, group_frames)
    torch.cuda.synchronize()
    return ret, [w[j].result for j in range(W)], [int(sp[j].saturated) for j in range(W)]


# A1 -----------------------------------------------------------------------------------------------------------------------------
def far_items(far):
    rng = np.random.default_rng(41)
    b70, b1, b64 = random_basis(rng, 19, 70), np.array([[1], [-1], [32767], [-32768]], dtype=np.int16), random_basis(rng, 5, 64)
    items = []

    def add(t, first, n, basis, H, before, **more):
        assert 0 <= first and first + n <= project_length(N32, H)
        f32, sh, cb, order, pad = (int(v) for v in rng.integers(0, (2, 4, 4, 2, 3)))         # (drawn, so that no choice goes with one kind of window alone)
        items.append(item(t, first, n, basis, H, before=before, shift=(0, 15, 31, 7)[sh], clip_bits=(0, 16, 24, 32)[cb], f32=f32 == 1, float_exp=31 if f32 == 1 else 0,
                          order=("fk", "kf")[order], pad=(0, 3, 1)[pad], **more))
    for t in (far["far16"], far["far24"]):
        for basis in (b70, b64):
            N = basis.shape[1]
            for j, H in enumerate((1, 3, N, N + 5)):
                F = project_length(N32, H)
                b0, b1_ = (0, N - 1)[j % 2], (N - 1, 0)[j % 2]
                add(t, (A - 40) // H, min(-(-300 // H), 120) if H > 1 else 130, basis, H, b0)       # into island A
                add(t, (HALF - 60) // H, -(-200 // H), basis, H, b1_)                               # across sample 2^31
                add(t, (B + LA - 150) // H, -(-300 // H), basis, H, b0)                             # off island B, into its SILENT block
                add(t, F - 40, 40, basis, H, b1_, last=True)                                        # the stream's last frames: the halo runs off 2^32 - 1
        add(t, HALF + 5, 150, b70, 1, 0)                        # a first frame above 2^31 at hop 1
        add(t, HALF + 1000, 700, b1, 1, 0)                      # island A's end, sample by sample
        add(t, (B - 20) // 3, 90, b1, 3, 0)
        # hop 65536: frame 32768 reads from 2^31 on, inside island A; its neighbours and the stream's last frames read silence
        add(t, 32760, 17, b70, 65536, 0)
        add(t, 32768, 1, b64, 65536, 63)
        add(t, 65536 - 70, 70, b70, 65536, 69)
    return items


def test_values_at_far_positions(ctx, far):
    """both stream shapes in one call: frames around island A and across sample 2^31, around island B, and the stream's last frames; hops
    1, 3, N, N + 5 and 65536; before at 0 and N - 1; both stride orders, padded strides; int32 and float32; every shift and clip"""
    items = far_items(far)
    refs = held(ctx, items)
    loud = [bool(r[1].any()) for r in refs]
    assert sum(loud) >= 3 and sum(1 for it, l in zip(items, loud) if l and it["first"] * it["hop"] > HALF) >= 3      # non-zero rows, from frames that begin above 2^31
    assert any(it["hop"] == 1 and it["first"] > HALF and l for it, l in zip(items, loud))
    assert {it["hop"] for it in items} >= {1, 3, 64, 69, 70, 75, 65536} and {it["before"] for it in items} >= {0, 63, 69}
    # what is drawn per window occurs among the windows with non-zero rows, in both stream shapes
    for name in NAMES:
        mine = [it for it, l in zip(items, loud) if l and it["t"].name == name]
        assert {(it["f32"], it["order"]) for it in mine} == {(a, b) for a in (False, True) for b in ("fk", "kf")} and {it["pad"] for it in mine} == {0, 1, 3}
        assert {it["shift"] for it in mine} == {0, 7, 15, 31} and {it["clip"] for it in mine} == {0, 16, 24, 32}
    # the window at hop 65536 alternates: silence, island, silence
    j = next(i for i, it in enumerate(items) if it["hop"] == 65536 and it["n"] == 17)
    assert refs[j][0].tolist() == [8] and loud[j] and 0 < 8 < 16
    # the last frames read beyond the stream: their halo is zeros, not the memory behind the stream
    assert all(it["first"] + it["n"] == project_length(N32, it["hop"]) and (it["first"] + it["n"] - 1) * it["hop"] - it["before"] + it["basis"].shape[1] > N32
               for it in items if it.get("last") and it["before"] == 0)
    assert sum(1 for it in items if it.get("last") and it["before"] == 0) >= 4


# A2 -----------------------------------------------------------------------------------------------------------------------------
def test_images_beyond_2_32_words(made):
    """a window of 32769 frames at hop 65536 of the two-channel stream: a channel of its image is 2^31 + 8 words, so that its last frame
    -- frame 32768, which reads island A from sample 2^31 on -- lies behind word 2^31 of the first channel and behind word 2^32 of the
    second, and the window behind it, at hop 1 over island A, has its image behind word 2^32.  On a context of its own, closed at the
    end, so that the suite's context does not keep the 16 GiB of scratch."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 20 << 30:
        pytest.skip("%.1f GiB of device memory free: the images take 16 GiB" % (free / 2 ** 30))
    c = linne_amd.Context(0, use_torch_stream=False)
    far = tracks(c, made)
    try:
        t = far["far16"]
        rng = np.random.default_rng(43)
        b8, b70 = random_basis(rng, 3, 8), random_basis(rng, 19, 70)
        items = [item(t, 0, 32769, b8, 65536, before=0, shift=3), item(t, A - 100, 400, b70, 1, before=69, shift=15, order="kf", pad=1)]
        # the plan's arithmetic (lnn_windows_plan.h wx_project_record): the images of a call's windows follow each other, a channel's
        # words ((n - 1) * H + N + 3) & ~3 apart
        istride = [((it["n"] - 1) * it["hop"] + it["basis"].shape[1] + 3) & ~3 for it in items]
        img = [0, t.nch * istride[0]]
        assert t.nch == 2 and istride[0] == HALF + 8 and img[1] == (1 << 32) + 16 > 1 << 32
        assert 32768 * 65536 == HALF and img[0] + istride[0] + 32768 * 65536 > 1 << 32            # the last frame of the last channel
        assert 4 * (img[1] + 2 * istride[1]) < 17 << 30
        refs = held(c, items)
        assert refs[0][0].tolist() == [32768] and refs[0][1][1].any() and refs[1][1].any()       # the island is in the last channel's last frame
    finally:
        for x in far.values():
            x.index.close()
        c.close()


def test_tables_beyond_2_32_elements(ctx, far):
    """two windows whose strides put elements more than 2^32 elements (16 GiB) from d_pcm, into one allocation of 2^32 + 4096 words of
    sentinels: three frames by two rows of two channels over island A, once with the channels 2^32 + 5 elements apart, once with the
    frames 2^31 + 3 apart.  On the device: the number of words that are no sentinel is at most the elements written, and the elements
    and both neighbours of each are gathered; on the host: the gathered elements equal the reference's, the neighbours that are no
    element are sentinels."""
    import torch
    if torch.cuda.mem_get_info()[0] < 20 << 30:
        pytest.skip("less than 20 GiB of device memory free: the table takes 16 GiB")
    t = far["far16"]
    words = (1 << 32) + 4096
    buf = torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
    try:
        basis = random_basis(np.random.default_rng(44), 2, 70)
        spec = dict(t=t, first=(A + 200) // 70, n=3, basis=basis, hop=70, before=0, shift=9)
        wins = [dict(spec, ptr=buf.data_ptr() + 4 * 16, cs=(1 << 32) + 5, fs=2, rs=1), dict(spec, ptr=buf.data_ptr() + 4 * 1024, cs=7, fs=HALF + 3, rs=1, first=(A + 900) // 70)]
        idx, rows, sat = zip(*(fs.far_project(t.pcm, q["first"], 3, basis, 70, 0, 9) for q in wins))
        assert all(i.tolist() == [0, 1, 2] and r.any(axis=2).all() for i, r in zip(idx, rows))
        where, value = [], []
        for q, off, r in zip(wins, (16, 1024), rows):
            for ch in range(2):
                for f in range(3):
                    for k in range(2):
                        where.append(off + ch * q["cs"] + f * q["fs"] + k * q["rs"])
                        value.append(int(r[ch, f, k]) & 0xFFFFFFFF)
        assert len(set(where)) == 24 and max(where) < words - 1
        assert sum(1 for x in where[:12] if x - 16 > 1 << 32) == 6 and sum(1 for x in where[12:] if x - 1024 > 1 << 32) == 4
        ret, codes, sats = call(ctx, wins)
        assert ret == OK and codes == [OK, OK] and sats == [int(s) for s in sat], last_error(ctx)
        near = sorted(set(where) | {x - 1 for x in where} | {x + 1 for x in where})
        got = buf[torch.tensor(near, dtype=torch.int64, device="cuda")].cpu().numpy().view(np.uint32)
        want = dict(zip(where, value))
        assert got.tolist() == [want.get(x, SENTINEL) for x in near]
        changed = sum(int((buf[a:a + (1 << 28)] != SENTINEL).sum()) for a in range(0, words, 1 << 28))
        assert changed == sum(1 for v in value if v != SENTINEL)
    finally:
        del buf
        torch.cuda.empty_cache()


# A3 -----------------------------------------------------------------------------------------------------------------------------
def test_a_window_at_the_products_bound(ctx, far):
    """exactly 2^40 products in one window: frame_len 4096, 2048 rows, 2 channels, 2^16 frames at hop 64 centred on island A.  The table
    is 1 GiB between sentinels and stays on the device, where everything outside the rows of the frames that touch the island (about a
    hundred; the reference computes those alone) must be zeros and the sentinels whole; those rows come to the host and equal the
    reference's.  One frame more is refused with the table untouched."""
    import torch
    t = far["far16"]
    N, K, n, H = 4096, 2048, 1 << 16, 64
    assert n * K * N * t.nch == 1 << 40 == linne_amd.PROJECT_MAX_PRODUCTS and (N, K) == (linne_amd.PROJECT_MAX_FRAME, linne_amd.PROJECT_MAX_ROWS)
    first = HALF // H - n // 2
    basis = random_basis(np.random.default_rng(45), K, N)
    t0 = time.perf_counter()
    idx, rows, sat = fs.far_project(t.pcm, first, n, basis, H, before=N // 2, shift=14, clip_bits=0)
    t_ref = time.perf_counter() - t0
    a, b = int(idx[0]), int(idx[-1]) + 1
    assert idx.tolist() == list(range(a, b)) and 100 <= b - a <= 130 and 0 < a and b < n and rows.any(axis=2).all()
    pad = 4
    buf = torch.full((pad + t.nch * (n + 1) * K + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    spec = dict(t=t, first=first, basis=basis, hop=H, before=N // 2, shift=14, ptr=buf.data_ptr() + 4 * pad, fs=K, rs=1)
    ret, codes, sats = call(ctx, [dict(spec, n=n + 1, cs=(n + 1) * K)])
    assert (ret, codes, sats) == (INVALID_ARGUMENT, [INVALID_ARGUMENT], [7]) and "> 2^40 products" in last_error(ctx)
    assert bool((buf == SENTINEL).all())
    t0 = time.perf_counter()
    ret, codes, sats = call(ctx, [dict(spec, n=n, cs=n * K)])
    t_gpu = time.perf_counter() - t0
    print("the products' bound: the call %.3f s, the reference %.3f s" % (t_gpu, t_ref))
    assert ret == OK and codes == [OK] and sats == [int(sat)], last_error(ctx)
    table = buf[pad:pad + t.nch * n * K].view(t.nch, n, K)
    assert not bool(table[:, :a].any()) and not bool(table[:, b:].any())                      # on the device: silence is zeros
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + t.nch * n * K:] == SENTINEL).all())
    assert np.array_equal(table[:, a:b].cpu().numpy(), rows)                                     # on the host: the island's rows
    del table, buf
    torch.cuda.empty_cache()


# A4 -----------------------------------------------------------------------------------------------------------------------------
def test_too_many_tiles_are_refused(ctx, far):
    """2^29 - 31 frames of one sample by one row at hop 1, two channels: 2 * 2^23 tiles, one more than a launch of 256-thread workgroups
    may have below 2^32 threads.  Refused before any launch; nothing is written.  (The strides keep the elements apart; the memory
    behind them is never touched, so there is none.)"""
    import torch
    t = far["far16"]
    n = 64 * MAX_TILES // 2 + 1
    tiles = t.nch * -(-n // 64)
    assert n > 64 * MAX_TILES / 2 and tiles == MAX_TILES + 1 and n * t.nch <= linne_amd.PROJECT_MAX_PRODUCTS and n <= project_length(N32, 1)
    buf = torch.full((4096,), SENTINEL, dtype=torch.int32, device="cuda")
    one = np.array([[1]], dtype=np.int16)
    ctx.enable_timing(True)
    try:
        ctx.measure_windows([(t.dev, t.index, A, 100)])              # (the launches of the call before are another kind's)
        ret, codes, sats = call(ctx, [dict(t=t, first=5, n=n, basis=one, hop=1, ptr=buf.data_ptr() + 64, cs=n, fs=1, rs=1)])
        assert (ret, codes, sats) == (NG, [NG], [7]), (ret, codes, last_error(ctx))
        assert last_error(ctx) == "ProjectWindowsDevice: %d tiles of outputs in one call: too many" % tiles
        assert bool((buf == SENTINEL).all())
        assert all(ctx.last_launches(KIND[k]) <= 0 for k in ("PROJECT_T_PRESET", "PROJECT_T_PROJECT", "T_WX_PLACE"))
    finally:
        ctx.enable_timing(False)
