"""CPU side of the windows calls (DecodeWindowsDevice and the calls that compare, measure and digest): the host's plan of a call
(linne_amd/csrc/lnn_windows_plan.h), driven by a small stand-alone program over synthetic block indexes and held to a short
restatement of its contract -- which records go into which pass, where a COMPRESS block lies in a pass's packed segment, what the
lists are reserved for, and where a bucketed consumer's accumulators lie.  The program is built twice, the second time with the
address and undefined-behaviour sanitizers, and both run every case."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
COMPRESS, SILENT, RAW, TAIL = 0, 1, 2, 3
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
/* stdin: group_frames bucketing nstreams nwindows; per stream: C bits S nb covered stream_bytes address, then nb x (off first size type
 * nsmp); per window: stream lo n bucket_samples */
struct Stream { WxIndexView x; std::vector<uint64_t> off, first; std::vector<uint32_t> size, type, nsmp; unsigned long long address; };
int main(void)
{
    unsigned gf, bucketing, ns, nw;
    if (scanf("%u %u %u %u", &gf, &bucketing, &ns, &nw) != 4) return 2;
    std::vector<Stream> st(ns);
    for (Stream &s : st) {
        unsigned long long covered, bytes;
        memset(&s.x, 0, sizeof(s.x));
        if (scanf("%u %u %u %u %llu %llu %llu", &s.x.shape.num_channels, &s.x.shape.bits_per_sample, &s.x.shape.num_samples_per_block, &s.x.nb, &covered, &bytes, &s.address) != 7) return 2;
        s.x.covered = covered; s.x.stream_bytes = bytes;
        for (uint32_t r = 0; r < s.x.nb; r++) {
            unsigned long long off, first; unsigned size, type, nsmp;
            if (scanf("%llu %llu %u %u %u", &off, &first, &size, &type, &nsmp) != 5) return 2;
            s.off.push_back(off); s.first.push_back(first); s.size.push_back(size); s.type.push_back(type); s.nsmp.push_back(nsmp);
        }
        s.x.h_off = s.off.data(); s.x.h_first = s.first.data(); s.x.h_size = s.size.data(); s.x.h_type = s.type.data(); s.x.h_nsmp = s.nsmp.data();
    }
    std::vector<WxRange> rg(nw);
    for (WxRange &r : rg) {
        unsigned k; unsigned long long lo, n, b;
        if (scanf("%u %llu %llu %llu", &k, &lo, &n, &b) != 4 || k >= ns) return 2;
        memset(&r, 0, sizeof(r));
        r.x = st[k].x; r.stream = (const uint8_t *)(uintptr_t)st[k].address; r.lo = lo; r.n = n; r.live = n != 0; r.bucket_samples = b;
        r.fmt = LINNE_AMD_PCM_S32; r.sstride = 1; r.stride = n;
        if (n) r.r1 = (lo + n - 1u < r.x.covered) ? wx_block_of(r.x.h_first, r.x.nb, lo + n - 1u) : r.x.nb;
    }
    WxPlanned p;
    const int why = wx_plan_count(rg.data(), nw, gf, p);
    printf("count %d %llu %llu %llu %u\n", why, (unsigned long long)p.nlive, (unsigned long long)p.total_rec, (unsigned long long)p.total_crec, p.ngroups);
    if (why != WXP_OK) return 0;
    const WxLists ls = wx_lists(p, nw, 0, bucketing ? sizeof(WxBucket) : 0);
    printf("lists %llu %llu %llu %llu %llu %llu\n", (unsigned long long)ls.back_bytes, (unsigned long long)ls.o_win, (unsigned long long)ls.o_side, (unsigned long long)ls.o_rec,
            (unsigned long long)ls.o_crec, (unsigned long long)ls.bytes);
    /* exactly the reserved sizes, from the heap: the sanitizer build sees a record written past them */
    std::vector<WxWindow> win(p.nlive); std::vector<WxBucket> side(bucketing ? p.nlive : 0); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
    wx_plan_fill(rg.data(), nw, gf, (WxBucketing)bucketing, p, win.data(), bucketing ? side.data() : NULL, rec.data(), crec.data());
    printf("fill %u %u %u %llu %llu %llu\n", p.nwin, p.nrec, p.ncrec, (unsigned long long)p.scratch_bytes, (unsigned long long)p.nacc, (unsigned long long)p.nout);
    for (uint32_t i = 0; i < nw; i++) printf("plan %d %u %u %u\n", p.win[i].group, p.win[i].r0, p.win[i].nr, p.win[i].ncomp);
    for (uint32_t i = 0; i < p.nwin; i++) printf("win %llu %llu %llu %u\n", (unsigned long long)win[i].lo, (unsigned long long)win[i].hi, (unsigned long long)win[i].covered, win[i].fidx);
    for (size_t i = 0; i < side.size(); i++) printf("bucket %llu %llu %u %llu %llu %u %u %u %llu\n", (unsigned long long)side[i].b, (unsigned long long)side[i].nb, side[i].ns,
            (unsigned long long)side[i].abase, (unsigned long long)side[i].obase, side[i].fidx, side[i].C, side[i].sstride, (unsigned long long)side[i].n);
    for (const WxPass &q : p.passes) printf("pass %u %u %u %u %u %llu %d\n", q.group, q.rec0, q.nrec, q.c0, q.nc, (unsigned long long)q.seg_bytes, q.check_only);
    for (uint32_t i = 0; i < p.nrec; i++) printf("rec %u %u %u %u %llu %llu %u %llu %llu\n", rec[i].type, rec[i].win, rec[i].blk, rec[i].cidx, (unsigned long long)rec[i].off,
            (unsigned long long)rec[i].dst, rec[i].size, (unsigned long long)(uintptr_t)rec[i].b, (unsigned long long)rec[i].N);
    for (uint32_t i = 0; i < p.ncrec; i++) printf("crec %u\n", crec[i]);
    return 0;
}
"""


def stream(C, bits, S, types, sizes, address, short_of=0):
    """a synthetic index: blocks of S samples (the last one short by `short_of`), `sizes` their size fields"""
    blocks, off, first = [], 30, 0
    for k, (t, size) in enumerate(zip(types, sizes)):
        nsmp = S - (short_of if k == len(types) - 1 else 0)
        blocks.append((off, first, size, t, nsmp))
        off += size + 6
        first += nsmp
    return {"C": C, "bits": bits, "S": S, "blocks": blocks, "covered": first, "bytes": off, "address": address}


A = stream(2, 16, 64, [COMPRESS, SILENT, COMPRESS, RAW, COMPRESS, COMPRESS], [37, 5, 52, 261, 21, 44], 0x10000 + 3, short_of=10)   # covered 374
B = stream(1, 24, 32, [RAW, COMPRESS, COMPRESS, SILENT], [101, 19, 33, 5], 0x20000 + 9)                                            # covered 128
STREAMS = [A, B]
# (stream, lo, n): n == 0 is an empty window; the streams' headers promise more samples than their blocks hold (covered), so a window
# may straddle `covered` or lie wholly beyond it
CASES = {
    "one": [(0, 0, 374)],
    "empty_and_inside": [(0, 5, 0), (0, 70, 100)],
    "beyond_and_straddling": [(0, 380, 20), (0, 300, 100), (1, 120, 30)],
    "overlapping": [(0, 10, 200), (0, 100, 274), (1, 0, 128)],
    "six": [(1, 31, 2), (0, 0, 374), (0, 5, 0), (1, 40, 100), (0, 374, 9), (0, 63, 258)],
    "silent_only": [(0, 64, 64), (1, 96, 32)],
}
BUCKETS = [0, 7, 8192, 1]                                      # per window, cycled


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("windows_plan")
    src = str(d / "plan.cpp")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    exes = []
    for name, extra in (("plan", []), ("plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        b = subprocess.run(cmd + ["-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        exes.append(exe)
    return exes


def run(programs, windows, gf, bucketing, residue=0, streams=STREAMS, buckets=BUCKETS):
    text = ["%d %d %d %d" % (gf, bucketing, len(streams), len(windows))]
    for s in streams:
        text.append("%d %d %d %d %d %d %d" % (s["C"], s["bits"], s["S"], len(s["blocks"]), s["covered"], s["bytes"], s["address"] + residue))
        text += ["%d %d %d %d %d" % b for b in s["blocks"]]
    text += ["%d %d %d %d" % (k, lo, n, buckets[i % len(buckets)]) for i, (k, lo, n) in enumerate(windows)]
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    got = {}
    for line in outs[0].splitlines():
        key, *v = line.split()
        got.setdefault(key, []).append([int(x) for x in v])
    return got


def expected_blocks(s, lo, n):
    """the blocks of stream s that [lo, lo + n) overlaps, and whether it reaches beyond them"""
    hits = [r for r, (_, first, _, _, nsmp) in enumerate(s["blocks"]) if first < lo + n and lo < first + nsmp]
    return hits, lo + n > s["covered"]


def slots(b):
    ns = 1
    while ns < 64 and (b >> 12) >= 2 * ns:
        ns *= 2
    return ns


@pytest.mark.parametrize("residue", [0, 5, 15])
@pytest.mark.parametrize("bucketing", [0, 1, 2])
@pytest.mark.parametrize("gf", [0, 1, 2, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plan(programs, case, gf, bucketing, residue):
    windows = CASES[case]
    g = run(programs, windows, gf, bucketing, residue)
    why, nlive, total_rec, total_crec, ngroups = g["count"][0]
    live = [i for i, (_, _, n) in enumerate(windows) if n]
    assert why == 0 and nlive == len(live) and ngroups == len({windows[i][0] for i in live})
    nwin, nrec, ncrec, scratch, nacc, nout = g["fill"][0]
    # what was written never exceeds what the lists were reserved for
    assert nwin == nlive and nrec <= total_rec and ncrec <= total_crec
    back, o_win, o_side, o_rec, o_crec, lbytes = g["lists"][0]
    assert back == 8 * len(windows) and o_win >= back and o_side >= o_win + 56 * nlive and o_rec >= o_side + (64 * nlive if bucketing else 0)
    assert o_crec >= o_rec + 64 * total_rec and lbytes >= o_crec + 4 * (total_crec + 1) and all(v % 256 == 0 for v in (o_win, o_side, o_rec, o_crec, lbytes))
    recs, crec, passes, wins = g.get("rec", []), [v[0] for v in g.get("crec", [])], g["pass"], g["win"]
    assert len(recs) == nrec and len(crec) == ncrec and len(wins) == nwin
    # window records: the groups in order of first appearance, a group's windows in the caller's order
    order = [i for k in dict.fromkeys(windows[i][0] for i in live) for i in live if windows[i][0] == k]
    assert [w[3] for w in wins] == order
    for w, i in zip(wins, order):
        k, lo, n = windows[i]
        assert w[:3] == [lo, lo + n, STREAMS[k]["covered"]]
    for i, (k, lo, n) in enumerate(windows):
        group, r0, nr, ncomp = g["plan"][i]
        if not n:
            assert group == -1
            continue
        hits, _ = expected_blocks(STREAMS[k], lo, n)
        assert (nr, ncomp) == (len(hits), sum(STREAMS[k]["blocks"][r][3] == COMPRESS for r in hits)) and (not hits or r0 == hits[0])
    # the passes tile the records and the COMPRESS entries
    at = cat = 0
    for group, rec0, n_, c0, nc, seg, check_only in passes:
        assert (rec0, c0) == (at, cat) and n_ > 0
        at += n_
        cat += nc
        assert gf == 0 or nc <= gf                              # no pass holds more than group_frames COMPRESS records
        mine = recs[rec0:rec0 + n_]
        comp = [j for j, r in enumerate(mine) if r[0] == COMPRESS]
        assert crec[c0:c0 + nc] == comp and [mine[j][3] for j in comp] == list(range(nc))       # cidx and crec are consistent
        assert all(r[3] == 0xFFFFFFFF for r in mine if r[0] != COMPRESS)
        assert all(windows[wins[r[1]][3]][0] == windows[wins[mine[0][1]][3]][0] for r in mine)  # one group's windows
        # slots: whole 16-byte groups, disjoint and in order, the block at its source's address modulo 16; seg_bytes ends the last
        end = 0
        for j in comp:
            _, _, _, _, off, dst, size, b, N = mine[j]
            assert dst & 15 == (b + off) & 15 and dst & ~15 == end
            end = (dst + size + 6 + 15) & ~15
        assert seg == end
        if check_only:
            assert comp == list(range(n_)) and len({r[1] for r in mine}) == 1
    assert (at, cat) == (nrec, ncrec)
    # every live window: its blocks exactly once in placing passes, in order, the tail first; a window of more COMPRESS blocks than a
    # pass takes has all of them in check-only passes before its first placing pass
    placing = [r + [pi] for pi, p in enumerate(passes) if not p[6] for r in recs[p[1]:p[1] + p[2]]]
    checking = [r + [pi] for pi, p in enumerate(passes) if p[6] for r in recs[p[1]:p[1] + p[2]]]
    for wi, i in enumerate(order):
        k, lo, n = windows[i]
        s = STREAMS[k]
        hits, tail = expected_blocks(s, lo, n)
        mine = [r for r in placing if r[1] == wi]
        assert [(r[0], r[2]) for r in mine] == ([(TAIL, 0)] if tail else []) + [(s["blocks"][r][3], r) for r in hits]
        for r in mine:
            if r[0] != TAIL:
                assert (r[4], r[6], r[7], r[8]) == (s["blocks"][r[2]][0], s["blocks"][r[2]][2], s["address"] + residue, s["bytes"])
        comp = [r for r in hits if s["blocks"][r][3] == COMPRESS]
        checked = [r for r in checking if r[1] == wi]
        if gf and len(comp) > gf:
            assert [r[2] for r in checked] == comp and max(r[-1] for r in checked) < min(r[-1] for r in mine)
        else:
            assert not checked
    # buckets
    if bucketing:
        a = o = 0
        for bk, i in zip(g["bucket"], order):
            k, lo, n = windows[i]
            b_, nb, ns, abase, obase, fidx, cf, sstride, n_or_cstride = bk
            spec = BUCKETS[i % len(BUCKETS)]
            C, w = STREAMS[k]["C"], (STREAMS[k]["bits"] + 7) // 8
            assert b_ == (n if spec == 0 or spec > n else spec) and nb == -(-n // b_) and fidx == i
            assert ns == slots(b_) and ns in (1, 2, 4, 8, 16, 32, 64) and (b_ >= 8192 or ns == 1)
            assert (abase, obase) == (a, o)                     # disjoint accumulator ranges; obase the running sum
            if bucketing == 1:
                assert cf == C and sstride == 0
                a += ns * C * nb
                o += C * nb
            else:
                assert cf == C * w and n_or_cstride == n and sstride % 16 == 0 and sstride >= nb
                a += ns * sstride if ns > 1 else nb
                o += nb
        assert (nacc, nout) == (a, o)
    else:
        assert "bucket" not in g and (nacc, nout) == (0, 0)


def test_slots_of_long_buckets(programs):
    """a window of one long bucket gets slots: the rule at its steps"""
    long = stream(1, 16, 4096, [SILENT] * 40, [5] * 40, 0x30000)
    for n, ns in ((8191, 1), (8192, 2), (16383, 2), (16384, 4), (40 * 4096, 32)):
        g = run(programs, [(0, 0, n)], 0, 2, streams=[long], buckets=[0])
        assert g["bucket"][0][2] == ns == slots(n) and g["bucket"][0][7] == 16 and g["fill"][0][4] == (ns * 16 if ns > 1 else 1)
