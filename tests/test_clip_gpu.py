"""The clipped mode on the GPU (kernels_chain_align.hip.h and kernels_map.hip.h with CLIP = true) against tests/clip_ref.py: the device
primitive on hand-made chains over a text of three records -- every length, junk tails, the two sides of the end-bonus decision, reads
hanging over the text's ends and over a record join, indels inside and outside the band, ties, N, gaps on both sides of the class
edges with both ends clipped, bad chains, every launch size, streams, the census, an amino text -- and the batch entry points end to
end: against the reference, and against the composition that needs no reference.  Everything must be equal: records, run counts,
offsets, runs, status."""
import ctypes as C
import os

import numpy as np
import pytest

from awry_amd.fm_index import (ALN_BAD_CHAIN, ALN_CLIP_DTYPE, ALN_OK, ALN_SKEW, CHAIN_DTYPE, ERR_ARG, ERR_INVALID_QUERY, MAP_CLIP_DTYPE, MAP_SECONDARY,
                               AwryError, FmIndex, cigar_string, pack_queries)
from tests import chain_align_ref as ca
from tests import chain_ref as cr
from tests import clip_ref as cl
from tests import map_ref as mp
from tests import mismatch_ref as mr
from tests import synth
from tests.test_chain_align_gpu import KEY, pack_job, substitute
from tests.test_chain_gpu import E2E_PARAMS
from tests.test_map_gpu import OracleWorld, positions_of
from tests.test_smems_gpu import World

pytestmark = pytest.mark.gpu

BANDS = (0, 1, 4, 8)
LENGTHS = (1, 2, 17, 64, 65, 101, 1024)
TAILS = (1, 3, 4, 5, 16, 60)
HANGS = (1, 16, 17, 100)
SKEWS = (0, 1, 6, 7, 8, 9, 14, 15, 16, 17)  # |b - a| of a gap: both sides of the class edges at every band, and one past the limit
LAUNCH_SIZES = (0, 1, 255, 256, 257, 3000)
# (a, b, g, E): the issue's four, and (1, 4, 6) at every end bonus that decides a single mismatch at the last letter (H* - H_e = 4)
WEIGHTS = ((1, 4, 6, 5), (2, 3, 4, 0), (1, 1, 1, 0), (1, 0, 1, 0), (1, 4, 6, 0), (1, 4, 6, 3), (1, 4, 6, 4), (1, 4, 6, 1024))
MAIN = (1, 4, 6, 5)
P_MAIN = E2E_PARAMS[KEY]


def symbols(x, alphabet=0):
    return [int(v) for v in mr.to_symbols(bytes(x), alphabet)]


# ---- the device primitive on hand-made chains ---------------------------------------------------------------------------------

def small_text(alphabet=0):
    """a few thousand letters in three records, with an "AC" x 40 stretch planted in the first"""
    text, st, hd = synth.make_text(6_000, alphabet, (77, 76)[alphabet], 3, 0.02)  # (seeds that give a first record of 1900+ letters)
    assert len(st) == 3 and int(st[1]) > 1600 and int(st[2]) - int(st[1]) > 300
    text = np.array(text, copy=True)
    text[400:480] = np.frombuffer((b"AC" if alphabet == 0 else b"WY") * 40, np.uint8)
    return text, st, hd


def clip_cases(text, st, letters=b"ACGT", filler=b"A"):
    """-> [(name, query, members)]"""
    tb = bytes(text[:-1])
    n = len(tb)
    rng = np.random.default_rng(9)
    rnd = lambda k: bytes(letters[int(x)] for x in rng.integers(0, len(letters), size=k))
    cut = lambda p, L: tb[p:p + L]
    amb = np.asarray(text[:-1]) == (ord("N") if letters == b"ACGT" else ord("X"))
    nrun = int(np.nonzero(amb[:-1] & amb[1:])[0][0])
    j1 = int(st[1])  # record 1 starts here; the letter before it is the join, the last letter of record 0
    cases = []
    for L in LENGTHS:
        p = 500 + L % 7
        cases.append(("whole %d" % L, cut(p, L), [(0, L, p)]))
        if L >= 17:
            s, ln = L // 3, L // 3
            cases.append(("middle %d" % L, cut(p, L), [(s, ln, p + s)]))
            cases.append(("left extension only %d" % L, substitute(cut(p, L), (2,), letters), [(L - 10, 10, p + L - 10)]))
            cases.append(("right extension only %d" % L, substitute(cut(p, L), (L - 3,), letters), [(0, 10, p)]))
    p = 900
    for t in TAILS:
        cases.append(("tail of %d on the right" % t, cut(p, 80) + rnd(t), [(30, 20, p + 30)]))
        cases.append(("tail of %d on the left" % t, rnd(t) + cut(p, 80), [(t + 30, 20, p + 30)]))
        cases.append(("tails of %d on both" % t, rnd(t) + cut(p, 80) + rnd(t), [(t + 30, 20, p + 30)]))
    cases += [
        ("mismatch at the last letter", substitute(cut(p, 60), (59,), letters), [(0, 20, p)]),
        ("mismatch at the second-last letter", substitute(cut(p, 60), (58,), letters), [(0, 20, p)]),
        ("mismatch at the first letter", substitute(cut(p, 60), (0,), letters), [(40, 20, p + 40)]),
        ("mismatch at the second letter", substitute(cut(p, 60), (1,), letters), [(40, 20, p + 40)]),
    ]
    for h in HANGS:
        cases += [
            ("%d over the start, avail 0" % h, rnd(h) + cut(0, 40), [(h, 40, 0)]),
            ("%d over the start, avail 10" % h, rnd(h) + cut(0, 40), [(h + 10, 30, 10)]),
            ("%d over the end, avail 0" % h, cut(n - 40, 40) + rnd(h), [(0, 40, n - 40)]),
            ("%d over the end, avail 10" % h, cut(n - 40, 40) + rnd(h), [(0, 30, n - 40)]),
            ("%d over the join on the right" % h, cut(j1 - 41, 40) + rnd(h), [(0, 30, j1 - 41)]),
            ("%d over the join on the left" % h, rnd(h) + cut(j1, 40), [(h + 5, 35, j1 + 5)]),
            ("%d over the join on the left, avail 0" % h, rnd(h) + cut(j1, 40), [(h, 40, j1)]),
        ]
    cases.append(("the join symbol under the query's filler", cut(j1 - 30, 29) + filler + cut(j1, 10), [(0, 20, j1 - 30)]))
    p = 1100
    ins = letters[:1]
    for k in (1, 2, 5, 9):  # one letter, and W + 1 letters at every band
        cases += [
            ("%d inserted ten letters into the right extension" % k, cut(p, 30) + ins * k + cut(p + 30, 40), [(0, 20, p)]),
            ("%d deleted ten letters into the right extension" % k, cut(p, 30) + cut(p + 30 + k, 40), [(0, 20, p)]),
            ("%d inserted ten letters into the left extension" % k, cut(p, 40) + ins * k + cut(p + 40, 30), [(50 + k, 20, p + 50)]),
            ("%d deleted ten letters into the left extension" % k, cut(p, 40) + cut(p + 40 + k, 30), [(50, 20, p + 50 + k)]),
        ]
    unit = tb[400:402]
    cases += [
        ("ties in the repeat, both extensions", unit * 15, [(10, 10, 420)]),
        ("ties in the repeat, a letter inserted", unit * 5 + unit[:1] + unit * 10, [(0, 8, 400)]),
        ("ties in the repeat, a unit missing on the left", unit * 12, [(14, 10, 440)]),
        ("ties in the repeat, a junk tail", unit * 10 + rnd(12), [(0, 8, 410)]),
        ("N against N in the right extension", cut(nrun - 30, 60), [(0, 10, nrun - 30)]),
        ("the query's N against other letters", cut(p, 30) + b"NN" + cut(p + 32, 28), [(0, 10, p)]),
    ]
    p = 1300
    for d in SKEWS:
        cases.append(("gap with %d deleted, both ends clipped" % d, rnd(20) + cut(p, 30) + cut(p + 30 + d, 30) + rnd(20), [(20, 20, p), (60, 20, p + 40 + d)]))
        cases.append(("gap with %d inserted, both ends clipped" % d, rnd(20) + cut(p, 30) + ins * d + cut(p + 30, 30) + rnd(20),
                      [(20, 20, p), (60 + d, 20, p + 40)]))
    q60 = cut(p, 60)
    cases += [
        ("unsorted in the query", q60, [(20, 10, p), (10, 5, p + 30)]),
        ("past L", q60, [(0, 20, p), (50, 11, p + 50)]),
        ("t_pos past n", q60, [(0, 20, n + 5)]),
        ("empty", q60, []),
        ("a good chain after the bad ones", rnd(5) + q60 + rnd(5), [(25, 20, p + 20)]),
    ]
    return cases


class Reference:
    """tests/clip_ref.py on the cases, each (case, band, weights) computed once and never changed"""

    def __init__(self, tsym, st, cases, alphabet=0):
        self.tsym, self.st, self.cases, self.memo = tsym, [int(v) for v in st], cases, {}
        self.qsym = [symbols(c[1], alphabet) for c in cases]

    def one(self, i, W, wts):
        key = (i, W, wts)
        if key not in self.memo:
            self.memo[key] = cl.align_chain(self.tsym, self.st, self.qsym[i], list(self.cases[i][2]), W, wts)
        return self.memo[key]

    def many(self, pick, W, wts):
        alns = np.zeros(len(pick), cl.ALN_CLIP_NP)
        nops, runs, ok, cells = np.zeros(len(pick), np.uint64), [np.zeros(0, np.uint32)], 0, 0
        for k, i in enumerate(pick):
            status, tb, te, ed, r, nc, score, c_l, c_r = self.one(i, W, wts)
            alns[k] = (tb, te, ed, status, score, c_l, c_r)
            nops[k] = len(r)
            runs.append(cl.encode(r))
            ok += status == ALN_OK
            cells += nc
        return alns, nops, np.concatenate(runs), (ok, cells)


def device_job(ix, packed, W, wts, nruns, stream=None):
    """upload, pre-fill the outputs with 0xEE; run_job queues count, scan and fill on the stream; job_result downloads"""
    qb, qo, cq, moff, mem = packed
    m = len(cq)
    j = dict(m=m, W=W, wts=wts, s=stream, cap=nruns + 4, d_q=ix.dev_upload(qb), d_qo=ix.dev_upload(qo),
             d_cq=ix.dev_upload(cq if m else np.zeros(1, np.uint32)), d_mo=ix.dev_upload(moff), d_mem=ix.dev_upload(mem.view(np.uint8)),
             d_al=ix.dev_malloc(32 * (m + 2)), d_no=ix.dev_malloc(8 * (m + 2)), d_co=ix.dev_malloc(8 * (m + 1)),
             d_scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(max(m, 1))), d_cg=ix.dev_malloc(4 * (nruns + 4)), d_t=ix.dev_malloc(16))
    ix.dev_memset(j["d_al"], 0xEE, 32 * (m + 2))
    ix.dev_memset(j["d_no"], 0xEE, 8 * (m + 2))
    ix.dev_memset(j["d_cg"], 0xEE, 4 * (nruns + 4))
    ix.dev_memset(j["d_t"], 0, 16)
    return j


def run_job(ix, j):
    args = (j["d_q"], j["d_qo"], j["d_cq"], j["d_mo"], j["d_mem"], j["m"], j["W"]) + tuple(j["wts"])
    ix.dev_align_chains_clip(*args, j["d_al"], j["d_no"], None, None, j["s"], 0, j["d_t"])
    ix.dev_scan_counts(j["d_no"], j["m"], j["d_co"], j["d_scr"], j["s"])
    ix.dev_align_chains_clip(*args, None, None, j["d_co"], j["d_cg"], j["s"])


def job_result(ix, j):
    m = j["m"]
    out = dict(al=ix.dev_download(j["d_al"], (32 * (m + 2),), np.uint8), no=ix.dev_download(j["d_no"], (m + 2,), np.uint64),
               co=ix.dev_download(j["d_co"], (m + 1,), np.uint64), cg=ix.dev_download(j["d_cg"], (j["cap"],), np.uint32),
               t=ix.dev_download(j["d_t"], (2,), np.uint64))
    for key in ("d_q", "d_qo", "d_cq", "d_mo", "d_mem", "d_al", "d_no", "d_co", "d_scr", "d_cg", "d_t"):
        ix.dev_free(j[key])
    return out


def assert_equals_reference(got, want, names=None, what=None):
    alns, nops, runs, tally = want
    m = len(alns)
    g = got["al"][:32 * m].view(ALN_CLIP_DTYPE)
    for f in ALN_CLIP_DTYPE.names:
        bad = np.nonzero(g[f] != alns[f])[0]
        assert not len(bad), (what, f, names[bad[0]] if names else int(bad[0]), g[bad[0]], alns[bad[0]])
    assert np.array_equal(got["no"][:m], nops), what
    assert np.array_equal(got["co"][1:], np.cumsum(nops, dtype=np.uint64)) and got["co"][0] == 0, what
    bad = np.nonzero(got["cg"][:len(runs)] != runs)[0]
    if len(bad):
        c = int(np.searchsorted(got["co"], bad[0], side="right")) - 1
        lo, hi = int(got["co"][c]), int(got["co"][c + 1])
        raise AssertionError((what, names[c] if names else c, cigar_string(got["cg"][lo:hi]), cigar_string(runs[lo:hi])))
    # nothing written past the last record or run
    assert np.all(got["al"][32 * m:] == 0xEE) and np.all(got["no"][m:] == 0xEEEEEEEEEEEEEEEE) and np.all(got["cg"][len(runs):] == 0xEEEEEEEE), what
    assert tuple(int(x) for x in got["t"]) == tuple(int(x) for x in tally), what  # chains aligned, table cells (the count pass)


@pytest.fixture(scope="module")
def small(oracle):
    text, st, hd = small_text()
    w = World(oracle, text, st, hd, 0)
    cases = clip_cases(text, st)
    return w, cases, Reference(symbols(text)[:-1], st, cases)


def test_the_hand_made_chains_hold_what_they_are_for(small):
    w, cases, ref = small
    n = len(w.text) - 1
    j1 = int(w.st[1])
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) <= 255
    by = lambda name, W=4, wts=MAIN: ref.one(names.index(name), W, wts)
    text = lambda name, W=4, wts=MAIN: cl.cigar_text(by(name, W, wts)[4])
    for L in LENGTHS:
        assert text("whole %d" % L) == "%d=" % L and by("whole %d" % L)[6:] == (L, 0, 0)
        if L >= 17:
            assert text("middle %d" % L) == "%d=" % L  # (3) extensions whose letters all match are never clipped
            assert by("left extension only %d" % L)[0] == ALN_OK and by("right extension only %d" % L)[0] == ALN_OK
    for t in TAILS:
        if t >= 16:  # a long random tail is clipped, all but a few letters of it
            assert by("tail of %d on the right" % t)[8] >= t - 4 and by("tail of %d on the left" % t)[7] >= t - 4
            both = by("tails of %d on both" % t)
            assert both[7] >= t - 4 and both[8] >= t - 4 and both[4][0][1] == "S" and both[4][-1][1] == "S"
    # the two sides of the end-bonus decision: H* - H_e = 4 for a mismatch at the last letter
    assert text("mismatch at the last letter", 4, (1, 4, 6, 4)) == "59=1X" and text("mismatch at the last letter", 4, (1, 4, 6, 3)) == "59=1S"
    assert text("mismatch at the first letter", 4, (1, 4, 6, 4)) == "1X59=" and text("mismatch at the first letter", 4, (1, 4, 6, 3)) == "1S59="
    assert text("mismatch at the second-last letter", 4, (1, 4, 6, 3)) == "58=1X1=" and text("mismatch at the second-last letter", 4, (1, 4, 6, 2)) == "58=2S"
    for h in HANGS:
        for W in BANDS:
            a = by("%d over the start, avail 0" % h, W)
            assert (a[0], a[1], a[2], a[7]) == (ALN_OK, 0, 40, h) and cl.cigar_text(a[4]) == "%dS40=" % h
            a = by("%d over the end, avail 0" % h, W)
            assert (a[0], a[1], a[2], a[8]) == (ALN_OK, n - 40, n, h) and cl.cigar_text(a[4]) == "40=%dS" % h
            a = by("%d over the end, avail 10" % h, W)
            assert a[0] == ALN_OK and a[2] <= n
            a = by("%d over the join on the right" % h, W)
            assert a[0] == ALN_OK and a[2] <= j1 and a[8] >= h - 4  # never into the next record
            a = by("%d over the join on the left" % h, W)
            assert a[0] == ALN_OK and a[1] >= j1 and a[7] >= h - 4
            assert by("%d over the join on the left, avail 0" % h, W)[1] == j1
        qsym = ref.qsym[names.index("%d over the end, avail 0" % h)]
        assert (ca.align_chain(ref.tsym, qsym, [(0, 40, n - 40)], 4)[0] == ALN_SKEW) == (h > 16)  # end to end: refused beyond 16
    for W, k in zip(BANDS, (1, 2, 5, 9)):
        for side, field in (("right", 8), ("left", 7)):
            for kind in ("inserted", "deleted"):
                assert by("%d %s ten letters into the %s extension" % (k, kind, side), W)[field] > 20, (W, k, side, kind)  # W + 1 letters: clipped
                if W >= 1:
                    a = by("1 %s ten letters into the %s extension" % (kind, side), W)
                    assert (a[3], a[7], a[8]) == (1, 0, 0) and ("I" if kind == "inserted" else "D") in cl.cigar_text(a[4])
    for d in SKEWS:
        for kind in ("deleted", "inserted"):
            a = by("gap with %d %s, both ends clipped" % (d, kind))
            assert a[0] == (ALN_OK if d <= 16 else ALN_SKEW) and (d > 16 or (a[7] >= 16 and a[8] >= 16))
    for W in BANDS:  # chains on both sides of both class edges, by the gaps' skew alone
        nbs = {d + 2 * W + 1 for d in SKEWS if d <= 16}
        edges = [e for e in (9, 17) if 2 * W + 1 <= e and e + 1 <= 16 + 2 * W + 1]
        assert len(edges) >= 1 and all(e in nbs and e + 1 in nbs for e in edges), (W, sorted(nbs))
    for name in ("unsorted in the query", "past L", "t_pos past n", "empty"):
        assert by(name) == (ALN_BAD_CHAIN, 0, 0, 0, [], 0, 0, 0, 0)
    assert by("a good chain after the bad ones")[0] == ALN_OK and by("N against N in the right extension")[6:] == (60, 0, 0)
    assert by("the join symbol under the query's filler")[2] <= j1


@pytest.mark.parametrize("band", BANDS)
def test_device_primitive_equals_the_reference_at_every_launch_size(small, band):
    w, cases, ref = small
    names = [c[0] for c in cases]
    for k, m in enumerate(LAUNCH_SIZES):
        pick = [x % len(cases) for x in range(m)] if m == 255 else [(5 * x + m) % len(cases) for x in range(m)]  # 255: every case, in order
        for wts in WEIGHTS if m == 255 else (WEIGHTS[k % 4], MAIN):
            want = ref.many(pick, band, wts)
            j = device_job(w.ix, pack_job(cases, pick), band, wts, len(want[2]))
            run_job(w.ix, j)
            w.ix.dev_synchronize()
            assert_equals_reference(job_result(w.ix, j), want, [names[i] for i in pick], (band, m, wts))


def test_two_streams_with_all_launches_queued_before_any_wait(small):
    import torch
    w, cases, ref = small
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    plan = [(list(range(len(cases))), 4, MAIN), (list(range(len(cases)))[::-1] * 3, 8, (2, 3, 4, 0))]
    wants = [ref.many(pick, W, wts) for pick, W, wts in plan]
    jobs = [device_job(w.ix, pack_job(cases, pick), W, wts, len(want[2]), stream=s.cuda_stream) for (pick, W, wts), want, s in zip(plan, wants, streams)]
    w.ix.dev_synchronize()
    for j in jobs:
        run_job(w.ix, j)
    w.ix.dev_synchronize()
    for j, want in zip(jobs, wants):
        assert_equals_reference(job_result(w.ix, j), want)


def test_amino_chains(oracle):
    text, st, hd = small_text(1)
    ix = FmIndex.from_text(text, 1, 8, 0, st, hd).set_devices([0])
    cases = [c for c in clip_cases(text, st, bytes(synth.AA), b"W") if len(c[1]) <= 250 and "N" not in c[0]]
    ref = Reference(symbols(text, 1)[:-1], st, cases, 1)
    pick = list(range(len(cases)))
    want = ref.many(pick, 4, MAIN)
    assert want[3][0] > 80 and int((want[0]["clip_right"] > 0).sum()) > 20 and int((want[0]["clip_left"] > 0).sum()) > 20
    j = device_job(ix, pack_job(cases, pick), 4, MAIN, len(want[2]))
    run_job(ix, j)
    ix.dev_synchronize()
    assert_equals_reference(job_result(ix, j), want, [c[0] for c in cases])
    ix.close()


# ---- the batch entry points ---------------------------------------------------------------------------------------------------------

FAMILY = 50
L_READ = 101


@pytest.fixture(scope="module")
def nt(oracle):
    w = OracleWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)
    w.tsym = symbols(w.text)[:-1]
    w.starts = [int(v) for v in w.st]
    return w


def families(w):
    """-> {family: [(read, strand, origin, extra)]}: about 50 reads of 101 letters per family, every second one reverse-complemented"""
    rng = np.random.default_rng(2026)
    tb = bytes(w.text[:-1])
    n = len(tb)
    st = w.starts + [n]
    rnd = lambda k: bytes(synth.NT[rng.integers(0, 4, size=k)])

    def window(r=None, L=L_READ):  # L letters inside one record, free of N
        while True:
            r_ = int(rng.integers(0, len(st) - 1)) if r is None else r
            p = int(rng.integers(st[r_], st[r_ + 1] - 1 - L))
            if all(c in b"ACGT" for c in tb[p:p + L]):
                return p, r_

    fam = {k: [] for k in ("exact", "subst", "tail", "join", "end", "chimera")}
    for i in range(FAMILY):
        p, _ = window()
        fam["exact"].append((tb[p:p + L_READ], p, None))
        p, _ = window()
        fam["subst"].append((substitute(tb[p:p + L_READ], [int(x) for x in rng.choice(L_READ, size=3, replace=False)]), p, None))
        p, _ = window()
        t = int(rng.integers(16, 52))
        fam["tail"].append((tb[p:p + L_READ - t] + rnd(t), p, t))
        # across the join before record k: the end of record k - 1 and the start of record k, without the delimiter (a join with an N
        # run next to it is passed over)
        for tries in range(1000):
            k = 1 + (i + tries // 50) % (len(st) - 2)
            left = int(rng.integers(25, 77))
            cutp = st[k] - 1 - left
            q = tb[cutp:st[k] - 1] + tb[st[k]:st[k] + L_READ - left]
            if all(c in b"ACGT" for c in q):
                break
        fam["join"].append((q, cutp, k))
        over = int(rng.integers(10, 60))
        fam["end"].append((tb[n - (L_READ - over):] + rnd(over), n - (L_READ - over), over))
        (p1, r1), (p2, r2) = window(L=60), window(L=41)
        while r2 == r1:
            p2, r2 = window(L=41)
        fam["chimera"].append((tb[p1:p1 + 60] + tb[p2:p2 + 41], p1, p2))
    out = {}
    for name, rows in fam.items():
        out[name] = [(mp.rc(q) if i % 2 else q, i % 2, origin, extra) for i, (q, origin, extra) in enumerate(rows)]
        assert all(len(r[0]) == L_READ for r in out[name])
    return out


def random_select_input(n, seed, n_text):
    """alignment records of a doubled batch of n reads: few distinct values per key, so that every key decides somewhere and spans collide"""
    rng = np.random.default_rng(seed)
    counts = rng.choice([0, 0, 1, 1, 2, 3, 5, 8, 10], size=2 * n)
    off = np.zeros(2 * n + 1, np.uint64)
    off[1:] = np.cumsum(counts, dtype=np.uint64)
    tot = int(off[-1])
    alns, chains = np.zeros(max(1, tot), cl.ALN_CLIP_NP), np.zeros(max(1, tot), CHAIN_DTYPE)
    alns["t_begin"][:tot] = rng.choice([100, 150, 200, 5000, n_text - 120], size=tot) + rng.integers(0, 3, size=tot)
    alns["t_end"][:tot] = alns["t_begin"][:tot] + rng.choice([0, 40, 60, 101], size=tot).astype(np.uint64)
    alns["status"][:tot] = np.where(rng.random(tot) < 0.8, 0, rng.choice([ALN_SKEW, ALN_BAD_CHAIN], size=tot))
    alns["edits"][:tot] = rng.integers(0, 4, size=tot)
    alns["score"][:tot] = rng.choice([-3, 0, 29, 30, 31, 60, 86, 101], size=tot)
    alns["clip_left"][:tot], alns["clip_right"][:tot] = rng.choice([0, 0, 7, 41], size=tot), rng.choice([0, 0, 30], size=tot)
    chains["score"][:tot] = rng.choice([30, 60, 101], size=tot)
    status = np.where(rng.random(2 * n) < 0.05, mp.Q_SEED_CAP, 0).astype(np.uint8)
    return off, alns, chains, status


@pytest.mark.parametrize("A", (1, 3, 8))
def test_map_select_clip_equals_the_ranking_function_in_both_passes(nt, A):
    ix = nt.ix
    for n in (1, 257, 3000):
        off, alns, chains, status = random_select_input(n, 7 * n + A, len(nt.text) - 1)
        for R, wts, T in ((1, MAIN, 0), (2 * A, MAIN, 30), (A, (2, 3, 4, 0), 0), (2 * A, (1, 0, 1, 0), 31)):
            woff, wrec, wsel, wst = cl.rank_alignments(off, chains, alns, status, n, A, R, wts, T)
            tot = int(woff[-1])
            d = dict(off=ix.dev_upload(off), al=ix.dev_upload(alns.view(np.uint8)), ch=ix.dev_upload(chains.view(np.uint8)), st=ix.dev_upload(status),
                     nm=ix.dev_malloc(8 * (n + 2)), rs=ix.dev_malloc(n + 8), mo=ix.dev_malloc(8 * (n + 1)),
                     scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(n)), mp=ix.dev_malloc(40 * (tot + 2)), sel=ix.dev_malloc(4 * (tot + 2)),
                     pos=ix.dev_malloc(16 * (tot + 2)))
            for key, size in (("nm", 8 * (n + 2)), ("rs", n + 8), ("mp", 40 * (tot + 2)), ("sel", 4 * (tot + 2)), ("pos", 16 * (tot + 2))):
                ix.dev_memset(d[key], 0xEE, size)
            args = (d["off"], d["al"], d["ch"], d["st"], n, A, R, *wts, T)
            ix.dev_map_select_clip(*args, d["nm"], d["rs"])
            ix.dev_scan_counts(d["nm"], n, d["mo"], d["scr"])
            ix.dev_synchronize()
            mo = ix.dev_download(d["mo"], (n + 1,), np.uint64)
            assert np.array_equal(mo, woff), (A, R, n, wts, T)  # (the fill pass below writes within these offsets)
            ix.dev_map_select_clip(*args, None, None, d["mo"], d["mp"], d["sel"], d["pos"])
            ix.dev_synchronize()
            nm, rs = ix.dev_download(d["nm"], (n + 2,), np.uint64), ix.dev_download(d["rs"], (n + 8,), np.uint8)
            got = ix.dev_download(d["mp"], (40 * (tot + 2),), np.uint8)
            sel, pos = ix.dev_download(d["sel"], (tot + 2,), np.uint32), ix.dev_download(d["pos"], (tot + 2, 2), np.uint64)
            for p in d.values():
                ix.dev_free(p)
            what = (A, R, n, wts, T)
            assert np.array_equal(nm[:n], np.diff(woff)) and np.all(nm[n:] == 0xEEEEEEEEEEEEEEEE) and np.array_equal(rs[:n], wst) and np.all(rs[n:] == 0xEE), what
            g = got[:40 * tot].view(MAP_CLIP_DTYPE)
            for f in MAP_CLIP_DTYPE.names:
                bad = np.nonzero(g[f] != wrec[f])[0]
                assert not len(bad), (what, f, int(bad[0]), g[bad[0]], wrec[bad[0]])
            assert np.array_equal(sel[:tot], np.array(wsel, np.uint32)) and np.array_equal(pos[:tot], positions_of(nt.st, wrec["t_begin"])), what
            assert np.all(got[40 * tot:] == 0xEE) and np.all(sel[tot:] == 0xEEEEEEEE) and np.all(pos[tot:] == 0xEEEEEEEEEEEEEEEE), what
            assert tot > 0 or n == 1
    ix.dev_map_select_clip(None, None, None, None, 0, A, 1, *MAIN, 0, None)


def want_maps(w, reads, A, R, W, wts, T, memo):
    return cl.as_csr(cl.map_reads(w.tsym, w.starts, reads, w.chains_of(P_MAIN), A, R, W, wts, T, memo))


def got_maps(ix, reads, A, R, W, wts, T, **kw):
    return ix.parallel_map_clip_csr(*pack_queries(reads), *KEY, A, R, W, *wts, T, *P_MAIN, **kw)


def assert_maps_equal(got, want, st, what=None):
    off, maps, pos, coff, cg, status = got
    woff, wrec, wcoff, wcg, wst = want
    assert maps.dtype == MAP_CLIP_DTYPE
    assert np.array_equal(off, woff) and np.array_equal(status, wst), what
    for f in MAP_CLIP_DTYPE.names:
        bad = np.nonzero(maps[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), maps[bad[0]], wrec[bad[0]])
    assert np.array_equal(pos, positions_of(st, wrec["t_begin"])), what
    assert np.array_equal(coff, wcoff) and np.array_equal(cg, wcg), what


def composition(ix, reads, A, R, W, wts, T):
    """what needs no reference: awry_align_chains_clip_batch on the doubled batch built on the host, ranked by the pure ranking function"""
    off, ch, al, coff, cg, st = ix.parallel_align_chains_clip_csr(*pack_queries(mp.doubled(reads)), *KEY, A, W, *wts, *P_MAIN)
    assert ch.dtype == CHAIN_DTYPE and al.dtype == ALN_CLIP_DTYPE
    moff, rec, sel, rst = cl.rank_alignments(off, ch, al, st, len(reads), A, R, wts, T)
    runs = [cg[int(coff[c]):int(coff[c + 1])] for c in sel]
    wcoff = np.zeros(len(sel) + 1, np.uint64)
    wcoff[1:] = np.cumsum([len(r) for r in runs], dtype=np.uint64)
    return moff, rec, wcoff, np.concatenate(runs + [np.zeros(0, np.uint32)]).astype(np.uint32), rst


@pytest.fixture(scope="module")
def main(nt):
    fam = families(nt)
    reads = [r[0] for rows in fam.values() for r in rows]
    return fam, reads, {}


def rec_of(starts, t):
    return max(k for k in range(len(starts)) if starts[k] <= t)


def test_the_reference_meets_the_conditions_the_families_are_for(nt, main):
    fam, _, memo = main
    per = {name: cl.map_reads(nt.tsym, nt.starts, [r[0] for r in rows], nt.chains_of(P_MAIN), 3, 2, 4, MAIN, 0, memo) for name, rows in fam.items()}
    for (q, strand, origin, _), (status, recs, runs) in zip(fam["exact"], per["exact"]):  # score a L, no clip, 101=
        assert status == 0 and recs and recs[0][:3] == (origin, origin + L_READ, 0) and recs[0][5] == strand and recs[0][8:] == (L_READ, 0, 0)
        assert cl.cigar_text(runs[0]) == "101="
    clipped = 0
    for (q, strand, origin, t), (_, recs, runs) in zip(fam["tail"], per["tail"]):
        if recs and recs[0][5] == strand:
            # (a reversed read is rc(window + tail): its strand-1 alignment is that of window + tail, the tail at the right end)
            clipped += recs[0][10] >= t - 4 and recs[0][0] == origin
    print("random-tailed reads clipped by at least tail - 4 letters at the window's origin: %d of %d" % (clipped, len(fam["tail"])))
    assert clipped >= 0.95 * len(fam["tail"])
    for (q, strand, origin, k), (_, recs, _) in zip(fam["join"], per["join"]):  # every join-straddling primary lies in one record
        assert recs and recs[0][1] > recs[0][0] and rec_of(nt.starts, recs[0][0]) == rec_of(nt.starts, recs[0][1] - 1)
    two = 0
    for (q, strand, p1, p2), (_, recs, _) in zip(fam["chimera"], per["chimera"]):
        two += len(recs) == 2 and rec_of(nt.starts, recs[0][0]) != rec_of(nt.starts, recs[1][0]) and recs[1][7] == MAP_SECONDARY
    print("chimeras reported as two records in different records at R = 2: %d of %d" % (two, len(fam["chimera"])))
    assert two >= len(fam["chimera"]) // 2
    n = len(nt.tsym)
    for (q, strand, origin, over), (_, recs, _) in zip(fam["end"], per["end"]):
        assert recs and recs[0][1] <= n


@pytest.mark.parametrize("band", (0, 4, 8))
def test_batch_equals_the_reference_and_the_composition(nt, main, band):
    _, reads, memo = main
    for (A, R), wts, T in (((1, 1), MAIN, 0), ((3, 6), MAIN, 0), ((8, 16), MAIN, 30), ((3, 6), (2, 3, 4, 0), 0)):
        want = want_maps(nt, reads, A, R, band, wts, T, memo)
        got = got_maps(nt.ix, reads, A, R, band, wts, T)
        assert_maps_equal(got, want, nt.st, (A, R, band, wts, T))
        assert_maps_equal(got, composition(nt.ix, reads, A, R, band, wts, T), nt.st, ("composition", A, R, band, wts, T))
        assert int(got[0][-1]) > len(reads) // 2


def test_clipping_against_the_end_to_end_mode(nt, main):
    fam, _, memo = main
    rows = fam["tail"]
    reads = [r[0] for r in rows]
    off, maps, _, coff, cg, _ = nt.ix.parallel_map_csr(*pack_queries(reads), *KEY, 3, 1, 4, *P_MAIN)
    off2, maps2, pos2, coff2, cg2, _ = got_maps(nt.ix, reads, 3, 1, 4, MAIN, 0)
    e2e_edits = clipped_at_origin = 0
    for i, (q, strand, origin, t) in enumerate(rows):
        if off[i + 1] > off[i]:
            e2e_edits += int(maps[int(off[i])]["edits"]) > 0
        if off2[i + 1] > off2[i]:
            m = maps2[int(off2[i])]
            c = int(m["clip_right"])  # (a reversed read is rc(window + tail): the tail is at the right end on either strand)
            clipped_at_origin += c >= t - 4 and int(m["strand"]) == strand and int(m["t_begin"]) == origin
            assert cigar_string(cg2[int(coff2[int(off2[i])]):int(coff2[int(off2[i]) + 1])]).endswith("%dS" % c) or c == 0
    assert e2e_edits >= 0.9 * len(rows) and clipped_at_origin >= 0.9 * len(rows), (e2e_edits, clipped_at_origin)


def test_the_list_api_and_the_call_without_the_optional_arrays(nt, main):
    _, reads, memo = main
    sub = reads[2 * FAMILY:2 * FAMILY + 4]
    woff, wrec, wcoff, wcg, _ = want_maps(nt, sub, 3, 6, 4, MAIN, 0, memo)
    pos = positions_of(nt.st, wrec["t_begin"])
    want = [[(int(pos[c][0]), int(pos[c][1]), int(wrec[c]["strand"]), int(wrec[c]["mapq"]), int(wrec[c]["edits"]),
              cigar_string(wcg[int(wcoff[c]):int(wcoff[c + 1])]), int(wrec[c]["flags"]), int(wrec[c]["score"]), int(wrec[c]["clip_left"]),
              int(wrec[c]["clip_right"])) for c in range(int(woff[i]), int(woff[i + 1]))] for i in range(4)]
    assert nt.ix.parallel_map_clip(sub, *KEY, 3, 6, 4, *MAIN, 0, **P_MAIN._asdict()) == want and sum(len(x) for x in want) >= 4
    assert nt.ix.map_clip_string(sub[1], *KEY, 3, 6, 4, *MAIN, 0, **P_MAIN._asdict()) == want[1] and any("S" in r[5] for x in want for r in x)
    lst = nt.ix.parallel_align_chains_clip(sub, *KEY, 2, 4, *MAIN, **P_MAIN._asdict())
    assert len(lst) == 4 and any(a[7] + a[8] > 0 and "S" in a[4] for x in lst for a in x)
    full = got_maps(nt.ix, reads, 3, 6, 4, MAIN, 0)
    bare = got_maps(nt.ix, reads, 3, 6, 4, MAIN, 0, want_pos=False, want_cigar=False)
    assert np.array_equal(bare[0], full[0]) and np.array_equal(bare[1], full[1]) and np.array_equal(bare[5], full[5])
    assert len(bare[2]) == 0 and len(bare[3]) == 0 and len(bare[4]) == 0


@pytest.mark.parametrize("n", (1, 257, 3000))
def test_batch_sizes(nt, main, n):
    _, reads, memo = main
    sub = [reads[(7 * i) % len(reads)] for i in range(n)]
    assert_maps_equal(got_maps(nt.ix, sub, 3, 6, 4, MAIN, 0), want_maps(nt, sub, 3, 6, 4, MAIN, 0, memo), nt.st, n)


def test_results_do_not_depend_on_capacity_sub_batch_replicas_table_accelerators_or_grid(nt, main):
    import awry_amd
    _, reads, memo = main
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]
    want = want_maps(nt, reads, 3, 6, 4, MAIN, 0, memo)
    L_ = awry_amd.load_library()

    def check(ix, name):
        assert_maps_equal(got_maps(ix, reads, 3, 6, 4, MAIN, 0), want, st, name)

    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    for env in ("AWRY_ANCHOR_HIT_CAP=64", "AWRY_CHAIN_ALIGN_SUB_BATCH=7"):
        k, v = env.split("=")
        os.environ[k] = v
        try:
            check(ix, env)
        finally:
            del os.environ[k]
    before = L_.awry_debug_max_blocks()
    L_.awry_debug_set_max_blocks(2)
    try:
        check(ix, "a grid of two blocks")
    finally:
        L_.awry_debug_set_max_blocks(before)
    for name, knob in (("two replicas", lambda: ix.set_devices([0, 0])), ("k0", lambda: ix.set_seed_kmer_len(0)), ("k6", lambda: ix.set_seed_kmer_len(6)),
                       ("verify off", lambda: ix.set_verify(-1)), ("lcx off", lambda: ix.set_lcx(False)), ("dense sa", lambda: ix.set_locate_sa_ratio(1))):
        knob()
        check(ix, name)
    ix.close()
    L_.awry_debug_force_wide_rows(1)
    try:
        wide = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    finally:
        L_.awry_debug_force_wide_rows(0)
    try:
        assert "wide" in wide.count_schedule(31)
        for call in (lambda: got_maps(wide, reads, 3, 6, 4, MAIN, 0), lambda: wide.parallel_align_chains_clip_csr(*pack_queries(reads))):
            with pytest.raises(AwryError) as e:
                call()
            assert e.value.code == ERR_ARG
    finally:
        wide.close()


def test_invalid_reads_fail_the_batch_as_the_siblings_do(nt):
    import awry_amd
    from awry_amd import _lib
    long_q = bytes(nt.text[100:1125])
    assert len(long_q) == 1025 and b"$" not in long_q
    for bad in (long_q, b"AC$T", b""):
        with pytest.raises(AwryError) as e:
            nt.ix.parallel_map_clip_csr(*pack_queries([b"ACGT", b"GGA", bad, b"GGA"]), 1, 50)
        assert e.value.code == ERR_INVALID_QUERY and "query 2:" in str(e.value), bad[:8]
        with pytest.raises(AwryError) as e:
            nt.ix.parallel_align_chains_clip_csr(*pack_queries([b"ACGT", bad, b"GGA"]), 1, 50)
        assert e.value.code == ERR_INVALID_QUERY, bad[:8]
    L = awry_amd.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    off, m, ps, coff, cg, st = u64p(), C.POINTER(_lib.MapClip)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p()
    qb, qo = pack_queries([b"ACGT", long_q])
    rc = L.awry_map_clip_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 1, 50, 100, 16, 100, 10, 1, 4, 1, 4, 1, 4, 6, 5, 0, C.byref(off),
                               C.byref(m), C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st))
    assert rc == ERR_INVALID_QUERY and not off and not m and not ps and not coff and not cg and not st
    t, st_, hd = synth.make_text(3_000, 1, 33, 1, 0.0)
    aa = FmIndex.from_text(t, 1, 8, 0, st_, hd).set_devices([0])
    try:
        with pytest.raises(AwryError) as e:
            aa.parallel_map_clip_csr(*pack_queries([b"ACDEFGHIKLMNPQ"]))
        assert e.value.code == ERR_ARG
    finally:
        aa.close()
    assert nt.ix.map_clip_string(bytes(nt.text[100:1124]), 12, 20)[0][4:] == (0, "1024=", 0, 1024, 0, 0)  # and the index still answers
