"""Chain alignment on the GPU (awry_amd/csrc/kernels_chain_align.hip.h) against tests/chain_align_ref.py: the device primitive on
hand-made chains -- every length, band and skew at which the kernel takes another path, pieces that overlap or are swallowed, bad
chains between good ones, the text's ends, joins and N runs, every launch size, streams, the census -- and the batch entry point
end to end with the chains of tests/chain_ref.py.  Everything must be equal: records, run counts, offsets, runs."""
import ctypes as C
import os

import numpy as np
import pytest

from awry_amd.fm_index import (ALN_BAD_CHAIN, ALN_DTYPE, ALN_OK, ALN_SKEW, CHAIN_DTYPE, ERR_ARG, ERR_INVALID_QUERY, Q_SEED_CAP, SEED_DTYPE, AwryError,
                               FmIndex, cigar_string, pack_queries)
from tests import chain_align_ref as ca
from tests import chain_ref as cr
from tests import mismatch_ref as mr
from tests import synth
from tests.test_anchors_gpu import nt_queries, planted
from tests.test_chain_gpu import E2E_PARAMS, want_chains
from tests.test_smems_gpu import World, edge_queries

pytestmark = pytest.mark.gpu

BANDS = (0, 1, 4, 8)
LENGTHS = (1, 2, 17, 64, 65, 101, 250, 1024)
# NB = |m| + 2 W + 1 crosses the class edges 9 | 10 and 17 | 18 at |m| = 8 | 9 (W = 0; 17 | 18 is out of reach), 6 | 7 and 14 | 15 (W = 1), 0 | 1
# and 8 | 9 (W = 4), 0 | 1 (W = 8; 9 | 10 is out of reach)
SKEWS = (1, 6, 7, 8, 9, 14, 15, 16, 17)
LAUNCH_SIZES = (0, 1, 255, 256, 257, 3000)
# what tests/chain_align_ref.py gives (computed on the CPU when the test was written): of the 200 planted reads at (min_len, max_hits)
# = (12, 20) and band 4, the primary alignments with status OK, edits <= the planted edit total and |t_begin - origin| <= the indel
# total: 196 of 200 (the condition is 180)
FIXTURE = dict(placed_min=180, placed=196)


@pytest.fixture(scope="module")
def nt(oracle):
    return World(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)


def symbols(x, alphabet=0):
    return [int(v) for v in mr.to_symbols(bytes(x), alphabet)]


# ---- the device primitive on hand-made chains ---------------------------------------------------------------------------------

def substitute(q, at, letters=b"ACGT"):
    q = bytearray(q)
    for i in at:
        if 0 <= i < len(q):
            q[i] = letters[(letters.find(bytes([q[i]])) + 1) % len(letters)]
    return bytes(q)


def hand_made_chains(text, st, letters=b"ACGT", filler=b"A"):
    """-> [(name, query, members)]; the text positions lie in the first record unless the case says otherwise"""
    tb = bytes(text[:-1])
    n = len(tb)
    cut = lambda p, L: tb[p:p + L]
    amb = np.asarray(text[:-1]) == (ord("N") if letters == b"ACGT" else ord("X"))
    nrun = int(np.nonzero(amb[:-1] & amb[1:])[0][0])  # the first run of N (X)
    join = int(st[2]) - 1                             # the delimiter byte between records 1 and 2: the query has another letter there
    jq = cut(join - 29, 29) + filler + cut(join + 1, 30)
    cases = []
    for L in LENGTHS:
        p = 1000 + 3 * L
        cases.append(("whole %d" % L, cut(p, L), [(0, L, p)]))
        s, ln = L // 3, max(1, L // 3)
        cases.append(("middle %d" % L, substitute(cut(p, L), (s - 3, s - 9, s + ln + 2, L - 1)), [(s, ln, p + s)]))
    cases += [
        ("first piece at 0", cut(0, 50), [(0, 20, 0), (30, 20, 30)]),
        ("left flank reaches 0", cut(0, 50), [(10, 20, 10)]),
        ("left flank within a + W of 0", filler * 2 + cut(0, 48), [(12, 20, 10)]),
        ("last piece ends at n", cut(n - 50, 50), [(20, 30, n - 30)]),
        ("right flank reaches n", cut(n - 50, 50), [(20, 20, n - 30)]),
        ("right flank within a + W of n", cut(n - 50, 50) + filler * 2, [(20, 20, n - 30)]),
    ]
    for h in (1, 16, 17):
        cases.append(("%d over the start" % h, filler * h + cut(0, 40), [(h, 40, 0)]))
        cases.append(("%d over the end" % h, cut(n - 40, 40) + filler * h, [(0, 40, n - 40)]))
    p = 3000
    cases += [
        ("gap a = 0", cut(p, 20) + cut(p + 25, 20), [(0, 20, p), (20, 20, p + 25)]),
        ("gap b = 0", cut(p, 20) + letters[:4] + filler + cut(p + 20, 20), [(0, 20, p), (25, 20, p + 20)]),
        ("gap a = b = 0", cut(p, 40), [(0, 20, p), (20, 20, p + 20)]),
        ("gap of substitutions", substitute(cut(p, 60), (25, 30, 31)), [(0, 20, p), (40, 20, p + 40)]),
    ]
    for d in SKEWS:
        cases.append(("gap with %d deleted" % d, cut(p, 30) + cut(p + 30 + d, 30), [(0, 20, p), (40, 20, p + 40 + d)]))
        cases.append(("gap with %d inserted" % d, cut(p, 30) + letters[:1] * d + cut(p + 30, 30), [(0, 20, p), (40 + d, 20, p + 40)]))
    q60 = cut(p, 60)
    cases += [
        ("overlap in the query", q60, [(0, 20, p), (15, 20, p + 25)]),
        ("overlap in the text", q60, [(0, 20, p), (25, 20, p + 15)]),
        ("overlap in both", q60, [(0, 20, p), (15, 20, p + 15)]),
        ("swallowed member", q60, [(0, 30, p), (5, 10, p + 5), (40, 10, p + 40)]),
        ("swallowed member, then a skew", q60, [(0, 30, p), (5, 10, p + 5), (31, 10, p + 51)]),
        ("seeds that are no exact matches", substitute(q60, (3, 4, 44)), [(0, 20, p), (40, 20, p + 40)]),
        ("unsorted in the query", q60, [(20, 10, p), (10, 5, p + 30)]),
        ("unsorted in the text", q60, [(10, 5, p + 30), (20, 10, p)]),
        ("equal q_begin", q60, [(10, 5, p + 10), (10, 5, p + 20)]),
        ("past L", q60, [(0, 20, p), (50, 11, p + 50)]),
        ("past n", q60, [(0, 20, n - 19)]),
        ("t_pos past n", q60, [(0, 20, n + 5)]),
        ("empty", q60, []),
        ("join inside the left extension", jq, [(40, 15, join + 11)]),
        ("join inside the right extension", jq, [(3, 15, join - 26)]),
        ("join inside a gap", jq, [(0, 20, join - 29), (40, 20, join + 11)]),
        ("N run inside the extensions", substitute(cut(nrun - 20, 60), (0, 59)), [(2, 10, nrun - 18)]),
        ("N run inside a gap, the query's N over the text's", cut(nrun - 20, 60), [(0, 15, nrun - 20), (45, 15, nrun + 25)]),
        ("the query's N over other letters", cut(p, 20) + b"NN" + cut(p + 22, 20), [(0, 10, p), (30, 12, p + 30)]),
    ]
    return cases


def pack_job(cases, pick):
    """the chains cases[i] for i in pick, each with a query of its own -> (qbytes, qoff, chain_query, member_off, members)"""
    qb, qo = pack_queries([cases[i][1] for i in range(len(cases))])
    cq = np.array(pick, np.uint32)
    moff = np.zeros(len(pick) + 1, np.uint64)
    moff[1:] = np.cumsum([len(cases[i][2]) for i in pick], dtype=np.uint64)
    mem = np.zeros(max(1, int(moff[-1])), SEED_DTYPE)
    rows = [m for i in pick for m in cases[i][2]]
    if rows:
        a = np.array(rows, np.int64)
        mem["q_begin"], mem["q_len"], mem["t_pos"] = a[:, 0], a[:, 1], a[:, 2]
    return np.concatenate([qb, np.zeros(16, np.uint8)]), qo, cq, moff, mem


class Reference:
    """tests/chain_align_ref.py on the cases, each (case, band) computed once"""

    def __init__(self, tsym, cases, alphabet=0):
        self.tsym, self.cases, self.memo = tsym, cases, {}
        self.qsym = [symbols(c[1], alphabet) for c in cases]

    def one(self, i, W):
        if (i, W) not in self.memo:
            self.memo[(i, W)] = ca.align_chain(self.tsym, self.qsym[i], list(self.cases[i][2]), W)
        return self.memo[(i, W)]

    def many(self, pick, W):
        alns = np.zeros(len(pick), ca.ALN_NP)
        nops, runs, ok, cells = np.zeros(len(pick), np.uint64), [np.zeros(0, np.uint32)], 0, 0
        for k, i in enumerate(pick):
            st, tb, te, ed, r, cl = self.one(i, W)
            alns[k] = (tb, te, ed, st)
            nops[k] = len(r)
            runs.append(ca.encode(r))
            ok += st == ALN_OK
            cells += cl
        return alns, nops, np.concatenate(runs), (ok, cells)


def device_job(ix, packed, W, nruns, stream=None):
    """upload, pre-fill the outputs with 0xEE; run_job queues count, scan and fill on the stream; job_result downloads"""
    qb, qo, cq, moff, mem = packed
    m = len(cq)
    j = dict(m=m, W=W, s=stream, cap=nruns + 4, d_q=ix.dev_upload(qb), d_qo=ix.dev_upload(qo), d_cq=ix.dev_upload(cq if m else np.zeros(1, np.uint32)),
             d_mo=ix.dev_upload(moff), d_mem=ix.dev_upload(mem.view(np.uint8)), d_al=ix.dev_malloc(24 * (m + 2)), d_no=ix.dev_malloc(8 * (m + 2)),
             d_co=ix.dev_malloc(8 * (m + 1)), d_scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(max(m, 1))), d_cg=ix.dev_malloc(4 * (nruns + 4)),
             d_t=ix.dev_malloc(16))
    ix.dev_memset(j["d_al"], 0xEE, 24 * (m + 2))
    ix.dev_memset(j["d_no"], 0xEE, 8 * (m + 2))
    ix.dev_memset(j["d_cg"], 0xEE, 4 * (nruns + 4))
    ix.dev_memset(j["d_t"], 0, 16)
    return j


def run_job(ix, j):
    args = (j["d_q"], j["d_qo"], j["d_cq"], j["d_mo"], j["d_mem"], j["m"], j["W"])
    ix.dev_align_chains_tally(*args, j["d_al"], j["d_no"], j["d_t"], None, None, j["s"])
    ix.dev_scan_counts(j["d_no"], j["m"], j["d_co"], j["d_scr"], j["s"])
    ix.dev_align_chains(*args, None, None, j["d_co"], j["d_cg"], j["s"])


def job_result(ix, j):
    m = j["m"]
    out = dict(al=ix.dev_download(j["d_al"], (24 * (m + 2),), np.uint8), no=ix.dev_download(j["d_no"], (m + 2,), np.uint64),
               co=ix.dev_download(j["d_co"], (m + 1,), np.uint64), cg=ix.dev_download(j["d_cg"], (j["cap"],), np.uint32),
               t=ix.dev_download(j["d_t"], (2,), np.uint64))
    for key in ("d_q", "d_qo", "d_cq", "d_mo", "d_mem", "d_al", "d_no", "d_co", "d_scr", "d_cg", "d_t"):
        ix.dev_free(j[key])
    return out


def assert_equals_reference(got, want, names=None):
    alns, nops, runs, tally = want
    m = len(alns)
    g = got["al"][:24 * m].view(ALN_DTYPE)
    for f in ALN_DTYPE.names:
        bad = np.nonzero(g[f] != alns[f])[0]
        assert not len(bad), (f, names[bad[0]] if names else int(bad[0]), g[bad[0]], alns[bad[0]])
    assert np.array_equal(got["no"][:m], nops)
    assert np.array_equal(got["co"][1:], np.cumsum(nops, dtype=np.uint64)) and got["co"][0] == 0
    bad = np.nonzero(got["cg"][:len(runs)] != runs)[0]
    if len(bad):
        c = int(np.searchsorted(got["co"], bad[0], side="right")) - 1
        lo, hi = int(got["co"][c]), int(got["co"][c + 1])
        raise AssertionError((names[c] if names else c, cigar_string(got["cg"][lo:hi]), cigar_string(runs[lo:hi])))
    # nothing written past the last record or run
    assert np.all(got["al"][24 * m:] == 0xEE) and np.all(got["no"][m:] == 0xEEEEEEEEEEEEEEEE) and np.all(got["cg"][len(runs):] == 0xEEEEEEEE)
    assert tuple(int(x) for x in got["t"]) == tuple(int(x) for x in tally)  # chains aligned, table cells (the count pass)


@pytest.fixture(scope="module")
def hand(nt):
    cases = hand_made_chains(nt.text, nt.st)
    return cases, Reference(symbols(nt.text)[:-1], cases)


def test_the_hand_made_chains_hold_what_they_are_for(nt, hand):
    cases, ref = hand
    n = len(nt.text) - 1
    by = {name: ref.one(i, 4) for i, (name, _, _) in enumerate(cases)}
    text = lambda name: ca.cigar_text(by[name][4])
    for L in LENGTHS:
        assert text("whole %d" % L) == "%d=" % L and by["middle %d" % L][0] == ALN_OK
    assert by["middle 1024"][3] == 4 and by["left flank reaches 0"][1] == 0 and by["right flank reaches n"][2] == n
    assert by["first piece at 0"][1] == 0 and by["last piece ends at n"][2] == n
    for h in (1, 16):
        assert text("%d over the start" % h) == "%dI40=" % h and text("%d over the end" % h) == "40=%dI" % h
    assert by["17 over the start"][:4] == (ALN_SKEW, 0, 40, 0) and by["17 over the end"][:4] == (ALN_SKEW, n - 40, n, 0)
    assert text("gap a = 0") == "20=5D20=" and text("gap b = 0") == "20=5I20=" and text("gap a = b = 0") == "40="
    assert set(c for _, c in by["gap of substitutions"][4]) == {"=", "X"} and by["gap of substitutions"][3] == 3
    for d in SKEWS:
        for kind in ("deleted", "inserted"):
            st, _, _, edits, runs, _ = by["gap with %d %s" % (d, kind)]
            assert (st, edits) == ((ALN_OK, d) if d <= 16 else (ALN_SKEW, 0))
            assert st != ALN_OK or sum(ln for ln, c in runs if c == "DI"[kind == "inserted"]) == d
    for W in BANDS:  # both sides of every class edge
        nbs = {ca.widest_band(n, len(c[1]), c[2], W) for c in cases} - {None}
        edges = [e for e in (9, 17) if 2 * W + 1 <= e and e + 1 <= 16 + 2 * W + 1]
        assert len(edges) >= 1 and all(e in nbs and e + 1 in nbs for e in edges) and max(nbs) == 16 + 2 * W + 1, (W, sorted(nbs))
    for name in ("overlap in the query", "overlap in the text", "overlap in both", "swallowed member"):
        assert by[name][0] == ALN_OK
    assert len(ca.pieces_of(dict((c[0], c[2]) for c in cases)["swallowed member"], 60, n)[1]) == 2
    assert by["swallowed member, then a skew"][:4] == (ALN_SKEW, 3000, 3061, 0)
    assert "X" in text("seeds that are no exact matches") and by["seeds that are no exact matches"][3] == 3
    bad = ("unsorted in the query", "unsorted in the text", "equal q_begin", "past L", "past n", "t_pos past n", "empty")
    names = [c[0] for c in cases]
    for name in bad:
        assert by[name] == (ALN_BAD_CHAIN, 0, 0, 0, [], 0)
    assert by[names[names.index(bad[0]) - 1]][0] == ALN_OK and by[names[names.index(bad[-1]) + 1]][0] == ALN_OK  # between OK neighbours
    for name in ("join inside the left extension", "join inside the right extension", "join inside a gap", "N run inside the extensions"):
        assert by[name][0] == ALN_OK and by[name][3] >= 1, name
    assert text("N run inside a gap, the query's N over the text's") == "60=" and by["the query's N over other letters"][3] == 2


@pytest.mark.parametrize("band", BANDS)
def test_device_primitive_equals_the_reference_at_every_launch_size(nt, hand, band):
    cases, ref = hand
    for m in LAUNCH_SIZES:
        pick = [k % len(cases) for k in range(m)] if m == 255 else [(5 * k + m) % len(cases) for k in range(m)]  # 255: every case, in order
        want = ref.many(pick, band)
        j = device_job(nt.ix, pack_job(cases, pick), band, len(want[2]))
        run_job(nt.ix, j)
        nt.ix.dev_synchronize()
        assert_equals_reference(job_result(nt.ix, j), want, [cases[i][0] for i in pick])
    assert len(cases) <= 255


def test_two_streams_with_all_launches_queued_before_any_wait(nt, hand):
    import torch
    cases, ref = hand
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    plan = [(list(range(len(cases))), 4), (list(range(len(cases)))[::-1] * 3, 8)]
    wants = [ref.many(pick, W) for pick, W in plan]
    jobs = [device_job(nt.ix, pack_job(cases, pick), W, len(want[2]), stream=s.cuda_stream) for (pick, W), want, s in zip(plan, wants, streams)]
    nt.ix.dev_synchronize()
    for j in jobs:
        run_job(nt.ix, j)
    nt.ix.dev_synchronize()
    for j, want in zip(jobs, wants):
        assert_equals_reference(job_result(nt.ix, j), want)


def test_amino_chains(oracle):
    text, st, hd = synth.make_text(6_000, 1, 33, 3, 0.02)
    ix = FmIndex.from_text(text, 1, 8, 0, st, hd).set_devices([0])
    letters = bytes(synth.AA)
    cases = [c for c in hand_made_chains(text, st, letters, b"W") if len(c[1]) <= 250 and "N" not in c[0]]
    ref = Reference(symbols(text, 1)[:-1], cases, 1)
    pick = list(range(len(cases)))
    want = ref.many(pick, 4)
    assert want[3][0] > 30 and int((want[0]["edits"] > 0).sum()) > 10
    j = device_job(ix, pack_job(cases, pick), 4, len(want[2]))
    run_job(ix, j)
    ix.dev_synchronize()
    assert_equals_reference(job_result(ix, j), want, [c[0] for c in cases])
    ix.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def planted_with_edits(text, rng):
    """-> (read, origin, planted edit total, indel total): 101..250 letters of the text with 0..5 substitutions and 0..2 indels of
    1..3 letters"""
    L = int(rng.integers(101, 251))
    p = int(rng.integers(0, len(text) - 1 - L - 8))
    nsub = int(rng.integers(0, 6))
    q = bytearray(planted(text[p:p + L + 2], np.random.default_rng(int(rng.integers(0, 1 << 30))), L, nsub, synth.NT))
    total = 0
    for _ in range(int(rng.integers(0, 3))):
        at, k = int(rng.integers(20, len(q) - 20)), int(rng.integers(1, 4))
        if rng.random() < 0.5:
            del q[at:at + k]
        else:
            q[at:at] = bytes(synth.NT[rng.integers(0, 4, size=k)])
        total += k
    return bytes(q), p, nsub + total, total


def edited_reads(text, n=200, seed=47):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        r = planted_with_edits(text, rng)
        if b"N" not in r[0]:  # (a read across a record join or an N run has no single origin)
            out.append(r)
    return out


KEY = (12, 20)


def want_alignments(tsym, qs, chains_per, max_alignments, W, memo):
    """chains_per: tests/chain_ref.py's (status, chains) per query -> what awry_align_chains_batch returns"""
    off, rows, alns, coff, runs, st = [0], [], [], [0], [np.zeros(0, np.uint32)], []
    for q, (status, chains) in zip(qs, chains_per):
        st.append(status)
        take = chains[:max_alignments]
        for c in take:
            key = (bytes(q), tuple(c[6]), W)
            if key not in memo:
                memo[key] = ca.align_chain(tsym, symbols(q), list(c[6]), W)
            s, tb, te, ed, r, _ = memo[key]
            rows.append(c[:6])
            alns.append((tb, te, ed, s))
            runs.append(ca.encode(r))
            coff.append(coff[-1] + len(r))
        off.append(off[-1] + len(take))
    return (np.array(off, np.uint64), np.array(rows, np.int64).reshape(-1, 6), np.array(alns, ca.ALN_NP), np.array(coff, np.uint64), np.concatenate(runs),
            np.array(st, np.uint8))


def assert_batch_equals(got, want):
    off, ch, al, coff, cg, st = got
    woff, wrows, waln, wcoff, wruns, wst = want
    assert ch.dtype == CHAIN_DTYPE and al.dtype == ALN_DTYPE
    assert np.array_equal(off, woff) and np.array_equal(st, wst)
    assert np.array_equal(cr.got_chain_rows(ch), wrows)
    for f in ALN_DTYPE.names:
        assert np.array_equal(al[f], waln[f]), f
    assert np.array_equal(coff, wcoff) and np.array_equal(cg, wruns)


@pytest.fixture(scope="module")
def e2e(nt):
    reads = edited_reads(nt.text)
    # the SMEM suite's queries, without those longer than AWRY_CHAIN_ALIGN_MAX_LEN (a whole record, a 5000-letter read), and the reads
    qs = [q for q in nt_queries(nt, (6, nt.ix.seed_kmer_len())) + edge_queries(nt) if len(q) <= 1024] + [r[0] for r in reads]
    assert max(len(q) for q in qs) >= 1000
    chains = {key: want_chains(nt, qs, *key, P)[0] for key, P in E2E_PARAMS.items()}
    return qs, reads, chains, symbols(nt.text)[:-1], {}


def test_batch_equals_the_reference_and_the_fixture_has_its_character(nt, e2e):
    qs, reads, chains, tsym, memo = e2e
    qb, qo = pack_queries(qs)
    for key, P in E2E_PARAMS.items():
        for max_alignments, band in ((1, 4), (3, 0), (10 ** 6, 8)) if key == KEY else ((3, 4),):
            want = want_alignments(tsym, qs, chains[key], max_alignments, band, memo)
            got = nt.ix.parallel_align_chains_csr(qb, qo, *key, max_alignments, band, *P)
            assert_batch_equals(got, want)
            assert int(got[0][-1]) > len(qs) // 2
            # the chains array equals awry_chain_batch's records
            coff, ch, _, _, _ = nt.ix.parallel_chains_csr(qb, qo, *key, *P, want_seeds=False)
            first = np.concatenate([np.arange(int(coff[i]), int(coff[i]) + int(got[0][i + 1] - got[0][i])) for i in range(len(qs))]).astype(np.int64)
            assert np.array_equal(got[1], ch[first])
    # the character of the fixture, from the reference: the planted reads are aligned where they come from, within their planted edits
    want = want_alignments(tsym, qs, chains[KEY], 1, 4, memo)
    placed = 0
    for i, (_, origin, edits, indels) in enumerate(reads, len(qs) - len(reads)):
        lo, hi = int(want[0][i]), int(want[0][i + 1])
        if hi > lo:
            a = want[2][lo]
            placed += int(a["status"]) == ALN_OK and int(a["edits"]) <= edits and abs(int(a["t_begin"]) - origin) <= indels
    print("planted reads whose primary alignment is OK, within the planted edits and at the origin: %d of %d" % (placed, len(reads)))
    assert placed >= FIXTURE["placed_min"] and placed == FIXTURE["placed"]
    # the list API, and the call without the CIGAR arrays
    i = len(qs) - 3
    lst = nt.ix.parallel_align_chains(qs[i:i + 2], *KEY, 3, 4, **E2E_PARAMS[KEY]._asdict())
    w3 = want_alignments(tsym, qs[i:i + 2], chains[KEY][i:i + 2], 3, 4, memo)
    assert lst == [[(int(w3[1][c][0]), int(w3[2][c]["t_begin"]), int(w3[2][c]["t_end"]), int(w3[2][c]["edits"]),
                     cigar_string(w3[4][int(w3[3][c]):int(w3[3][c + 1])]), int(w3[2][c]["status"])) for c in range(int(w3[0][k]), int(w3[0][k + 1]))]
                   for k in range(2)]
    assert nt.ix.align_chains_string(qs[i], *KEY, 3, 4, **E2E_PARAMS[KEY]._asdict()) == lst[0]
    noc = nt.ix.parallel_align_chains_csr(qb, qo, *KEY, 1, 4, *E2E_PARAMS[KEY], want_cigar=False)
    assert np.array_equal(noc[2], nt.ix.parallel_align_chains_csr(qb, qo, *KEY, 1, 4, *E2E_PARAMS[KEY])[2]) and len(noc[3]) == 0 and len(noc[4]) == 0


@pytest.mark.parametrize("n", [1, 257, 3000])
def test_batch_sizes(nt, e2e, n):
    qs, _, chains, tsym, memo = e2e
    short = [i for i, q in enumerate(qs) if len(q) <= 260]
    pick = [short[(7 * i) % len(short)] for i in range(n)]
    sub = [qs[i] for i in pick]
    want = want_alignments(tsym, sub, [chains[KEY][i] for i in pick], 3, 4, memo)
    assert_batch_equals(nt.ix.parallel_align_chains_csr(*pack_queries(sub), *KEY, 3, 4, *E2E_PARAMS[KEY]), want)


def test_results_do_not_depend_on_capacity_sub_batch_replicas_table_or_accelerators(nt, e2e):
    import awry_amd
    qs, _, chains, tsym, memo = e2e
    qb, qo = pack_queries(qs)
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]
    want = want_alignments(tsym, qs, chains[KEY], 3, 4, memo)

    def check(ix, name):
        try:
            assert_batch_equals(ix.parallel_align_chains_csr(qb, qo, *KEY, 3, 4, *E2E_PARAMS[KEY]), want)
        except AssertionError as e:
            raise AssertionError(name) from e

    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    for env in ("AWRY_ANCHOR_HIT_CAP=64", "AWRY_CHAIN_ALIGN_SUB_BATCH=7"):
        k, v = env.split("=")
        os.environ[k] = v
        try:
            check(ix, env)
        finally:
            del os.environ[k]
    for name, knob in (("two replicas", lambda: ix.set_devices([0, 0])), ("k0", lambda: ix.set_seed_kmer_len(0)), ("k6", lambda: ix.set_seed_kmer_len(6)),
                       ("verify off", lambda: ix.set_verify(-1)), ("lcx off", lambda: ix.set_lcx(False)), ("dense sa", lambda: ix.set_locate_sa_ratio(1))):
        knob()
        check(ix, name)
    ix.close()
    L_ = awry_amd.load_library()
    L_.awry_debug_force_wide_rows(1)
    try:
        wide = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    finally:
        L_.awry_debug_force_wide_rows(0)
    try:
        assert "wide" in wide.count_schedule(31)
        with pytest.raises(AwryError) as e:
            wide.parallel_align_chains_csr(qb, qo, *KEY, 3, 4, *E2E_PARAMS[KEY])
        assert e.value.code == ERR_ARG
    finally:
        wide.close()


def test_invalid_queries_fail_the_batch_and_a_capped_query_has_no_alignments(nt, e2e):
    import awry_amd
    from awry_amd import _lib
    qs, _, chains, tsym, memo = e2e
    long_q = bytes(nt.text[100:1125])
    assert len(long_q) == 1025 and b"$" not in long_q
    for bad in (long_q, b"AC$T", b""):
        with pytest.raises(AwryError) as e:
            nt.ix.parallel_align_chains_csr(*pack_queries([b"ACGT", bad, b"GGA"]), 1, 50)
        assert e.value.code == ERR_INVALID_QUERY, bad[:8]
    L = awry_amd.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for bad in (long_q, b"AC$T"):
        off, ch, al, coff, cg, st = u64p(), C.POINTER(_lib.Chain)(), C.POINTER(_lib.Aln)(), u64p(), u32p(), u8p()
        qb, qo = pack_queries([b"ACGT", bad])
        rc = L.awry_align_chains_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 1, 50, 100, 16, 100, 10, 1, 1, 4, C.byref(off), C.byref(ch),
                                       C.byref(al), C.byref(coff), C.byref(cg), C.byref(st))
        assert rc == ERR_INVALID_QUERY and not off and not ch and not al and not coff and not cg and not st
    assert nt.ix.align_chains_string(bytes(nt.text[100:1124]), 12, 20)[0][1:] == (100, 1124, 0, "1024=", ALN_OK)  # and the index still answers
    # a query over max_seeds between neighbours: status Q_SEED_CAP and no alignments
    three = [bytes(nt.text[1000:1030]), qs[len(qs) - 3], bytes(nt.text[1100:1130])]
    P = E2E_PARAMS[KEY]._replace(max_seeds=3)
    per = want_chains(nt, three, 1, 50, P)[0]
    assert [s for s, _ in per] == [0, Q_SEED_CAP, 0] and per[0][1] and per[2][1]
    want = want_alignments(tsym, three, per, 2, 4, memo)
    got = nt.ix.parallel_align_chains_csr(*pack_queries(three), 1, 50, 2, 4, *P)
    assert_batch_equals(got, want)
    assert got[5][1] == Q_SEED_CAP and got[0][2] == got[0][1]


# ---- the chunk driver's rarely taken branches, on 64 reads of 101 letters ------------------------------------------------------------

from tests.test_smems_gpu import all_equal, shrunk_cap, small_reads, with_bad_read  # noqa: E402

NO_CHAIN = E2E_PARAMS[KEY]._replace(min_score=10 ** 6)  # above any reachable score


def assert_no_alignments(got, n):
    off, ch, al, coff, cg, st = got
    assert np.array_equal(off, np.zeros(n + 1, np.uint64)) and len(ch) == 0 and len(al) == 0 and np.array_equal(coff, [0]) and len(cg) == 0
    assert st.dtype == np.uint8 and np.array_equal(st, np.zeros(n, np.uint8))


def test_chunks_without_smems_and_without_chains_give_zero_offsets_and_ok_status(nt):
    reads = small_reads(nt)
    qb, qo = pack_queries(reads)
    assert_no_alignments(nt.ix.parallel_align_chains_csr(qb, qo, 102, 20, 3, 4, *E2E_PARAMS[KEY]), len(reads))  # min_len above every read's length
    assert int(nt.ix.parallel_locate_smems_csr(qb, qo, KEY[1], KEY[0])[2][-1]) >= len(reads)  # seeds, and no chain of them
    assert_no_alignments(nt.ix.parallel_align_chains_csr(qb, qo, *KEY, 3, 4, *NO_CHAIN), len(reads))


def test_the_call_without_the_cigar_arrays_agrees_field_for_field(nt):
    qb, qo = pack_queries(small_reads(nt))
    full = nt.ix.parallel_align_chains_csr(qb, qo, *KEY, 3, 4, *E2E_PARAMS[KEY])
    bare = nt.ix.parallel_align_chains_csr(qb, qo, *KEY, 3, 4, *E2E_PARAMS[KEY], want_cigar=False)
    assert int(full[0][-1]) >= 64 and len(full[4]) >= 64
    assert all(np.array_equal(bare[k], full[k]) for k in (0, 1, 2, 5)) and len(bare[3]) == 0 and len(bare[4]) == 0


def test_a_bad_read_is_named_before_the_capacity_test_splits_its_chunk(nt):
    reads = small_reads(nt, 6)
    with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
        for bad in (b"AC$T", b"", bytes([0x41, 0x80])):
            with pytest.raises(AwryError) as e:
                nt.ix.parallel_align_chains_csr(*pack_queries(with_bad_read(reads, bad)), *KEY, 3, 4, *E2E_PARAMS[KEY])
            assert e.value.code == ERR_INVALID_QUERY and "query 3:" in str(e.value), bad


def test_seven_reads_halved_down_to_single_reads_equal_the_uncapped_call(nt):
    qb, qo = pack_queries(small_reads(nt, 7))
    want = nt.ix.parallel_align_chains_csr(qb, qo, *KEY, 3, 4, *E2E_PARAMS[KEY])
    assert int(want[0][-1]) >= 7
    with shrunk_cap("AWRY_ANCHOR_HIT_CAP"):
        assert all_equal(want, nt.ix.parallel_align_chains_csr(qb, qo, *KEY, 3, 4, *E2E_PARAMS[KEY]))
