"""Mapping read pairs on the GPU (awry_amd/csrc/kernels_pair.hip.h, pair_host.h) against tests/pair_ref.py: awry_dev_pair_windows and
awry_dev_pair_select on the hand-made and on random lists in both passes, and awry_map_pairs_batch end to end -- against the
reference, and with rescue_anchors = 0 against the pair choice applied to the device's own single-end output.  Everything must be
equal: offsets, records, positions, runs, insert, status."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import awry_amd
from awry_amd.fm_index import (ERR_ARG, ERR_INVALID_QUERY, MAP_DTYPE, MAP_MATE_UNMAPPED, MAP_PROPER_PAIR, MAP_RESCUED, PAIR_NO_CHAIN, Q_SEED_CAP, AwryError,
                               FmIndex, cigar_string, pack_queries)
from tests import edit_ref as er
from tests import map_ref as mp
from tests import mismatch_ref as mr
from tests import pair_ref as pr
from tests import synth
from tests.test_chain_align_gpu import KEY
from tests.test_map_gpu import P_MAIN, OracleWorld, positions_of
from tests.test_pair_cpu import FIXTURE, HAND, N_TEXT, PAIR_ARGS, ST, fixture_character, fixture_pairs, hand_made_pairs, interleaved

pytestmark = pytest.mark.gpu

SIZES = (1, 257, 3000)
L_ = awry_amd.load_library()


@contextlib.contextmanager
def max_blocks(b):
    assert L_.awry_debug_set_max_blocks(b) == 0
    try:
        yield
    finally:
        L_.awry_debug_set_max_blocks(0)


@contextlib.contextmanager
def env(name, value):
    os.environ[name] = str(value)
    try:
        yield
    finally:
        del os.environ[name]


# ---- awry_dev_pair_windows, awry_dev_pair_select on lists ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lists_ix():
    """an index whose records are the hand-made lists': [0, 10000), [10000, 20000), [20000, 30000)"""
    rng = np.random.default_rng(9)
    text = np.concatenate([synth.NT[rng.integers(0, 4, size=N_TEXT)], np.frombuffer(b"$", np.uint8)])
    ix = FmIndex.from_text(text, 0, 8, 0, ST, ["r0", "r1", "r2"]).set_devices([0])
    yield ix
    ix.close()


def random_pairs(n, seed, G):
    """per pair (candidates 0, candidates 1, capped 0, capped 1, {(t, a): rescued record or None}, read lengths): few distinct values per
    key, so that every key decides somewhere, spans collide, and pairs are proper, improper on every ground, or alone"""
    rng = np.random.default_rng(seed)
    places = [1000, 1300, 1390, 5000, 9900, 10050, 29800]
    out = []
    for _ in range(n):
        cands = []
        for m in (0, 1):
            lst = []
            for j in range(int(rng.choice([0, 1, 1, 2, 3, 6]))):
                tb = int(rng.choice(places)) + int(rng.integers(0, 3))
                lst.append((int(rng.integers(0, 2)), j, int(rng.integers(0, 4)), int(rng.choice([30, 60, 101])), tb, tb + int(rng.choice([0, 40, 101]))))
            cands.append(lst)
        resc = {}
        for t in (0, 1):
            for a in range(G):
                tb = int(rng.choice(places)) + int(rng.integers(0, 3))
                resc[(t, a)] = None if rng.random() < 0.5 else (tb, tb + int(rng.choice([0, 60, 101])), int(rng.integers(0, 5)), 0, PAIR_NO_CHAIN,
                                                                  int(rng.integers(0, 2)), 0, MAP_RESCUED)
        out.append((cands[0], cands[1], bool(rng.random() < 0.1), bool(rng.random() < 0.1), resc, [int(rng.choice([3, 4, 5, 101, 256, 257, 1024])) for _ in (0, 1)]))
    return out


def with_slots(hand, G):
    """the hand-made pairs at G anchors: their rescued candidates are written for G = 2"""
    return [(c0, c1, bool(cap0), bool(cap1), {(t, a): resc.get((t, a)) for t in (0, 1) for a in range(G)}, [101, 101]) for _, c0, c1, cap0, cap1, resc, _ in hand]


def pair_inputs(pairs, G):
    """-> (cand_off uint64[2P+1], cands MAP_DTYPE, resc MAP_DTYPE[2 G P], read status uint8[2P], qoff uint64[2P+1], kept lists per read)"""
    off, rows, status, qoff, kept = [0], [], [], [0], []
    resc = np.zeros(max(1, 2 * G * len(pairs)), MAP_DTYPE)
    resc.view(np.uint8)[:] = 0xA5  # what lies in a slot without a candidate is not read, apart from edits
    resc["edits"] = 0xFFFFFFFF
    for p, (c0, c1, cap0, cap1, rz, lens) in enumerate(pairs):
        for m, (cands, capped) in enumerate(((c0, cap0), (c1, cap1))):
            K = pr.kept_list(cands, capped)
            kept.append(K)
            rows += K
            off.append(off[-1] + len(K))
            status.append(Q_SEED_CAP if capped else 0)
            qoff.append(qoff[-1] + lens[m])
        for (t, a), z in rz.items():
            if z is not None:
                resc[(2 * p + 1 - t) * G + a] = z
    cands = np.array(rows, MAP_DTYPE) if rows else np.zeros(1, MAP_DTYPE)
    return np.array(off, np.uint64), cands, resc, np.array(status, np.uint8), np.array(qoff, np.uint64), kept


def want_select(pairs, inp, G, mn, mx, U):
    off = inp[0]
    moff, rows, sel, ins = [0], [], [], []
    for p, (c0, c1, cap0, cap1, rz, _) in enumerate(pairs):
        recs, insert, s = pr.rank_pairs(c0, c1, cap0, cap1, rz if G else {}, ST, mn, mx, U)
        for m in (0, 1):
            if recs[m] is not None:
                rows.append(recs[m])
                sel.append(int(off[2 * p + m]) + s[m][1] if s[m][0] == "c" else pr.SEL_RESCUED | ((2 * p + 1 - m) * G + s[m][1]))
            moff.append(len(rows))
        ins.append(insert)
    return np.array(moff, np.uint64), np.array(rows, MAP_DTYPE) if rows else np.zeros(0, MAP_DTYPE), np.array(sel, np.uint32), np.array(ins, np.uint32)


def select_on_device(ix, inp, P, G, mn, mx, U):
    off, cands, resc, status, _, _ = inp
    n = 2 * P
    d = dict(off=ix.dev_upload(off), cd=ix.dev_upload(cands.view(np.uint8)), rs=ix.dev_upload(resc.view(np.uint8)), st=ix.dev_upload(status),
             nm=ix.dev_malloc(8 * (n + 2)), mo=ix.dev_malloc(8 * (n + 1)), scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(max(n, 1))))
    ix.dev_memset(d["nm"], 0xEE, 8 * (n + 2))
    ix.dev_pair_select(d["off"], d["cd"], d["rs"], d["st"], P, mn, mx, U, G, d["nm"])
    ix.dev_scan_counts(d["nm"], n, d["mo"], d["scr"])
    ix.dev_synchronize()
    nm, mo = ix.dev_download(d["nm"], (n + 2,), np.uint64), ix.dev_download(d["mo"], (n + 1,), np.uint64)
    tot = int(mo[-1])
    d.update(mp=ix.dev_malloc(32 * (tot + 2)), sel=ix.dev_malloc(4 * (tot + 2)), pos=ix.dev_malloc(16 * (tot + 2)), ins=ix.dev_malloc(4 * (P + 2)))
    for key, size in (("mp", 32 * (tot + 2)), ("sel", 4 * (tot + 2)), ("pos", 16 * (tot + 2)), ("ins", 4 * (P + 2))):
        ix.dev_memset(d[key], 0xEE, size)
    ix.dev_pair_select(d["off"], d["cd"], d["rs"], d["st"], P, mn, mx, U, G, None, d["mo"], d["mp"], d["sel"], d["pos"], d["ins"])
    ix.dev_synchronize()
    got = dict(nm=nm, mo=mo, mp=ix.dev_download(d["mp"], (32 * (tot + 2),), np.uint8), sel=ix.dev_download(d["sel"], (tot + 2,), np.uint32),
               pos=ix.dev_download(d["pos"], (tot + 2, 2), np.uint64), ins=ix.dev_download(d["ins"], (P + 2,), np.uint32))
    for ptr in d.values():
        ix.dev_free(ptr)
    return got


def assert_select(got, want, P, what):
    woff, wrec, wsel, wins = want
    n, tot = 2 * P, int(woff[-1])
    assert np.array_equal(got["mo"], woff), what
    assert np.array_equal(got["nm"][:n], np.diff(woff)) and np.all(got["nm"][n:] == 0xEEEEEEEEEEEEEEEE), what
    g = got["mp"][:32 * tot].view(MAP_DTYPE)
    for f in MAP_DTYPE.names:
        bad = np.nonzero(g[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), g[bad[0]], wrec[bad[0]])
    assert np.array_equal(got["sel"][:tot], wsel), what
    assert np.array_equal(got["pos"][:tot], positions_of(ST, wrec["t_begin"])), what
    assert np.array_equal(got["ins"][:P], wins), what
    assert np.all(got["mp"][32 * tot:] == 0xEE) and np.all(got["sel"][tot:] == 0xEEEEEEEE) and np.all(got["pos"][tot:] == 0xEEEEEEEEEEEEEEEE), what
    assert np.all(got["ins"][P:] == 0xEEEEEEEE), what


def windows_on_device(ix, inp, P, G, mn, mx, k):
    off, cands, _, _, qoff, _ = inp
    slots = 2 * P * G
    d = dict(off=ix.dev_upload(off), cd=ix.dev_upload(cands.view(np.uint8)), qo=ix.dev_upload(qoff), wq=ix.dev_malloc(4 * (slots + 2)),
             wf=ix.dev_malloc(8 * (slots + 2)), wc=ix.dev_malloc(4 * (slots + 2)))
    for key, size in (("wq", 4), ("wf", 8), ("wc", 4)):
        ix.dev_memset(d[key], 0xEE, size * (slots + 2))
    ix.dev_pair_windows(d["off"], d["cd"], d["qo"], P, mn, mx, G, k, d["wq"], d["wf"], d["wc"])
    ix.dev_synchronize()
    got = (ix.dev_download(d["wq"], (slots + 2,), np.uint32), ix.dev_download(d["wf"], (slots + 2,), np.uint64), ix.dev_download(d["wc"], (slots + 2,), np.uint32))
    for ptr in d.values():
        ix.dev_free(ptr)
    return got


def assert_windows(got, pairs, inp, P, G, mn, mx, k, what):
    kept, slots = inp[5], 2 * P * G
    want = [w for p, pair in enumerate(pairs) for w in pr.windows_of(kept[2 * p], kept[2 * p + 1], pair[5][0], pair[5][1], ST, N_TEXT, mn, mx, G, k, p)]
    wq, wf, wc = got
    assert [(int(a), int(b), int(c)) for a, b, c in zip(wq[:slots], wf[:slots], wc[:slots])] == want, what
    assert np.all(wq[slots:] == 0xEEEEEEEE) and np.all(wf[slots:] == 0xEEEEEEEEEEEEEEEE) and np.all(wc[slots:] == 0xEEEEEEEE), what
    return want


def lists_of(n, G):
    hand = with_slots(hand_made_pairs(), G)
    return (hand * (n // len(hand) + 1))[:n] if n <= len(hand) else hand + random_pairs(n - len(hand), 300 + n + G, G)


@pytest.mark.parametrize("G", (1, 2, 4))
def test_windows_and_pair_choice_equal_the_reference_in_both_passes(lists_ix, G):
    ix, (mn, mx, U) = lists_ix, (HAND["mn"], HAND["mx"], HAND["U"])
    anchors = rescued = improper = 0
    for P in SIZES:
        pairs = lists_of(P, G)
        inp = pair_inputs(pairs, G)
        want = want_select(pairs, inp, G, mn, mx, U)
        assert_select(select_on_device(ix, inp, P, G, mn, mx, U), want, P, (G, P))
        wins = assert_windows(windows_on_device(ix, inp, P, G, mn, mx, 4), pairs, inp, P, G, mn, mx, 4, (G, P))
        anchors += sum(1 for w in wins if w[2])
        rescued += int(np.count_nonzero(want[1]["flags"] & MAP_RESCUED))
        improper += int(np.count_nonzero((want[1]["flags"] & (MAP_PROPER_PAIR | MAP_MATE_UNMAPPED)) == 0))
        if P == 257:  # once with lanes that take several pairs and slots, and at other parameters
            with max_blocks(1):
                assert_select(select_on_device(ix, inp, P, G, mn, mx, U), want, P, (G, P, "one block"))
                assert_windows(windows_on_device(ix, inp, P, G, mn, mx, 4), pairs, inp, P, G, mn, mx, 4, (G, P, "one block"))
            for mn2, mx2, U2, k2 in ((0, 97, 0, 0), (300, 1 << 20, 255, 8)):
                assert_select(select_on_device(ix, inp, P, G, mn2, mx2, U2), want_select(pairs, inp, G, mn2, mx2, U2), P, (G, P, mn2))
                assert_windows(windows_on_device(ix, inp, P, G, mn2, mx2, k2), pairs, inp, P, G, mn2, mx2, k2, (G, P, mn2))
    assert anchors > 100 and rescued > 100 and improper > 100
    # no rescue: d_resc is not read; and no pair at all: nothing is written
    pairs = lists_of(257, 2)
    inp = pair_inputs(pairs, 2)
    got = select_on_device(ix, inp, 257, 0, mn, mx, U)
    assert_select(got, want_select(pairs, inp, 0, mn, mx, U), 257, "G = 0")
    ix.dev_pair_select(None, None, None, None, 0, mn, mx, U, G, None)
    ix.dev_pair_windows(None, None, None, 0, mn, mx, G, 4, None, None, None)
    ix.dev_pair_windows(None, None, None, 5, mn, mx, 0, 4, None, None, None)
    ix.dev_synchronize()


# ---- awry_map_pairs_batch --------------------------------------------------------------------------------------------------------------

def symbols(x):
    return [int(v) for v in mr.to_symbols(bytes(x), 0)]


class PairWorld(OracleWorld):
    def __init__(self, *a):
        super().__init__(*a)
        self.tsym = symbols(self.text)[:-1]
        self.t = er.Text(self.text, 0)

    def want(self, reads, A, W, P, args, memo, key=KEY):
        def chains_of(qs):
            return self.chains_for(key, P)(qs)
        per, ins = pr.map_pairs(self.t, self.tsym, reads, chains_of, A, W, self.st, args["mn"], args["mx"], args["U"], args["G"], args["k"], memo)
        return pr.as_csr(per, ins), per

    def chains_for(self, key, P):
        from tests.test_chain_gpu import want_chains

        def get(qs):
            miss = [q for q in dict.fromkeys(bytes(q) for q in qs) if (q, key, P) not in self._chains]
            if miss:
                for q, c in zip(miss, want_chains(self, miss, *key, P)[0]):
                    self._chains[(q, key, P)] = c
            return [self._chains[(bytes(q), key, P)] for q in qs]
        return get

    def got(self, reads, A, W, P, args, key=KEY, ix=None, **kw):
        return (ix or self.ix).parallel_map_pairs_csr(*pack_queries(reads), *key, A, W, args["mn"], args["mx"], args["U"], args["G"], args["k"], *P, **kw)


def assert_pairs_equal(got, want, st, what=None):
    off, maps, pos, coff, cg, status, ins = got
    woff, wrec, wcoff, wcg, wst, wins = want
    assert maps.dtype == MAP_DTYPE and ins.dtype == np.uint32
    assert np.array_equal(off, woff) and np.array_equal(status, wst), what
    for f in MAP_DTYPE.names:
        bad = np.nonzero(maps[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), maps[bad[0]], wrec[bad[0]])
    assert np.array_equal(pos, positions_of(st, wrec["t_begin"])), what
    assert np.array_equal(coff, wcoff) and np.array_equal(cg, wcg), what
    assert np.array_equal(ins, wins), what


@pytest.fixture(scope="module")
def nt(oracle):
    return PairWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)


@pytest.fixture(scope="module")
def main(nt):
    pairs = fixture_pairs(nt.text, nt.st)
    return interleaved(pairs), pairs, {}


SPECIAL_KEY = (30, 20)  # min_len 30: a 256-letter mate with a substitution every 29th letter seeds nowhere and lies within 8 edits
SPECIAL_ARGS = dict(mn=150, mx=400, U=4, G=2, k=8)


def sparse_subs(q, step):
    q = bytearray(q)
    for at in range(step - 1, len(q), step):
        q[at] = b"ACGT"[(b"ACGT".index(q[at]) + 1) % 4]
    return bytes(q)


def special_world(oracle):
    """two records of random letters, a 101-letter unit R planted twice in the first; -> (world, {name: (mate 0, mate 1)})"""
    rng = np.random.default_rng(515)
    rnd = lambda k: bytes(synth.NT[rng.integers(0, 4, size=k)])
    R = rnd(101)
    rec0 = bytearray(rnd(6000))
    rec0[1250:1351], rec0[4000:4101] = R, R  # the copy at 1250 is proper with a forward mate at 1000, the one at 4000 is not
    rec1 = rnd(3000)
    body = bytes(rec0) + rec1
    T = lambda a, b: body[a:b]
    fr = lambda p, ins: (T(p, p + 101), mp.rc(T(p + ins - 101, p + ins)))  # an exact pair with its forward mate at p and that insert
    a = SPECIAL_ARGS
    absent = rnd(101)
    pairs = {
        "a mate in a two-copy repeat, one copy proper": (T(1000, 1101), mp.rc(R)),
        "both mates on the same strand": (T(2000, 2101), T(2200, 2301)),
        "a pair across a record join": (T(5850, 5951), mp.rc(T(6050, 6151))),
        "a mate that occurs nowhere": (T(2500, 2601), absent),
        "a mate of 257 letters that seeds nowhere": (T(3000, 3101), mp.rc(sparse_subs(T(3100, 3357), 29))),
        "a mate of 1024 letters that seeds nowhere": (sparse_subs(T(6500, 7524), 29), mp.rc(T(7600, 7701))),
        "a mate of 256 letters that seeds nowhere, rescued": (T(4300, 4401), mp.rc(sparse_subs(T(4400, 4656), 29))),
        "a mate of 96 letters that seeds nowhere, rescued by a reverse-strand anchor": (sparse_subs(T(7800, 7896), 11), mp.rc(T(8000, 8101))),
        "insert at min": fr(500, a["mn"]), "insert at max": fr(1500, a["mx"]), "insert at min - 1": fr(3400, a["mn"] - 1), "insert at max + 1": fr(5000, a["mx"] + 1),
    }
    for k in range(len(absent) - 11):
        assert absent[k:k + 12] not in body and mp.rc(absent)[k:k + 12] not in body
    assert body.count(R) == 2
    w = PairWorld(oracle, np.frombuffer(body + b"$", np.uint8).copy(), [0, 6000], ["r0", "r1"], 0)
    return w, pairs


@pytest.fixture(scope="module")
def special(oracle):
    w, pairs = special_world(oracle)
    return w, pairs, [q for p in pairs.values() for q in p], {}


def test_the_special_pairs_hold_what_they_are_for(special):
    w, pairs, reads, memo = special
    _, per = w.want(reads, 3, 4, P_MAIN, SPECIAL_ARGS, memo, SPECIAL_KEY)
    by = {name: (per[2 * i], per[2 * i + 1]) for i, name in enumerate(pairs)}
    U = SPECIAL_ARGS["U"]

    def flags(name):
        return [r[1][0][7] if r[1] else None for r in by[name]]

    (_, r0, _), (_, r1, _) = by["a mate in a two-copy repeat, one copy proper"]
    assert (r0[0][0], r1[0][0], r1[0][5]) == (1000, 1250, 1) and r0[0][6] == r1[0][6] == min(60, 10 * U) and flags("a mate in a two-copy repeat, one copy proper") == [2, 2]
    assert flags("both mates on the same strand") == [0, 0] and flags("a pair across a record join") == [0, 0]
    assert flags("a mate that occurs nowhere") == [MAP_MATE_UNMAPPED, None]
    assert flags("a mate of 257 letters that seeds nowhere") == [MAP_MATE_UNMAPPED, None]
    assert flags("a mate of 1024 letters that seeds nowhere") == [None, MAP_MATE_UNMAPPED]
    assert flags("a mate of 256 letters that seeds nowhere, rescued") == [MAP_PROPER_PAIR, MAP_PROPER_PAIR | MAP_RESCUED]
    assert by["a mate of 256 letters that seeds nowhere, rescued"][1][1][0][:5] == (4400, 4656, 8, 0, PAIR_NO_CHAIN)
    assert flags("a mate of 96 letters that seeds nowhere, rescued by a reverse-strand anchor") == [MAP_PROPER_PAIR | MAP_RESCUED, MAP_PROPER_PAIR]
    assert flags("insert at min") == [2, 2] and flags("insert at max") == [2, 2] and flags("insert at min - 1") == [0, 0] and flags("insert at max + 1") == [0, 0]


@pytest.mark.parametrize("band", (0, 4, 8))
def test_batch_equals_the_reference(nt, main, special, band):
    reads, pairs, memo = main
    for A in (1, 3, 8):
        want, per = nt.want(reads, A, band, P_MAIN, PAIR_ARGS, memo)
        got = nt.got(reads, A, band, P_MAIN, PAIR_ARGS)
        assert_pairs_equal(got, want, nt.st, (A, band))
        assert np.count_nonzero(got[1]["flags"] & MAP_RESCUED) >= FIXTURE["rescued_min"]  # not vacuously: rescued records here, improper pairs below
        if (A, band) == (3, 4):
            per4 = nt.want(reads, 4, 4, P_MAIN, PAIR_ARGS, memo)[1]
            assert fixture_character(pairs, per4) == (FIXTURE["proper"], FIXTURE["rescued"])  # the fixture's character, as the CPU suite records it
    w, _, sreads, smemo = special
    for A in (1, 3, 8):
        want, _ = w.want(sreads, A, band, P_MAIN, SPECIAL_ARGS, smemo, SPECIAL_KEY)
        got = w.got(sreads, A, band, P_MAIN, SPECIAL_ARGS, SPECIAL_KEY)
        assert_pairs_equal(got, want, w.st, ("special", A, band))
        flags = got[1]["flags"]
        assert np.count_nonzero(flags & MAP_RESCUED) >= 2 and np.count_nonzero((flags & (MAP_PROPER_PAIR | MAP_MATE_UNMAPPED)) == 0) >= 6


def rank_single_end(ix, reads, A, W, P, args, st):
    """what needs no reference: the pair choice applied to the device's own single-end records at max_report = 2 A"""
    off, maps, _, coff, cg, status = ix.parallel_map_csr(*pack_queries(reads), *KEY, A, 2 * A, W, *P)
    per, inserts = [], []
    for p in range(len(reads) // 2):
        K = [[tuple(int(v) for v in maps[c]) for c in range(int(off[2 * p + m]), int(off[2 * p + m + 1]))] for m in (0, 1)]
        recs, ins, sel = pr.rank_pairs([pr.cand_of(r) for r in K[0]], [pr.cand_of(r) for r in K[1]], status[2 * p] == Q_SEED_CAP, status[2 * p + 1] == Q_SEED_CAP,
                                       {}, st, args["mn"], args["mx"], args["U"])
        for m in (0, 1):
            c = int(off[2 * p + m]) + sel[m][1] if recs[m] is not None else None
            per.append((int(status[2 * p + m]), [] if c is None else [recs[m]], [] if c is None else [cg[int(coff[c]):int(coff[c + 1])]]))
        inserts.append(ins)
    return pr.as_csr(per, inserts)


def test_without_rescue_the_batch_is_the_pair_choice_over_the_single_end_records(nt, main):
    reads, _, _ = main
    args = dict(PAIR_ARGS, G=0)
    for A, W in ((1, 4), (3, 0), (8, 8)):
        got = nt.got(reads, A, W, P_MAIN, args)
        assert_pairs_equal(got, rank_single_end(nt.ix, reads, A, W, P_MAIN, args, nt.st), nt.st, (A, W))
        assert not np.count_nonzero(got[1]["flags"] & MAP_RESCUED) and np.count_nonzero(got[1]["flags"] & MAP_MATE_UNMAPPED) >= 20


def test_the_list_api_and_the_call_without_the_optional_arrays(nt, main):
    reads, _, memo = main
    (woff, wrec, wcoff, wcg, _, wins), _ = nt.want(reads[:16], 3, 4, P_MAIN, PAIR_ARGS, memo)
    pos = positions_of(nt.st, wrec["t_begin"])

    def rec(i):
        if woff[i] == woff[i + 1]:
            return None
        c = int(woff[i])
        return (int(pos[c][0]), int(pos[c][1]), int(wrec[c]["strand"]), int(wrec[c]["mapq"]), int(wrec[c]["edits"]), cigar_string(wcg[int(wcoff[c]):int(wcoff[c + 1])]),
                int(wrec[c]["flags"]))
    want = [(rec(2 * p), rec(2 * p + 1), int(wins[p])) for p in range(8)]
    a = PAIR_ARGS
    got = nt.ix.parallel_map_pairs(reads[0:16:2], reads[1:16:2], *KEY, 3, 4, a["mn"], a["mx"], a["U"], a["G"], a["k"], **P_MAIN._asdict())
    assert got == want and any(x[0] and x[0][6] & MAP_RESCUED or x[1] and x[1][6] & MAP_RESCUED for x in want) and sum(1 for x in want if x[2]) >= 6
    with pytest.raises(ValueError):
        nt.ix.parallel_map_pairs(reads[:3], reads[:2])
    full = nt.got(reads, 3, 4, P_MAIN, PAIR_ARGS)
    bare = nt.got(reads, 3, 4, P_MAIN, PAIR_ARGS, want_pos=False, want_cigar=False)
    assert all(np.array_equal(bare[i], full[i]) for i in (0, 1, 5, 6)) and len(bare[2]) == 0 and len(bare[3]) == 0 and len(bare[4]) == 0
    nopos = nt.got(reads, 3, 4, P_MAIN, PAIR_ARGS, want_pos=False)
    assert np.array_equal(nopos[3], full[3]) and np.array_equal(nopos[4], full[4]) and len(nopos[2]) == 0
    empty = nt.ix.parallel_map_pairs_csr(*pack_queries([]))
    assert np.array_equal(empty[0], [0]) and len(empty[1]) == 0 and len(empty[6]) == 0


def all_equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def test_results_do_not_depend_on_capacity_sub_batch_replicas_table_accelerators_grid_or_window_cut(nt, main):
    reads, _, memo = main
    reads = reads[:2 * 99]  # an odd number of pairs: two replicas would cut inside a pair if they cut per read
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]
    want = nt.got(reads, 3, 4, P_MAIN, PAIR_ARGS)
    assert_pairs_equal(want, nt.want(reads, 3, 4, P_MAIN, PAIR_ARGS, memo)[0], st)

    def check(ix, name):
        assert all_equal(want, nt.got(reads, 3, 4, P_MAIN, PAIR_ARGS, ix=ix)), name

    ix = FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    for name, value in (("AWRY_ANCHOR_HIT_CAP", 64), ("AWRY_CHAIN_ALIGN_SUB_BATCH", 7), ("AWRY_PAIR_SUB_WINDOW", 1 << 20), ("AWRY_PAIR_SUB_WINDOW", 7)):
        with env(name, value):  # 64 hits: the halving fallback, down to single pairs
            check(ix, (name, value))
    with max_blocks(1):
        check(ix, "one block")
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
        with pytest.raises(AwryError) as e:
            nt.got(reads, 3, 4, P_MAIN, PAIR_ARGS, ix=wide)
        assert e.value.code == ERR_ARG
    finally:
        wide.close()


def test_a_single_pair_over_the_hit_capacity_finishes():
    """a 60-letter unit 70 times between random letters: a pair of two copies of it has 140 located hits and more, over a capacity of
    64 -- a chunk of one pair is never refused, so the halving ends"""
    rng = np.random.default_rng(77)
    rnd = lambda k: bytes(synth.NT[rng.integers(0, 4, size=k)])
    unit = rnd(60)
    body = b"".join(unit + rnd(40) for _ in range(70)) + rnd(500)
    ix = FmIndex.from_text(np.frombuffer(body + b"$", np.uint8).copy(), 0, 8, 0, [0], ["r0"]).set_devices([0])
    reads = [body[5000:5101], mp.rc(body[5200:5301]), unit, mp.rc(unit), body[7000:7101], mp.rc(body[7250:7351])]
    qb, qo = pack_queries(reads)
    assert int(ix.parallel_locate_smems_csr(*pack_queries(reads[2:4]), 100, 12)[2][-1]) >= 70
    args = (12, 100, 2, 4, 0, 1000, 4, 2, 4, 2000, 16, 300, 20, 15)
    want = ix.parallel_map_pairs_csr(qb, qo, *args)
    alone = ix.parallel_map_pairs_csr(*pack_queries(reads[2:4]), *args)
    assert int(want[0][-1]) >= 4 and int(alone[0][-1]) == 2
    with env("AWRY_ANCHOR_HIT_CAP", 64):
        assert all_equal(want, ix.parallel_map_pairs_csr(qb, qo, *args))
        assert all_equal(alone, ix.parallel_map_pairs_csr(*pack_queries(reads[2:4]), *args))
    ix.close()


def test_invalid_reads_fail_the_batch_and_name_the_read(nt, main):
    from awry_amd import _lib
    reads, _, _ = main
    long_q = bytes(nt.text[100:1125])
    assert len(long_q) == 1025 and b"$" not in long_q
    for bad in (long_q, b"AC$T", b""):
        for at in (4, 5):  # either mate of the middle pair
            batch = reads[:10]
            batch[at] = bad
            with pytest.raises(AwryError) as e:
                nt.got(batch, 3, 4, P_MAIN, PAIR_ARGS)
            assert e.value.code == ERR_INVALID_QUERY and "query %d:" % at in str(e.value), (bad[:8], at)  # the read's own index in the interleaved batch
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    for bad in (long_q, b"AC$T"):
        off, m, ps, coff, cg, st, ins = u64p(), C.POINTER(_lib.Map)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p(), u32p()
        qb, qo = pack_queries([b"ACGT", b"GGA", bad, b"ACGT"])
        rc = L_.awry_map_pairs_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 4, 1, 50, 100, 16, 100, 10, 1, 4, 4, 0, 1000, 4, 2, 4, C.byref(off),
                                     C.byref(m), C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st), C.byref(ins))
        assert rc == ERR_INVALID_QUERY and not off and not m and not ps and not coff and not cg and not st and not ins
    # and the index still answers: a 1024-letter read and a 101-letter mate downstream of it, no rescue of either
    two = [bytes(nt.text[100:1124]), mp.rc(nt.text[1300:1401])]
    args = dict(PAIR_ARGS, mx=1400)
    got = nt.got(two, 3, 4, P_MAIN, args)
    assert_pairs_equal(got, nt.want(two, 3, 4, P_MAIN, args, {})[0], nt.st)
    assert [(int(r["t_begin"]), int(r["strand"]), int(r["edits"])) for r in got[1]] == [(100, 0, 0), (1300, 1, 0)] and cigar_string(got[4][:1]) == "1024="
