"""Mapping read pairs in the clipped mode on the GPU (the clipped instantiations of awry_amd/csrc/kernels_pair.hip.h, pair_host.h)
against tests/pair_clip_ref.py: awry_dev_pair_windows_clip and awry_dev_pair_select_clip on the hand-made and on random lists with
random clips in both passes, and awry_map_pairs_clip_batch end to end -- against the reference, by replay of every record's runs, with
rescue_anchors = 0 against the pair choice applied to the device's own clipped single-end output, and against the end-to-end mode on
read-through pairs.  Everything must be equal: offsets, records, positions, runs, insert, status."""
import ctypes as C

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (ERR_ARG, ERR_INVALID_QUERY, MAP_CLIP_DTYPE, MAP_MATE_UNMAPPED, MAP_PROPER_PAIR, MAP_RESCUED, PAIR_NO_CHAIN, Q_SEED_CAP, AwryError,
                               FmIndex, cigar_string, pack_queries)
from tests import clip_ref as cr
from tests import map_ref as mp
from tests import pair_clip_ref as pc
from tests import pair_ref as pr
from tests import synth
from tests.test_chain_align_gpu import KEY
from tests.test_map_gpu import P_MAIN, positions_of
from tests.test_pair_clip_cpu import (FIXTURE, HAND, N_TEXT, PAIR_ARGS, ST, T_MAIN, WTS, fixture_character, fixture_pairs, hand_made_pairs, interleaved,
                                      replay_record)
from tests.test_pair_gpu import L_, SIZES, SPECIAL_KEY, PairWorld, all_equal, env, max_blocks, sparse_subs

pytestmark = pytest.mark.gpu

REC = MAP_CLIP_DTYPE.itemsize  # 40


# ---- awry_dev_pair_windows_clip, awry_dev_pair_select_clip on lists -------------------------------------------------------------------

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
    key, so that every key decides somewhere, spans collide, some candidates fall below T_MAIN, and pairs are proper, improper on every
    ground -- by the clips alone among them: clips of 0..60 at places 0..90 apart --, or alone"""
    rng = np.random.default_rng(seed)
    places = [3, 1000, 1300, 1390, 5000, 9900, 10050, 29800]
    clip = lambda: int(rng.choice([0, 0, 1, 9, 10, 49, 50, 60]))
    out = []
    for _ in range(n):
        cands = []
        for m in (0, 1):
            lst = []
            for j in range(int(rng.choice([0, 1, 1, 2, 3, 6]))):
                tb = int(rng.choice(places)) + int(rng.integers(0, 3))
                lst.append((int(rng.integers(0, 2)), j, int(rng.integers(0, 4)), int(rng.choice([30, 60, 101])), tb, tb + int(rng.choice([0, 40, 101])),
                            int(rng.choice([-3, 29, 30, 60, 61, 65, 101])), clip(), clip()))
            cands.append(lst)
        resc = {}
        for t in (0, 1):
            for a in range(G):
                tb = int(rng.choice(places)) + int(rng.integers(0, 3))
                resc[(t, a)] = None if rng.random() < 0.5 else (tb, tb + int(rng.choice([0, 60, 101])), int(rng.integers(0, 5)), 0, PAIR_NO_CHAIN,
                                                                  int(rng.integers(0, 2)), 0, MAP_RESCUED, int(rng.choice([30, 60, 61, 96, 101])), 0, 0)
        out.append((cands[0], cands[1], bool(rng.random() < 0.1), bool(rng.random() < 0.1), resc, [int(rng.choice([3, 4, 5, 101, 256, 257, 1024])) for _ in (0, 1)]))
    return out


def with_slots(hand, G):
    """the hand-made pairs at G anchors: their rescued candidates are written for G = 2"""
    return [(c0, c1, bool(cap0), bool(cap1), {(t, a): resc.get((t, a)) for t in (0, 1) for a in range(G)}, [101, 101]) for _, c0, c1, cap0, cap1, resc, _ in hand]


def pair_inputs(pairs, G, wts=WTS, T=T_MAIN):
    """-> (cand_off uint64[2P+1], cands MAP_CLIP_DTYPE, resc MAP_CLIP_DTYPE[2 G P], read status uint8[2P], qoff uint64[2P+1], kept lists per read)"""
    off, rows, status, qoff, kept = [0], [], [], [0], []
    resc = np.zeros(max(1, 2 * G * len(pairs)), MAP_CLIP_DTYPE)
    resc.view(np.uint8)[:] = 0xA5  # what lies in a slot without a candidate is not read, apart from edits
    resc["edits"] = 0xFFFFFFFF
    for p, (c0, c1, cap0, cap1, rz, lens) in enumerate(pairs):
        for m, (cands, capped) in enumerate(((c0, cap0), (c1, cap1))):
            K = pc.kept_list(cands, capped, wts, T)
            kept.append(K)
            rows += K
            off.append(off[-1] + len(K))
            status.append(Q_SEED_CAP if capped else 0)
            qoff.append(qoff[-1] + lens[m])
        for (t, a), z in rz.items():
            if z is not None:
                resc[(2 * p + 1 - t) * G + a] = z
    cands = np.array(rows, MAP_CLIP_DTYPE) if rows else np.zeros(1, MAP_CLIP_DTYPE)
    return np.array(off, np.uint64), cands, resc, np.array(status, np.uint8), np.array(qoff, np.uint64), kept


def want_select(pairs, inp, G, mn, mx, U, wts=WTS, T=T_MAIN):
    off = inp[0]
    moff, rows, sel, ins = [0], [], [], []
    for p, (c0, c1, cap0, cap1, rz, _) in enumerate(pairs):
        recs, insert, s = pc.rank_pairs_clip(c0, c1, cap0, cap1, rz if G else {}, ST, mn, mx, U, wts, T)
        for m in (0, 1):
            if recs[m] is not None:
                rows.append(recs[m])
                sel.append(int(off[2 * p + m]) + s[m][1] if s[m][0] == "c" else pr.SEL_RESCUED | ((2 * p + 1 - m) * G + s[m][1]))
            moff.append(len(rows))
        ins.append(insert)
    return np.array(moff, np.uint64), np.array(rows, MAP_CLIP_DTYPE) if rows else np.zeros(0, MAP_CLIP_DTYPE), np.array(sel, np.uint32), np.array(ins, np.uint32)


def select_on_device(ix, inp, P, G, mn, mx, U, wts=WTS, T=T_MAIN):
    off, cands, resc, status, _, _ = inp
    n = 2 * P
    d = dict(off=ix.dev_upload(off), cd=ix.dev_upload(cands.view(np.uint8)), rs=ix.dev_upload(resc.view(np.uint8)), st=ix.dev_upload(status),
             nm=ix.dev_malloc(8 * (n + 2)), mo=ix.dev_malloc(8 * (n + 1)), scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(max(n, 1))))
    ix.dev_memset(d["nm"], 0xEE, 8 * (n + 2))
    ix.dev_pair_select_clip(d["off"], d["cd"], d["rs"], d["st"], P, mn, mx, U, G, *wts, T, d["nm"])
    ix.dev_scan_counts(d["nm"], n, d["mo"], d["scr"])
    ix.dev_synchronize()
    nm, mo = ix.dev_download(d["nm"], (n + 2,), np.uint64), ix.dev_download(d["mo"], (n + 1,), np.uint64)
    tot = int(mo[-1])
    sizes = dict(mp=REC * (tot + 2), sel=4 * (tot + 2), pos=16 * (tot + 2), ins=4 * (P + 2))
    for key, size in sizes.items():
        d[key] = ix.dev_malloc(size)
        ix.dev_memset(d[key], 0xEE, size)
    ix.dev_pair_select_clip(d["off"], d["cd"], d["rs"], d["st"], P, mn, mx, U, G, *wts, T, None, d["mo"], d["mp"], d["sel"], d["pos"], d["ins"])
    ix.dev_synchronize()
    got = dict(nm=nm, mo=mo, mp=ix.dev_download(d["mp"], (REC * (tot + 2),), np.uint8), sel=ix.dev_download(d["sel"], (tot + 2,), np.uint32),
               pos=ix.dev_download(d["pos"], (tot + 2, 2), np.uint64), ins=ix.dev_download(d["ins"], (P + 2,), np.uint32))
    for ptr in d.values():
        ix.dev_free(ptr)
    return got


def assert_select(got, want, P, what):
    woff, wrec, wsel, wins = want
    n, tot = 2 * P, int(woff[-1])
    assert np.array_equal(got["mo"], woff), what
    assert np.array_equal(got["nm"][:n], np.diff(woff)) and np.all(got["nm"][n:] == 0xEEEEEEEEEEEEEEEE), what
    g = got["mp"][:REC * tot].view(MAP_CLIP_DTYPE)
    for f in MAP_CLIP_DTYPE.names:
        bad = np.nonzero(g[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), g[bad[0]], wrec[bad[0]])
    assert np.array_equal(got["sel"][:tot], wsel), what
    assert np.array_equal(got["pos"][:tot], positions_of(ST, wrec["t_begin"])), what
    assert np.array_equal(got["ins"][:P], wins), what
    assert np.all(got["mp"][REC * tot:] == 0xEE) and np.all(got["sel"][tot:] == 0xEEEEEEEE) and np.all(got["pos"][tot:] == 0xEEEEEEEEEEEEEEEE), what
    assert np.all(got["ins"][P:] == 0xEEEEEEEE), what


def windows_on_device(ix, inp, P, G, mn, mx, k):
    off, cands, _, _, qoff, _ = inp
    slots = 2 * P * G
    d = dict(off=ix.dev_upload(off), cd=ix.dev_upload(cands.view(np.uint8)), qo=ix.dev_upload(qoff), wq=ix.dev_malloc(4 * (slots + 2)),
             wf=ix.dev_malloc(8 * (slots + 2)), wc=ix.dev_malloc(4 * (slots + 2)))
    for key, size in (("wq", 4), ("wf", 8), ("wc", 4)):
        ix.dev_memset(d[key], 0xEE, size * (slots + 2))
    ix.dev_pair_windows_clip(d["off"], d["cd"], d["qo"], P, mn, mx, G, k, d["wq"], d["wf"], d["wc"])
    ix.dev_synchronize()
    got = (ix.dev_download(d["wq"], (slots + 2,), np.uint32), ix.dev_download(d["wf"], (slots + 2,), np.uint64), ix.dev_download(d["wc"], (slots + 2,), np.uint32))
    for ptr in d.values():
        ix.dev_free(ptr)
    return got


def assert_windows(got, pairs, inp, P, G, mn, mx, k, what):
    kept, slots = inp[5], 2 * P * G
    want = [w for p, pair in enumerate(pairs) for w in pc.windows_of_clip(kept[2 * p], kept[2 * p + 1], pair[5][0], pair[5][1], ST, N_TEXT, mn, mx, G, k, p)]
    wq, wf, wc = got
    assert [(int(a), int(b), int(c)) for a, b, c in zip(wq[:slots], wf[:slots], wc[:slots])] == want, what
    assert np.all(wq[slots:] == 0xEEEEEEEE) and np.all(wf[slots:] == 0xEEEEEEEEEEEEEEEE) and np.all(wc[slots:] == 0xEEEEEEEE), what
    return want


def lists_of(n, G):
    hand = with_slots(hand_made_pairs(), G)
    return (hand * (n // len(hand) + 1))[:n] if n <= len(hand) else hand + random_pairs(n - len(hand), 700 + n + G, G)


@pytest.mark.parametrize("G", (1, 2, 4))
def test_windows_and_pair_choice_equal_the_reference_in_both_passes(lists_ix, G):
    ix, (mn, mx, U) = lists_ix, (HAND["mn"], HAND["mx"], HAND["U"])
    anchors = rescued = improper = clipped = 0
    for P in SIZES:
        pairs = lists_of(P, G)
        inp = pair_inputs(pairs, G)
        want = want_select(pairs, inp, G, mn, mx, U)
        assert_select(select_on_device(ix, inp, P, G, mn, mx, U), want, P, (G, P))
        wins = assert_windows(windows_on_device(ix, inp, P, G, mn, mx, 4), pairs, inp, P, G, mn, mx, 4, (G, P))
        anchors += sum(1 for w in wins if w[2])
        rescued += int(np.count_nonzero(want[1]["flags"] & MAP_RESCUED))
        improper += int(np.count_nonzero((want[1]["flags"] & (MAP_PROPER_PAIR | MAP_MATE_UNMAPPED)) == 0))
        clipped += int(np.count_nonzero(((want[1]["flags"] & MAP_PROPER_PAIR) != 0) & ((want[1]["clip_left"] != 0) | (want[1]["clip_right"] != 0))))
        if P == 257:  # once with lanes that take several pairs and slots, and at other parameters, weights and thresholds
            with max_blocks(1):
                assert_select(select_on_device(ix, inp, P, G, mn, mx, U), want, P, (G, P, "one block"))
                assert_windows(windows_on_device(ix, inp, P, G, mn, mx, 4), pairs, inp, P, G, mn, mx, 4, (G, P, "one block"))
            for mn2, mx2, U2, k2, wts2, T2 in ((0, 97, 0, 0, (2, 3, 4, 0), 0), (300, 1 << 20, 16384, 8, (16, 64, 64, 1024), 61)):
                inp2 = pair_inputs(pairs, G, wts2, T2)
                assert_select(select_on_device(ix, inp2, P, G, mn2, mx2, U2, wts2, T2), want_select(pairs, inp2, G, mn2, mx2, U2, wts2, T2), P, (G, P, mn2))
                assert_windows(windows_on_device(ix, inp2, P, G, mn2, mx2, k2), pairs, inp2, P, G, mn2, mx2, k2, (G, P, mn2))
    assert anchors > 100 and rescued > 100 and improper > 100 and clipped > 100
    # no rescue: d_resc is not read; and no pair at all: nothing is written
    pairs = lists_of(257, 2)
    inp = pair_inputs(pairs, 2)
    got = select_on_device(ix, inp, 257, 0, mn, mx, U)
    assert_select(got, want_select(pairs, inp, 0, mn, mx, U), 257, "G = 0")
    ix.dev_pair_select_clip(None, None, None, None, 0, mn, mx, U, G, *WTS, T_MAIN, None)
    ix.dev_pair_windows_clip(None, None, None, 0, mn, mx, G, 4, None, None, None)
    ix.dev_pair_windows_clip(None, None, None, 5, mn, mx, 0, 4, None, None, None)
    ix.dev_synchronize()


# ---- awry_map_pairs_clip_batch ---------------------------------------------------------------------------------------------------------

class ClipPairWorld(PairWorld):
    def want_clip(self, reads, A, W, P, args, wts, T, memo, key=KEY):
        per, ins = pc.map_pairs_clip(self.t, self.tsym, reads, self.chains_for(key, P), A, W, self.st, args["mn"], args["mx"], args["U"], args["G"],
                                     args["k"], wts, T, memo)
        return pc.as_csr(per, ins), per

    def got_clip(self, reads, A, W, P, args, wts, T, key=KEY, ix=None, **kw):
        return (ix or self.ix).parallel_map_pairs_clip_csr(*pack_queries(reads), *key, A, W, args["mn"], args["mx"], args["U"], args["G"], args["k"], *wts, T,
                                                           *P, **kw)


def assert_pairs_equal(got, want, st, what=None):
    off, maps, pos, coff, cg, status, ins = got
    woff, wrec, wcoff, wcg, wst, wins = want
    assert maps.dtype == MAP_CLIP_DTYPE and ins.dtype == np.uint32
    assert np.array_equal(off, woff) and np.array_equal(status, wst), what
    for f in MAP_CLIP_DTYPE.names:
        bad = np.nonzero(maps[f] != wrec[f])[0]
        assert not len(bad), (what, f, int(bad[0]), maps[bad[0]], wrec[bad[0]])
    assert np.array_equal(pos, positions_of(st, wrec["t_begin"])), what
    assert np.array_equal(coff, wcoff) and np.array_equal(cg, wcg), what
    assert np.array_equal(ins, wins), what


def assert_replays(w, reads, got, args, wts):
    """properties 1 and 3 on what the device returned, without the reference"""
    off, maps, _, coff, cg, _, ins = got
    for i, q in enumerate(reads):
        for c in range(int(off[i]), int(off[i + 1])):
            replay_record(w.tsym, q, tuple(int(v) for v in maps[c]), cg[int(coff[c]):int(coff[c + 1])], wts)
    for p in range(len(reads) // 2):
        recs = [maps[int(off[2 * p + m])] for m in (0, 1) if off[2 * p + m] != off[2 * p + m + 1]]
        proper = len(recs) == 2 and all(int(r["flags"]) & MAP_PROPER_PAIR for r in recs)
        assert (args["mn"] <= int(ins[p]) <= args["mx"]) if proper else ins[p] == 0, p
        if proper:
            f, v = sorted(recs, key=lambda r: int(r["strand"]))
            assert int(ins[p]) == int(v["t_end"]) + int(v["clip_right"]) - (int(f["t_begin"]) - int(f["clip_left"]))


@pytest.fixture(scope="module")
def nt(oracle):
    return ClipPairWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)


@pytest.fixture(scope="module")
def main(nt):
    pairs = fixture_pairs(nt.text, nt.st)
    return interleaved(pairs), pairs, {}


SPECIAL_ARGS = dict(mn=60, mx=400, U=20, G=2, k=8)


def special_world(oracle):
    """two records of random letters, [0, 6000) and [6000, 9000); -> (world, {name: (mate 0, mate 1)}).  Junk letters differ from the
    text that continues the genomic part at every place, so that nothing of them is aligned."""
    rng = np.random.default_rng(616)
    rnd = lambda k: bytes(synth.NT[rng.integers(0, 4, size=k)])
    body = rnd(9000)
    T = lambda a, b: body[a:b]
    other = lambda ch: b"ACGT"[(b"ACGT".index(ch) + 1) % 4:][:1]

    unlike = lambda a, b: bytes(other(bytes([ch]))[0] for ch in T(a, b))  # letters that differ from the text's at every place of [a, b)
    through = (T(500, 560) + unlike(560, 601), mp.rc(unlike(459, 500) + T(500, 560)))
    hang = T(5910, 5990) + other(T(5990, 5991)) + T(5991, 6011)  # 80 letters, a substitution, 9 letters to the record's end and 11 beyond it
    pairs = {
        "a read-through pair with I = 60": through,
        "a mate hanging over a record end": (T(5800, 5901), mp.rc(hang)),
        "a mate with a 30-letter junk head": (unlike(970, 1000) + T(1000, 1071), mp.rc(T(1150, 1251))),
        "a chimeric mate": (T(2000, 2050) + T(5000, 5051), mp.rc(T(2150, 2251))),
        "an unseedable mate of 256 letters, rescued": (T(4300, 4401), mp.rc(sparse_subs(T(4400, 4656), 29))),
        "an unseedable mate with a 20-letter tail, not rescued": (T(7800, 7901), mp.rc(sparse_subs(T(8000, 8081), 29) + unlike(8081, 8101))),
        "an unseedable mate of 257 letters": (T(3000, 3101), mp.rc(sparse_subs(T(3100, 3357), 29))),
    }
    w = ClipPairWorld(oracle, np.frombuffer(body + b"$", np.uint8).copy(), [0, 6000], ["r0", "r1"], 0)
    return w, pairs


@pytest.fixture(scope="module")
def special(oracle):
    w, pairs = special_world(oracle)
    return w, pairs, [q for p in pairs.values() for q in p], {}


def test_the_special_pairs_hold_what_they_are_for(special):
    w, pairs, reads, memo = special
    _, per = w.want_clip(reads, 3, 4, P_MAIN, SPECIAL_ARGS, WTS, T_MAIN, memo, SPECIAL_KEY)
    (_, _, _, _, _, wins), _ = w.want_clip(reads, 3, 4, P_MAIN, SPECIAL_ARGS, WTS, T_MAIN, memo, SPECIAL_KEY)
    names = list(pairs)
    by = {name: (per[2 * i], per[2 * i + 1]) for i, name in enumerate(names)}
    ins = {name: int(wins[i]) for i, name in enumerate(names)}
    rec = lambda name, m: by[name][m][1][0] if by[name][m][1] else None
    flags = lambda name: [rec(name, m)[7] if rec(name, m) else None for m in (0, 1)]
    span = lambda r: (r[0], r[1], r[9], r[10])  # t_begin, t_end, clip_left, clip_right

    name = "a read-through pair with I = 60"
    assert flags(name) == [2, 2] and ins[name] == 60 and span(rec(name, 0)) == (500, 560, 0, 41) and span(rec(name, 1)) == (500, 560, 41, 0)
    # the same with min_insert = 61: both mates still lie at the fragment, the pair is not proper
    (_, _, _, _, _, wins61), per61 = w.want_clip(list(pairs[name]), 3, 4, P_MAIN, dict(SPECIAL_ARGS, mn=61), WTS, T_MAIN, memo, SPECIAL_KEY)
    assert [r[1][0][7] for r in per61] == [0, 0] and int(wins61[0]) == 0 and [span(r[1][0]) for r in per61] == [(500, 560, 0, 41), (500, 560, 41, 0)]
    # end to end the same reads are not proper either way round
    per_e, _ = pr.map_pairs(w.t, w.tsym, list(pairs[name]), w.chains_for(SPECIAL_KEY, P_MAIN), 3, 4, w.st, 60, 400, 20, 2, 8)
    assert not any(r[1] and r[1][0][7] & MAP_PROPER_PAIR for r in per_e)
    name = "a mate hanging over a record end"
    assert flags(name) == [2, 2] and span(rec(name, 1)) == (5910, 6000, 0, 11) and ins[name] == 6011 - 5800
    name = "a mate with a 30-letter junk head"
    assert flags(name) == [2, 2] and span(rec(name, 0)) == (1000, 1071, 30, 0) and ins[name] == 1251 - 970  # the insert counts the head
    name = "a chimeric mate"  # the part beside the mate wins over the part that scores one more
    assert flags(name) == [2, 2] and span(rec(name, 0)) == (2000, 2050, 0, 51) and ins[name] == 251
    name = "an unseedable mate of 256 letters, rescued"
    assert flags(name) == [MAP_PROPER_PAIR, MAP_PROPER_PAIR | MAP_RESCUED] and rec(name, 1)[:5] == (4400, 4656, 8, 0, PAIR_NO_CHAIN) and rec(name, 1)[8:] == (216, 0, 0)
    assert flags("an unseedable mate with a 20-letter tail, not rescued") == [MAP_MATE_UNMAPPED, None]  # the stated limit: the tail exceeds k edits
    assert flags("an unseedable mate of 257 letters") == [MAP_MATE_UNMAPPED, None]


@pytest.mark.parametrize("T", (0, T_MAIN))
@pytest.mark.parametrize("band", (0, 4, 8))
def test_batch_equals_the_reference_and_replays(nt, main, special, band, T):
    reads, pairs, memo = main
    for A in (1, 3, 8):
        want, per = nt.want_clip(reads, A, band, P_MAIN, PAIR_ARGS, WTS, T, memo)
        got = nt.got_clip(reads, A, band, P_MAIN, PAIR_ARGS, WTS, T)
        assert_pairs_equal(got, want, nt.st, (A, band, T))
        assert_replays(nt, reads, got, PAIR_ARGS, WTS)
        assert np.count_nonzero(got[1]["flags"] & MAP_RESCUED) >= FIXTURE["rescued_min"]  # not vacuously
        assert np.count_nonzero((got[1]["flags"] & MAP_PROPER_PAIR != 0) & (got[1]["clip_left"] + got[1]["clip_right"] > 0)) >= 2 * FIXTURE["through_min"]
    w, _, sreads, smemo = special
    for A in (1, 3, 8):
        want, _ = w.want_clip(sreads, A, band, P_MAIN, SPECIAL_ARGS, WTS, T, smemo, SPECIAL_KEY)
        got = w.got_clip(sreads, A, band, P_MAIN, SPECIAL_ARGS, WTS, T, SPECIAL_KEY)
        assert_pairs_equal(got, want, w.st, ("special", A, band, T))
        assert_replays(w, sreads, got, SPECIAL_ARGS, WTS)
    one = sreads[:2]  # the read-through pair at min_insert = 61
    args = dict(SPECIAL_ARGS, mn=61)
    got = w.got_clip(one, 3, band, P_MAIN, args, WTS, T, SPECIAL_KEY)
    assert_pairs_equal(got, w.want_clip(one, 3, band, P_MAIN, args, WTS, T, smemo, SPECIAL_KEY)[0], w.st, ("mn = 61", band, T))
    assert list(got[1]["flags"]) == [0, 0] and list(got[6]) == [0]


def test_the_fixture_keeps_its_character_on_the_device_and_other_weights_agree(nt, main):
    reads, pairs, memo = main
    got = nt.got_clip(reads, 4, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN)
    want, per = nt.want_clip(reads, 4, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN, memo)
    assert_pairs_equal(got, want, nt.st)
    assert fixture_character(pairs, per, [int(x) for x in want[5]]) == (FIXTURE["through_proper"], FIXTURE["others_proper"], FIXTURE["rescued"])
    wts, args = (2, 3, 4, 0), dict(PAIR_ARGS, mn=55, mx=500, U=0, G=1, k=4)  # other weights, penalty 0, a min_insert some fragments miss
    got = nt.got_clip(reads[:120], 3, 4, P_MAIN, args, wts, 40)
    assert_pairs_equal(got, nt.want_clip(reads[:120], 3, 4, P_MAIN, args, wts, 40, {})[0], nt.st, "other weights")
    assert_replays(nt, reads[:120], got, args, wts)


def rank_single_end(ix, reads, A, W, P, args, wts, T, st):
    """what needs no reference: the pair choice applied to the device's own clipped single-end records at max_report = 2 A"""
    off, maps, _, coff, cg, status = ix.parallel_map_clip_csr(*pack_queries(reads), *KEY, A, 2 * A, W, *wts, T, *P)
    per, inserts = [], []
    for p in range(len(reads) // 2):
        K = [[tuple(int(v) for v in maps[c]) for c in range(int(off[2 * p + m]), int(off[2 * p + m + 1]))] for m in (0, 1)]
        recs, ins, sel = pc.rank_pairs_clip([pc.cand_of(r) for r in K[0]], [pc.cand_of(r) for r in K[1]], status[2 * p] == Q_SEED_CAP,
                                            status[2 * p + 1] == Q_SEED_CAP, {}, st, args["mn"], args["mx"], args["U"], wts, T)
        for m in (0, 1):
            c = int(off[2 * p + m]) + sel[m][1] if recs[m] is not None else None
            per.append((int(status[2 * p + m]), [] if c is None else [recs[m]], [] if c is None else [cg[int(coff[c]):int(coff[c + 1])]]))
        inserts.append(ins)
    return pc.as_csr(per, inserts)


def test_without_rescue_the_batch_is_the_pair_choice_over_the_clipped_single_end_records(nt, main):
    reads, _, _ = main
    args = dict(PAIR_ARGS, G=0)
    for A, W in ((1, 4), (3, 0), (8, 8)):
        got = nt.got_clip(reads, A, W, P_MAIN, args, WTS, T_MAIN)
        assert_pairs_equal(got, rank_single_end(nt.ix, reads, A, W, P_MAIN, args, WTS, T_MAIN, nt.st), nt.st, (A, W))
        assert not np.count_nonzero(got[1]["flags"] & MAP_RESCUED) and np.count_nonzero(got[1]["flags"] & MAP_MATE_UNMAPPED) >= 20


def proper_through(pairs, got):
    off, maps = got[0], got[1]
    return sum(1 for p, pair in enumerate(pairs) if pair[4] is not None and
               all(off[2 * p + m] != off[2 * p + m + 1] and int(maps[int(off[2 * p + m])]["flags"]) & MAP_PROPER_PAIR for m in (0, 1)))


def test_the_end_to_end_mode_marks_fewer_read_through_pairs_proper(nt, main):
    reads, pairs, _ = main
    a = PAIR_ARGS
    clip = nt.got_clip(reads, 4, 4, P_MAIN, a, WTS, T_MAIN)
    e2e = nt.ix.parallel_map_pairs_csr(*pack_queries(reads), *KEY, 4, 4, a["mn"], a["mx"], a["U"], a["G"], a["k"], *P_MAIN)
    n_clip, n_e2e = proper_through(pairs, clip), proper_through(pairs, e2e)
    print("read-through pairs marked proper: clipped mode %d, end-to-end mode %d, of %d" % (n_clip, n_e2e, FIXTURE["through"]))
    assert n_e2e < n_clip and n_clip >= FIXTURE["through_min"] and n_e2e <= FIXTURE["e2e_max"]


def test_the_list_api_and_the_call_without_the_optional_arrays(nt, main):
    reads, _, memo = main
    (woff, wrec, wcoff, wcg, _, wins), _ = nt.want_clip(reads[:16], 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN, memo)
    pos = positions_of(nt.st, wrec["t_begin"])

    def rec(i):
        if woff[i] == woff[i + 1]:
            return None
        c = int(woff[i])
        r = wrec[c]
        return (int(pos[c][0]), int(pos[c][1]), int(r["strand"]), int(r["mapq"]), int(r["edits"]), cigar_string(wcg[int(wcoff[c]):int(wcoff[c + 1])]),
                int(r["flags"]), int(r["score"]), int(r["clip_left"]), int(r["clip_right"]))
    want = [(rec(2 * p), rec(2 * p + 1), int(wins[p])) for p in range(8)]
    a = PAIR_ARGS
    got = nt.ix.parallel_map_pairs_clip(reads[0:16:2], reads[1:16:2], *KEY, 3, 4, a["mn"], a["mx"], a["U"], a["G"], a["k"], *WTS, T_MAIN, **P_MAIN._asdict())
    assert got == want and any("S" in x[m][5] for x in want for m in (0, 1) if x[m]) and sum(1 for x in want if x[2]) >= 6
    with pytest.raises(ValueError):
        nt.ix.parallel_map_pairs_clip(reads[:3], reads[:2])
    full = nt.got_clip(reads, 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN)
    bare = nt.got_clip(reads, 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN, want_pos=False, want_cigar=False)
    assert all(np.array_equal(bare[i], full[i]) for i in (0, 1, 5, 6)) and len(bare[2]) == 0 and len(bare[3]) == 0 and len(bare[4]) == 0
    empty = nt.ix.parallel_map_pairs_clip_csr(*pack_queries([]))
    assert np.array_equal(empty[0], [0]) and len(empty[1]) == 0 and empty[1].dtype == MAP_CLIP_DTYPE and len(empty[6]) == 0


def test_results_do_not_depend_on_capacity_sub_batch_replicas_table_accelerators_grid_or_window_cut(nt, main):
    reads, _, memo = main
    reads = reads[:2 * 99]  # an odd number of pairs: two replicas would cut inside a pair if they cut per read
    text, st = nt.text, nt.st
    hd = ["r%d" % i for i in range(len(st))]
    want = nt.got_clip(reads, 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN)
    assert_pairs_equal(want, nt.want_clip(reads, 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN, memo)[0], st)

    def check(ix, name):
        assert all_equal(want, nt.got_clip(reads, 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN, ix=ix)), name

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


def test_an_odd_batch_a_bad_scalar_and_an_invalid_read_fail_as_the_siblings_do(nt, main):
    reads, _, _ = main
    with pytest.raises(AwryError) as e:
        nt.got_clip(reads[:3], 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN)
    assert e.value.code == ERR_ARG
    for wts, args in (((0, 4, 6, 5), PAIR_ARGS), ((1, 65, 6, 5), PAIR_ARGS), ((1, 4, 6, 1025), PAIR_ARGS), (WTS, dict(PAIR_ARGS, U=16385)), (WTS, dict(PAIR_ARGS, k=9))):
        with pytest.raises(AwryError) as e:
            nt.got_clip(reads[:4], 3, 4, P_MAIN, args, wts, T_MAIN)
        assert e.value.code == ERR_ARG, (wts, args)
    long_q = bytes(nt.text[100:1125])
    assert len(long_q) == 1025 and b"$" not in long_q
    for bad in (long_q, b"AC$T", b""):
        for at in (4, 5):  # either mate of the middle pair
            batch = reads[:10]
            batch[at] = bad
            with pytest.raises(AwryError) as e:
                nt.got_clip(batch, 3, 4, P_MAIN, PAIR_ARGS, WTS, T_MAIN)
            assert e.value.code == ERR_INVALID_QUERY and "query %d:" % at in str(e.value), (bad[:8], at)  # the read's own index in the interleaved batch
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    off, m, ps, coff, cg, st, ins = u64p(), C.POINTER(_lib.MapClip)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p(), u32p()
    qb, qo = pack_queries([b"ACGT", b"GGA", b"AC$T", b"ACGT"])
    rc = L_.awry_map_pairs_clip_batch(nt.ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 4, 1, 50, 100, 16, 100, 10, 1, 4, 4, 0, 1000, 20, 2, 4, 1, 4, 6, 5, 0,
                                      C.byref(off), C.byref(m), C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st), C.byref(ins))
    assert rc == ERR_INVALID_QUERY and not off and not m and not ps and not coff and not cg and not st and not ins
    # and the index still answers: a 1024-letter read and a 101-letter mate downstream of it, no rescue of either
    two = [bytes(nt.text[100:1124]), mp.rc(nt.text[1300:1401])]
    args = dict(PAIR_ARGS, mx=1400)
    got = nt.got_clip(two, 3, 4, P_MAIN, args, WTS, T_MAIN)
    assert_pairs_equal(got, nt.want_clip(two, 3, 4, P_MAIN, args, WTS, T_MAIN, {})[0], nt.st)
    assert [(int(r["t_begin"]), int(r["strand"]), int(r["score"])) for r in got[1]] == [(100, 0, 1024), (1300, 1, 101)] and cigar_string(got[4][:1]) == "1024="
