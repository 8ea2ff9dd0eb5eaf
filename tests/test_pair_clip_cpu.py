"""Mapping read pairs in the clipped mode without a GPU: the pair choice of tests/pair_clip_ref.py on hand-made lists (proper against
improper, every tie, each ground on which a pair is not proper, MAPQ, the single-mate cases, a rescued candidate below the
threshold), the insert bounds where only a clip decides, read-through pairs, the window arithmetic, the end-to-end section on
clip-free lists, the declarations in every binding, the argument errors that need no device, and the character of the fixture pairs
from the reference alone."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib
from awry_amd.fm_index import (BUILD_HOST, ERR_ARG, ERR_NO_DEVICE, MAP_MATE_UNMAPPED, MAP_PROPER_PAIR, MAP_RESCUED, PAIR_MAX_INSERT, PAIR_NO_CHAIN,
                               AwryError, FmIndex, pack_queries)
from tests import clip_ref as cr
from tests import edit_ref as er
from tests import map_ref as mp
from tests import mismatch_ref as mr
from tests import pair_clip_ref as pc
from tests import pair_ref as pr
from tests import synth
from tests.test_chain_align_gpu import KEY
from tests.test_chain_gpu import E2E_PARAMS, want_chains
from tests.test_map_cpu import HostWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_map_pairs_clip_batch", "awry_dev_pair_windows_clip", "awry_dev_pair_select_clip")
WTS, T_MAIN = (1, 4, 6, 5), 30
# The fixture: 200 pairs at (min_len, max_hits) = (12, 20), A = 4, band 4, WTS, T_MAIN and PAIR_ARGS; every fourth one is a read-through
# pair.  The conditions (the *_min / *_max entries) are the issue's; beside them what tests/pair_clip_ref.py and tests/pair_ref.py gave
# on the CPU when the test was written: read-through pairs proper with |insert - F| <= 4 and both mates at the fragment (at least 80 %
# of 50), read-through pairs proper end to end (fewer than half of 50), other pairs proper at their origins (at least 90 % of 150),
# rescued mates (at least 10).
FIXTURE = dict(through=50, through_min=40, through_proper=50, e2e_max=24, e2e_proper=0, others_min=135, others_proper=150, rescued_min=10, rescued=25)
PAIR_ARGS = dict(mn=0, mx=1000, U=20, G=2, k=8)

ST, N_TEXT = [0, 10_000, 20_000], 30_000  # the record starts and text length of the hand-made lists
HAND = dict(mn=100, mx=500, U=20)
NC = PAIR_NO_CHAIN


def c(s, j, e, sc, tb, te, score, cl=0, cr_=0):
    return (s, j, e, sc, tb, te, score, cl, cr_)


def z(s, e, tb, te, score):
    """a rescued record"""
    return (tb, te, e, 0, NC, s, 0, MAP_RESCUED, score, 0, 0)


def hand_made_pairs():
    """-> [(name, candidates of mate 0, of mate 1, capped 0, capped 1, {(t, a): rescued record}, (sel of mate 0's record, of mate 1's,
    proper, MAPQ, insert))] at HAND's parameters, WTS (a + b = 5) and T_MAIN on records [0, 10000), [10000, 20000), [20000, 30000); sel =
    ("c", index in the kept list), ("r", anchor index) or None"""
    x0, xp = c(0, 0, 1, 80, 1000, 1101, 96), c(0, 0, 0, 80, 1000, 1101, 101)
    out = [
        # K_1 = [the one at 1300, the one at 5000]: equal score and edits, the smaller t_begin first
        ("proper beats improper at equal score", [x0], [c(1, 0, 1, 90, 5000, 5101, 96), c(1, 1, 1, 80, 1300, 1401, 96)], 0, 0, {}, (("c", 0), ("c", 0), True, 40, 401)),
        ("improper wins when it is more than U better", [xp], [c(1, 0, 0, 80, 5000, 5101, 101), c(1, 1, 5, 80, 1300, 1401, 76)], 0, 0, {},
         (("c", 0), ("c", 0), False, 10, 0)),
        ("a tie on S goes to the proper pair", [xp], [c(1, 0, 0, 80, 5000, 5101, 101), c(1, 1, 4, 80, 1300, 1401, 81)], 0, 0, {}, (("c", 0), ("c", 1), True, 0, 401)),
        ("a tie between proper pairs: the smaller index of x", [x0, c(0, 1, 1, 80, 1200, 1301, 96)], [c(1, 0, 1, 80, 1390, 1491, 96)], 0, 0, {},
         (("c", 0), ("c", 0), True, 0, 491)),
        ("then the smaller index of y", [x0], [c(1, 0, 1, 80, 1300, 1401, 96), c(1, 1, 1, 80, 1402, 1499, 96)], 0, 0, {}, (("c", 0), ("c", 0), True, 0, 401)),
        ("the score decides, not the edits", [xp], [c(1, 0, 0, 80, 1300, 1360, 60, 0, 41), c(1, 1, 2, 80, 1380, 1481, 91)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 481)),
        ("the same strand is never proper", [xp], [c(0, 0, 0, 80, 1300, 1401, 101)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("different records are never proper", [c(0, 0, 0, 80, 9800, 9901, 101)], [c(1, 0, 0, 80, 10050, 10151, 101)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("f after v is not proper", [c(0, 0, 0, 80, 1300, 1401, 101)], [c(1, 0, 0, 80, 1000, 1101, 101)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("f ending after v is not proper", [c(0, 0, 0, 80, 1000, 1201, 201)], [c(1, 0, 0, 80, 1050, 1151, 101)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("the order is on the aligned spans: f's span after v's though fb is not", [c(0, 0, 0, 80, 1310, 1401, 91, 20, 0)], [c(1, 0, 0, 80, 1300, 1450, 150)], 0, 0,
         {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("mate 0 on the reverse strand", [c(1, 0, 0, 80, 1300, 1401, 101)], [c(0, 0, 0, 80, 1000, 1101, 101)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 401)),
        ("the inner clips play no part", [c(0, 0, 0, 80, 1000, 1060, 60, 0, 41)], [c(1, 0, 0, 80, 1030, 1090, 60, 41, 0)], 0, 0, {}, (("c", 0), ("c", 0), False, 60, 0)),
        ("a rescued candidate dropped against an original, another kept and chosen", [c(0, 0, 2, 80, 1000, 1101, 91)], [c(1, 0, 2, 80, 5000, 5101, 91)], 0, 0,
         {(1, 0): z(1, 0, 5050, 5151, 101), (0, 0): z(0, 3, 4700, 4801, 86)}, (("r", 0), ("c", 0), True, 30, 401)),
        ("a rescued candidate dropped against an earlier rescued one", [c(0, 0, 2, 80, 1000, 1101, 91), c(0, 1, 2, 70, 7000, 7101, 91)], [], 0, 0,
         {(1, 0): z(1, 1, 1300, 1401, 96), (1, 1): z(1, 0, 1350, 1451, 101)}, (("c", 0), ("r", 0), True, 40, 401)),
        ("no rescue hit in any slot", [x0], [], 0, 0, {(1, 0): None, (1, 1): None}, (("c", 0), None, False, 60, 0)),
        ("a proper pair alone has MAPQ 60", [x0], [c(1, 0, 1, 80, 1300, 1401, 96)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 401)),
        ("a capped read has pair MAPQ 0", [x0], [c(1, 0, 1, 80, 1300, 1401, 96)], 1, 0, {}, (("c", 0), ("c", 0), True, 0, 401)),
        ("the mate capped", [x0], [c(1, 0, 1, 80, 1300, 1401, 96)], 0, 1, {}, (("c", 0), ("c", 0), True, 0, 401)),
        ("one list empty: the single-end primary and its MAPQ", [c(0, 1, 3, 80, 7000, 7101, 86), x0], [], 0, 0, {}, (("c", 0), None, False, 20, 0)),
        ("the other list empty, capped", [], [c(1, 0, 1, 80, 1300, 1401, 96)], 0, 1, {}, (None, ("c", 0), False, 0, 0)),
        ("a candidate below T is none: its mate is alone", [x0], [c(1, 0, 9, 80, 1300, 1366, T_MAIN - 1, 0, 35)], 0, 0, {}, (("c", 0), None, False, 60, 0)),
        ("a candidate at T is one", [x0], [c(1, 0, 9, 80, 1300, 1366, T_MAIN, 0, 35)], 0, 0, {}, (("c", 0), ("c", 0), True, 60, 401)),
        ("both lists empty", [], [], 0, 0, {}, (None, None, False, None, 0)),
    ]
    # S1 - S2 = d: 0, a + b - 1, a + b, 6 (a + b) - 1, 6 (a + b); K_1 = [the clean one at 1300, the one with an edit at 1200]
    out += [("S1 - S2 = %d" % d, [xp], [c(1, 0, 0, 80, 1300, 1401, 101), c(1, 1, 1, 70, 1200, 1290, 101 - d)], 0, 0, {}, (("c", 0), ("c", 0), True, q, 401))
            for d, q in ((0, 0), (4, 8), (5, 10), (29, 58), (30, 60))]
    return out


def run_hand(case):
    _, c0, c1, cap0, cap1, resc, _ = case
    return pc.rank_pairs_clip(c0, c1, bool(cap0), bool(cap1), resc, ST, HAND["mn"], HAND["mx"], HAND["U"], WTS, T_MAIN)


def test_pair_choice_on_hand_made_lists():
    cases = hand_made_pairs()
    assert len({case[0] for case in cases}) == len(cases) == 29
    for case in cases:
        name, c0, c1, cap0, cap1, resc, (sel0, sel1, proper, mapq, insert) = case
        recs, ins, sel = run_hand(case)
        assert sel == [sel0, sel1] and ins == insert, (name, recs, ins, sel)
        K = [pc.kept_list(c0, bool(cap0), WTS, T_MAIN), pc.kept_list(c1, bool(cap1), WTS, T_MAIN)]
        for m, (r, s) in enumerate(zip(recs, sel)):
            assert (r is None) == (s is None), name
            if r is None:
                continue
            src = K[m][s[1]] if s[0] == "c" else resc[(m, s[1])]
            assert r[:6] == src[:6] and r[8:] == src[8:] and len(r) == 11, (name, m)
            if sel0 is not None and sel1 is not None:
                assert r[6] == mapq and r[7] == (MAP_PROPER_PAIR if proper else 0) | (MAP_RESCUED if s[0] == "r" else 0), (name, m, r)
            else:  # the single-end primary, exactly as the clipped single-end ranking reports it
                single = cr.rank_candidates([c0, c1][m], bool([cap0, cap1][m]), 1, WTS, T_MAIN)[0][0]
                assert r == single[:7] + (MAP_MATE_UNMAPPED,) + single[8:] and r[6] == mapq, (name, m, r)
        if proper:  # property 3
            assert HAND["mn"] <= ins <= HAND["mx"], name
        # the input order of the lists changes nothing: the rank is a total order
        assert pc.rank_pairs_clip(c0[::-1], c1[::-1], bool(cap0), bool(cap1), resc, ST, HAND["mn"], HAND["mx"], HAND["U"], WTS, T_MAIN) == (recs, ins, sel), name
    # a larger penalty turns the improper winner into the loser; U = 0 makes the order that of the scores alone
    _, c0, c1, *_ = cases[1]
    assert pc.rank_pairs_clip(c0, c1, False, False, {}, ST, 100, 500, 26, WTS, T_MAIN)[2] == [("c", 0), ("c", 1)]
    assert pc.rank_pairs_clip(c0, c1, False, False, {}, ST, 100, 500, 0, WTS, T_MAIN)[0][0][6:8] == (50, 0)
    # the MAPQ divisor is a + b of the weights
    _, c0, c1, *_ = cases[-2]  # S1 - S2 = 29
    assert pc.rank_pairs_clip(c0, c1, False, False, {}, ST, 100, 500, 20, (2, 3, 4, 0), T_MAIN)[0][0][6] == 58
    assert pc.rank_pairs_clip(c0, c1, False, False, {}, ST, 100, 500, 20, (16, 64, 6, 0), T_MAIN)[0][0][6] == 290 // 80


def test_a_rescued_candidate_below_the_threshold_is_dropped():
    enc = cr.encode
    at = lambda runs, T=T_MAIN: pc.rescued_record(1300, sum(n for n, o in runs if o != "I"), sum(n for n, o in runs if o != "="), 1, enc(runs), WTS, T)
    assert pc.score_of_runs(enc([(60, "="), (1, "X"), (40, "=")]), WTS) == 96 and pc.score_of_runs(enc([(5, "="), (2, "I"), (3, "D")]), (2, 3, 4, 0)) == -10
    assert at([(60, "="), (1, "X"), (40, "=")]) == (1300, 1401, 1, 0, NC, 1, 0, MAP_RESCUED, 96, 0, 0)
    assert at([(4, "="), (1, "X")] * 8) is None  # 32 - 32 = 0
    assert at([(34, "="), (1, "X")]) == (1300, 1335, 1, 0, NC, 1, 0, MAP_RESCUED, 30, 0, 0) and at([(33, "="), (1, "X")]) is None  # T and T - 1
    assert at([(10, "="), (2, "I"), (30, "="), (1, "D"), (8, "=")]) == (1300, 1349, 3, 0, NC, 1, 0, MAP_RESCUED, 30, 0, 0)
    assert at([(4, "="), (1, "X")] * 8, 0)[8] == 0 and at([(3, "="), (1, "X")] * 8, 0) is None  # T = 0 still drops what scores below 0
    # the dropped one leaves its slot empty; the next anchor's candidate is chosen
    x = c(0, 0, 0, 80, 1000, 1101, 101)
    resc = {(1, 0): at([(4, "="), (1, "X")] * 8), (1, 1): at([(60, "="), (1, "X"), (40, "=")])}
    recs, ins, sel = pc.rank_pairs_clip([x], [], False, False, resc, ST, 100, 500, 20, WTS, T_MAIN)
    assert sel == [("c", 0), ("r", 1)] and ins == 401 and recs[1][7] == MAP_PROPER_PAIR | MAP_RESCUED and recs[1][8:] == (96, 0, 0)
    assert pc.rank_pairs_clip([x], [], False, False, {(1, 0): resc[(1, 0)]}, ST, 100, 500, 20, WTS, T_MAIN)[2] == [("c", 0), None]


def test_insert_bounds_where_only_a_clip_decides():
    rec = lambda s, tb, te, cl=0, cr_=0: (tb, te, 0, 80, 0, s, 60, 0, te - tb, cl, cr_)
    P = lambda f, v, mn=100, mx=500: pc.proper_clip(f, v, ST, mn, mx)
    # the aligned spans give 90: the forward mate's left clip, or the reverse mate's right clip, moves the insert to min and to min - 1
    assert P(rec(0, 1000, 1060, 10), rec(1, 1030, 1090)) and not P(rec(0, 1000, 1060, 9), rec(1, 1030, 1090)) and not P(rec(0, 1000, 1060), rec(1, 1030, 1090))
    assert P(rec(0, 1000, 1060), rec(1, 1030, 1090, 0, 10)) and not P(rec(0, 1000, 1060), rec(1, 1030, 1090, 0, 9))
    assert P(rec(0, 1000, 1060, 4), rec(1, 1030, 1090, 0, 6)) and pc.insert_of(rec(1, 1030, 1090, 0, 6), rec(0, 1000, 1060, 4)) == 100
    # 451 on the aligned spans: to max and to max + 1
    assert P(rec(0, 1000, 1101, 49), rec(1, 1350, 1451)) and not P(rec(0, 1000, 1101, 50), rec(1, 1350, 1451)) and P(rec(0, 1000, 1101), rec(1, 1350, 1451))
    assert P(rec(0, 1000, 1101), rec(1, 1350, 1451, 0, 49)) and not P(rec(0, 1000, 1101), rec(1, 1350, 1451, 0, 50))
    # symmetric in its arguments; the inner clips move nothing
    assert P(rec(1, 1030, 1090, 0, 10), rec(0, 1000, 1060)) and not P(rec(0, 1000, 1060, 0, 60), rec(1, 1030, 1090, 60, 0))
    # fb below 0 and ve past the text are used only in the difference
    assert pc.fb(rec(0, 5, 60, 40)) == -35 and P(rec(0, 5, 60, 40), rec(1, 10, 65), 100, 100) and pc.ve(rec(1, 29900, 29990, 0, 50)) == 30040
    # a read-through pair: equal aligned spans [s, s + I), L - I letters of adapter clipped right of f and left of v
    L = 101
    for I in (50, 60, 61, 95, 100, 101):
        f, v = rec(0, 2000, 2000 + I, 0, L - I), rec(1, 2000, 2000 + I, L - I, 0)
        assert pc.insert_of(f, v) == I
        for mn in (0, I - 1, I, I + 1, 101):
            assert P(f, v, mn, 500) == (mn <= I), (I, mn)
        # end to end both alignments run through the adapter: the forward record ends after the reverse one and begins after it
        fe, ve_ = (2000, 2000 + L, 0, 80, 0, 0, 60, 0), (2000 + I - L, 2000 + I, 0, 80, 0, 1, 60, 0)
        assert pr.proper(fe, ve_, ST, 0, 500) == (I == L)


def test_windows_of_clip_on_hand_made_lists():
    rec = lambda s, tb, te, cl=0, cr_=0: (tb, te, 0, 80, 0, s, 60, 0, te - tb, cl, cr_)
    W = lambda K0, K1, L0=101, L1=101, mn=100, mx=500, G=2, k=4, p=0: pc.windows_of_clip(K0, K1, L0, L1, ST, N_TEXT, mn, mx, G, k, p)
    none0, none1 = (2, 0, 0), (0, 0, 0)
    # without clips: the end-to-end windows
    assert W([rec(0, 1000, 1101)], []) == [(3, 1000, 404), none0, none1, none1]
    assert W([rec(1, 1300, 1401)], []) == [(2, 901, 400), none0, none1, none1]
    assert W([], [rec(0, 1000, 1101)], p=3) == [(14, 0, 0), (14, 0, 0), (13, 1000, 404), (12, 0, 0)]
    # a left clip of the forward anchor moves hi down with fb; lo never lies before the aligned span
    assert W([rec(0, 1000, 1101, 30)], [])[0] == (3, 1000, 374)
    assert W([rec(0, 1000, 1101, 30)], [], mn=300)[0] == (3, 970 + 300 - 101 - 4, 1373 - 1165 + 1)
    assert W([rec(0, 1000, 1101, 30)], [], mn=136)[0] == (3, 1001, 373) and W([rec(0, 1000, 1101, 30)], [], mn=135)[0] == (3, 1000, 374)
    # a right clip of the reverse anchor moves both ends up with ve, hi no further than t_begin
    assert W([rec(1, 1300, 1401, 0, 20)], [])[0] == (2, 921, 380)
    assert W([rec(1, 1300, 1401, 0, 20)], [], mn=130)[0] == (2, 921, 1291 - 921 + 1) and W([rec(1, 1300, 1401, 5, 0)], [])[0] == (2, 901, 400)
    # fb < 0 near the text start; ve beyond the record's and the text's end
    assert W([rec(0, 5, 60, 40)], [])[0] == (3, 5, 364)
    assert W([rec(1, 9900, 9990, 0, 50)], [])[0] == (2, 9540, 361) and W([rec(1, 29900, 29990, 0, 50)], [])[0] == (2, 29540, 361)
    assert W([rec(1, 200, 301, 0, 30)], [])[0] == (2, 0, 201)
    # record borders
    assert W([rec(0, 9800, 9901, 30)], [])[0] == (3, 9800, 200) and W([rec(1, 10100, 10201, 0, 20)], [])[0] == (2, 10000, 101)
    assert W([rec(0, 29800, 29901, 10)], [])[0] == (3, 29800, 200) and W([rec(0, 9999, 10100, 50)], [])[0] == (3, 9999, 1)
    # the other mate's length at k, k + 1, 256 and 257
    x = rec(0, 1000, 1101, 10)
    assert W([x], [], L1=4)[0] == none0 and W([x], [], L1=5)[0] == (3, 1081, 409)
    assert W([x], [], L1=256)[0] == (3, 1000, 239) and W([x], [], L1=257)[0] == none0
    # windows that are empty
    assert W([x], [], mn=0, mx=50)[0] == (3, 0, 0) and W([rec(1, 1300, 1401, 0, 20)], [], mn=0, mx=50)[0] == (2, 0, 0)
    # a candidate that is proper with one of the mate's only through its clip is no anchor
    K0, K1 = [rec(0, 1000, 1060, 10), rec(0, 7000, 7101)], [rec(1, 1030, 1090)]
    assert W(K0, K1) == [none0, (3, 7000, 404), none1, none1] and W([rec(0, 1000, 1060, 10)], K1) == [none0, none0, none1, none1]
    # G below, at and above the list's length
    K = [rec(0, 1000, 1101, 30), rec(0, 3000, 3101), rec(1, 5300, 5401, 0, 20)]
    for G in (1, 2, 3, 4):
        got = W(K, [], G=G)
        want = [(3, 1000, 374), (3, 3000, 404), (2, 4921, 380), none0][:G]
        assert len(got) == 2 * G and got[:G] == want[:G] and got[G:] == [none1] * G, G
    assert W(K, [], G=0) == []


def test_property_2_clip_free_lists_give_the_end_to_end_section():
    rng = np.random.default_rng(2)
    places = [0, 3, 1000, 1300, 1390, 5000, 9900, 10050, 29800, 29950]
    anchors = propers = 0
    for it in range(500):
        K = []
        for m in (0, 1):
            lst = []
            for j in range(int(rng.choice([0, 1, 1, 2, 3, 6]))):
                tb = int(rng.choice(places)) + int(rng.integers(0, 3))
                te = tb + int(rng.choice([0, 40, 101]))
                lst.append((tb, te, int(rng.integers(0, 4)), 60, j, int(rng.integers(0, 2)), 0, 0, te - tb, 0, 0))
            K.append(lst)
        L0, L1 = (int(rng.choice([3, 4, 5, 101, 256, 257, 1024])) for _ in (0, 1))
        mn, mx = [(100, 500), (0, 97), (300, 1 << 20), (0, 1000)][it % 4]
        G, k = int(rng.integers(0, 5)), int(rng.choice([0, 4, 8]))
        got = pc.windows_of_clip(K[0], K[1], L0, L1, ST, N_TEXT, mn, mx, G, k, it)
        assert got == pr.windows_of([r[:8] for r in K[0]], [r[:8] for r in K[1]], L0, L1, ST, N_TEXT, mn, mx, G, k, it), it
        anchors += sum(1 for w in got if w[2])
        for x in K[0]:
            for y in K[1]:
                assert pc.proper_clip(x, y, ST, mn, mx) == pr.proper(x[:8], y[:8], ST, mn, mx) == pc.proper_clip(y, x, ST, mn, mx), it
                propers += pc.proper_clip(x, y, ST, mn, mx)
                assert pc.insert_of(x, y) == pr.insert_of(x[:8], y[:8])
    assert anchors > 200 and propers > 50


# ---- declarations ---------------------------------------------------------------------------------------------------------------------

def test_header_ctypes_cpp_mirror_and_rust_agree():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_PAIR_CLIP_MAX_UNPAIRED = 16384", "map read pairs, clipped"):
        assert word in header, word
    assert header.index("map read pairs: insert-size pairing") < header.index("---- map read pairs, clipped") < header.index("releases an array one of the calls above")
    assert pc.PAIR_CLIP_MAX_UNPAIRED == 16384 == 1024 * cr.MAX_MATCH
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
    # the clipped batch call is the end-to-end one with the five scalars after rescue_edits, the records in the clipped type
    e2e = re.search(r"\bawry_map_pairs_batch\s*\(([^)]*)\)", src).group(1).split(",")
    clip = re.search(r"\bawry_map_pairs_clip_batch\s*\(([^)]*)\)", src).group(1).split(",")
    at = [i for i, a in enumerate(e2e) if "rescue_edits" in a][0] + 1
    norm = lambda args: [" ".join(a.split()) for a in args]
    assert norm(clip[:at]) == norm(e2e[:at]) and norm(clip[at + 5:]) == [a.replace("awry_map_t", "awry_map_clip_t") for a in norm(e2e[at:])]
    assert norm(clip[at:at + 5]) == ["uint32_t match", "uint32_t mismatch", "uint32_t gap", "uint32_t end_bonus", "uint32_t min_aln_score"]
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for word in ("pub const AWRY_PAIR_CLIP_MAX_UNPAIRED: u32 = 16384;", "pub fn awry_map_pairs_clip_batch(", "pub fn awry_dev_pair_windows_clip(",
                 "pub fn awry_dev_pair_select_clip("):
        assert word in rust, word
    safe = open(os.path.join(ROOT, "rust", "awry", "src", "fm_index.rs")).read()
    assert "pub fn parallel_map_pairs_clip(" in safe and "sys::awry_map_pairs_clip_batch(" in safe
    hpp = open(os.path.join(ROOT, "include", "awry.hpp")).read()
    assert "parallel_map_pairs_clip(" in hpp and "awry_map_pairs_clip_batch(" in hpp
    for fn in (FmIndex.parallel_map_pairs_clip_csr, FmIndex.parallel_map_pairs_clip):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in ("min_insert", "max_insert", "unpaired_penalty", "rescue_anchors", "rescue_edits", "match", "mismatch", "gap",
                                         "end_bonus", "min_aln_score")] == [0, 1000, 20, 2, 4, 1, 4, 6, 5, 0]
    assert callable(FmIndex.dev_pair_windows_clip) and callable(FmIndex.dev_pair_select_clip)


def test_cpp_mirror_method_compiles(tmp_path):
    src = tmp_path / "pairs_clip.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "int64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> r1{"ACGTACGTACGT", "GATTACAGATTACA"}, r2{"TTTTACGTACGT", "GATTACAGACCACA"};\n'
                   "  int64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  awry::FmIndex::PairParams pp;\n"
                   "  pp.max_insert = 600; pp.rescue_edits = 8; pp.unpaired_penalty = 20;\n"
                   "  awry::FmIndex::ClipParams cp;\n"
                   "  cp.min_aln_score = 30;\n"
                   "  for (const awry::FmIndex::ClippedPairMapping& pm : ix.parallel_map_pairs_clip(r1, r2, 12, 50, 4, 4, pp, cp, awry::FmIndex::ChainParams(), &status)) {\n"
                   "    s += pm.insert;\n"
                   "    for (const awry::FmIndex::ClippedMapping& m : pm.mate1) s += m.map.score + m.map.clip_left + (m.map.flags & AWRY_MAP_PROPER_PAIR);\n"
                   "    for (const awry::FmIndex::ClippedMapping& m : pm.mate2) s += m.map.t_end + m.map.clip_right + (m.map.chain_index == AWRY_PAIR_NO_CHAIN) + m.cigar.size();\n"
                   "  }\n"
                   "  static_assert(AWRY_PAIR_CLIP_MAX_UNPAIRED == 16384, \"limit\");\n"
                   "  if (awry::FmIndex::clipped_pair_defaults().unpaired_penalty != 20) return -1;\n"
                   "  return s + (int64_t)ix.parallel_map_pairs_clip(r1, r2).size();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- errors that need no device ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hostonly_index():
    t, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    return FmIndex.from_text(t, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def test_without_replicas_the_calls_return_no_device(hostonly_index):
    ix = hostonly_index
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACA"])
    for call in (lambda: ix.parallel_map_pairs_clip_csr(qb, qo), lambda: ix.parallel_map_pairs_clip([b"ACGT"], [b"ACGG"], min_len=1, max_hits=5),
                 lambda: ix.dev_pair_windows_clip(None, None, None, 0, 0, 1000, 2, 4, None, None, None),
                 lambda: ix.dev_pair_select_clip(None, None, None, None, 0, 0, 1000, 20, 2, 1, 4, 6, 5, 0, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_bad_parameters_are_argument_errors(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT", b"GATTACAGATTACA"])
    qb3, qo3 = pack_queries([b"ACGTACGTACGT", b"GATTACAGATTACA", b"ACGTACGTACGT"])
    ix = hostonly_index
    sel = lambda *a: ix.dev_pair_select_clip(None, None, None, None, 0, *a, None)
    bad = [lambda: ix.parallel_map_pairs_clip_csr(qb3, qo3),  # an odd number of reads
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, min_insert=501, max_insert=500), lambda: ix.parallel_map_pairs_clip_csr(qb, qo, max_insert=PAIR_MAX_INSERT + 1),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, unpaired_penalty=16385), lambda: ix.parallel_map_pairs_clip_csr(qb, qo, rescue_anchors=5),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, rescue_edits=9), lambda: ix.parallel_map_pairs_clip_csr(qb, qo, rescue_edits=-1),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, chains_per_strand=0), lambda: ix.parallel_map_pairs_clip_csr(qb, qo, chains_per_strand=9),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, band=9), lambda: ix.parallel_map_pairs_clip_csr(qb, qo, min_len=0),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, max_hits=0),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, match=0), lambda: ix.parallel_map_pairs_clip_csr(qb, qo, match=17),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, mismatch=65), lambda: ix.parallel_map_pairs_clip_csr(qb, qo, gap=65),
           lambda: ix.parallel_map_pairs_clip_csr(qb, qo, end_bonus=1025),
           lambda: ix.dev_pair_windows_clip(None, None, None, 0, 2, 1, 2, 4, None, None, None),
           lambda: ix.dev_pair_windows_clip(None, None, None, 0, 0, 1000, 5, 4, None, None, None),
           lambda: ix.dev_pair_windows_clip(None, None, None, 0, 0, 1000, 2, 9, None, None, None),
           lambda: sel(0, PAIR_MAX_INSERT + 1, 20, 2, 1, 4, 6, 5, 0), lambda: sel(0, 1000, 16385, 2, 1, 4, 6, 5, 0), lambda: sel(0, 1000, 20, 5, 1, 4, 6, 5, 0),
           lambda: sel(0, 1000, 20, 2, 0, 4, 6, 5, 0), lambda: sel(0, 1000, 20, 2, 1, 65, 6, 5, 0), lambda: sel(0, 1000, 20, 2, 1, 4, 65, 5, 0),
           lambda: sel(0, 1000, 20, 2, 1, 4, 6, 1025, 0)]
    for k, call in enumerate(bad):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG, k
    # the limits themselves pass the argument checks: what is left to fail is the missing replica.  The penalty is in score units here:
    # 256, one past the end-to-end call's range, is inside
    for call in (lambda: ix.parallel_map_pairs_clip_csr(qb, qo, min_insert=PAIR_MAX_INSERT, max_insert=PAIR_MAX_INSERT, unpaired_penalty=16384, rescue_anchors=4,
                                                        rescue_edits=8, match=16, mismatch=64, gap=64, end_bonus=1024, min_aln_score=1 << 31),
                 lambda: ix.parallel_map_pairs_clip_csr(qb, qo, unpaired_penalty=0, rescue_anchors=0, rescue_edits=0, match=1, mismatch=0, gap=0, end_bonus=0),
                 lambda: ix.parallel_map_pairs_clip_csr(qb, qo, unpaired_penalty=256), lambda: sel(0, 1000, 16384, 4, 16, 64, 64, 1024, 1 << 31)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE
    with pytest.raises(AwryError) as e:  # the end-to-end call keeps its own range
        ix.parallel_map_pairs_csr(qb, qo, unpaired_penalty=256)
    assert e.value.code == ERR_ARG
    # an amino index is an argument error, before any device is asked for
    t, st, hd = synth.make_text(1_000, 1, 5, 1, 0.0)
    aa = FmIndex.from_text(t, 1, 8, 0, st, hd, build_device=BUILD_HOST)
    for call in (lambda: aa.parallel_map_pairs_clip_csr(*pack_queries([b"ACDEFGHIKLMN", b"ACDEFGHIKLMN"])),
                 lambda: aa.dev_pair_windows_clip(None, None, None, 0, 0, 1000, 2, 4, None, None, None),
                 lambda: aa.dev_pair_select_clip(None, None, None, None, 0, 0, 1000, 20, 2, 1, 4, 6, 5, 0, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    aa.close()
    # the out-pointers of a failed call stay as they were; cigar_off_out without cigar_out is an argument error too
    L = _lib.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    clip = (1, 4, 6, 5, 0)
    for n, tail in ((3, (4, 4, 0, 1000, 20, 2, 4) + clip), (2, (4, 4, 2, 1, 20, 2, 4) + clip), (2, (4, 4, 0, 1000, 16385, 2, 4) + clip),
                    (2, (4, 4, 0, 1000, 20, 2, 9) + clip), (2, (4, 4, 0, 1000, 20, 2, 4, 17, 4, 6, 5, 0)), (2, (4, 4, 0, 1000, 20, 2, 4, 1, 4, 6, 1025, 0))):
        off, m, ps, coff, cg, st, ins = u64p(), C.POINTER(_lib.MapClip)(), C.POINTER(_lib.Pos)(), u64p(), u32p(), u8p(), u32p()
        rc = L.awry_map_pairs_clip_batch(ix._h, qb3.ctypes.data, qo3.ctypes.data_as(u64p), n, 12, 50, 100, 16, 100, 0, 1, *tail, C.byref(off), C.byref(m),
                                         C.byref(ps), C.byref(coff), C.byref(cg), C.byref(st), C.byref(ins))
        assert rc == ERR_ARG and not off and not m and not ps and not coff and not cg and not st and not ins, tail
    off, coff = u64p(), u64p()
    rc = L.awry_map_pairs_clip_batch(ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), 2, 12, 50, 100, 16, 100, 0, 1, 4, 4, 0, 1000, 20, 2, 4, *clip, C.byref(off),
                                     None, None, C.byref(coff), None, None, None)
    assert rc == ERR_ARG and not off and not coff


# ---- the fixture, from the reference alone ------------------------------------------------------------------------------------------

def unseedable(q):
    """96 letters with a substitution every 11th letter: no exact run reaches min_len = 12, and that is 8 edits"""
    q = bytearray(q[:96])
    for at in range(10, 96, 11):
        q[at] = b"ACGT"[(b"ACGT".index(q[at]) + 1) % 4]
    return bytes(q)


def fixture_pairs(text, st, n=200, seed=71):
    """n simulated pairs, built as the end-to-end suite's: fragments of 150..600 letters inside one record and free of N, mates of 101
    letters from the fragment's two ends with 0..2 substitutions and at most one indel of one letter each, every second pair taken from
    the reverse strand (mate 0 is the fragment's right end); in every eighth pair one mate -- mate 0 and mate 1 in turn -- is
    `unseedable`.  Every fourth pair (i % 4 == 1) is a read-through pair instead: a fragment of F in 50..95 letters, both mates the
    whole fragment, unedited, read from either end and filled up to 101 letters with 101 - F random letters, the first of which does
    not continue the fragment; they alternate between the strands too.
    -> [(mate 0, mate 1, (strand, origin, indel total) of mate 0, the same of mate 1, F or None)]; origin: where the mate's forward
    window begins, of a read-through mate where the fragment begins"""
    rng = np.random.default_rng(seed)
    body, bounds = bytes(text[:-1]), [int(x) for x in st] + [len(text) - 1]
    out = []
    while len(out) < n:
        i = len(out)
        through = i % 4 == 1
        F, r = int(rng.integers(50, 96)) if through else int(rng.integers(150, 601)), int(rng.integers(0, len(st)))
        at = int(rng.integers(bounds[r], bounds[r + 1] - F))
        frag = body[at:at + F]
        if any(ch not in b"ACGT" for ch in frag):
            continue
        if through:
            # (the letter next to the fragment differs from the text's: a tail letter that happens to continue the fragment is aligned, not
            # clipped, the two aligned spans then differ at that end, and the order conditions of proper_clip, which are on the aligned
            # spans, fail -- with wholly random tails that happened to 28 of these 50 pairs)
            tails = [bytearray(synth.NT[rng.integers(0, 4, size=101 - F)]) for _ in (0, 1)]
            for tail, nxt in ((tails[0], body[at + F:at + F + 1]), (tails[1], mp.rc(body[max(at - 1, 0):at]))):
                while tail[:1] == nxt:
                    tail[0] = b"ACGT"[(b"ACGT".index(tail[:1]) + 1) % 4]
            fwd, rev = (frag + bytes(tails[0]), (0, at, 0)), (mp.rc(frag) + bytes(tails[1]), (1, at, 0))
            a, b = (rev, fwd) if (i // 4) % 2 else (fwd, rev)
            out.append((a[0], b[0], a[1], b[1], F))
            continue
        hard = (i // 8) % 2 if i % 8 == 3 else None  # which mate seeds nowhere
        mates = []
        for m, (w, origin) in enumerate(((frag[:101], at), (frag[-101:], at + F - 101))):
            if hard == m:  # (of the right end the last 96 letters, so that the fragment's outer end stays)
                mates.append((unseedable(frag[:96]), at, 0) if m == 0 else (unseedable(frag[-96:]), at + F - 96, 0))
                continue
            q, indels = bytearray(w), 0
            for _ in range(int(rng.integers(0, 3))):
                p = int(rng.integers(0, len(q)))
                q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1 + int(rng.integers(0, 3))) % 4]
            if rng.random() < 0.3:
                p = int(rng.integers(30, 70))
                if rng.random() < 0.5:
                    del q[p]
                else:
                    q[p:p] = b"ACGT"[int(rng.integers(0, 4)):][:1]
                indels = 1
            mates.append((bytes(q), origin, indels))
        (f, fo, fi), (v, vo, vi) = mates
        fwd, rev = (f, (0, fo, fi)), (mp.rc(v), (1, vo, vi))
        a, b = (rev, fwd) if i % 2 else (fwd, rev)
        out.append((a[0], b[0], a[1], b[1], None))
    return out


def fixture_character(pairs, per_read, inserts):
    """-> (read-through pairs that come out proper with |insert - F| <= 4 and both mates at the fragment -- on their planted strands,
    both ends of the aligned span within 4 letters of the fragment's --, other pairs that come out proper with both mates on their
    planted strands within their indel totals of their origins, rescued mates)"""
    through = others = rescued = 0
    for p, (_, _, w0, w1, F) in enumerate(pairs):
        recs = [per_read[2 * p + m][1] for m in (0, 1)]
        rescued += sum(1 for r in recs if r and r[0][7] & MAP_RESCUED)
        if not all(r and r[0][7] & MAP_PROPER_PAIR and r[0][5] == w[0] for r, w in zip(recs, (w0, w1))):
            continue
        if F is None:
            others += all(abs(r[0][0] - w[1]) <= w[2] for r, w in zip(recs, (w0, w1)))
        else:
            through += abs(inserts[p] - F) <= 4 and all(abs(r[0][0] - w[1]) <= 4 and abs(r[0][1] - (w[1] + F)) <= 4 for r, w in zip(recs, (w0, w1)))
    return through, others, rescued


def interleaved(pairs):
    return [q for p in pairs for q in p[:2]]


def test_the_fixture_pairs_are_paired_clipped_and_rescued_by_the_reference(oracle):
    w = HostWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)
    pairs = fixture_pairs(w.text, w.st)
    thr = [p for p in pairs if p[4] is not None]
    assert len(pairs) == 200 and len(thr) == FIXTURE["through"] and all(50 <= p[4] <= 95 and len(p[0]) == len(p[1]) == 101 for p in thr)
    assert sum(p[2][0] for p in thr) == 25 and sum(p[2][0] for p in pairs) == 75
    hard = [q for p in pairs for q in p[:2] if len(q) == 96]
    assert len(hard) == 25
    chains_of = lambda qs: want_chains(w, qs, *KEY, E2E_PARAMS[KEY])[0]
    t = er.Text(w.text, 0)
    tsym = [int(v) for v in mr.to_symbols(bytes(w.text), 0)][:-1]
    a = PAIR_ARGS
    per, inserts = pc.map_pairs_clip(t, tsym, interleaved(pairs), chains_of, 4, 4, w.st, a["mn"], a["mx"], a["U"], a["G"], a["k"], WTS, T_MAIN)
    through, others, rescued = fixture_character(pairs, per, inserts)
    # the same reads and parameters end to end: how many read-through pairs come out proper at all
    per_e, _ = pr.map_pairs(t, tsym, interleaved(pairs), chains_of, 4, 4, w.st, a["mn"], a["mx"], a["U"], a["G"], a["k"])
    e2e = sum(1 for p, pair in enumerate(pairs) if pair[4] is not None and
              all(per_e[2 * p + m][1] and per_e[2 * p + m][1][0][7] & MAP_PROPER_PAIR for m in (0, 1)))
    print("read-through pairs proper at the fragment: %d of %d (end to end, proper at all: %d); other pairs proper at their origins: %d of %d; rescued mates: %d"
          % (through, len(thr), e2e, others, len(pairs) - len(thr), rescued))
    assert through >= FIXTURE["through_min"] and 10 * FIXTURE["through_min"] >= 8 * len(thr)
    assert e2e <= FIXTURE["e2e_max"] and 2 * FIXTURE["e2e_max"] < len(thr)
    assert others >= FIXTURE["others_min"] and 10 * FIXTURE["others_min"] >= 9 * (len(pairs) - len(thr))
    assert rescued >= FIXTURE["rescued_min"] == 10
    assert (through, e2e, others, rescued) == (FIXTURE["through_proper"], FIXTURE["e2e_proper"], FIXTURE["others_proper"], FIXTURE["rescued"])
    for p, x in enumerate(inserts):  # property 3, and every record's runs replay to its fields (property 1)
        if x:
            assert a["mn"] <= x <= a["mx"]
    for q, (_, recs, runs) in zip(interleaved(pairs), per):
        for r, cg in zip(recs, runs):
            replay_record(tsym, q, r, cg, WTS)


def replay_record(tsym, read, r, cigar, wts):
    """property 1: the runs of record r (uint32, length << 4 | op) over the read (its reverse complement on strand 1) and the text from
    t_begin reproduce the read's length, t_end, edits, score and both clips"""
    q = [int(v) for v in mr.to_symbols(mp.rc(read) if r[5] else bytes(read), 0)]
    runs = [(int(x) >> 4, "MIDNS..=X"[int(x) & 15]) for x in cigar]
    used, t_end, edits, score, cl, cr_ = cr.replay(q, tsym, r[0], runs, wts)
    assert (used, t_end, edits, score, cl, cr_) == (len(q), r[1], r[2], r[8], r[9], r[10]), (r, runs)
