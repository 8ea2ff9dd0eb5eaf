"""The read pipelines -- anchors, SMEMs, edit locate, edit align, chaining, chain alignment, mapping -- with lanes that take item
after item.  Their kernels are stride loops over items (one per lane or per group of lanes) with scratch indexed by grid lane,
and the suites of tests/test_{anchors,smems,edit,align,chain,chain_align,map}_gpu.py launch at most ~3000 items on grids of 10^5
lanes: no lane there meets a second item.  awry_debug_set_max_blocks bounds the grid instead of growing the batch: under
max_blocks(1) a launch has 256 lanes (16 or 4 groups), under max_blocks(3) 768, so a few hundred items wrap by construction.
Each case runs under both.  Where a case has more than 768 items the two strides pair them differently; the cases the issue
sizes below that -- the 700 reads of the SMEM and anchor device forms, the few hundred reads of the map, chain-align and chain
batch calls -- wrap under the first bound only, and their lane-order assertions are made at stride 256 (at the second bound the
locate drivers' tile queue and the chaining groups still take several items).

Every case reuses the inputs, helpers and references of the module that owns the kernel and compares for exact equality, guard
words included.  What a case is for is asserted on its own inputs before anything runs: no lane (group) meets the same item twice
in a row (items[k] != items[k + stride]), and the named transitions occur on one lane, in both orders.  For the chain alignment
kernels the lanes stride over the class lists, which the classify kernel fills in the order of its atomics; the assertions are
made on the lists in chain order.  The long / short pairs lie in runs of 384 and 750 equal-kind chains, so any order inside one
classify trip leaves most lanes their pairs; the pair "both extensions and two gaps" -> "whole 1" is eight single chains and holds
on the device only where a trip's atomics append in chain order.

One test runs at the real geometry without a bound (test_map_at_one_grid_and_a_bit): a map call of CUs x 8 x 256 + 4096 reads,
where the default sub-batch of 2^18 chains is crossed and every offset passes the grid.

Wall times on one MI355X (256 CUs) from one sitting of the whole suite (574 passed in 490 s, `--durations=0`).  The slowest test
of test_mismatch_scale_gpu.py there: test_lane_refill_count[amino] 7.30 s.  This file, setup and call of the slowest case of each:
  read pool fixture 2.88 s; SMEMs and anchors 0.61 s (lf), 0.41 s (sa), 0.24 / 0.13 s at bound 3
  sub-batch of 7 and hit capacity of 64: 1.51 s; map, chain-align and chain calls 0.86 s
  edit batch fixture 0.67 s, its calls 0.15 s; test_map_at_one_grid_and_a_bit 0.53 s (528 384 reads, the call 0.1 s)
  chain seeds 0.26 s; select lists fixture 0.25 s, map select 0.18 s; revcomp 0.21 s; edit windows 0.19 s
  chain alignment, edit alignment and the input checks: under 0.05 s each (references memoised per distinct chain or hit)
"""
import contextlib
import os
import time

import numpy as np
import pytest

import awry_amd
from awry_amd.fm_index import ALN_OK, ANCHOR_DTYPE, Q_SEED_CAP, pack_queries
from tests import align_ref as al
from tests import anchor_ref as ar
from tests import chain_align_ref as ca
from tests import chain_ref as cr
from tests import edit_ref as er
from tests import map_ref as mp
from tests import smem_ref as sr
from tests import synth
from tests import test_align_gpu as ag
from tests import test_chain_align_gpu as cag
from tests import test_chain_gpu as cg
from tests import test_edit_gpu as eg
from tests import test_map_gpu as mg
from tests.test_anchors_gpu import nt_queries
from tests.test_map_cpu import fixture_reads, hand_made_lists
from tests.test_mismatch_scale_gpu import gather
from tests.test_smems_gpu import edge_queries

pytestmark = pytest.mark.gpu

BOUNDS = (1, 3)
KEY, P_MAIN = cag.KEY, mg.P_MAIN
L_ = awry_amd.load_library()


@contextlib.contextmanager
def max_blocks(b):
    assert L_.awry_debug_set_max_blocks(b) == 0
    try:
        yield
    finally:
        L_.awry_debug_set_max_blocks(0)


def teardown_module(module):
    assert L_.awry_debug_max_blocks() == 0


def lane_pairs(items, stride):
    """what one lane of a stride loop meets one after the other: {(items[k], items[k + stride])}"""
    return {(items[k], items[k + stride]) for k in range(len(items) - stride)}


def assert_no_lane_repeats(items, stride):
    bad = [k for k in range(len(items) - stride) if items[k] == items[k + stride]]
    assert not bad, (stride, bad[:5])


def test_the_getter_follows_the_switch_and_the_bound_is_lifted_on_the_way_out():
    assert L_.awry_debug_max_blocks() == 0
    with max_blocks(3):
        assert L_.awry_debug_max_blocks() == 3
        with max_blocks(1):
            assert L_.awry_debug_max_blocks() == 1
    assert L_.awry_debug_max_blocks() == 0
    with pytest.raises(ZeroDivisionError):
        with max_blocks(2):
            1 // 0
    assert L_.awry_debug_max_blocks() == 0
    assert L_.awry_debug_set_max_blocks(-1) != 0 and L_.awry_debug_max_blocks() == 0


@pytest.fixture(scope="module")
def nt(oracle):
    w = mg.OracleWorld(oracle, *synth.make_text(40_000, 0, 21, 5, 0.03), 0)
    w.tsym = mg.symbols(w.text)[:-1]
    return w


# ---- dev_align_chains ---------------------------------------------------------------------------------------------------------------

M_CHAINS = 1500
SHORT_RUN, LONG_RUN = 384, 750  # chains [0, 384) short, [384, 1134) of 1024 letters, then the other cases and short ones again


def chain_cases(text, st):
    """tests/test_chain_align_gpu.py's hand-made chains and three of this file's: a chain with both extensions and two gaps, and
    two more of 1024 letters whose tables cover most of the rows (left extension, gaps, right extension)"""
    cases = cag.hand_made_chains(text, st)
    tb = bytes(text[:-1])
    cut = lambda p, L: tb[p:p + L]
    p = 5000
    cases.append(("both extensions and two gaps", cag.substitute(cut(p, 90), (3, 35, 36, 62, 88)), [(10, 20, p + 10), (40, 15, p + 40), (65, 15, p + 65)]))
    p = 9000
    cases.append(("two gaps 1024", cag.substitute(cut(p, 1024), (5, 250, 500, 650, 1000)), [(300, 100, p + 300), (700, 100, p + 700)]))
    p = 13000
    cases.append(("late piece 1024", cag.substitute(cut(p, 1024), (100, 400, 800, 1023)), [(900, 60, p + 900)]))
    return cases


@pytest.fixture(scope="module")
def chains(nt):
    cases = chain_cases(nt.text, nt.st)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    at = {name: i for i, name in enumerate(names)}
    short = [at["%s %d" % (kind, L)] for L in (1, 2, 17) for kind in ("whole", "middle")]
    long_ = [at["middle 1024"], at["two gaps 1024"], at["late piece 1024"]]
    both, whole1 = at["both extensions and two gaps"], at["whole 1"]
    bad = [at[x] for x in ("unsorted in the query", "past L", "empty", "17 over the start", "gap with 17 deleted", "t_pos past n", "past n")]
    others = [i for i in range(len(cases)) if i not in short and i not in long_ and len(cases[i][1]) < 1024]
    cyc = [i for i in short if i != whole1]  # five kinds: 256 and 263 (a list position after the seven dropped chains) are no multiples of 5
    pick = [cyc[k % 5] for k in range(SHORT_RUN)] + [long_[k % 3] for k in range(LONG_RUN)] + others
    pick += [cyc[k % 5] for k in range(M_CHAINS - len(pick))]
    for j in range(7):
        pick[100 + j] = bad[j]          # chains that are not aligned: an aligned one on the same classify lane one trip later, and before
    for j in range(8):                  # "whole 1" one trip after `both` in the class list, which has lost the seven by then
        pick[8 + j] = both
        pick[8 + j + 256 + 7] = pick[8 + j + 768 + 7] = whole1
    assert len(pick) == M_CHAINS
    return cases, cag.Reference(nt.tsym, cases), pick, dict(short=set(short), long=set(long_), both=both, whole1=whole1)


@pytest.mark.parametrize("band", (0, 4, 8))
def test_the_chain_job_holds_what_it_is_for(nt, chains, band):
    cases, ref, pick, kinds = chains
    n = len(nt.text) - 1
    nb = [ca.widest_band(n, len(cases[i][1]), cases[i][2], band) for i in pick]
    cls = [None if b is None else 0 if b <= 9 else 1 if b <= 17 else 2 for b in nb]
    main = 0 if 2 * band + 1 <= 9 else 1
    # the runs are one class: skew 0, the narrowest class the band allows
    assert all(len(cases[i][1]) <= 17 for i in kinds["short"]) and all(len(cases[i][1]) == 1024 for i in kinds["long"])
    assert all(cls[k] == main and nb[k] == 2 * band + 1 for k in range(SHORT_RUN + LONG_RUN) if pick[k] in kinds["short"] | kinds["long"])
    assert ref.one(kinds["both"], band)[0] == ALN_OK and cls[8] == main
    runs = ref.one(kinds["both"], band)[4]
    assert cases[kinds["both"]][2][0][0] > 0 and sum(ln for ln, _ in runs if _ != "D") == 90 and len(cases[kinds["both"]][2]) == 3
    for i in kinds["long"] | {j for j in kinds["short"] if cases[j][0] in ("middle 17", "middle 2")}:
        assert ref.one(i, band)[5] > 0, cases[i][0]  # table cells: the chain writes direction words
    status = [ref.one(i, band)[0] for i in pick]
    lists = {c: [pick[k] for k in range(M_CHAINS) if cls[k] == c] for c in (0, 1, 2)}
    assert sum(1 for c in lists if lists[c]) >= 2 and len(lists[main]) > SHORT_RUN + LONG_RUN
    kind = lambda i: "long" if i in kinds["long"] else "short" if i in kinds["short"] else cases[i][0]
    for stride in (256, 768):
        assert_no_lane_repeats(pick, stride)              # the classify kernel's lanes
        for c in lists:
            assert_no_lane_repeats(lists[c], stride)      # the alignment kernels' lanes
        pairs = {(kind(a), kind(b)) for a, b in lane_pairs(lists[main], stride)}
        assert ("long", "short") in pairs and ("short", "long") in pairs, stride
        assert ("both extensions and two gaps", "short") in pairs and (kinds["both"], kinds["whole1"]) in lane_pairs(lists[main], stride)
        assert any(status[k] != ALN_OK and status[k + stride] == ALN_OK for k in range(M_CHAINS - stride))
        assert any(status[k] == ALN_OK and status[k + stride] != ALN_OK for k in range(M_CHAINS - stride))
    assert any(status[k] != ALN_OK and status[k + 1] == ALN_OK for k in range(M_CHAINS - 1))


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("band", (0, 4, 8))
def test_align_chains_with_lanes_that_take_several_chains(nt, chains, band, bound):
    cases, ref, pick, _ = chains
    want = ref.many(pick, band)
    j = cag.device_job(nt.ix, cag.pack_job(cases, pick), band, len(want[2]))
    with max_blocks(bound):
        cag.run_job(nt.ix, j)
        nt.ix.dev_synchronize()
    cag.assert_equals_reference(cag.job_result(nt.ix, j), want, [cases[i][0] for i in pick])


# ---- dev_chain_seeds ----------------------------------------------------------------------------------------------------------------

def chain_order(sets, ngroups, max_seeds, tile):
    """-> the set taken by query q, so that group g (queries g, g + ngroups, ..) takes in turn the 4096-seed set (slab), a set within
    the LDS tile, the set one over max_seeds, a slab set again, and a tile set before the next 4096"""
    size = [len(s) for s in sets]
    big, again, over = size.index(4096), size.index(300), size.index(max_seeds + 1)
    small = [i for i, s in enumerate(size) if 1 <= s <= 64]
    assert len(small) >= 10 and tile < 300
    n = max(120, 5 * ngroups)
    order = []
    for q in range(n):
        g, t = q % ngroups, q // ngroups
        order.append((big, small[(g + 3 * t) % len(small)], over, again, small[(g + 3 * t + 1) % len(small)])[t % 5])
    return order


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("lookback,width", ((16, None), (64, None), (16, "64")))
def test_chain_seeds_with_groups_that_alternate_between_slab_and_tile(nt, lookback, width, bound):
    sets = cg.synthetic_sets(nt.st)
    P = cr.Params(4096, lookback, 120, 6, 4)
    G = 16 if lookback <= 16 and width is None else 64
    ngroups = bound * 256 // G
    order = chain_order(sets, ngroups, P.max_seeds, 64 if G == 16 else 256)
    assert_no_lane_repeats(order, ngroups)
    size = lambda i: len(sets[i])
    path = lambda i: "capped" if size(i) > P.max_seeds else "tile" if size(i) <= (64 if G == 16 else 256) else "slab"
    seq = [path(i) for i in order[0::ngroups]]  # group 0; every group's sequence has these paths in this order
    assert len(order) > 4 * ngroups and seq[:5] == ["slab", "tile", "capped", "slab", "tile"] and (len(seq) == 5 or seq[5] == "slab")
    assert all([path(i) for i in order[g::ngroups]][:5] == seq[:5] for g in range(ngroups))
    st = [int(x) for x in nt.st]
    memo = {}
    for i in set(order):
        memo[i] = cr.chain_query(sets[i], st, P)
    want = cr.as_csr([memo[i][:2] for i in order])
    wtally = tuple(sum(memo[i][2][k] for i in order) for k in range(3))
    assert int(want[4][order.index(size_index(sets, 4097))]) == Q_SEED_CAP and int(want[0][-1]) > len(order)
    jobs_sets = [sets[i] for i in order]
    if width:
        os.environ["AWRY_CHAIN_GROUP"] = width
    try:
        j = cg.device_job(nt.ix, jobs_sets, P, tally=True)
        with max_blocks(bound):
            cg.run_job(nt.ix, j)
            nt.ix.dev_synchronize()
        got = cg.job_result(nt.ix, j)
        cg.assert_equals_reference(got, want, j["cap_c"], j["cap_m"])
        assert tuple(int(x) for x in got["t"]) == wtally
        # the slabs were allocated for one block's groups: the first launch without the bound grows them
        j = cg.device_job(nt.ix, jobs_sets, P, tally=True)
        cg.run_job(nt.ix, j)
        nt.ix.dev_synchronize()
        got = cg.job_result(nt.ix, j)
        cg.assert_equals_reference(got, want, j["cap_c"], j["cap_m"])
        assert tuple(int(x) for x in got["t"]) == wtally
    finally:
        os.environ.pop("AWRY_CHAIN_GROUP", None)


def size_index(sets, n):
    return [len(s) for s in sets].index(n)


# ---- dev_smems, dev_anchors and their locate drivers --------------------------------------------------------------------------------

N_QUERIES, MIN_LEN, MAX_HITS = 700, 12, 500


def gather2(off, rows, sub_off, draw, *arrays):
    """a two-level CSR (item i owns the records [off[i], off[i + 1]), record r the entries [sub_off[r], sub_off[r + 1]) of `arrays`)
    for the items `draw` -> (off, rows, sub_off, arrays) of the drawn batch"""
    o, r, cnt = gather(off, draw, rows, np.diff(sub_off.astype(np.int64)))
    so = np.zeros(len(r) + 1, np.uint64)
    so[1:] = np.cumsum(cnt)
    outs = gather(sub_off[off.astype(np.int64)], draw, *arrays)
    assert int(outs[0][-1]) == int(so[-1])
    return (o, r, so) + tuple(outs[1:])


@pytest.fixture(scope="module")
def read_pool(nt):
    """the fixture reads of the anchor and SMEM suites with the edge queries, each with the definition's SMEMs and anchors, and the
    draw of 700: lanes 0 .. 7 of a 256-lane grid take a long read, then a one-letter read, then a long read; lanes 8 .. 15 a read
    without an SMEM of MIN_LEN letters, then one with many, then one without (every letter occurs in the text, so every read has SMEMs
    of one letter)"""
    pool = list(dict.fromkeys(nt_queries(nt, (6, nt.ix.seed_kmer_len())) + edge_queries(nt)))
    smems = [sr.smems_definition(nt.ctext, nt.oi, q, 0, 1) for q in pool]
    anchors = [ar.anchors_definition(nt.ctext, nt.oi, q, 0, 1, 0) for q in pool]
    longs = [i for i, q in enumerate(pool) if len(q) >= 1000]
    ones = [i for i, q in enumerate(pool) if len(q) == 1]
    kept = [sum(1 for a in s if a[1] >= MIN_LEN) for s in smems]
    none = [i for i in range(len(pool)) if not kept[i] and len(pool[i]) > 1]
    many = sorted(range(len(pool)), key=lambda i: -kept[i])[:8]
    assert len(longs) >= 3 and len(ones) >= 3 and len(none) >= 2 and kept[many[-1]] >= 4, (len(none), [kept[i] for i in many])
    rest = [i for i in range(len(pool)) if i not in longs]
    draw = [rest[(7 * k + 3) % len(rest)] for k in range(N_QUERIES)]
    for j in range(8):
        draw[j], draw[256 + j], draw[512 + j] = longs[j % len(longs)], ones[j % len(ones)], longs[(j + 1) % len(longs)]
        draw[8 + j], draw[264 + j], draw[520 + j] = none[j % len(none)], many[j], none[(j + 1) % len(none)]
    assert_no_lane_repeats(draw, 256)
    pairs = lane_pairs(draw, 256)
    assert any(a in longs and b in ones for a, b in pairs) and any(a in ones and b in longs for a, b in pairs)
    assert any(a in none and b in many for a, b in pairs) and any(a in many and b in none for a, b in pairs)
    return pool, smems, anchors, np.array(draw, np.int64), {}


def records_job(ix, qs, n_records, launch):
    """both passes of a device form that writes 24-byte records: upload, pre-fill with 0xEE, count, scan, fill -> (n, off, status, raw)"""
    qb, qo = pack_queries(qs)
    n, cap = len(qs), n_records + 4
    d = dict(q=ix.dev_upload(np.concatenate([qb, np.zeros(16, np.uint8)])), o=ix.dev_upload(qo), n=ix.dev_malloc(8 * (n + 2)), off=ix.dev_malloc(8 * (n + 1)),
             scr=ix.dev_malloc(ix.dev_scan_scratch_bytes(n)), st=ix.dev_malloc(n + 8), a=ix.dev_malloc(24 * cap))
    try:
        ix.dev_memset(d["a"], 0xEE, 24 * cap)
        ix.dev_memset(d["st"], 0xEE, n + 8)
        ix.dev_memset(d["n"], 0xEE, 8 * (n + 2))
        launch(d["q"], d["o"], n, d["n"], None, None, d["st"])
        ix.dev_scan_counts(d["n"], n, d["off"], d["scr"])
        launch(d["q"], d["o"], n, None, d["off"], d["a"], None)
        ix.dev_synchronize()
        return (ix.dev_download(d["n"], (n + 2,), np.uint64), ix.dev_download(d["off"], (n + 1,), np.uint64), ix.dev_download(d["st"], (n + 8,), np.uint8),
                ix.dev_download(d["a"], (24 * cap,), np.uint8))
    finally:
        for p in d.values():
            ix.dev_free(p)


def assert_records(got, n, good, woff, wrows):
    ns, off, status, raw = got
    wn = np.zeros(n, np.uint64)
    wn[good] = np.diff(woff)
    assert np.array_equal(ns[:n], wn) and np.all(ns[n:] == 0xEEEEEEEEEEEEEEEE)
    assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(wn, dtype=np.uint64))
    bad = np.ones(n, bool)
    bad[good] = False
    assert np.all(status[:n][~bad] == 0) and np.all(status[:n][bad] != 0) and np.all(status[n:] == 0xEE)
    tot = int(off[-1])
    got_rows = ar.got_as_rows(raw[:24 * tot].view(ANCHOR_DTYPE))
    miss = np.nonzero((got_rows != wrows).any(axis=1))[0]
    assert not len(miss), ("query", int(np.searchsorted(off, miss[0], side="right")) - 1, got_rows[miss[0]], wrows[miss[0]])
    assert np.all(raw[24 * tot:] == 0xEE)  # nothing written past the last record


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("form", ("sa", "lf"))
def test_smems_and_anchors_with_lanes_that_take_several_reads(nt, read_pool, form, bound):
    pool, smems, anchors, draw, located_memo = read_pool
    ix = nt.ix
    located = lambda what, make: located_memo[what] if what in located_memo else located_memo.setdefault(what, make())
    qs = [pool[i] for i in draw]
    dev_qs = list(qs)
    for j in (256, 258):
        dev_qs[j] = b""  # the device forms answer an empty read with a status: the long read of lane j is followed by it
    good = [i for i, q in enumerate(dev_qs) if len(q)]
    qb, qo = pack_queries(qs)
    if form == "lf":
        ix.set_verify(-1)
    try:
        assert ix.verify_enabled() == (form == "sa")
        for what, full, launch, locate in (
                ("smems", smems, lambda m: lambda q, o, n, *a: ix.dev_smems(q, o, n, m, *a), lambda: ix.parallel_locate_smems_csr(qb, qo, MAX_HITS, 1)),
                ("anchors", anchors, lambda m: lambda q, o, n, *a: ix.dev_anchors(q, o, n, m, 0, *a), lambda: ix.parallel_locate_anchors_csr(qb, qo, MAX_HITS, 1, 0))):
            for min_len in (1, MIN_LEN):
                doff, drows = ar.as_csr([[a for a in full[draw[i]] if a[1] >= min_len] for i in good])
                with max_blocks(bound):
                    got = records_job(ix, dev_qs, int(doff[-1]), launch(min_len))
                assert_records(got, len(dev_qs), good, doff, drows)
            poff, prows = ar.as_csr(full)
            phoff, pg, pp = located(what, lambda: ar.locate_reference(nt.oi, pool, full, 0, MAX_HITS))
            woff, wrows, whoff, wg, wp = gather2(poff, prows, phoff, draw, pg, pp)
            with max_blocks(bound):
                off, rec, hoff, g, p = locate()
            assert np.array_equal(off, woff) and np.array_equal(ar.got_as_rows(rec), wrows), what
            assert np.array_equal(hoff, whoff) and np.array_equal(g, wg) and np.array_equal(p, wp), what
            assert int(hoff[-1]) > 8 * 1024  # tiles of the locate kernel: its blocks draw from the work-queue head again and again
    finally:
        if form == "lf":
            ix.set_verify(2)


# ---- dev_edit_windows, dev_edit_align -----------------------------------------------------------------------------------------------

EDIT_KS = (0, 2, 5, 8)
ALIGN_KS = (0, 2, 4, 5, 8)  # launch_edit_align's half-widths 2, 2, 4, 6, 8: the issue's values, and 4 for the width they leave out
N_EDIT = 1500


@pytest.fixture(scope="module")
def ed():
    w = eg.World(*synth.make_text(20_000, 0, 51, 5, 0.01), 0)
    rng = np.random.default_rng(70)
    q0, _ = eg.planted(w, rng, 101, [("s", 30), ("d", 70)], p=5000)
    q2, _ = eg.planted(w, rng, 200, [("i", 100)], p=12_000)
    q64, _ = eg.planted(w, rng, 64, [("s", 10)], p=3000)
    q65, _ = eg.planted(w, rng, 65, [("d", 20)], p=7000)
    q256, _ = eg.planted(w, rng, 256, [("s", 3), ("i", 128), ("s", 250)], p=9000)
    qs = [q0, bytes(w.text[:40]), q2, b"A" * 12, b"G", q64, q65, q256, bytes(w.text[15_000:15_256])]
    return w, qs


def arrange(base, n, is_a, is_b, mult):
    """n items drawn from `base` in a fixed order; lanes 0 .. 7 of a 256-lane grid take an a, a b, an a, a b; lanes 8 .. 15 a b, ..,
    and one trip of 768 lanes later an a, so that both orders occur at either stride"""
    a, b = [x for x in base if is_a(x)], [x for x in base if is_b(x)]
    assert a and b and np.gcd(mult, len(base)) == 1
    items = [base[(mult * k + 5) % len(base)] for k in range(n)]
    pinned = set()
    for j in range(8):
        for t in range(4):
            items[256 * t + j] = (a, b)[t % 2][j % len((a, b)[t % 2])]
        items[8 + j], items[776 + j] = b[j % len(b)], a[j % len(a)]
        pinned |= {j, 256 + j, 512 + j, 768 + j, 8 + j, 776 + j}
    near = lambda x: [items[y] for y in (x - 768, x - 256, x + 256, x + 768) if 0 <= y < n]
    for x in range(n):  # an item that is not pinned and equals what its lane takes before or after it: the next of the base that does not
        if x not in pinned and items[x] in near(x):
            items[x] = next(c for c in base[x % len(base):] + base if c not in near(x))
    return items


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("k", EDIT_KS)
def test_edit_windows_with_lanes_that_take_several_windows(ed, k, bound):
    w, qs = ed
    n = w.n
    base = [(0, 5000, 1), (0, 4999, 1), (1, 0, n), (3, 0, n), (2, 11_900, 50), (2, 11_950, 60), (2, 12_010, 1), (2, 12_011, 200), (1, 0, 1), (0, n - 1, 5),
            (0, n + 7, 3), (0, 100, 0),                                                       # tests/test_edit_gpu.py's hand-made windows, and:
            (4, 0, n), (4, 100, 300), (5, 2990, 20), (5, 0, n), (6, 6990, 25), (6, n - 70, 70), (7, 8990, 20), (7, 0, n), (7, n - 300, 300), (8, 14_990, 20),
            (8, 15_000, 1)]
    L = lambda win: len(qs[win[0]])
    wins = arrange(base, N_EDIT, lambda x: L(x) == 1, lambda x: L(x) == 256, 7)
    for stride in (256, 768):
        assert_no_lane_repeats(wins, stride)
        pairs = {(L(a), L(b)) for a, b in lane_pairs(wins, stride)}
        assert (1, 256) in pairs and (256, 1) in pairs and {64, 65} <= {x for p in pairs for x in p}, stride
    memo, cols, scanned = {}, 0, 0
    for win in wins:
        qi, first, count = win
        if win not in memo:
            memo[win] = er.hits_of(w.t.D(qs[qi]), k, first, first + count) if len(qs[qi]) > k else (np.zeros(0, np.int64), np.zeros(0, np.uint8))
        cnt = min(first + count, n) - first
        if cnt > 0 and len(qs[qi]) > k:
            a, b = er.scanned(first, cnt, len(qs[qi]), k, n)
            cols += b - a
            scanned += 1
    assert sum(len(memo[x][0]) for x in wins) > 256 and scanned > 768
    with max_blocks(bound):
        n_hits, g, e, t = eg.dev_windows(w, qs, wins, k, tally=True)
    for i, win in enumerate(wins):
        assert int(n_hits[i]) == len(memo[win][0]), (i, win)
    assert np.array_equal(g, np.concatenate([memo[x][0] for x in wins]).astype(np.uint64))
    assert np.array_equal(e, np.concatenate([memo[x][1] for x in wins]))
    assert [int(v) for v in t] == [cols, scanned]


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("k", ALIGN_KS)
def test_edit_align_with_lanes_that_take_several_hits(ed, k, bound):
    w, qs = ed
    n = w.n
    base = []
    for qi in (0, 1, 2, 4, 5, 6, 7, 8):
        if len(qs[qi]) > k:
            p, d = er.hits_of(w.t.D(qs[qi]), k)
            step = max(1, len(p) // 6)
            base += [(qi, int(s), int(x)) for s, x in list(zip(p, d))[::step][:6]]
    true = len(base)
    base += [(0, 4999, min(k, 3)), (0, 7000, k), (1, 300, 0), (3, 100, k), (0, n, k), (1, n + 7, 0), (4, 100, 0), (7, 8990, k), (7, 100, 0), (4, 0, k)]
    base = list(dict.fromkeys(base))
    L = lambda x: len(qs[x[0]])
    if len(base) % 7 == 0:
        base.append((2, 11_000, k))
    triples = arrange(base, N_EDIT, lambda x: L(x) == 1, lambda x: L(x) == 256, 7)
    for stride in (256, 768):
        assert_no_lane_repeats(triples, stride)
        pairs = {(L(a), L(b)) for a, b in lane_pairs(triples, stride)}
        assert (1, 256) in pairs and (256, 1) in pairs, stride
    memo = {x: al.align_triple(w.t, qs[x[0]], x[1], x[2]) if L(x) > k else (0, np.zeros(0, np.uint32)) for x in base}
    assert sum(1 for x in base[:true] if len(memo[x][1])) == true >= 6
    want_aligned = sum(1 for x in triples if len(memo[x][1]))
    assert want_aligned > N_EDIT // 4
    with max_blocks(bound):
        tl, n_ops, ops, t = ag.dev_align(w, qs, triples, k, tally=True)
    aligned = 0
    for h, x in enumerate(triples):
        wtl, wruns = memo[x]
        assert int(tl[h]) == wtl and int(n_ops[h]) == len(wruns), (h, x)
        assert np.array_equal(ops[h, :len(wruns)], wruns), (h, x)
        aligned += len(wruns) > 0
    assert int(t[0]) == aligned == want_aligned


# ---- dev_revcomp, dev_map_select ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bound", BOUNDS)
def test_revcomp_with_groups_that_take_many_reads(nt, bound):
    reads = mg.revcomp_reads(3000, 17)  # (a seed at which no two one- or two-letter reads a group takes in turn are equal)
    reads = reads[1500:] + reads[:1500]  # the empty read in the middle of its group's sequence
    groups = bound * 256 // 16
    assert_no_lane_repeats(reads, groups)
    empty = reads.index(b"")
    trips = len(reads) // groups
    assert trips >= 62 and trips // 4 <= empty // groups <= 3 * trips // 4
    with max_blocks(bound):
        for lead in (0, 13):
            j = mg.revcomp_job(nt.ix, reads, None, lead)
            nt.ix.dev_synchronize()
            mg.assert_revcomp(nt.ix, j, reads)


@pytest.fixture(scope="module")
def select_lists(nt):
    hand = [(mg.strand_lists(c), capped) for _, c, capped, _ in hand_made_lists()]
    lists = hand + mg.random_lists(3000 - len(hand), 3100, len(nt.text) - 1)
    for k in range(len(lists)):  # no lane meets the same lists twice in a row: an equal pair is broken by moving the later one on
        for stride in (256, 768):
            x = k + stride
            while x < len(lists) and lists[x] == lists[k]:
                y = next(y for y in range(x + 1, len(lists)) if lists[y] != lists[k] and (y < stride or lists[y - stride] != lists[x]))
                lists[x], lists[y] = lists[y], lists[x]
    for stride in (256, 768):
        assert_no_lane_repeats(lists, stride)
    return lists, mg.select_inputs(lists), {}


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("A", (1, 3, 8))
def test_map_select_with_lanes_that_take_several_reads(nt, select_lists, A, bound):
    lists, inp, _ = select_lists
    for R in sorted({1, A, 2 * A}):
        with max_blocks(bound):
            got = mg.select_on_device(nt.ix, inp, A, R)
        mg.assert_select(got, inp, A, R, nt.st, (A, R, bound))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def e2e_reads(nt):
    """the `main` reads of tests/test_map_gpu.py and the `e2e` queries of tests/test_chain_align_gpu.py, as those modules make them.
    Their references are this module's own (a module's fixtures cannot be taken from another), through the oracle's counts and
    memoised per query, which takes a second or two for the few hundred reads: the sets are not cut."""
    reads = [r[0] for r in fixture_reads(nt.text)] + [q for q in edge_queries(nt) if len(q) <= 1024]
    qs = [q for q in nt_queries(nt, (6, nt.ix.seed_kmer_len())) + edge_queries(nt) if len(q) <= 1024] + [r[0] for r in cag.edited_reads(nt.text)]
    assert max(len(q) for q in reads) >= 1000 and max(len(q) for q in qs) >= 1000
    return reads, qs, {}, {}


def e2e_checks(nt, reads, qs, memo, amemo):
    qb, qo = pack_queries(reads)
    want = mg.want_maps(nt, reads, 3, 6, 4, P_MAIN, memo)
    cqb, cqo = pack_queries(qs)
    per = nt.chains_of(P_MAIN)(qs)
    walign = cag.want_alignments(nt.tsym, qs, per, 3, 4, amemo)
    doubled = nt.chains_of(P_MAIN)(mp.doubled(reads))
    # Under max_blocks(1): the map call's 2 x len(reads) queries wrap the SMEM kernel (more than 256), its chains the chaining groups
    # (16 or 4 a block) and its aligned chains the alignment lanes; the reads themselves are fewer than 256, so map_select and
    # map_gather take one read per lane.  The chain-align and chain calls wrap in queries, chains and aligned chains.  Under
    # max_blocks(3) only the chaining groups (48 or 12) and strand_expand's (48) take several items; the sets are the modules' own.
    assert 2 * len(reads) > 256 > len(reads) > 3 * 256 // 16 and sum(min(len(c), 3) for _, c in doubled) > 256 and int(want[0][-1]) > len(reads) // 2
    assert len(qs) > 256 and int(walign[0][-1]) > 256 and sum(len(c) for _, c in per) > 256
    yield "map", lambda: mg.assert_maps_equal(nt.ix.parallel_map_csr(qb, qo, *KEY, 3, 6, 4, *P_MAIN), want, nt.st, "map")
    yield "align chains", lambda: cag.assert_batch_equals(nt.ix.parallel_align_chains_csr(cqb, cqo, *KEY, 3, 4, *P_MAIN), walign)
    yield "chains", lambda: cg.assert_batch_equals(nt.ix.parallel_chains_csr(cqb, cqo, *KEY, *P_MAIN), per)


@pytest.mark.parametrize("bound", BOUNDS)
def test_map_align_chains_and_chains_end_to_end_under_the_bound(nt, e2e_reads, bound):
    reads, qs, memo, amemo = e2e_reads
    for name, call in e2e_checks(nt, reads, qs, memo, amemo):
        with max_blocks(bound):
            call()


@pytest.mark.parametrize("bound", BOUNDS)
def test_sub_batches_and_the_halving_fallback_under_the_bound(nt, e2e_reads, bound):
    reads, qs, memo, amemo = e2e_reads
    os.environ["AWRY_CHAIN_ALIGN_SUB_BATCH"] = "7"
    os.environ["AWRY_ANCHOR_HIT_CAP"] = "64"
    try:
        for name, call in e2e_checks(nt, reads, qs, memo, amemo):
            with max_blocks(bound):
                call()
    finally:
        del os.environ["AWRY_CHAIN_ALIGN_SUB_BATCH"], os.environ["AWRY_ANCHOR_HIT_CAP"]


N_EDIT_READS = 47 * 13


@pytest.fixture(scope="module")
def edit_batch(ed):
    """the reads of tests/test_edit_gpu.py's test_mixed_lengths_in_one_call (12 lengths from 3 to 256 letters, k = 2), the first 47
    of its 48 in its order -- 47 is prime, so no stride below repeats a read -- tiled to 611, with the reference computed once per
    distinct read and gathered"""
    w, _ = ed
    k = 2
    rng = np.random.default_rng(7)
    qs = []
    for L in (3, 6, 20, 63, 64, 65, 101, 128, 129, 192, 193, 256):
        qs += eg.reads_for(w, rng, L, 2)[0][:4]
    pool = [qs[i] for i in rng.permutation(len(qs))][:47]
    assert len(set(pool)) == 47 and {(len(q) + 63) // 64 for q in pool} == {1, 2, 3, 4}
    draw = np.arange(N_EDIT_READS, dtype=np.int64) % 47
    # lanes take reads (strides 256, 768), pieces (k + 1 a read: 85 or 86 and 256 reads apart) and windows and hits of reads further on
    for stride in (256, 768, 85, 86):
        assert stride % 47 and (stride + 1) % 47
        assert_no_lane_repeats(list(draw), stride)
    off, g, d, st, tl, coff, cg = al.align(w.t, pool, k, eg.NO_CAP)
    assert not st.any()
    boff, bg, bd, btl, bruns = gather(off, draw, g, d, tl, np.diff(coff.astype(np.int64)))
    bcoff = np.zeros(len(bg) + 1, np.uint64)
    bcoff[1:] = np.cumsum(bruns)
    _, bcg = gather(coff[off.astype(np.int64)], draw, cg)
    # every kernel of the two drivers wraps at both bounds: pieces, candidates (at least one per hit), windows' hits, hits
    assert (k + 1) * N_EDIT_READS > 768 and len(bg) > 768 and N_EDIT_READS < 768
    assert len(bcg) == int(bcoff[-1])
    return [pool[i] for i in draw], k, (boff, bg, bd, btl, bcoff, bcg)


@pytest.mark.parametrize("bound", BOUNDS)
def test_edit_locate_and_edit_align_end_to_end_under_the_bound(ed, edit_batch, bound):
    w, _ = ed
    qs, k, (woff, wg, wd, wtl, wcoff, wcg) = edit_batch
    qb, qo = pack_queries(qs)
    with max_blocks(bound):
        off, g, p, d, st = w.ix.parallel_locate_edit_csr(qb, qo, k, eg.NO_CAP)
        got = w.ix.parallel_align_edit_csr(qb, qo, k, eg.NO_CAP)
    assert not st.any() and np.array_equal(off, woff) and np.array_equal(g, wg) and np.array_equal(d, wd)
    rec = np.searchsorted(w.st, g, side="right") - 1
    assert np.array_equal(p[:, 0], rec.astype(np.uint64)) and np.array_equal(p[:, 1], g - w.st[rec])
    assert ag.same(got[:5], (off, g, p, d, st))
    bad = np.nonzero(got[5] != wtl)[0]
    assert not len(bad), ("read", int(np.searchsorted(woff, bad[0], side="right")) - 1, int(got[5][bad[0]]), int(wtl[bad[0]]))
    assert np.array_equal(got[6], wcoff) and np.array_equal(got[7], wcg)


# ---- the real geometry --------------------------------------------------------------------------------------------------------------

def test_map_at_one_grid_and_a_bit(nt):
    import torch
    t0 = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * 8 * 256  # 8 x 256 threads is the most a CU holds, and grid_for's bound
    n = grid + 4096
    rng = np.random.default_rng(251)
    src = [r[0] for r in fixture_reads(nt.text)]
    pool = []
    for j in range(251):  # 251 is prime: a lane's reads j, j + stride, .. differ whatever the stride below 251 x anything
        q = src[j % len(src)]
        L = 40 + (j * 5) % 62
        at = int(rng.integers(0, len(q) - L + 1))
        pool.append(q[at:at + L])
    assert len(set(pool)) == 251 and min(len(q) for q in pool) >= 40 and max(len(q) for q in pool) == 101
    draw = np.arange(n, dtype=np.int64) % 251
    for stride in (grid, 2 * grid, grid // 16, grid // 8, grid // 4, grid // 2):
        assert stride % 251 != 0
    A, R, W = 3, 6, 4
    poff, prec, pcoff, pcg, pst = mg.want_maps(nt, pool, A, R, W, P_MAIN, {})
    woff, wrec, wcoff, wcg = gather2(poff, prec, pcoff, draw, pcg)
    per = nt.chains_of(P_MAIN)(mp.doubled(pool))
    cand = np.array([min(len(per[2 * i][1]), A) + min(len(per[2 * i + 1][1]), A) for i in range(251)], np.int64)
    aligned = int(cand[draw].sum())
    assert aligned > 1 << 18 and aligned > grid, aligned  # the default sub-batch is crossed, and every kernel's grid
    qo, qb = gather(pack_queries(pool)[1], draw, pack_queries(pool)[0])
    t1 = time.time()
    got = nt.ix.parallel_map_csr(qb, qo, *KEY, A, R, W, *P_MAIN)
    t2 = time.time()
    mg.assert_maps_equal(got, (woff, wrec, wcoff, wcg, pst[draw]), nt.st, "one grid and a bit")
    print("n = %d reads, %d aligned candidates, %d records: reference and batch %.1f s, the call %.1f s, comparison %.1f s"
          % (n, aligned, len(got[1]), t1 - t0, t2 - t1, time.time() - t2))
