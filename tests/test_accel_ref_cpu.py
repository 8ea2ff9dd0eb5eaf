"""The host recomputation of the device-only accelerators (tests/accel_ref.py) checked against the definition: every seed entry
against the oracle's range of its k-mer, every BWT symbol, context and symbol mask against plain slicing of the text, and the
hand-made edge cases the GPU audit (tests/test_accel_audit_gpu.py) relies on it for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import awry_amd
from awry_amd import _lib
from awry_amd.fm_index import BUILD_HOST, FmIndex
from tests import accel_ref as ar
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_debug_accelerators", "awry_debug_seed_rung", "awry_debug_set_ctx_extra_cap", "awry_debug_dense_sa")
NT_LETTERS, AA_LETTERS = "ACGT", "ACDEFGHIKLMNPQRSTVWYX"       # table digit -> letter
NT_INDEX = {"$": 0, "A": 1, "C": 2, "G": 3, "N": 4, "T": 5}
AA_INDEX = {c: i for i, c in enumerate("$ACDEFGHIKLMNPQRSTVWXY")}


def entry_index(kmer, letters):
    return sum(letters.index(c) * len(letters) ** t for t, c in enumerate(kmer))


def all_kmers(k, letters):
    out = [""]
    for _ in range(k):
        out = [w + c for c in letters for w in out]  # the first letter varies fastest: out[o] is the k-mer of entry o
    return out


def world(alphabet):
    if alphabet == 0:
        text, st, hd = synth.make_text(300, 0, 17, 2, 0.04)
    else:
        text, st, hd = synth.make_text(400, 1, 18, 3, 0.03)
    return text, st, hd, ar.AccelRef(text, st, alphabet), bytes(text).decode()


@pytest.fixture(scope="module")
def nt():
    return world(0)


@pytest.fixture(scope="module")
def aa():
    return world(1)


def test_the_suffix_arrays_agree(oracle, nt, aa):
    for text, st, hd, ref, s in (nt, aa):
        assert np.array_equal(ref.sa, oracle.suffix_array(text).astype(np.int64))
        assert np.array_equal(ar.numpy_suffix_array(text), ref.sa)
        assert all(s[a:] < s[b:] for a, b in zip(ref.sa[:-1].tolist(), ref.sa[1:].tolist()))  # '$' is the smallest byte of a text


@pytest.mark.parametrize("alphabet", [0, 1])
def test_every_entry_is_the_oracle_s_range(oracle, nt, aa, alphabet):
    text, st, hd, ref, s = (nt, aa)[alphabet]
    oi = oracle.OracleIndex.from_text(text, alphabet, 8, 0, st, hd)
    letters = (NT_LETTERS, AA_LETTERS)[alphabet]
    for k in ((1, 2, 3, 4), (1, 2))[alphabet]:
        T = ref.table(k)
        kmers = all_kmers(k, letters)
        assert len(kmers) == len(T.entries) and all(entry_index(w, letters) == o for o, w in list(enumerate(kmers))[::7])
        present = 0
        for o, w in enumerate(kmers):
            lo, hi = oi.search_range(w)
            cnt = oi.count_string(w)
            assert cnt == max(0, hi - lo + 1) == int(T.rows[o]) == len(occurrences(s, w)), (k, w)
            assert bool(T.defined[o]) == (cnt > 0)
            if cnt:
                assert int(T.first_row[o]) == lo, (k, w)
                assert int(T.entries["sp"][o]) == lo
                present += 1
            plain = cnt == 0 or (cnt >= 2 if alphabet == 0 else cnt >= 5)
            if plain:
                assert int(T.entries["cnt"][o]) == cnt, (k, w)
        assert present > len(kmers) // 50
    oi.close()


def occurrences(s, w):
    return [i for i in range(len(s) - len(w) + 1) if s[i:i + len(w)] == w]


def nt_entry_by_slicing(s, sa, w, seed_pos, extra, lcx):
    """(sp or None, cnt) of the nucleotide entry of k-mer w, from slices of the text s (and the suffix array for rows)"""
    occ = occurrences(s, w)
    if not occ:
        return None, 0
    rows = sorted(int(np.flatnonzero(sa == p)[0]) for p in occ)
    assert rows == list(range(rows[0], rows[0] + len(rows)))
    if len(occ) >= 2:
        tail = lcx and any(p < 32 or set(s[p - 32:p]) - set("ACGT") for p in occ)
        return rows[0], len(occ) | (ar.SEED_LCX_TAIL if tail else 0)
    p = occ[0]
    sym = NT_INDEX[s[p - 1]]  # (p = 0: s[-1] is the '$')
    if not seed_pos:
        return rows[0], 1 | sym << 29
    clen = 14 + extra
    ctx = s[p - clen:p] if p >= clen else ""
    if len(ctx) < clen or set(ctx) - set("ACGT"):
        return p, 1 | sym << 29
    full = sum("ACGT".index(c) << (2 * j) for j, c in enumerate(ctx))
    return p | (full & (4 ** extra - 1)) << (32 - 2 * extra), sym << 29 | ar.SEED_CTX | full >> (2 * extra)


def aa_entry_by_slicing(s, sa, w, seed_pos):
    occ = occurrences(s, w)
    if not occ:
        return None, 0
    rows = sorted(int(np.flatnonzero(sa == p)[0]) for p in occ)
    assert rows == list(range(rows[0], rows[0] + len(rows)))
    syms = [AA_INDEX[s[p - 1]] for p in occ]
    if len(occ) >= 5:
        return rows[0], len(occ)
    if len(occ) >= 2:
        mask = 0
        for x in syms:
            mask |= 1 << x
        return rows[0], ar.AA_SEED_SPECIAL | ar.AA_SEED_MULTI | (len(occ) - 2) << 22 | mask
    p = occ[0]
    if not seed_pos:
        return rows[0], 1 | syms[0] << 27
    if p < 6:
        return p, 1 | syms[0] << 27
    return p, syms[0] << 27 | ar.AA_SEED_SPECIAL | sum(AA_INDEX[s[p - 2 - j]] << (5 * j) for j in range(5))


@pytest.mark.parametrize("seed_pos,extra,lcx", [(False, 0, False), (True, 0, False), (True, 2, False), (True, 3, False), (True, 9, False)])
def test_nucleotide_symbols_and_contexts_are_slices_of_the_text(nt, seed_pos, extra, lcx):
    text, st, hd, ref, s = nt
    seen = {"ctx": 0, "noctx": 0, "multi": 0}
    for k in (1, 2, 3, 4):
        T = ref.table(k, seed_pos, extra, lcx)
        for o, w in enumerate(all_kmers(k, NT_LETTERS)):
            sp, cnt = nt_entry_by_slicing(s, ref.sa, w, seed_pos, extra, lcx)
            assert int(T.entries["cnt"][o]) == cnt, (k, w)
            if sp is not None:
                assert int(T.entries["sp"][o]) == sp, (k, w)
            seen["multi"] += cnt >= 2 and not cnt & ar.SEED_CTX
            seen["ctx"] += bool(cnt & ar.SEED_CTX)
            seen["noctx"] += sp is not None and cnt & ar.SEED_CNT_SAT == 1 and not cnt & ar.SEED_CTX
    assert seen["multi"] > 50 and seen["noctx"] >= 1 and (not seed_pos or seen["ctx"] >= 10), seen


def test_tail_flags_are_slices_of_the_text():
    """buckets of 2+ rows with the left-context index resident (k >= 8 there; a text of two planted 8-mers here)"""
    rng = np.random.default_rng(3)
    body = synth.NT[rng.integers(0, 4, size=400, dtype=np.uint8)]
    for at in (3, 90, 200, 310):
        body[at:at + 8] = np.frombuffer(b"ACGTTGCA", np.uint8)  # four copies: one within 32 letters of the text's start
    for at in (50, 150, 250):
        body[at:at + 8] = np.frombuffer(b"GGATCCAA", np.uint8)  # three copies, all with 32 ACGT letters in front
    for at in (120, 350):
        body[at:at + 8] = np.frombuffer(b"TTTTCCCC", np.uint8)  # two copies, one behind an N
    body[340] = ord("N")
    text = np.concatenate([body, np.frombuffer(b"$", np.uint8)])
    s = bytes(text).decode()
    ref = ar.AccelRef(text, [0], 0)
    T = ref.table(8, True, 5, True)
    for w, tail in (("ACGTTGCA", True), ("GGATCCAA", False), ("TTTTCCCC", True)):
        o = entry_index(w, NT_LETTERS)
        sp, cnt = nt_entry_by_slicing(s, ref.sa, w, True, 5, True)
        assert (int(T.entries["sp"][o]), int(T.entries["cnt"][o])) == (sp, cnt) and bool(cnt & ar.SEED_LCX_TAIL) == tail == bool(T.tail[o]), w
    assert not (T.entries["cnt"][T.rows >= 2] & np.uint32(ar.SEED_LCX_NONE)).any()
    flagged = np.flatnonzero((T.rows >= 2) & ((T.entries["cnt"] & np.uint32(ar.SEED_LCX_TAIL)) != 0))
    want = [o for o in np.flatnonzero(T.rows >= 2).tolist() if nt_entry_by_slicing(s, ref.sa, ref.kmer_of(8, o), True, 5, True)[1] & ar.SEED_LCX_TAIL]
    assert flagged.tolist() == want
    off = ref.table(8, True, 5, False)
    assert not (off.entries["cnt"][off.rows >= 2] >> np.uint32(29)).any()


@pytest.mark.parametrize("seed_pos", [False, True])
def test_amino_symbols_contexts_and_masks_are_slices_of_the_text(aa, seed_pos):
    text, st, hd, ref, s = aa
    kinds = set()
    for k in (1, 2):
        T = ref.table(k, seed_pos)
        for o, w in enumerate(all_kmers(k, AA_LETTERS)):
            sp, cnt = aa_entry_by_slicing(s, ref.sa, w, seed_pos)
            assert int(T.entries["cnt"][o]) == cnt, (k, w)
            if sp is not None:
                assert int(T.entries["sp"][o]) == sp, (k, w)
                kinds.add(min(len(occurrences(s, w)), 5))
                if "X" in w:
                    kinds.add("X")
    assert kinds == {1, 2, 3, 4, 5, "X"}


# ---- hand-made cases ------------------------------------------------------------------------------------------------------
def nt_entry(s, k, w, seed_pos=True, extra=0, starts=(0,)):
    text = np.frombuffer(s.encode(), np.uint8)
    T = ar.AccelRef(text, list(starts), 0, ar.numpy_suffix_array(text)).table(k, seed_pos, extra)
    o = entry_index(w, NT_LETTERS)
    return int(T.entries["sp"][o]), int(T.entries["cnt"][o])


def test_an_occurrence_at_clen_minus_one_has_no_context():
    assert nt_entry("A" * 13 + "CGTTC$", 4, "CGTT") == (13, 1 | 1 << 29)  # p = 13 < 14; in front of it an A


def test_an_occurrence_at_clen_has_its_context():
    assert nt_entry("A" * 13 + "CGTTC$", 4, "GTTC") == (14, 2 << 29 | ar.SEED_CTX | 1 << 26)  # context A x 13, then C at j = 13


def test_a_context_whose_far_end_is_an_n_is_none():
    assert nt_entry("N" + "A" * 12 + "CGTTC$", 4, "GTTC") == (14, 1 | 2 << 29)


def test_a_context_that_starts_right_behind_an_n_is_kept():
    assert nt_entry("N" + "A" * 13 + "CGTTC$", 4, "GTTC") == (15, 2 << 29 | ar.SEED_CTX | 1 << 26)


def test_a_context_that_crosses_a_record_join_is_none():
    # records ACGTAC and AAAAAAAAAACGTTC joined by the delimiter N: the 14 letters in front of GTTC (p = 18) start at 4
    assert nt_entry("ACGTAC" + "N" + "A" * 10 + "CGTTC$", 4, "GTTC", starts=(0, 7)) == (18, 1 | 2 << 29)


@pytest.mark.parametrize("extra", [0, 2, 3, 9])
def test_the_context_is_split_between_cnt_and_the_top_of_sp(extra):
    front = "GATTACAGATTACACCGTAGCTAGCA"  # 26 letters, then the singleton TTTT at p = 26, an A in front of it
    s = front + "TTTT" + "$"
    clen = 14 + extra
    full = sum("ACGT".index(c) << (2 * j) for j, c in enumerate(front[26 - clen:]))
    assert nt_entry(s, 4, "TTTT", True, extra) == (26 | (full & (4 ** extra - 1)) << (32 - 2 * extra), NT_INDEX["A"] << 29 | ar.SEED_CTX | full >> (2 * extra))


AA_BUCKETS = "AMKCMKDMKEMKFMK" + "GWYHWYGWYHWY" + "IQRLQR" + "$"


def aa_entry(w, seed_pos=False):
    text = np.frombuffer(AA_BUCKETS.encode(), np.uint8)
    ref = ar.AccelRef(text, [0], 1, ar.numpy_suffix_array(text))
    T = ref.table(2, seed_pos)
    o = entry_index(w, AA_LETTERS)
    return int(T.first_row[o]) == int(T.entries["sp"][o]), int(T.entries["cnt"][o])


def test_an_amino_bucket_of_exactly_two_rows_is_a_mask():
    assert aa_entry("QR") == (True, ar.AA_SEED_SPECIAL | ar.AA_SEED_MULTI | 0 << 22 | 1 << AA_INDEX["I"] | 1 << AA_INDEX["L"])


def test_an_amino_bucket_of_exactly_four_rows_is_a_mask():
    assert aa_entry("WY", True) == (True, ar.AA_SEED_SPECIAL | ar.AA_SEED_MULTI | 2 << 22 | 1 << AA_INDEX["G"] | 1 << AA_INDEX["H"])


def test_an_amino_bucket_of_exactly_five_rows_is_plain():
    assert aa_entry("MK", True) == (True, 5)


# ---- the other structures -------------------------------------------------------------------------------------------------
def test_expected_ctx_extra_follows_the_bits_per_element_rule(oracle):
    for n in (2, 3, 257, 5_401, 20_001, 90_001, 600_001, 1 << 20, (1 << 20) + 1, 248_956_423, 3_099_750_719, (1 << 32) - 513):
        assert ar.sa_bits(n) == int(oracle.lib().orc_csa_bits_per_element(n)), n
    assert [ar.expected_ctx_extra(n) for n in (5_401, 20_001, 90_001, 600_001, 248_956_423, 3_099_750_719)] == [9, 8, 7, 6, 2, 0]
    assert [ar.expected_ctx_extra(5_401, cap) for cap in (0, 1, 2, 3, 12, -1)] == [0, 1, 2, 3, 9, 9]
    assert ar.expected_ctx_extra(3) == 15


def test_text_codes_sa_samples_and_the_n_block_are_the_text_s(oracle, nt, aa):
    L = awry_amd.load_library()
    for alphabet, (text, st, hd, ref, s) in enumerate((nt, aa)):
        want8 = [int(L.awry_symbol_index(alphabet, ord(c))) for c in s]
        assert ref.text8().tolist() == want8 == [int(oracle.lib().orc_ascii_to_index(alphabet, ord(c))) for c in s] and want8[-1] == 0
        assert ref.bwt.tolist() == [want8[p - 1] for p in ref.sa.tolist()]
        for ratio in (1, 2, 3, 5, 8):
            assert ref.dense_sa(ratio).tolist() == [int(ref.sa[j * ratio]) for j in range((len(s) + ratio - 1) // ratio)]
    text, st, hd, ref, s = nt
    t4 = ref.text4()
    assert len(t4) == (len(s) + 7) // 8 + 8
    nib = [(int(t4[p >> 3]) >> (4 * (p & 7))) & 15 for p in range(8 * len(t4))]
    assert nib[:len(s)] == [{"A": 0, "C": 1, "G": 2, "T": 3}.get(c, 8) for c in s] and not any(nib[len(s):])
    lo, hi = ref.nblock_window()
    rows_n = [r for r, p in enumerate(ref.sa.tolist()) if s[p] == "N"]
    assert rows_n == list(range(lo, hi)) and hi - lo == s.count("N") >= 3
    assert ref.sa_nblock().tolist() == [int(ref.sa[r]) for r in rows_n]


def test_the_sampled_levels_take_every_sixteenth_key(nt):
    ref = nt[3]
    keys = np.arange(1000, 1000 + ref.n, dtype=np.uint64)
    levels, total = ref.lcx_levels()
    assert levels[1][0] == 16 and total == levels[7][0] + levels[7][1]
    for t in range(1, 8):
        lev = ref.lcx_inner_level(keys, t)
        assert len(lev) == levels[t][1] and len(lev) % 16 == 0 and len(lev) >= ((ref.n - 1) >> (4 * t)) + 1 + 16
        assert lev.tolist() == [1000 + (j << (4 * t)) if (j << (4 * t)) < ref.n else 0 for j in range(len(lev))]
        if t < 7:
            assert levels[t + 1][0] == levels[t][0] + levels[t][1]


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree():
    L = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "awry-hip-sys", "src", "lib.rs")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name).argtypes is not None, name
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(getattr(L, name).argtypes), name
        assert "pub fn %s(" % name in rust, name
    # the struct: the header's fields in order, with ctypes' and Rust's
    body = re.search(r"typedef struct \{([^}]*)\} awry_debug_accel_t;", src).group(1)
    c_fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind = re.match(r"(const void \*|int32_t|uint64_t|uint32_t)", decl).group(1)
            c_fields += [(re.sub(r"\[\d+\]", "", nm.strip()), kind, "[" in nm) for nm in decl[len(kind):].split(",")]
    ctype_of = {"const void *": C.c_void_p, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    rust_of = {"const void *": "*const c_void", "int32_t": "i32", "uint64_t": "u64", "uint32_t": "u32"}
    assert [n for n, _, _ in c_fields] == [n for n, _ in _lib.DebugAccel._fields_]
    rbody = re.search(r"pub struct awry_debug_accel_t \{([^}]*)\}", rust).group(1)
    r_fields = [tuple(x.strip() for x in ln.strip().rstrip(",")[4:].split(":")) for ln in rbody.strip().splitlines()]
    for (name, kind, arr), (pn, pt), (rn, rt) in zip(c_fields, _lib.DebugAccel._fields_, r_fields):
        assert name == pn == rn
        assert pt == (ctype_of[kind] * 8 if arr else ctype_of[kind]), name
        assert rt == ("[%s; 8]" % rust_of[kind] if arr else rust_of[kind]), name
    assert len(r_fields) == len(c_fields) and C.sizeof(_lib.DebugAccel) == 136
    # without replicas: an argument error, no pointer; the cap takes -1 and up
    ix = FmIndex.from_text(b"ACGTACGT$", 0, 8, 0, [0], ["one"], build_device=BUILD_HOST)
    a = _lib.DebugAccel()
    assert L.awry_debug_accelerators(ix._h, 0, C.byref(a)) == -6 and not L.awry_debug_dense_sa(ix._h, 0)
    assert not L.awry_debug_seed_rung(ix._h, 0, 8)
    assert L.awry_debug_set_ctx_extra_cap(-2) == -6 and L.awry_debug_set_ctx_extra_cap(3) == 0 and L.awry_debug_set_ctx_extra_cap(-1) == 0
    ix.close()
