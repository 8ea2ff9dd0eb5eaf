"""References for class-pattern search (IUPAC / residue classes with <= k mismatches, include/awry_hip.h):

(a) class_table: the letter -> class table, written out here independently of alphabet.h;
(b) brute_force: the definition itself -- sliding windows over the text as symbol indices, a position mismatches when the
    text symbol is outside the pattern letter's class, windows holding '$' excluded;
(c) ordered_hits: the promised order -- the distinct matched window strings in symbol-index order, each located by the oracle
    (the exact-match checker under oracle/);
(d) expand: every concrete string of a pattern, for the k = 0 cross-check against the oracle's exact counts.

Text bytes map to symbol indices the way the exact path maps them (tests/mismatch_ref.py)."""
import itertools

import numpy as np

from tests import mismatch_ref as mr

NT_CLASSES = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
              "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
AA_STANDARD = "ACDEFGHIKLMNPQRSTVWY"
AA_CLASSES = dict({c: c for c in AA_STANDARD}, B="DN", Z="EQ", J="IL", X=AA_STANDARD)
MAX_CLASS_POSITIONS = 16


def class_table(alphabet):
    """uint32[256]: byte -> class mask (bit s = symbol index s), 0 for a byte that is no class letter"""
    classes = NT_CLASSES if alphabet == 0 else AA_CLASSES
    letters = mr.letters(alphabet).decode()
    tab = np.zeros(256, np.uint32)
    for b in range(128):
        members = classes.get(chr(b).upper())
        if members and chr(b).isalpha():
            tab[b] = sum(1 << letters.index(m) for m in members)
    return tab


def class_positions(pattern, alphabet):
    m = class_table(alphabet)[np.frombuffer(bytes(pattern), np.uint8)]
    return int(((m & (m - 1)) != 0).sum())


def window_dist(tsym, pattern, alphabet):
    """distance of every window of the text (symbol indices) from the pattern; -1 where the window holds '$'"""
    cls = class_table(alphabet)[np.frombuffer(bytes(pattern), np.uint8)]
    assert len(cls) and (cls != 0).all(), "not a pattern"
    L, n = len(cls), len(tsym)
    W = max(0, n - L + 1)
    dist = np.zeros(W, np.int32)
    sent = np.zeros(W, bool)
    for j in range(L):
        w = tsym[j:j + W]
        dist += ((cls[j] >> w.astype(np.uint32)) & 1) == 0
        sent |= w == 0
    dist[sent] = -1
    return dist


def brute_force(text, pattern, k, alphabet=0):
    """-> (counts uint64[k + 1] at exactly 0..k mismatches, positions int64[], distances uint8[]) sorted by position"""
    dist = window_dist(mr.to_symbols(text, alphabet), pattern, alphabet)
    pos = np.nonzero((dist >= 0) & (dist <= k))[0]
    d = dist[pos].astype(np.uint8)
    return np.bincount(d, minlength=k + 1)[:k + 1].astype(np.uint64), pos.astype(np.int64), d


def ordered_hits(oi, text, pattern, k, alphabet=0):
    """-> (global positions uint64[], (record, offset) uint64[, 2], distances uint8[]) in the promised order: the distinct
    matched window strings sorted by symbol index (byte order of the canonical letters), the oracle's locate list of each"""
    _, pos, d = brute_force(text, pattern, k, alphabet)
    L = len(pattern)
    if len(pos) == 0:
        return np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64), np.zeros(0, np.uint8)
    lt = np.frombuffer(mr.letters(alphabet), np.uint8)
    win = lt[mr.to_symbols(text, alphabet)[pos[:, None] + np.arange(L)[None, :]]]
    keys = np.ascontiguousarray(win).view("S%d" % L).ravel()
    uniq, first = np.unique(keys, return_index=True)  # sorted as bytes
    qb = np.ascontiguousarray(win[first]).reshape(-1)
    qo = np.arange(len(uniq) + 1, dtype=np.uint64) * np.uint64(L)
    off, g, p, _ = oi.parallel_locate(qb, qo, 4)
    dist = np.repeat(d[first], np.diff(off.astype(np.int64))).astype(np.uint8)
    return g.astype(np.uint64), p, dist


def expand(pattern, alphabet=0):
    """every concrete string of the pattern, as canonical letters"""
    classes = NT_CLASSES if alphabet == 0 else AA_CLASSES
    return [("".join(s)).encode() for s in itertools.product(*[classes[chr(b).upper()] for b in bytes(pattern)])]


def replace_with_classes(window, positions, hold, alphabet, rng, narrowest=False):
    """the window (canonical letters, no ambiguity symbol at `positions`) with a class letter at each of `positions`: one that
    holds the text's letter there where hold[i], else one that does not; narrowest: only the smallest such classes are drawn"""
    classes = NT_CLASSES if alphabet == 0 else AA_CLASSES
    multi = sorted(c for c, m in classes.items() if len(m) > 1)
    q = bytearray(window)
    for j, h in zip(positions, hold):
        x = chr(q[j]).upper()
        x = "T" if alphabet == 0 and x == "U" else x
        pick = [c for c in multi if (x in classes[c]) == bool(h)]
        assert pick, (x, h)
        if narrowest:
            pick = [c for c in pick if len(classes[c]) == min(len(classes[d]) for d in pick)]
        q[j] = ord(pick[int(rng.integers(0, len(pick)))])
    return bytes(q)
