"""Host recomputation of the device-only accelerators (awry_amd/csrc/layout.h, accelerators.h), from the text alone: the seed
table in all its encodings, the dense SA, the text as 4-bit and 8-bit codes, the SA of the N block and the sampled levels of
the left-context index.  Pure numpy over the text and its suffix array; no device code and none of the library's decoders.

Conventions (layout.h): symbol indices $0 A1 C2 G3 N4 T5 (nucleotide) and $0 A..W 1..19 X20 Y21 (amino; every other byte is the
ambiguity symbol N / X).  Seed entry o of a k-mer w_0 .. w_{k-1} is sum_t d(w_t) sigma^t -- the FIRST letter least significant --
with d = A0 C1 G2 T3 (sigma 4) or A..W 0..18, Y 19, X 20 (sigma 21).  An entry whose k-mer does not occur has cnt 0 and an
UNSPECIFIED sp (the builder leaves its parent's there): Table.defined is False for it and only cnt is compared."""
import ctypes as C

import numpy as np

NUCLEOTIDE, AMINO = 0, 1
SEED_CTX, SEED_CTX_LEN, SEED_CNT_SAT = 0x10000000, 14, 0x0FFFFFFF
SEED_LCX_TAIL, SEED_LCX_NONE = 0x20000000, 0x40000000
AA_SEED_SPECIAL, AA_SEED_MULTI, AA_SEED_CTX_LEN, AA_SIGMA = 0x04000000, 0x02000000, 6, 21
LCX_CTX = 32
ENTRY32 = np.dtype([("sp", np.uint32), ("cnt", np.uint32)])
ENTRY64 = np.dtype([("sp", np.uint64), ("cnt", np.uint64)])

NT_SYM = np.full(256, 4, np.uint8)           # byte -> symbol index
NT_SYM[[36, 65, 67, 71, 84]] = [0, 1, 2, 3, 5]
AA_SYM = np.full(256, 20, np.uint8)
AA_SYM[36] = 0
AA_SYM[np.frombuffer(b"ACDEFGHIKLMNPQRSTVW", np.uint8)] = np.arange(1, 20)
AA_SYM[ord("Y")] = 21
NT_DIGIT = np.array([8, 0, 1, 2, 8, 3], np.uint8)                                      # symbol index -> table digit (8: none)
AA_DIGIT = np.array([255] + list(range(19)) + [20, 19], np.uint8)                      # ('$' is in no window)


def host_suffix_array(text):
    """the suffix array of a text that ends in '$', by the library's HOST suffix sorter (no device)"""
    from awry_amd import _lib
    L = _lib.load_library()
    t = np.ascontiguousarray(text, np.uint8)
    sa = np.zeros(len(t), dtype=np.uint64)
    assert L.awry_host_suffix_array(t.ctypes.data, len(t), sa.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    return sa.astype(np.int64)


def numpy_suffix_array(text):
    """prefix doubling; bytes compare as such ('$' < letters, and byte order is symbol-index order for canonical texts)"""
    t = np.ascontiguousarray(text, np.uint8).astype(np.int64)
    n = len(t)
    rank, h = t.copy(), 1
    while True:
        nxt = np.full(n, -1, np.int64)
        nxt[:n - h] = rank[h:] if h < n else 0
        order = np.lexsort((nxt, rank))
        key = rank[order] * (n + 257) + nxt[order] + 1
        new = np.zeros(n, np.int64)
        new[order] = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank = new
        if rank.max() == n - 1:
            return np.argsort(rank).astype(np.int64)
        h *= 2


def sa_bits(bwt_len):
    """bits per element of the sampled suffix array: those of the largest value, bwt_len - 1"""
    return int(bwt_len - 1).bit_length()


def expected_ctx_extra(bwt_len, cap=-1):
    """E: the context letters of a position seed beyond 14, kept in the bits of sp that no position of the text uses"""
    e = min(15, (32 - min(32, sa_bits(bwt_len))) // 2)
    return e if cap < 0 else min(e, cap)


class Table:
    """expected seed table: .entries (ENTRY32 or ENTRY64, sp of undefined entries 0), .defined, and per entry what the
    condition asserts of the tests count: .rows (occurrences), .pos (text position of a singleton, else -1), .has_ctx, .tail"""

    def differences(self, got):
        """indices of the entries of `got` that differ from the expectation where it is defined"""
        bad = got["cnt"] != self.entries["cnt"]
        bad |= self.defined & (got["sp"] != self.entries["sp"])
        return np.flatnonzero(bad)

    def masked(self, got):
        """`got` with the sp of undefined entries zeroed, as .entries has it: np.array_equal(masked(got), entries) is the audit"""
        out = got.copy()
        out["sp"][~self.defined] = 0
        return out

    def explain(self, got, o):
        g, e = got[o], self.entries[o]
        return ("entry %d (k-mer %s): got sp=0x%x cnt=0x%x, want sp=0x%x cnt=0x%x; %d row(s), first row %d, position %d, context %s, tail %s"
                % (o, self.kmer_of(o), int(g["sp"]), int(g["cnt"]), int(e["sp"]), int(e["cnt"]), int(self.rows[o]), int(self.first_row[o]),
                   int(self.pos[o]), bool(self.has_ctx[o]), bool(self.tail[o])))


class AccelRef:
    def __init__(self, text, seq_starts, alphabet, sa=None):
        self.text = np.ascontiguousarray(text, np.uint8)
        assert self.text[-1] == 36 and (self.text[:-1] != 36).all()
        self.n = len(self.text)
        self.alphabet = alphabet
        self.seq_starts = list(seq_starts)
        self.sa = np.asarray(host_suffix_array(self.text) if sa is None else sa, np.int64)
        assert len(self.sa) == self.n
        self.sym = (NT_SYM if alphabet == NUCLEOTIDE else AA_SYM)[self.text]       # symbol index per position: text8
        self.digit = (NT_DIGIT if alphabet == NUCLEOTIDE else AA_DIGIT)[self.sym]  # table digit per position
        self.sigma = 4 if alphabet == NUCLEOTIDE else AA_SIGMA
        self.bwt = self.sym[self.sa - 1]                                           # sa = 0 -> text[n - 1] = '$' = 0
        self._tables = {}

    # ---- the structures other than the seed table
    def text8(self):
        return self.sym.copy()

    def text4_words(self):
        return (self.n + 7) // 8 + 8

    def text4(self):
        """A0 C1 G2 T3, else 8, eight per u32, position p in bits [4 (p % 8), ...) of word p / 8; zero past the text"""
        code = np.zeros(8 * self.text4_words(), np.uint32)
        code[:self.n] = np.where(self.digit < 4, self.digit, 8)
        w = np.zeros(self.text4_words(), np.uint32)
        for j in range(8):
            w |= code[j::8] << np.uint32(4 * j)
        return w

    def dense_sa(self, ratio):
        return self.sa[::ratio].astype(np.uint32)

    def nblock_window(self):
        """rows [lo, hi) of the suffixes that start with N: below them those of '$', A, C and G"""
        lo = int((self.sym < 4).sum())
        return lo, lo + int((self.sym == 4).sum())

    def sa_nblock(self):
        lo, hi = self.nblock_window()
        assert (self.sym[self.sa[lo:hi]] == 4).all()
        return self.sa[lo:hi].astype(np.uint32)

    def lcx_levels(self):
        """[(offset in words, entries)] of levels 0..7 of lcx_inner (level 0 is not stored: 16 unused words), and the total"""
        off, total = [(0, 0)], 16
        for t in range(1, 8):
            cnt = ((((self.n - 1) >> (4 * t)) + 1 + 15) // 16) * 16 + 16
            off.append((total, cnt))
            total += cnt
        return off, total

    def lcx_inner_level(self, keys, t):
        """level t: the key of every 16^t-th row, 0 past the last row"""
        cnt = self.lcx_levels()[0][t][1]
        rows = np.arange(cnt, dtype=np.int64) << (4 * t)
        out = np.zeros(cnt, np.uint64)
        ok = rows < self.n
        out[ok] = keys[rows[ok]]
        return out

    # ---- the seed table
    def _windows(self, k):
        """per row: does its suffix start with k table digits, and the entry index of those"""
        pad = np.concatenate([self.digit, np.full(k + 1, 255, np.uint8)])
        ok = np.ones(self.n, bool)
        idx = np.zeros(self.n, np.int64)
        mul = 1
        for t in range(k):
            d = pad[self.sa + t]
            ok &= d < self.sigma
            idx += np.where(d < self.sigma, d, 0).astype(np.int64) * mul
            mul *= self.sigma
        return ok, idx

    def _left_complete(self, m):
        """per text position p: do the m letters text[p - m .. p) exist and are all A, C, G or T"""
        bad = np.concatenate([[0], np.cumsum(self.digit >= 4)])  # bad[p] = non-ACGT letters in text[0 .. p)
        p = np.arange(self.n)
        return (p >= m) & (bad[p] - bad[np.maximum(p - m, 0)] == 0)

    def _left_letters(self, p, m):
        """text[p - m + j] in bits [2j, 2j + 2), for positions p whose m left letters are all ACGT"""
        full = np.zeros(len(p), np.uint64)
        for j in range(m):
            full |= self.digit[p - m + j].astype(np.uint64) << np.uint64(2 * j)
        return full

    def kmer_of(self, k, o):
        letters = "ACGT" if self.alphabet == NUCLEOTIDE else "ACDEFGHIKLMNPQRSTVWYX"
        return "".join(letters[(o // self.sigma ** t) % self.sigma] for t in range(k))

    def table(self, k, seed_pos=False, extra=0, lcx=False, wide=False):
        key = (k, bool(seed_pos), int(extra), bool(lcx), bool(wide))
        if key not in self._tables:
            self._tables[key] = self._table(*key)
        return self._tables[key]

    def _table(self, k, seed_pos, extra, lcx, wide):
        nt = self.alphabet == NUCLEOTIDE
        assert not wide or (nt and not seed_pos and not lcx)
        assert not lcx or (nt and seed_pos and k >= 8)
        nent = self.sigma ** k
        ok, idx = self._windows(k)
        rows_ok = np.flatnonzero(ok)
        o_rows = idx[rows_ok]
        assert (np.diff(o_rows) != 0).sum() + 1 == len(np.unique(o_rows)) or len(o_rows) == 0  # a k-mer's rows are contiguous
        T = Table()
        T.kmer_of = lambda o: self.kmer_of(k, int(o))
        T.rows = np.bincount(o_rows, minlength=nent).astype(np.int64)
        uniq, first = np.unique(o_rows, return_index=True)
        T.first_row = np.full(nent, -1, np.int64)
        T.first_row[uniq] = rows_ok[first]
        T.defined = T.rows > 0
        single = np.flatnonzero(T.rows == 1)
        srow = T.first_row[single]
        spos = self.sa[srow]
        ssym = self.bwt[srow].astype(np.uint64)
        T.pos = np.full(nent, -1, np.int64)
        T.pos[single] = spos
        T.has_ctx = np.zeros(nent, bool)
        T.tail = np.zeros(nent, bool)
        sp = np.where(T.defined, T.first_row, 0).astype(np.uint64)
        cnt = T.rows.astype(np.uint64)
        if nt:
            assert T.rows.max() < SEED_CNT_SAT
            sym_shift = 61 if wide else 29
            cnt[single] = np.uint64(1) | (ssym << np.uint64(sym_shift))
            if seed_pos:
                clen = SEED_CTX_LEN + extra
                assert 0 <= extra <= 15
                sp[single] = spos.astype(np.uint64)
                with_ctx = self._left_complete(clen)[spos]
                T.has_ctx[single] = with_ctx
                c_ent, c_pos = single[with_ctx], spos[with_ctx]
                full = self._left_letters(c_pos, clen)
                far = full & np.uint64((1 << (2 * extra)) - 1)
                assert extra == 0 or (c_pos < (1 << (32 - 2 * extra))).all()
                sp[c_ent] = c_pos.astype(np.uint64) | ((far << np.uint64(32 - 2 * extra)) if extra else np.uint64(0))
                cnt[c_ent] = (ssym[with_ctx] << np.uint64(29)) | np.uint64(SEED_CTX) | (full >> np.uint64(2 * extra))
            if lcx:  # a bucket of 2+ rows one of whose suffixes lacks 32 ACGT letters in front has a tail
                incomplete = ~self._left_complete(LCX_CTX)[self.sa[rows_ok]]
                n_inc = np.bincount(o_rows[incomplete], minlength=nent)
                T.tail = (T.rows >= 2) & (n_inc > 0)
                cnt[T.tail] |= np.uint64(SEED_LCX_TAIL)
        else:
            assert T.rows.max() < 0x03FFFFFF
            cnt[single] = np.uint64(1) | (ssym << np.uint64(27))
            for c in (2, 3, 4):  # the set of BWT symbols over the entry's rows
                ent = np.flatnonzero(T.rows == c)
                mask = np.zeros(len(ent), np.uint64)
                for j in range(c):
                    mask |= np.uint64(1) << self.bwt[T.first_row[ent] + j].astype(np.uint64)
                cnt[ent] = np.uint64(AA_SEED_SPECIAL | AA_SEED_MULTI | ((c - 2) << 22)) | mask
            if seed_pos:
                sp[single] = spos.astype(np.uint64)
                with_ctx = spos >= AA_SEED_CTX_LEN
                T.has_ctx[single] = with_ctx
                c_ent, c_pos = single[with_ctx], spos[with_ctx]
                ctx = np.zeros(len(c_ent), np.uint64)
                for j in range(AA_SEED_CTX_LEN - 1):
                    ctx |= (self.sym[c_pos - 2 - j].astype(np.uint64) & np.uint64(0x1F)) << np.uint64(5 * j)
                cnt[c_ent] = (ssym[with_ctx] << np.uint64(27)) | np.uint64(AA_SEED_SPECIAL) | ctx
        T.entries = np.zeros(nent, ENTRY64 if wide else ENTRY32)
        if not wide:
            assert sp.max() < (1 << 32) and cnt.max() < (1 << 32)
        T.entries["sp"] = sp
        T.entries["cnt"] = cnt
        return T
