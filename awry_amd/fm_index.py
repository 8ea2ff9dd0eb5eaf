"""Host-side mirror of the reference's public `FmIndex` surface (/root/reference src/fm_index.rs) over the
C ABI of libawry_hip.so.  Same names, argument meaning and error behaviour: query functions raise where
the reference panics (empty query, '$'/'#').  All searching happens in HIP kernels on the GPU(s) chosen
with `set_devices`; nothing here computes a count or a location on the CPU."""
import ctypes as C
import os
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import _lib

NUCLEOTIDE, AMINO = 0, 1
BUILD_HOST, BUILD_AUTO = -1, -2


class SymbolAlphabet:  # src/alphabet.rs:28-31
    Nucleotide = NUCLEOTIDE
    Amino = AMINO


class AwryError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("awry error %d: %s" % (code, msg))
        self.code = code


ERR_IO, ERR_FORMAT, ERR_INVALID_QUERY, ERR_HIP, ERR_OOM, ERR_ARG, ERR_NO_DEVICE = -1, -2, -3, -4, -5, -6, -7
MAX_MISMATCHES = 2  # AWRY_MAX_MISMATCHES
MAX_EDITS, EDIT_MAX_LEN, Q_CANDIDATE_CAP = 8, 256, 7  # AWRY_MAX_EDITS, AWRY_EDIT_MAX_LEN, AWRY_Q_CANDIDATE_CAP
ALIGN_MAX_OPS = 17  # AWRY_ALIGN_MAX_OPS
CHAIN_MAX_SEEDS, CHAIN_MAX_LOOKBACK, Q_SEED_CAP = 4096, 64, 8  # AWRY_CHAIN_MAX_SEEDS, AWRY_CHAIN_MAX_LOOKBACK, AWRY_Q_SEED_CAP
CHAIN_ALIGN_MAX_BAND, CHAIN_ALIGN_MAX_SKEW, CHAIN_ALIGN_MAX_LEN = 8, 16, 1024  # AWRY_CHAIN_ALIGN_MAX_BAND, _MAX_SKEW, _MAX_LEN
ALN_OK, ALN_SKEW, ALN_BAD_CHAIN = 0, 1, 2  # AWRY_ALN_OK, AWRY_ALN_SKEW, AWRY_ALN_BAD_CHAIN
MAP_MAX_CHAINS, MAP_SECONDARY = 8, 1  # AWRY_MAP_MAX_CHAINS, AWRY_MAP_SECONDARY
MAP_SUPPLEMENTARY, SPLIT_MAX_SEGMENTS = 16, 4  # AWRY_MAP_SUPPLEMENTARY, AWRY_SPLIT_MAX_SEGMENTS
MAP_PROPER_PAIR, MAP_RESCUED, MAP_MATE_UNMAPPED = 2, 4, 8  # AWRY_MAP_PROPER_PAIR, AWRY_MAP_RESCUED, AWRY_MAP_MATE_UNMAPPED
PAIR_MAX_INSERT, PAIR_MAX_ANCHORS, PAIR_NO_CHAIN = 1 << 20, 4, 0xFFFFFFFF  # AWRY_PAIR_MAX_INSERT, AWRY_PAIR_MAX_ANCHORS, AWRY_PAIR_NO_CHAIN
CLIP_MAX_MATCH, CLIP_MAX_PENALTY, CLIP_MAX_END_BONUS = 16, 64, 1024  # AWRY_CLIP_MAX_MATCH, AWRY_CLIP_MAX_PENALTY, AWRY_CLIP_MAX_END_BONUS
CIGAR_OPS = {1: "I", 2: "D", 4: "S", 7: "=", 8: "X"}  # the BAM op codes the alignment passes produce ('S': the clipped mode)


def cigar_string(ops) -> str:
    """runs (len << 4 | BAM op) -> the CIGAR string, "57=1X43=" """
    return "".join("%d%s" % (int(v) >> 4, CIGAR_OPS[int(v) & 15]) for v in ops)


def sa_tags(records, headers):
    """the SA:Z values of one read's records as parallel_map_split returns them, headers[r] the name of record r: per record, for a
    segment the entries "rname,pos1,+/-,CIGAR,mapq,edits;" of its sibling segments in their order (pos1 is 1-based; "" for a read of one
    segment), for a secondary None"""
    segs = [r for r in records if not r[6] & MAP_SECONDARY]
    entry = lambda r: "%s,%d,%s,%s,%d,%d;" % (headers[r[0]], r[1] + 1, "-" if r[2] else "+", r[5], r[3], r[4])
    return [None if r[6] & MAP_SECONDARY else "".join(entry(g) for g in segs if g is not r) for r in records]


@dataclass
class FmBuildArgs:  # src/fm_index.rs:78-96
    input_file_src: str
    suffix_array_output_src: Optional[str] = None
    suffix_array_compression_ratio: Optional[int] = None
    lookup_table_kmer_len: Optional[int] = None
    alphabet: int = NUCLEOTIDE
    max_query_len: Optional[int] = None
    remove_intermediate_suffix_array_file: bool = False


@dataclass(frozen=True, order=True)
class LocalizedSequencePosition:  # src/sequence_index.rs:31-78
    sequence_idx: int
    local_position: int


@dataclass(frozen=True, order=True)
class SearchRange:  # src/search.rs:25-81
    start_ptr: int
    end_ptr: int

    @staticmethod
    def zero():
        return SearchRange(1, 0)

    def is_empty(self):
        return self.start_ptr > self.end_ptr

    def len(self):
        return 0 if self.is_empty() else self.end_ptr - self.start_ptr + 1

    def range_iter(self):
        return range(0) if self.is_empty() else range(self.start_ptr, self.end_ptr + 1)


def _check(rc):
    if rc != 0:
        raise AwryError(rc, _lib.load_library().awry_last_error().decode(errors="replace"))


def _as_bytes(q):
    if isinstance(q, str):
        return q.encode("latin-1")
    if isinstance(q, np.ndarray):
        return np.ascontiguousarray(q, dtype=np.uint8).tobytes()
    return bytes(q)


def pack_queries(queries: Iterable):
    """iterable of str / bytes / uint8 arrays -> (uint8[total], uint64[n+1]) CSR"""
    qs = [_as_bytes(q) for q in queries]
    off = np.zeros(len(qs) + 1, dtype=np.uint64)
    if qs:
        off[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(qs), dtype=np.uint8).copy() if qs else np.zeros(0, np.uint8)
    return buf, off


_u64p = C.POINTER(C.c_uint64)

# awry_anchor_t as a numpy record (24 bytes, the C layout)
ANCHOR_DTYPE = np.dtype([("q_begin", np.uint32), ("q_len", np.uint32), ("start_row", np.uint64), ("count", np.uint64)])
SEED_DTYPE = np.dtype([("q_begin", np.uint32), ("q_len", np.uint32), ("t_pos", np.uint64)])  # awry_seed_t
CHAIN_DTYPE = np.dtype([("score", np.uint32), ("n_seeds", np.uint32), ("q_begin", np.uint32), ("q_end", np.uint32), ("t_begin", np.uint64),
                        ("t_end", np.uint64)])  # awry_chain_t
ALN_DTYPE = np.dtype([("t_begin", np.uint64), ("t_end", np.uint64), ("edits", np.uint32), ("status", np.uint32)])  # awry_aln_t
MAP_DTYPE = np.dtype([("t_begin", np.uint64), ("t_end", np.uint64), ("edits", np.uint32), ("chain_score", np.uint32), ("chain_index", np.uint32),
                      ("strand", np.uint8), ("mapq", np.uint8), ("flags", np.uint16)])  # awry_map_t
_CLIP_FIELDS = [("score", np.int32), ("clip_left", np.uint16), ("clip_right", np.uint16)]
ALN_CLIP_DTYPE = np.dtype(ALN_DTYPE.descr + _CLIP_FIELDS)  # awry_aln_clip_t, 32 bytes
MAP_CLIP_DTYPE = np.dtype(MAP_DTYPE.descr + _CLIP_FIELDS)  # awry_map_clip_t, 40 bytes
MAP_SPLIT_DTYPE = np.dtype(MAP_CLIP_DTYPE.descr + [("q_begin", np.uint16), ("q_end", np.uint16), ("parent", np.uint16),
                                                   ("reserved", np.uint16)])  # awry_map_split_t, 48 bytes


class _Owned:
    """a malloc'ed result buffer of the C ABI, exposed to numpy without a copy and released (awry_free_buffer) with
    the last array that views it"""

    def __init__(self, lib, addr, nbytes):
        self._lib, self._addr = lib, addr
        self.__array_interface__ = {"data": (addr, False), "shape": (nbytes,), "typestr": "|u1", "version": 3}

    def __del__(self):
        try:
            self._lib.awry_free_buffer(C.c_void_p(self._addr))
        except Exception:
            pass


def _adopt(lib, ptr, count, dtype):
    addr = C.cast(ptr, C.c_void_p).value
    if not count or not addr:
        if addr:
            lib.awry_free_buffer(C.c_void_p(addr))
        return np.zeros(0, dtype)
    return np.asarray(_Owned(lib, addr, count * np.dtype(dtype).itemsize)).view(dtype)


def read_query_file(path):
    """FASTA / FASTQ file -> (uint8 bytes, uint64 offsets[n+1]): one query per record (query ingestion)"""
    L = _lib.load_library()
    b, o, n = C.POINTER(C.c_uint8)(), _u64p(), C.c_uint64()
    _check(L.awry_read_query_file(os.fsencode(path), C.byref(b), C.byref(o), C.byref(n)))
    off = _adopt(L, o, int(n.value) + 1, np.uint64)
    qb = _adopt(L, b, int(off[-1]), np.uint8)
    return qb, off


def pattern_class(alphabet: int, letter) -> int:
    """class mask of a pattern letter (parallel_count_pattern): bit s = symbol index s belongs to the class, 0 = the byte is
    no class letter of that alphabet.  Needs no GPU."""
    b = letter if isinstance(letter, int) else _as_bytes(letter)[0]
    return int(_lib.load_library().awry_pattern_class(int(alphabet), b))


class FmIndex:
    def __init__(self, handle):
        self._L = _lib.load_library()
        self._h = C.c_void_p(handle)

    # ------------------------------------------------------------------ construction / persistence
    @classmethod
    def new(cls, args: FmBuildArgs) -> "FmIndex":
        """FmIndex::new, src/fm_index.rs:142-268"""
        L = _lib.load_library()
        a = _lib.BuildArgs(os.fsencode(args.input_file_src),
                           os.fsencode(args.suffix_array_output_src) if args.suffix_array_output_src else None,
                           args.suffix_array_compression_ratio or 0, args.lookup_table_kmer_len or 0, args.alphabet,
                           args.max_query_len or 0, 1 if args.remove_intermediate_suffix_array_file else 0)
        h = C.c_void_p()
        _check(L.awry_build(C.byref(a), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_text(cls, text, alphabet=NUCLEOTIDE, sa_ratio=8, kmer_len=0, seq_starts=(0,), headers=("seq0",),
                  build_device=BUILD_AUTO) -> "FmIndex":
        """index an in-memory text that already follows the reference's text model (ends in '$');
        build_device: GPU id, BUILD_HOST (host SA-IS) or BUILD_AUTO"""
        L = _lib.load_library()
        t = np.frombuffer(_as_bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        st = np.ascontiguousarray(list(seq_starts), dtype=np.uint64)
        if len(st) != len(headers):
            raise ValueError("seq_starts and headers must have one entry per record (%d != %d)" % (len(st), len(headers)))
        hd = (C.c_char_p * len(headers))(*[h.encode() for h in headers])
        h = C.c_void_p()
        _check(L.awry_build_from_text_on(t.ctypes.data, len(t), alphabet, sa_ratio, kmer_len, st.ctypes.data_as(_u64p), hd,
                                         len(headers), build_device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def load(cls, path) -> "FmIndex":
        """FmIndex::load, src/fm_index_file.rs:132"""
        L = _lib.load_library()
        h = C.c_void_p()
        _check(L.awry_load(os.fsencode(path), C.byref(h)))
        return cls(h.value)

    def save(self, path):
        """FmIndex::save, src/fm_index_file.rs:42"""
        _check(self._L.awry_save(self._h, os.fsencode(path)))

    def close(self):
        if self._h:
            self._L.awry_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ device placement
    def set_devices(self, device_ids: Sequence[int] = (0,)) -> "FmIndex":
        ids = (C.c_int * len(device_ids))(*device_ids)
        _check(self._L.awry_set_devices(self._h, ids, len(device_ids)))
        return self

    def set_seed_kmer_len(self, k: int):
        _check(self._L.awry_set_seed_kmer_len(self._h, k))

    def seed_kmer_len(self) -> int:
        return self._L.awry_seed_kmer_len(self._h)

    def count_schedule(self, L: int) -> str:
        """kernel(s) dev_count_nt2 launches for k-mers of length L"""
        return self._L.awry_count_schedule(self._h, L).decode()

    def num_devices(self) -> int:
        return self._L.awry_num_devices(self._h)

    # ------------------------------------------------------------------ accessors (src/fm_index.rs:302-399)
    def alphabet(self) -> int:
        return self._L.awry_alphabet(self._h)

    def bwt_len(self) -> int:
        return int(self._L.awry_bwt_len(self._h))

    def version_number(self) -> int:
        return int(self._L.awry_version(self._h))

    def suffix_array_compression_ratio(self) -> int:
        return int(self._L.awry_sa_ratio(self._h))

    def lookup_table_kmer_len(self) -> int:
        return int(self._L.awry_kmer_len(self._h))

    def sentinel_row(self) -> int:
        return int(self._L.awry_sentinel_row(self._h))

    def _arr(self, fn):
        n = C.c_uint64()
        p = getattr(self._L, fn)(self._h, C.byref(n))
        return np.ctypeslib.as_array(p, shape=(int(n.value),)).copy() if n.value else np.zeros(0, np.uint64)

    def prefix_sums(self) -> np.ndarray:
        return self._arr("awry_prefix_sums")

    def device_block_words(self) -> np.ndarray:
        return self._arr("awry_block_words")

    def sa_words(self) -> np.ndarray:
        return self._arr("awry_sa_words")

    def reference_block_words(self) -> np.ndarray:
        """all BWT blocks converted to the reference layout (planes then milestones, src/bwt.rs:12-25)"""
        rw = 20 if self.alphabet() == NUCLEOTIDE else 44
        nb = (self.bwt_len() + 255) // 256
        out = np.zeros(nb * rw, dtype=np.uint64)
        for b in range(nb):
            _check(self._L.awry_block_reference_layout(self._h, b, out[b * rw:].ctypes.data_as(_u64p), rw))
        return out

    def sequences(self):
        n = int(self._L.awry_num_sequences(self._h))
        return [(int(self._L.awry_sequence_start(self._h, i)), self._L.awry_sequence_header(self._h, i).decode()) for i in range(n)]

    # ------------------------------------------------------------------ scalar queries
    def count_string(self, query) -> int:
        """src/fm_index.rs:499-501"""
        q = _as_bytes(query)
        c = C.c_uint64()
        _check(self._L.awry_count(self._h, q, len(q), C.byref(c)))
        return int(c.value)

    def search_range(self, query) -> SearchRange:
        """get_search_range_for_string, src/fm_index.rs:402-438"""
        q = _as_bytes(query)
        r = _lib.Range()
        _check(self._L.awry_search_range(self._h, q, len(q), C.byref(r)))
        return SearchRange(int(r.start_ptr), int(r.end_ptr))

    def locate_string(self, query) -> List[LocalizedSequencePosition]:
        """src/fm_index.rs:516-544 (ascending BWT-row order)"""
        return [LocalizedSequencePosition(int(a), int(b)) for a, b in self.locate_string_raw(query)[1]]

    def locate_string_raw(self, query):
        """-> (global positions uint64[n], (seq_idx, local_pos) uint64[n, 2])"""
        q = _as_bytes(query)
        hits, gp, n = C.POINTER(_lib.Pos)(), _u64p(), C.c_uint64()
        _check(self._L.awry_locate(self._h, q, len(q), C.byref(hits), C.byref(gp), C.byref(n)))
        k = int(n.value)
        g = np.ctypeslib.as_array(gp, shape=(k,)).copy() if k else np.zeros(0, np.uint64)
        p = np.ctypeslib.as_array(C.cast(hits, _u64p), shape=(2 * k,)).copy().reshape(-1, 2) if k else np.zeros((0, 2), np.uint64)
        self._L.awry_free_buffer(hits)
        self._L.awry_free_buffer(gp)
        return g, p

    def initial_search_range(self, symbol) -> SearchRange:
        r = _lib.Range()
        _check(self._L.awry_initial_range(self._h, ord(symbol) if isinstance(symbol, str) else int(symbol), C.byref(r)))
        return SearchRange(int(r.start_ptr), int(r.end_ptr))

    def update_range_with_symbol(self, search_range: SearchRange, symbol) -> SearchRange:
        """src/fm_index.rs:559-582"""
        r = _lib.Range()
        _check(self._L.awry_update_range(self._h, _lib.Range(search_range.start_ptr, search_range.end_ptr),
                                         ord(symbol) if isinstance(symbol, str) else int(symbol), C.byref(r)))
        return SearchRange(int(r.start_ptr), int(r.end_ptr))

    def backstep(self, search_pointer: int) -> int:
        """src/fm_index.rs:585-593"""
        o = C.c_uint64()
        _check(self._L.awry_backstep(self._h, search_pointer, C.byref(o)))
        return int(o.value)

    def get_seq_location(self, global_position: int) -> LocalizedSequencePosition:
        p = _lib.Pos()
        _check(self._L.awry_get_seq_location(self._h, global_position, C.byref(p)))
        return LocalizedSequencePosition(int(p.seq_idx), int(p.local_pos))

    # ------------------------------------------------------------------ batch queries
    def parallel_count_csr(self, qbytes: np.ndarray, qoff: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """counts of the CSR batch in input order; `out` (uint64[n], contiguous) is filled and returned when given -- the
        C ABI's counts_out is caller-owned, and a caller that reuses its result array spares the batch the first-touch
        page faults of a fresh one"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        if out is None:
            out = np.empty(n, dtype=np.uint64)
        elif out.dtype != np.uint64 or out.shape != (n,) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint64 array with one entry per query")
        _check(self._L.awry_count_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, out.ctypes.data_as(_u64p)))
        return out

    def parallel_count_packed(self, words: np.ndarray, L: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """k-mers already packed 2 bits per letter (letter j of a k-mer in bits [2j, 2j+2) of its uint64, A0 C1 G2 T3)"""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if out is None:
            out = np.empty(len(w), dtype=np.uint64)
        elif out.dtype != np.uint64 or out.shape != (len(w),) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint64 array with one entry per query")
        _check(self._L.awry_count_packed_kmers(self._h, w.ctypes.data_as(_u64p), len(w), L, out.ctypes.data_as(_u64p)))
        return out

    def parallel_count(self, queries: Iterable) -> np.ndarray:
        """src/fm_index.rs:455-460: counts in input order"""
        return self.parallel_count_csr(*pack_queries(queries))

    def parallel_locate_csr(self, qbytes: np.ndarray, qoff: np.ndarray, want_pos: bool = True):
        """-> (hit_off uint64[n+1], global_pos uint64[total], pos uint64[total, 2]); want_pos=False passes hits_out = NULL
        (text positions only: 8 B per hit cross PCIe instead of 24) and returns an empty pos"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, hits, gp = _u64p(), C.POINTER(_lib.Pos)(), _u64p()
        _check(self._L.awry_locate_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, C.byref(off),
                                         C.byref(hits) if want_pos else None, C.byref(gp)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        g = _adopt(self._L, gp, tot, np.uint64)
        p = _adopt(self._L, hits, 2 * tot, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        return offs, g, p

    def parallel_locate(self, queries: Iterable) -> List[List[LocalizedSequencePosition]]:
        """src/fm_index.rs:479-487: outer order = input order, inner order = ascending BWT row"""
        off, _, p = self.parallel_locate_csr(*pack_queries(queries))
        return [[LocalizedSequencePosition(int(a), int(b)) for a, b in p[off[i]:off[i + 1]]] for i in range(len(off) - 1)]

    # ------------------------------------------------------------------ substitution-tolerant search (Hamming distance <= k)
    def parallel_count_mismatch_csr(self, qbytes: np.ndarray, qoff: np.ndarray, k: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """-> uint64[n, k + 1]: row i holds the occurrences of query i at exactly 0, 1, .., k substitutions (include/awry_hip.h
        states the semantics); `out` (contiguous uint64[n, k + 1]) is filled and returned when given"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        w = max(int(k), 0) + 1
        if out is None:
            out = np.empty((n, w), dtype=np.uint64)
        elif out.dtype != np.uint64 or out.shape != (n, w) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint64 array of shape (n, k + 1)")
        _check(self._L.awry_count_mismatch_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(k), out.ctypes.data_as(_u64p)))
        return out

    def parallel_count_mismatch(self, queries: Iterable, k: int) -> np.ndarray:
        """counts per query and distance, uint64[n, k + 1], in input order"""
        return self.parallel_count_mismatch_csr(*pack_queries(queries), k)

    def parallel_locate_mismatch_csr(self, qbytes: np.ndarray, qoff: np.ndarray, k: int, want_pos: bool = True):
        """-> (hit_off uint64[n+1], global_pos uint64[total], pos uint64[total, 2], mismatches uint8[total]): hits of query i
        in ascending BWT-row order with the distance of each; want_pos=False leaves pos empty"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, hits, gp, mm = _u64p(), C.POINTER(_lib.Pos)(), _u64p(), C.POINTER(C.c_uint8)()
        _check(self._L.awry_locate_mismatch_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(k), C.byref(off),
                                                  C.byref(hits) if want_pos else None, C.byref(gp), C.byref(mm)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        g = _adopt(self._L, gp, tot, np.uint64)
        p = _adopt(self._L, hits, 2 * tot, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        d = _adopt(self._L, mm, tot, np.uint8)
        return offs, g, p, d

    def count_string_mismatch(self, query, k: int) -> int:
        """occurrences of one query with at most k substitutions"""
        return int(self.parallel_count_mismatch([query], k).sum())

    def locate_string_mismatch(self, query, k: int):
        """-> [(LocalizedSequencePosition, distance)] of one query, ascending BWT-row order"""
        off, _, p, d = self.parallel_locate_mismatch_csr(*pack_queries([query]), k)
        return [(LocalizedSequencePosition(int(a), int(b)), int(m)) for (a, b), m in zip(p, d)]

    def dev_count_mismatch(self, d_qbytes, d_qoff, n, k, d_counts, d_status=None, stream=None, slot=0):
        """device-resident count: d_counts[n * (k + 1)] (u64), optional d_status[n] bytes"""
        _check(self._L.awry_dev_count_mismatch(self._h, slot, d_qbytes, d_qoff, n, int(k), d_counts, d_status, stream))

    def dev_count_mismatch_tally(self, d_qbytes, d_qoff, n, k, d_counts, d_tally, d_status=None, stream=None, slot=0):
        """dev_count_mismatch + census: d_tally[2] += (expansions, queries searched)"""
        _check(self._L.awry_dev_count_mismatch_tally(self._h, slot, d_qbytes, d_qoff, n, int(k), d_counts, d_status, d_tally, stream))

    # ------------------------------------------------------------------ class patterns (IUPAC / residue classes, <= k mismatches)
    def parallel_count_pattern_csr(self, qbytes: np.ndarray, qoff: np.ndarray, k: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
        """-> uint64[n, k + 1]: row i holds the occurrences of pattern i at exactly 0, 1, .., k mismatches.  A pattern is a string
        of class letters (nucleotide IUPAC codes, amino B / Z / J / X; include/awry_hip.h states the definition and limits);
        `out` (contiguous uint64[n, k + 1]) is filled and returned when given"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        w = max(int(k), 0) + 1
        if out is None:
            out = np.empty((n, w), dtype=np.uint64)
        elif out.dtype != np.uint64 or out.shape != (n, w) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint64 array of shape (n, k + 1)")
        _check(self._L.awry_count_pattern_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(k), out.ctypes.data_as(_u64p)))
        return out

    def parallel_count_pattern(self, patterns: Iterable, k: int = 0) -> np.ndarray:
        """counts per pattern and distance, uint64[n, k + 1], in input order"""
        return self.parallel_count_pattern_csr(*pack_queries(patterns), k)

    def parallel_locate_pattern_csr(self, qbytes: np.ndarray, qoff: np.ndarray, k: int = 0, want_pos: bool = True):
        """-> (hit_off uint64[n+1], global_pos uint64[total], pos uint64[total, 2], mismatches uint8[total]): hits of pattern i
        in ascending BWT-row order (the matched strings in symbol-index order) with the distance of each; want_pos=False
        leaves pos empty"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, hits, gp, mm = _u64p(), C.POINTER(_lib.Pos)(), _u64p(), C.POINTER(C.c_uint8)()
        _check(self._L.awry_locate_pattern_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(k), C.byref(off),
                                                 C.byref(hits) if want_pos else None, C.byref(gp), C.byref(mm)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        g = _adopt(self._L, gp, tot, np.uint64)
        p = _adopt(self._L, hits, 2 * tot, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        d = _adopt(self._L, mm, tot, np.uint8)
        return offs, g, p, d

    def count_string_pattern(self, pattern, k: int = 0) -> int:
        """occurrences of one class pattern with at most k mismatches"""
        return int(self.parallel_count_pattern([pattern], k).sum())

    def locate_string_pattern(self, pattern, k: int = 0):
        """-> [(LocalizedSequencePosition, distance)] of one class pattern, ascending BWT-row order"""
        off, _, p, d = self.parallel_locate_pattern_csr(*pack_queries([pattern]), k)
        return [(LocalizedSequencePosition(int(a), int(b)), int(m)) for (a, b), m in zip(p, d)]

    def dev_count_pattern(self, d_qbytes, d_qoff, n, k, d_counts, d_status=None, stream=None, slot=0):
        """device-resident pattern count: d_counts[n * (k + 1)] (u64), optional d_status[n] bytes (0 ok, 1 empty, 2 sentinel,
        3 byte >= 0x80, 4 no class letter, 5 too many class positions, 6 abandoned at the expansion cap)"""
        _check(self._L.awry_dev_count_pattern(self._h, slot, d_qbytes, d_qoff, n, int(k), d_counts, d_status, stream))

    def dev_count_pattern_tally(self, d_qbytes, d_qoff, n, k, d_counts, d_tally, d_status=None, stream=None, slot=0):
        """dev_count_pattern + census: d_tally[3]: [0] += expansions, [1] += patterns searched, [2] = max(deepest stack, frames)"""
        _check(self._L.awry_dev_count_pattern_tally(self._h, slot, d_qbytes, d_qoff, n, int(k), d_counts, d_status, d_tally, stream))

    # ------------------------------------------------------------------ anchors (greedy longest-match factorisation)
    def parallel_anchors_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 1, skip: int = 0):
        """-> (anchor_off uint64[n+1], anchors ANCHOR_DTYPE[total]): the maximal exact matches of every query, found right to
        left (include/awry_hip.h states the definition); anchors of query i are anchors[anchor_off[i]:anchor_off[i+1]]"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, an = _u64p(), C.POINTER(_lib.Anchor)()
        _check(self._L.awry_anchor_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), int(skip), C.byref(off), C.byref(an)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        return offs, _adopt(self._L, an, 24 * int(offs[-1]), np.uint8).view(ANCHOR_DTYPE)

    def parallel_anchors(self, queries: Iterable, min_len: int = 1, skip: int = 0):
        """-> per query, its anchors as (q_begin, q_len, start_row, count) tuples in the order found (descending q_begin)"""
        off, an = self.parallel_anchors_csr(*pack_queries(queries), min_len, skip)
        return [[tuple(int(v) for v in a) for a in an[off[i]:off[i + 1]]] for i in range(len(off) - 1)]

    def anchors_string(self, query, min_len: int = 1, skip: int = 0):
        """anchors of one query"""
        return self.parallel_anchors([query], min_len, skip)[0]

    def parallel_locate_anchors_csr(self, qbytes: np.ndarray, qoff: np.ndarray, max_hits: int, min_len: int = 1, skip: int = 0,
                                    want_pos: bool = True):
        """-> (anchor_off, anchors, hit_off uint64[total+1], global_pos uint64[hits], pos uint64[hits, 2]): hits of anchor s are
        [hit_off[s], hit_off[s+1]) in ascending BWT-row order; an anchor of more than max_hits rows gets none"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, an, hoff, hits, gp = _u64p(), C.POINTER(_lib.Anchor)(), _u64p(), C.POINTER(_lib.Pos)(), _u64p()
        _check(self._L.awry_locate_anchors_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), int(skip), int(max_hits),
                                                 C.byref(off), C.byref(an), C.byref(hoff), C.byref(hits) if want_pos else None, C.byref(gp)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        anchors = _adopt(self._L, an, 24 * tot, np.uint8).view(ANCHOR_DTYPE)
        hit_off = _adopt(self._L, hoff, tot + 1, np.uint64)
        nh = int(hit_off[-1])
        g = _adopt(self._L, gp, nh, np.uint64)
        p = _adopt(self._L, hits, 2 * nh, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        return offs, anchors, hit_off, g, p

    def dev_anchors(self, d_qbytes, d_qoff, n, min_len, skip, d_n_anchors, d_anchor_off=None, d_anchors=None, d_status=None, stream=None, slot=0):
        """device-resident anchors: d_anchor_off None = the count pass (d_n_anchors[n] u64, optional d_status[n]); else the fill
        pass writing 24-byte records at d_anchors[d_anchor_off[q] ...); scan d_n_anchors with dev_scan_counts in between"""
        _check(self._L.awry_dev_anchors(self._h, slot, d_qbytes, d_qoff, n, int(min_len), int(skip), d_n_anchors, d_anchor_off, d_anchors, d_status, stream))

    def dev_anchors_tally(self, d_qbytes, d_qoff, n, min_len, skip, d_n_anchors, d_tally, d_anchor_off=None, d_anchors=None, d_status=None,
                          stream=None, slot=0):
        """dev_anchors + census: d_tally[3] += (LF steps executed, probes that supplied a range, anchors reported)"""
        _check(self._L.awry_dev_anchors_tally(self._h, slot, d_qbytes, d_qoff, n, int(min_len), int(skip), d_n_anchors, d_anchor_off, d_anchors,
                                              d_status, d_tally, stream))

    # ------------------------------------------------------------------ SMEMs (all super-maximal exact matches)
    def parallel_smems_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 1):
        """-> (smem_off uint64[n+1], smems ANCHOR_DTYPE[total]): every super-maximal exact match of every query (include/awry_hip.h
        states the definition), in descending q_begin; SMEMs of query i are smems[smem_off[i]:smem_off[i+1]]"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, an = _u64p(), C.POINTER(_lib.Anchor)()
        _check(self._L.awry_smem_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), C.byref(off), C.byref(an)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        return offs, _adopt(self._L, an, 24 * int(offs[-1]), np.uint8).view(ANCHOR_DTYPE)

    def parallel_smems(self, queries: Iterable, min_len: int = 1):
        """-> per query, its SMEMs as (q_begin, q_len, start_row, count) tuples in descending q_begin"""
        off, an = self.parallel_smems_csr(*pack_queries(queries), min_len)
        return [[tuple(int(v) for v in a) for a in an[off[i]:off[i + 1]]] for i in range(len(off) - 1)]

    def smems_string(self, query, min_len: int = 1):
        """SMEMs of one query"""
        return self.parallel_smems([query], min_len)[0]

    def parallel_locate_smems_csr(self, qbytes: np.ndarray, qoff: np.ndarray, max_hits: int, min_len: int = 1, want_pos: bool = True):
        """-> (smem_off, smems, hit_off uint64[total+1], global_pos uint64[hits], pos uint64[hits, 2]): hits of record s are
        [hit_off[s], hit_off[s+1]) in ascending BWT-row order; a record of more than max_hits rows gets none"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, an, hoff, hits, gp = _u64p(), C.POINTER(_lib.Anchor)(), _u64p(), C.POINTER(_lib.Pos)(), _u64p()
        _check(self._L.awry_locate_smems_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), int(max_hits),
                                               C.byref(off), C.byref(an), C.byref(hoff), C.byref(hits) if want_pos else None, C.byref(gp)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        smems = _adopt(self._L, an, 24 * tot, np.uint8).view(ANCHOR_DTYPE)
        hit_off = _adopt(self._L, hoff, tot + 1, np.uint64)
        nh = int(hit_off[-1])
        g = _adopt(self._L, gp, nh, np.uint64)
        p = _adopt(self._L, hits, 2 * nh, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        return offs, smems, hit_off, g, p

    def dev_smems(self, d_qbytes, d_qoff, n, min_len, d_n_smems, d_smem_off=None, d_smems=None, d_status=None, stream=None, slot=0):
        """device-resident SMEMs: d_smem_off None = the count pass (d_n_smems[n] u64, optional d_status[n]); else the fill pass
        writing 24-byte records at d_smems[d_smem_off[q] ...); scan d_n_smems with dev_scan_counts in between"""
        _check(self._L.awry_dev_smems(self._h, slot, d_qbytes, d_qoff, n, int(min_len), d_n_smems, d_smem_off, d_smems, d_status, stream))

    def dev_smems_tally(self, d_qbytes, d_qoff, n, min_len, d_n_smems, d_tally, d_smem_off=None, d_smems=None, d_status=None, stream=None, slot=0):
        """dev_smems + census: d_tally[4] += (LF steps executed, suffixes compared by the SA search, forward extensions, SMEMs reported)"""
        _check(self._L.awry_dev_smems_tally(self._h, slot, d_qbytes, d_qoff, n, int(min_len), d_n_smems, d_smem_off, d_smems, d_status, d_tally,
                                            stream))

    # ------------------------------------------------------------------ colinear chaining of the located SMEM seeds
    def parallel_chains_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, max_seeds: int = 1024,
                            lookback: int = 32, max_gap: int = 1000, max_skew: int = 100, min_score: int = 20, want_seeds: bool = True):
        """-> (chain_off uint64[n+1], chains CHAIN_DTYPE[total], seed_off uint64[total+1], seeds SEED_DTYPE[members], status uint8[n]):
        the chains of every query's located SMEM seeds (include/awry_hip.h states the definition), the primary chain first; the
        members of chain c are seeds[seed_off[c]:seed_off[c+1]], first to last; status[i] == Q_SEED_CAP marks a query abandoned
        because it has more than max_seeds seeds (it has no chains); want_seeds=False leaves seed_off and seeds empty"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, ch, soff, sd, st = _u64p(), C.POINTER(_lib.Chain)(), _u64p(), C.POINTER(_lib.Seed)(), C.POINTER(C.c_uint8)()
        _check(self._L.awry_chain_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), int(max_hits), int(max_seeds),
                                        int(lookback), int(max_gap), int(max_skew), int(min_score), C.byref(off), C.byref(ch),
                                        C.byref(soff) if want_seeds else None, C.byref(sd) if want_seeds else None, C.byref(st)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        chains = _adopt(self._L, ch, 32 * tot, np.uint8).view(CHAIN_DTYPE)
        status = _adopt(self._L, st, n, np.uint8)
        if not want_seeds:
            return offs, chains, np.zeros(0, np.uint64), np.zeros(0, SEED_DTYPE), status
        seed_off = _adopt(self._L, soff, tot + 1, np.uint64)
        return offs, chains, seed_off, _adopt(self._L, sd, 16 * int(seed_off[-1]), np.uint8).view(SEED_DTYPE), status

    def parallel_chains(self, queries: Iterable, min_len: int = 12, max_hits: int = 50, **params):
        """-> per query, its chains as (score, q_begin, q_end, t_begin, t_end, [(q_begin, q_len, t_pos), ...]), the primary chain
        first (none for an abandoned query); params: max_seeds, lookback, max_gap, max_skew, min_score"""
        off, ch, soff, sd, _ = self.parallel_chains_csr(*pack_queries(queries), min_len, max_hits, **params)
        return [[(int(c["score"]), int(c["q_begin"]), int(c["q_end"]), int(c["t_begin"]), int(c["t_end"]),
                  [tuple(int(v) for v in m) for m in sd[soff[j]:soff[j + 1]]]) for j, c in enumerate(ch[off[i]:off[i + 1]], int(off[i]))]
                for i in range(len(off) - 1)]

    def chains_string(self, query, min_len: int = 12, max_hits: int = 50, **params):
        """chains of one query"""
        return self.parallel_chains([query], min_len, max_hits, **params)[0]

    def dev_chain_seeds(self, d_seed_off, d_seeds, n, max_seeds, lookback, max_gap, max_skew, min_score, d_n_chains, d_n_members,
                        d_chain_off=None, d_member_off=None, d_chains=None, d_members=None, d_status=None, stream=None, slot=0):
        """device-resident chaining of the caller's seeds (16-byte records, query q: d_seeds[d_seed_off[q] .. d_seed_off[q+1])):
        d_chain_off None = the count pass (d_n_chains[n], d_n_members[n] u64, optional d_status[n]); else the fill pass writing
        32-byte chain records at d_chains[d_chain_off[q] ...) and their members at d_members[d_member_off[q] ...); scan both
        counts with dev_scan_counts in between"""
        _check(self._L.awry_dev_chain_seeds(self._h, slot, d_seed_off, d_seeds, n, int(max_seeds), int(lookback), int(max_gap), int(max_skew),
                                            int(min_score), d_n_chains, d_n_members, d_chain_off, d_member_off, d_chains, d_members, d_status,
                                            stream))

    def dev_chain_seeds_tally(self, d_seed_off, d_seeds, n, max_seeds, lookback, max_gap, max_skew, min_score, d_n_chains, d_n_members, d_tally,
                              d_chain_off=None, d_member_off=None, d_chains=None, d_members=None, d_status=None, stream=None, slot=0):
        """dev_chain_seeds + census: d_tally[3] += (seeds chained, predecessor pairs evaluated, chains reported)"""
        _check(self._L.awry_dev_chain_seeds_tally(self._h, slot, d_seed_off, d_seeds, n, int(max_seeds), int(lookback), int(max_gap),
                                                  int(max_skew), int(min_score), d_n_chains, d_n_members, d_chain_off, d_member_off, d_chains,
                                                  d_members, d_status, d_tally, stream))

    # ------------------------------------------------------------------ locate within k edits (substitutions, insertions, deletions)
    def parallel_locate_edit_csr(self, qbytes: np.ndarray, qoff: np.ndarray, k: int, max_candidates: int, want_pos: bool = True):
        """-> (hit_off uint64[n+1], global_pos uint64[total], pos uint64[total, 2], edits uint8[total], status uint8[n]): the
        locally best starts of every query within k edits (include/awry_hip.h states the definition), ascending text position;
        status[i] == Q_CANDIDATE_CAP marks a query abandoned because its k + 1 pieces occur more than max_candidates times in all
        (it has no hits); want_pos=False leaves pos empty"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, hits, gp, ed, st = _u64p(), C.POINTER(_lib.Pos)(), _u64p(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
        _check(self._L.awry_locate_edit_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(k), int(max_candidates), C.byref(off),
                                              C.byref(hits) if want_pos else None, C.byref(gp), C.byref(ed), C.byref(st)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        g = _adopt(self._L, gp, tot, np.uint64)
        p = _adopt(self._L, hits, 2 * tot, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        return offs, g, p, _adopt(self._L, ed, tot, np.uint8), _adopt(self._L, st, n, np.uint8)

    def parallel_locate_edit(self, queries: Iterable, k: int, max_candidates: int):
        """-> per query, [(LocalizedSequencePosition, distance)] in ascending text position (empty for an abandoned query)"""
        off, _, p, d, _ = self.parallel_locate_edit_csr(*pack_queries(queries), k, max_candidates)
        return [[(LocalizedSequencePosition(int(a), int(b)), int(e)) for (a, b), e in zip(p[off[i]:off[i + 1]], d[off[i]:off[i + 1]])]
                for i in range(len(off) - 1)]

    def locate_string_edit(self, query, k: int, max_candidates: int):
        """-> [(LocalizedSequencePosition, distance)] of one query"""
        return self.parallel_locate_edit([query], k, max_candidates)[0]

    def count_string_edit(self, query, k: int, max_candidates: int) -> int:
        """hits of one query within k edits (0 for an abandoned query)"""
        return int(self.parallel_locate_edit_csr(*pack_queries([query]), k, max_candidates, want_pos=False)[0][-1])

    def dev_edit_windows(self, d_qbytes, d_qoff, d_win_query, d_win_first, d_win_count, m, k, d_n_hits, d_hit_off=None, d_gpos=None, d_edits=None,
                         stream=None, slot=0):
        """device-resident verify of candidate windows: d_hit_off None = the count pass (d_n_hits[m] u64); else the fill pass writing
        window w's hits at d_gpos (u64) / d_edits (u8) [d_hit_off[w], d_hit_off[w+1]); scan d_n_hits with dev_scan_counts in between"""
        _check(self._L.awry_dev_edit_windows(self._h, slot, d_qbytes, d_qoff, d_win_query, d_win_first, d_win_count, m, int(k), d_n_hits, d_hit_off,
                                             d_gpos, d_edits, stream))

    def dev_edit_windows_tally(self, d_qbytes, d_qoff, d_win_query, d_win_first, d_win_count, m, k, d_n_hits, d_tally, d_hit_off=None, d_gpos=None,
                               d_edits=None, stream=None, slot=0):
        """dev_edit_windows + census: d_tally[2] += (text columns scanned, windows scanned)"""
        _check(self._L.awry_dev_edit_windows_tally(self._h, slot, d_qbytes, d_qoff, d_win_query, d_win_first, d_win_count, m, int(k), d_n_hits,
                                                   d_hit_off, d_gpos, d_edits, d_tally, stream))

    # ------------------------------------------------------------------ align the hits within k edits: text span and CIGAR per hit
    def parallel_align_edit_csr(self, qbytes: np.ndarray, qoff: np.ndarray, k: int, max_candidates: int, want_pos: bool = True):
        """-> (hit_off, global_pos, pos, edits, status) exactly as parallel_locate_edit_csr, then text_len uint32[total], cigar_off
        uint64[total+1], cigar uint32[runs]: hit h matches T[global_pos[h] .. + text_len[h]) by the runs cigar[cigar_off[h] ..
        cigar_off[h+1]), each len << 4 | BAM op (include/awry_hip.h states the canonical script)"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        off, hits, gp, ed, st = _u64p(), C.POINTER(_lib.Pos)(), _u64p(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
        tl, coff, cg = C.POINTER(C.c_uint32)(), _u64p(), C.POINTER(C.c_uint32)()
        _check(self._L.awry_align_edit_batch(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(k), int(max_candidates), C.byref(off),
                                             C.byref(hits) if want_pos else None, C.byref(gp), C.byref(ed), C.byref(st), C.byref(tl), C.byref(coff),
                                             C.byref(cg)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        g = _adopt(self._L, gp, tot, np.uint64)
        p = _adopt(self._L, hits, 2 * tot, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        d, status = _adopt(self._L, ed, tot, np.uint8), _adopt(self._L, st, n, np.uint8)
        coffs = _adopt(self._L, coff, tot + 1, np.uint64)
        return offs, g, p, d, status, _adopt(self._L, tl, tot, np.uint32), coffs, _adopt(self._L, cg, int(coffs[-1]), np.uint32)

    def parallel_align_edit(self, queries: Iterable, k: int, max_candidates: int):
        """-> per query, [(LocalizedSequencePosition, distance, text_len, "57=1X43=")] in ascending text position (empty for an
        abandoned query)"""
        off, _, p, d, _, tl, coff, cg = self.parallel_align_edit_csr(*pack_queries(queries), k, max_candidates)
        return [[(LocalizedSequencePosition(int(p[h, 0]), int(p[h, 1])), int(d[h]), int(tl[h]), cigar_string(cg[coff[h]:coff[h + 1]]))
                 for h in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]

    def align_string_edit(self, query, k: int, max_candidates: int):
        """-> [(LocalizedSequencePosition, distance, text_len, CIGAR string)] of one query"""
        return self.parallel_align_edit([query], k, max_candidates)[0]

    def dev_edit_align(self, d_qbytes, d_qoff, d_hit_query, d_hit_gpos, d_hit_edits, m, k, d_text_len, d_n_ops, d_ops, stream=None, slot=0):
        """device-resident alignment of the triples (d_hit_query u32, d_hit_gpos u64, d_hit_edits u8)[m]: d_text_len[m] u32, d_n_ops[m] u8
        and the runs d_ops[h * ALIGN_MAX_OPS ..] u32; a triple that is no alignment at that distance gets d_n_ops = 0"""
        _check(self._L.awry_dev_edit_align(self._h, slot, d_qbytes, d_qoff, d_hit_query, d_hit_gpos, d_hit_edits, m, int(k), d_text_len, d_n_ops, d_ops,
                                           stream))

    def dev_edit_align_tally(self, d_qbytes, d_qoff, d_hit_query, d_hit_gpos, d_hit_edits, m, k, d_text_len, d_n_ops, d_ops, d_tally, stream=None,
                             slot=0):
        """dev_edit_align + census: d_tally[2] += (hits aligned, table cells computed)"""
        _check(self._L.awry_dev_edit_align_tally(self._h, slot, d_qbytes, d_qoff, d_hit_query, d_hit_gpos, d_hit_edits, m, int(k), d_text_len, d_n_ops,
                                                 d_ops, d_tally, stream))

    # ------------------------------------------------------------------ align chains: gap fill, end extension, CIGAR per chain
    def parallel_align_chains_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, max_alignments: int = 1,
                                  band: int = 4, max_seeds: int = 1024, lookback: int = 32, max_gap: int = 1000, max_skew: int = 100,
                                  min_score: int = 20, want_cigar: bool = True):
        """-> (aln_off uint64[n+1], chains CHAIN_DTYPE[total], alns ALN_DTYPE[total], cigar_off uint64[total+1], cigar uint32[runs],
        status uint8[n]): the first min(n_chains, max_alignments) chains of every query, primary first, as parallel_chains_csr
        reports them, each aligned base by base (include/awry_hip.h states the definition): alignment c covers
        T[alns[c].t_begin .. alns[c].t_end) with alns[c].edits edits by the runs cigar[cigar_off[c] .. cigar_off[c+1]), each
        len << 4 | BAM op; alns[c].status is ALN_OK, ALN_SKEW or ALN_BAD_CHAIN; want_cigar=False leaves cigar_off and cigar empty"""
        return self._align_chains_csr(None, qbytes, qoff, min_len, max_hits, max_alignments, band, max_seeds, lookback, max_gap, max_skew, min_score,
                                      want_cigar)

    def _align_chains_csr(self, clip, qbytes, qoff, min_len, max_hits, max_alignments, band, max_seeds, lookback, max_gap, max_skew, min_score, want_cigar):
        """awry_align_chains_batch (clip None), or awry_align_chains_clip_batch with clip = (match, mismatch, gap, end_bonus)"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        fn, rec, dt = ((self._L.awry_align_chains_batch, _lib.Aln, ALN_DTYPE) if clip is None else
                       (self._L.awry_align_chains_clip_batch, _lib.AlnClip, ALN_CLIP_DTYPE))
        off, ch, al, coff, cg, st = _u64p(), C.POINTER(_lib.Chain)(), C.POINTER(rec)(), _u64p(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        _check(fn(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), int(max_hits), int(max_seeds), int(lookback), int(max_gap),
                  int(max_skew), int(min_score), int(max_alignments), int(band), *(() if clip is None else [int(x) for x in clip]), C.byref(off),
                  C.byref(ch), C.byref(al), C.byref(coff) if want_cigar else None, C.byref(cg) if want_cigar else None, C.byref(st)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        chains = _adopt(self._L, ch, 32 * tot, np.uint8).view(CHAIN_DTYPE)
        alns = _adopt(self._L, al, dt.itemsize * tot, np.uint8).view(dt)
        status = _adopt(self._L, st, n, np.uint8)
        if not want_cigar:
            return offs, chains, alns, np.zeros(0, np.uint64), np.zeros(0, np.uint32), status
        coffs = _adopt(self._L, coff, tot + 1, np.uint64)
        return offs, chains, alns, coffs, _adopt(self._L, cg, int(coffs[-1]), np.uint32), status

    def parallel_align_chains(self, queries: Iterable, min_len: int = 12, max_hits: int = 50, max_alignments: int = 1, band: int = 4,
                              **chain_params):
        """-> per query, [(score, t_begin, t_end, edits, "57=1X43=", status)] of its first max_alignments chains, the primary first
        (none for an abandoned query); chain_params: max_seeds, lookback, max_gap, max_skew, min_score"""
        off, ch, al, coff, cg, _ = self.parallel_align_chains_csr(*pack_queries(queries), min_len, max_hits, max_alignments, band, **chain_params)
        return [[(int(ch[c]["score"]), int(al[c]["t_begin"]), int(al[c]["t_end"]), int(al[c]["edits"]), cigar_string(cg[coff[c]:coff[c + 1]]),
                  int(al[c]["status"])) for c in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]

    def align_chains_string(self, query, min_len: int = 12, max_hits: int = 50, max_alignments: int = 1, band: int = 4, **chain_params):
        """alignments of one query's chains"""
        return self.parallel_align_chains([query], min_len, max_hits, max_alignments, band, **chain_params)[0]

    def parallel_align_chains_clip_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, max_alignments: int = 1,
                                       band: int = 4, match: int = 1, mismatch: int = 4, gap: int = 6, end_bonus: int = 5, max_seeds: int = 1024,
                                       lookback: int = 32, max_gap: int = 1000, max_skew: int = 100, min_score: int = 20, want_cigar: bool = True):
        """parallel_align_chains_csr in the clipped mode (include/awry_hip.h, "soft-clip read ends"): the two end extensions are scored
        (match, mismatch, gap) and local, and may stop early unless the whole extension scores within end_bonus of the best cell; alns
        is ALN_CLIP_DTYPE -- t_begin / t_end span the aligned part, score, clip_left / clip_right -- and the runs may begin and end with
        an 'S' run (BAM op 4); an extension never reaches into another record"""
        return self._align_chains_csr((match, mismatch, gap, end_bonus), qbytes, qoff, min_len, max_hits, max_alignments, band, max_seeds, lookback,
                                      max_gap, max_skew, min_score, want_cigar)

    def parallel_align_chains_clip(self, queries: Iterable, min_len: int = 12, max_hits: int = 50, max_alignments: int = 1, band: int = 4,
                                   match: int = 1, mismatch: int = 4, gap: int = 6, end_bonus: int = 5, **chain_params):
        """-> per query, [(chain score, t_begin, t_end, edits, "70=31S", status, score, clip_left, clip_right)] of its first max_alignments
        chains in the clipped mode; chain_params: max_seeds, lookback, max_gap, max_skew, min_score"""
        off, ch, al, coff, cg, _ = self.parallel_align_chains_clip_csr(*pack_queries(queries), min_len, max_hits, max_alignments, band, match, mismatch,
                                                                       gap, end_bonus, **chain_params)
        return [[(int(ch[c]["score"]), int(al[c]["t_begin"]), int(al[c]["t_end"]), int(al[c]["edits"]), cigar_string(cg[coff[c]:coff[c + 1]]),
                  int(al[c]["status"]), int(al[c]["score"]), int(al[c]["clip_left"]), int(al[c]["clip_right"]))
                 for c in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]

    def dev_align_chains(self, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, band, d_alns, d_n_ops, d_cigar_off=None, d_cigar=None,
                         stream=None, slot=0):
        """device-resident alignment of the caller's chains (chain c: query d_chain_query[c] u32, members d_members[d_member_off[c] ..
        d_member_off[c+1]) as 16-byte seed records): d_cigar_off None = the count pass (d_alns[m] 24-byte records, d_n_ops[m] u64); else
        the fill pass writing the runs of chain c at d_cigar[d_cigar_off[c] ..); scan d_n_ops with dev_scan_counts in between"""
        _check(self._L.awry_dev_align_chains(self._h, slot, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, int(band), d_alns, d_n_ops,
                                             d_cigar_off, d_cigar, stream))

    def dev_align_chains_tally(self, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, band, d_alns, d_n_ops, d_tally, d_cigar_off=None,
                               d_cigar=None, stream=None, slot=0):
        """dev_align_chains + census: d_tally[2] += (chains aligned with status ALN_OK, table cells computed)"""
        _check(self._L.awry_dev_align_chains_tally(self._h, slot, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, int(band), d_alns,
                                                   d_n_ops, d_cigar_off, d_cigar, d_tally, stream))

    def dev_align_chains_clip(self, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, band, match, mismatch, gap, end_bonus, d_alns, d_n_ops,
                              d_cigar_off=None, d_cigar=None, stream=None, slot=0, d_tally=None):
        """dev_align_chains in the clipped mode: d_alns holds 32-byte ALN_CLIP_DTYPE records; d_tally (optional) as in dev_align_chains_tally"""
        _check(self._L.awry_dev_align_chains_clip_tally(self._h, slot, d_qbytes, d_qoff, d_chain_query, d_member_off, d_members, m, int(band), int(match),
                                                        int(mismatch), int(gap), int(end_bonus), d_alns, d_n_ops, d_cigar_off, d_cigar, d_tally, stream))

    # ------------------------------------------------------------------ map reads on both strands: ranked alignments, MAPQ
    def parallel_map_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4,
                         max_report: int = 1, band: int = 4, max_seeds: int = 1024, lookback: int = 32, max_gap: int = 1000, max_skew: int = 100,
                         min_score: int = 20, want_pos: bool = True, want_cigar: bool = True):
        """-> (map_off uint64[n+1], maps MAP_DTYPE[total], pos uint64[total, 2], cigar_off uint64[total+1], cigar uint32[runs], status
        uint8[n]): per read its best alignments over both strands, the primary first (include/awry_hip.h states the definition):
        record c covers T[t_begin .. t_end) with `edits` edits by the runs cigar[cigar_off[c] .. cigar_off[c+1]) -- for strand 1 of
        the read's reverse complement against the forward text -- pos[c] is the record and offset of t_begin, mapq the mapping
        quality (0 for secondaries, which carry MAP_SECONDARY in flags); status[i] == Q_SEED_CAP marks a read one of whose strands
        was abandoned at max_seeds; want_pos / want_cigar = False leave those arrays empty"""
        return self._map_csr(None, qbytes, qoff, min_len, max_hits, chains_per_strand, max_report, band, max_seeds, lookback, max_gap, max_skew, min_score,
                             want_pos, want_cigar)

    def _map_csr(self, clip, qbytes, qoff, min_len, max_hits, chains_per_strand, max_report, band, max_seeds, lookback, max_gap, max_skew, min_score,
                 want_pos, want_cigar, split=None):
        """awry_map_batch (clip None), or awry_map_clip_batch with clip = (match, mismatch, gap, end_bonus, min_aln_score), or
        awry_map_split_batch with that and split = (max_segments, max_secondary, max_overlap) in the place of max_report"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        fn, rec, dt = (self._L.awry_map_batch, _lib.Map, MAP_DTYPE) if clip is None else (self._L.awry_map_clip_batch, _lib.MapClip, MAP_CLIP_DTYPE)
        if split is not None:
            fn, rec, dt = self._L.awry_map_split_batch, _lib.MapSplit, MAP_SPLIT_DTYPE
        report = [int(max_report)] if split is None else [int(x) for x in split]
        off, mp, ps, coff, cg, st = _u64p(), C.POINTER(rec)(), C.POINTER(_lib.Pos)(), _u64p(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        _check(fn(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), int(max_hits), int(max_seeds), int(lookback), int(max_gap),
                  int(max_skew), int(min_score), int(chains_per_strand), *report, int(band), *(() if clip is None else [int(x) for x in clip]),
                  C.byref(off), C.byref(mp), C.byref(ps) if want_pos else None, C.byref(coff) if want_cigar else None,
                  C.byref(cg) if want_cigar else None, C.byref(st)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        maps = _adopt(self._L, mp, dt.itemsize * tot, np.uint8).view(dt)
        pos = _adopt(self._L, ps, 2 * tot, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        status = _adopt(self._L, st, n, np.uint8)
        if not want_cigar:
            return offs, maps, pos, np.zeros(0, np.uint64), np.zeros(0, np.uint32), status
        coffs = _adopt(self._L, coff, tot + 1, np.uint64)
        return offs, maps, pos, coffs, _adopt(self._L, cg, int(coffs[-1]), np.uint32), status

    def parallel_map(self, queries: Iterable, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4, max_report: int = 1, band: int = 4,
                     **chain_params):
        """-> per read, [(record, offset, strand, mapq, edits, "57=1X43=", flags)] of its reported alignments, the primary first (none
        for a read that maps nowhere); chain_params: max_seeds, lookback, max_gap, max_skew, min_score"""
        off, mp, pos, coff, cg, _ = self.parallel_map_csr(*pack_queries(queries), min_len, max_hits, chains_per_strand, max_report, band, **chain_params)
        return [[(int(pos[c][0]), int(pos[c][1]), int(mp[c]["strand"]), int(mp[c]["mapq"]), int(mp[c]["edits"]), cigar_string(cg[coff[c]:coff[c + 1]]),
                  int(mp[c]["flags"])) for c in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]

    def map_string(self, query, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4, max_report: int = 1, band: int = 4, **chain_params):
        """alignments of one read over both strands"""
        return self.parallel_map([query], min_len, max_hits, chains_per_strand, max_report, band, **chain_params)[0]

    def parallel_map_clip_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4,
                              max_report: int = 1, band: int = 4, match: int = 1, mismatch: int = 4, gap: int = 6, end_bonus: int = 5,
                              min_aln_score: int = 0, max_seeds: int = 1024, lookback: int = 32, max_gap: int = 1000, max_skew: int = 100,
                              min_score: int = 20, want_pos: bool = True, want_cigar: bool = True):
        """parallel_map_csr in the clipped mode (include/awry_hip.h, "soft-clip read ends"): maps is MAP_CLIP_DTYPE -- the aligned part's
        span, its score and the letters clipped at either end (for strand 1 of the read's reverse complement) -- a candidate needs score
        >= min_aln_score, the rank is by (-score, edits, strand, t_begin, chain index), mapq = min(60, 10 (s1 - s2) // (match + mismatch));
        with max_report >= 2 a chimeric read comes out as a primary and a secondary covering different parts of the read"""
        return self._map_csr((match, mismatch, gap, end_bonus, min_aln_score), qbytes, qoff, min_len, max_hits, chains_per_strand, max_report, band,
                             max_seeds, lookback, max_gap, max_skew, min_score, want_pos, want_cigar)

    def parallel_map_clip(self, queries: Iterable, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4, max_report: int = 1, band: int = 4,
                          match: int = 1, mismatch: int = 4, gap: int = 6, end_bonus: int = 5, min_aln_score: int = 0, **chain_params):
        """-> per read, [(record, offset, strand, mapq, edits, "70=31S", flags, score, clip_left, clip_right)] of its reported alignments in
        the clipped mode, the primary first; chain_params: max_seeds, lookback, max_gap, max_skew, min_score"""
        off, mp, pos, coff, cg, _ = self.parallel_map_clip_csr(*pack_queries(queries), min_len, max_hits, chains_per_strand, max_report, band, match,
                                                               mismatch, gap, end_bonus, min_aln_score, **chain_params)
        return [[(int(pos[c][0]), int(pos[c][1]), int(mp[c]["strand"]), int(mp[c]["mapq"]), int(mp[c]["edits"]), cigar_string(cg[coff[c]:coff[c + 1]]),
                  int(mp[c]["flags"]), int(mp[c]["score"]), int(mp[c]["clip_left"]), int(mp[c]["clip_right"]))
                 for c in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]

    def map_clip_string(self, query, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4, max_report: int = 1, band: int = 4, match: int = 1,
                        mismatch: int = 4, gap: int = 6, end_bonus: int = 5, min_aln_score: int = 0, **chain_params):
        """clipped alignments of one read over both strands"""
        return self.parallel_map_clip([query], min_len, max_hits, chains_per_strand, max_report, band, match, mismatch, gap, end_bonus, min_aln_score,
                                      **chain_params)[0]

    def dev_revcomp(self, d_qbytes, d_qoff, n, d_out_bytes, d_out_off, stream=None, slot=0):
        """device-resident doubled batch: query 2i of (d_out_bytes, d_out_off) is read i as given, query 2i + 1 its reverse
        complement; the caller sizes d_out_bytes at 2 x the reads' bytes and d_out_off at 2 n + 1 u64"""
        _check(self._L.awry_dev_revcomp(self._h, slot, d_qbytes, d_qoff, n, d_out_bytes, d_out_off, stream))

    def dev_map_select(self, d_aln_off, d_alns, d_chains, d_chain_status, n, chains_per_strand, max_report, d_n_maps, d_read_status=None,
                       d_map_off=None, d_maps=None, d_sel=None, d_pos=None, stream=None, slot=0):
        """device-resident rank / redundancy / report / MAPQ over the alignment records of a doubled batch of n reads (24-byte
        alignment and 32-byte chain records of query x at [d_aln_off[x], d_aln_off[x+1]), 2 n + 1 offsets): d_map_off None = the count
        pass (d_n_maps[n] u64, optional d_read_status[n]); else the fill pass writing 32-byte records at d_maps[d_map_off[i] ..) and,
        optionally, per record the alignment's index (d_sel, u32) and the position of t_begin (d_pos, 2 u64); scan d_n_maps with
        dev_scan_counts in between"""
        _check(self._L.awry_dev_map_select(self._h, slot, d_aln_off, d_alns, d_chains, d_chain_status, n, int(chains_per_strand), int(max_report),
                                           d_n_maps, d_read_status, d_map_off, d_maps, d_sel, d_pos, stream))

    def dev_map_select_clip(self, d_aln_off, d_alns, d_chains, d_chain_status, n, chains_per_strand, max_report, match, mismatch, gap, end_bonus,
                            min_aln_score, d_n_maps, d_read_status=None, d_map_off=None, d_maps=None, d_sel=None, d_pos=None, stream=None, slot=0):
        """dev_map_select in the clipped mode: 32-byte ALN_CLIP_DTYPE records in, 40-byte MAP_CLIP_DTYPE records out"""
        _check(self._L.awry_dev_map_select_clip(self._h, slot, d_aln_off, d_alns, d_chains, d_chain_status, n, int(chains_per_strand), int(max_report),
                                                int(match), int(mismatch), int(gap), int(end_bonus), int(min_aln_score), d_n_maps, d_read_status,
                                                d_map_off, d_maps, d_sel, d_pos, stream))

    # ------------------------------------------------------------------ split reads: supplementary alignments by query overlap
    def parallel_map_split_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4,
                               max_segments: int = 2, max_secondary: int = 0, max_overlap: int = 50, band: int = 4, match: int = 1, mismatch: int = 4,
                               gap: int = 6, end_bonus: int = 5, min_aln_score: int = 0, max_seeds: int = 1024, lookback: int = 32, max_gap: int = 1000,
                               max_skew: int = 100, min_score: int = 20, want_pos: bool = True, want_cigar: bool = True):
        """parallel_map_clip_csr with the selection by query interval (include/awry_hip.h, "split reads"): maps is MAP_SPLIT_DTYPE.  Per
        read first its segments -- up to max_segments clipped alignments that explain different letters [q_begin, q_end) of the read, the
        primary and then the supplementaries (MAP_SUPPLEMENTARY in flags), each with a mapq of its own -- then up to max_secondary
        secondaries (MAP_SECONDARY, mapq 0), each overlapping its segment `parent` (an index among the read's records) by at least
        max_overlap percent of the shorter of the two intervals"""
        return self._map_csr((match, mismatch, gap, end_bonus, min_aln_score), qbytes, qoff, min_len, max_hits, chains_per_strand, None, band, max_seeds,
                             lookback, max_gap, max_skew, min_score, want_pos, want_cigar, split=(max_segments, max_secondary, max_overlap))

    def parallel_map_split(self, queries: Iterable, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4, max_segments: int = 2,
                           max_secondary: int = 0, max_overlap: int = 50, band: int = 4, match: int = 1, mismatch: int = 4, gap: int = 6,
                           end_bonus: int = 5, min_aln_score: int = 0, **chain_params):
        """-> per read, [(record, offset, strand, mapq, edits, "60=41S", flags, score, q_begin, q_end, parent)] of its segments and then its
        secondaries; chain_params: max_seeds, lookback, max_gap, max_skew, min_score"""
        off, mp, pos, coff, cg, _ = self.parallel_map_split_csr(*pack_queries(queries), min_len, max_hits, chains_per_strand, max_segments, max_secondary,
                                                                max_overlap, band, match, mismatch, gap, end_bonus, min_aln_score, **chain_params)
        return [[(int(pos[c][0]), int(pos[c][1]), int(mp[c]["strand"]), int(mp[c]["mapq"]), int(mp[c]["edits"]), cigar_string(cg[coff[c]:coff[c + 1]]),
                  int(mp[c]["flags"]), int(mp[c]["score"]), int(mp[c]["q_begin"]), int(mp[c]["q_end"]), int(mp[c]["parent"]))
                 for c in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]

    def map_split_string(self, query, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4, max_segments: int = 2, max_secondary: int = 0,
                         max_overlap: int = 50, band: int = 4, match: int = 1, mismatch: int = 4, gap: int = 6, end_bonus: int = 5, min_aln_score: int = 0,
                         **chain_params):
        """segments and secondaries of one read over both strands"""
        return self.parallel_map_split([query], min_len, max_hits, chains_per_strand, max_segments, max_secondary, max_overlap, band, match, mismatch, gap,
                                       end_bonus, min_aln_score, **chain_params)[0]

    def dev_map_select_split(self, d_aln_off, d_alns, d_chains, d_chain_status, d_qoff, n, chains_per_strand, max_segments, max_secondary, max_overlap,
                             match, mismatch, min_aln_score, d_n_maps, d_read_status=None, d_map_off=None, d_maps=None, d_sel=None, d_pos=None, stream=None,
                             slot=0):
        """dev_map_select_clip with the split selection: 32-byte ALN_CLIP_DTYPE records in, 48-byte MAP_SPLIT_DTYPE records out; d_qoff
        holds the reads' own n + 1 offsets (u64), of which only the lengths are read"""
        _check(self._L.awry_dev_map_select_split(self._h, slot, d_aln_off, d_alns, d_chains, d_chain_status, d_qoff, n, int(chains_per_strand),
                                                 int(max_segments), int(max_secondary), int(max_overlap), int(match), int(mismatch), int(min_aln_score),
                                                 d_n_maps, d_read_status, d_map_off, d_maps, d_sel, d_pos, stream))

    # ------------------------------------------------------------------ map read pairs: insert-size pairing, mate rescue, proper-pair flag
    def parallel_map_pairs_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4,
                               band: int = 4, min_insert: int = 0, max_insert: int = 1000, unpaired_penalty: int = 4, rescue_anchors: int = 2,
                               rescue_edits: int = 4, max_seeds: int = 1024, lookback: int = 32, max_gap: int = 1000, max_skew: int = 100,
                               min_score: int = 20, want_pos: bool = True, want_cigar: bool = True):
        """the 2P reads interleaved (read 2p and 2p + 1 are the mates of pair p) -> (map_off uint64[2P+1], maps MAP_DTYPE[total], pos
        uint64[total, 2], cigar_off uint64[total+1], cigar uint32[runs], status uint8[2P], insert uint32[P]): at most one record per
        read, the placements of the best pair (include/awry_hip.h states the definition): both mates carry the pair MAPQ and
        MAP_PROPER_PAIR iff they lie on opposite strands of one record, forward first, min_insert <= outer distance <= max_insert
        (insert[p] is that distance, else 0); a mate found by rescue -- within rescue_edits edits where the insert size puts it --
        carries MAP_RESCUED; a read whose mate has no placement carries MAP_MATE_UNMAPPED and its single-end MAPQ"""
        return self._map_pairs_csr(None, qbytes, qoff, min_len, max_hits, chains_per_strand, band, min_insert, max_insert, unpaired_penalty, rescue_anchors,
                                   rescue_edits, max_seeds, lookback, max_gap, max_skew, min_score, want_pos, want_cigar)

    def _map_pairs_csr(self, clip, qbytes, qoff, min_len, max_hits, chains_per_strand, band, min_insert, max_insert, unpaired_penalty, rescue_anchors,
                       rescue_edits, max_seeds, lookback, max_gap, max_skew, min_score, want_pos, want_cigar):
        """awry_map_pairs_batch (clip None), or awry_map_pairs_clip_batch with clip = (match, mismatch, gap, end_bonus, min_aln_score)"""
        qb = np.ascontiguousarray(qbytes, dtype=np.uint8)
        qo = np.ascontiguousarray(qoff, dtype=np.uint64)
        n = len(qo) - 1
        fn, rec, dt = ((self._L.awry_map_pairs_batch, _lib.Map, MAP_DTYPE) if clip is None else
                       (self._L.awry_map_pairs_clip_batch, _lib.MapClip, MAP_CLIP_DTYPE))
        off, mp, ps, coff, cg, st = _u64p(), C.POINTER(rec)(), C.POINTER(_lib.Pos)(), _u64p(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        ins = C.POINTER(C.c_uint32)()
        _check(fn(self._h, qb.ctypes.data, qo.ctypes.data_as(_u64p), n, int(min_len), int(max_hits), int(max_seeds), int(lookback), int(max_gap),
                  int(max_skew), int(min_score), int(chains_per_strand), int(band), int(min_insert), int(max_insert), int(unpaired_penalty),
                  int(rescue_anchors), int(rescue_edits), *(() if clip is None else [int(x) for x in clip]), C.byref(off), C.byref(mp),
                  C.byref(ps) if want_pos else None, C.byref(coff) if want_cigar else None, C.byref(cg) if want_cigar else None, C.byref(st),
                  C.byref(ins)))
        offs = _adopt(self._L, off, n + 1, np.uint64)
        tot = int(offs[-1])
        maps = _adopt(self._L, mp, dt.itemsize * tot, np.uint8).view(dt)
        pos = _adopt(self._L, ps, 2 * tot, np.uint64).reshape(-1, 2) if want_pos else np.zeros((0, 2), np.uint64)
        status, insert = _adopt(self._L, st, n, np.uint8), _adopt(self._L, ins, n // 2, np.uint32)
        if not want_cigar:
            return offs, maps, pos, np.zeros(0, np.uint64), np.zeros(0, np.uint32), status, insert
        coffs = _adopt(self._L, coff, tot + 1, np.uint64)
        return offs, maps, pos, coffs, _adopt(self._L, cg, int(coffs[-1]), np.uint32), status, insert

    def parallel_map_pairs(self, reads1: Iterable, reads2: Iterable, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4, band: int = 4,
                           min_insert: int = 0, max_insert: int = 1000, unpaired_penalty: int = 4, rescue_anchors: int = 2, rescue_edits: int = 4,
                           **chain_params):
        """-> per pair (record of reads1[p] or None, record of reads2[p] or None, insert), a record in parallel_map's form: (record,
        offset, strand, mapq, edits, "57=1X43=", flags); chain_params: max_seeds, lookback, max_gap, max_skew, min_score"""
        r1, r2 = list(reads1), list(reads2)
        if len(r1) != len(r2):
            raise ValueError("reads1 and reads2 must have one read per pair each")
        off, mp, pos, coff, cg, _, ins = self.parallel_map_pairs_csr(*pack_queries([q for pair in zip(r1, r2) for q in pair]), min_len, max_hits,
                                                                     chains_per_strand, band, min_insert, max_insert, unpaired_penalty, rescue_anchors,
                                                                     rescue_edits, **chain_params)

        def rec(i):
            if off[i] == off[i + 1]:
                return None
            c = int(off[i])
            return (int(pos[c][0]), int(pos[c][1]), int(mp[c]["strand"]), int(mp[c]["mapq"]), int(mp[c]["edits"]), cigar_string(cg[coff[c]:coff[c + 1]]),
                    int(mp[c]["flags"]))
        return [(rec(2 * p), rec(2 * p + 1), int(ins[p])) for p in range(len(r1))]

    def dev_pair_windows(self, d_cand_off, d_cands, d_qoff, n_pairs, min_insert, max_insert, rescue_anchors, rescue_edits, d_win_query, d_win_first,
                         d_win_count, stream=None, slot=0):
        """device-resident rescue windows over the kept lists of 2 n_pairs interleaved reads (32-byte records of read i at [d_cand_off[i],
        d_cand_off[i+1]) in rank order; d_qoff: the reads' own 2 n_pairs + 1 offsets): slot (2p + m) * rescue_anchors + a = candidate a
        of mate m gets the doubled-batch query it seeks (d_win_query u32) and its window of starts (d_win_first u64, d_win_count u32;
        count 0 where the candidate is no anchor or the window is empty)"""
        _check(self._L.awry_dev_pair_windows(self._h, slot, d_cand_off, d_cands, d_qoff, n_pairs, int(min_insert), int(max_insert), int(rescue_anchors),
                                             int(rescue_edits), d_win_query, d_win_first, d_win_count, stream))

    def dev_pair_select(self, d_cand_off, d_cands, d_resc, d_read_status, n_pairs, min_insert, max_insert, unpaired_penalty, rescue_anchors, d_n_maps,
                        d_map_off=None, d_maps=None, d_sel=None, d_pos=None, d_insert=None, stream=None, slot=0):
        """device-resident pair choice over the kept lists and the rescued candidates d_resc[2 * rescue_anchors * n_pairs] (32-byte records
        per window slot, edits == 0xFFFFFFFF for none): d_map_off None = the count pass (d_n_maps[2 n_pairs] u64); else the fill pass
        writing read i's record at d_maps[d_map_off[i]] and, optionally, per record d_sel (u32: the index into d_cands, or 0x80000000 |
        slot for a rescued record) and d_pos (2 u64), and d_insert[n_pairs] (u32); scan d_n_maps with dev_scan_counts in between"""
        _check(self._L.awry_dev_pair_select(self._h, slot, d_cand_off, d_cands, d_resc, d_read_status, n_pairs, int(min_insert), int(max_insert),
                                            int(unpaired_penalty), int(rescue_anchors), d_n_maps, d_map_off, d_maps, d_sel, d_pos, d_insert, stream))

    def parallel_map_pairs_clip_csr(self, qbytes: np.ndarray, qoff: np.ndarray, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4,
                                    band: int = 4, min_insert: int = 0, max_insert: int = 1000, unpaired_penalty: int = 20, rescue_anchors: int = 2,
                                    rescue_edits: int = 4, match: int = 1, mismatch: int = 4, gap: int = 6, end_bonus: int = 5, min_aln_score: int = 0,
                                    max_seeds: int = 1024, lookback: int = 32, max_gap: int = 1000, max_skew: int = 100, min_score: int = 20,
                                    want_pos: bool = True, want_cigar: bool = True):
        """parallel_map_pairs_csr in the clipped mode (include/awry_hip.h, "map read pairs, clipped"): maps is MAP_CLIP_DTYPE, the kept
        lists are parallel_map_clip_csr's, the insert is measured between the mates' 5' ends projected through their clips (t_begin -
        clip_left of the forward mate to t_end + clip_right of the reverse one), unpaired_penalty is in score units, the best pair has the
        largest score + score - (unpaired_penalty if improper), mapq = min(60, 10 (S1 - S2) // (match + mismatch)); a rescued mate is a
        whole-read alignment within rescue_edits edits with score >= min_aln_score and clips 0"""
        return self._map_pairs_csr((match, mismatch, gap, end_bonus, min_aln_score), qbytes, qoff, min_len, max_hits, chains_per_strand, band, min_insert,
                                   max_insert, unpaired_penalty, rescue_anchors, rescue_edits, max_seeds, lookback, max_gap, max_skew, min_score, want_pos,
                                   want_cigar)

    def parallel_map_pairs_clip(self, reads1: Iterable, reads2: Iterable, min_len: int = 12, max_hits: int = 50, chains_per_strand: int = 4,
                                band: int = 4, min_insert: int = 0, max_insert: int = 1000, unpaired_penalty: int = 20, rescue_anchors: int = 2,
                                rescue_edits: int = 4, match: int = 1, mismatch: int = 4, gap: int = 6, end_bonus: int = 5, min_aln_score: int = 0,
                                **chain_params):
        """-> per pair (record of reads1[p] or None, record of reads2[p] or None, insert), a record in parallel_map_clip's form: (record,
        offset, strand, mapq, edits, "60=41S", flags, score, clip_left, clip_right); chain_params: max_seeds, lookback, max_gap, max_skew,
        min_score"""
        r1, r2 = list(reads1), list(reads2)
        if len(r1) != len(r2):
            raise ValueError("reads1 and reads2 must have one read per pair each")
        off, mp, pos, coff, cg, _, ins = self.parallel_map_pairs_clip_csr(*pack_queries([q for pair in zip(r1, r2) for q in pair]), min_len, max_hits,
                                                                          chains_per_strand, band, min_insert, max_insert, unpaired_penalty,
                                                                          rescue_anchors, rescue_edits, match, mismatch, gap, end_bonus, min_aln_score,
                                                                          **chain_params)

        def rec(i):
            if off[i] == off[i + 1]:
                return None
            c = int(off[i])
            return (int(pos[c][0]), int(pos[c][1]), int(mp[c]["strand"]), int(mp[c]["mapq"]), int(mp[c]["edits"]), cigar_string(cg[coff[c]:coff[c + 1]]),
                    int(mp[c]["flags"]), int(mp[c]["score"]), int(mp[c]["clip_left"]), int(mp[c]["clip_right"]))
        return [(rec(2 * p), rec(2 * p + 1), int(ins[p])) for p in range(len(r1))]

    def dev_pair_windows_clip(self, d_cand_off, d_cands, d_qoff, n_pairs, min_insert, max_insert, rescue_anchors, rescue_edits, d_win_query, d_win_first,
                              d_win_count, stream=None, slot=0):
        """dev_pair_windows in the clipped mode: 40-byte MAP_CLIP_DTYPE records in, the windows measured from the clipped fragment ends"""
        _check(self._L.awry_dev_pair_windows_clip(self._h, slot, d_cand_off, d_cands, d_qoff, n_pairs, int(min_insert), int(max_insert),
                                                  int(rescue_anchors), int(rescue_edits), d_win_query, d_win_first, d_win_count, stream))

    def dev_pair_select_clip(self, d_cand_off, d_cands, d_resc, d_read_status, n_pairs, min_insert, max_insert, unpaired_penalty, rescue_anchors, match,
                             mismatch, gap, end_bonus, min_aln_score, d_n_maps, d_map_off=None, d_maps=None, d_sel=None, d_pos=None, d_insert=None,
                             stream=None, slot=0):
        """dev_pair_select in the clipped mode: 40-byte MAP_CLIP_DTYPE records in d_cands, d_resc and d_maps, unpaired_penalty in score units"""
        _check(self._L.awry_dev_pair_select_clip(self._h, slot, d_cand_off, d_cands, d_resc, d_read_status, n_pairs, int(min_insert), int(max_insert),
                                                 int(unpaired_penalty), int(rescue_anchors), int(match), int(mismatch), int(gap), int(end_bonus),
                                                 int(min_aln_score), d_n_maps, d_map_off, d_maps, d_sel, d_pos, d_insert, stream))

    def debug_rank_all(self, rows: np.ndarray, slot=0) -> np.ndarray:
        """Occ of every non-sentinel symbol at each row through the kernels' all-symbol rank -> uint64[len(rows), S]
        (column s - 1 = symbol index s; S = 5 nucleotide, 21 amino)"""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        S = 5 if self.alphabet() == NUCLEOTIDE else 21
        if len(r) == 0:
            return np.zeros((0, S), np.uint64)
        d_r, d_o = self.dev_upload(r, slot), self.dev_malloc(8 * S * len(r), slot)
        try:
            _check(self._L.awry_debug_rank_all(self._h, slot, d_r, len(r), d_o, None))
            self.dev_synchronize(slot)
            return self.dev_download(d_o, (len(r), S), np.uint64, slot)
        finally:
            self.dev_free(d_r, slot)
            self.dev_free(d_o, slot)

    # ------------------------------------------------------------------ device-resident path
    def dev_malloc(self, nbytes, slot=0) -> int:
        p = C.c_void_p()
        _check(self._L.awry_dev_malloc(self._h, slot, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, ptr, slot=0):
        _check(self._L.awry_dev_free(self._h, slot, ptr))

    def dev_upload(self, arr: np.ndarray, slot=0) -> int:
        a = np.ascontiguousarray(arr)
        p = self.dev_malloc(a.nbytes, slot)
        _check(self._L.awry_dev_memcpy_h2d(self._h, slot, p, a.ctypes.data, a.nbytes))
        return p

    def dev_download(self, ptr, shape, dtype, slot=0) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        _check(self._L.awry_dev_memcpy_d2h(self._h, slot, out.ctypes.data, ptr, out.nbytes))
        return out

    def dev_memset(self, ptr, value, nbytes, slot=0):
        _check(self._L.awry_dev_memset(self._h, slot, ptr, value, nbytes))

    def dev_synchronize(self, slot=0):
        _check(self._L.awry_dev_synchronize(self._h, slot))

    def dev_pack_nt2(self, d_ascii, n, L, d_words, d_bad, stream=None, slot=0):
        _check(self._L.awry_dev_pack_nt2(self._h, slot, d_ascii, n, L, d_words, d_bad, stream))

    def dev_count_nt2(self, d_words, n, L, d_counts, use_seed=True, stream=None, slot=0):
        _check(self._L.awry_dev_count_nt2(self._h, slot, d_words, n, L, d_counts, 1 if use_seed else 0, stream))

    def dev_count_nt2_tally(self, d_words, n, L, d_counts, d_tally, use_seed=True, stream=None, slot=0):
        _check(self._L.awry_dev_count_nt2_tally(self._h, slot, d_words, n, L, d_counts, 1 if use_seed else 0, d_tally, stream))

    def dev_count_ascii(self, d_qbytes, d_qoff, n, d_counts, d_ranges=None, d_status=None, stream=None, slot=0):
        _check(self._L.awry_dev_count_ascii(self._h, slot, d_qbytes, d_qoff, n, d_counts, d_ranges, d_status, stream))

    def dev_count_ascii_for_locate(self, d_qbytes, d_qoff, n, d_counts, d_locate_words, d_status=None, stream=None, slot=0):
        """count pass of a device-resident parallel_locate: d_locate_words[2n] are opaque words for dev_locate (range_stride 2)"""
        _check(self._L.awry_dev_count_ascii_for_locate(self._h, slot, d_qbytes, d_qoff, n, d_counts, d_locate_words, d_status, stream))

    def dev_count_ascii_uniform(self, d_qbytes, n, length, d_counts, d_status=None, stream=None, slot=0):
        """n ASCII queries of `length` bytes each, back to back (amino k-mers: the two-phase schedule)"""
        _check(self._L.awry_dev_count_ascii_uniform(self._h, slot, d_qbytes, n, length, d_counts, d_status, stream))

    def dev_count_ascii_uniform_tally(self, d_qbytes, n, length, d_counts, d_tally, stream=None, slot=0):
        """amino k-mer schedule + census: d_tally[5] += (seed probes, steps, blocks ranked, SA reads, text comparisons)"""
        _check(self._L.awry_dev_count_ascii_uniform_tally(self._h, slot, d_qbytes, n, length, d_counts, d_tally, stream))

    def dev_scan_counts(self, d_counts, n, d_hit_off, d_scratch, stream=None, slot=0):
        _check(self._L.awry_dev_scan_counts(self._h, slot, d_counts, n, d_hit_off, d_scratch, stream))

    def dev_scan_scratch_bytes(self, n) -> int:
        return int(self._L.awry_dev_scan_scratch_bytes(n))

    def dev_locate(self, d_ranges, d_hit_off, n, total, d_gpos, d_pos=None, stream=None, slot=0, range_stride=2):
        _check(self._L.awry_dev_locate(self._h, slot, d_ranges, range_stride, d_hit_off, n, total, d_gpos, d_pos, stream))

    def dev_locate_tally(self, d_ranges, d_hit_off, n, total, d_gpos, d_pos, d_tally, stream=None, slot=0, range_stride=2):
        """dev_locate + the walk kernel's census: d_tally[2] += (LF steps, hits that walked)"""
        _check(self._L.awry_dev_locate_tally(self._h, slot, d_ranges, range_stride, d_hit_off, n, total, d_gpos, d_pos, d_tally, stream))

    def dev_phase_marker(self, phase_id, stream=None, slot=0):
        """profiling aid: an empty kernel whose grid size names a phase in rocprofv3 counter output"""
        _check(self._L.awry_dev_phase_marker(self._h, slot, phase_id, stream))

    def dev_count_nt2_long(self, d_words, n, L, d_counts, d_range_start=None, use_seed=True, stream=None, slot=0):
        _check(self._L.awry_dev_count_nt2_long(self._h, slot, d_words, n, L, d_counts, d_range_start, 1 if use_seed else 0, stream))

    def set_locate_sa_ratio(self, ratio: int):
        """device-side SA density for locate (0 = the file's samples); results do not depend on it"""
        _check(self._L.awry_set_locate_sa_ratio(self._h, ratio))

    def locate_sa_ratio(self) -> int:
        return self._L.awry_locate_sa_ratio(self._h)

    def set_lcx(self, on: bool):
        """left-context index on / off (performance knob; results do not depend on it)"""
        _check(self._L.awry_set_lcx(self._h, 1 if on else 0))

    def lcx_enabled(self) -> bool:
        return bool(self._L.awry_lcx_enabled(self._h))

    def set_kmer_table(self, mode: int):
        """k-mer count table (performance knob; results do not depend on it): -1 the policy (built by the first batch of 65536
        k-mers or more of a length), 0 off, 1 build for the length of the next launch whatever its size"""
        _check(self._L.awry_set_kmer_table(self._h, mode))

    def kmer_table_info(self, slot=0) -> dict:
        """the table resident on replica `slot`: its k-mer length (0: none), entries, lines, overflowed lines, bytes, build time"""
        info = (C.c_uint64 * 6)()
        _check(self._L.awry_kmer_table_info(self._h, slot, info))
        return {"length": int(info[0]), "entries": int(info[1]), "lines": int(info[2]), "overflowed_lines": int(info[3]),
                "bytes": int(info[4]), "build_ms": int(info[5]) / 1000.0}

    def debug_kmer_table(self, slot=0):
        """-> (uint64[lines * 16] the table resident on replica `slot`, copied; bits = log2(lines); its k-mer length L), or None
        when none is resident"""
        L, bits = C.c_int(0), C.c_uint32(0)
        for _ in range(4):  # (another launch may replace the table between the size query and the copy)
            _check(self._L.awry_debug_kmer_table(self._h, slot, None, 0, C.byref(L), C.byref(bits)))
            if L.value == 0:
                return None
            want = bits.value
            tab = np.empty(16 << want, np.uint64)
            _check(self._L.awry_debug_kmer_table(self._h, slot, tab.ctypes.data, len(tab), C.byref(L), C.byref(bits)))
            if L.value == 0:
                return None
            if bits.value <= want:  # (a larger one was not copied)
                return tab[:16 << bits.value], int(bits.value), int(L.value)
        raise AwryError(ERR_ARG, "the k-mer count table kept changing size while it was read")

    def debug_lcx(self, slot=0):
        """-> (keys uint64[bwt_len], rowpos uint64[bwt_len]) copied from replica `slot`, or None when it is not resident"""
        k, rp = C.c_void_p(), C.c_void_p()
        _check(self._L.awry_debug_lcx(self._h, slot, C.byref(k), C.byref(rp)))
        if not k.value:
            return None
        n = self.bwt_len()
        keys, rowpos = np.empty(n, np.uint64), np.empty(n, np.uint64)
        _check(self._L.awry_dev_memcpy_d2h(self._h, slot, keys.ctypes.data, k, n * 8))
        _check(self._L.awry_dev_memcpy_d2h(self._h, slot, rowpos.ctypes.data, rp, n * 8))
        return keys, rowpos

    def debug_accelerators(self, slot=0) -> dict:
        """replica `slot`'s device-only accelerators: device pointers (None: not resident) and sizes, the fields of
        awry_debug_accel_t by name; valid until the next call that rebuilds accelerators"""
        a = _lib.DebugAccel()
        _check(self._L.awry_debug_accelerators(self._h, slot, C.byref(a)))
        out = {n: getattr(a, n) for n, _ in _lib.DebugAccel._fields_}
        out["lcx_off"] = [int(x) for x in a.lcx_off]
        return out

    def debug_seed_table(self, slot=0):
        """-> the seed table of replica `slot`, copied: a structured array with fields sp and cnt (uint32, or uint64 for
        16-byte wide-row entries) of sigma^seed_k entries, or None when there is none"""
        a = self.debug_accelerators(slot)
        if not a["seed"]:
            return None
        word = np.uint64 if a["seed_entry_bytes"] == 16 else np.uint32
        n = (4 if self.alphabet() == NUCLEOTIDE else 21) ** a["seed_k"]
        return self.dev_download(a["seed"], (n,), np.dtype([("sp", word), ("cnt", word)]), slot)

    def debug_seed_rung(self, L: int, slot=0):
        """-> the table for nucleotide k-mers of L < seed k letters (built if absent) as debug_seed_table's array, or None
        where a launch would get none"""
        p = self._L.awry_debug_seed_rung(self._h, slot, int(L))
        if not p:
            return None
        return self.dev_download(p, (4 ** int(L),), np.dtype([("sp", np.uint32), ("cnt", np.uint32)]), slot)

    def debug_dense_sa(self, slot=0):
        """-> (uint32 SA[j * ratio] copied from replica `slot`, ratio), or None when no dense SA is resident"""
        p = self._L.awry_debug_dense_sa(self._h, slot)
        a = self.debug_accelerators(slot)
        if not p:
            return None
        ratio = int(a["dense_ratio"])
        return self.dev_download(p, ((self.bwt_len() + ratio - 1) // ratio,), np.uint32, slot), ratio

    def dev_stream_copy(self, d_dst, d_src, nbytes, stream=None, slot=0):
        _check(self._L.awry_dev_stream_copy(self._h, slot, d_dst, d_src, nbytes, stream))

    def set_verify(self, after_steps: int):
        """seed-and-verify for packed nucleotide reads (-1 = off); results do not depend on it"""
        _check(self._L.awry_set_verify(self._h, after_steps))

    def set_verify_kmers(self, on: bool):
        """let the k-mer (L <= 32) kernel use seed-and-verify too (pays off on batches of present k-mers)"""
        _check(self._L.awry_set_verify_kmers(self._h, 1 if on else 0))

    def verify_enabled(self) -> bool:
        return bool(self._L.awry_verify_enabled(self._h))

    def locate_reads_nt2(self, q2d: np.ndarray, use_seed=True, slot=0):
        """fixed-length ACGT reads uint8[n, L] of any L through the packed pipeline:
        pack -> seeded quad count -> scan -> tile locate.  -> (hit_off, global_pos, pos[total, 2])"""
        q2d = np.ascontiguousarray(q2d, dtype=np.uint8)
        n, L = q2d.shape
        W = (L + 31) // 32
        d_ascii = self.dev_upload(q2d.reshape(-1), slot)
        bufs = [d_ascii]
        try:
            d_words, d_counts, d_sp, d_bad = (self.dev_malloc(8 * n * W, slot), self.dev_malloc(8 * n, slot), self.dev_malloc(8 * n, slot),
                                              self.dev_malloc(8, slot))
            d_off, d_scr = self.dev_malloc(8 * (n + 1), slot), self.dev_malloc(self.dev_scan_scratch_bytes(n), slot)
            bufs += [d_words, d_counts, d_sp, d_bad, d_off, d_scr]
            self.dev_memset(d_bad, 0, 8, slot)
            self.dev_pack_nt2(d_ascii, n, L, d_words, d_bad, None, slot)
            self.dev_count_nt2_long(d_words, n, L, d_counts, d_sp, use_seed, None, slot)
            self.dev_scan_counts(d_counts, n, d_off, d_scr, None, slot)
            self.dev_synchronize(slot)
            if int(self.dev_download(d_bad, (1,), np.uint64, slot)[0]):
                raise AwryError(ERR_INVALID_QUERY, "reads contain bytes outside ACGT; use parallel_locate")
            off = self.dev_download(d_off, (n + 1,), np.uint64, slot)
            total = int(off[-1])
            d_g, d_p = self.dev_malloc(8 * max(total, 1), slot), self.dev_malloc(16 * max(total, 1), slot)
            bufs += [d_g, d_p]
            self.dev_locate(d_sp, d_off, n, total, d_g, d_p, None, slot, range_stride=1)
            self.dev_synchronize(slot)
            return off, self.dev_download(d_g, (total,), np.uint64, slot), self.dev_download(d_p, (total, 2), np.uint64, slot)
        finally:
            for p in bufs:
                self.dev_free(p, slot)

    def dev_timer_begin(self, stream=None, slot=0):
        _check(self._L.awry_dev_timer_begin(self._h, slot, stream))

    def dev_timer_end(self, stream=None, slot=0) -> float:
        ms = C.c_float()
        _check(self._L.awry_dev_timer_end(self._h, slot, stream, C.byref(ms)))
        return float(ms.value)

    # convenience: count packed-able fixed-length ACGT k-mers given as uint8[n, L] through the hot kernel
    def count_kmers_nt2(self, q2d: np.ndarray, use_seed=True, slot=0, tally=False):
        """fixed-length ACGT k-mers uint8[n, L <= 32] through the packed kernel -> counts; tally=True also returns the
        kernel's census uint64[5] = (seed probes, LF steps, ranked blocks, verify SA reads, verify text windows)"""
        q2d = np.ascontiguousarray(q2d, dtype=np.uint8)
        n, L = q2d.shape
        d_ascii = self.dev_upload(q2d.reshape(-1), slot)
        d_words, d_counts, d_bad = self.dev_malloc(8 * n, slot), self.dev_malloc(8 * n, slot), self.dev_malloc(8, slot)
        d_tally = self.dev_malloc(64, slot) if tally else None
        try:
            self.dev_memset(d_bad, 0, 8, slot)
            self.dev_pack_nt2(d_ascii, n, L, d_words, d_bad, None, slot)
            self.dev_synchronize(slot)
            bad = int(self.dev_download(d_bad, (1,), np.uint64, slot)[0])
            if bad:
                raise AwryError(ERR_INVALID_QUERY, "%d queries contain bytes outside ACGT; use parallel_count" % bad)
            if tally:
                self.dev_memset(d_tally, 0, 64, slot)
                self.dev_count_nt2_tally(d_words, n, L, d_counts, d_tally, use_seed, None, slot)
            else:
                self.dev_count_nt2(d_words, n, L, d_counts, use_seed, None, slot)
            self.dev_synchronize(slot)
            counts = self.dev_download(d_counts, (n,), np.uint64, slot)
            return (counts, self.dev_download(d_tally, (5,), np.uint64, slot)) if tally else counts
        finally:
            for p in (d_ascii, d_words, d_counts, d_bad, d_tally):
                if p is not None:
                    self.dev_free(p, slot)
