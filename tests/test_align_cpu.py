"""The alignment of edit-distance hits without a GPU: on planted reads the banded table of tests/align_ref.py gives the full
table's span and script, and the properties include/awry_hip.h states hold (no 'D' at either end, exactly d operations other
than '=', |text_len - L| <= d, at most 2d + 1 runs, gaps left-normalised); cigar_string round-trips; the C ABI declares and
exports the entry points, and the argument / no-replica errors come back as status codes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awry_amd import _lib, cigar_string
from awry_amd.fm_index import ALIGN_MAX_OPS, BUILD_HOST, ERR_ARG, ERR_NO_DEVICE, AwryError, FmIndex, pack_queries
from tests import align_ref as al
from tests import edit_ref as er
from tests import mismatch_ref as mr
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("awry_align_edit_batch", "awry_dev_edit_align", "awry_dev_edit_align_tally")


def planted(rng, text, letters, L, edits):
    """a read of about L letters: the text somewhere, with `edits` random substitutions, insertions and deletions"""
    p = int(rng.integers(0, len(text) - L - 1))
    q = bytearray(text[p:p + L])
    for _ in range(edits):
        kind, j = int(rng.integers(0, 3)), int(rng.integers(0, len(q)))
        if kind == 0:
            q[j] = int(letters[(int(np.nonzero(letters == q[j])[0][0]) + 1) % len(letters)]) if q[j] in bytes(letters) else int(letters[0])
        elif kind == 1:
            q.insert(j, int(letters[rng.integers(0, len(letters))]))
        elif len(q) > 1:
            del q[j]
    return bytes(q)


def check_hit(t, q, s, d):
    """full table == banded table, and the stated properties; -> the runs"""
    qs = mr.to_symbols(q, t.alphabet)
    L = len(qs)
    full = al.script(al.table(t.sym, qs, s, d), t.sym, qs, s, d)
    band = al.script(al.table(t.sym, qs, s, d, band=True), t.sym, qs, s, d)
    assert full is not None and full == band, (q, s, d, full, band)
    text_len, runs = full
    assert int(er.distances(t.sym[s:s + text_len], qs)[0]) <= d  # the span holds an alignment at that distance
    assert sum(ln for ln, c in runs if c != "=") == d
    assert sum(ln for ln, c in runs if c != "D") == L and sum(ln for ln, c in runs if c != "I") == text_len
    assert abs(text_len - L) <= d and 1 <= len(runs) <= 2 * d + 1 <= ALIGN_MAX_OPS
    assert runs[0][1] != "D" and runs[-1][1] != "D"
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:]))
    return runs


@pytest.mark.parametrize("alphabet,seed", [(0, 81), (1, 82)])
def test_banded_table_equals_full_table_and_the_properties_hold(alphabet, seed):
    rng = np.random.default_rng(seed)
    text, _, _ = synth.make_text(3_000, alphabet, seed, 3, 0.01)
    t = er.Text(text, alphabet)
    letters = synth.NT if alphabet == 0 else synth.AA
    hits = 0
    for L, k in ((9, 8), (12, 3), (20, 1), (33, 5), (64, 8), (65, 2), (101, 3), (101, 8)):
        for e in sorted({0, 1, k // 2, k}):
            q = planted(rng, text, letters, L, e)
            if len(q) <= k:
                continue
            p, d = er.hits_of(t.D(q), k)
            for s, dist in zip(p[:12], d[:12]):
                check_hit(t, q, int(s), int(dist))
                hits += 1
    assert hits >= 25  # every planted read has at least one hit (27 reads, fewer where deletions leave one no longer than k)


def test_the_vectorised_reference_equals_the_cell_by_cell_one():
    rng = np.random.default_rng(86)
    text, _, _ = synth.make_text(1_500, 0, 86, 2, 0.01)
    t = er.Text(text, 0)
    n, total = t.n, 0
    qs = [planted(rng, text, synth.NT, L, e) for L, e in ((6, 1), (9, 2), (18, 4), (40, 3), (101, 5))]
    qs += [bytes(text[n - 30:n]) + b"ACG", b"GT" + bytes(text[:25]), bytes(text[:9])]  # the text's two ends
    for q in qs:
        for k in (2, 5, 8):
            if len(q) <= k:
                continue
            p, d = er.hits_of(t.D(q), k)
            tls, runs = al.align_many(t, q, p, d)
            for h in range(0, len(p), max(1, len(p) // 40)):
                tl, r = al.align_triple(t, q, int(p[h]), int(d[h]))
                assert tl == int(tls[h]) and np.array_equal(r, runs[h]), (q, k, int(p[h]))
                total += 1
    assert total > 200


def test_gaps_are_left_normalised_and_ties_take_the_diagonal():
    body = b"GATTACAGGCTCTTGACCGT" + b"AC" * 10 + b"TTGCAGGCATCGGATCAAGT" + b"A" * 12 + b"CGTTGCATGCCTAGGATCCA"
    t = er.Text(np.frombuffer(body + b"$", np.uint8), 0)

    def cigars(q, k):
        p, d = er.hits_of(t.D(q), k)
        return {int(s): al.cigar_text(check_hit(t, q, int(s), int(e))) for s, e in zip(p, d)}

    q = b"CTTGACCGT" + b"AC" * 9 + b"TTGCAGGCA"  # one unit of the array deleted from the read: the text's extra unit is a 'D'
    assert cigars(q, 2)[11] == "9=2D27="           # ... at the array's left end
    q = b"CTTGACCGT" + b"AC" * 11 + b"TTGCAGGCA"  # one unit more in the read
    assert cigars(q, 2)[11] == "9=2I29="
    q = b"GGCATCGGATCAAGT" + b"A" * 13 + b"CGTTGCATG"  # a homopolymer one longer in the read
    assert cigars(q, 1)[45] == "15=1I21="
    q = b"GGCATCGGATCAAGT" + b"A" * 11 + b"CGTTGCATG"
    assert cigars(q, 1)[45] == "15=1D20="
    q = b"GATTACAGGCTCTTGACCGT"
    assert cigars(q, 3) == {0: "20="}
    q = b"GATTACAGGCTGTTGACCGT"
    assert cigars(q, 1) == {0: "11=1X8="}


def test_a_triple_that_is_no_alignment_has_no_script():
    text, _, _ = synth.make_text(2_000, 0, 83, 1, 0.0)
    t = er.Text(text, 0)
    q = bytes(text[500:540])
    assert al.align_triple(t, q, 500, 0)[0] == 40 and al.cigar_text([(40, "=")]) == "40="
    for s, d in ((500, 1), (700, 2), (t.n, 0), (t.n + 5, 1)):  # a wrong distance, a start that is no hit, starts >= n
        for band in (False, True):
            tl, runs = al.align_triple(t, q, s, d, band)
            assert tl == 0 and len(runs) == 0


def test_cigar_string_round_trips():
    rng = np.random.default_rng(84)
    for _ in range(50):
        runs = [(int(rng.integers(1, 300)), "=XID"[int(rng.integers(0, 4))]) for _ in range(int(rng.integers(1, ALIGN_MAX_OPS + 1)))]
        s = cigar_string(al.encode(runs))
        assert s == al.cigar_text(runs)
        assert [(int(n), c) for n, c in re.findall(r"(\d+)([=XID])", s)] == runs
    assert cigar_string(np.zeros(0, np.uint32)) == "" and cigar_string([57 << 4 | 7, 1 << 4 | 8, 43 << 4 | 7]) == "57=1X43="


def test_header_declares_and_library_exports_the_entry_points():
    L = _lib.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols(), name
        assert getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "awry_hip.h")).read()
    for word in ("AWRY_ALIGN_MAX_OPS = 17", "Banded table", "No 'D' at either end", "left-normalised", "I = 1, D = 2, '=' = 7, X = 8"):
        assert word in header, word
    for method in ("parallel_align_edit_csr", "parallel_align_edit", "align_string_edit", "dev_edit_align", "dev_edit_align_tally"):
        assert callable(getattr(FmIndex, method))


@pytest.fixture(scope="module")
def hostonly_index():
    text, st, hd = synth.make_text(2_000, 0, 85, 1, 0.0)
    return FmIndex.from_text(text, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica


def raw_call(ix, qb, qo, k, cap, want_coff=True, want_cigar=True):
    L = _lib.load_library()
    u64p, u8p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    out = [u64p(), C.POINTER(_lib.Pos)(), u64p(), u8p(), u8p(), u32p(), u64p(), u32p()]
    refs = [C.byref(o) for o in out]
    if not want_coff:
        refs[6] = None
    if not want_cigar:
        refs[7] = None
    rc = L.awry_align_edit_batch(ix._h, qb.ctypes.data, qo.ctypes.data_as(u64p), len(qo) - 1, k, cap, *refs)
    assert not any(bool(o) for o in out)  # the out-pointers of a failed call stay as they were
    return rc


def test_argument_errors_come_before_the_missing_replica(hostonly_index):
    qb, qo = pack_queries([b"ACGTACGTACGT"])
    for k, cap in ((-1, 100), (9, 100), (1, 0)):
        assert raw_call(hostonly_index, qb, qo, k, cap) == ERR_ARG
        with pytest.raises(AwryError) as e:
            hostonly_index.parallel_align_edit_csr(qb, qo, k, cap)
        assert e.value.code == ERR_ARG
    assert raw_call(hostonly_index, qb, qo, 1, 100, want_coff=False) == ERR_ARG  # one cigar pointer without the other
    assert raw_call(hostonly_index, qb, qo, 1, 100, want_cigar=False) == ERR_ARG
    assert raw_call(hostonly_index, qb, qo, 1, 100) == ERR_NO_DEVICE
    assert raw_call(hostonly_index, qb, qo, 1, 100, want_coff=False, want_cigar=False) == ERR_NO_DEVICE
    for call in (lambda: hostonly_index.dev_edit_align(None, None, None, None, None, 0, 9, None, None, None),
                 lambda: hostonly_index.dev_edit_align_tally(None, None, None, None, None, 0, -1, None, None, None, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_ARG
    for call in (lambda: hostonly_index.parallel_align_edit_csr(qb, qo, 1, 100), lambda: hostonly_index.parallel_align_edit([b"ACGT"], 0, 5),
                 lambda: hostonly_index.align_string_edit(b"ACGT", 1, 5),
                 lambda: hostonly_index.dev_edit_align(None, None, None, None, None, 0, 1, None, None, None),
                 lambda: hostonly_index.dev_edit_align_tally(None, None, None, None, None, 0, 1, None, None, None, None)):
        with pytest.raises(AwryError) as e:
            call()
        assert e.value.code == ERR_NO_DEVICE


def test_cpp_mirror_method_compiles(tmp_path):
    src = tmp_path / "align.cpp"
    src.write_text('#include <string>\n#include <vector>\n#include "awry.hpp"\n'
                   "uint64_t use(awry::FmIndex& ix) {\n"
                   '  std::vector<std::string> qs{"ACGTACGTACGT", "GATTACAGATTACA"};\n'
                   "  uint64_t s = 0;\n"
                   "  std::vector<uint8_t> status;\n"
                   "  for (auto& per : ix.parallel_align_edit(qs, 2, 1000, &status))\n"
                   "    for (const awry::FmIndex::EditAlignment& h : per) {\n"
                   "      s += h.position.sequence_idx() + h.position.local_position() + h.global_position + h.edits + h.text_len + h.cigar_string().size();\n"
                   "      for (uint32_t op : h.cigar) s += op >> 4;\n"
                   "    }\n"
                   "  for (uint8_t st : status) s += st == AWRY_Q_CANDIDATE_CAP;\n"
                   "  return s + ix.parallel_align_edit(qs, 0, 10).size() + AWRY_ALIGN_MAX_OPS;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
