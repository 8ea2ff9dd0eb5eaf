"""The order of the argument checks of the chain / align chains / map / split / pairs entry points, without a GPU: calls with two or
three bad arguments at once on a host-built index with no replica, faults adjacent in the order the entry points check them (null
argument, null query bytes, min_len, max_hits, chain parameters, map / split / align parameters, pair parameters, clip weights, the
cigar pair, the driver's own checks).  The first failing check's message is the one reported."""
import ctypes as C

import pytest

from awry_amd import _lib
from awry_amd.fm_index import BUILD_HOST, ERR_ARG, ERR_INVALID_QUERY, ERR_NO_DEVICE, FmIndex, pack_queries
from tests import synth

CHAIN = dict(min_len=12, max_hits=50, max_seeds=100, lookback=16, max_gap=100, max_skew=0, min_score=1)
CLIP = dict(match=1, mismatch=4, gap=6, end_bonus=5)
PAIR = dict(min_insert=0, max_insert=1000, unpaired_penalty=4, rescue_anchors=2, rescue_edits=4)
# the scalar arguments of every entry point between n and the result arrays, in the header's order, at values that pass
SCALARS = {
    "awry_chain_batch": dict(CHAIN),
    "awry_align_chains_batch": dict(CHAIN, max_alignments=1, band=4),
    "awry_align_chains_clip_batch": dict(CHAIN, max_alignments=1, band=4, **CLIP),
    "awry_map_batch": dict(CHAIN, chains_per_strand=4, max_report=1, band=4),
    "awry_map_clip_batch": dict(CHAIN, chains_per_strand=4, max_report=1, band=4, **CLIP, min_aln_score=0),
    "awry_map_split_batch": dict(CHAIN, chains_per_strand=4, max_segments=2, max_secondary=0, max_overlap=50, band=4, **CLIP, min_aln_score=0),
    "awry_map_pairs_batch": dict(CHAIN, chains_per_strand=4, band=4, **PAIR),
    "awry_map_pairs_clip_batch": dict(CHAIN, chains_per_strand=4, band=4, **PAIR, **CLIP, min_aln_score=0),
}
ALL = tuple(SCALARS)
ALIGNED = ALL[1:]  # the calls with a cigar pair: result arrays 3 and 4
MAPPED = ALL[3:]
CLIPPED = tuple(n for n in ALL if "match" in SCALARS[n])
PAIRED = ALL[6:]

NULL_ARG, NULL_BYTES = "null argument", "null query bytes"
MIN_LEN = "min_len must be at least 1"
MAX_HITS = "max_hits must be at least 1 (a one-letter match has a quarter of the text as hits)"
MAX_SEEDS, LOOKBACK = "max_seeds must be in 1..4096 (AWRY_CHAIN_MAX_SEEDS)", "lookback must be in 1..64 (AWRY_CHAIN_MAX_LOOKBACK)"
MAX_GAP, MIN_SCORE = "max_gap must be at least 1", "min_score must be at least 1"
SEED_PAIR = "seed_off_out and seeds_out are given or omitted together"
MAX_ALNS, BAND = "max_alignments must be at least 1", "band must be in 0..8 (AWRY_CHAIN_ALIGN_MAX_BAND)"
CPS, MAX_REPORT = "chains_per_strand must be in 1..8 (AWRY_MAP_MAX_CHAINS)", "max_report must be in 1 .. 2 * chains_per_strand"
SEGMENTS, SECONDARY = "max_segments must be in 1..4 (AWRY_SPLIT_MAX_SEGMENTS)", "max_secondary must be in 0 .. 2 * chains_per_strand"
OVERLAP = "max_overlap is a percentage in 1..100"
MAX_INSERT, MIN_INSERT = "max_insert must be at most 2^20 (AWRY_PAIR_MAX_INSERT)", "min_insert must not exceed max_insert"
UNPAIRED, UNPAIRED_CLIP = "unpaired_penalty must be in 0..255", "unpaired_penalty must be in 0..16384 (AWRY_PAIR_CLIP_MAX_UNPAIRED)"
ANCHORS, RESCUE_EDITS = "rescue_anchors must be in 0..4 (AWRY_PAIR_MAX_ANCHORS)", "rescue_edits must be in 0..8 (AWRY_MAX_EDITS)"
MATCH, PENALTY = "match must be in 1..16 (AWRY_CLIP_MAX_MATCH)", "mismatch and gap must be in 0..64 (AWRY_CLIP_MAX_PENALTY)"
END_BONUS = "end_bonus must be in 0..1024 (AWRY_CLIP_MAX_END_BONUS)"
CIGAR_PAIR = "cigar_off_out and cigar_out are given or omitted together"
ODD = "read pairs are interleaved: an odd number of reads"
AMINO_MAP, AMINO_PAIRS = "mapping on both strands needs a nucleotide index", "mapping read pairs needs a nucleotide index"
TOO_LONG = "query 1: longer than 1024 letters (AWRY_CHAIN_ALIGN_MAX_LEN)"
NO_DEVICE = "no device replica: call awry_set_devices() first (there is no CPU search path)"


@pytest.fixture(scope="module")
def world():
    t, st, hd = synth.make_text(2_000, 0, 61, 1, 0.0)
    ix = FmIndex.from_text(t, 0, 8, 0, st, hd, build_device=BUILD_HOST)  # no set_devices: no replica
    t, st, hd = synth.make_text(1_000, 1, 5, 1, 0.0)
    aa = FmIndex.from_text(t, 1, 8, 0, st, hd, build_device=BUILD_HOST)
    reads = dict(two=pack_queries([b"ACGTACGTACGT", b"GATTACAGATTACA"]), three=pack_queries([b"ACGTACGTACGT", b"GATTACAGATTACA", b"ACGTACGTACGT"]),
                 long=pack_queries([b"ACGTACGTACGT", b"ACGT" * 257]), long3=pack_queries([b"ACGTACGTACGT", b"ACGT" * 257, b"ACGTACGTACGT"]))
    yield ix, aa, reads
    ix.close()
    aa.close()


def call(world, name, reads="two", index="nt", null=(), half_cigar=False, half_seeds=False, **bad):
    """-> (return code, awry_last_error()) of entry point `name` with the scalars of SCALARS[name] but for **bad; null: of "idx", "qbytes",
    "qoff", "off_out"; half_cigar: cigar_off_out given, cigar_out omitted; half_seeds: the same of awry_chain_batch's seed arrays"""
    ix, aa, packed = world
    L = _lib.load_library()
    fn = getattr(L, name)
    scalars = dict(SCALARS[name])
    assert set(bad) <= set(scalars), (name, bad)
    scalars.update(bad)
    qb, qo = packed[reads]
    holders = [t._type_() for t in fn.argtypes[4 + len(scalars):]]
    outs = [C.byref(h) for h in holders]
    if "off_out" in null:
        outs[0] = None
    if half_cigar:
        outs[4] = None
    if half_seeds:
        outs[3] = None
    rc = fn(None if "idx" in null else (ix if index == "nt" else aa)._h, None if "qbytes" in null else qb.ctypes.data,
            None if "qoff" in null else qo.ctypes.data_as(C.POINTER(C.c_uint64)), len(qo) - 1, *scalars.values(), *outs)
    assert not any(holders), (name, bad)  # the out-pointers of a failed call stay as they were
    return rc, L.awry_last_error().decode()


def expect(world, names, message, code=ERR_ARG, **kw):
    for name in names:
        assert call(world, name, **kw) == (code, message), (name, kw)


def test_the_calls_pass_their_checks_at_the_table_s_values(world):
    """what is left to fail is the missing replica: every fault below is the argument's"""
    expect(world, ALL, NO_DEVICE, code=ERR_NO_DEVICE)


def test_null_arguments_come_first(world):
    for null in (("idx",), ("qoff",), ("off_out",), ("idx", "qbytes"), ("qoff", "qbytes"), ("off_out", "qbytes")):
        expect(world, ALL, NULL_ARG, null=null, min_len=0)
    expect(world, ALL, NULL_BYTES, null=("qbytes",), min_len=0)
    expect(world, ALL, NULL_BYTES, null=("qbytes",), min_len=0, max_hits=0, reads="three")


def test_seeding_and_chaining_parameters_in_their_order(world):
    expect(world, ALL, MIN_LEN, min_len=0, max_hits=0)
    expect(world, ALL, MIN_LEN, min_len=0, max_hits=0, lookback=0)
    expect(world, ALL, MAX_HITS, max_hits=0, lookback=0)
    expect(world, ALL, MAX_HITS, max_hits=0, max_seeds=0)
    expect(world, ALL, MAX_SEEDS, max_seeds=4097, lookback=65)
    expect(world, ALL, LOOKBACK, lookback=0, max_gap=0)
    expect(world, ALL, MAX_GAP, max_gap=0, min_score=0)
    expect(world, ALIGNED, MIN_SCORE, min_score=0, band=9)
    expect(world, MAPPED, LOOKBACK, lookback=65, chains_per_strand=9)
    expect(world, ALL[1:3], MAX_GAP, max_gap=0, max_alignments=0)
    expect(world, ["awry_chain_batch"], MIN_SCORE, min_score=0, half_seeds=True)
    expect(world, ["awry_chain_batch"], SEED_PAIR, half_seeds=True)


def test_map_split_and_align_parameters_before_pair_parameters_and_clip_weights(world):
    expect(world, ALL[1:3], MAX_ALNS, max_alignments=0, band=9)
    expect(world, ["awry_align_chains_batch"], BAND, band=9, half_cigar=True)
    expect(world, ["awry_align_chains_clip_batch"], BAND, band=9, match=0)
    expect(world, ["awry_map_batch", "awry_map_clip_batch"], CPS, chains_per_strand=9, max_report=0)
    expect(world, ["awry_map_batch", "awry_map_clip_batch"], MAX_REPORT, max_report=9, band=9)
    expect(world, ["awry_map_batch"], BAND, band=9, half_cigar=True)
    expect(world, [n for n in CLIPPED if n in MAPPED], CPS, chains_per_strand=9, match=0)
    expect(world, [n for n in CLIPPED if n in MAPPED], BAND, band=9, match=0)
    expect(world, ["awry_map_split_batch"], CPS, chains_per_strand=0, max_segments=5)
    expect(world, ["awry_map_split_batch"], SEGMENTS, max_segments=5, max_secondary=9)
    expect(world, ["awry_map_split_batch"], SECONDARY, max_secondary=9, max_overlap=0)
    expect(world, ["awry_map_split_batch"], OVERLAP, max_overlap=101, band=9)
    expect(world, ["awry_map_split_batch"], BAND, band=9, mismatch=65, half_cigar=True)
    expect(world, PAIRED, CPS, chains_per_strand=9, rescue_edits=9)
    expect(world, PAIRED, BAND, band=9, max_insert=(1 << 20) + 1)
    expect(world, PAIRED, BAND, band=9, rescue_edits=9, half_cigar=True)


def test_pair_parameters_before_clip_weights_and_the_cigar_pair(world):
    expect(world, PAIRED, MAX_INSERT, max_insert=(1 << 20) + 1, min_insert=(1 << 20) + 2)
    expect(world, PAIRED, MIN_INSERT, min_insert=501, max_insert=500, unpaired_penalty=16385)
    expect(world, ["awry_map_pairs_batch"], UNPAIRED, unpaired_penalty=256, rescue_anchors=5)
    expect(world, ["awry_map_pairs_clip_batch"], UNPAIRED_CLIP, unpaired_penalty=16385, rescue_anchors=5)
    expect(world, PAIRED, ANCHORS, rescue_anchors=5, rescue_edits=9)
    expect(world, ["awry_map_pairs_batch"], RESCUE_EDITS, rescue_edits=9, half_cigar=True)
    expect(world, ["awry_map_pairs_batch"], RESCUE_EDITS, rescue_edits=-1, half_cigar=True, reads="three")
    expect(world, ["awry_map_pairs_clip_batch"], RESCUE_EDITS, rescue_edits=9, match=17)
    expect(world, ["awry_map_pairs_clip_batch"], RESCUE_EDITS, rescue_edits=9, match=17, half_cigar=True)


def test_clip_weights_before_the_cigar_pair(world):
    expect(world, CLIPPED, MATCH, match=17, half_cigar=True)
    expect(world, CLIPPED, MATCH, match=0, mismatch=65)
    expect(world, CLIPPED, PENALTY, mismatch=65, end_bonus=1025)
    expect(world, CLIPPED, PENALTY, gap=65, end_bonus=1025, half_cigar=True)
    expect(world, CLIPPED, END_BONUS, end_bonus=1025, half_cigar=True)
    expect(world, CLIPPED, END_BONUS, end_bonus=1025, half_cigar=True, reads="long")


def test_the_cigar_pair_before_the_driver_s_own_checks(world):
    expect(world, ALIGNED, CIGAR_PAIR, half_cigar=True)
    expect(world, ALIGNED, CIGAR_PAIR, half_cigar=True, reads="long")
    expect(world, MAPPED, CIGAR_PAIR, half_cigar=True, index="aa")
    expect(world, PAIRED, CIGAR_PAIR, half_cigar=True, reads="three")
    expect(world, PAIRED, CIGAR_PAIR, half_cigar=True, reads="long3", index="aa")


def test_the_driver_s_own_checks_come_last_and_in_their_order(world):
    # an odd read count with any earlier fault
    expect(world, PAIRED, NULL_BYTES, reads="three", null=("qbytes",))
    expect(world, PAIRED, MIN_LEN, reads="three", min_len=0)
    expect(world, PAIRED, MAX_HITS, reads="three", max_hits=0)
    expect(world, PAIRED, MIN_SCORE, reads="three", min_score=0)
    expect(world, PAIRED, CPS, reads="three", chains_per_strand=0)
    expect(world, PAIRED, RESCUE_EDITS, reads="three", rescue_edits=9)
    expect(world, ["awry_map_pairs_clip_batch"], END_BONUS, reads="three", end_bonus=1025)
    expect(world, PAIRED, ODD, reads="three")
    # alphabet, odd read count, read lengths, and then the missing replica
    expect(world, ALL[3:6], AMINO_MAP, index="aa", reads="long")
    expect(world, PAIRED, AMINO_PAIRS, index="aa", reads="three")
    expect(world, PAIRED, ODD, reads="long3")
    expect(world, ALIGNED, TOO_LONG, reads="long", code=ERR_INVALID_QUERY)
    expect(world, ["awry_chain_batch"], NO_DEVICE, reads="long", code=ERR_NO_DEVICE)
