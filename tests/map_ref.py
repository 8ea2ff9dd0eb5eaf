"""Reference for mapping on both strands (include/awry_hip.h, "map reads on both strands"): the definition in plain Python
integers, on top of tests/chain_ref.py and tests/chain_align_ref.py.

rc() is the reverse complement on bytes through the symbol indices; rank_candidates() is the pure ranking function -- rank,
redundancy, report and MAPQ over the per-strand alignment lists, whoever computed them; map_reads() feeds it with the reference's
chains and alignments of a read and of its reverse complement.  A candidate is (strand, j, edits, chain score, t_begin, t_end); a
record is (t_begin, t_end, edits, chain score, j, strand, mapq, flags), the fields of awry_map_t in their order."""
import numpy as np

from tests import chain_align_ref as ca
from tests import chain_ref as cr
from tests import mismatch_ref as mr

MAP_MAX_CHAINS, MAP_SECONDARY, MAPQ_MAX = 8, 1, 60
Q_OK, Q_SEED_CAP = 0, cr.Q_SEED_CAP
NT_LETTERS = b"$ACGNT"
COMP = (0, 5, 3, 2, 4, 1)  # $ -> $, A -> T, C -> G, G -> C, N -> N, T -> A

MAP_NP = np.dtype([("t_begin", "<u8"), ("t_end", "<u8"), ("edits", "<u4"), ("chain_score", "<u4"), ("chain_index", "<u4"), ("strand", "u1"),
                   ("mapq", "u1"), ("flags", "<u2")])


def index_of_ascii(b):
    """the nucleotide symbol index of a byte: case folded, U == T, '#' == '$', anything else N"""
    c = b - 32 if 97 <= b <= 122 else b
    return {36: 0, 35: 0, 65: 1, 67: 2, 71: 3, 84: 5, 85: 5}.get(c, 4)


def rc(q):
    return bytes(NT_LETTERS[COMP[index_of_ascii(b)]] for b in reversed(bytes(q)))


def canonical(q):
    return bytes(NT_LETTERS[index_of_ascii(b)] for b in bytes(q))


def doubled(reads):
    """the doubled batch: query 2i = read i as given, query 2i + 1 = rc(read i)"""
    return [x for q in reads for x in (bytes(q), rc(q))]


def rank_candidates(cands, capped, R):
    """cands: [(strand, j, edits, score, t_begin, t_end)] (status OK only) -> (records, kept count)"""
    order = sorted(cands, key=lambda c: (c[2], -c[3], c[0], c[4], c[1]))
    kept = []
    for c in order:
        if any(k[0] == c[0] and max(k[4], c[4]) < min(k[5], c[5]) for k in kept):
            continue
        kept.append(c)
    out = []
    for r, (s, j, e, sc, tb, te) in enumerate(kept[:R]):
        mapq = 0
        if r == 0 and not capped:
            mapq = MAPQ_MAX if len(kept) < 2 else min(MAPQ_MAX, 10 * (kept[1][2] - e))
        out.append((tb, te, e, sc, j, s, mapq, MAP_SECONDARY if r else 0))
    return out, len(kept)


def candidates_of(per_strand, A):
    """per_strand: for s in (0, 1) the list [(score, status, t_begin, t_end, edits)] of the strand's alignments, primary first"""
    return [(s, j, e, sc, tb, te) for s in (0, 1) for j, (sc, st, tb, te, e) in enumerate(per_strand[s][:A]) if st == ca.ALN_OK]


def rank_alignments(aln_off, chains, alns, chain_status, n, A, R):
    """the pure ranking over the arrays awry_align_chains_batch returns for the doubled batch of n reads
    -> (map_off uint64[n+1], records MAP_NP, per record the index of its alignment, status uint8[n])"""
    off, rows, sel, st = [0], [], [], []
    for i in range(n):
        per = []
        for s in (0, 1):
            lo, hi = int(aln_off[2 * i + s]), int(aln_off[2 * i + s + 1])
            per.append([(int(chains[c]["score"]), int(alns[c]["status"]), int(alns[c]["t_begin"]), int(alns[c]["t_end"]), int(alns[c]["edits"]))
                        for c in range(lo, hi)])
        capped = Q_SEED_CAP in (int(chain_status[2 * i]), int(chain_status[2 * i + 1]))
        recs, _ = rank_candidates(candidates_of(per, A), capped, R)
        rows += recs
        sel += [int(aln_off[2 * i + r[5]]) + r[4] for r in recs]
        off.append(off[-1] + len(recs))
        st.append(Q_SEED_CAP if capped else Q_OK)
    return np.array(off, np.uint64), np.array(rows, MAP_NP) if rows else np.zeros(0, MAP_NP), sel, np.array(st, np.uint8)


def align_strand(tsym, q, status_chains, A, W, memo=None):
    """one strand: tests/chain_ref.py's (status, chains) of q -> (status, [(score, aln status, t_begin, t_end, edits)], [runs])"""
    status, chains = status_chains
    out, runs = [], []
    qs = None
    for c in chains[:A]:
        key = (bytes(q), tuple(c[6]), W)
        if memo is None or key not in memo:
            qs = qs if qs is not None else [int(v) for v in mr.to_symbols(bytes(q), 0)]
            got = ca.align_chain(tsym, qs, list(c[6]), W)
            if memo is not None:
                memo[key] = got
        else:
            got = memo[key]
        s, tb, te, ed, r, _ = got
        out.append((c[0], s, tb, te, ed))
        runs.append(r)
    return status, out, runs


def map_reads(tsym, reads, chains_of, A, R, W, memo=None):
    """chains_of(queries) -> tests/chain_ref.py's [(status, chains)] per query.  -> per read (status, [record], [runs per record])"""
    qs = doubled(reads)
    per = chains_of(qs)
    out = []
    for i in range(len(reads)):
        strands = [align_strand(tsym, qs[2 * i + s], per[2 * i + s], A, W, memo) for s in (0, 1)]
        capped = Q_SEED_CAP in (strands[0][0], strands[1][0])
        recs, _ = rank_candidates(candidates_of([strands[0][1], strands[1][1]], A), capped, R)
        out.append((Q_SEED_CAP if capped else Q_OK, recs, [strands[r[5]][2][r[4]] for r in recs]))
    return out


def as_csr(per_read):
    """[(status, records, runs)] -> (map_off, records MAP_NP, cigar_off, cigar uint32, status)"""
    off, rows, coff, cg, st = [0], [], [0], [np.zeros(0, np.uint32)], []
    for status, recs, runs in per_read:
        st.append(status)
        rows += recs
        for r in runs:
            cg.append(ca.encode(r))
            coff.append(coff[-1] + len(r))
        off.append(off[-1] + len(recs))
    return (np.array(off, np.uint64), np.array(rows, MAP_NP) if rows else np.zeros(0, MAP_NP), np.array(coff, np.uint64), np.concatenate(cg),
            np.array(st, np.uint8))
