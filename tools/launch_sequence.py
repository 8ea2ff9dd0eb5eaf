"""The kernel launches of the read pipelines' batch drivers, for comparing two builds of the library: one call each of
awry_locate_smems_batch, awry_chain_batch, awry_align_chains_batch (with CIGARs), awry_map_batch (with everything),
awry_locate_edit_batch and awry_locate_mismatch_batch, of 200 reads of 101 letters on a 50-kbp text, on one replica; then, with
positions and CIGARs, awry_map_clip_batch on the same reads, awry_map_split_batch on reads of which every fourth is two 50-letter
windows from different places joined together, and awry_map_pairs_batch and awry_map_pairs_clip_batch on 100 pairs of 96-letter mates
from fragments of 200 to 600 letters, where in every eighth pair one mate has a substitution every 11th letter, so that only rescue
places it (the scheme of tools/time_pairs.py).
usage: rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/launch_sequence.py     run under a kernel trace
       python3 tools/launch_sequence.py --list <dir>      -> the traced launches in dispatch order, one `kernel grid` line each
Two builds drive the kernels alike when the two lists are equal (diff them)."""
import csv
import glob
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RC = bytes.maketrans(b"ACGT", b"TGCA")


def substituted(q, places):
    q = bytearray(q)
    for at in places:
        q[at] = b"ACGT"[(b"ACGT".index(q[at]) + 1) % 4]
    return bytes(q)


def window(text, rng, length):
    """a window of the text free of anything but ACGT"""
    while True:
        p = int(rng.integers(0, len(text) - length - 1))
        if all(c in b"ACGT" for c in text[p:p + length]):
            return bytes(text[p:p + length])


def split_reads(text, rng, n=200):
    """windows of 100 letters with three substitutions; every fourth read two 50-letter windows from different places"""
    return [window(text, rng, 50) + window(text, rng, 50) if i % 4 == 3 else substituted(window(text, rng, 100), rng.integers(0, 100, size=3)) for i in range(n)]


def read_pairs(text, rng, n_pairs=100):
    """interleaved mates of 96 letters from the two ends of fragments of 200..600 letters, three substitutions each, the right mate
    reverse-complemented, every second pair in the other order; in every eighth pair one mate -- the two in turn -- has a substitution
    every 11th letter instead: no exact run reaches min_len = 12, and that is 8 edits"""
    out = []
    for p in range(n_pairs):
        frag = window(text, rng, int(rng.integers(200, 601)))
        mates = [frag[:96], frag[-96:]]
        for m in (0, 1):
            hard = p % 8 == 3 and (p // 8) % 2 == m
            mates[m] = substituted(mates[m], range(10, 96, 11) if hard else rng.integers(0, 96, size=3))
        fwd, rev = mates[0], mates[1][::-1].translate(RC)
        out += [rev, fwd] if p % 2 else [fwd, rev]
    return out


def run():
    import numpy as np

    import awry_amd
    from awry_amd.fm_index import MAP_RESCUED, MAP_SUPPLEMENTARY, pack_queries
    from tests import synth

    text, st, hd = synth.make_text(50_000, 0, 21, 5, 0.03)
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    rng = np.random.default_rng(1)
    reads = []
    while len(reads) < 200:  # windows of the text with three substitutions, every second one reverse-complemented by hand
        p = int(rng.integers(0, len(text) - 102))
        q = bytearray(text[p:p + 101])
        if any(c not in b"ACGT" for c in q):
            continue
        for at in rng.integers(0, 101, size=3):
            q[at] = b"ACGT"[(b"ACGT".index(q[at]) + 1) % 4]
        reads.append(bytes(q) if len(reads) % 2 else bytes(q[::-1]).translate(RC))
    qb, qo = pack_queries(reads)
    short = pack_queries([r[:25] for r in reads])
    sizes = [int(ix.parallel_locate_smems_csr(qb, qo, 50, 12)[2][-1]), int(ix.parallel_chains_csr(qb, qo, 12, 50)[0][-1]),
             int(ix.parallel_align_chains_csr(qb, qo, 12, 50, 3, 4)[0][-1]), int(ix.parallel_map_csr(qb, qo, 12, 50, 4, 2, 4)[0][-1]),
             int(ix.parallel_locate_edit_csr(qb, qo, 3, 10 ** 6)[0][-1]), int(ix.parallel_locate_mismatch_csr(*short, 2)[0][-1])]
    assert all(sizes), sizes  # every pipeline ran all of its stages
    print("hits, chains, alignments, records, edit hits, mismatch hits:", sizes)
    # the clipped, split and paired calls, with positions and CIGARs
    clip = ix.parallel_map_clip_csr(qb, qo, 12, 50, 4, 2, 4)
    split = ix.parallel_map_split_csr(*pack_queries(split_reads(bytes(text), rng)), 12, 50, 4, 2, 0, 50, 4)
    pq = pack_queries(read_pairs(bytes(text), rng))
    pairs = ix.parallel_map_pairs_csr(*pq, 12, 50, 4, 4, 0, 1000, 4, 2, 8)
    pairs_clip = ix.parallel_map_pairs_clip_csr(*pq, 12, 50, 4, 4, 0, 1000, 20, 2, 8)
    sizes = [int(r[0][-1]) for r in (clip, split, pairs, pairs_clip)] + [int(r[4].size) for r in (clip, split, pairs, pairs_clip)]
    assert all(sizes), sizes
    supplementary = int(((split[1]["flags"] & MAP_SUPPLEMENTARY) != 0).sum())
    assert supplementary, "no split read came out in two segments"
    for r in (pairs, pairs_clip):  # both CIGAR sources ran: the aligner's slots and the fill pass over chain-derived records
        rescued = int(((r[1]["flags"] & MAP_RESCUED) != 0).sum())
        assert 0 < rescued < len(r[1]), (rescued, len(r[1]))
    print("records of the clipped, split, paired and clipped paired calls, and their CIGAR runs:", sizes, "supplementary:", supplementary, "rescued:", rescued)
    ix.close()


def short_name(name):
    """a kernel's name without its parameter list (the template arguments stay) and without `void ` and `awry::`; of a name that is
    still longer than 100 letters (rocprim's) the first 60 and a hash of the whole: the lists are a sixth of the bytes and as distinct"""
    full = name
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                name = name[:i]
                break
    name = name.replace("void ", "").replace("awry::", "")
    return name if len(name) <= 100 else name[:60] + "...#" + hashlib.sha256(full.encode()).hexdigest()[:12]


def listing(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print(short_name(r["Kernel_Name"]), r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"])


if __name__ == "__main__":
    listing(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--list" else run()
