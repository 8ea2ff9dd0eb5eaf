"""The kernel launches of the read pipelines' batch drivers, for comparing two builds of the library: one call each of
awry_locate_smems_batch, awry_chain_batch, awry_align_chains_batch (with CIGARs), awry_map_batch (with everything),
awry_locate_edit_batch and awry_locate_mismatch_batch, of 200 reads of 101 letters on a 50-kbp text, on one replica.
usage: rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/launch_sequence.py     run under a kernel trace
       python3 tools/launch_sequence.py --list <dir>      -> the traced launches in dispatch order, one `kernel grid` line each
Two builds drive the kernels alike when the two lists are equal (diff them)."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    import numpy as np

    import awry_amd
    from awry_amd.fm_index import pack_queries
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
        reads.append(bytes(q) if len(reads) % 2 else bytes(q[::-1]).translate(bytes.maketrans(b"ACGT", b"TGCA")))
    qb, qo = pack_queries(reads)
    short = pack_queries([r[:25] for r in reads])
    sizes = [int(ix.parallel_locate_smems_csr(qb, qo, 50, 12)[2][-1]), int(ix.parallel_chains_csr(qb, qo, 12, 50)[0][-1]),
             int(ix.parallel_align_chains_csr(qb, qo, 12, 50, 3, 4)[0][-1]), int(ix.parallel_map_csr(qb, qo, 12, 50, 4, 2, 4)[0][-1]),
             int(ix.parallel_locate_edit_csr(qb, qo, 3, 10 ** 6)[0][-1]), int(ix.parallel_locate_mismatch_csr(*short, 2)[0][-1])]
    assert all(sizes), sizes  # every pipeline ran all of its stages
    print("hits, chains, alignments, records, edit hits, mismatch hits:", sizes)
    ix.close()


def listing(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"])


if __name__ == "__main__":
    listing(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--list" else run()
