"""worker for tests/test_inflight_gpu.py::test_generic_host_drivers_in_a_child_process: started once as a fresh process
with AWRY_HOST_PATH=generic (the knob is read once per process) and AWRY_TRACE_HOST=1.  Builds a nucleotide and an amino
index, runs parallel_count_csr / parallel_locate_csr on every batch of cases() -- first from one thread, then from NTHREADS
threads at once, each with batches of its own -- and writes what it got as .npy files into the directory given as argv[1].
Computes no reference: the parent compares the files with the oracle.  Exits non-zero on any exception."""
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import synth  # noqa: E402

NTHREADS = 4


def callers():
    return ["single"] + ["thread%d" % t for t in range(NTHREADS)]


def cases():
    """-> [(name, alphabet, text, seq_starts, headers, {caller: [(batch name, qbytes, qoff)]})]; seeded, so that the parent
    rebuilds exactly what the child ran"""
    out = []
    text, st, hd = synth.make_text(400000, 0, 61, 3, 0.05)
    batches = {}
    for c, who in enumerate(callers()):
        L = (31, 12, 32, 40, 101)[c]
        clean = np.concatenate([synth.sampled_queries(text, 3000, L, L + c), synth.random_queries(3000, L, 0, L + 1 + c)])
        dirty = clean.copy()
        dirty[7, 3] = ord("N"); dirty[100, 0] = ord("u"); dirty[2999, L - 1] = ord("R")
        dirty[11] = np.frombuffer(bytes(dirty[11]).lower(), np.uint8)
        batches[who] = [("clean", *synth.fixed_to_csr(clean)), ("dirty", *synth.fixed_to_csr(dirty))]
    out.append(("nt", 0, text, st, hd, batches))
    text, st, hd = synth.make_text(300000, 1, 62, 40, 0.0)
    batches = {}
    for c, who in enumerate(callers()):
        q = np.concatenate([synth.sampled_queries(text, 6000, 12, 200 + c, True, 1), synth.random_queries(2192, 12, 1, 300 + c)])
        batches[who] = [("kmers", *synth.fixed_to_csr(q))]  # 8 192 12-mers: the amino two-phase schedule
    out.append(("aa", 1, text, st, hd, batches))
    return out


def main():
    out_dir = sys.argv[1]
    assert os.environ.get("AWRY_HOST_PATH") == "generic", "start this worker with AWRY_HOST_PATH=generic"
    from awry_amd.fm_index import FmIndex
    built = [(name, FmIndex.from_text(text, alphabet, 8, 0, st, hd).set_devices([0]), batches)
             for name, alphabet, text, st, hd, batches in cases()]
    errors = []

    def run(who):
        try:
            for name, ix, batches in built:
                for bname, qb, qo in batches[who]:
                    counts = ix.parallel_count_csr(qb, qo)
                    off, g, p = ix.parallel_locate_csr(qb, qo)
                    for a, v in (("counts", counts), ("off", off), ("gpos", g), ("pos", p)):
                        np.save(os.path.join(out_dir, "%s_%s_%s_%s.npy" % (name, bname, who, a)), np.array(v))
        except BaseException:  # noqa: BLE001
            errors.append((who, traceback.format_exc()))

    run("single")
    if not errors:
        threads = [threading.Thread(target=run, args=("thread%d" % t,)) for t in range(NTHREADS)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    for who, tb in errors:
        print("worker %s failed:\n%s" % (who, tb), file=sys.stderr)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
