"""Host cost of one tiny packed k-mer launch: queues `launches` awry_dev_count_nt2 launches of `nq` 31-mers on one stream, then
synchronises; wall time per launch, `reps` times.  The kernels are tiny, so the figure is what the host spends per launch
(the schedule decision, scratch bookkeeping, the launch itself).  Prints one JSON line.

    python tools/time_count_launch.py [launches=2000] [nq=64] [reps=3]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import awry_amd
from tests import synth

launches = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
L = 31
text, st, hd = synth.make_text(1_000_000, 0, 11, 1, 0.02)
ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
q2d = synth.sampled_queries(text, nq, L, 5)
d_ascii = ix.dev_upload(q2d.reshape(-1))
d_words, d_counts, d_bad = ix.dev_malloc(8 * nq), ix.dev_malloc(8 * nq), ix.dev_malloc(8)
ix.dev_memset(d_bad, 0, 8)
ix.dev_pack_nt2(d_ascii, nq, L, d_words, d_bad)
for _ in range(200):  # first uses
    ix.dev_count_nt2(d_words, nq, L, d_counts, True)
ix.dev_synchronize()
us = []
for _ in range(reps):
    t0 = time.perf_counter()
    for _ in range(launches):
        ix.dev_count_nt2(d_words, nq, L, d_counts, True)
    ix.dev_synchronize()
    us.append((time.perf_counter() - t0) / launches * 1e6)
counts = ix.dev_download(d_counts, (nq,), np.uint64)
assert (counts >= 1).all(), "k-mers of the text must be found"
print(json.dumps({"schedule": ix.count_schedule(L), "launches": launches, "queries_per_launch": nq, "us_per_launch": [round(u, 3) for u in us],
                  "median_us": round(float(np.median(us)), 3)}), flush=True)
