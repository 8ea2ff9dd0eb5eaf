"""Rates of the alignment pass over edit-distance hits (awry_align_edit_batch, kernels_align.hip.h) on the workload of
tools/time_edit.py: the repeat-rich GRCh38-shaped text (tests/synth.repeat_rich_text, as bench.py), 101-bp reads with 3 edits --
2 substitutions and 1 insertion or deletion -- at k = 3, 5, 8 and max_candidates = MAX_CANDIDATES.  Per k:
  * awry_align_edit_batch next to awry_locate_edit_batch on the same batch in the same process, alternating, REPS times each: wall
    times (transfers included) and their medians; the difference is the cost of the feature;
  * the alignment pass alone through awry_dev_edit_align on the hits of that batch, resident on the device in query order:
    device-event time, hits aligned per second, and table cells per second from the census.
usage: time_align.py [text_len] [n_reads] [k,k,..]   -> one JSON object on stdout"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import awry_amd
from awry_amd.fm_index import ALIGN_MAX_OPS
from tests import synth
from tools.read_sets import L, plant, timed
from tools.time_edit import with_indel

FULL = 3_100_000_000
MAX_CANDIDATES = 1000
REPS = 3
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else FULL
nq = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
ks = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [3, 5, 8]


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def wall(fn):
    t = time.time()
    r = fn()
    return time.time() - t, r


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("text + index + replica %.1f s" % (time.time() - t))
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "full_size_text": n == FULL, "n_reads": nq, "read_len": L,
           "reads": "windows of the text with 2 substitutions and 1 insertion or deletion", "max_candidates": MAX_CANDIDATES, "seed_k": ix.seed_kmer_len(),
           "host_reps": REPS, "k": {}}
    text_d = torch.from_numpy(text).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(503)
    pos = torch.randint(0, text_d.numel() - 2 - L, (nq,), device=dev, generator=gen)
    wide = text_d[pos[:, None] + torch.arange(L + 1, device=dev)[None, :]]
    reads = with_indel(torch.cat([plant(wide[:, :L].contiguous(), 2, 7), wide[:, L:]], 1), 9)
    del text_d, wide
    off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * L
    flat = torch.cat([reads.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    qb = reads.reshape(-1).cpu().numpy()
    qo = np.arange(nq + 1, dtype=np.uint64) * np.uint64(L)
    for k in ks:
        ix.parallel_align_edit_csr(qb[:L * 1000], qo[:1001], k, MAX_CANDIDATES, want_pos=False)  # warm
        ix.parallel_locate_edit_csr(qb[:L * 1000], qo[:1001], k, MAX_CANDIDATES, want_pos=False)
        loc_s, al_s = [], []
        for _ in range(REPS):
            s, loc = wall(lambda: ix.parallel_locate_edit_csr(qb, qo, k, MAX_CANDIDATES, want_pos=False))
            loc_s.append(s)
            s, al = wall(lambda: ix.parallel_align_edit_csr(qb, qo, k, MAX_CANDIDATES, want_pos=False))
            al_s.append(s)
        assert all(np.array_equal(a, b) for a, b in zip(al[:5], loc))
        hoff, g, _, d, status, tl, coff, cg = al
        m = len(g)
        leg = {"locate_edit_batch_s": loc_s, "align_edit_batch_s": al_s, "locate_edit_batch_median_s": float(np.median(loc_s)),
               "align_edit_batch_median_s": float(np.median(al_s)), "feature_cost_s": float(np.median(al_s) - np.median(loc_s)),
               "share_abandoned": float((status != 0).mean()), "hits": m, "hits_per_read": m / nq, "runs_per_hit": len(cg) / max(m, 1),
               "mean_distance": float(d.mean()) if m else 0.0}
        hq = torch.from_numpy(np.repeat(np.arange(nq, dtype=np.uint32), np.diff(hoff.astype(np.int64))).view(np.int32)).to(dev)
        hg = torch.from_numpy(g.view(np.int64)).to(dev)
        he = torch.from_numpy(d).to(dev)
        d_tl = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
        d_n = torch.zeros(max(m, 1), dtype=torch.uint8, device=dev)
        d_ops = torch.zeros(max(m, 1) * ALIGN_MAX_OPS, dtype=torch.int32, device=dev)
        args = (flat.data_ptr(), off.data_ptr(), hq.data_ptr(), hg.data_ptr(), he.data_ptr(), m, k, d_tl.data_ptr(), d_n.data_ptr(), d_ops.data_ptr())
        ix.dev_edit_align(*args, stream, 0)  # (warm: the direction workspace grows here)
        torch.cuda.synchronize()
        ms = sorted(timed(lambda: ix.dev_edit_align(*args, stream, 0), 1, 3) for _ in range(5))
        tally = torch.zeros(2, dtype=torch.int64, device=dev)
        ix.dev_edit_align_tally(*args, tally.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        aligned, cells = [int(x) for x in tally.cpu().tolist()]
        assert aligned == m and np.array_equal(d_tl.cpu().numpy().view(np.uint32)[:m], tl)
        leg.update(align_pass_ms=ms, align_pass_median_ms=ms[2], align_pass_spread=(ms[-1] - ms[0]) / ms[2] if ms[2] else 0.0, hits_aligned=aligned,
                   table_cells=cells, hits_per_s=aligned / (ms[2] * 1e-3) if ms[2] else 0.0, cells_per_s=cells / (ms[2] * 1e-3) if ms[2] else 0.0,
                   band_half_width=2 if k <= 2 else 4 if k <= 4 else 6 if k <= 6 else 8, rows_per_launch=256)
        out["k"][str(k)] = leg
        log("k", k, json.dumps(leg))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
