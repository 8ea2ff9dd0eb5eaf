"""Rates of anchors (awry_dev_anchors, kernels_anchor.hip.h) on the repeat-rich GRCh38-shaped text (tests/synth.repeat_rich_text,
as bench.py) with 101-bp reads resident in HBM, over: windows of the text with 0 / 1 / 3 planted substitutions, windows from
N-free regions, uniform random reads; skip 0 / 1 and min_len 1 / 20.  Per leg: device-event time (warmed) of the count pass
and of count + scan + fill, reads/s, anchors per read, LF steps and table probes per read from the kernel's census, and the
bytes those steps need at 2 x 128 B each per second as a fraction of the 8 TB/s HBM peak.  Also the host batch calls (PCIe
included) and the yardstick: awry_dev_count_ascii on the 0-substitution reads with seed-and-verify and the left-context index
off -- the same L - seed_k dependent steps per read as the anchor count pass -- timed repeatedly in the same process.
usage: time_anchors.py [text_len] [n_reads] [n_host_reads]   -> one JSON object on stdout"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import awry_amd
import bench
from tests import synth
from tools.read_sets import L, plant, timed, windows

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 3_100_000_000
nq = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
nh = int(float(sys.argv[3])) if len(sys.argv) > 3 else 200_000
HBM_PEAK = 8.0e12
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    log("text %.1f s" % (time.time() - t))
    t = time.time()
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("index + replica %.1f s" % (time.time() - t))
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "n_reads": nq, "read_len": L, "seed_k": ix.seed_kmer_len(),
           "hbm_peak_Bps": HBM_PEAK, "legs": {}}
    text_d = torch.from_numpy(text).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    nt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    sampled = windows(text_d, nq, 503)
    legs = {
        "sampled_sub0": sampled,
        "sampled_sub1": plant(sampled, 1, 7),
        "sampled_sub3": plant(sampled, 3, 8),
        "sampled_n_free": bench.device_sampled_reads(torch, text_d, nq, L, 502, ord("N")),
        "random": nt[torch.randint(0, 4, (nq, L), device=dev, generator=gen)],
    }
    del text_d
    off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * L
    n_anchors = torch.zeros(nq, dtype=torch.int64, device=dev)
    anchor_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    scratch = torch.zeros(ix.dev_scan_scratch_bytes(nq) // 8 + 1, dtype=torch.int64, device=dev)
    records = torch.zeros(nq * (L + 1) * 3, dtype=torch.int64, device=dev)  # room for one anchor per letter
    tally = torch.zeros(3, dtype=torch.int64, device=dev)
    flats = {name: torch.cat([q.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)]) for name, q in legs.items()}

    def count_pass(flat, min_len, skip):
        ix.dev_anchors(flat.data_ptr(), off.data_ptr(), nq, min_len, skip, n_anchors.data_ptr(), None, None, None, stream, 0)

    def both_passes(flat, min_len, skip):
        count_pass(flat, min_len, skip)
        ix.dev_scan_counts(n_anchors.data_ptr(), nq, anchor_off.data_ptr(), scratch.data_ptr(), stream, 0)
        ix.dev_anchors(flat.data_ptr(), off.data_ptr(), nq, min_len, skip, None, anchor_off.data_ptr(), records.data_ptr(), None, stream, 0)

    for name, flat in flats.items():
        for skip in (0, 1):
            for min_len in (1, 20):
                ms_c = timed(lambda: count_pass(flat, min_len, skip))
                ms_f = timed(lambda: both_passes(flat, min_len, skip))
                tally.zero_()
                ix.dev_anchors_tally(flat.data_ptr(), off.data_ptr(), nq, min_len, skip, n_anchors.data_ptr(), tally.data_ptr(), None, None, None, stream, 0)
                torch.cuda.synchronize()
                steps, probes, reported = [int(x) for x in tally.cpu().tolist()]
                bps = steps * 256 / (ms_c * 1e-3)
                leg = {"skip": skip, "min_len": min_len, "count_pass_ms": ms_c, "count_scan_fill_ms": ms_f, "reads_per_s_count_pass": nq / (ms_c * 1e-3),
                       "reads_per_s_count_scan_fill": nq / (ms_f * 1e-3), "anchors_per_read": reported / nq, "steps_per_read": steps / nq,
                       "probes_per_read": probes / nq, "step_bytes_per_s": bps, "hbm_fraction": bps / HBM_PEAK}
                out["legs"]["%s_skip%d_min%d" % (name, skip, min_len)] = leg
                log(name, json.dumps(leg))
    # host batch calls (PCIe, chunking, result arrays included)
    for name in ("sampled_sub0", "sampled_sub3", "random"):
        qb, qo = synth.fixed_to_csr(legs[name][:nh].cpu().numpy())
        ix.parallel_anchors_csr(qb, qo, 20, 0)
        t = time.perf_counter()
        aoff, _ = ix.parallel_anchors_csr(qb, qo, 20, 0)
        ta = time.perf_counter() - t
        ix.parallel_locate_anchors_csr(qb, qo, 50, 20, 0, want_pos=False)
        t = time.perf_counter()
        r = ix.parallel_locate_anchors_csr(qb, qo, 50, 20, 0, want_pos=False)
        tl = time.perf_counter() - t
        out["legs"]["host_%s_skip0_min20" % name] = {"n": nh, "anchors_ms": ta * 1e3, "anchors_reads_per_s": nh / ta, "anchors": int(aoff[-1]),
                                                      "locate_max_hits": 50, "locate_ms": tl * 1e3, "locate_reads_per_s": nh / tl, "hits": int(r[2][-1])}
        log("host", name, json.dumps(out["legs"]["host_%s_skip0_min20" % name]))
    # yardstick: the generic count kernel on the 0-substitution reads, without text verification and without the left-context index
    ix.set_lcx(False)
    ix.set_verify(-1)
    flat = flats["sampled_sub0"]
    counts = torch.zeros(nq, dtype=torch.int64, device=dev)
    yard = sorted(timed(lambda: ix.dev_count_ascii(flat.data_ptr(), off.data_ptr(), nq, counts.data_ptr(), None, None, stream, 0)) for _ in range(7))
    mine = sorted(timed(lambda: count_pass(flat, 1, 0)) for _ in range(7))
    tally.zero_()
    ix.dev_anchors_tally(flat.data_ptr(), off.data_ptr(), nq, 1, 0, n_anchors.data_ptr(), tally.data_ptr(), None, None, None, stream, 0)
    torch.cuda.synchronize()
    steps, probes, reported = [int(x) for x in tally.cpu().tolist()]
    out["yardstick"] = {"what": "awry_dev_count_ascii on sampled_sub0, set_verify(-1), set_lcx(0); anchors count pass (skip 0, min_len 1) in the same state",
                        "seed_k": ix.seed_kmer_len(), "count_ascii_ms": yard, "anchors_count_pass_ms": mine, "count_ascii_median_ms": yard[3],
                        "anchors_median_ms": mine[3], "ratio_anchors_over_count_ascii": mine[3] / yard[3],
                        "count_ascii_spread": (yard[-1] - yard[0]) / yard[3], "anchors_steps_per_read": steps / nq, "anchors_probes_per_read": probes / nq,
                        "anchors_per_read": reported / nq}
    log("yardstick", json.dumps(out["yardstick"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
