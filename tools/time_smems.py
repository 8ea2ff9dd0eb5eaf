"""Rates of SMEMs (awry_dev_smems, kernels_smem.hip.h) on the repeat-rich GRCh38-shaped text (tests/synth.repeat_rich_text, as
bench.py) with 101-bp reads resident in HBM, over: windows of the text with 0 / 1 / 3 planted substitutions and uniform random
reads; min_len 1 / 20; and the two forward forms -- the suffix-array search (the replica as built, verify accelerators
resident) and the bisection over backward searches (set_verify(-1)).  Per leg: device-event time (warmed) of the count pass
and of count + scan + fill, reads/s, and SMEMs, forward extensions, LF steps and suffix comparisons per read from the kernel's
census.  The yardstick, in the same process and on the same reads: the anchors count pass (skip 0, min_len 1), 7 repetitions,
median and spread.  Ratios: SMEM SA form / anchors and LF form / SA form per leg.
usage: time_smems.py [text_len] [n_reads]   -> one JSON object on stdout"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import awry_amd
from tests import synth
from tools.read_sets import L, plant, timed, windows

FULL = 3_100_000_000
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else FULL
nq = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
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
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "full_size_text": n == FULL, "n_reads": nq, "read_len": L,
           "seed_k": ix.seed_kmer_len(), "legs": {}, "ratios": {}}
    if n != FULL:
        out["note"] = "a text of %d letters instead of the full %d: the suffix-array search takes log2 of the bucket fewer comparisons here" % (n, FULL)
    text_d = torch.from_numpy(text).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    nt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    sampled = windows(text_d, nq, 503)
    legs = {"sampled_sub0": sampled, "sampled_sub1": plant(sampled, 1, 7), "sampled_sub3": plant(sampled, 3, 8),
            "random": nt[torch.randint(0, 4, (nq, L), device=dev, generator=gen)]}
    del text_d
    off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * L
    n_rec = torch.zeros(nq, dtype=torch.int64, device=dev)
    rec_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    scratch = torch.zeros(ix.dev_scan_scratch_bytes(nq) // 8 + 1, dtype=torch.int64, device=dev)
    records = torch.zeros(nq * (L + 1) * 3, dtype=torch.int64, device=dev)  # room for one record per letter
    tally = torch.zeros(4, dtype=torch.int64, device=dev)
    flats = {name: torch.cat([q.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)]) for name, q in legs.items()}

    def count_pass(flat, min_len):
        ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, min_len, n_rec.data_ptr(), None, None, None, stream, 0)

    def both_passes(flat, min_len):
        count_pass(flat, min_len)
        ix.dev_scan_counts(n_rec.data_ptr(), nq, rec_off.data_ptr(), scratch.data_ptr(), stream, 0)
        ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, min_len, None, rec_off.data_ptr(), records.data_ptr(), None, stream, 0)

    def anchors_count_pass(flat):
        ix.dev_anchors(flat.data_ptr(), off.data_ptr(), nq, 1, 0, n_rec.data_ptr(), None, None, None, stream, 0)

    # yardstick first, in the state the SA form runs in: the anchors count pass on every leg's reads
    out["yardstick"] = {"what": "awry_dev_anchors count pass (skip 0, min_len 1), 7 repetitions of a warmed 5-launch mean, replica as built"}
    for name, flat in flats.items():
        ms = sorted(timed(lambda: anchors_count_pass(flat)) for _ in range(7))
        out["yardstick"][name] = {"ms": ms, "median_ms": ms[3], "spread": (ms[-1] - ms[0]) / ms[3], "reads_per_s": nq / (ms[3] * 1e-3)}
        log("yardstick", name, json.dumps(out["yardstick"][name]))

    for form in ("sa", "lf"):
        if form == "lf":
            ix.set_verify(-1)
        assert ix.verify_enabled() == (form == "sa")
        for name, flat in flats.items():
            for min_len in (1, 20):
                ms_c = timed(lambda: count_pass(flat, min_len))
                ms_f = timed(lambda: both_passes(flat, min_len))
                tally.zero_()
                ix.dev_smems_tally(flat.data_ptr(), off.data_ptr(), nq, min_len, n_rec.data_ptr(), tally.data_ptr(), None, None, None, stream, 0)
                torch.cuda.synchronize()
                steps, compared, extensions, reported = [int(x) for x in tally.cpu().tolist()]
                assert form == "sa" or compared == 0  # (reads that occur whole compare no suffix in either form: nothing to extend into)
                leg = {"form": form, "min_len": min_len, "count_pass_ms": ms_c, "count_scan_fill_ms": ms_f, "reads_per_s_count_pass": nq / (ms_c * 1e-3),
                       "reads_per_s_count_scan_fill": nq / (ms_f * 1e-3), "smems_per_read": reported / nq, "extensions_per_read": extensions / nq,
                       "steps_per_read": steps / nq, "suffixes_compared_per_read": compared / nq}
                out["legs"]["%s_min%d_%s" % (name, min_len, form)] = leg
                log(name, json.dumps(leg))
    for name in flats:
        for min_len in (1, 20):
            sa, lf = out["legs"]["%s_min%d_sa" % (name, min_len)], out["legs"]["%s_min%d_lf" % (name, min_len)]
            out["ratios"]["%s_min%d" % (name, min_len)] = {"smem_sa_ms_over_anchors_ms": sa["count_pass_ms"] / out["yardstick"][name]["median_ms"],
                                                            "lf_ms_over_sa_ms": lf["count_pass_ms"] / sa["count_pass_ms"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
