"""Rates of class-pattern count (awry_dev_count_pattern, the class mode of mismatch_kernels.hip.h) on the repeat-rich GRCh38-shaped text
(tests/synth.repeat_rich_text, as bench.py) with the patterns resident in HBM; device events, warmed launches.

Yardstick legs: plain-letter 31-mers and 101-bp reads at k = 0, 1, 2 through awry_dev_count_pattern and through
awry_dev_count_mismatch (the letter mode of the same kernel) on the same queries in the same run, 7 timings each: median, min..max, and the
ratio of the medians beside the yardstick's own spread.
Pattern legs: 23-mers "20 nt + NGG" at k = 0, 1, 2 and sampled 31-mers with 1, 2, 4 class positions at k = 0: patterns/s and
expansions per pattern (the kernel's census).
Cap sizing: one launch in which every resident lane runs N x 16 to an expansion cap of 2^14 gives the single-lane expansion
rate under a full launch, and from it the largest power of two a lane works through in about 2 s.
usage: time_pattern.py [text_len] [n_patterns] [lanes_per_cu]   -> one JSON object on stdout"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import awry_amd
import bench
from tests import pattern_ref, synth

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 3_100_000_000
nq = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
lanes_per_cu = int(sys.argv[3]) if len(sys.argv) > 3 else 1024  # count_dfs_kernel<NUCLEOTIDE, true, false>: 4 waves per SIMD
REPS = 7
CAP_PROBE = 1 << 14
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timings(fn, warm=2, reps=REPS):
    """-> reps device-event times (ms) of single warmed launches"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def with_classes(q, c, seed):
    """c distinct random positions of every row of q (uint8[n, L], ACGT, on the device) replaced by an IUPAC letter whose class
    holds the letter that was there"""
    holding = {x: sorted(l for l, m in pattern_ref.NT_CLASSES.items() if len(m) > 1 and x in m) for x in "ACGT"}
    table = torch.zeros((256, 7), dtype=torch.uint8, device=q.device)
    for x, ls in holding.items():
        assert len(ls) == 7
        table[ord(x)] = torch.tensor([ord(l) for l in ls], dtype=torch.uint8)
    gen = torch.Generator(device=q.device)
    gen.manual_seed(seed)
    q = q.clone()
    rows = torch.arange(q.shape[0], device=q.device)
    cols = torch.argsort(torch.rand(q.shape, device=q.device, generator=gen), dim=1)[:, :c]
    for j in range(c):
        pick = torch.randint(0, 7, (q.shape[0],), device=q.device, generator=gen)
        q[rows, cols[:, j]] = table[q[rows, cols[:, j]].long(), pick]
    return q


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    log("text %.1f s" % (time.time() - t))
    t = time.time()
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("index + replica %.1f s" % (time.time() - t))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "n_patterns": nq, "timings_per_leg": REPS, "compute_units": cus,
           "yardstick": {}, "patterns": {}, "cap": {}}
    text_d = torch.from_numpy(text).to(dev)
    counts = torch.zeros(max(nq, cus * lanes_per_cu) * 3, dtype=torch.int64, device=dev)
    tally = torch.zeros(3, dtype=torch.int64, device=dev)
    status = torch.zeros(max(nq, cus * lanes_per_cu), dtype=torch.uint8, device=dev)

    def resident(q):
        L = q.shape[1]
        return torch.cat([q.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)]), torch.arange(q.shape[0] + 1, dtype=torch.int64, device=dev) * L

    def census(flat, off, m, k):
        tally.zero_()
        ix.dev_count_pattern_tally(flat.data_ptr(), off.data_ptr(), m, k, counts.data_ptr(), tally.data_ptr(), None, stream, 0)
        torch.cuda.synchronize()
        return [int(x) for x in tally.cpu().tolist()]

    sampled31 = bench.device_sampled_reads(torch, text_d, nq, 31, 501, ord("N"))
    reads101 = bench.device_sampled_reads(torch, text_d, nq, 101, 502, ord("N"))
    # ---- yardstick legs: the same plain-letter queries through both kernels
    for name, q in (("sampled_31", sampled31), ("reads_101", reads101)):
        flat, off = resident(q)
        for k in (0, 1, 2):
            leg = {"L": q.shape[1], "k": k}
            ms = timings(lambda: ix.dev_count_mismatch(flat.data_ptr(), off.data_ptr(), nq, k, counts.data_ptr(), None, stream, 0))
            leg["mismatch"] = dict(summary(ms), queries_per_s=nq / (float(np.median(ms)) * 1e-3))
            want = counts[:nq * (k + 1)].clone().view(nq, k + 1)
            ms = timings(lambda: ix.dev_count_pattern(flat.data_ptr(), off.data_ptr(), nq, k, counts.data_ptr(), status.data_ptr(), stream, 0))
            leg["pattern"] = dict(summary(ms), queries_per_s=nq / (float(np.median(ms)) * 1e-3))
            ok = status[:nq] == 0  # (a search abandoned at the expansion cap has counts 0: the letter mode has no cap)
            assert int((status[:nq] != 0).sum()) == int((status[:nq] == 6).sum())
            assert torch.equal(counts[:nq * (k + 1)].view(nq, k + 1)[ok], want[ok]), "the two kernels disagree"
            leg["abandoned_at_the_expansion_cap"] = int((~ok).sum())
            leg["ratio_pattern_over_mismatch"] = leg["pattern"]["median_ms"] / leg["mismatch"]["median_ms"]
            leg["yardstick_spread"] = leg["mismatch"]["max_ms"] / leg["mismatch"]["min_ms"]
            out["yardstick"]["%s_k%d" % (name, k)] = leg
            log(name, k, json.dumps(leg))
    # ---- pattern legs
    guides = bench.device_sampled_reads(torch, text_d, nq, 23, 503, ord("N")).clone()
    guides[:, 20:] = torch.tensor(list(b"NGG"), dtype=torch.uint8, device=dev)
    legs = [("guide_20_NGG_k%d" % k, guides, k) for k in (0, 1, 2)]
    legs += [("sampled_31_classes%d_k0" % c, with_classes(sampled31, c, 600 + c), 0) for c in (1, 2, 4)]
    for name, q, k in legs:
        flat, off = resident(q)
        ms = timings(lambda: ix.dev_count_pattern(flat.data_ptr(), off.data_ptr(), nq, k, counts.data_ptr(), None, stream, 0))
        exp, searched, deepest = census(flat, off, nq, k)
        c = counts[:nq * (k + 1)].view(nq, k + 1).sum(dim=1)
        ix.dev_count_pattern(flat.data_ptr(), off.data_ptr(), nq, k, counts.data_ptr(), status.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        leg = dict(summary(ms), L=q.shape[1], k=k, abandoned_at_the_expansion_cap=int((status[:nq] == 6).sum()), patterns_per_s=nq / (float(np.median(ms)) * 1e-3), expansions_per_pattern=exp / max(searched, 1),
                   deepest_stack=deepest, mean_hits=float(c.double().mean()), present_fraction=float((c > 0).double().mean()))
        out["patterns"][name] = leg
        log(name, json.dumps(leg))
    # ---- cap sizing: every resident lane runs N x 16 to the cap
    m = cus * lanes_per_cu
    flat, off = resident(torch.full((m, 16), ord("N"), dtype=torch.uint8, device=dev))
    os.environ["AWRY_PATTERN_MAX_EXPANSIONS"] = str(CAP_PROBE)
    try:
        ms = timings(lambda: ix.dev_count_pattern(flat.data_ptr(), off.data_ptr(), m, 0, counts.data_ptr(), status.data_ptr(), stream, 0), warm=1, reps=3)
        exp, searched, _ = census(flat, off, m, 0)
    finally:
        del os.environ["AWRY_PATTERN_MAX_EXPANSIONS"]
    assert int((status[:m] == 6).sum()) == m and exp == m * CAP_PROBE, "every lane must have run to the cap"
    rate = CAP_PROBE / (float(np.median(ms)) * 1e-3)  # expansions per second of one lane while every lane is busy
    cap = 1 << int(np.floor(np.log2(2.0 * rate)))
    out["cap"] = dict(summary(ms), lanes=m, lanes_per_cu=lanes_per_cu, probe_cap=CAP_PROBE, lane_expansions_per_s=rate,
                      device_expansions_per_s=rate * m, largest_power_of_two_within_2s=cap, seconds_at_that_cap=cap / rate)
    log("cap", json.dumps(out["cap"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
