"""Rates of substitution-tolerant count (awry_dev_count_mismatch, mismatch_kernels.hip.h) on the repeat-rich GRCh38-shaped
text (tests/synth.repeat_rich_text, as bench.py) with the queries resident in HBM, for k = 0, 1, 2 over: random 31-mers,
text-sampled 31-mers with 0 / 1 / 2 planted substitutions, 101-bp sampled reads.  Per leg: device-event time (warmed),
queries/s, expansions per query from the kernel's census, and the bytes those expansions need at 2 x 128 B each (the two
block lines of one expansion) per second as a fraction of the 8 TB/s HBM peak.  Also the host batch calls (PCIe included)
and, optionally, a CPU baseline: every variant enumerated and counted by the oracle on 16 threads.
usage: time_mismatch.py [text_len] [n_queries] [n_host_queries] [cpu_baseline_queries]   -> one JSON object on stdout"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import awry_amd
import bench
from tests import mismatch_ref, synth

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 3_100_000_000
nq = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
nh = int(float(sys.argv[3])) if len(sys.argv) > 3 else 200_000
ncpu = int(float(sys.argv[4])) if len(sys.argv) > 4 else 0
HBM_PEAK = 8.0e12
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def plant(q, m, seed):
    """m substitutions at distinct random positions of every row of q (uint8[n, L] on the device)"""
    if m == 0:
        return q
    gen = torch.Generator(device=q.device)
    gen.manual_seed(seed)
    q = q.clone()
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=q.device)
    code = torch.full((256,), 0, dtype=torch.int64, device=q.device)
    code[lut.long()] = torch.arange(4, device=q.device)
    rows = torch.arange(q.shape[0], device=q.device)
    cols = torch.argsort(torch.rand(q.shape, device=q.device, generator=gen), dim=1)[:, :m]
    for j in range(m):
        c = cols[:, j]
        old = code[q[rows, c].long()]
        q[rows, c] = lut[(old + torch.randint(1, 4, (q.shape[0],), device=q.device, generator=gen)) % 4]
    return q


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    log("text %.1f s" % (time.time() - t))
    t = time.time()
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("index + replica %.1f s" % (time.time() - t))
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "n_queries": nq, "hbm_peak_Bps": HBM_PEAK, "legs": {}}
    text_d = torch.from_numpy(text).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    nt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    sampled31 = bench.device_sampled_reads(torch, text_d, nq, 31, 501, ord("N"))
    legs = {
        "random_31": nt[torch.randint(0, 4, (nq, 31), device=dev, generator=gen)],
        "sampled_31_sub0": sampled31,
        "sampled_31_sub1": plant(sampled31, 1, 7),
        "sampled_31_sub2": plant(sampled31, 2, 8),
        "reads_101": bench.device_sampled_reads(torch, text_d, nq, 101, 502, ord("N")),
    }
    counts = torch.zeros(nq * 3, dtype=torch.int64, device=dev)
    tally = torch.zeros(2, dtype=torch.int64, device=dev)
    for name, q in legs.items():
        L = q.shape[1]
        flat = torch.cat([q.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
        off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * L
        for k in (0, 1, 2):
            f = lambda: ix.dev_count_mismatch(flat.data_ptr(), off.data_ptr(), nq, k, counts.data_ptr(), None, stream, 0)
            ms = timed(f)
            tally.zero_()
            ix.dev_count_mismatch_tally(flat.data_ptr(), off.data_ptr(), nq, k, counts.data_ptr(), tally.data_ptr(), None, stream, 0)
            torch.cuda.synchronize()
            exp, qn = [int(x) for x in tally.cpu().tolist()]
            c = counts[:nq * (k + 1)].view(nq, k + 1).sum(dim=1)
            bps = exp * 256 / (ms * 1e-3)
            leg = {"L": L, "k": k, "ms": ms, "queries_per_s": nq / (ms * 1e-3), "expansions_per_query": exp / max(qn, 1),
                   "expansion_bytes_per_s": bps, "hbm_fraction": bps / HBM_PEAK, "mean_hits": float(c.double().mean()),
                   "present_fraction": float((c > 0).double().mean())}
            out["legs"]["%s_k%d" % (name, k)] = leg
            log(name, k, json.dumps(leg))
    # host batch calls (PCIe, chunking, result arrays included)
    for name in ("random_31", "sampled_31_sub1", "reads_101"):
        q = legs[name][:nh].cpu().numpy()
        qb, qo = synth.fixed_to_csr(q)
        for k in (1, 2):
            ix.parallel_count_mismatch_csr(qb, qo, k)
            t = time.perf_counter()
            ix.parallel_count_mismatch_csr(qb, qo, k)
            tc = time.perf_counter() - t
            ix.parallel_locate_mismatch_csr(qb, qo, k, want_pos=False)
            t = time.perf_counter()
            off, _, _, _ = ix.parallel_locate_mismatch_csr(qb, qo, k, want_pos=False)
            tl = time.perf_counter() - t
            out["legs"]["host_%s_k%d" % (name, k)] = {"n": nh, "count_ms": tc * 1e3, "count_queries_per_s": nh / tc, "locate_ms": tl * 1e3,
                                                        "locate_queries_per_s": nh / tl, "hits": int(off[-1])}
            log("host", name, k, json.dumps(out["legs"]["host_%s_k%d" % (name, k)]))
    if ncpu:  # CPU baseline: enumerate the variants of a sample, count them with the oracle on 16 threads
        from oracle import oracle_ffi
        oracle_ffi.build()
        t = time.time()
        oi = oracle_ffi.OracleIndex.from_text(text, 0, 8, 0, starts, headers)
        log("oracle index %.1f s" % (time.time() - t))
        q = legs["sampled_31_sub1"][:ncpu].cpu().numpy()
        for k in (1, 2):
            vs = []
            for row in q:
                for d in range(k + 1):
                    vs += mismatch_ref.variants(bytes(row), d)
            qb = np.frombuffer(b"".join(vs), np.uint8)
            qo = np.arange(len(vs) + 1, dtype=np.uint64) * np.uint64(31)
            t = time.perf_counter()
            oi.parallel_count(qb, qo, 16)
            dt = time.perf_counter() - t
            out["legs"]["cpu_oracle_sampled_31_sub1_k%d" % k] = {"n": ncpu, "variants": len(vs), "s": dt, "queries_per_s": ncpu / dt,
                                                                 "note": "enumeration time excluded; 16 threads"}
            log("cpu", k, json.dumps(out["legs"]["cpu_oracle_sampled_31_sub1_k%d" % k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
