"""Rates of chaining (awry_dev_chain_seeds, kernels_chain.hip.h) on the repeat-rich GRCh38-shaped text (tests/synth.repeat_rich_text,
as bench.py) with reads resident in HBM: 101-bp windows of the text with 3 planted substitutions at min_len 12 / max_hits 50, and
a leg of 1-kb windows with 2 % edits (14 substitutions, 3 one-letter deletions, 3 one-letter insertions per read).
Per leg, device time (awry_dev_timer_*, 7 repetitions of a warmed 5-launch mean, median and spread) of
  seeding   the yardstick, code that does not change with chaining: SMEM count pass + scan + fill pass, the records' row pairs and
            located counts (elementwise tensor glue here; anchor_ranges_kernel in the library), scan, awry_dev_locate;
  chaining  seeds out of the records and located hits (tensor glue here; chain_expand_kernel in the library), then the chain
            count pass (which sorts), two scans, the fill pass.
and reads/s, seeds/s, predecessor pairs/s from the census, the ratio chain ms / seeding ms, and the rate of awry_chain_batch across
the host boundary (one warmed call on a part of the reads).
usage: time_chain.py [text_len] [n_reads] [n_long_reads]   -> one JSON object on stdout (profiles/chain_rates.json)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import awry_amd
from tests import synth
from tools.read_sets import plant

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 250_000_000
nq_short = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
nq_long = int(float(sys.argv[3])) if len(sys.argv) > 3 else 100_000
MIN_LEN, MAX_HITS = 12, 50
PARAMS = {"short": dict(max_seeds=1024, lookback=16, max_gap=500, max_skew=50, min_score=20),
          "long": dict(max_seeds=4096, lookback=32, max_gap=2000, max_skew=100, min_score=40)}
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
i64 = dict(dtype=torch.int64, device=dev)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def windows(text_d, count, length, seed):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    pos = torch.randint(0, text_d.numel() - 1 - length, (count,), device=dev, generator=gen)
    return text_d[pos[:, None] + torch.arange(length, device=dev)[None, :]]


def with_indels(text_d, count, length, ndel, nins, seed):
    """windows with ndel one-letter deletions and nins one-letter insertions each"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    w = windows(text_d, count, length + ndel, seed + 1)
    j = torch.arange(length, device=dev)[None, :]
    dels = torch.randint(10, length - 10, (count, ndel), device=dev, generator=gen)
    src = j + (dels[:, :, None] <= j[:, None, :]).sum(1)
    r = torch.gather(w, 1, src)
    ins = torch.randint(10, length - 10, (count, nins), device=dev, generator=gen)
    src = j - (ins[:, :, None] < j[:, None, :]).sum(1)
    out = torch.gather(r, 1, src)
    nt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    out.scatter_(1, ins, nt[torch.randint(0, 4, (count, nins), device=dev, generator=gen)])
    return out


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("text, index, replica %.1f s" % (time.time() - t))
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "min_len": MIN_LEN, "max_hits": MAX_HITS, "seed_k": ix.seed_kmer_len(),
           "timing": "awry_dev_timer_*, 7 repetitions of a warmed 5-launch mean: median and spread ((max - min) / median)", "legs": {}}
    text_d = torch.from_numpy(text).to(dev)
    reads = {"short": plant(windows(text_d, nq_short, 101, 503), 3, 8), "long": plant(with_indels(text_d, nq_long, 1000, 3, 3, 71), 14, 9)}
    del text_d

    def timed7(fn):
        def once():
            for _ in range(2):
                fn()
            ix.dev_timer_begin(stream)
            for _ in range(5):
                fn()
            return ix.dev_timer_end(stream) / 5
        ms = sorted(once() for _ in range(7))
        return {"ms": ms, "median_ms": ms[3], "spread": (ms[-1] - ms[0]) / ms[3]}

    for name, q in reads.items():
        nq, L = q.shape
        P = PARAMS[name]
        pv = (P["max_seeds"], P["lookback"], P["max_gap"], P["max_skew"], P["min_score"])
        flat = torch.cat([q.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
        off = torch.arange(nq + 1, **i64) * L
        n_rec, rec_off = torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64)
        scratch = torch.zeros(ix.dev_scan_scratch_bytes(nq) // 8 + 1, **i64)
        ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, MIN_LEN, n_rec.data_ptr(), None, None, None, stream, 0)
        torch.cuda.synchronize()
        total = int(n_rec.sum().item())
        records = torch.zeros(3 * max(total, 1), **i64)

        def smems():
            ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, MIN_LEN, n_rec.data_ptr(), None, None, None, stream, 0)
            ix.dev_scan_counts(n_rec.data_ptr(), nq, rec_off.data_ptr(), scratch.data_ptr(), stream, 0)
            ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, MIN_LEN, None, rec_off.data_ptr(), records.data_ptr(), None, stream, 0)

        smems()
        rec = records[:3 * total].view(total, 3)
        located, hit_off = torch.zeros(total, **i64), torch.zeros(total + 1, **i64)
        ranges = torch.zeros(total, 2, **i64)
        lscratch = torch.zeros(ix.dev_scan_scratch_bytes(total) // 8 + 1, **i64)

        def ranges_and_scan():
            torch.mul(rec[:, 2], rec[:, 2] <= MAX_HITS, out=located)
            ranges[:, 0] = rec[:, 1]
            ranges[:, 1] = rec[:, 1] + rec[:, 2] - 1
            ix.dev_scan_counts(located.data_ptr(), total, hit_off.data_ptr(), lscratch.data_ptr(), stream, 0)

        ranges_and_scan()
        torch.cuda.synchronize()
        nhits = int(hit_off[-1].item())
        gpos = torch.zeros(max(nhits, 1), **i64)

        def seeding():
            smems()
            ranges_and_scan()
            ix.dev_locate(ranges.data_ptr(), hit_off.data_ptr(), total, nhits, gpos.data_ptr(), None, stream, 0)

        seeds = torch.zeros(max(nhits, 1), 2, **i64)
        seed_off = torch.zeros(nq + 1, **i64)
        n_ch, n_mem, ch_off, mem_off = torch.zeros(nq, **i64), torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64), torch.zeros(nq + 1, **i64)
        status = torch.zeros(nq, dtype=torch.uint8, device=dev)
        chains, members = torch.zeros(max(nhits, 1) * 4, **i64), torch.zeros(max(nhits, 1) * 2, **i64)
        arange_rec = torch.arange(total, **i64)
        tally = torch.zeros(3, **i64)

        def chaining():
            torch.index_select(hit_off, 0, rec_off, out=seed_off)
            owner = torch.repeat_interleave(arange_rec, located, output_size=nhits)
            seeds[:nhits, 0] = rec[:, 0][owner]
            seeds[:nhits, 1] = gpos[:nhits]
            ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, n_ch.data_ptr(), n_mem.data_ptr(), None, None, None, None, status.data_ptr(),
                               stream, 0)
            ix.dev_scan_counts(n_ch.data_ptr(), nq, ch_off.data_ptr(), scratch.data_ptr(), stream, 0)
            ix.dev_scan_counts(n_mem.data_ptr(), nq, mem_off.data_ptr(), scratch.data_ptr(), stream, 0)
            ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, None, None, ch_off.data_ptr(), mem_off.data_ptr(), chains.data_ptr(),
                               members.data_ptr(), None, stream, 0)

        def chain_kernels_only():
            ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, n_ch.data_ptr(), n_mem.data_ptr(), None, None, None, None, None, stream, 0)
            ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, None, None, ch_off.data_ptr(), mem_off.data_ptr(), chains.data_ptr(),
                               members.data_ptr(), None, stream, 0)

        seeding()
        t_seed = timed7(seeding)
        t_chain = timed7(chaining)
        t_kern = timed7(chain_kernels_only)
        ix.dev_chain_seeds_tally(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, n_ch.data_ptr(), n_mem.data_ptr(), tally.data_ptr(), None, None, None, None,
                                 None, stream, 0)
        torch.cuda.synchronize()
        chained, pairs, reported = [int(x) for x in tally.cpu().tolist()]
        leg = {"n_reads": nq, "read_len": L, "params": P, "smems": total, "seeds": nhits, "seeds_per_read": nhits / nq, "seeds_chained": chained,
               "abandoned_reads": int((status != 0).sum().item()), "chains": reported, "chains_per_read": reported / nq, "pairs": pairs,
               "reads_with_a_chain": int((n_ch > 0).sum().item()), "seeding": t_seed, "chaining": t_chain, "chain_kernels_only": t_kern,
               "chain_reads_per_s": nq / (t_chain["median_ms"] * 1e-3), "chain_seeds_per_s": nhits / (t_chain["median_ms"] * 1e-3),
               "chain_pairs_per_s_both_passes": 2 * pairs / (t_kern["median_ms"] * 1e-3), "seeding_reads_per_s": nq / (t_seed["median_ms"] * 1e-3),
               "chain_ms_over_seeding_ms": t_chain["median_ms"] / t_seed["median_ms"]}
        nb = min(nq, 200_000 if name == "short" else 20_000)
        qb = q[:nb].reshape(-1).cpu().numpy()
        qo = (torch.arange(nb + 1, dtype=torch.int64) * L).numpy().astype("uint64")
        ix.parallel_chains_csr(qb, qo, MIN_LEN, MAX_HITS, *pv)
        t = time.time()
        r = ix.parallel_chains_csr(qb, qo, MIN_LEN, MAX_HITS, *pv)
        dt = time.time() - t
        leg["host_boundary"] = {"n_reads": nb, "seconds": dt, "reads_per_s": nb / dt, "chains": int(r[0][-1])}
        out["legs"][name] = leg
        log(name, json.dumps(leg))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
