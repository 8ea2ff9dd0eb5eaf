"""Rates of chain alignment (awry_dev_align_chains, kernels_chain_align.hip.h) on the workload of tools/time_chain.py: the repeat-rich
GRCh38-shaped text (tests/synth.repeat_rich_text, as bench.py) with reads resident in HBM -- 101-bp windows with 3 planted
substitutions, and a leg of 1-kb windows with 2 % edits (14 substitutions, 3 one-letter deletions, 3 one-letter insertions).
Per leg, device time (awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean, median and spread) of
  seeding + chaining  the yardstick, code this stage does not touch: tools/time_chain.py's two steps, back to back;
  alignment           the primary chain of every read (max_alignments 1) at band 4: count pass, scan, fill pass;
and chains/s, table cells/s from the census (both passes compute the tables), the ratio alignment ms / yardstick ms, and the rate of
awry_align_chains_batch across the host boundary (one warmed call on a part of the reads).  Beside them, from the same process,
awry_dev_edit_align's cells/s on tools/time_align.py's workload (101-bp reads with 3 edits at k = 5): the nearest existing kernel.
usage: time_chain_align.py [text_len] [n_reads] [n_long_reads]   -> one JSON object on stdout (profiles/chain_align_rates.json)"""
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
from tools.read_sets import plant
from tools.time_edit import with_indel

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 250_000_000
nq_short = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
nq_long = int(float(sys.argv[3])) if len(sys.argv) > 3 else 100_000
MIN_LEN, MAX_HITS, BAND = 12, 50, 4
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
    """windows with ndel one-letter deletions and nins one-letter insertions each (tools/time_chain.py's)"""
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
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "min_len": MIN_LEN, "max_hits": MAX_HITS, "band": BAND, "max_alignments": 1,
           "seed_k": ix.seed_kmer_len(),
           "timing": "awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean: median and spread ((max - min) / median)", "legs": {}}
    text_d = torch.from_numpy(text).to(dev)
    reads = {"short": plant(windows(text_d, nq_short, 101, 503), 3, 8), "long": plant(with_indels(text_d, nq_long, 1000, 3, 3, 71), 14, 9)}
    n_edit = min(nq_short, 200_000)
    gen = torch.Generator(device=dev)
    gen.manual_seed(503)
    pos = torch.randint(0, text_d.numel() - 2 - 101, (n_edit,), device=dev, generator=gen)
    wide = text_d[pos[:, None] + torch.arange(102, device=dev)[None, :]]
    edit_reads = with_indel(torch.cat([plant(wide[:, :101].contiguous(), 2, 7), wide[:, 101:]], 1), 9)
    del text_d, wide

    def once(fn):
        for _ in range(2):
            fn()
        ix.dev_timer_begin(stream)
        for _ in range(5):
            fn()
        return ix.dev_timer_end(stream) / 5

    def alternating7(fns):
        ms = {k: [] for k in fns}
        for _ in range(7):
            for k, fn in fns.items():
                ms[k].append(once(fn))
        return {k: {"ms": sorted(v), "median_ms": sorted(v)[3], "spread": (max(v) - min(v)) / sorted(v)[3]} for k, v in ms.items()}

    # ---- the nearest existing kernel: awry_dev_edit_align on tools/time_align.py's workload, k = 5 ----
    K = 5
    L = edit_reads.shape[1]
    eflat = torch.cat([edit_reads.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    eoff = torch.arange(n_edit + 1, **i64) * L
    hoff, g, _, d, _, _, _, _ = ix.parallel_align_edit_csr(edit_reads.reshape(-1).cpu().numpy(), np.arange(n_edit + 1, dtype=np.uint64) * np.uint64(L), K, 1000,
                                                          want_pos=False)
    m_e = len(g)
    hq = torch.from_numpy(np.repeat(np.arange(n_edit, dtype=np.uint32), np.diff(hoff.astype(np.int64))).view(np.int32)).to(dev)
    hg, he = torch.from_numpy(g.view(np.int64)).to(dev), torch.from_numpy(d).to(dev)
    d_tl, d_n = torch.zeros(max(m_e, 1), dtype=torch.int32, device=dev), torch.zeros(max(m_e, 1), dtype=torch.uint8, device=dev)
    d_ops = torch.zeros(max(m_e, 1) * ALIGN_MAX_OPS, dtype=torch.int32, device=dev)
    eargs = (eflat.data_ptr(), eoff.data_ptr(), hq.data_ptr(), hg.data_ptr(), he.data_ptr(), m_e, K, d_tl.data_ptr(), d_n.data_ptr(), d_ops.data_ptr())
    etally = torch.zeros(2, **i64)
    ix.dev_edit_align_tally(*eargs, etally.data_ptr(), stream, 0)
    torch.cuda.synchronize()
    edit_cells = int(etally[1].item())

    def edit_align():
        ix.dev_edit_align(*eargs, stream, 0)

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
        seeds = torch.zeros(max(nhits, 1), 2, **i64)
        seed_off = torch.zeros(nq + 1, **i64)
        n_ch, n_mem, ch_off, mem_off = torch.zeros(nq, **i64), torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64), torch.zeros(nq + 1, **i64)
        chains, members = torch.zeros(max(nhits, 1) * 4, **i64), torch.zeros(max(nhits, 1) * 2, **i64)
        arange_rec = torch.arange(total, **i64)

        def seeding_and_chaining():
            smems()
            ranges_and_scan()
            ix.dev_locate(ranges.data_ptr(), hit_off.data_ptr(), total, nhits, gpos.data_ptr(), None, stream, 0)
            torch.index_select(hit_off, 0, rec_off, out=seed_off)
            owner = torch.repeat_interleave(arange_rec, located, output_size=nhits)
            seeds[:nhits, 0] = rec[:, 0][owner]
            seeds[:nhits, 1] = gpos[:nhits]
            ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, n_ch.data_ptr(), n_mem.data_ptr(), None, None, None, None, None, stream, 0)
            ix.dev_scan_counts(n_ch.data_ptr(), nq, ch_off.data_ptr(), scratch.data_ptr(), stream, 0)
            ix.dev_scan_counts(n_mem.data_ptr(), nq, mem_off.data_ptr(), scratch.data_ptr(), stream, 0)
            ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, None, None, ch_off.data_ptr(), mem_off.data_ptr(), chains.data_ptr(),
                               members.data_ptr(), None, stream, 0)

        seeding_and_chaining()
        torch.cuda.synchronize()
        # the primary chain of every read that has one, and its members, compacted (tensor glue; chain_align_select / gather in the library)
        has = n_ch > 0
        cq = torch.nonzero(has).reshape(-1)
        m = int(cq.numel())
        n_seeds = chains.view(-1, 4)[ch_off[:-1][has], 0] >> 32
        sel_moff = torch.zeros(m + 1, **i64)
        sel_moff[1:] = torch.cumsum(n_seeds, 0)
        nsel = int(sel_moff[-1].item())
        gidx = torch.repeat_interleave(mem_off[:-1][has] - sel_moff[:-1], n_seeds, output_size=nsel) + torch.arange(nsel, **i64)
        sel_members = members.view(-1, 2)[gidx].contiguous()
        cq32 = cq.to(torch.int32)
        alns, n_ops, c_off = torch.zeros(3 * max(m, 1), **i64), torch.zeros(max(m, 1), **i64), torch.zeros(m + 1, **i64)
        ascratch = torch.zeros(ix.dev_scan_scratch_bytes(max(m, 1)) // 8 + 1, **i64)
        aargs = (flat.data_ptr(), off.data_ptr(), cq32.data_ptr(), sel_moff.data_ptr(), sel_members.data_ptr(), m, BAND)
        tally = torch.zeros(2, **i64)
        ix.dev_align_chains_tally(*aargs, alns.data_ptr(), n_ops.data_ptr(), tally.data_ptr(), None, None, stream, 0)
        ix.dev_scan_counts(n_ops.data_ptr(), m, c_off.data_ptr(), ascratch.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        aligned, cells = [int(x) for x in tally.cpu().tolist()]
        runs = int(c_off[-1].item())
        cigar = torch.zeros(max(runs, 1), dtype=torch.int32, device=dev)

        def count_pass():
            ix.dev_align_chains(*aargs, alns.data_ptr(), n_ops.data_ptr(), None, None, stream, 0)

        def alignment():
            count_pass()
            ix.dev_scan_counts(n_ops.data_ptr(), m, c_off.data_ptr(), ascratch.data_ptr(), stream, 0)
            ix.dev_align_chains(*aargs, None, None, c_off.data_ptr(), cigar.data_ptr(), stream, 0)

        alignment()
        tm = alternating7({"seeding_and_chaining": seeding_and_chaining, "alignment": alignment, "alignment_count_pass": count_pass, "edit_align_pass": edit_align})
        a = alns.view(-1, 3)[:m]
        status = a[:, 2] >> 32
        edits = (a[:, 2] & 0xFFFFFFFF)[status == 0]
        al_ms, y_ms = tm["alignment"]["median_ms"], tm["seeding_and_chaining"]["median_ms"]
        leg = {"n_reads": nq, "read_len": L, "params": P, "seeds": nhits, "chains_aligned": m, "status_ok": aligned, "status_skew": int((status == 1).sum().item()),
               "status_bad_chain": int((status == 2).sum().item()), "mean_edits": float(edits.double().mean().item()) if edits.numel() else 0.0,
               "members_per_chain": nsel / max(m, 1), "runs_per_chain": runs / max(m, 1), "table_cells_per_pass": cells, "cells_per_chain": cells / max(aligned, 1),
               **tm, "chains_per_s": m / (al_ms * 1e-3), "cells_per_s_both_passes": 2 * cells / (al_ms * 1e-3),
               "cells_per_s_count_pass": cells / (tm["alignment_count_pass"]["median_ms"] * 1e-3), "alignment_ms_over_seeding_and_chaining_ms": al_ms / y_ms,
               "edit_align": {"k": K, "hits": m_e, "table_cells": edit_cells, "cells_per_s": edit_cells / (tm["edit_align_pass"]["median_ms"] * 1e-3)}}
        nb = min(nq, 200_000 if name == "short" else 20_000)
        qb = q[:nb].reshape(-1).cpu().numpy()
        qo = (torch.arange(nb + 1, dtype=torch.int64) * L).numpy().astype("uint64")
        ix.parallel_align_chains_csr(qb, qo, MIN_LEN, MAX_HITS, 1, BAND, *pv)
        t = time.time()
        r = ix.parallel_align_chains_csr(qb, qo, MIN_LEN, MAX_HITS, 1, BAND, *pv)
        dt = time.time() - t
        t = time.time()
        ix.parallel_chains_csr(qb, qo, MIN_LEN, MAX_HITS, *pv)
        dt_chain = time.time() - t
        leg["host_boundary"] = {"n_reads": nb, "seconds": dt, "reads_per_s": nb / dt, "alignments": int(r[0][-1]), "chain_batch_seconds": dt_chain}
        out["legs"][name] = leg
        log(name, json.dumps(leg))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
