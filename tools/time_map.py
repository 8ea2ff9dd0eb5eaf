"""Rates of mapping on both strands (awry_map_batch and its device primitives, kernels_map.hip.h) on the workload of
tools/time_chain_align.py: the repeat-rich GRCh38-shaped text with reads resident in HBM -- 101-bp windows with 3 planted
substitutions, and a leg of 1-kb windows with 2 % edits -- every second read replaced by its reverse complement.  Per leg, device
time (awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean, median and spread) of
  the mapping pipeline at (A, R) = (4, 1): awry_dev_revcomp, seeding + chaining of the doubled batch, the alignment count pass over
                        the first A chains of every query, awry_dev_map_select (count, scan, fill), the CIGAR fill pass over the
                        reported alignments;
  the yardstick         what a caller pays today for both strands by hand: the forward-only seeding + chaining + awry_dev_align_chains
                        (count pass, scan, fill pass over the first A chains) on the reads and again on their reverse complements --
                        code this change does not alter;
  the CIGAR fill pass   over the reported alignments, and over every candidate (no selection before it);
and the rate of awry_map_batch across the host boundary next to awry_align_chains_batch on the doubled batch built on the host (one
warmed call each on a part of the reads).  The choice of chains and the compaction of their members between the stages is tensor
glue outside the timers, as in tools/time_chain_align.py (the library has kernels for it: chain_align_take / select / gather,
map_gather).
usage: time_map.py [text_len] [n_reads] [n_long_reads]   -> one JSON object on stdout (profiles/map_rates.json)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import awry_amd
from tests import synth
from tools.read_sets import plant

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 250_000_000
nq_short = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
nq_long = int(float(sys.argv[3])) if len(sys.argv) > 3 else 100_000
MIN_LEN, MAX_HITS, BAND, A, R = 12, 50, 4, 4, 1
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
    r = torch.gather(w, 1, j + (dels[:, :, None] <= j[:, None, :]).sum(1))
    ins = torch.randint(10, length - 10, (count, nins), device=dev, generator=gen)
    out = torch.gather(r, 1, j - (ins[:, :, None] < j[:, None, :]).sum(1))
    nt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    out.scatter_(1, ins, nt[torch.randint(0, 4, (count, nins), device=dev, generator=gen)])
    return out


def revcomp(q):
    """reverse complement of equal-length reads on the device (letters outside ACGT become N): the planted strand of the reads, and
    the second batch of the yardstick"""
    lut = torch.full((256,), ord("N"), dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGTacgt", b"TGCATGCA"):
        lut[a] = b
    return lut[q.flip(1).long()]


class Stage:
    """seeding + chaining + the first A chains of every query of one batch (flat bytes, offsets) through the device primitives"""

    def __init__(self, ix, flat, off, nq, P):
        self.ix, self.flat, self.off, self.nq = ix, flat, off, nq
        self.pv = (P["max_seeds"], P["lookback"], P["max_gap"], P["max_skew"], P["min_score"])
        self.n_rec, self.rec_off = torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64)
        self.scratch = torch.zeros(ix.dev_scan_scratch_bytes(nq) // 8 + 1, **i64)
        ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, MIN_LEN, self.n_rec.data_ptr(), None, None, None, stream, 0)
        torch.cuda.synchronize()
        self.total = int(self.n_rec.sum().item())
        self.records = torch.zeros(3 * max(self.total, 1), **i64)
        self.smems()
        total = self.total
        self.rec = self.records[:3 * total].view(total, 3)
        self.located, self.hit_off = torch.zeros(total, **i64), torch.zeros(total + 1, **i64)
        self.ranges = torch.zeros(total, 2, **i64)
        self.lscratch = torch.zeros(ix.dev_scan_scratch_bytes(max(total, 1)) // 8 + 1, **i64)
        self.ranges_and_scan()
        torch.cuda.synchronize()
        self.nhits = nhits = int(self.hit_off[-1].item())
        self.gpos, self.seeds = torch.zeros(max(nhits, 1), **i64), torch.zeros(max(nhits, 1), 2, **i64)
        self.seed_off = torch.zeros(nq + 1, **i64)
        self.n_ch, self.n_mem = torch.zeros(nq, **i64), torch.zeros(nq, **i64)
        self.ch_off, self.mem_off = torch.zeros(nq + 1, **i64), torch.zeros(nq + 1, **i64)
        self.chains, self.members = torch.zeros(max(nhits, 1) * 4, **i64), torch.zeros(max(nhits, 1) * 2, **i64)
        self.arange_rec = torch.arange(total, **i64)
        self.seeding_and_chaining()
        torch.cuda.synchronize()
        # the first A chains of every query and their members, compacted (tensor glue; chain_align_take / select / gather in the library)
        taken = torch.clamp(self.n_ch, max=A)
        self.aln_off = torch.zeros(nq + 1, **i64)
        self.aln_off[1:] = torch.cumsum(taken, 0)
        m = self.m = int(self.aln_off[-1].item())
        cq = torch.repeat_interleave(torch.arange(nq, **i64), taken, output_size=m)
        cidx = self.ch_off[:-1][cq] + torch.arange(m, **i64) - self.aln_off[:-1][cq]
        self.sel_chains = self.chains.view(-1, 4)[cidx].contiguous()
        n_seeds = self.sel_chains[:, 0] >> 32
        self.sel_moff = torch.zeros(m + 1, **i64)
        self.sel_moff[1:] = torch.cumsum(n_seeds, 0)
        nsel = int(self.sel_moff[-1].item())
        first = torch.zeros(nq + 1, **i64)  # members of a query's chains lie back to back in chain order: the taken ones are a prefix
        first[1:] = torch.cumsum(torch.zeros(nq, **i64).index_add_(0, cq, n_seeds), 0)
        gidx = torch.repeat_interleave(self.mem_off[:-1][cq] - first[:-1][cq], n_seeds, output_size=nsel) + torch.arange(nsel, **i64)
        self.sel_members = self.members.view(-1, 2)[gidx].contiguous()
        self.cq32 = cq.to(torch.int32)
        self.alns, self.n_ops, self.c_off = torch.zeros(3 * max(m, 1), **i64), torch.zeros(max(m, 1), **i64), torch.zeros(m + 1, **i64)
        self.ascratch = torch.zeros(ix.dev_scan_scratch_bytes(max(m, 1)) // 8 + 1, **i64)
        self.aargs = (flat.data_ptr(), off.data_ptr(), self.cq32.data_ptr(), self.sel_moff.data_ptr(), self.sel_members.data_ptr(), m, BAND)
        self.count_pass()
        ix.dev_scan_counts(self.n_ops.data_ptr(), m, self.c_off.data_ptr(), self.ascratch.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        self.runs = int(self.c_off[-1].item())
        self.cigar = torch.zeros(max(self.runs, 1), dtype=torch.int32, device=dev)

    def smems(self):
        ix, f, o, nq = self.ix, self.flat.data_ptr(), self.off.data_ptr(), self.nq
        ix.dev_smems(f, o, nq, MIN_LEN, self.n_rec.data_ptr(), None, None, None, stream, 0)
        ix.dev_scan_counts(self.n_rec.data_ptr(), nq, self.rec_off.data_ptr(), self.scratch.data_ptr(), stream, 0)
        ix.dev_smems(f, o, nq, MIN_LEN, None, self.rec_off.data_ptr(), self.records.data_ptr(), None, stream, 0)

    def ranges_and_scan(self):
        rec = self.rec
        torch.mul(rec[:, 2], rec[:, 2] <= MAX_HITS, out=self.located)
        self.ranges[:, 0] = rec[:, 1]
        self.ranges[:, 1] = rec[:, 1] + rec[:, 2] - 1
        self.ix.dev_scan_counts(self.located.data_ptr(), self.total, self.hit_off.data_ptr(), self.lscratch.data_ptr(), stream, 0)

    def seeding_and_chaining(self):
        ix, nq, nhits = self.ix, self.nq, self.nhits
        self.smems()
        self.ranges_and_scan()
        ix.dev_locate(self.ranges.data_ptr(), self.hit_off.data_ptr(), self.total, nhits, self.gpos.data_ptr(), None, stream, 0)
        torch.index_select(self.hit_off, 0, self.rec_off, out=self.seed_off)
        owner = torch.repeat_interleave(self.arange_rec, self.located, output_size=nhits)
        self.seeds[:nhits, 0] = self.rec[:, 0][owner]
        self.seeds[:nhits, 1] = self.gpos[:nhits]
        so, sd = self.seed_off.data_ptr(), self.seeds.data_ptr()
        ix.dev_chain_seeds(so, sd, nq, *self.pv, self.n_ch.data_ptr(), self.n_mem.data_ptr(), None, None, None, None, None, stream, 0)
        ix.dev_scan_counts(self.n_ch.data_ptr(), nq, self.ch_off.data_ptr(), self.scratch.data_ptr(), stream, 0)
        ix.dev_scan_counts(self.n_mem.data_ptr(), nq, self.mem_off.data_ptr(), self.scratch.data_ptr(), stream, 0)
        ix.dev_chain_seeds(so, sd, nq, *self.pv, None, None, self.ch_off.data_ptr(), self.mem_off.data_ptr(), self.chains.data_ptr(),
                           self.members.data_ptr(), None, stream, 0)

    def count_pass(self):
        self.ix.dev_align_chains(*self.aargs, self.alns.data_ptr(), self.n_ops.data_ptr(), None, None, stream, 0)

    def fill_pass(self):  # over every selected chain: no selection before it
        self.ix.dev_scan_counts(self.n_ops.data_ptr(), self.m, self.c_off.data_ptr(), self.ascratch.data_ptr(), stream, 0)
        self.ix.dev_align_chains(*self.aargs, None, None, self.c_off.data_ptr(), self.cigar.data_ptr(), stream, 0)

    def forward_only(self):  # the yardstick's half: what awry_align_chains_batch(max_alignments = A) does on the device
        self.seeding_and_chaining()
        self.count_pass()
        self.fill_pass()


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("text, index, replica %.1f s" % (time.time() - t))
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "min_len": MIN_LEN, "max_hits": MAX_HITS, "band": BAND, "chains_per_strand": A,
           "max_report": R, "seed_k": ix.seed_kmer_len(),
           "timing": "awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean: median and spread ((max - min) / median)", "legs": {}}
    text_d = torch.from_numpy(text).to(dev)
    reads = {"short": plant(windows(text_d, nq_short, 101, 503), 3, 8), "long": plant(with_indels(text_d, nq_long, 1000, 3, 3, 71), 14, 9)}
    del text_d

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

    for name, q in reads.items():
        nq, L = q.shape
        P = PARAMS[name]
        q = q.clone()
        q[1::2] = revcomp(q[1::2])  # every second read comes from the reverse strand
        q_rc = revcomp(q)
        pad = torch.zeros(16, dtype=torch.uint8, device=dev)
        flat, flat_rc = torch.cat([q.reshape(-1), pad]), torch.cat([q_rc.reshape(-1), pad])
        off = torch.arange(nq + 1, **i64) * L
        fwd, rev = Stage(ix, flat, off, nq, P), Stage(ix, flat_rc, off, nq, P)
        # the mapping pipeline
        flat2, off2 = torch.zeros(2 * nq * L + 16, dtype=torch.uint8, device=dev), torch.zeros(2 * nq + 1, **i64)

        def expand():
            ix.dev_revcomp(flat.data_ptr(), off.data_ptr(), nq, flat2.data_ptr(), off2.data_ptr(), stream, 0)

        expand()
        torch.cuda.synchronize()
        both = Stage(ix, flat2, off2, 2 * nq, P)
        status = torch.zeros(2 * nq, dtype=torch.uint8, device=dev)
        n_maps, map_off, rstatus = torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64), torch.zeros(nq, dtype=torch.uint8, device=dev)
        mscratch = torch.zeros(ix.dev_scan_scratch_bytes(nq) // 8 + 1, **i64)
        sargs = (both.aln_off.data_ptr(), both.alns.data_ptr(), both.sel_chains.data_ptr(), status.data_ptr(), nq, A, R)
        ix.dev_map_select(*sargs, n_maps.data_ptr(), rstatus.data_ptr(), None, None, None, None, stream, 0)
        ix.dev_scan_counts(n_maps.data_ptr(), nq, map_off.data_ptr(), mscratch.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        nwin = int(map_off[-1].item())
        maps, sel, pos = torch.zeros(4 * max(nwin, 1), **i64), torch.zeros(max(nwin, 1), dtype=torch.int32, device=dev), torch.zeros(2 * max(nwin, 1), **i64)

        def select():
            ix.dev_map_select(*sargs, n_maps.data_ptr(), rstatus.data_ptr(), None, None, None, None, stream, 0)
            ix.dev_scan_counts(n_maps.data_ptr(), nq, map_off.data_ptr(), mscratch.data_ptr(), stream, 0)
            ix.dev_map_select(*sargs, None, None, map_off.data_ptr(), maps.data_ptr(), sel.data_ptr(), pos.data_ptr(), stream, 0)

        select()
        torch.cuda.synchronize()
        # the reported alignments as a chain list of their own (tensor glue; map_gather_kernel in the library)
        w = sel[:nwin].long()
        w_q = both.cq32[w].contiguous()
        w_cnt = both.sel_moff[1:][w] - both.sel_moff[:-1][w]
        w_moff = torch.zeros(nwin + 1, **i64)
        w_moff[1:] = torch.cumsum(w_cnt, 0)
        nwm = int(w_moff[-1].item())
        gidx = torch.repeat_interleave(both.sel_moff[:-1][w] - w_moff[:-1], w_cnt, output_size=nwm) + torch.arange(nwm, **i64)
        w_members = both.sel_members[gidx].contiguous()
        w_nops, w_coff = both.n_ops[w].contiguous(), torch.zeros(nwin + 1, **i64)
        ix.dev_scan_counts(w_nops.data_ptr(), nwin, w_coff.data_ptr(), both.ascratch.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        w_cigar = torch.zeros(max(int(w_coff[-1].item()), 1), dtype=torch.int32, device=dev)
        wargs = (flat2.data_ptr(), off2.data_ptr(), w_q.data_ptr(), w_moff.data_ptr(), w_members.data_ptr(), nwin, BAND)

        def fill_winners():
            ix.dev_scan_counts(w_nops.data_ptr(), nwin, w_coff.data_ptr(), both.ascratch.data_ptr(), stream, 0)
            ix.dev_align_chains(*wargs, None, None, w_coff.data_ptr(), w_cigar.data_ptr(), stream, 0)

        def pipeline():
            expand()
            both.seeding_and_chaining()
            both.count_pass()
            select()
            fill_winners()

        def yardstick():
            fwd.forward_only()
            rev.forward_only()

        pipeline()
        tm = alternating7({"pipeline": pipeline, "yardstick": yardstick, "expand": expand, "seeding_and_chaining_doubled": both.seeding_and_chaining,
                           "alignment_count_pass_all_candidates": both.count_pass, "select": select, "fill_pass_reported": fill_winners,
                           "fill_pass_all_candidates": both.fill_pass})
        mp = maps.view(-1, 4)[:nwin]
        strand = (mp[:, 3] >> 32) & 0xFF
        mapq = (mp[:, 3] >> 40) & 0xFF
        owner = torch.repeat_interleave(torch.arange(nq, **i64), n_maps, output_size=nwin)
        p_ms, y_ms = tm["pipeline"]["median_ms"], tm["yardstick"]["median_ms"]
        leg = {"n_reads": nq, "read_len": L, "params": P, "candidates": both.m, "candidates_forward_only": fwd.m, "candidates_reverse_only": rev.m,
               "reads_reported": nwin, "planted_strand": float((strand == (owner & 1)).double().mean().item()) if nwin else 0.0,
               "mapq_60": int((mapq == 60).sum().item()), "mapq_0": int((mapq == 0).sum().item()), "runs_reported": int(w_coff[-1].item()),
               "runs_all_candidates": both.runs, **tm, "reads_per_s": nq / (p_ms * 1e-3), "pipeline_ms_over_yardstick_ms": p_ms / y_ms,
               "fill_share_of_pipeline": tm["fill_pass_reported"]["median_ms"] / p_ms,
               "fill_share_without_selection": tm["fill_pass_all_candidates"]["median_ms"] /
               (p_ms - tm["fill_pass_reported"]["median_ms"] - tm["select"]["median_ms"] + tm["fill_pass_all_candidates"]["median_ms"])}
        nb = min(nq, 200_000 if name == "short" else 20_000)
        pv = both.pv
        qb = q[:nb].reshape(-1).cpu().numpy()
        qo = (torch.arange(nb + 1, dtype=torch.int64) * L).numpy().astype("uint64")
        q2 = torch.stack([q[:nb], q_rc[:nb]], 1).reshape(-1).cpu().numpy()  # the doubled batch built on the host side
        qo2 = (torch.arange(2 * nb + 1, dtype=torch.int64) * L).numpy().astype("uint64")
        ix.parallel_map_csr(qb, qo, MIN_LEN, MAX_HITS, A, R, BAND, *pv)
        t = time.time()
        r = ix.parallel_map_csr(qb, qo, MIN_LEN, MAX_HITS, A, R, BAND, *pv)
        dt = time.time() - t
        ix.parallel_align_chains_csr(q2, qo2, MIN_LEN, MAX_HITS, A, BAND, *pv)
        t = time.time()
        r2 = ix.parallel_align_chains_csr(q2, qo2, MIN_LEN, MAX_HITS, A, BAND, *pv)
        dt2 = time.time() - t
        leg["host_boundary"] = {"n_reads": nb, "map_batch_seconds": dt, "reads_per_s": nb / dt, "records": int(r[0][-1]),
                                "align_chains_batch_on_doubled_seconds": dt2, "alignments_on_doubled": int(r2[0][-1])}
        out["legs"][name] = leg
        log(name, json.dumps(leg))
        del fwd, rev, both
    print(json.dumps(out))


if __name__ == "__main__":
    main()
