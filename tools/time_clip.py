"""Cost of the clipped mode of chain alignment (awry_dev_align_chains_clip, kernels_chain_align.hip.h with CLIP = true) against the
end-to-end mode on the same chains in the same process: tools/time_chain_align.py's 101-bp workload -- the repeat-rich text
(tests/synth.repeat_rich_text, as bench.py), 101-bp windows with 3 planted substitutions, reads resident in HBM -- where a third of the
reads get 20..40 random letters as their tail.  The primary chain of every read is built once (tools/time_chain_align.py's steps);
then, per mode, device time (awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean, median and spread) of
  count pass          records and run counts;
  fill pass           the runs, at the offsets of the mode's own count pass;
and from the census the table cells per chain of both modes, the ratio clipped / end to end per pass, and what the clipped mode did
to the tailed reads.  The yardstick is the end-to-end pass.  --e2e-only times the end-to-end mode alone (the entry points of the
commit before the clipped mode suffice), for runs of two builds alternating.
usage: time_clip.py [text_len] [n_reads] [--e2e-only]   -> one JSON object on stdout (profiles/clip_rates.json)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import awry_amd
from tests import synth
from tools.read_sets import plant

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
E2E_ONLY = "--e2e-only" in sys.argv
n = int(float(argv[0])) if len(argv) > 0 else 250_000_000
nq = int(float(argv[1])) if len(argv) > 1 else 1_000_000
MIN_LEN, MAX_HITS, BAND, L = 12, 50, 4, 101
WEIGHTS = (1, 4, 6, 5)
P = dict(max_seeds=1024, lookback=16, max_gap=500, max_skew=50, min_score=20)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
i64 = dict(dtype=torch.int64, device=dev)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def reads_with_tails(text_d):
    """nq windows of L letters with 3 substitutions; read i with i % 3 == 0 gets 20..40 random letters as its tail"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(503)
    pos = torch.randint(0, text_d.numel() - 1 - L, (nq,), device=dev, generator=gen)
    q = plant(text_d[pos[:, None] + torch.arange(L, device=dev)[None, :]], 3, 8)
    tail = torch.randint(20, 41, (nq,), device=dev, generator=gen)
    tail[torch.arange(nq, device=dev) % 3 != 0] = 0
    nt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    junk = nt[torch.randint(0, 4, (nq, L), device=dev, generator=gen)]
    in_tail = torch.arange(L, device=dev)[None, :] >= (L - tail)[:, None]
    return torch.where(in_tail, junk, q), tail


def primary_chains(ix, flat, off):
    """tools/time_chain_align.py's steps, once: SMEMs, located seeds, chains; -> (chain_query i32, member_off, members, m)"""
    pv = (P["max_seeds"], P["lookback"], P["max_gap"], P["max_skew"], P["min_score"])
    n_rec, rec_off = torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64)
    scratch = torch.zeros(ix.dev_scan_scratch_bytes(nq) // 8 + 1, **i64)
    ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, MIN_LEN, n_rec.data_ptr(), None, None, None, stream, 0)
    ix.dev_scan_counts(n_rec.data_ptr(), nq, rec_off.data_ptr(), scratch.data_ptr(), stream, 0)
    torch.cuda.synchronize()
    total = int(rec_off[-1].item())
    records = torch.zeros(3 * max(total, 1), **i64)
    ix.dev_smems(flat.data_ptr(), off.data_ptr(), nq, MIN_LEN, None, rec_off.data_ptr(), records.data_ptr(), None, stream, 0)
    rec = records[:3 * total].view(total, 3)
    located = rec[:, 2] * (rec[:, 2] <= MAX_HITS)
    hit_off = torch.zeros(total + 1, **i64)
    ranges = torch.stack([rec[:, 1], rec[:, 1] + rec[:, 2] - 1], 1).contiguous()
    lscratch = torch.zeros(ix.dev_scan_scratch_bytes(total) // 8 + 1, **i64)
    ix.dev_scan_counts(located.data_ptr(), total, hit_off.data_ptr(), lscratch.data_ptr(), stream, 0)
    torch.cuda.synchronize()
    nhits = int(hit_off[-1].item())
    gpos = torch.zeros(max(nhits, 1), **i64)
    ix.dev_locate(ranges.data_ptr(), hit_off.data_ptr(), total, nhits, gpos.data_ptr(), None, stream, 0)
    seed_off = hit_off[rec_off].contiguous()
    owner = torch.repeat_interleave(torch.arange(total, **i64), located, output_size=nhits)
    seeds = torch.stack([rec[:, 0][owner], gpos[:nhits]], 1).contiguous()
    n_ch, n_mem, ch_off, mem_off = torch.zeros(nq, **i64), torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64), torch.zeros(nq + 1, **i64)
    chains, members = torch.zeros(max(nhits, 1) * 4, **i64), torch.zeros(max(nhits, 1) * 2, **i64)
    ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, n_ch.data_ptr(), n_mem.data_ptr(), None, None, None, None, None, stream, 0)
    ix.dev_scan_counts(n_ch.data_ptr(), nq, ch_off.data_ptr(), scratch.data_ptr(), stream, 0)
    ix.dev_scan_counts(n_mem.data_ptr(), nq, mem_off.data_ptr(), scratch.data_ptr(), stream, 0)
    ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), nq, *pv, None, None, ch_off.data_ptr(), mem_off.data_ptr(), chains.data_ptr(), members.data_ptr(),
                       None, stream, 0)
    torch.cuda.synchronize()
    has = n_ch > 0
    cq = torch.nonzero(has).reshape(-1)
    m = int(cq.numel())
    n_seeds = chains.view(-1, 4)[ch_off[:-1][has], 0] >> 32
    sel_moff = torch.zeros(m + 1, **i64)
    sel_moff[1:] = torch.cumsum(n_seeds, 0)
    nsel = int(sel_moff[-1].item())
    gidx = torch.repeat_interleave(mem_off[:-1][has] - sel_moff[:-1], n_seeds, output_size=nsel) + torch.arange(nsel, **i64)
    return cq, cq.to(torch.int32), sel_moff, members.view(-1, 2)[gidx].contiguous(), m


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("text, index, replica %.1f s" % (time.time() - t))
    q, tail = reads_with_tails(torch.from_numpy(text).to(dev))
    flat = torch.cat([q.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    off = torch.arange(nq + 1, **i64) * L
    cq, cq32, moff, mem, m = primary_chains(ix, flat, off)
    base = (flat.data_ptr(), off.data_ptr(), cq32.data_ptr(), moff.data_ptr(), mem.data_ptr(), m, BAND)
    ascratch = torch.zeros(ix.dev_scan_scratch_bytes(max(m, 1)) // 8 + 1, **i64)
    modes = {"end_to_end": dict(words=3, call=lambda al, no, co, cg, tl: (ix.dev_align_chains_tally(*base, al, no, tl, co, cg, stream, 0) if tl else
                                                                            ix.dev_align_chains(*base, al, no, co, cg, stream, 0)))}
    if not E2E_ONLY:
        modes["clipped"] = dict(words=4, call=lambda al, no, co, cg, tl: ix.dev_align_chains_clip(*base, *WEIGHTS, al, no, co, cg, stream, 0, tl))
    fns, facts = {}, {}
    for name, md in modes.items():
        alns, n_ops, c_off = torch.zeros(md["words"] * max(m, 1), **i64), torch.zeros(max(m, 1), **i64), torch.zeros(m + 1, **i64)
        tally = torch.zeros(2, **i64)
        md["call"](alns.data_ptr(), n_ops.data_ptr(), None, None, tally.data_ptr())
        ix.dev_scan_counts(n_ops.data_ptr(), m, c_off.data_ptr(), ascratch.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        aligned, cells = [int(x) for x in tally.cpu().tolist()]
        runs = int(c_off[-1].item())
        cigar = torch.zeros(max(runs, 1), dtype=torch.int32, device=dev)
        md.update(alns=alns, n_ops=n_ops, c_off=c_off, cigar=cigar)
        fns[name + "_count_pass"] = lambda md=md: md["call"](md["alns"].data_ptr(), md["n_ops"].data_ptr(), None, None, None)
        fns[name + "_fill_pass"] = lambda md=md: md["call"](None, None, md["c_off"].data_ptr(), md["cigar"].data_ptr(), None)
        a = alns.view(-1, md["words"])[:m]
        ok = (a[:, 2] >> 32) == 0
        facts[name] = {"status_ok": aligned, "table_cells_per_pass": cells, "cells_per_chain": cells / max(aligned, 1), "runs_per_chain": runs / max(m, 1),
                       "mean_edits": float((a[:, 2] & 0xFFFFFFFF)[ok].double().mean().item())}
        if name == "clipped":
            clip_right = (a[:, 3] >> 48) & 0xFFFF
            t_of = tail[cq]
            tailed = ok & (t_of > 0)
            facts[name].update(mean_score=float(((a[:, 3] << 32) >> 32)[ok].double().mean().item()), tailed_chains=int(tailed.sum().item()),
                               tailed_clipped_by_tail_minus_4=int((tailed & (clip_right >= t_of - 4)).sum().item()),
                               untailed_clipped=int((ok & (t_of == 0) & (((a[:, 3] >> 32) & 0xFFFF) + clip_right > 0)).sum().item()))

    def once(fn):
        for _ in range(2):
            fn()
        ix.dev_timer_begin(stream)
        for _ in range(5):
            fn()
        return ix.dev_timer_end(stream) / 5

    ms = {k: [] for k in fns}
    for _ in range(7):
        for k, fn in fns.items():
            ms[k].append(once(fn))
    tm = {k: {"ms": sorted(v), "median_ms": sorted(v)[3], "spread": (max(v) - min(v)) / sorted(v)[3]} for k, v in ms.items()}
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "n_reads": nq, "read_len": L, "tailed": "every third read, 20..40 random letters",
           "min_len": MIN_LEN, "max_hits": MAX_HITS, "band": BAND, "weights_a_b_g_E": WEIGHTS, "params": P, "chains": m,
           "timing": "awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean: median and spread ((max - min) / median)", "modes": facts, **tm}
    if not E2E_ONLY:
        for p in ("count_pass", "fill_pass"):
            out["clipped_over_end_to_end_" + p] = tm["clipped_" + p]["median_ms"] / tm["end_to_end_" + p]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
