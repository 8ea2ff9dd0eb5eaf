"""Rates of mapping read pairs (awry_map_pairs_batch and its device primitives, kernels_pair.hip.h) on the text of tools/time_map.py:
the repeat-rich GRCh38-shaped text with reads resident in HBM.  P simulated pairs of 96-bp mates from the two ends of fragments of
200..600 letters, 3 planted substitutions per mate, every second pair taken from the reverse strand; in every eighth pair one mate
has a substitution every 11th letter instead: it seeds nowhere at min_len = 12 and lies within 8 edits, so only rescue places it.
Device time (awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean, median and spread) of
  the paired pipeline   awry_dev_revcomp, seeding + chaining of the doubled batch of 2 P reads, the alignment count pass over the
                        first A chains of every query, awry_dev_map_select at max_report = 2 A (count, scan, fill),
                        awry_dev_pair_windows, the rescue scan (awry_dev_edit_windows count pass, scan, fill pass over the windows cut
                        to 64 starts), the rescue alignment (awry_dev_edit_align over every slot's best hit), awry_dev_pair_select
                        (count, scan, fill), the CIGAR fill pass over the chain-derived records -- each stage also on its own;
  the yardstick         the single-end mapping pipeline of tools/time_map.py on the same 2 P reads at max_report = 1 -- code this
                        change does not alter.
The cut of the windows, the best hit per window and the rescued records between the stages are tensor glue outside the timers, as
the choice of chains is in tools/time_map.py (the library has kernels for them: pair_sub_windows, pair_best_hit, pair_rescued).
The public scan and aligner primitives run at their widest (4 words per column with masks per window, 256 trace rows); the batch
driver runs them at the chunk's longest rescuable read (2 words, masks per query, 96 rows here), so the two rescue stages are upper
bounds of what the driver pays.  And the rate of awry_map_pairs_batch across the host boundary next to awry_map_batch on the same
reads (one warmed call each on a part of the pairs).
The clipped leg (host_legs): awry_map_pairs_clip_batch next to awry_map_pairs_batch across the host boundary on the same reads, 7
alternating repetitions of one call each after a warming call, median and spread of the wall time; the yardstick is the end-to-end
call of the same library.  --host-only runs nothing but this leg; --end-to-end-only leaves the clipped call out of it (for a
library from before the clipped mode).
usage: time_pairs.py [text_len] [n_pairs] [--host-only] [--end-to-end-only]
       -> one JSON object on stdout (profiles/pair_rates.json; the clipped leg alone: profiles/pair_clip_rates.json)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
HOST_ONLY, E2E_ONLY = "--host-only" in sys.argv, "--end-to-end-only" in sys.argv
sys.argv = sys.argv[:1] + ARGS  # (tools/time_map.py reads its sizes from the same positions when it is imported)

import awry_amd
from tests import synth
from tools import time_map as tm
from tools.read_sets import plant

n = int(float(ARGS[0])) if len(ARGS) > 0 else 250_000_000
n_pairs = int(float(ARGS[1])) if len(ARGS) > 1 else 500_000
L, A, BAND, MIN_LEN, MAX_HITS = 96, tm.A, tm.BAND, tm.MIN_LEN, tm.MAX_HITS
MN, MX, U, G, K, SUB = 0, 1000, 4, 2, 8, 64
CLIP, U_CLIP = (1, 4, 6, 5, 30), 20  # match, mismatch, gap, end_bonus, min_aln_score; the penalty in score units: U (a + b)
PARAMS = tm.PARAMS["short"]
dev, stream, i64 = tm.dev, tm.stream, tm.i64
i32 = dict(dtype=torch.int32, device=dev)
u8 = dict(dtype=torch.uint8, device=dev)


def simulated_pairs(text_d, P, seed):
    """-> uint8[2 P, L]: reads 2p and 2p + 1 are the mates of pair p"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    F = torch.randint(200, 601, (P,), device=dev, generator=gen)
    pos = torch.randint(0, text_d.numel() - 1 - 600, (P,), device=dev, generator=gen)
    ar = torch.arange(L, device=dev)[None, :]
    left, right = text_d[pos[:, None] + ar], text_d[(pos + F - L)[:, None] + ar]
    hard = torch.arange(P, device=dev) % 8 == 3
    which = (torch.arange(P, device=dev) // 8) % 2
    nxt = torch.full((256,), ord("A"), dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    cols = torch.arange(10, L, 11, device=dev)
    out = []
    for m, w in enumerate((left, right)):
        planted = plant(w, 3, seed + 1 + m)
        sparse = w.clone()
        sparse[:, cols] = nxt[w[:, cols].long()]
        out.append(torch.where((hard & (which == m))[:, None], sparse, planted))
    fwd, rev = out[0], tm.revcomp(out[1])
    swap = (torch.arange(P, device=dev) % 2 == 1)[:, None]
    q = torch.empty(2 * P, L, **u8)
    q[0::2], q[1::2] = torch.where(swap, rev, fwd), torch.where(swap, fwd, rev)
    return q, int(hard.sum().item())


def host_legs(ix, q, nb, pv, clipped=True):
    """wall time of the batch calls on the first nb pairs of q, positions and CIGARs included -> the clipped leg's JSON object"""
    qb = q[:2 * nb].reshape(-1).cpu().numpy()
    qo = (torch.arange(2 * nb + 1, dtype=torch.int64) * L).numpy().astype("uint64")
    legs = {"end_to_end": lambda: ix.parallel_map_pairs_csr(qb, qo, MIN_LEN, MAX_HITS, A, BAND, MN, MX, U, G, K, *pv)}
    if clipped:
        legs["clipped"] = lambda: ix.parallel_map_pairs_clip_csr(qb, qo, MIN_LEN, MAX_HITS, A, BAND, MN, MX, U_CLIP, G, K, *CLIP, *pv)
    res = {k: fn() for k, fn in legs.items()}  # the warming call, and what the legs return
    s = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            t = time.time()
            fn()
            s[k].append(time.time() - t)
    out = {"n_pairs": nb, "read_len": L, "timing": "wall time of one batch call, 7 alternating repetitions after a warming call: median and spread ((max - min) / median)",
           "unpaired_penalty_clipped": U_CLIP, "match_mismatch_gap_end_bonus_min_aln_score": list(CLIP)}
    for k, v in s.items():
        r, med = res[k], sorted(v)[3]
        out[k] = {"seconds": sorted(v), "median_seconds": med, "spread": (max(v) - min(v)) / med, "pairs_per_s": nb / med, "records": int(r[0][-1]),
                  "records_proper": int(((r[1]["flags"] & 2) != 0).sum()), "records_rescued": int(((r[1]["flags"] & 4) != 0).sum()),
                  "records_mate_unmapped": int(((r[1]["flags"] & 8) != 0).sum())}
    if clipped:
        c = res["clipped"][1]
        out["clipped"]["records_with_a_clip"] = int(((c["clip_left"] != 0) | (c["clip_right"] != 0)).sum())
        out["clipped_seconds_over_end_to_end_seconds"] = out["clipped"]["median_seconds"] / out["end_to_end"]["median_seconds"]
    return out


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    tm.log("text, index, replica %.1f s" % (time.time() - t))
    text_d = torch.from_numpy(text).to(dev)
    P = n_pairs
    q, n_hard = simulated_pairs(text_d, P, 909)
    del text_d
    nq = 2 * P
    if HOST_ONLY:
        p = PARAMS
        pv = (p["max_seeds"], p["lookback"], p["max_gap"], p["max_skew"], p["min_score"])
        print(json.dumps({"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "min_len": MIN_LEN, "max_hits": MAX_HITS, "band": BAND,
                          "chains_per_strand": A, "min_insert": MN, "max_insert": MX, "unpaired_penalty": U, "rescue_anchors": G, "rescue_edits": K,
                          "params": PARAMS, "seed_k": ix.seed_kmer_len(), "pairs_with_an_unseedable_mate": n_hard,
                          "clipped_leg": host_legs(ix, q, min(P, 100_000), pv, not E2E_ONLY)}))
        return

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

    def scan(counts, count, offs, scratch):
        ix.dev_scan_counts(counts.data_ptr(), count, offs.data_ptr(), scratch.data_ptr(), stream, 0)

    def scratch_for(count):
        return torch.zeros(ix.dev_scan_scratch_bytes(max(count, 1)) // 8 + 1, **i64)

    flat = torch.cat([q.reshape(-1), torch.zeros(16, **u8)])
    off = torch.arange(nq + 1, **i64) * L
    flat2, off2 = torch.zeros(2 * nq * L + 16, **u8), torch.zeros(2 * nq + 1, **i64)

    def expand():
        ix.dev_revcomp(flat.data_ptr(), off.data_ptr(), nq, flat2.data_ptr(), off2.data_ptr(), stream, 0)

    expand()
    torch.cuda.synchronize()
    both = tm.Stage(ix, flat2, off2, 2 * nq, PARAMS)
    status = torch.zeros(2 * nq, **u8)
    rstatus, mscratch = torch.zeros(nq, **u8), scratch_for(nq)

    def selection(R):
        """awry_dev_map_select at max_report = R over the doubled batch -> (the three launches, offsets, records, alignment indices)"""
        n_maps, map_off = torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64)
        sargs = (both.aln_off.data_ptr(), both.alns.data_ptr(), both.sel_chains.data_ptr(), status.data_ptr(), nq, A, R)
        ix.dev_map_select(*sargs, n_maps.data_ptr(), rstatus.data_ptr(), None, None, None, None, stream, 0)
        scan(n_maps, nq, map_off, mscratch)
        torch.cuda.synchronize()
        total = int(map_off[-1].item())
        maps, sel = torch.zeros(max(total, 1), 4, **i64), torch.zeros(max(total, 1), **i32)

        def run():
            ix.dev_map_select(*sargs, n_maps.data_ptr(), rstatus.data_ptr(), None, None, None, None, stream, 0)
            scan(n_maps, nq, map_off, mscratch)
            ix.dev_map_select(*sargs, None, None, map_off.data_ptr(), maps.data_ptr(), sel.data_ptr(), None, stream, 0)

        run()
        torch.cuda.synchronize()
        return run, map_off, maps, sel, total

    def cigar_fill(w):
        """the alignments w (indices among the selected chains) as a chain list of their own (tensor glue; map_gather_kernel in the
        library) -> (the fill pass over them, their runs)"""
        nwin = w.numel()
        w_q = both.cq32[w].contiguous()
        w_cnt = both.sel_moff[1:][w] - both.sel_moff[:-1][w]
        w_moff = torch.zeros(nwin + 1, **i64)
        w_moff[1:] = torch.cumsum(w_cnt, 0)
        nwm = int(w_moff[-1].item())
        gidx = torch.repeat_interleave(both.sel_moff[:-1][w] - w_moff[:-1], w_cnt, output_size=nwm) + torch.arange(nwm, **i64)
        w_members = both.sel_members[gidx].contiguous()
        w_nops, w_coff, w_scratch = both.n_ops[w].contiguous(), torch.zeros(nwin + 1, **i64), scratch_for(nwin)
        scan(w_nops, nwin, w_coff, w_scratch)
        torch.cuda.synchronize()
        runs = int(w_coff[-1].item())
        w_cigar = torch.zeros(max(runs, 1), **i32)

        def run():  # (it names every tensor it hands over as a pointer: they live as long as it does)
            scan(w_nops, nwin, w_coff, w_scratch)
            ix.dev_align_chains(flat2.data_ptr(), off2.data_ptr(), w_q.data_ptr(), w_moff.data_ptr(), w_members.data_ptr(), nwin, BAND, None, None,
                                w_coff.data_ptr(), w_cigar.data_ptr(), stream, 0)

        return run, runs

    # the kept lists, then the rescue windows
    select_kept, kept_off, cands, cand_aln, ncand = selection(2 * A)
    slots = nq * G
    wq, wf, wc = torch.zeros(slots, **i32), torch.zeros(slots, **i64), torch.zeros(slots, **i32)

    def windows():
        ix.dev_pair_windows(kept_off.data_ptr(), cands.data_ptr(), off.data_ptr(), P, MN, MX, G, K, wq.data_ptr(), wf.data_ptr(), wc.data_ptr(), stream, 0)

    windows()
    torch.cuda.synchronize()
    # windows of more than SUB starts in pieces (tensor glue; pair_sub_windows_kernel in the library)
    cnt = wc.long()
    nsub = (cnt + SUB - 1) // SUB
    sub_off = torch.zeros(slots + 1, **i64)
    sub_off[1:] = torch.cumsum(nsub, 0)
    m = int(sub_off[-1].item())
    owner = torch.repeat_interleave(torch.arange(slots, **i64), nsub, output_size=m)
    j = torch.arange(m, **i64) - sub_off[:-1][owner]
    sq, sf = wq[owner].contiguous(), (wf[owner] + j * SUB).contiguous()
    sc = torch.minimum(cnt[owner] - j * SUB, torch.full_like(j, SUB)).to(torch.int32)
    nh, hoff, hscratch, tally = torch.zeros(max(m, 1), **i64), torch.zeros(m + 1, **i64), scratch_for(m), torch.zeros(2, **i64)
    eargs = (flat2.data_ptr(), off2.data_ptr(), sq.data_ptr(), sf.data_ptr(), sc.data_ptr(), m, K)
    ix.dev_edit_windows_tally(*eargs, nh.data_ptr(), tally.data_ptr(), None, None, None, stream, 0)
    scan(nh, m, hoff, hscratch)
    torch.cuda.synchronize()
    nhits, columns = int(hoff[-1].item()), int(tally[0].item())
    hg, he = torch.zeros(max(nhits, 1), **i64), torch.zeros(max(nhits, 1), **u8)

    def rescue_scan():
        ix.dev_edit_windows(*eargs, nh.data_ptr(), None, None, None, stream, 0)
        scan(nh, m, hoff, hscratch)
        ix.dev_edit_windows(*eargs, None, hoff.data_ptr(), hg.data_ptr(), he.data_ptr(), stream, 0)

    rescue_scan()
    torch.cuda.synchronize()
    # the best hit of every slot: the smallest (distance, position) (tensor glue; pair_best_hit_kernel in the library)
    hit_slot = owner[torch.repeat_interleave(torch.arange(m, **i64), nh[:m], output_size=nhits)]
    none = torch.full((slots,), 1 << 62, **i64)
    best = none.clone().scatter_reduce_(0, hit_slot, (he[:nhits].long() << 40) | hg[:nhits], "amin")
    has = best != none
    bg = torch.where(has, best & ((1 << 40) - 1), torch.zeros_like(best)).contiguous()
    be = torch.where(has, best >> 40, torch.full_like(best, 255)).to(torch.uint8).contiguous()
    tl, rn, rops = torch.zeros(slots, **i32), torch.zeros(slots, **u8), torch.zeros(slots * 17, **i32)

    def rescue_align():
        ix.dev_edit_align(flat2.data_ptr(), off2.data_ptr(), wq.data_ptr(), bg.data_ptr(), be.data_ptr(), slots, K, tl.data_ptr(), rn.data_ptr(),
                          rops.data_ptr(), stream, 0)

    rescue_align()
    torch.cuda.synchronize()
    # the rescued candidates as awry_map_t records (tensor glue; pair_rescued_kernel in the library)
    ok = has & (rn != 0)
    resc = torch.zeros(slots, 4, **i64)
    resc[:, 0], resc[:, 1] = bg, bg + tl.long()
    resc[:, 2] = torch.where(ok, be.long(), torch.full_like(bg, 0xFFFFFFFF))
    resc[:, 3] = 0xFFFFFFFF | ((wq.long() & 1) << 32) | (4 << 48)
    n_rec, rec_off, pscratch, ins = torch.zeros(nq, **i64), torch.zeros(nq + 1, **i64), scratch_for(nq), torch.zeros(P, **i32)
    pargs = (kept_off.data_ptr(), cands.data_ptr(), resc.data_ptr(), rstatus.data_ptr(), P, MN, MX, U, G)
    ix.dev_pair_select(*pargs, n_rec.data_ptr(), None, None, None, None, None, stream, 0)
    scan(n_rec, nq, rec_off, pscratch)
    torch.cuda.synchronize()
    nrec = int(rec_off[-1].item())
    recs, rsel = torch.zeros(max(nrec, 1), 4, **i64), torch.zeros(max(nrec, 1), **i32)

    def pair_select():
        ix.dev_pair_select(*pargs, n_rec.data_ptr(), None, None, None, None, None, stream, 0)
        scan(n_rec, nq, rec_off, pscratch)
        ix.dev_pair_select(*pargs, None, rec_off.data_ptr(), recs.data_ptr(), rsel.data_ptr(), None, ins.data_ptr(), stream, 0)

    pair_select()
    torch.cuda.synchronize()
    rs = rsel[:nrec].long() & 0xFFFFFFFF
    from_chain = rs[(rs & 0x80000000) == 0]
    fill_pairs, runs_pairs = cigar_fill(cand_aln[from_chain].long())
    # the yardstick's last two stages: one record per read, and its CIGAR
    select_single, _, _, sel1, n1 = selection(1)
    fill_single, runs_single = cigar_fill(sel1[:n1].long())

    def pipeline():
        expand()
        both.seeding_and_chaining()
        both.count_pass()
        select_kept()
        windows()
        rescue_scan()
        rescue_align()
        pair_select()
        fill_pairs()

    def yardstick():
        expand()
        both.seeding_and_chaining()
        both.count_pass()
        select_single()
        fill_single()

    pipeline()
    t_ms = alternating7({"pipeline": pipeline, "yardstick": yardstick, "expand": expand, "seeding_and_chaining_doubled": both.seeding_and_chaining,
                         "alignment_count_pass_all_candidates": both.count_pass, "select_kept_lists": select_kept, "pair_windows": windows,
                         "rescue_scan": rescue_scan, "rescue_align": rescue_align, "pair_select": pair_select, "fill_pass_chain_records": fill_pairs})
    flags = (recs[:nrec, 3] >> 48) & 0xFFFF
    p_ms, y_ms, s_ms = t_ms["pipeline"]["median_ms"], t_ms["yardstick"]["median_ms"], t_ms["rescue_scan"]["median_ms"]
    n_windows = int((wc > 0).sum().item())
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "min_len": MIN_LEN, "max_hits": MAX_HITS, "band": BAND, "chains_per_strand": A,
           "min_insert": MN, "max_insert": MX, "unpaired_penalty": U, "rescue_anchors": G, "rescue_edits": K, "sub_window": SUB, "params": PARAMS,
           "seed_k": ix.seed_kmer_len(), "n_pairs": P, "read_len": L, "pairs_with_an_unseedable_mate": n_hard,
           "timing": "awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean: median and spread ((max - min) / median)",
           "candidates_kept": ncand, "window_slots": slots, "windows": n_windows, "window_pieces": m, "text_columns_scanned": columns, "window_hits": nhits,
           "slots_with_a_hit": int(has.sum().item()), "records": nrec, "records_proper": int(((flags & 2) != 0).sum().item()),
           "records_rescued": int(((flags & 4) != 0).sum().item()), "records_mate_unmapped": int(((flags & 8) != 0).sum().item()),
           "runs_chain_records": runs_pairs, "runs_single_end": runs_single, **t_ms,
           "pairs_per_s": P / (p_ms * 1e-3), "pipeline_ms_over_yardstick_ms": p_ms / y_ms,
           "rescue_scan_us_per_window": 1e3 * s_ms / max(n_windows, 1), "rescue_scan_ns_per_text_column": 1e6 * s_ms / max(2 * columns, 1),
           "rescue_share_of_pipeline": (s_ms + t_ms["rescue_align"]["median_ms"]) / p_ms}
    nb = min(P, 100_000)
    pv = both.pv
    qb = q[:2 * nb].reshape(-1).cpu().numpy()
    qo = (torch.arange(2 * nb + 1, dtype=torch.int64) * L).numpy().astype("uint64")
    ix.parallel_map_pairs_csr(qb, qo, MIN_LEN, MAX_HITS, A, BAND, MN, MX, U, G, K, *pv)
    t = time.time()
    r = ix.parallel_map_pairs_csr(qb, qo, MIN_LEN, MAX_HITS, A, BAND, MN, MX, U, G, K, *pv)
    dt = time.time() - t
    ix.parallel_map_csr(qb, qo, MIN_LEN, MAX_HITS, A, 1, BAND, *pv)
    t = time.time()
    r1 = ix.parallel_map_csr(qb, qo, MIN_LEN, MAX_HITS, A, 1, BAND, *pv)
    dt1 = time.time() - t
    out["host_boundary"] = {"n_pairs": nb, "map_pairs_batch_seconds": dt, "pairs_per_s": nb / dt, "records": int(r[0][-1]),
                            "records_rescued": int(((r[1]["flags"] & 4) != 0).sum()), "map_batch_seconds_same_reads": dt1, "records_single_end": int(r1[0][-1])}
    out["clipped_leg"] = host_legs(ix, q, nb, pv, not E2E_ONLY)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
