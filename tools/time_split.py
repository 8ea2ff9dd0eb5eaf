"""Cost of the split selection (awry_dev_map_select_split, kernels_split.hip.h) against the clipped map level's selection
(awry_dev_map_select_clip at max_report = 2) on the same device-resident alignment records in the same process: tools/time_clip.py's
workload -- the repeat-rich text (tests/synth.repeat_rich_text, as bench.py), 101-bp windows with 3 planted substitutions, every third
read with a random tail -- where every sixth read is replaced by a chimera of 60 letters of one window and 41 of another.  The doubled
batch (awry_dev_revcomp), the first A chains of every query of both strands and their clipped alignment records are built once
(tools/time_clip.py's steps over both strands); then, per selection, device time (awry_dev_timer_*, 7 alternating repetitions of a warmed
5-launch mean, median and spread) of
  count pass          records per read, and the reads' status;
  fill pass           the records, at the offsets of the selection's own count pass;
and what the selections report for the chimeras.  The yardstick is the clipped selection at R = 2.
usage: time_split.py [text_len] [n_reads]   -> one JSON object on stdout (profiles/split_rates.json)"""
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
n = int(float(argv[0])) if len(argv) > 0 else 50_000_000
nq = int(float(argv[1])) if len(argv) > 1 else 600_000
MIN_LEN, MAX_HITS, BAND, L, A = 12, 50, 4, 101, 4
WEIGHTS = (1, 4, 6, 5)
T = 0
SPLITS = {"split_p2": (2, 1, 50), "split_p4": (4, 2 * A, 50)}  # (max_segments, max_secondary, max_overlap)
P = dict(max_seeds=1024, lookback=16, max_gap=500, max_skew=50, min_score=20)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
i64 = dict(dtype=torch.int64, device=dev)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def reads_with_chimeras(text_d):
    """tools/time_clip.py's reads (3 substitutions, every third read a random tail of 20..40 letters), every sixth replaced by the
    first 60 letters of one window followed by the first 41 of another"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(503)
    ar = torch.arange(L, device=dev)
    pos = torch.randint(0, text_d.numel() - 1 - L, (nq,), device=dev, generator=gen)
    q = plant(text_d[pos[:, None] + ar[None, :]], 3, 8)
    tail = torch.randint(20, 41, (nq,), device=dev, generator=gen)
    tail[torch.arange(nq, device=dev) % 3 != 0] = 0
    nt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    junk = nt[torch.randint(0, 4, (nq, L), device=dev, generator=gen)]
    q = torch.where(ar[None, :] >= (L - tail)[:, None], junk, q)
    pos2 = torch.randint(0, text_d.numel() - 1 - L, (nq,), device=dev, generator=gen)
    chim = torch.where(ar[None, :] < 60, text_d[pos[:, None] + ar[None, :]], text_d[pos2[:, None] + (ar[None, :] - 60).clamp(min=0)])
    code = torch.full((256,), ord("A"), dtype=torch.uint8, device=dev)
    code[nt.long()] = nt
    is_chim = torch.arange(nq, device=dev) % 6 == 5
    return torch.where(is_chim[:, None], code[chim.long()], q), is_chim


def first_chains(ix, flat, off, m_q):
    """SMEMs, located seeds, chains of the m_q queries (tools/time_clip.py's steps), then the first min(chains, A) chains of every query
    -> (aln_off[m_q + 1], chain_query i32, member_off, members, chain records, m)"""
    pv = (P["max_seeds"], P["lookback"], P["max_gap"], P["max_skew"], P["min_score"])
    n_rec, rec_off = torch.zeros(m_q, **i64), torch.zeros(m_q + 1, **i64)
    scratch = torch.zeros(ix.dev_scan_scratch_bytes(m_q) // 8 + 1, **i64)
    ix.dev_smems(flat.data_ptr(), off.data_ptr(), m_q, MIN_LEN, n_rec.data_ptr(), None, None, None, stream, 0)
    ix.dev_scan_counts(n_rec.data_ptr(), m_q, rec_off.data_ptr(), scratch.data_ptr(), stream, 0)
    torch.cuda.synchronize()
    total = int(rec_off[-1].item())
    records = torch.zeros(3 * max(total, 1), **i64)
    ix.dev_smems(flat.data_ptr(), off.data_ptr(), m_q, MIN_LEN, None, rec_off.data_ptr(), records.data_ptr(), None, stream, 0)
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
    n_ch, n_mem, ch_off, mem_off = torch.zeros(m_q, **i64), torch.zeros(m_q, **i64), torch.zeros(m_q + 1, **i64), torch.zeros(m_q + 1, **i64)
    chains, members = torch.zeros(max(nhits, 1) * 4, **i64), torch.zeros(max(nhits, 1) * 2, **i64)
    ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), m_q, *pv, n_ch.data_ptr(), n_mem.data_ptr(), None, None, None, None, None, stream, 0)
    ix.dev_scan_counts(n_ch.data_ptr(), m_q, ch_off.data_ptr(), scratch.data_ptr(), stream, 0)
    ix.dev_scan_counts(n_mem.data_ptr(), m_q, mem_off.data_ptr(), scratch.data_ptr(), stream, 0)
    ix.dev_chain_seeds(seed_off.data_ptr(), seeds.data_ptr(), m_q, *pv, None, None, ch_off.data_ptr(), mem_off.data_ptr(), chains.data_ptr(), members.data_ptr(),
                       None, stream, 0)
    torch.cuda.synchronize()
    n_all = int(ch_off[-1].item())
    ch = chains.view(-1, 4)[:n_all]
    n_seeds = ch[:, 0] >> 32
    m_start = torch.cumsum(n_seeds, 0) - n_seeds  # a query's members lie back to back in chain order
    assert int(m_start[-1].item() + n_seeds[-1].item()) == int(mem_off[-1].item()), "members are not the chains' seeds back to back"
    take = torch.clamp(n_ch, max=A)
    aln_off = torch.zeros(m_q + 1, **i64)
    aln_off[1:] = torch.cumsum(take, 0)
    m = int(aln_off[-1].item())
    query = torch.repeat_interleave(torch.arange(m_q, **i64), take, output_size=m)
    idx = ch_off[:-1][query] + torch.arange(m, **i64) - aln_off[:-1][query]  # the chain's index among all chains
    sel_seeds = n_seeds[idx]
    sel_moff = torch.zeros(m + 1, **i64)
    sel_moff[1:] = torch.cumsum(sel_seeds, 0)
    nsel = int(sel_moff[-1].item())
    gidx = torch.repeat_interleave(m_start[idx] - sel_moff[:-1], sel_seeds, output_size=nsel) + torch.arange(nsel, **i64)
    return aln_off, query.to(torch.int32), sel_moff, members.view(-1, 2)[gidx].contiguous(), ch[idx].contiguous(), m


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("text, index, replica %.1f s" % (time.time() - t))
    q, is_chim = reads_with_chimeras(torch.from_numpy(text).to(dev))
    flat = torch.cat([q.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    off = torch.arange(nq + 1, **i64) * L
    flat2, off2 = torch.zeros(2 * nq * L + 16, dtype=torch.uint8, device=dev), torch.zeros(2 * nq + 1, **i64)
    ix.dev_revcomp(flat.data_ptr(), off.data_ptr(), nq, flat2.data_ptr(), off2.data_ptr(), stream, 0)
    torch.cuda.synchronize()
    aln_off, cq32, moff, mem, chains, m = first_chains(ix, flat2, off2, 2 * nq)
    alns, n_ops = torch.zeros(4 * max(m, 1), **i64), torch.zeros(max(m, 1), **i64)
    ix.dev_align_chains_clip(flat2.data_ptr(), off2.data_ptr(), cq32.data_ptr(), moff.data_ptr(), mem.data_ptr(), m, BAND, *WEIGHTS, alns.data_ptr(),
                             n_ops.data_ptr(), None, None, stream, 0, None)
    torch.cuda.synchronize()
    log("%d alignment records of %d reads, %.1f s" % (m, nq, time.time() - t))
    base = (aln_off.data_ptr(), alns.data_ptr(), chains.data_ptr(), None)
    sscratch = torch.zeros(ix.dev_scan_scratch_bytes(nq) // 8 + 1, **i64)
    calls = {"clip_r2": dict(words=5, call=lambda nm, rs, mo, mp: ix.dev_map_select_clip(*base, nq, A, 2, *WEIGHTS, T, nm, rs, mo, mp, None, None, stream, 0))}
    for name, (P_, R2, O) in SPLITS.items():
        calls[name] = dict(words=6, call=lambda nm, rs, mo, mp, s=(P_, R2, O): ix.dev_map_select_split(*base, off.data_ptr(), nq, A, *s, WEIGHTS[0], WEIGHTS[1], T,
                                                                                                      nm, rs, mo, mp, None, None, stream, 0))
    fns, facts = {}, {}
    for name, md in calls.items():
        n_maps, rstatus, map_off = torch.zeros(nq, **i64), torch.zeros(nq + 8, dtype=torch.uint8, device=dev), torch.zeros(nq + 1, **i64)
        md["call"](n_maps.data_ptr(), rstatus.data_ptr(), None, None)
        ix.dev_scan_counts(n_maps.data_ptr(), nq, map_off.data_ptr(), sscratch.data_ptr(), stream, 0)
        torch.cuda.synchronize()
        total = int(map_off[-1].item())
        maps = torch.zeros(md["words"] * max(total, 1), **i64)
        md["call"](None, None, map_off.data_ptr(), maps.data_ptr())
        torch.cuda.synchronize()
        md.update(n_maps=n_maps, rstatus=rstatus, map_off=map_off, maps=maps)
        fns[name + "_count_pass"] = lambda md=md: md["call"](md["n_maps"].data_ptr(), md["rstatus"].data_ptr(), None, None)
        fns[name + "_fill_pass"] = lambda md=md: md["call"](None, None, md["map_off"].data_ptr(), md["maps"].data_ptr())
        rec = maps.view(-1, md["words"])[:total]
        first = map_off[:-1][n_maps > 0]
        mapq = (rec[:, 3] >> 40) & 0xFF
        flags = (rec[:, 3] >> 48) & 0xFFFF
        chim_first = map_off[:-1][is_chim & (n_maps > 0)]
        two = is_chim & (n_maps > 1)
        second = map_off[:-1][two] + 1
        facts[name] = {"records": total, "reads_with_records": int(first.numel()), "chimeras": int(is_chim.sum().item()),
                       "chimeras_with_two_records": int(two.sum().item()), "chimera_primary_mapq_60": int((mapq[chim_first] == 60).sum().item()),
                       "chimera_second_flag_supplementary": int((flags[second] == 16).sum().item()),
                       "chimera_second_flag_secondary": int((flags[second] == 1).sum().item()),
                       "chimera_second_mapq_60": int((mapq[second] == 60).sum().item())}

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
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "n_reads": nq, "read_len": L,
           "reads": "tools/time_clip.py's; every sixth a 60 + 41 chimera of two windows", "min_len": MIN_LEN, "max_hits": MAX_HITS, "band": BAND,
           "chains_per_strand": A, "weights_a_b_g_E": WEIGHTS, "min_aln_score": T, "params": P, "alignment_records": m,
           "split_settings_P_R2_O": SPLITS, "timing": "awry_dev_timer_*, 7 alternating repetitions of a warmed 5-launch mean: median and spread ((max - min) / median)",
           "selections": facts, **tm}
    for name in SPLITS:
        both = tm[name + "_count_pass"]["median_ms"] + tm[name + "_fill_pass"]["median_ms"]
        out[name + "_both_passes_ms"] = both
        out[name + "_over_clip_r2"] = both / (tm["clip_r2_count_pass"]["median_ms"] + tm["clip_r2_fill_pass"]["median_ms"])
    out["clip_r2_both_passes_ms"] = tm["clip_r2_count_pass"]["median_ms"] + tm["clip_r2_fill_pass"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
