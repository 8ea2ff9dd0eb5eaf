"""Rates of locate within k edits (awry_locate_edit_batch, edit_kernels.hip.h) on the repeat-rich GRCh38-shaped text
(tests/synth.repeat_rich_text, as bench.py): 101-bp reads with 3 edits -- 2 substitutions and 1 insertion or deletion -- at
k = 1, 3, 5 and max_candidates = MAX_CANDIDATES.  Per k:
  * the host batch call (the whole pipeline, transfers included): wall time, reads/s, share of reads abandoned, hits per read;
  * the pipeline again on the device, stage by stage with the device entry points and torch for the glue (piece count for
    locate, scan, locate, diagonals + sort + windows, awry_dev_edit_windows count pass / scan / fill pass): device-event time
    of each stage, windows and text columns per read from the census, the scan kernel's columns/s, and that rate against
    the kernel's own ceiling (VALU_PER_COLUMN[W] 32-bit VALU instructions per column, counted from the ISA of the count pass's
    column loop -- a 64-bit operation is a pair of them -- against the issue rate VALU_LANE_OPS_PER_S).  The device form builds
    the pattern masks per window and runs at 4 words per column (the batch driver: per query, 2 words for 101-bp reads), so
    its scan times are an upper bound of the batch driver's; a kernel trace of this tool separates the two by W.
The yardstick in the same process and on the same reads: the anchors count pass, 7 repetitions, median and spread.
usage: time_edit.py [text_len] [n_reads] [k,k,..]   -> one JSON object on stdout"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import awry_amd
from tests import synth
from tools.read_sets import L, plant, timed

FULL = 3_100_000_000
MAX_CANDIDATES = 1000
# edit_scan_kernel<A, W, count>, gfx950: VALU instructions in the column loop, by W (12 + 39 per word: 19.5 64-bit operations
# per column and word), and what the card issues: 256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz
VALU_PER_COLUMN = {1: 51, 2: 90, 3: 129, 4: 166}
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else FULL
nq = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
ks = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 3, 5]
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def with_indel(q, seed):
    """q: uint8[n, L + 1] on the device, windows of L + 1 letters.  -> uint8[n, L]: one insertion (a random letter; the window's
    last two letters fall off) or one deletion (the window's letter L moves in) per row, at a position 5 or more from either end"""
    gen = torch.Generator(device=q.device)
    gen.manual_seed(seed)
    rows, cols = q.shape[0], q.shape[1] - 1
    at = torch.randint(5, cols - 5, (rows, 1), device=q.device, generator=gen)
    ins = torch.rand((rows, 1), device=q.device, generator=gen) < 0.5
    j = torch.arange(cols, device=q.device)[None, :]
    src = torch.where(ins, torch.where(j > at, j - 1, j), torch.where(j >= at, j + 1, j))
    out = torch.gather(q, 1, src)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=q.device)
    new = lut[torch.randint(0, 4, (rows,), device=q.device, generator=gen)]
    r = torch.arange(rows, device=q.device)
    out[r, at[:, 0]] = torch.where(ins[:, 0], new, out[r, at[:, 0]])
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def device_pipeline(ix, flat, off, k, n_text):
    """the chunk driver's stages on the device -> dict of stage times and the census"""
    w = k + 1
    t = torch.arange(w, device=dev)
    begins = (t * L) // w
    poff = torch.cat([(off[:-1, None] + begins[None, :]).reshape(-1), off[-1:]]).contiguous()
    npieces = nq * w
    counts = torch.zeros(npieces, dtype=torch.int64, device=dev)
    words = torch.zeros(2 * npieces, dtype=torch.int64, device=dev)
    hoff = torch.zeros(npieces + 1, dtype=torch.int64, device=dev)
    scratch = torch.zeros(ix.dev_scan_scratch_bytes(max(npieces, 4 * nq)) // 8 + 8, dtype=torch.int64, device=dev)
    st = {}
    st["count_pieces_ms"], _ = event_ms(lambda: ix.dev_count_ascii_for_locate(flat.data_ptr(), poff.data_ptr(), npieces, counts.data_ptr(), words.data_ptr(),
                                                                              None, stream, 0))

    def cap():
        c = counts.view(nq, w)
        over = c.sum(1) > MAX_CANDIDATES
        c[over] = 0
        return over
    st["cap_ms"], over = event_ms(cap)
    st["scan_ms"], _ = event_ms(lambda: ix.dev_scan_counts(counts.data_ptr(), npieces, hoff.data_ptr(), scratch.data_ptr(), stream, 0))
    total = int(hoff[-1].item())
    gpos = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
    st["locate_pieces_ms"], _ = event_ms(lambda: ix.dev_locate(words.data_ptr(), hoff.data_ptr(), npieces, total, gpos.data_ptr(), None, stream, 0))

    def make_windows():
        piece = torch.repeat_interleave(torch.arange(npieces, device=dev), counts)
        q = piece // w
        diag = gpos[:total] - begins[piece % w]  # may be negative
        key = q * (1 << 33) + (diag + L)
        key = torch.sort(key).values
        q, d = key >> 33, (key & ((1 << 33) - 1)) - L
        head = torch.ones(total, dtype=torch.bool, device=dev)
        head[1:] = (q[1:] != q[:-1]) | (d[1:] - d[:-1] > 2 * k + 1)
        tail = torch.ones(total, dtype=torch.bool, device=dev)
        tail[:-1] = head[1:]
        lo = (d[head] - k).clamp(min=0)
        hi = (d[tail] + k).clamp(max=n_text - 1)
        return q[head].to(torch.int32).contiguous(), lo.contiguous(), (hi - lo + 1).clamp(min=0).to(torch.int32).contiguous()
    st["diagonals_sort_windows_ms"], (wq, wfirst, wcount) = event_ms(make_windows)
    m = int(wq.numel())
    nh = torch.zeros(m, dtype=torch.int64, device=dev)
    whoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    args = (flat.data_ptr(), off.data_ptr(), wq.data_ptr(), wfirst.data_ptr(), wcount.data_ptr(), m, k)
    ix.dev_edit_windows(*args, nh.data_ptr(), None, None, None, stream, 0)  # (warm: the mask workspace grows here)
    torch.cuda.synchronize()
    st["scan_count_pass_ms"] = timed(lambda: ix.dev_edit_windows(*args, nh.data_ptr(), None, None, None, stream, 0), 1, 3)
    ix.dev_scan_counts(nh.data_ptr(), m, whoff.data_ptr(), scratch.data_ptr(), stream, 0)
    nhits = int(whoff[-1].item())
    hg = torch.zeros(max(nhits, 1), dtype=torch.int64, device=dev)
    he = torch.zeros(max(nhits, 1), dtype=torch.uint8, device=dev)
    st["scan_fill_pass_ms"] = timed(lambda: ix.dev_edit_windows(*args, None, whoff.data_ptr(), hg.data_ptr(), he.data_ptr(), stream, 0), 1, 3)
    tally = torch.zeros(2, dtype=torch.int64, device=dev)
    ix.dev_edit_windows_tally(*args, nh.data_ptr(), tally.data_ptr(), None, None, None, stream, 0)
    torch.cuda.synchronize()
    cols, wins = [int(x) for x in tally.cpu().tolist()]
    st.update(candidates_per_read=total / nq, windows_per_read=wins / nq, columns_per_read=cols / nq, hits=nhits, abandoned=int(over.sum().item()),
              words_per_column=4, scan_columns_per_s=cols / (st["scan_count_pass_ms"] * 1e-3))
    st["scan_ceiling_columns_per_s"] = VALU_LANE_OPS_PER_S / VALU_PER_COLUMN[4]
    st["scan_fraction_of_ceiling"] = st["scan_columns_per_s"] / st["scan_ceiling_columns_per_s"]
    return st


def main():
    t = time.time()
    text, starts, headers, info = synth.repeat_rich_text(n, 11, 25, device="cuda")
    log("text %.1f s" % (time.time() - t))
    t = time.time()
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, starts, headers, build_device=0)
    ix.set_devices([0])
    log("index + replica %.1f s" % (time.time() - t))
    out = {"text": "synth.repeat_rich_text(%d, 11, 25)" % n, "text_len": n, "full_size_text": n == FULL, "n_reads": nq, "read_len": L,
           "reads": "windows of the text with 2 substitutions and 1 insertion or deletion", "max_candidates": MAX_CANDIDATES, "seed_k": ix.seed_kmer_len(),
           "valu_per_column_by_words": VALU_PER_COLUMN, "valu_lane_ops_per_s": VALU_LANE_OPS_PER_S, "k": {}}
    text_d = torch.from_numpy(text).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(503)
    pos = torch.randint(0, text_d.numel() - 2 - L, (nq,), device=dev, generator=gen)
    wide = text_d[pos[:, None] + torch.arange(L + 1, device=dev)[None, :]]
    reads = with_indel(torch.cat([plant(wide[:, :L].contiguous(), 2, 7), wide[:, L:]], 1), 9)
    del text_d
    off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * L
    flat = torch.cat([reads.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    n_rec = torch.zeros(nq, dtype=torch.int64, device=dev)
    ms = sorted(timed(lambda: ix.dev_anchors(flat.data_ptr(), off.data_ptr(), nq, 1, 0, n_rec.data_ptr(), None, None, None, stream, 0)) for _ in range(7))
    out["yardstick"] = {"what": "awry_dev_anchors count pass (skip 0, min_len 1), 7 repetitions of a warmed 5-launch mean", "ms": ms, "median_ms": ms[3],
                        "spread": (ms[-1] - ms[0]) / ms[3]}
    log("yardstick", json.dumps(out["yardstick"]))
    qb = reads.reshape(-1).cpu().numpy()
    qo = np.arange(nq + 1, dtype=np.uint64) * np.uint64(L)
    for k in ks:
        ix.parallel_locate_edit_csr(qb[:L * 1000], qo[:1001], k, MAX_CANDIDATES, want_pos=False)  # warm
        t = time.time()
        hoff, g, _, d, status = ix.parallel_locate_edit_csr(qb, qo, k, MAX_CANDIDATES, want_pos=False)
        wall = time.time() - t
        leg = {"host_batch_s": wall, "host_batch_reads_per_s": nq / wall, "share_abandoned": float((status != 0).mean()), "hits_per_read": len(g) / nq,
               "reads_with_a_hit": float((np.diff(hoff.astype(np.int64)) > 0).mean())}
        leg["device_stages"] = device_pipeline(ix, flat, off, k, n - 1)
        out["k"][str(k)] = leg
        log("k", k, json.dumps(leg))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
