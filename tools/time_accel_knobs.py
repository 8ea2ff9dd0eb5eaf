"""Wall time of replica construction and of every accelerator knob, for comparing two builds of the library: on a 20-Mbp synthetic
text, `runs` times set_devices([0]) and then the knob sequence of tools/accel_launch_sequence.py (the order in which
tests/test_accel_audit_gpu.py walks the knobs), one time per call and run.
usage: time_accel_knobs.py [--runs 7] [--text-len 20000000] OUT.json           one process of one build
       time_accel_knobs.py --merge RESULT.json parent=A.json,B.json result=C.json,D.json
           -> per call and build the median and spread ((max - min) / median) over the processes' runs, result over parent, and whether
              that ratio lies within 1 +- the parent's own spread"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(args):
    import awry_amd
    from tests import synth
    from tools.accel_launch_sequence import knob_sequence

    text, st, hd = synth.make_text(args.text_len, 0, 0xA5A50002, 3, 0.02)
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, st, hd, build_device=0)
    seconds, states = {}, []
    for run in range(args.runs + 1):  # the first run warms the process (code objects, pools) and is not counted
        t = time.perf_counter()
        ix.set_devices([0])
        calls = [("set_devices([0])", time.perf_counter() - t)]
        k = ix.seed_kmer_len()
        state = []
        for name, call in knob_sequence(ix, k):
            t = time.perf_counter()
            call()
            calls.append((name, time.perf_counter() - t))
            a = ix.debug_accelerators()
            state.append([ix.seed_kmer_len(), a["seed_pos"], a["ctx_extra"], int(ix.lcx_enabled()), int(a["dense_ratio"]), int(ix.verify_enabled())])
        states.append(state)
        if run:
            for name, s in calls:
                seconds.setdefault(name, []).append(round(s, 5))
    ix.close()
    assert all(s == states[0] for s in states)
    json.dump({"text_len": args.text_len, "seed_k": k, "runs": args.runs, "seconds": seconds, "state_after_each_knob": states[0]}, open(args.out, "w"), indent=1)
    for name, s in seconds.items():
        print("%-30s median %.4f s" % (name, statistics.median(s)))


def merge(out, groups):
    loaded = {}
    for g in groups:
        build, files = g.split("=")
        loaded[build] = [json.load(open(f)) for f in files.split(",")]
    first = loaded["parent"][0]
    calls = {}
    for name in first["seconds"]:
        row = {}
        for build, procs in loaded.items():
            s = sorted(x for p in procs for x in p["seconds"][name])
            med = statistics.median(s)
            row[build] = {"median_seconds": round(med, 5), "spread": round((s[-1] - s[0]) / med, 4), "seconds": s,
                          "medians_per_process": [round(statistics.median(p["seconds"][name]), 5) for p in procs]}
        row["result_over_parent"] = round(row["result"]["median_seconds"] / row["parent"]["median_seconds"], 4)
        row["within_parent_spread"] = abs(row["result_over_parent"] - 1) <= row["parent"]["spread"]
        calls[name] = row
    same = all(p["state_after_each_knob"] == first["state_after_each_knob"] and p["seed_k"] == first["seed_k"] for procs in loaded.values() for p in procs)
    json.dump({"text": "synth.make_text(%d, 0, 0xA5A50002, 3, 0.02)" % first["text_len"], "seed_k": first["seed_k"],
               "runs_per_process": {b: [p["runs"] for p in procs] for b, procs in loaded.items()},
               "processes": {b: len(p) for b, p in loaded.items()}, "same_state_after_each_knob": same, "calls": calls}, open(out, "w"), indent=1)
    for name, row in calls.items():
        print("%-30s parent %.4f s (spread %.3f)  result %.4f s  ratio %.4f  %s" % (name, row["parent"]["median_seconds"], row["parent"]["spread"],
              row["result"]["median_seconds"], row["result_over_parent"], "ok" if row["within_parent_spread"] else "OUTSIDE"))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3:])
    else:
        ap = argparse.ArgumentParser()
        ap.add_argument("--runs", type=int, default=7)
        ap.add_argument("--text-len", type=int, default=20_000_000)
        ap.add_argument("out")
        measure(ap.parse_args())
