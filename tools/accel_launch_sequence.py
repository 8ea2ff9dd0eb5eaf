"""The kernel launches that build, convert and drop the device-only accelerators (awry_amd/csrc/accelerators.h), for comparing two
builds of the library: on one process the default replica of a 5.4-kbp nucleotide text, of a 20-k amino text and of the nucleotide
text on forced wide rows; on the nucleotide replica every knob in the order tests/test_accel_audit_gpu.py walks them
(test_the_table_after_every_transition); then on the default replica of a 20-kbp text (seed k = 9) one packed count of 4096 8-mers,
which builds the rung of that length, and after set_kmer_table(1) one of 4096 20-mers, which builds the k-mer count table.
usage: rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/accel_launch_sequence.py     run under a kernel trace
       python3 tools/accel_launch_sequence.py --list <dir>      -> the traced launches in dispatch order, one `kernel grid` line each
Two builds drive the kernels alike when the two lists are equal (diff them)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.launch_sequence import listing  # noqa: E402


def knob_sequence(ix, k):
    """the calls of test_the_table_after_every_transition after the default replica, as (name, call)"""
    return [("set_lcx(0)", lambda: ix.set_lcx(False)), ("set_lcx(1)", lambda: ix.set_lcx(True)),
            ("set_verify(-1)", lambda: ix.set_verify(-1)), ("set_verify(2)", lambda: ix.set_verify(2)),
            ("set_locate_sa_ratio(3)", lambda: ix.set_locate_sa_ratio(3)), ("set_locate_sa_ratio(0)", lambda: ix.set_locate_sa_ratio(0)),
            ("set_verify(2) after ratio 0", lambda: ix.set_verify(2)),
            ("set_seed_kmer_len(k - 1)", lambda: ix.set_seed_kmer_len(k - 1)), ("set_seed_kmer_len(8)", lambda: ix.set_seed_kmer_len(8)),
            ("set_seed_kmer_len(6)", lambda: ix.set_seed_kmer_len(6)), ("set_seed_kmer_len(7)", lambda: ix.set_seed_kmer_len(7)),
            ("set_seed_kmer_len(-1)", lambda: ix.set_seed_kmer_len(-1)), ("set_devices([0, 0])", lambda: ix.set_devices([0, 0]))]


def run():
    import awry_amd
    from tests import synth

    lib = awry_amd.load_library()
    text, st, hd = synth.make_text(5_400, 0, 3, 3, 0.02)
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    k = ix.seed_kmer_len()
    state = [(k, ix.debug_accelerators()["seed_pos"], ix.lcx_enabled())]
    atext, ast, ahd = synth.make_text(20_000, 1, 62, 3, 0.01)
    aa = awry_amd.FmIndex.from_text(atext, 1, 8, 0, ast, ahd).set_devices([0])
    state.append((aa.seed_kmer_len(), aa.debug_accelerators()["seed_pos"], aa.lcx_enabled()))
    aa.close()
    wide = awry_amd.FmIndex.from_text(text, 0, 8, 0, st, hd)
    lib.awry_debug_force_wide_rows(1)
    try:
        wide.set_devices([0])
    finally:
        lib.awry_debug_force_wide_rows(0)
    state.append((wide.seed_kmer_len(), wide.debug_accelerators()["seed_entry_bytes"], wide.lcx_enabled()))
    wide.close()
    for name, call in knob_sequence(ix, k):
        call()
        a = ix.debug_accelerators()
        state.append((name, ix.seed_kmer_len(), a["seed_pos"], ix.lcx_enabled(), int(a["dense_ratio"]), ix.verify_enabled(), bool(a["sa_nblock"])))
    ix.close()
    text, st, hd = synth.make_text(20_000, 0, 61, 2, 0.02)
    ix = awry_amd.FmIndex.from_text(text, 0, 8, 0, st, hd).set_devices([0])
    assert ix.seed_kmer_len() == 9 and ix.lcx_enabled()
    n8 = int(ix.count_kmers_nt2(synth.sampled_queries(text, 4096, 8, 8), True).sum())
    ix.set_kmer_table(1)
    n20 = int(ix.count_kmers_nt2(synth.sampled_queries(text, 4096, 20, 20), True).sum())
    info = ix.kmer_table_info()
    assert ix.debug_seed_rung(8) is not None and info["length"] == 20 and info["lines"] >= 1, info
    state.append((n8, n20, info["length"], info["entries"], info["lines"]))
    ix.close()
    for s in state:
        print(s)


if __name__ == "__main__":
    listing(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--list" else run()
