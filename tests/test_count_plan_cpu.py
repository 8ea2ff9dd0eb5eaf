"""The count plan (awry_amd/csrc/count_plan.h) as a pure function: a stand-alone program compiled against the header alone
evaluates plan_kmers / plan_reads / plan_name on a table of (facts, n, L, use_seed, tally or ragged), and every row's schedule,
flags, grids and name are compared with values written by hand from the launchers this plan replaced (launch_count_nt2,
launch_count_nt2_long, launch_count_nt2_wide, seed_rung's guard, kmer_table_wanted).  Each row names the condition it pins; the
rows sit on both sides of every threshold those launchers had."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include "count_plan.h"
using namespace awry;
static const char* sched(CountSchedule s) {
  switch (s) {
    case CountSchedule::STRIDED_QUADS: return "STRIDED_QUADS";
    case CountSchedule::LDS_CHUNKS: return "LDS_CHUNKS";
    case CountSchedule::QUAD4: return "QUAD4";
    case CountSchedule::PROBE_RESUME: return "PROBE_RESUME";
    case CountSchedule::PROBE_THEN_RESUME: return "PROBE_THEN_RESUME";
    case CountSchedule::READS_SINGLE: return "READS_SINGLE";
    case CountSchedule::READS_LISTS: return "READS_LISTS";
    case CountSchedule::READS_LANES: return "READS_LANES";
    case CountSchedule::WIDE_SINGLE: return "WIDE_SINGLE";
    case CountSchedule::WIDE_TWO_PHASE: return "WIDE_TWO_PHASE";
  }
  return "?";
}
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = std::fopen(argv[1], "r");
  if (!in) return 3;
  char kind;
  CountFacts f;
  int b[12];
  unsigned long long bwt_len, n;
  int L, use_seed, flag;
  while (std::fscanf(in, " %c %d %d %llu %d %d %d %d %u %d %d %d %d %d %d %d %d %u %u %d %d %d %d %d %llu %d %d %d", &kind, &f.alphabet, &b[0], &bwt_len,
                     &f.seed_k, &b[1], &b[2], &b[3], &f.dense_ratio, &b[4], &f.kt_mode, &b[5], &f.num_cus, &f.probe_resume_per_cu[0],
                     &f.probe_resume_per_cu[1], &f.probe_resume_per_cu[2], &f.probe_resume_per_cu[3], &f.lcx_reads_grid[0], &f.lcx_reads_grid[1],
                     &f.forced, &b[6], &b[7], &b[8], &b[9], &n, &L, &use_seed, &flag) == 28) {
    f.wide = b[0]; f.bwt_len = bwt_len; f.seed = b[1]; f.seed64 = b[2]; f.text4 = b[3]; f.lcx_key = b[4]; f.verify_kmers = b[5];
    f.rungs_off = b[6]; f.table_off = b[7]; f.rung_failed = b[8]; f.table_failed = b[9];
    const CountPlan p = kind == 'k' ? plan_kmers(f, n, L, use_seed != 0, flag != 0) : plan_reads(f, n, L, use_seed != 0, flag != 0);
    std::printf("%s %d %d %d %d %u %u %u|%s\n", sched(p.schedule), (int)p.seeded, (int)p.verify, (int)p.rung, (int)p.table, p.blocks, p.items_per_query,
                p.lcx_grid, plan_name(p));
  }
  static_assert(SEED_RUNG_MIN == 6 && SEED_RUNG_MAX == 16 && SEED_RUNG_MIN_BATCH == 4096 && KMER_TABLE_MIN_BATCH == 65536, "thresholds");
  static_assert(LIST_MAX_LISTS == 4096 && LCX_LF_CHUNK == 256, "limits of the kernels");
  return std::feof(in) ? 0 : 4;
}
'''

FIELDS = ("alphabet", "wide", "bwt_len", "seed_k", "seed", "seed64", "text4", "dense_ratio", "lcx_key", "kt_mode", "verify_kmers", "num_cus", "per_cu",
          "lcx_reads_grid", "forced", "rungs_off", "table_off", "rung_failed", "table_failed")
# A narrow nucleotide replica with everything resident.  4^12 / 3 = 5592405: SPARSE sits on the rule's boundary, DENSE one row past it.
# per_cu and lcx_reads_grid hold four / two different numbers so that a row shows which of them the plan took.
SPARSE = dict(alphabet=0, wide=0, bwt_len=5592405, seed_k=12, seed=1, seed64=0, text4=1, dense_ratio=1, lcx_key=1, kt_mode=-1, verify_kmers=0, num_cus=256,
              per_cu=(8, 6, 5, 4), lcx_reads_grid=(512, 768), forced=-1, rungs_off=0, table_off=0, rung_failed=0, table_failed=0)
DENSE = dict(SPARSE, bwt_len=5592406)
# a wide-row replica: 64-bit rows have none of the 32-bit accelerators
WIDE = dict(SPARSE, wide=1, seed=0, seed64=1, text4=0, dense_ratio=0, lcx_key=0, lcx_reads_grid=(0, 0))

QUAD, CHUNK, QUAD4 = "count_nt2_quad_kernel", "count_nt2_chunk_kernel", "count_nt2_quad4_kernel"
ONE, PAIR = "count_nt2_probe_resume_kernel", "count_nt2_probe_kernel+count_nt2_resume_kernel"
RUNG = ONE + " (table of its own for this length; batches of 4096 queries and more)"
TABLE = ONE + " (k-mer count table of this length: on first use with awry_set_kmer_table(1), else for batches of 65536 queries and more)"
READS, LISTS = "count_nt2_reads_kernel", "count_nt2_reads_probe_kernel+count_nt2_reads_kernel"
LANES = "count_nt2_reads_probe_kernel+lcx_quad_reads_kernel+count_nt2_reads_pool_kernel"
WIDE1, WIDE2 = "count_nt2_wide_kernel", "count_nt2_wide_probe_kernel+count_nt2_wide_kernel"
G32 = 1 << 32
BIG = 1 << 20  # awry_count_schedule's batch


def F(base, **kw):
    assert set(kw) <= set(FIELDS), kw
    return dict(base, **kw)


# (kind, facts, n, L, use_seed, tally (k) / ragged (r))  ->  (schedule, seeded, verify, rung, table, blocks, items_per_query, lcx_grid, name)
# blocks != 0: the grid (and the number of survivor lists); blocks == 0: grid_for(n * items_per_query, 256)
ROWS = [
    # ---- launch_count_nt2: count_kernel_mode's rule (1 << 2k) / 3 >= bwt_len, seeded only
    ("k", SPARSE, 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 6, 0, 0, TABLE)),  # 4^12 / 3 == bwt_len: mode 3; grid num_cus * per_cu[2 * 0 + vfy]
    ("k", DENSE, 65536, 31, 1, 0, ("QUAD4", 1, 0, 0, 0, 0, 1, 0, QUAD4)),              # one row more: mode 2, grid_for(n, 256), verify only on request
    ("k", F(DENSE, seed_k=13), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 6, 0, 0, TABLE)),  # 4^13 / 3 = 22369621 >= bwt_len
    ("k", F(SPARSE, seed_k=0), 65536, 31, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),  # no seed table: seeded = use_seed && seed_k > 0 && ...
    ("k", SPARSE, 65536, 31, 0, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),               # use_seed off: not seeded, so the rule gives 2
    # ---- the two-phase branch: vfy = text4 && dense_ratio == 1 picks the instantiation and the grid
    ("k", SPARSE, 65536, 31, 1, 1, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 4, 0, 0, TABLE)),                 # tally: per_cu[2 * 1 + 1]
    ("k", F(SPARSE, text4=0), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 0, 0, 0, 256 * 8, 0, 0, ONE)),       # no text: per_cu[0], and no table (needs vfy)
    ("k", F(SPARSE, dense_ratio=8), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 0, 0, 0, 256 * 8, 0, 0, ONE)),  # dense SA at ratio 8: the same
    ("k", F(SPARSE, text4=0), 65536, 31, 1, 1, ("PROBE_RESUME", 1, 0, 0, 0, 256 * 5, 0, 0, ONE)),       # tally without vfy: per_cu[2]
    ("k", SPARSE, G32 - 1, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 6, 0, 0, TABLE)),                # n < 2^32
    ("k", SPARSE, G32, 31, 1, 0, ("QUAD4", 1, 0, 0, 0, 0, 1, 0, QUAD4)),                                 # n == 2^32: kmode 3 falls through to the groups of four
    # ---- kmer_table_wanted and the launcher's own conditions (!pair && vfy && !rung && lcx_key && L > seed_k)
    ("k", SPARSE, 65535, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),                     # policy: below KMER_TABLE_MIN_BATCH
    ("k", F(SPARSE, kt_mode=1), 1, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 6, 0, 0, TABLE)),         # awry_set_kmer_table(1): whatever the batch
    ("k", F(SPARSE, kt_mode=0), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),       # awry_set_kmer_table(0): never
    ("k", F(SPARSE, table_off=1), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),     # AWRY_KMER_TABLE=0 under policy
    ("k", F(SPARSE, table_off=1, kt_mode=1), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),  # ... and over awry_set_kmer_table(1)
    ("k", F(SPARSE, kt_mode=0, table_off=1), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),
    ("k", F(SPARSE, lcx_key=0), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),       # no left-context index: no bucket to answer
    ("k", F(SPARSE, table_failed=1), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),  # kmer_table() returned nullptr: the same launch without
    ("k", F(SPARSE, table_failed=1, kt_mode=1), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),
    ("k", SPARSE, 65536, 12, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),                     # L == seed_k: the entry is the answer, L > seed_k fails
    ("k", SPARSE, 65536, 13, 1, 0, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 6, 0, 0, TABLE)),                   # L == seed_k + 1
    ("k", SPARSE, 65536, 32, 1, 0, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 6, 0, 0, TABLE)),                   # the longest k-mer
    ("k", F(SPARSE, forced=3), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),        # a forced schedule keeps its searches under policy
    ("k", F(SPARSE, forced=3, kt_mode=1), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 1, 256 * 6, 0, 0, TABLE)),  # kt_mode == 1 comes before the override
    ("k", F(SPARSE, forced=4, kt_mode=1), 65536, 31, 1, 0, ("PROBE_THEN_RESUME", 1, 1, 0, 0, 256 * 8, 0, 0, PAIR)),  # pair: no table
    ("k", F(SPARSE, forced=5, kt_mode=1), 65536, 31, 1, 0, ("PROBE_THEN_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, PAIR)),
    # ---- the rung: use_seed && seed_k > L && seed.p && 4096 <= n < 2^32 && no override, and seed_rung's guard (switch, alphabet, 6 <= L <= 16, not refused)
    ("k", SPARSE, 4096, 11, 1, 0, ("PROBE_RESUME", 1, 1, 1, 0, 256 * 6, 0, 0, RUNG)),          # L == seed_k - 1: kmode 3 whatever the index size
    ("k", DENSE, 4096, 11, 1, 0, ("PROBE_RESUME", 1, 1, 1, 0, 256 * 6, 0, 0, RUNG)),
    ("k", DENSE, 4096, 11, 1, 1, ("PROBE_RESUME", 1, 1, 1, 0, 256 * 4, 0, 0, RUNG)),           # tally
    ("k", F(DENSE, kt_mode=1), 4096, 11, 1, 0, ("PROBE_RESUME", 1, 1, 1, 0, 256 * 6, 0, 0, RUNG)),  # a rung launch takes no count table
    ("k", SPARSE, 4095, 11, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),                      # small batch: LF steps, unseeded, so the rule gives 2
    ("k", SPARSE, G32 - 1, 11, 1, 0, ("PROBE_RESUME", 1, 1, 1, 0, 256 * 6, 0, 0, RUNG)),
    ("k", SPARSE, G32, 11, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", SPARSE, 4096, 5, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),                       # L < SEED_RUNG_MIN
    ("k", SPARSE, 4096, 6, 1, 0, ("PROBE_RESUME", 1, 1, 1, 0, 256 * 6, 0, 0, RUNG)),           # L == SEED_RUNG_MIN
    ("k", F(SPARSE, seed_k=18), 4096, 16, 1, 0, ("PROBE_RESUME", 1, 1, 1, 0, 256 * 6, 0, 0, RUNG)),  # L == 16 (a seed k beyond what the library builds, to reach the bound)
    ("k", F(SPARSE, seed_k=18), 4096, 17, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),        # L == 17: no rung of 4^17 entries
    ("k", SPARSE, 4096, 11, 0, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),                      # use_seed off
    ("k", F(SPARSE, seed=0), 4096, 11, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),           # r.seed.p == nullptr
    ("k", F(SPARSE, rungs_off=1), 4096, 11, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),      # AWRY_SEED_RUNGS=0
    ("k", F(SPARSE, rung_failed=1), 4096, 11, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),    # seed_rung() returned nullptr (HBM budget)
    ("k", F(SPARSE, alphabet=1), 4096, 11, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),       # seed_rung: nucleotide only
    ("k", F(SPARSE, forced=3), 4096, 11, 1, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),         # an override: no rung, and kmode 3 unseeded is the groups of four
    ("k", F(SPARSE, forced=0), 4096, 11, 1, 0, ("STRIDED_QUADS", 0, 0, 0, 0, 0, 4, 0, QUAD)),
    ("k", F(SPARSE, text4=0), 4096, 11, 1, 0, ("PROBE_RESUME", 1, 0, 1, 0, 256 * 8, 0, 0, RUNG)),  # a rung without the verify accelerators
    # ---- every forced schedule, seeded and unseeded (SPARSE: the policy alone would say 3)
    ("k", F(SPARSE, forced=0), 65536, 31, 1, 0, ("STRIDED_QUADS", 1, 0, 0, 0, 0, 4, 0, QUAD)),  # grid_for(n * 4, 256)
    ("k", F(SPARSE, forced=0), 65536, 31, 0, 0, ("STRIDED_QUADS", 0, 0, 0, 0, 0, 4, 0, QUAD)),
    ("k", F(SPARSE, forced=1), 65536, 31, 1, 0, ("LDS_CHUNKS", 1, 0, 0, 0, 0, 4, 0, CHUNK)),
    ("k", F(SPARSE, forced=1), 65536, 31, 0, 1, ("LDS_CHUNKS", 0, 0, 0, 0, 0, 4, 0, CHUNK)),
    ("k", F(SPARSE, forced=2), 65536, 31, 1, 0, ("QUAD4", 1, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(SPARSE, forced=2), 65536, 31, 0, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(DENSE, forced=3), 65536, 31, 1, 0, ("PROBE_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, ONE)),
    ("k", F(DENSE, forced=3), 65536, 31, 0, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),          # kmode 3..5 unseeded: groups of four
    ("k", F(DENSE, forced=4), 65536, 31, 1, 0, ("PROBE_THEN_RESUME", 1, 1, 0, 0, 256 * 8, 0, 0, PAIR)),   # mode 4: num_cus * 8
    ("k", F(DENSE, forced=4), 65536, 31, 1, 1, ("PROBE_THEN_RESUME", 1, 1, 0, 0, 256 * 8, 0, 0, PAIR)),
    ("k", F(DENSE, forced=4), 65536, 31, 0, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(DENSE, forced=4), G32, 31, 1, 0, ("QUAD4", 1, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(DENSE, forced=5), 65536, 31, 1, 0, ("PROBE_THEN_RESUME", 1, 1, 0, 0, 256 * 6, 0, 0, PAIR)),   # mode 5: the one launch's grid
    ("k", F(DENSE, forced=5), 65536, 31, 1, 1, ("PROBE_THEN_RESUME", 1, 1, 0, 0, 256 * 4, 0, 0, PAIR)),
    ("k", F(DENSE, forced=5, text4=0), 65536, 31, 1, 0, ("PROBE_THEN_RESUME", 1, 0, 0, 0, 256 * 8, 0, 0, PAIR)),
    ("k", F(DENSE, forced=5), 65536, 31, 0, 0, ("QUAD4", 0, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(DENSE, forced=6), 65536, 31, 1, 0, ("STRIDED_QUADS", 1, 0, 0, 0, 0, 4, 0, QUAD)),   # any other number: the strided quads
    # ---- the groups of four verify only on request, and only with the accelerators
    ("k", F(DENSE, verify_kmers=1), 65536, 31, 1, 0, ("QUAD4", 1, 1, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(DENSE, verify_kmers=1, text4=0), 65536, 31, 1, 0, ("QUAD4", 1, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(DENSE, verify_kmers=1, dense_ratio=8), 65536, 31, 1, 0, ("QUAD4", 1, 0, 0, 0, 0, 1, 0, QUAD4)),
    ("k", F(DENSE, verify_kmers=1, forced=0), 65536, 31, 1, 0, ("STRIDED_QUADS", 1, 0, 0, 0, 0, 4, 0, QUAD)),  # (the strided quads have no VERIFY)
    # ---- launch_count_nt2_wide for k-mers: sdw = use_seed && seed_k > 0 && seed64 && seed_k <= L; two-phase only forced (3..5) and n < 2^32
    ("k", WIDE, 65536, 31, 1, 0, ("WIDE_SINGLE", 1, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("k", WIDE, 65536, 31, 0, 0, ("WIDE_SINGLE", 0, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("k", F(WIDE, seed64=0), 65536, 31, 1, 0, ("WIDE_SINGLE", 0, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("k", F(WIDE, forced=2), 65536, 31, 1, 0, ("WIDE_SINGLE", 1, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("k", F(WIDE, forced=3), 65536, 31, 1, 0, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),
    ("k", F(WIDE, forced=3), 65536, 31, 1, 1, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),
    ("k", F(WIDE, forced=4), 65536, 31, 1, 0, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),
    ("k", F(WIDE, forced=5), 65536, 31, 1, 0, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),
    ("k", F(WIDE, forced=3, seed64=0), 65536, 31, 1, 0, ("WIDE_SINGLE", 0, 0, 0, 0, 0, 4, 0, WIDE1)),  # no wide table: nothing to probe
    ("k", F(WIDE, forced=3), 65536, 31, 0, 0, ("WIDE_SINGLE", 0, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("k", F(WIDE, forced=3), 65536, 12, 1, 0, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),   # L == seed_k
    ("k", F(WIDE, forced=3), 65536, 11, 1, 0, ("WIDE_SINGLE", 0, 0, 0, 0, 0, 4, 0, WIDE1)),            # L < seed_k: no rung on wide rows either
    ("k", F(WIDE, forced=3), G32 - 1, 31, 1, 0, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),
    ("k", F(WIDE, forced=3), G32, 31, 1, 0, ("WIDE_SINGLE", 1, 0, 0, 0, 0, 4, 0, WIDE1)),
    # ---- launch_count_nt2_long: sd = use_seed && seed_k > 0 && (ragged || seed_k <= L); two-phase when
    #      vfy && sd && L - seed_k >= 3 && L <= 512 && n < 2^32 && (no override || 3..5), on num_cus * 8 blocks; lanes = lcx_key && vfy &&
    #      lcx_reads_grid[ragged] > 0 && nblk <= LIST_MAX_LISTS && lcx_lf_list_bound(slots) <= 2^32 - 1
    ("r", SPARSE, 5000, 101, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),
    ("r", DENSE, 5000, 101, 1, 1, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 768, LANES)),                        # ragged: the other instantiation's grid
    ("r", F(SPARSE, lcx_key=0), 5000, 101, 1, 0, ("READS_LISTS", 1, 1, 0, 0, 256 * 8, 0, 0, LISTS)),
    ("r", F(SPARSE, lcx_reads_grid=(0, 768)), 5000, 101, 1, 0, ("READS_LISTS", 1, 1, 0, 0, 256 * 8, 0, 0, LISTS)),
    ("r", F(SPARSE, lcx_reads_grid=(0, 768)), 5000, 101, 1, 1, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 768, LANES)),
    ("r", F(SPARSE, text4=0), 5000, 101, 1, 0, ("READS_SINGLE", 1, 0, 0, 0, 0, 4, 0, READS)),                  # grid_for(n * 4, 256), <S, V = false>
    ("r", F(SPARSE, dense_ratio=8), 5000, 101, 1, 0, ("READS_SINGLE", 1, 0, 0, 0, 0, 4, 0, READS)),
    ("r", SPARSE, 5000, 101, 0, 0, ("READS_SINGLE", 0, 1, 0, 0, 0, 4, 0, READS)),                              # use_seed off: <S = false, V = true>
    ("r", F(SPARSE, seed_k=0), 5000, 101, 1, 0, ("READS_SINGLE", 0, 1, 0, 0, 0, 4, 0, READS)),
    ("r", SPARSE, 5000, 14, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),                               # L - seed_k == 2
    ("r", SPARSE, 5000, 15, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),                        # L - seed_k == 3
    ("r", SPARSE, 5000, 11, 1, 0, ("READS_SINGLE", 0, 1, 0, 0, 0, 4, 0, READS)),                               # L == seed_k - 1, equal lengths: not seeded
    ("r", SPARSE, 5000, 11, 1, 1, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),                               # ... ragged reads decide per read
    ("r", SPARSE, 5000, 12, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),                               # L == seed_k
    ("r", SPARSE, 5000, 13, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),                               # L == seed_k + 1
    ("r", SPARSE, 5000, 32, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),                        # (the reads launcher takes short reads too)
    ("r", SPARSE, 5000, 33, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),
    ("r", SPARSE, 5000, 512, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),
    ("r", SPARSE, 5000, 513, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),
    # slots = ceil(n / (2048 * 256)) * 256 * 2048; bound = slots + 15 * ceil(slots / 241) + 4 * 512 * 256:
    # 7711 * 2^19 = 4042784768 slots -> 4294934671 <= 2^32 - 1; 7712 * 2^19 -> 4295491584
    ("r", SPARSE, 4042784768, 101, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),
    ("r", SPARSE, 4042784769, 101, 1, 0, ("READS_LISTS", 1, 1, 0, 0, 256 * 8, 0, 0, LISTS)),
    ("r", SPARSE, 4042260481, 101, 1, 1, ("READS_LISTS", 1, 1, 0, 0, 256 * 8, 0, 0, LISTS)),                   # ragged, grid 768: 7710 * 2^19 is the last that fits
    ("r", SPARSE, 4042260480, 101, 1, 1, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 768, LANES)),
    ("r", SPARSE, G32 - 1, 101, 1, 0, ("READS_LISTS", 1, 1, 0, 0, 256 * 8, 0, 0, LISTS)),
    ("r", SPARSE, G32, 101, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),
    ("r", F(SPARSE, num_cus=512), 5000, 101, 1, 0, ("READS_LANES", 1, 1, 0, 0, 4096, 0, 512, LANES)),          # num_cus * 8 == LIST_MAX_LISTS
    ("r", F(SPARSE, num_cus=513), 5000, 101, 1, 0, ("READS_LISTS", 1, 1, 0, 0, 4104, 0, 0, LISTS)),            # one CU more: the prefix sums no longer fit LDS
    ("r", F(SPARSE, forced=0), 5000, 101, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),
    ("r", F(SPARSE, forced=1), 5000, 101, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),
    ("r", F(SPARSE, forced=2), 5000, 101, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),
    ("r", F(SPARSE, forced=3), 5000, 101, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),
    ("r", F(SPARSE, forced=4), 5000, 101, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),
    ("r", F(SPARSE, forced=5), 5000, 101, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),
    ("r", F(SPARSE, forced=5, lcx_key=0), 5000, 101, 1, 0, ("READS_LISTS", 1, 1, 0, 0, 256 * 8, 0, 0, LISTS)),
    ("r", F(SPARSE, forced=6), 5000, 101, 1, 0, ("READS_SINGLE", 1, 1, 0, 0, 0, 4, 0, READS)),
    ("r", F(SPARSE, forced=3), 5000, 101, 0, 0, ("READS_SINGLE", 0, 1, 0, 0, 0, 4, 0, READS)),
    ("r", F(SPARSE, kt_mode=1, verify_kmers=1), 5000, 101, 1, 0, ("READS_LANES", 1, 1, 0, 0, 256 * 8, 0, 512, LANES)),  # k-mer switches: not read
    # ---- launch_count_nt2_wide for reads: sdw = use_seed && seed_k > 0 && seed64 && (ragged || seed_k <= L)
    ("r", WIDE, 5000, 101, 1, 0, ("WIDE_SINGLE", 1, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("r", WIDE, 5000, 101, 1, 1, ("WIDE_SINGLE", 1, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("r", F(WIDE, forced=3), 5000, 101, 1, 0, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),
    ("r", F(WIDE, forced=3), 5000, 101, 1, 1, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),
    ("r", F(WIDE, forced=3), 5000, 11, 1, 0, ("WIDE_SINGLE", 0, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("r", F(WIDE, forced=3), 5000, 11, 1, 1, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),            # ragged: seeded whatever L
    ("r", F(WIDE, forced=3), 5000, 513, 1, 0, ("WIDE_TWO_PHASE", 1, 0, 0, 0, 256 * 8, 0, 0, WIDE2)),           # (no length bound on wide rows)
    ("r", F(WIDE, forced=3, seed64=0), 5000, 101, 1, 0, ("WIDE_SINGLE", 0, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("r", F(WIDE, forced=3), G32, 101, 1, 0, ("WIDE_SINGLE", 1, 0, 0, 0, 0, 4, 0, WIDE1)),
    ("r", F(WIDE, forced=2), 5000, 101, 1, 0, ("WIDE_SINGLE", 1, 0, 0, 0, 0, 4, 0, WIDE1)),
]

# What awry_count_schedule(L) returns: the name of the plan for n = 2^20, seeded, no census -- the k-mer plan up to L = 32, the reads
# plan above.  The strings the GPU tests assert, from the facts those tests set up.
REPEAT3M = F(SPARSE, bwt_len=3_000_004, seed_k=13)  # test_count_one_launch_gpu: 3 Mbp, default k = 13 (4^13 >= 12 n), all accelerators
PARITY1M = F(SPARSE, bwt_len=1_000_002, seed_k=12)  # test_gpu_parity.test_default_device_policies: 1 Mbp, k = 12
CENSUS = F(SPARSE, bwt_len=200_003, seed_k=8)       # test_count_census_gpu's narrow index (dense SA 1, verify, lcx), a seed k of the test's
REPORT = [
    ("k", F(REPEAT3M, forced=3), BIG, 31, 1, 0, ONE), ("k", F(REPEAT3M, forced=4), BIG, 31, 1, 0, PAIR), ("k", F(REPEAT3M, forced=5), BIG, 31, 1, 0, PAIR),
    ("k", F(REPEAT3M, forced=3), BIG, 32, 1, 0, ONE), ("k", F(REPEAT3M, forced=4), BIG, 32, 1, 0, PAIR), ("k", F(REPEAT3M, forced=5), BIG, 32, 1, 0, PAIR),
    ("k", F(REPEAT3M, forced=3), BIG, 13, 1, 0, ONE), ("k", F(REPEAT3M, forced=4), BIG, 13, 1, 0, PAIR), ("k", F(REPEAT3M, forced=5), BIG, 13, 1, 0, PAIR),
    ("k", REPEAT3M, BIG, 11, 1, 0, RUNG),                                   # test_rung_table_takes_the_one_launch: L = k - 2
    ("k", F(SPARSE, bwt_len=1_000_004, seed_k=12), BIG, 6, 1, 0, RUNG),     # test_kmers_shorter_than_the_seed_table: L = 6, 7, 9, 10
    ("k", F(SPARSE, bwt_len=1_000_004, seed_k=12), BIG, 10, 1, 0, RUNG),
    ("k", PARITY1M, BIG, 31, 1, 0, TABLE),                                  # "probe" in it: 4^12 >= 3 n
    ("k", F(PARITY1M, seed_k=8), BIG, 31, 1, 0, QUAD4),                     # after set_seed_kmer_len(8)
    ("k", F(PARITY1M, seed_k=8), BIG, 5, 1, 0, QUAD4),                      # L = 5 < SEED_RUNG_MIN
    ("k", F(CENSUS, forced=3), BIG, 31, 1, 0, ONE),                         # test_count_census_gpu: exactly the kernel's name under mode 3
    ("k", F(CENSUS, forced=3), BIG, 8, 1, 0, ONE),
    ("k", F(SPARSE, kt_mode=1), BIG, 31, 1, 0, TABLE),                      # test_kmer_table*_gpu: "k-mer count table" in it ...
    ("k", F(SPARSE, dense_ratio=2, lcx_key=0), BIG, 31, 1, 0, ONE),         # ... and not after set_locate_sa_ratio(2)
    ("k", WIDE, BIG, 31, 1, 0, WIDE1),                                      # the wide-row cases: "wide" / "count_nt2_wide_kernel" in it
    ("k", F(WIDE, forced=3), BIG, 31, 1, 0, WIDE2),                         # test_inflight_gpu: "count_nt2_wide_probe_kernel" under mode 3
    ("r", SPARSE, BIG, 101, 1, 0, LANES),                                   # test_count_plan_gpu: reads with / without the left-context index
    ("r", F(SPARSE, lcx_key=0), BIG, 101, 1, 0, LISTS),
    ("r", F(SPARSE, text4=0, lcx_key=0), BIG, 101, 1, 0, READS),
    ("k", F(SPARSE, kt_mode=0), BIG, 31, 1, 0, ONE),                        # test_count_plan_gpu: set_kmer_table(0)
]


def line(kind, facts, n, L, use_seed, flag):
    f = [facts[k] for k in FIELDS]
    flat = [v for x in f for v in (x if isinstance(x, tuple) else (x,))]
    return " ".join([kind] + [str(int(v)) for v in flat + [n, L, use_seed, flag]])


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """-> {input line: output line} of the stand-alone program over every row of both tables"""
    d = tmp_path_factory.mktemp("count_plan")
    src, exe, rows = d / "plan.cpp", d / "plan", d / "rows.txt"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "awry_amd", "csrc"), str(src), "-o", str(exe)])
    lines = [line(*r[:6]) for r in ROWS + REPORT]
    rows.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([str(exe), str(rows)], text=True, timeout=60).splitlines()
    assert len(out) == len(lines)
    return dict(zip(lines, out))


def test_the_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "count_plan.h"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "awry_amd", "csrc"), str(src)])
    text = open(os.path.join(ROOT, "awry_amd", "csrc", "count_plan.h")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text


def test_every_row_of_the_table(plans):
    assert len(ROWS) > 120
    bad = []
    for row in ROWS:
        sched, seeded, verify, rung, table, blocks, per_query, lcx_grid, name = row[6]
        want = "%s %d %d %d %d %d %d %d|%s" % (sched, seeded, verify, rung, table, blocks, per_query, lcx_grid, name)
        got = plans[line(*row[:6])]
        if got != want:
            bad.append((row[0], {k: v for k, v in row[1].items() if SPARSE[k] != v}, row[2:6], want, got))
    assert not bad, bad


def test_the_table_covers_every_schedule_and_both_sides_of_the_flags():
    scheds = {r[6][0] for r in ROWS}
    assert scheds == {"STRIDED_QUADS", "LDS_CHUNKS", "QUAD4", "PROBE_RESUME", "PROBE_THEN_RESUME", "READS_SINGLE", "READS_LISTS", "READS_LANES",
                      "WIDE_SINGLE", "WIDE_TWO_PHASE"}
    for col in range(1, 5):  # seeded, verify, rung, table
        assert {r[6][col] for r in ROWS} == {0, 1}, col
    for forced in range(-1, 6):
        for use_seed in (0, 1):
            assert any(r[0] == "k" and not r[1]["wide"] and r[1]["forced"] == forced and r[4] == use_seed and r[3] == 31 for r in ROWS), (forced, use_seed)


def test_the_strings_the_gpu_tests_assert(plans):
    for row in REPORT:
        assert plans[line(*row[:6])].split("|", 1)[1] == row[6], row
