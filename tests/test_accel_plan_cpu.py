"""The accelerator plan (awry_amd/csrc/accel_plan.h) as pure functions: a stand-alone program compiled against the header alone
evaluates every decision on a table of rows, and each row's result is compared with a value written by hand from the rules
accelerators.h had between its HIP calls (default_seed_k, the verify policy of make_replica, refresh_nblock, sync_seed_mode,
build_lcx, seed_rung, build_kmer_table, the record buckets of make_replica).  Each row names the condition it pins; the rows sit on
both sides of every threshold.  The same program runs once more under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from tests import accel_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <cstring>
#include "accel_plan.h"
using namespace awry;
typedef unsigned long long ull;
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = std::fopen(argv[1], "r");
  if (!in) return 3;
  char line[512], fn[32];
  while (std::fgets(line, sizeof line, in)) {
    ull a[12] = {0};
    long long s[12] = {0};
    double d[2] = {0, 0};
    int used = 0;
    if (std::sscanf(line, "%31s%n", fn, &used) != 1) return 4;
    const char* rest = line + used;
    AccelFacts f;
    AccelHeld h;
    HbmFree free;
    int got = -1;
    if (!std::strcmp(fn, "seed_k")) {  // alphabet wide bwt_len request env_set env_value known free
      got = std::sscanf(rest, "%lld %lld %llu %lld %lld %lld %lld %llu", &s[0], &s[1], &a[0], &s[2], &s[3], &s[4], &s[5], &a[1]) - 8;
      f.alphabet = (int)s[0]; f.wide = s[1]; f.bwt_len = a[0]; f.seed_k_request = (int)s[2]; f.seed_k_env = s[3]; f.seed_k_env_value = (int)s[4];
      free.known = s[5]; free.bytes = a[1];
      std::printf("%d\n", seed_k_wanted(f, free));
    } else if (!std::strcmp(fn, "verify")) {  // wide bwt_len request env_off env_steps known free
      got = std::sscanf(rest, "%lld %llu %lld %lld %lld %lld %llu", &s[0], &a[0], &s[1], &s[2], &s[3], &s[4], &a[1]) - 7;
      f.wide = s[0]; f.bwt_len = a[0]; f.verify_request = (int)s[1]; f.verify_env_off = s[2]; f.verify_env_steps = (int)s[3];
      free.known = s[4]; free.bytes = a[1];
      std::printf("%d\n", verify_steps_wanted(f, free));
    } else if (!std::strcmp(fn, "nblock")) {  // alphabet wide dense_ratio nblock_rows
      got = std::sscanf(rest, "%lld %lld %u %llu", &s[0], &s[1], &h.dense_ratio, &a[0]) - 4;
      f.alphabet = (int)s[0]; f.wide = s[1]; f.nblock_rows = a[0];
      std::printf("%d\n", (int)nblock_wanted(f, h));
    } else if (!std::strcmp(fn, "seed_pos")) {  // alphabet wide bwt_len env_off seed_k seed dense_ratio text4 text8
      got = std::sscanf(rest, "%lld %lld %llu %lld %d %lld %u %lld %lld", &s[0], &s[1], &a[0], &s[2], &h.seed_k, &s[3], &h.dense_ratio, &s[4], &s[5]) - 9;
      f.alphabet = (int)s[0]; f.wide = s[1]; f.bwt_len = a[0]; f.seed_pos_off = s[2]; h.seed = s[3]; h.text4 = s[4]; h.text8 = s[5];
      std::printf("%d\n", (int)seed_pos_wanted(f, h));
    } else if (!std::strcmp(fn, "ctx_extra")) {  // alphabet sa_bits cap
      got = std::sscanf(rest, "%lld %llu %lld", &s[0], &a[0], &s[1]) - 3;
      f.alphabet = (int)s[0]; f.sa_bits = a[0]; f.ctx_extra_cap = (int)s[1];
      std::printf("%d\n", ctx_extra(f));
    } else if (!std::strcmp(fn, "lcx_wanted")) {  // request env_off
      got = std::sscanf(rest, "%lld %lld", &s[0], &s[1]) - 2;
      f.lcx_request = (int)s[0]; f.lcx_env_off = s[1];
      std::printf("%d\n", (int)lcx_wanted(f));
    } else if (!std::strcmp(fn, "lcx_possible")) {  // alphabet wide seed seed_k text4 dense_ratio
      got = std::sscanf(rest, "%lld %lld %lld %d %lld %u", &s[0], &s[1], &s[2], &h.seed_k, &s[3], &h.dense_ratio) - 6;
      f.alphabet = (int)s[0]; f.wide = s[1]; h.seed = s[2]; h.text4 = s[3];
      std::printf("%d\n", (int)lcx_possible(f, h));
    } else if (!std::strcmp(fn, "lcx_plan")) {  // bwt_len known free
      got = std::sscanf(rest, "%llu %lld %llu", &a[0], &s[0], &a[1]) - 3;
      free.known = s[0]; free.bytes = a[1];
      const LcxPlan p = lcx_plan(a[0], free);
      for (int t = 1; t <= 7; t++) std::printf("%llu:%llu ", (ull)p.lev_off[t], (ull)p.lev_n[t]);
      std::printf("%llu %.0f %d %llu %u\n", (ull)p.inner_total, p.resident, (int)p.admitted, (ull)p.chunk, p.max_bucket);
    } else if (!std::strcmp(fn, "rung_possible")) {  // rungs_off wide alphabet L
      got = std::sscanf(rest, "%lld %lld %lld %lld", &s[0], &s[1], &s[2], &s[3]) - 4;
      std::printf("%d\n", (int)rung_possible(s[0], s[1], (int)s[2], (int)s[3]));
    } else if (!std::strcmp(fn, "rung_admitted")) {  // L held_bytes cap_env_gb known free
      got = std::sscanf(rest, "%lld %lf %lf %lld %llu", &s[0], &d[0], &d[1], &s[1], &a[0]) - 5;
      free.known = s[1]; free.bytes = a[0];
      std::printf("%d\n", (int)rung_admitted((int)s[0], d[0], d[1], free));
    } else if (!std::strcmp(fn, "kt_possible")) {  // lcx text4 dense_ratio seed seed_k wide L
      got = std::sscanf(rest, "%lld %lld %u %lld %d %lld %lld", &s[0], &s[1], &h.dense_ratio, &s[2], &h.seed_k, &s[3], &s[4]) - 7;
      h.lcx = s[0]; h.text4 = s[1]; h.seed = s[2];
      std::printf("%d\n", (int)kmer_table_possible(h, s[3], (int)s[4]));
    } else if (!std::strcmp(fn, "kt_bits")) {  // keys L forced_lines
      got = std::sscanf(rest, "%llu %lld %llu", &a[0], &s[0], &a[1]) - 3;
      std::printf("%u\n", kmer_table_bits(a[0], (int)s[0], a[1]));
    } else if (!std::strcmp(fn, "kt_admitted")) {  // bits known free
      got = std::sscanf(rest, "%llu %lld %llu", &a[0], &s[0], &a[1]) - 3;
      free.known = s[0]; free.bytes = a[1];
      std::printf("%d\n", (int)kmer_table_admitted((uint32_t)a[0], free));
    } else if (!std::strcmp(fn, "seq_bucket")) {  // bwt_len nseq lds_records
      got = std::sscanf(rest, "%llu %llu %llu", &a[0], &a[1], &a[2]) - 3;
      const SeqBucketPlan p = seq_bucket_plan(a[0], a[1], a[2]);
      std::printf("%d %u %llu\n", (int)p.wanted, p.shift, (ull)p.buckets);
    }
    if (got != 0) return 5;  // an unknown function or a row with the wrong number of fields
  }
  static_assert(KT_TAG_BITS == 43 && AA_SEED_SIGMA == 21 && NUCLEOTIDE == 0, "what the rows below assume of layout.h");
  return std::feof(in) ? 0 : 6;
}
'''

NT, AA = 0, 1
GRCH38, CHR1, ECOLI, SWISSPROT = 3_100_000_000, 240_000_000, 4_600_000, 90_000_000
HBM = 288_000_000_000  # "ample": an empty MI355X
G32 = 1 << 32

# (function, arguments, expected output, the condition) -- the arguments in the order the program's comments give
ROWS = [
    # ---- default_seed_k, narrow nucleotide: the smallest k with 4^k >= 12 bwt_len, at most 17; then k-- while 10 * 4^k > 0.7 free
    ("seed_k", (NT, 0, GRCH38, -1, 0, 0, 1, HBM), "17", "GRCh38: 4^17 < 12 n, the loop stops at 17"),
    ("seed_k", (NT, 0, CHR1, -1, 0, 0, 1, HBM), "16", "chr1: 4^15 = 1.07e9 < 2.88e9 <= 4^16"),
    ("seed_k", (NT, 0, ECOLI, -1, 0, 0, 1, HBM), "13", "E. coli: 4^12 = 1.68e7 < 5.52e7 <= 4^13"),
    ("seed_k", (NT, 0, GRCH38, -1, 0, 0, 1, 245_426_702_628), "16", "10 * 4^17 / 0.7 = 245426702628.57: just below"),
    ("seed_k", (NT, 0, GRCH38, -1, 0, 0, 1, 245_426_702_629), "17", "... just above"),
    ("seed_k", (NT, 0, CHR1, -1, 0, 0, 1, 61_356_675_657), "15", "10 * 4^16 / 0.7 = 61356675657.14: just below"),
    ("seed_k", (NT, 0, CHR1, -1, 0, 0, 1, 61_356_675_658), "16", "... just above"),
    ("seed_k", (NT, 0, ECOLI, -1, 0, 0, 1, 958_698_057), "12", "10 * 4^13 / 0.7 = 958698057.14: just below"),
    ("seed_k", (NT, 0, ECOLI, -1, 0, 0, 1, 958_698_058), "13", "... just above"),
    ("seed_k", (NT, 0, ECOLI, -1, 0, 0, 1, 100), "1", "no room at all: k stops at 1"),
    ("seed_k", (NT, 0, ECOLI, -1, 0, 0, 0, 0), "13", "hipMemGetInfo failed: k is not cut"),
    ("seed_k", (NT, 0, 5_400, -1, 0, 0, 1, HBM), "8", "the 5.4-kbp text of the GPU audits: 4^8 = 65536 >= 64800"),
    ("seed_k", (NT, 0, 5_462, -1, 0, 0, 1, HBM), "9", "12 * 5462 = 65544 > 4^8"),
    ("seed_k", (NT, 0, ECOLI, 11, 0, 0, 1, 100), "11", "a request is taken as it is, whatever is free"),
    ("seed_k", (NT, 0, ECOLI, 0, 1, 9, 1, HBM), "0", "request 0: no table; AWRY_SEED_K is not asked"),
    # ---- AWRY_SEED_K: clamped to 0..17 (nucleotide) / 0..7 (amino), read only under the policy
    ("seed_k", (NT, 0, ECOLI, -1, 1, 99, 1, HBM), "17", "AWRY_SEED_K=99"),
    ("seed_k", (NT, 0, ECOLI, -1, 1, -5, 1, HBM), "0", "AWRY_SEED_K=-5"),
    ("seed_k", (NT, 0, ECOLI, -1, 1, 9, 1, 100), "9", "AWRY_SEED_K=9: whatever is free"),
    ("seed_k", (AA, 0, SWISSPROT, -1, 1, 9, 1, HBM), "7", "amino, AWRY_SEED_K=9"),
    ("seed_k", (AA, 0, SWISSPROT, -1, 1, -1, 1, HBM), "0", "amino, AWRY_SEED_K=-1"),
    ("seed_k", (NT, 1, G32, -1, 1, 20, 1, HBM), "17", "wide rows, AWRY_SEED_K=20"),
    ("seed_k", (NT, 1, G32, -1, 1, -1, 1, HBM), "0", "wide rows, AWRY_SEED_K=-1"),
    ("seed_k", (AA, 1, G32, -1, 1, 5, 1, HBM), "0", "wide amino: no table, before the environment is asked"),
    # ---- wide rows: min(17, floor(log4 n) + 2), then k-- while 20 * 4^k > 0.7 free, at least 1
    ("seed_k", (NT, 1, G32, -1, 0, 0, 1, HBM), "16", "2^32 rows: 17 by size, 20 * 4^17 = 3.4e11 > 0.7 * 288e9 >= 20 * 4^16"),
    ("seed_k", (NT, 1, G32, -1, 0, 0, 0, 0), "17", "... with no figure: not cut"),
    ("seed_k", (NT, 1, G32, -1, 0, 0, 1, 490_853_405_257), "16", "20 * 4^17 / 0.7 = 490853405257.14: just below"),
    ("seed_k", (NT, 1, G32, -1, 0, 0, 1, 490_853_405_258), "17", "... just above"),
    ("seed_k", (NT, 1, 5_400, -1, 0, 0, 1, HBM), "8", "forced wide rows on a small text: floor(6.2) + 2"),
    ("seed_k", (NT, 1, 5_400, -1, 0, 0, 1, 100), "1", "wide rows, no room: at least 1"),
    # ---- amino: min(7, floor(log20 n) + 1), then k-- while 8.5 * 21^k > 0.7 free
    ("seed_k", (AA, 0, SWISSPROT, -1, 0, 0, 1, HBM), "7", "Swiss-Prot: floor(6.11) + 1"),
    ("seed_k", (AA, 0, SWISSPROT, -1, 0, 0, 1, 21_870_360_000), "6", "8.5 * 21^7 = 15309252598.5 > 0.7 * 21870360000 = 15309252000"),
    ("seed_k", (AA, 0, SWISSPROT, -1, 0, 0, 1, 21_870_361_000), "7", "... <= 0.7 * 21870361000 = 15309252700"),
    ("seed_k", (AA, 0, 20_000, -1, 0, 0, 1, HBM), "4", "the amino text of the GPU audits: floor(3.31) + 1"),
    ("seed_k", (AA, 0, 10**12, -1, 0, 0, 1, 10**13), "7", "amino: at most 7"),
    # ---- the verify policy: 7 B per symbol under half of what is free; AWRY_VERIFY=0 off, =n the steps; default 2
    ("verify", (0, 10**9, -2, 0, 0, 1, 14_000_000_000), "-1", "7e9 < 0.5 * 14e9 fails: equal"),
    ("verify", (0, 10**9, -2, 0, 0, 1, 14_000_000_002), "2", "7e9 < 7000000001"),
    ("verify", (0, 10**9, -2, 0, 5, 1, HBM), "5", "AWRY_VERIFY=5"),
    ("verify", (0, 10**9, -2, 1, 0, 1, HBM), "-1", "AWRY_VERIFY=0"),
    ("verify", (0, 10**9, -2, 0, -3, 1, HBM), "2", "AWRY_VERIFY=-3: no step count, the default"),
    ("verify", (0, 10**9, -2, 0, 5, 1, 14_000_000_000), "-1", "AWRY_VERIFY=5 does not override the memory rule"),
    ("verify", (1, 10**9, -2, 0, 0, 1, HBM), "-1", "wide rows"),
    ("verify", (0, 10**9, -2, 0, 0, 0, 0), "-1", "no figure: not admitted"),
    ("verify", (0, 10**9, 3, 1, 0, 0, 0), "3", "awry_set_verify(3) before the replica: as asked"),
    ("verify", (0, 10**9, -1, 0, 5, 1, HBM), "-1", "awry_set_verify(-1) before the replica"),
    ("verify", (0, 10**9, 0, 0, 0, 1, HBM), "0", "awry_set_verify(0): verify at once"),
    # ---- the N block: nucleotide, 32-bit rows, locate walks (dense ratio != 1), 64 rows and more
    ("nblock", (NT, 0, 0, 63), "0", "63 rows"),
    ("nblock", (NT, 0, 0, 64), "1", "64 rows"),
    ("nblock", (NT, 0, 3, 64), "1", "a dense SA at ratio 3 still walks"),
    ("nblock", (NT, 0, 1, 64), "0", "ratio 1: no walk"),
    ("nblock", (NT, 1, 0, 64), "0", "wide rows"),
    ("nblock", (AA, 0, 0, 64), "0", "amino"),
    # ---- position seeds: nucleotide text4 and 4^k / 3 >= bwt_len (4^12 / 3 = 5592405); amino text8
    ("seed_pos", (NT, 0, 5_592_405, 0, 12, 1, 1, 1, 1), "1", "bwt_len == 4^k / 3"),
    ("seed_pos", (NT, 0, 5_592_406, 0, 12, 1, 1, 1, 1), "0", "one row more"),
    ("seed_pos", (NT, 0, 5_592_406, 0, 13, 1, 1, 1, 1), "1", "... is sparse again at k = 13"),
    ("seed_pos", (NT, 0, GRCH38, 0, 17, 1, 1, 1, 1), "1", "GRCh38 at k = 17: 4^17 / 3 = 5.7e9"),
    ("seed_pos", (NT, 0, GRCH38, 0, 16, 1, 1, 1, 1), "0", "GRCh38 at k = 16: 1.43e9"),
    ("seed_pos", (NT, 0, 5_592_405, 1, 12, 1, 1, 1, 1), "0", "AWRY_SEED_POS=0"),
    ("seed_pos", (NT, 1, 5_592_405, 0, 12, 1, 1, 1, 1), "0", "wide rows"),
    ("seed_pos", (NT, 0, 5_592_405, 0, 0, 1, 1, 1, 1), "0", "seed_k == 0"),
    ("seed_pos", (NT, 0, 5_592_405, 0, 12, 0, 1, 1, 1), "0", "no table of 8-byte entries"),
    ("seed_pos", (NT, 0, 5_592_405, 0, 12, 1, 2, 1, 1), "0", "dense SA at ratio 2"),
    ("seed_pos", (NT, 0, 5_592_405, 0, 12, 1, 0, 1, 1), "0", "no dense SA"),
    ("seed_pos", (NT, 0, 5_592_405, 0, 12, 1, 1, 0, 1), "0", "nucleotide without text4 (text8 alone does not do)"),
    ("seed_pos", (AA, 0, SWISSPROT, 0, 7, 1, 1, 0, 1), "1", "amino: text8, no density rule"),
    ("seed_pos", (AA, 0, SWISSPROT, 0, 1, 1, 1, 0, 1), "1", "amino at k = 1"),
    ("seed_pos", (AA, 0, SWISSPROT, 0, 7, 1, 1, 0, 0), "0", "amino without text8"),
    ("seed_pos", (AA, 0, SWISSPROT, 0, 7, 1, 3, 0, 1), "0", "amino, dense SA at ratio 3"),
    # ---- the left-context index: wanted (request, AWRY_LCX) and possible (k >= 8, text4, ratio-1 dense SA, narrow nucleotide)
    ("lcx_wanted", (-1, 0), "1", "the default request"),
    ("lcx_wanted", (1, 0), "1", "request 1"),
    ("lcx_wanted", (0, 0), "0", "awry_set_lcx(0)"),
    ("lcx_wanted", (-1, 1), "0", "AWRY_LCX=0"),
    ("lcx_possible", (NT, 0, 1, 8, 1, 1), "1", "k == 8"),
    ("lcx_possible", (NT, 0, 1, 7, 1, 1), "0", "k == 7"),
    ("lcx_possible", (NT, 0, 0, 8, 1, 1), "0", "no seed table"),
    ("lcx_possible", (NT, 0, 1, 8, 0, 1), "0", "no text4"),
    ("lcx_possible", (NT, 0, 1, 8, 1, 2), "0", "dense SA at ratio 2"),
    ("lcx_possible", (NT, 1, 1, 8, 1, 1), "0", "wide rows"),
    ("lcx_possible", (AA, 0, 1, 8, 1, 1), "0", "amino"),
    # ---- its sizes: level t has ceil(((n - 1 >> 4 t) + 1) / 16) * 16 + 16 keys at the running offset from 16; resident
    #      16 (n + 32) + 8 * total; admitted when resident + 96 * 2^24 <= 0.75 free; chunk = (0.75 free - resident) / 96 in 2^24..2^28
    ("lcx_plan", (17, 1, 2_147_487_253), "16:32 48:32 80:32 112:32 144:32 176:32 208:32 240 2704 0 0 0",
     "n = 17: one node per level; 2704 + 1610612736 > 0.75 * 2147487253 = 1610615439.75"),
    ("lcx_plan", (17, 1, 2_147_487_254), "16:32 48:32 80:32 112:32 144:32 176:32 208:32 240 2704 1 16777216 8388608",
     "... <= 1610615440.5: admitted, the smallest chunk, buckets up to half of it"),
    ("lcx_plan", (17, 1, 4_000_000_000), "16:32 48:32 80:32 112:32 144:32 176:32 208:32 240 2704 1 31249971 15624985", "(3e9 - 2704) / 96 = 31249971.8"),
    ("lcx_plan", (17, 1, HBM), "16:32 48:32 80:32 112:32 144:32 176:32 208:32 240 2704 1 268435456 16777216", "the chunk stops at 2^28, a bucket at 2^24"),
    ("lcx_plan", (17, 0, 0), "16:32 48:32 80:32 112:32 144:32 176:32 208:32 240 2704 0 0 0", "no figure: not admitted"),
    ("lcx_plan", (4097, 1, HBM), "16:288 304:48 352:32 384:32 416:32 448:32 480:32 512 70160 1 268435456 16777216",
     "n = 4097: 257, 17, 2, 1 .. keys -> 17, 2, 1 .. nodes + 1; 16 * 4129 + 8 * 512"),
    ("lcx_plan", (GRCH38, 1, HBM),
     "16:193750016 193750032:12109392 205859424:756864 206616288:47328 206663616:2976 206666592:208 206666800:32 206666832 51253335168 1 268435456 16777216",
     "GRCh38: 49.6 GB of keys and pairs, 1.65 GB of levels"),
    ("lcx_plan", (GRCH38, 1, 70_000_000_000),
     "16:193750016 193750032:12109392 205859424:756864 206616288:47328 206663616:2976 206666592:208 206666800:32 206666832 51253335168 0 0 0",
     "GRCh38 beside 218 GB of other things: 51.25e9 + 1.61e9 > 52.5e9"),
    # ---- a rung: lengths 6..16 of a narrow nucleotide replica; 10 B per entry under half of free; all rungs under the cap
    ("rung_possible", (0, 0, NT, 5), "0", "L = 5"),
    ("rung_possible", (0, 0, NT, 6), "1", "L = 6"),
    ("rung_possible", (0, 0, NT, 16), "1", "L = 16"),
    ("rung_possible", (0, 0, NT, 17), "0", "L = 17"),
    ("rung_possible", (1, 0, NT, 12), "0", "AWRY_SEED_RUNGS=0"),
    ("rung_possible", (0, 1, NT, 12), "0", "wide rows"),
    ("rung_possible", (0, 0, AA, 12), "0", "amino"),
    ("rung_admitted", (12, 0, 0, 1, 335_544_319), "0", "10 * 4^12 = 167772160 > 0.5 * 335544319"),
    ("rung_admitted", (12, 0, 0, 1, 335_544_320), "1", "... == 0.5 * 335544320"),
    ("rung_admitted", (12, 0, 0, 0, 0), "0", "no figure"),
    ("rung_admitted", (16, 13_640_261_632, 0, 1, HBM), "1", "held + 8 * 4^16 == 48e9"),
    ("rung_admitted", (16, 13_640_261_640, 0, 1, HBM), "0", "one entry more held: above the 48 GB cap"),
    ("rung_admitted", (16, 13_640_261_640, 50, 1, HBM), "1", "AWRY_SEED_RUNG_GB=50"),
    ("rung_admitted", (16, 13_640_261_640, -1, 1, HBM), "0", "AWRY_SEED_RUNG_GB=-1: the default"),
    ("rung_admitted", (16, 0, 30, 1, HBM), "0", "AWRY_SEED_RUNG_GB=30: 34.4 GB alone is above it"),
    ("rung_admitted", (6, 47_999_967_232, 0, 1, HBM), "1", "the smallest rung fills the cap to the byte: 8 * 4^6 = 32768"),
    ("rung_admitted", (6, 47_999_967_240, 0, 1, HBM), "0", "... and 8 bytes past it"),
    # ---- the count table: possible with the left-context index, text4, ratio-1 dense SA, seed table; seed_k < L <= 32
    ("kt_possible", (1, 1, 1, 1, 12, 0, 12), "0", "L == seed_k"),
    ("kt_possible", (1, 1, 1, 1, 12, 0, 13), "1", "L == seed_k + 1"),
    ("kt_possible", (1, 1, 1, 1, 12, 0, 32), "1", "L == 32"),
    ("kt_possible", (1, 1, 1, 1, 12, 0, 33), "0", "L == 33"),
    ("kt_possible", (0, 1, 1, 1, 12, 0, 20), "0", "no left-context index"),
    ("kt_possible", (1, 0, 1, 1, 12, 0, 20), "0", "no text4"),
    ("kt_possible", (1, 1, 2, 1, 12, 0, 20), "0", "dense SA at ratio 2"),
    ("kt_possible", (1, 1, 1, 0, 12, 0, 20), "0", "no seed table"),
    ("kt_possible", (1, 1, 1, 1, 12, 1, 20), "0", "wide rows"),
    # ---- its lines: 8 keys per line, the tag (2 L - bits) within KT_TAG_BITS = 43, a forced line count
    ("kt_bits", (1, 20, 0), "0", "1 key, L = 20: one line, a tag of 40 bits"),
    ("kt_bits", (8, 20, 0), "0", "8 keys: one line"),
    ("kt_bits", (9, 20, 0), "1", "9 keys: two lines"),
    ("kt_bits", (1 << 30, 20, 0), "27", "2^30 keys: 2^27 lines"),
    ("kt_bits", ((1 << 30) + 1, 20, 0), "28", "one key more"),
    ("kt_bits", (1, 32, 0), "21", "L = 32: 64 - bits <= 43"),
    ("kt_bits", (8, 32, 0), "21", ""),
    ("kt_bits", (9, 32, 0), "21", ""),
    ("kt_bits", (1 << 30, 32, 0), "27", "2^30 keys at L = 32: the load decides"),
    ("kt_bits", (1, 22, 0), "1", "L = 22: 44 - bits <= 43"),
    ("kt_bits", (1 << 30, 20, 1000), "9", "forced 1000 lines: 512, whatever the load"),
    ("kt_bits", (1 << 30, 32, 1000), "9", "... and whatever the tag"),
    ("kt_bits", (9, 20, 1024), "10", "forced 1024 lines"),
    ("kt_bits", (9, 20, 1), "0", "forced 1 line"),
    ("kt_bits", (9, 20, 1 << 50), "40", "a forced count stops at 2^40 lines"),
    ("kt_admitted", (20, 1, 268_443_647), "0", "128 * 2^20 + 4096 = 134221824 > 0.5 * 268443647"),
    ("kt_admitted", (20, 1, 268_443_648), "1", "... == 0.5 * 268443648"),
    ("kt_admitted", (0, 0, 0), "0", "no figure"),
    # ---- the record buckets: more records than the kernels' LDS copy (1024) and fewer than 2^32; about 4 buckets per record, at most 2^22
    ("seq_bucket", (1_000_000, 1024, 1024), "0 0 0", "1024 records fit LDS"),
    ("seq_bucket", (1_000_000, 1025, 1024), "1 7 7813", "1025: 8192 buckets wanted, (999999 >> 7) + 1 = 7813 <= 8192 < 15625"),
    ("seq_bucket", (GRCH38, 1 << 21, 1024), "1 10 3027344", "2^21 records: 2^22 buckets at most, (n - 1 >> 10) + 1"),
    ("seq_bucket", (GRCH38, (1 << 32) - 1, 1024), "1 10 3027344", "2^32 - 1 records"),
    ("seq_bucket", (GRCH38, 1 << 32, 1024), "0 0 0", "2^32 records: record numbers are u32"),
    ("seq_bucket", (5000, 2000, 1024), "1 0 5000", "more buckets wanted (8192) than positions: one position per bucket"),
]

# E = min(15, (32 - min(32, sa_bits)) / 2) for sa_bits = 1 .. 33, by hand
E_OF_SA_BITS = [15, 15, 14, 14, 13, 13, 12, 12, 11, 11, 10, 10, 9, 9, 8, 8, 7, 7, 6, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0]
CAPS = (-1, 0, 2, 15)
for _bits, _e in enumerate(E_OF_SA_BITS, start=1):
    for _cap in CAPS:
        ROWS.append(("ctx_extra", (NT, _bits, _cap), str(_e if _cap < 0 else min(_e, _cap)), "sa_bits = %d, cap %d" % (_bits, _cap)))
ROWS.append(("ctx_extra", (AA, 20, -1), "0", "amino: no extra letters"))
ROWS.append(("ctx_extra", (NT, 32, -1), "0", "GRCh38 (32 bits): E = 0"))
ROWS.append(("ctx_extra", (NT, 28, -1), "2", "chr1 (28 bits): E = 2"))


def line(fn, args):
    return " ".join([fn] + [str(int(a)) for a in args])


def compile_and_run(d, flags):
    src, exe, rows = d / "plan.cpp", d / "plan", d / "rows.txt"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "awry_amd", "csrc"), str(src), "-o", str(exe)] + flags)
    rows.write_text("\n".join(line(r[0], r[1]) for r in ROWS) + "\n")
    return subprocess.run([str(exe), str(rows)], text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    run = compile_and_run(tmp_path_factory.mktemp("accel_plan"), ["-O1"])
    assert run.returncode == 0, (run.returncode, run.stderr)
    out = run.stdout.splitlines()
    assert len(out) == len(ROWS)
    return out


def test_the_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "accel_plan.h"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "awry_amd", "csrc"), str(src)])
    text = open(os.path.join(ROOT, "awry_amd", "csrc", "accel_plan.h")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text and "getenv" not in text
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert [i for i in includes if i.startswith('"')] == ['"layout.h"'], includes


def test_every_row_of_the_table(results):
    assert len(ROWS) > 250
    bad = [(r[0], r[1], r[3], "want " + r[2], "got " + got) for r, got in zip(ROWS, results) if got != r[2]]
    assert not bad, bad


def test_the_table_covers_every_function_and_both_answers():
    src_functions = {ln.split('"')[1] for ln in SRC.splitlines() if "std::strcmp(fn" in ln}
    assert {r[0] for r in ROWS} == src_functions and len(src_functions) == 14
    for fn in ("nblock", "seed_pos", "lcx_wanted", "lcx_possible", "rung_possible", "rung_admitted", "kt_possible", "kt_admitted"):
        assert {r[2] for r in ROWS if r[0] == fn} == {"0", "1"}, fn
    assert {r[2] for r in ROWS if r[0] == "seed_k" and r[1][0] == NT and not r[1][1] and not r[1][4] and r[1][3] < 0} >= {"17", "16", "15", "13", "12"}


def test_e_is_the_reference_s_for_every_width():
    """tests/accel_ref.py states E in Python for the GPU audits: the same number as the table's, for positions of 1 to 33 bits"""
    for bits, e in enumerate(E_OF_SA_BITS, start=1):
        bwt_len = (1 << (bits - 1)) + 1  # the largest position, bwt_len - 1 = 2^(bits - 1), has `bits` bits
        assert ar.sa_bits(bwt_len) == bits
        for cap in CAPS:
            assert ar.expected_ctx_extra(bwt_len, cap) == (e if cap < 0 else min(e, cap)), (bits, cap)


def test_the_table_under_the_sanitizers(tmp_path, results):
    """the same program and rows under -fsanitize=address,undefined: exit status 0 and the same answers"""
    run = compile_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stdout.splitlines() == results
