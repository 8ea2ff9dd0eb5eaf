/*
 * awry_hip.h -- C ABI of libawry_hip.so: the MI355X (gfx950) FM-index search engine that stands in for
 * the query path of the Rust crate AWRY 0.3.1.  Plain pointers and sizes only; no exception crosses.
 *
 * Each entry point names the reference interface it replaces (file:line under /root/reference).  The
 * reference has no FFI of its own -- its boundary is the `pub` surface of `FmIndex` (src/fm_index.rs) --
 * so a Rust shim crate re-creating that surface binds exactly these symbols.
 *
 * There is NO CPU search path in this library: every query entry point runs HIP kernels on the devices
 * selected with awry_set_devices() and fails with AWRY_ERR_NO_DEVICE / AWRY_ERR_HIP otherwise.
 */
#ifndef AWRY_HIP_H
#define AWRY_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (0 = OK, < 0 = error class); awry_last_error() has the message */
enum {
  AWRY_OK = 0,
  AWRY_ERR_IO = -1,            /* file could not be opened / read / written                              */
  AWRY_ERR_FORMAT = -2,        /* not an .awry v1 file, corrupt header, unsupported size                 */
  AWRY_ERR_INVALID_QUERY = -3, /* empty query, '$' / '#', byte >= 0x80: the reference panics or is UB     */
  AWRY_ERR_HIP = -4,           /* a HIP runtime call or kernel failed                                    */
  AWRY_ERR_OOM = -5,
  AWRY_ERR_ARG = -6,           /* null pointer, bad alphabet id, bad device id ...                       */
  AWRY_ERR_NO_DEVICE = -7      /* query issued before awry_set_devices(), or no GPU present              */
};

enum { AWRY_NUCLEOTIDE = 0, AWRY_AMINO = 1 }; /* SymbolAlphabet, src/alphabet.rs:28-31,48-61 */

typedef struct awry_index awry_index_t; /* opaque: host copy of the index + one replica per selected GPU */

/* == LocalizedSequencePosition, src/sequence_index.rs:31-35 */
typedef struct { uint64_t seq_idx, local_pos; } awry_pos_t;

/* == SearchRange, src/search.rs:25-28 (closed interval of BWT rows; empty iff start_ptr > end_ptr) */
typedef struct { uint64_t start_ptr, end_ptr; } awry_range_t;

/* == FmBuildArgs, src/fm_index.rs:78-96 */
typedef struct {
  const char *input_path;  /* input_file_src: FASTA or FASTQ                                              */
  const char *sa_tmp_path; /* suffix_array_output_src: accepted for signature parity, unused (no .sufr)   */
  uint64_t sa_ratio;       /* suffix_array_compression_ratio, 0 => 8 (src/fm_index.rs:122)                */
  uint8_t kmer_len;        /* lookup_table_kmer_len, 0 => 10 nt / 4 aa (src/kmer_lookup_table.rs:23-24)   */
  uint8_t alphabet;        /* AWRY_NUCLEOTIDE / AWRY_AMINO                                                */
  uint64_t max_query_len;  /* accepted for signature parity; the full suffix array is always built        */
  uint8_t remove_tmp;      /* remove_intermediate_suffix_array_file: no intermediate file exists          */
} awry_build_args_t;

/* ---- construction / persistence ------------------------------------------------------------------ */
/* FmIndex::new, src/fm_index.rs:142-268 */
int awry_build(const awry_build_args_t *args, awry_index_t **out);
/* same, from an in-memory text that follows the reference's text model (records joined by 'N'/'X', one
 * trailing '$', src/fm_index.rs:148-153,220-223); seq_starts/headers describe the records */
int awry_build_from_text(const uint8_t *text, uint64_t bwt_len, int alphabet, uint64_t sa_ratio, uint8_t kmer_len,
                         const uint64_t *seq_starts, const char *const *headers, uint64_t nseq, awry_index_t **out);
/* same with an explicit choice of where the suffix array and the BWT are constructed: a device id >= 0
 * (GPU prefix doubling + streaming pack kernels), AWRY_BUILD_HOST (host SA-IS) or AWRY_BUILD_AUTO (what
 * awry_build / awry_build_from_text use: the calling thread's current GPU if one is visible and bwt_len >= 2^20, else host; env AWRY_BUILD=host|gpu
 * overrides; when the GPU chosen this way cannot do it -- its HBM taken by replicas, say -- the host builder takes over, while
 * an explicit device id fails with AWRY_ERR_HIP).  All choices produce bit-identical indexes. */
enum { AWRY_BUILD_HOST = -1, AWRY_BUILD_AUTO = -2 };
int awry_build_from_text_on(const uint8_t *text, uint64_t bwt_len, int alphabet, uint64_t sa_ratio, uint8_t kmer_len,
                            const uint64_t *seq_starts, const char *const *headers, uint64_t nseq, int build_device,
                            awry_index_t **out);
/* FmIndex::load / FmIndex::save, src/fm_index_file.rs:132,42 (.awry v1, byte-compatible) */
int awry_load(const char *path, awry_index_t **out);
int awry_save(awry_index_t *idx, const char *path); /* needs no device (the k-mer table is filled on a replica's GPU when there is one, else on the host) */
void awry_free(awry_index_t *idx);

/* ---- device placement (replaces rayon's global pool, src/fm_index.rs:455-487) ---------------------- */
/* replicate the index into the HBM of each listed device and build its seed table; batches are then
 * sharded contiguously over the replicas.  n_devices == 0 is an error: there is no CPU backend.  Replaces (and first
 * releases) any earlier replicas.  HBM use: the default policies size the seed table to 70 % of the free HBM and keep
 * the locate / verify accelerators (7 B per text symbol) when they fit in half of it -- ~160 GB for a GRCh38-scale
 * index; AWRY_HBM_BUDGET_GB caps the figure they plan with, AWRY_SEED_K / AWRY_VERIFY=0 pin the choices.  Later, the first
 * batch of >= 4096 nucleotide k-mers of a length L below the seed table's k adds a complete 4^L table for that length
 * (8 B x 4^L: 134 MB for L = 12, 34 GB for L = 16) when it fits half of the free HBM and all such tables of the replica stay
 * below AWRY_SEED_RUNG_GB (default 48); that first call builds the table (1.3 s for L = 16) while it holds the replica's
 * lane; AWRY_SEED_RUNGS=0 turns the feature off.
 * If building a replica fails (out of HBM on one of several GPUs, say) the index is left with NO replicas -- the old ones are
 * released first, because the policies size their tables from the HBM that is free -- and every query returns
 * AWRY_ERR_NO_DEVICE until a later awry_set_devices succeeds; do not call it while another thread is inside a batch call. */
int awry_set_devices(awry_index_t *idx, const int *device_ids, int n_devices);
/* device-side seed-table length (performance knob only; results do not depend on it).  0 disables,
 * -1 picks the default.  Takes effect immediately on all replicas. */
int awry_set_seed_kmer_len(awry_index_t *idx, int k);
int awry_seed_kmer_len(const awry_index_t *idx);
/* A/B switch for the packed-k-mer count kernel (process-wide; -1 policy, 0 strided quads, 1 LDS-staged chunks,
 * 2 groups of four queries per quad, 3 two-phase probe + resume).  All variants return identical counts. */
int awry_debug_set_count_kernel(int mode);
/* Indexes of 2^32 rows or more take "wide-row" packed kernels (64-bit rows, 16-byte seed entries, no 32-bit accelerators;
 * the reference is u64 throughout, src/search.rs:7).  on != 0 makes replicas placed AFTERWARDS (awry_set_devices) take
 * those kernels whatever the index size -- for tests: a real index of that size takes an hour of host SA-IS to build. */
int awry_debug_force_wide_rows(int on);
/* An upper bound on the block count of a launch (process-wide, read at every launch; 0, the default: none; negative:
 * AWRY_ERR_ARG).  For tests: on a grid of one block the lanes of the stride-loop kernels take item after item at batches of a
 * few hundred items.  Bounded: the grids that grid_for and resident_grid size (the read pipelines, the generic count kernel, the
 * mismatch and class-pattern search, the locate walk passes, index construction) and the tile grid of locate.  Not bounded:
 * grids that are a function of the data (the prefix scans) and the grids the k-mer count schedules, the amino two-phase
 * schedule, the list passes of the generic count kernel and the stream copy size themselves from the CU count or an occupancy
 * query.  Results do not depend on it. */
int awry_debug_set_max_blocks(int blocks);
int awry_debug_max_blocks(void);
/* device pointer of replica `slot`'s dense SA (u32 SA[j * ratio]) or NULL -- for tests that dump it */
const void *awry_debug_dense_sa(const awry_index_t *idx, int slot);
/* The device-only accelerators of replica `slot`, for tests that audit them against the text.  Every pointer is read-only
 * device memory (NULL: the structure is not resident) and stays valid until the next call that rebuilds accelerators
 * (awry_set_devices, awry_set_seed_kmer_len, awry_set_verify, awry_set_locate_sa_ratio, awry_set_lcx); copy out with
 * awry_dev_memcpy_d2h.
 *   seed: sigma^seed_k entries of seed_entry_bytes bytes (8: u32 sp, u32 cnt; 16, wide rows: u64 sp, u64 cnt; sigma = 4
 *         nucleotide, 21 amino); seed_pos != 0: singleton entries hold text positions, with 14 + ctx_extra context letters
 *   dense_sa: u32 SA[j * dense_ratio], j < ceil(bwt_len / dense_ratio)
 *   text4: text4_words u32 of eight 4-bit codes (A0 C1 G2 T3, else 8), zero past the text;  text8: bwt_len symbol indices
 *   sa_nblock: u32 SA of the rows [nblock_lo, nblock_hi), those whose suffix starts with N
 *   lcx_inner: lcx_inner_words u64, the sampled levels of the left-context index, level t = 1..7 at word lcx_off[t] */
typedef struct {
  const void *seed;
  int32_t seed_k, seed_entry_bytes, seed_pos, ctx_extra;
  const void *dense_sa;
  uint64_t dense_ratio;
  const void *text4;
  uint64_t text4_words;
  const void *text8;
  const void *sa_nblock;
  uint64_t nblock_lo, nblock_hi;
  const void *lcx_inner;
  uint64_t lcx_inner_words;
  uint32_t lcx_off[8];
} awry_debug_accel_t;
int awry_debug_accelerators(const awry_index_t *idx, int slot, awry_debug_accel_t *out);
/* device pointer of replica `slot`'s table for nucleotide k-mers of L < seed k letters (4^L entries of 8 bytes, rows, the BWT
 * symbol of singletons), built if it is not resident; NULL where a launch would get none (length outside the rungs' range,
 * wide rows, amino, no room, AWRY_SEED_RUNGS=0).  Valid as long as the replica. */
const void *awry_debug_seed_rung(awry_index_t *idx, int slot, int L);
/* An upper bound on E, the context letters a position seed keeps beyond 14 (process-wide; -1, the default: none; below -1:
 * AWRY_ERR_ARG).  Seed tables converted to position seeds AFTERWARDS keep min(E, cap) extra letters.  For tests: E is
 * min(15, (32 - sa bits) / 2), so that a text of test size never has the E = 0 of a GRCh38-scale index or the E = 2 of a
 * chr1-scale one.  Results do not depend on it. */
int awry_debug_set_ctx_extra_cap(int cap);
/* name(s) of the kernel(s) awry_dev_count_nt2 launches for k-mers of length L on replica 0 (for profiling reports) */
const char *awry_count_schedule(const awry_index_t *idx, int L);
/* device-side SA sampling used by locate (performance knob only; locations do not depend on it): 0 = walk to the
 * file's row samples (suffix_array_compression_ratio, default), r >= 1 = additionally keep SA[j r] as u32 in HBM
 * (r = 1: one read per hit, no LF walk; GRCh38: 12.4 GB).  Needs bwt_len < 2^32. */
int awry_set_locate_sa_ratio(awry_index_t *idx, int ratio);
int awry_locate_sa_ratio(const awry_index_t *idx);
/* seed-and-verify for packed nucleotide reads (performance knob only; counts and locations do not depend on it):
 * keeps the ratio-1 dense SA and the text as 4-bit codes in HBM (GRCh38: 12.4 + 1.55 GB), both recovered from the
 * index on the device.  Once a range holds a single row -- or <= 8 rows after `after_steps` LF steps -- the rest of the
 * query is compared with the text in front of each candidate instead of being matched by one dependent LF step per
 * symbol.  after_steps = -1 switches it off.  Default policy (awry_set_devices): on with after_steps = 2 for nucleotide
 * indexes with bwt_len < 2^32 whose accelerators fit in half of the free HBM; env AWRY_VERIFY=0 disables, =N sets
 * after_steps.  Used by the read kernels (awry_dev_count_nt2_long, the host paths) and by the two-phase k-mer schedule;
 * the single-kernel k-mer schedule (dense seed tables) uses it only after awry_set_verify_kmers(idx, 1), because there
 * the extra state costs random batches ~15 %. */
int awry_set_verify(awry_index_t *idx, int after_steps);
int awry_set_verify_kmers(awry_index_t *idx, int on);
int awry_verify_enabled(const awry_index_t *idx);
/* left-context index (performance knob only; counts and locations do not depend on it): with the seed-and-verify accelerators
 * resident, every seed bucket of 2+ rows keeps the 32 letters in FRONT of each of its suffixes, sorted, plus each suffix's text
 * position and BWT row (16.6 B per row of the index: 51 GB for GRCh38).  The letters a query has left of its seed window are
 * then matched by a 16-ary search over its bucket -- log16(rows) random lines -- instead of one LF step (two lines) per letter:
 * what makes k-mers and reads from repeat families (10^3..10^5 rows per seed, dozens of letters before the rows part) cost a
 * few lines like any other query.  Default policy (awry_set_devices): built when it and its build scratch fit 3/4 of the HBM
 * still free once everything else is resident; env AWRY_LCX=0 / on = 0 switch it off (rebuilds the seed table), on = 1
 * restores the policy.  awry_lcx_enabled: is it resident on replica 0. */
int awry_set_lcx(awry_index_t *idx, int on);
int awry_lcx_enabled(const awry_index_t *idx);
/* device pointers of replica `slot`'s left-context index for tests that dump it: keys[bwt_len] (u64) and
 * rowpos[bwt_len] (u64: text position | BWT row << 32); NULL when it is not resident */
int awry_debug_lcx(const awry_index_t *idx, int slot, const void **d_keys, const void **d_rowpos);
/* k-mer count table (performance knob only; counts do not depend on it): with the left-context index resident, a replica keeps,
 * for ONE k-mer length L (seed k < L <= 32) at a time, every distinct L-mer of every seed bucket of more than 4 rows with its
 * count, in a hash table of 128-B lines (16 entries of 8 B; about 8 keys per line; for small texts at least 2^(2L - 43)
 * lines).  Like the tables of k-mers shorter than the seed k, it is built on first use -- on the replica's own stream, from the
 * left-context index, within half of the HBM then free; a length it does not fit is remembered and searched as before -- and
 * a k-mer of a repeat family then costs one random line instead of a search of 4..6 dependent ones.  Entries whose count does
 * not fit and lines that took more than 16 keys send their queries to the search.
 * mode -1 (default): built by the first awry_dev_count_nt2 launch (or host batch chunk) of a length with 65536 queries or more
 * and no awry_debug_set_count_kernel / AWRY_COUNT_KERNEL override, and used by such launches; a large batch of another length
 * replaces it.  mode 0: off (drops it).  mode 1: built for the length of the next launch, whatever its size, and used by every
 * launch of that length.  env AWRY_KMER_TABLE=0 disables.  Whatever drops or rebuilds the left-context index or the seed table
 * (awry_set_lcx, awry_set_verify, awry_set_locate_sa_ratio, awry_set_seed_kmer_len, awry_set_devices) drops the table; the
 * warm-up batch of awry_set_devices builds none.  The reads (L > 32) and amino paths do not use it. */
int awry_set_kmer_table(awry_index_t *idx, int mode);
/* the table resident on replica `slot`: info[0] its length L (0: none), [1] distinct L-mers kept, [2] 128-B lines, [3] lines that
 * could not take all their keys, [4] bytes, [5] wall time of its construction in microseconds */
int awry_kmer_table_info(awry_index_t *idx, int slot, uint64_t *info);
/* lines of k-mer count tables built afterwards (process-wide; rounded down to a power of two; 0, the default: the policy).
 * For tests: a table far too small overflows in most lines.  Results do not depend on it. */
int awry_debug_set_kmer_table_lines(uint64_t lines);
/* the k-mer count table resident on replica `slot`, for tests that audit it: *L_out its length and *bits_out the log2 of its
 * number of lines (both 0: none resident).  With host_out non-null and capacity_words >= 16 << *bits_out, the table's
 * 16 << bits words (entry: tag << 21 | overflow << 20 | count, 16 entries per line) are copied to host_out.  A copy, not a
 * device pointer: any launch of another length may free the table, so it is read under the lock that keeps it resident. */
int awry_debug_kmer_table(awry_index_t *idx, int slot, uint64_t *host_out, uint64_t capacity_words, int *L_out, uint32_t *bits_out);
int awry_num_devices(const awry_index_t *idx);

/* ---- batch queries --------------------------------------------------------------------------------- */
/* FmIndex::parallel_count, src/fm_index.rs:455-460.  Query i = qbytes[qoff[i] .. qoff[i+1]); results in
 * input order in caller-owned counts_out[n].  Any undefined query => AWRY_ERR_INVALID_QUERY. */
int awry_count_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint64_t *counts_out);
/* no counterpart in the reference: the same for callers that already hold their k-mers packed (k-mer counters do) --
 * n k-mers of L <= 32 letters, letter j (0 = leftmost) of k-mer i in bits [2j, 2j + 2) of words[i], A0 C1 G2 T3;
 * nucleotide indexes of any size (2^32 rows or more: the wide-row kernels).  16 B per query cross PCIe instead of L + 8. */
int awry_count_packed_kmers(awry_index_t *idx, const uint64_t *words, uint64_t n, int L, uint64_t *counts_out);
/* FmIndex::parallel_locate, src/fm_index.rs:479-487.  CSR output, library-allocated (awry_free_buffer):
 * hits of query i are [hit_off[i], hit_off[i+1]) in ascending BWT-row order (src/fm_index.rs:521);
 * global_pos (nullable) receives (SA sample + steps) % bwt_len (src/fm_index.rs:534).  hits_out is nullable too: a
 * caller that wants text positions only (8 B per hit over PCIe instead of 24) passes NULL and (record, offset) pairs
 * are neither computed nor moved; with both NULL the call returns the offsets alone. */
int awry_locate_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n,
                      uint64_t **hit_off_out, awry_pos_t **hits_out, uint64_t **global_pos_out);
/* ---- substitution-tolerant search (Hamming distance, no counterpart in the reference) --------------------
 * Query i and the index text are compared as symbol indices, exactly as the exact path maps them: letters are
 * case-insensitive, U is T, any other byte is N (nucleotide) / X (amino).  The distance of text position p is the number
 * of positions j < L with text[p + j] != query[j]; p is an occurrence with <= k mismatches when its window
 * text[p .. p + L) holds no '$' and its distance is <= k.  Substitutions range over every non-sentinel symbol of the
 * alphabet (nucleotide A C G N T: 4 alternatives per position; amino the 21 symbols, X included: 20), so query N matches
 * text N as on the exact path, and k = 0 gives exactly awry_count_batch / awry_locate_batch.  k >= L is legal: every
 * window without '$' then matches.  max_mismatches outside 0..AWRY_MAX_MISMATCHES => AWRY_ERR_ARG; queries are rejected
 * as in awry_count_batch (empty, '$' / '#', byte >= 0x80 => AWRY_ERR_INVALID_QUERY); no replica => AWRY_ERR_NO_DEVICE.
 * Distinct substitution patterns spell distinct strings, so their row ranges are disjoint: counts are sums of ranges and
 * ascending BWT-row order is well defined. */
enum { AWRY_MAX_MISMATCHES = 2 };
/* no counterpart in the reference.  counts_out[n * (k + 1)]: row i holds the occurrences of query i at exactly
 * 0, 1, .., k substitutions (Hamming distance over symbol indices; windows holding '$' never match) */
int awry_count_mismatch_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n,
                              int max_mismatches, uint64_t *counts_out);
/* CSR like awry_locate_batch: hits of query i are [hit_off[i], hit_off[i+1]) in ascending BWT-row order, the
 * same order awry_locate_batch uses; mismatches_out (nullable) receives each hit's distance.  Each result array is
 * nullable as in awry_locate_batch; all are released with awry_free_buffer.  A chunk of queries whose occurring variants
 * exceed the device leaf capacity (2^26 row ranges; env AWRY_MISMATCH_LEAF_CAP, read per call) is split and redone. */
int awry_locate_mismatch_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n,
                               int max_mismatches, uint64_t **hit_off_out, awry_pos_t **hits_out,
                               uint64_t **global_pos_out, uint8_t **mismatches_out);

/* ---- class patterns: IUPAC / residue-class search with up to k mismatches (no counterpart in the reference) ----
 * A pattern is a string of class letters, case-insensitive, each a set of symbol indices (the indices of the alphabet):
 *   nucleotide  A C G T are themselves, U = T; R={A,G} Y={C,T} S={C,G} W={A,T} K={G,T} M={A,C} B={C,G,T} D={A,G,T}
 *               H={A,C,T} V={A,C,G}; N={A,C,G,T}.  No class holds the text's ambiguity symbol (index 4, the N that also joins
 *               records).
 *   amino       the 20 standard residues are themselves; B={D,N} Z={E,Q} J={I,L}; X = the 20 standard residues.  No class
 *               holds the text's X (index 20).
 * Any other byte is rejected.  A class of more than one symbol is a class position.
 * For a pattern of L positions with classes S_0 .. S_{L-1} the distance of text position p is the number of j with
 * text[p + j] not in S_j; p is an occurrence with <= k mismatches when text[p .. p + L) holds no '$' and its distance is <= k.
 * A mismatching text symbol may be any non-sentinel symbol outside the class, the ambiguity symbol included (the rule of
 * awry_count_mismatch_batch): at k = 0 no hit spans a record join or a text N / X, at k >= 1 one may, at one mismatch per
 * such symbol.  max_mismatches is 0..AWRY_MAX_MISMATCHES, else AWRY_ERR_ARG.  For a pattern of unambiguous letters only,
 * counts, hits, order and distances are exactly those of the mismatch entry points at the same k, and at k = 0 exactly those
 * of awry_count_batch / awry_locate_batch.  (Those paths keep mapping a query N / X to the text's ambiguity symbol.)
 * Order: distinct matched strings have disjoint row ranges; the hits of one pattern are in ascending BWT-row order, that is
 * the matched strings in lexicographic order of symbol indices and within a string the order of awry_locate_batch.
 * Limits: at most AWRY_MAX_CLASS_POSITIONS class positions per pattern (the search then holds at most min(L - 1, class
 * positions + k) <= AWRY_PATTERN_MAX_FRAMES stack frames), and at most AWRY_PATTERN_DEFAULT_MAX_EXPANSIONS expansions (one
 * expansion = the Occ of every symbol at the two rows of one node) per pattern; env AWRY_PATTERN_MAX_EXPANSIONS, read per
 * call, replaces the latter.  A pattern whose search needs more is abandoned, not run to the end: the default, 2^19, is what one
 * lane of a fully occupied MI355X works through in about 2 s on a 3.1 Gbp text (DESIGN.md 5d has the measurement), so that no
 * pattern keeps a launch busy for longer on a shared card.  This is the one case in which a plain-letter pattern and the
 * mismatch entry points differ: those have no cap.
 * Rejected, as on the other paths: an empty pattern, '$' / '#', a byte >= 0x80; and: a byte that is no class letter, more than
 * AWRY_MAX_CLASS_POSITIONS class positions, the expansion cap exceeded.  Host batch calls then fail the whole batch with
 * AWRY_ERR_INVALID_QUERY (the message names the query index and the reason) and leave the out-pointers untouched; device calls
 * write the status byte (AWRY_Q_*) and zero counts. */
enum { AWRY_MAX_CLASS_POSITIONS = 16, AWRY_PATTERN_MAX_FRAMES = 18, AWRY_PATTERN_DEFAULT_MAX_EXPANSIONS = 1 << 19 };
/* status byte of the device-resident query calls (d_status) */
enum {
  AWRY_Q_OK = 0, AWRY_Q_EMPTY = 1, AWRY_Q_SENTINEL = 2, AWRY_Q_NON_ASCII = 3,
  AWRY_Q_NOT_CLASS_LETTER = 4, AWRY_Q_CLASS_POSITIONS = 5, AWRY_Q_EXPANSION_CAP = 6 /* patterns only */,
  AWRY_Q_CANDIDATE_CAP = 7 /* awry_locate_edit_batch only: the query was abandoned, not rejected */,
  AWRY_Q_SEED_CAP = 8 /* awry_chain_batch / awry_dev_chain_seeds only: more seeds than max_seeds; abandoned, not rejected */
};
/* class mask of an ASCII byte as a pattern letter: bit s = symbol index s belongs to the class, 0 = not a class letter (or
 * an unknown alphabet id).  The one table of host and device; needs no GPU. */
uint32_t awry_pattern_class(int alphabet, uint8_t ascii);
/* counts_out[n * (k + 1)]: row i holds the occurrences of pattern i at exactly 0, 1, .., k mismatches */
int awry_count_pattern_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n,
                             int max_mismatches, uint64_t *counts_out);
/* arrays as awry_locate_mismatch_batch takes and returns them, nullable likewise; the leaf capacity and its env var
 * (AWRY_MISMATCH_LEAF_CAP) are shared with it */
int awry_locate_pattern_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n,
                              int max_mismatches, uint64_t **hit_off_out, awry_pos_t **hits_out,
                              uint64_t **global_pos_out, uint8_t **mismatches_out);

/* ---- anchors: greedy longest-match factorisation of a query (no counterpart in the reference) ---------------
 * What a mapper does with a read that does not occur as a whole: cut it into maximal exact matches and chain those.
 * Queries are mapped to symbol indices exactly as on the exact path (letters case-insensitive, U = T, any other byte N /
 * X; query N matches text N) and rejected as there (empty, '$' / '#', byte >= 0x80).  For a query q of L letters, with
 * occurs(b, e) = "q[b..e) has at least one occurrence (awry_count > 0)", min_len >= 1 and skip in {0, 1}:
 *     e = L
 *     while e > 0:
 *         if not occurs(e-1, e):        # the letter itself is absent from the text
 *             e -= 1; continue
 *         b = smallest b' such that occurs(b', e)     # backward search until the range would become empty
 *         if e - b >= min_len: report anchor (q_begin = b, q_len = e - b, start_row, count) = row range of q[b..e)
 *         if b == 0: stop
 *         e = b - skip                  # skip = 0: the letter that failed ends the next anchor; 1: it is left out
 * Anchors of one query are reported in the order found: right to left, descending q_begin.  Anchors shorter than min_len
 * are not reported but still consume their letters.  A query that occurs as a whole yields exactly one anchor, q_begin =
 * 0, q_len = L, whose rows are what awry_search_range returns for it.  start_row / count are rows of the BWT (awry_range_t:
 * start_ptr = start_row, end_ptr = start_row + count - 1); no accelerator changes them (the seed table only lets an anchor
 * start seed_k letters in).  min_len == 0 or skip outside 0..1 => AWRY_ERR_ARG; a rejected query fails the whole batch
 * with AWRY_ERR_INVALID_QUERY and leaves the out-pointers untouched; no replica => AWRY_ERR_NO_DEVICE; a query of 2^32
 * letters or more => AWRY_ERR_ARG. */
typedef struct { uint32_t q_begin, q_len; uint64_t start_row, count; } awry_anchor_t;
/* CSR output, library-allocated (awry_free_buffer): anchors of query i are anchors[anchor_off[i] .. anchor_off[i+1]) */
int awry_anchor_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len, int skip,
                      uint64_t **anchor_off_out, awry_anchor_t **anchors_out);
/* the same, and every anchor located: hits of anchor s (index into anchors) are [hit_off[s], hit_off[s+1]) in ascending
 * BWT-row order -- exactly what awry_locate_batch returns for that substring; hit_off has anchor_off[n] + 1 entries.  An
 * anchor with count > max_hits keeps its record and gets no hits; max_hits == 0 => AWRY_ERR_ARG (a cap is mandatory: a
 * one-letter anchor has a quarter of the text as hits).  hits_out / global_pos_out are nullable as in awry_locate_batch.  A
 * chunk of queries whose located hits exceed the device hit capacity (2^26; env AWRY_ANCHOR_HIT_CAP, read per call) and
 * which holds more than one query is split and redone. */
int awry_locate_anchors_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                              int skip, uint64_t max_hits, uint64_t **anchor_off_out, awry_anchor_t **anchors_out,
                              uint64_t **hit_off_out, awry_pos_t **hits_out, uint64_t **global_pos_out);

/* ---- SMEMs: all super-maximal exact matches of a query (no counterpart in the reference) ---------------------
 * The seeds of an FM-index read mapper: the substrings of the query that occur in the text and cannot be extended by one
 * letter on either side and still occur.  Queries are mapped to symbol indices and rejected exactly as for
 * awry_anchor_batch.  With occurs(b, e) = "q[b..e) has at least one occurrence (awry_count > 0)", an SMEM of a query q of L
 * letters is a pair (b, e), 0 <= b < e <= L, such that
 *     occurs(b, e)   and   (b == 0 or not occurs(b-1, e))   and   (e == L or not occurs(b, e+1))
 * Because occurs is about the whole text, this is the same as "a match contained in no other match of the query": the set
 * does not depend on any order of search.  Begins and ends are both strictly monotone over the set, so a query has at
 * most L SMEMs.  Each is reported as an awry_anchor_t: q_begin = b, q_len = e - b, and start_row / count = the row interval of
 * q[b..e), as awry_search_range gives it.  The SMEMs of one query are reported in descending q_begin (so also descending
 * end); only those with q_len >= min_len are reported.  A query that occurs as a whole yields exactly one record, (0, L); a
 * letter absent from the text belongs to no SMEM.  (Anchors, above, are left-maximal but mostly not right-maximal, and a
 * longer match that overlaps two anchors is not among them; the first SMEM of a query equals its first skip = 0 anchor.)
 * No accelerator, table length, row width or replica count changes any output.  min_len == 0 => AWRY_ERR_ARG; a rejected
 * query fails the whole batch with AWRY_ERR_INVALID_QUERY and leaves the out-pointers untouched; no replica =>
 * AWRY_ERR_NO_DEVICE; a query of 2^32 letters or more => AWRY_ERR_ARG.
 * CSR output, library-allocated (awry_free_buffer): SMEMs of query i are smems[smem_off[i] .. smem_off[i+1]) */
int awry_smem_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                    uint64_t **smem_off_out, awry_anchor_t **smems_out);
/* the same, and every SMEM located, with the semantics of awry_locate_anchors_batch: hits of record s are [hit_off[s],
 * hit_off[s+1]) in ascending BWT-row order; a record with count > max_hits keeps its place and gets no hits; max_hits == 0
 * => AWRY_ERR_ARG; hits_out / global_pos_out nullable; the device hit capacity (AWRY_ANCHOR_HIT_CAP) is the anchors' */
int awry_locate_smems_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                            uint64_t max_hits, uint64_t **smem_off_out, awry_anchor_t **smems_out, uint64_t **hit_off_out,
                            awry_pos_t **hits_out, uint64_t **global_pos_out);

/* ---- locate within k edits: pigeonhole seeds and a bit-vector verify (no counterpart in the reference) --------
 * Where a read matches the text with at most k substitutions, insertions and deletions, and at what distance.
 * Text model: queries are mapped to symbol indices and rejected exactly as on the exact path -- letters case-insensitive,
 * U = T, any other byte N / X, query N equals text N; empty queries, '$' / '#' and bytes >= 0x80 are rejected.
 * Let T be the text without its final '$', n = bwt_len - 1 symbols; q a query of L symbols, 1 <= L <= AWRY_EDIT_MAX_LEN;
 * k = max_edits, 0 <= k <= AWRY_MAX_EDITS and k < L.
 *     D(s) = min over e in [s, n] of  edit_distance(q, T[s..e))      for 0 <= s < n      (unit costs; D(-1) = D(n) = +inf)
 *     s is a hit with distance D(s)  iff  D(s) <= k  and  D(s-1) >= D(s)  and  D(s+1) >= D(s)
 * A hit is a START position whose best alignment is within k edits and is not beaten by either neighbouring start: a local
 * minimum; plateaus are reported whole.  So at k = 0 the hits of a query are exactly the positions awry_locate_batch returns
 * for it; an exact occurrence at s under k = 3 is reported once, not seven times; a record join or a text N costs one edit
 * unless the query has N there (the rule of the mismatch path).  Hits of one query are in ascending text position.
 * Piece rule (part of the contract: the cap depends on it): piece t of a query is q[floor(t L / (k+1)) .. floor((t+1) L /
 * (k+1))), t = 0..k; c(q) is the sum of the exact occurrence counts of its k + 1 pieces.  If c(q) > max_candidates the query
 * is abandoned: status byte AWRY_Q_CANDIDATE_CAP, no hits.  An abandoned query does not fail the batch (reads from a
 * 10^5-copy family are ordinary input).  max_candidates == 0 => AWRY_ERR_ARG: a cap is mandatory, as max_hits is for anchors.
 * Malformed queries fail the whole batch with AWRY_ERR_INVALID_QUERY and leave the out-pointers untouched: the reasons of the
 * exact path, and L > AWRY_EDIT_MAX_LEN, and L <= k.  max_edits outside 0..AWRY_MAX_EDITS => AWRY_ERR_ARG; no replica =>
 * AWRY_ERR_NO_DEVICE; an index with bwt_len >= 2^32 or a wide-row replica => AWRY_ERR_ARG; no HBM for the text copy (below)
 * => AWRY_ERR_OOM.  No accelerator, table length, replica count or chunk capacity changes any output; c(q) is a sum of exact
 * counts, so it does not either.  The scan reads the text as symbol indices: the verify accelerators' copy while it is
 * resident, else a copy of its own (1 B per symbol) that the replica recovers from the index on first use and keeps until
 * the replicas are replaced; nothing else of the replica changes.  A chunk of queries with more candidates than the device
 * capacity (2^26; env AWRY_EDIT_CANDIDATE_CAP, read per call) and more than one query is split and redone.
 * CSR output, library-allocated (awry_free_buffer): hits of query i are [hit_off[i], hit_off[i+1]) of hits (record, offset),
 * global_pos (text position), edits (distance); status[n] is AWRY_Q_OK or AWRY_Q_CANDIDATE_CAP.  All but hit_off_out nullable. */
enum { AWRY_MAX_EDITS = 8, AWRY_EDIT_MAX_LEN = 256 };
int awry_locate_edit_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, int max_edits,
                           uint64_t max_candidates, uint64_t **hit_off_out, awry_pos_t **hits_out, uint64_t **global_pos_out,
                           uint8_t **edits_out, uint8_t **status_out);

/* ---- align the hits of locate within k edits: text span and CIGAR per hit (no counterpart in the reference) ----
 * What a mapping needs beyond a start and a distance: where the match ends in the text, and which letters were substituted,
 * inserted or deleted.  T, n, q, L, k, D(s), the hit rule, the piece rule and the candidate cap are those of
 * awry_locate_edit_batch.  For a hit (q, s, d), d = D(s):
 *     C[i][j] = edit_distance(q[0..i), T[s..s+j))    0 <= i <= L, 0 <= j <= J = min(L + d, n - s)   (unit costs, symbol indices compared)
 *     text_len = the smallest j with C[L][j] == d                                 (the match is T[s .. s + text_len))
 *     traceback from (i, j) = (L, text_len) to (0, 0); at each cell take the first of these that holds:
 *         1. i > 0 and j > 0 and C[i-1][j-1] + (q[i-1] != T[s+j-1]) == C[i][j]  ->  '=' if the symbols are equal, else 'X';  i--, j--
 *         2. i > 0 and C[i-1][j] + 1 == C[i][j]                                 ->  'I' (a query letter with no text letter); i--
 *         3. otherwise (j > 0 and C[i][j-1] + 1 == C[i][j])                     ->  'D' (a text letter with no query letter); j--
 *     the operations, reversed into query order and run-length encoded, are the hit's CIGAR.
 * Properties (proven below, and tested against the full table):
 *   Banded table.  The table restricted to the band |i - j| <= d, cells outside it +infinity, gives the same text_len and the
 *     same script: an optimal path to a cell whose true value is v <= d holds at most v insertions and deletions, so it never
 *     leaves the band; hence a banded value <= d is exact (banded values are never below the true ones), and the equality tests
 *     of the traceback -- each with a cell of the path, value <= d, on its right side -- come out the same.  2d + 1 <= 17
 *     cells per row suffice.
 *   No 'D' at either end.  A script never begins with 'D': dropping the leading text letter would align q at s + 1 with d - 1
 *     edits, and s is a local minimum of D.  It never ends with 'D': dropping the last text letter would give C[L][text_len - 1]
 *     = d - 1 < d = D(s).
 *   Bounds.  The operations other than '=' number exactly d; |text_len - L| <= d; d operations separate at most d + 1 runs of
 *     '=', so a script has at most 2d + 1 runs: AWRY_ALIGN_MAX_OPS = 2 AWRY_MAX_EDITS + 1 = 17 is a hard bound.
 *   Where gaps fall.  Preferring the diagonal while walking from the end puts gaps as far left as the optimum allows (the
 *     usual left-normalised form): in "AC" x 10 with one unit deleted the gap is at the array's left end.
 * Encoding: one uint32_t per run, len << 4 | op, with BAM's op codes I = 1, D = 2, '=' = 7, X = 8; M is never produced.
 * awry_align_edit_batch: hit_off, hits, global_pos, edits and status are exactly what awry_locate_edit_batch returns for the same
 * arguments -- errors, the candidate cap, chunk splitting by AWRY_EDIT_CANDIDATE_CAP and sharding over replicas included; an
 * abandoned query has no hits and no runs.  text_len[h] is hit h's span; its runs are cigar[cigar_off[h] .. cigar_off[h+1]),
 * cigar_off has hit_off[n] + 1 entries.  All but hit_off_out nullable; cigar_off_out and cigar_out are given or omitted
 * together (one without the other => AWRY_ERR_ARG).  Arrays are pinned (awry_free_buffer).  The script is computed on the
 * device from the resident text copy, in sub-batches of 2^20 hits (env AWRY_ALIGN_SUB_BATCH, read per call), which bounds the
 * device staging at 89 B x the sub-batch whatever the hit count. */
enum { AWRY_ALIGN_MAX_OPS = 17 };
int awry_align_edit_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, int max_edits,
                          uint64_t max_candidates, uint64_t **hit_off_out, awry_pos_t **hits_out, uint64_t **global_pos_out,
                          uint8_t **edits_out, uint8_t **status_out, uint32_t **text_len_out, uint64_t **cigar_off_out,
                          uint32_t **cigar_out);

/* ---- colinear chaining of the located SMEM seeds of a query (no counterpart in the reference) -------------------
 * What a mapper puts between seeding and verification: seeds that lie in the same order, on nearly the same diagonal, in read
 * and text are grouped into chains, each chain gets a score, and the best chain is where the read belongs.  Everything is
 * integer and every tie is broken explicitly.
 * Seeds.  A seed is an awry_seed_t: q[q_begin .. q_begin + q_len) matches the text at t_pos.  The seeds of a query are the records
 *   of awry_locate_smems_batch(min_len, max_hits): every record with count <= max_hits gives one seed per hit (t_pos = that
 *   hit's global_pos); a record over max_hits gives none (repeat masking, exactly as locate treats it).  rec(seed) is the record
 *   index awry_get_seq_location(t_pos) returns.  With N the number of seeds of the query: N > max_seeds abandons the query --
 *   status byte AWRY_Q_SEED_CAP, no chains -- and does not fail the batch (the rule of AWRY_Q_CANDIDATE_CAP).
 * Order.  The seeds of a query are sorted ascending by (t_pos, q_begin, q_len, input index) and numbered 0 .. N-1.  SMEM begins
 *   are strictly monotone, so seeds that come from SMEMs never tie on the first two keys; the last two exist for the seeds a
 *   caller supplies (awry_dev_chain_seeds), which may.
 * Score.  Parameters lookback (1 .. AWRY_CHAIN_MAX_LOOKBACK), max_gap >= 1, max_skew >= 0.  For j < i with i - j <= lookback let
 *   dq = q_begin_i - q_begin_j, dt = t_pos_i - t_pos_j, g = |dq - dt|.  j may precede i iff rec_j == rec_i and 0 < dq <= max_gap
 *   and 0 < dt <= max_gap and g <= max_skew.  Then
 *       gain(j, i) = min(q_len_i, dq, dt) - g                                         (may be negative)
 *       f_i = max( q_len_i , max over admissible j of f_j + gain(j, i) )
 *       p_i = the admissible j with f_j + gain(j, i) == f_i, if f_i > q_len_i; among several the LARGEST j; else none
 *   Consequence: gain(j, i) <= dq, so along the predecessors of i back to the seed c that has none, f_i <= q_len_c + (q_begin_i -
 *   q_begin_c) <= q_begin_i + q_len_c; with seeds of one length (k-mers) that is f_i <= q_begin_i + q_len_i.  (For seeds of unequal
 *   lengths that last form does not hold: a long seed followed by a short one that begins inside it scores more than the short
 *   one's end.)  Seeds inside a query of L letters give f_i < 2 L: a query of 2^31 letters or more => AWRY_ERR_ARG, so every score
 *   fits 32 bits.
 * Chains (minimap2's backtrack rule).  Visit the seeds in descending f, ties in ascending sorted index.  An unvisited seed e ends
 *   a chain: walk e, p_e, p_{p_e}, ... and mark each seed used; stop when there is no predecessor (base = 0) or the predecessor u
 *   is already used (base = f_u; u is not a member).  Chain score = f_e - base; the chain is reported iff score >= min_score.
 *   Seeds walked by an unreported chain stay used.  Chains of a query are reported in the order found: the first is the primary.
 * Records.  awry_chain_t: q_begin / t_begin come from the chain's first member, q_end / t_end are the maxima of q_begin + q_len /
 *   t_pos + q_len over its members, n_seeds counts them; the members are listed first to last, in sorted order.
 * Scope.  The strand the query is given on; awry_map_batch (below) maps both.  Indexes with bwt_len >= 2^32 => AWRY_ERR_ARG, as on the edit path (a small index on wide-row
 *   replicas works).  No accelerator, seed-table length, row width, replica count or chunk capacity changes any output.
 * AWRY_ERR_ARG: max_seeds == 0 or > AWRY_CHAIN_MAX_SEEDS, lookback outside 1 .. AWRY_CHAIN_MAX_LOOKBACK, max_gap == 0, min_score
 * == 0, min_len == 0, max_hits == 0.  Malformed queries fail the batch with AWRY_ERR_INVALID_QUERY, as for SMEMs, and leave the
 * out-pointers untouched; no replica => AWRY_ERR_NO_DEVICE.  The hit capacity of a chunk (AWRY_ANCHOR_HIT_CAP) is the anchors'.
 * CSR output, library-allocated (awry_free_buffer): chains of query i are chains[chain_off[i] .. chain_off[i+1]); the members of
 * chain c are seeds[seed_off[c] .. seed_off[c+1]), seed_off has chain_off[n] + 1 entries; status[n] is AWRY_Q_OK or
 * AWRY_Q_SEED_CAP.  All but chain_off_out nullable; seed_off_out and seeds_out are given or omitted together. */
enum { AWRY_CHAIN_MAX_SEEDS = 4096, AWRY_CHAIN_MAX_LOOKBACK = 64 };
typedef struct { uint32_t q_begin, q_len; uint64_t t_pos; } awry_seed_t;
typedef struct { uint32_t score, n_seeds, q_begin, q_end; uint64_t t_begin, t_end; } awry_chain_t;
int awry_chain_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len, uint64_t max_hits,
                     uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score,
                     uint64_t **chain_off_out, awry_chain_t **chains_out, uint64_t **seed_off_out, awry_seed_t **seeds_out,
                     uint8_t **status_out);

/* ---- align chains: gap fill, end extension, one CIGAR per chain (no counterpart in the reference) ----------------
 * The stage after chaining in a seed-chain-extend mapper: a chain's seeds stay as diagonal runs, the query between consecutive
 * seeds is aligned to the text between them ("gap fill"), the two ends of the read are extended into the text, and the chain gets
 * a text span, an edit count and a CIGAR.  Everything is integer arithmetic and every tie is broken explicitly.
 * Text model: the edit path's.  T is the text without its final '$', n = bwt_len - 1; queries are mapped to symbol indices and
 *   rejected exactly as on the exact path; query N equals text N; a record join or text N is an ordinary symbol that costs an
 *   edit unless the query has N there.  Unit costs.
 * Parameters: band = W, 0 <= W <= AWRY_CHAIN_ALIGN_MAX_BAND = 8; AWRY_CHAIN_ALIGN_MAX_SKEW = 16; AWRY_CHAIN_ALIGN_MAX_LEN = 1024
 *   query letters.
 * Pieces.  A chain's members, in their reported order, are (qb, len, tp); (qe, te) is a running pair.  The first member is a
 *   piece as it stands: qe = qb + len, te = tp + len.  Every later member is clipped on the left by o = max(0, qe - qb, te - tp):
 *   if o >= len it is dropped and (qe, te) stay; otherwise the piece is (qb + o, len - o, tp + o) and qe = qb + len, te = tp + len.
 *   Consecutive pieces therefore overlap neither in the query nor in the text.  A piece is a diagonal run: letter by letter it
 *   emits '=' or 'X' by comparing symbol indices, and every 'X' is one edit (the chains of awry_chain_batch give only '='; a
 *   caller's own seeds need not be exact matches).
 * Segments.  A segment aligns x (a query letters) to a prefix of y (text; at most `avail` letters readable), inside the band
 *   lo <= j - i <= hi, lo = min(0, m) - W, hi = max(0, m) + W; cells outside the band, or with j > J, are +infinity.
 *   gap between consecutive pieces: x = q[qe_prev .. qb_next), y = T[te_prev .. tb_next), b = |y|, m = b - a, J = b; global: it
 *     ends at (a, b).  a = 0 gives b 'D's, b = 0 gives a 'I's.
 *   right extension: x = q[qe_last .. L), y_j = T[te_last + j], avail = n - te_last, m = min(0, avail - a), J = min(a + W,
 *     avail); it ends at j*, the smallest j that minimises C[a][j]; t_end = te_last + j*.
 *   left extension: the same on reversed strings, x = reverse(q[0 .. qb_first)), y_j = T[tb_first - 1 - j], avail = tb_first;
 *     t_begin = tb_first - j*; the traceback from (a, j*) back to (0, 0) emits the operations already in query order.
 *   Traceback, in every segment, by awry_align_edit_batch's rule on banded values: the diagonal first ('=' / 'X'), then 'I'
 *   (i--), then 'D' (j--).
 *   NB = |m| + 2 W + 1 <= 33 cells per row.  If any segment of a chain has |m| > AWRY_CHAIN_ALIGN_MAX_SKEW -- through dropped
 *   members, a caller's seeds, or a read that hangs far over the text's start or end -- the chain is not aligned: status
 *   AWRY_ALN_SKEW, t_begin / t_end = the pieces' span, edits = 0, no runs.  Members not strictly ascending in both q_begin and
 *   t_pos, members that reach past L or n, and an empty member list give AWRY_ALN_BAD_CHAIN (so does, in the device primitive, a
 *   query that is empty or longer than AWRY_CHAIN_ALIGN_MAX_LEN): t_begin = t_end = 0, edits = 0, no runs, nothing read out of
 *   bounds.  AWRY_ALN_OK is 0.
 * Result per chain: awry_aln_t; edits = the 'X's of the pieces + the costs of all segments.  The operations of left extension,
 *   pieces, gaps and right extension are concatenated in query order and run-length encoded over the whole script (a gap's
 *   leading '=' merges with the piece before it), in the encoding of awry_align_edit_batch: len << 4 | op, I 1, D 2, = 7, X 8.
 *   The query is always consumed whole: no clipping.
 * Properties.  (1) A gap's banded cost v <= |m| + 2 W + 1 is the unbanded optimum: a path that leaves the band needs at least
 *   |m| + 2 W + 2 indels.  (2) An extension's banded cost v <= W is the unbanded optimum (over all end columns) when avail >= a.
 *   (3) Replaying the CIGAR over q and T[t_begin .. t_end) reproduces both strings and the edit count.
 *
 * awry_align_chains_batch: the arguments of awry_chain_batch, then max_alignments >= 1 -- of each query's chains the first
 * min(n_chains, max_alignments) are aligned, primary first -- and band.  CSR output, library-allocated (awry_free_buffer): the
 * alignments of query i are alns[aln_off[i] .. aln_off[i+1]), chains[] holds the awry_chain_t records of exactly those chains
 * (equal to what awry_chain_batch returns for them), the runs of alignment c are cigar[cigar_off[c] .. cigar_off[c+1]); status[n]
 * is AWRY_Q_OK or AWRY_Q_SEED_CAP.  All but aln_off_out nullable; cigar_off_out and cigar_out are given or omitted together.
 * Errors: those of awry_chain_batch; the edit path's index restrictions (bwt_len >= 2^32 or a wide-row replica =>
 * AWRY_ERR_ARG, no HBM for the text copy => AWRY_ERR_OOM); band > 8 or max_alignments == 0 => AWRY_ERR_ARG; a query longer than
 * AWRY_CHAIN_ALIGN_MAX_LEN fails the batch with AWRY_ERR_INVALID_QUERY and leaves the out-pointers untouched.  Chains and their
 * members stay on the device; the alignment runs there in sub-batches of 2^18 chains (env AWRY_CHAIN_ALIGN_SUB_BATCH, read per
 * call).  No accelerator, seed length, replica count, chunk capacity or sub-batch size changes any output. */
enum { AWRY_CHAIN_ALIGN_MAX_BAND = 8, AWRY_CHAIN_ALIGN_MAX_SKEW = 16, AWRY_CHAIN_ALIGN_MAX_LEN = 1024 };
enum { AWRY_ALN_OK = 0, AWRY_ALN_SKEW = 1, AWRY_ALN_BAD_CHAIN = 2 };
typedef struct { uint64_t t_begin, t_end; uint32_t edits, status; } awry_aln_t;
int awry_align_chains_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                            uint64_t max_hits, uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew,
                            uint32_t min_score, uint64_t max_alignments, uint32_t band, uint64_t **aln_off_out,
                            awry_chain_t **chains_out, awry_aln_t **alns_out, uint64_t **cigar_off_out, uint32_t **cigar_out,
                            uint8_t **status_out);

/* ---- map reads on both strands: revcomp seeds, ranked alignments, MAPQ (no counterpart in the reference) --------
 * The end of the seed-chain-extend pipeline: reads in, ranked placements out -- strand, position, edits, CIGAR and a mapping
 * quality.  Nucleotide indexes only (an amino index => AWRY_ERR_ARG).  Everything is integer arithmetic and every tie is broken
 * explicitly.
 * Reverse complement.  rc(q) of a query of L bytes is the byte string rc(q)[i] = ascii_of_index(comp(index_of_ascii(q[L-1-i]))),
 *   comp on symbol indices: $0 -> 0, A1 -> T5, C2 -> G3, G3 -> C2, N4 -> N4, T5 -> A1.  So case is folded, U reads as T, every
 *   other byte becomes 'N' and a sentinel stays a sentinel: a query the exact path rejects is rejected on either strand, and the
 *   error names the read's own index.
 * Candidates.  Parameters: those of awry_align_chains_batch with max_alignments named chains_per_strand = A, 1 <= A <=
 *   AWRY_MAP_MAX_CHAINS = 8, and max_report = R, 1 <= R <= 2 A.  For read i and strand s (0 forward, 1 reverse) let (c_j, a_j),
 *   j = 0 .. min(n_chains, A) - 1, be the chain records and alignments awry_align_chains_batch(.., max_alignments = A, band)
 *   returns for q (s = 0) or rc(q) (s = 1).  A candidate is a pair (s, j) with a_j.status == AWRY_ALN_OK.  Reverse-strand spans
 *   and CIGARs are left as computed on rc(q) against the forward text (the SAM convention): no CIGAR is reversed.
 * Rank.  The candidates are sorted ascending by (edits, -chain score, strand, t_begin, j): a total order.
 * Redundancy.  Walking the sorted list, a candidate is dropped if a better-ranked KEPT candidate of the SAME strand has an
 *   intersecting text span, max(b1, b2) < min(e1, e2); an empty span intersects nothing.  Two chains the chainer split at one
 *   locus count once; the same span on opposite strands (a reverse-palindromic read) counts twice.
 * Report.  The first min(R, kept) kept candidates are the read's records, the primary first; those after it carry the flag
 *   AWRY_MAP_SECONDARY.  A read with no kept candidate has no records and is not an error.
 * Status and MAPQ.  status[i] is AWRY_Q_SEED_CAP if either strand's chaining status is, else AWRY_Q_OK.  MAPQ of the primary: 0
 *   if the status is AWRY_Q_SEED_CAP; else 60 if there is no second kept candidate (whether or not R would report it); else
 *   min(60, 10 * (e2 - e1)), e1 and e2 the edits of the first and second kept candidates.  MAPQ of secondaries is 0.
 * Record.  awry_map_t, 32 bytes: t_begin / t_end / edits of the alignment, chain_score, chain_index = j, strand, mapq, flags.
 *
 * awry_map_batch: CSR output, library-allocated (awry_free_buffer): the records of read i are maps[map_off[i] .. map_off[i+1]),
 * pos[] holds, record by record, what awry_get_seq_location(t_begin) returns, the runs of record c are cigar[cigar_off[c] ..
 * cigar_off[c+1]), status[n] as above.  All but map_off_out nullable; cigar_off_out and cigar_out are given or omitted together.
 * Errors and index restrictions: those of awry_align_chains_batch (bwt_len >= 2^32 or a wide-row replica => AWRY_ERR_ARG, a read
 * longer than AWRY_CHAIN_ALIGN_MAX_LEN or rejected on the exact path => AWRY_ERR_INVALID_QUERY, no HBM for the text copy =>
 * AWRY_ERR_OOM, no replica => AWRY_ERR_NO_DEVICE); A outside 1 .. 8, R outside 1 .. 2 A or band > 8 => AWRY_ERR_ARG.  The
 * out-pointers are written only on success.  Reads are uploaded once per chunk and expanded to both strands on the device; the
 * alignment count pass (spans, edits) runs over every candidate, the CIGAR fill pass only over the records that are reported, in
 * sub-batches (AWRY_CHAIN_ALIGN_SUB_BATCH).  The capacity fallback splits a chunk between reads, never between a read's strands.
 * No accelerator, seed-table length, replica count, chunk capacity, sub-batch size or split of a chunk changes any output. */
enum { AWRY_MAP_MAX_CHAINS = 8 };
enum { AWRY_MAP_SECONDARY = 1 };
typedef struct { uint64_t t_begin, t_end; uint32_t edits, chain_score, chain_index; uint8_t strand, mapq; uint16_t flags; } awry_map_t;
int awry_map_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len, uint64_t max_hits,
                   uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score,
                   uint64_t chains_per_strand, uint64_t max_report, uint32_t band, uint64_t **map_off_out, awry_map_t **maps_out,
                   awry_pos_t **pos_out, uint64_t **cigar_off_out, uint32_t **cigar_out, uint8_t **status_out);

/* ---- soft-clip read ends: scored local extension in chain align and map (no counterpart in the reference) --------
 * A clipped mode beside the end-to-end one.  The end-to-end pass consumes the query whole; a read with an adapter tail, a read that
 * hangs over a record's end and a chimeric read then pay for letters that belong nowhere near.  Here the two end extensions are
 * scored and local: an extension may stop early and the rest of the read is soft-clipped ('S').  No end-to-end entry point
 * changes its output.  Everything is integer arithmetic and every tie is broken explicitly.
 * Parameters, passed after band: match = a, 1 .. AWRY_CLIP_MAX_MATCH = 16, the score of an '='; mismatch = b, 0 ..
 *   AWRY_CLIP_MAX_PENALTY = 64, the penalty of an 'X'; gap = g, 0 .. 64, the penalty per inserted or deleted letter; end_bonus = E,
 *   0 .. AWRY_CLIP_MAX_END_BONUS = 1024, how much score an end-to-end extension may lose and still win; at the map level also
 *   min_aln_score = T >= 0, the lowest score a candidate may have.  Out of range => AWRY_ERR_ARG.
 * Score of a script: a #'=' - b #'X' - g (#'I' + #'D'); 'S' letters score nothing.  Every score fits 32 bits (L <= 1024).
 * What stays.  Pieces, and the gaps between pieces, are exactly "align chains"'s: gaps stay global, unit cost, same band, same
 *   traceback priority.  edits counts 'X' + 'I' + 'D' of the aligned part.  Letters compare as there: a text sentinel matches
 *   nothing, query N equals text N.
 * Record bounds.  r = the record of the first piece's text start tb_first by awry_get_seq_location's rule; the record is
 *   [seq_start[r], seq_start[r+1]), the last one ends at n.  Left avail = tb_first - seq_start[r]; right avail = max(0, record end -
 *   te_last).  So a clipped extension never reaches into another record.
 * Clipped extension.  x = the a query letters outward from the piece, y_j the text outward from it (the left extension on reversed
 *   strings, as in "align chains").  J = min(a + W, avail).  The band is -W <= j - i <= W whatever avail is: the extension's skew term
 *   is gone.  Cells outside the band, or with j > J, are -infinity.  H[0][0] = 0; H[i][j] = max(H[i-1][j-1] + (a if the letters match
 *   else -b), H[i-1][j] - g, H[i][j-1] - g).  Rows beyond J + W have no cell.
 * Where it ends.  (i*, j*) maximises H over all cells; ties go to the largest i, then the smallest j; H* >= 0 because of (0, 0).  If
 *   row a has a finite cell, j_e is the smallest j that maximises H[a][j] and H_e its value; if H_e + E >= H* the extension ends at
 *   (a, j_e) and nothing is clipped.  Otherwise it ends at (i*, j*) and a - i* letters are clipped.
 * Traceback from the end cell: the diagonal first, then 'I', then 'D', on banded values, as everywhere else.
 * Skew.  AWRY_ALN_SKEW arises from gaps only: a read hanging 17 or 100 letters over an end is AWRY_ALN_OK and clipped.
 * Record.  awry_aln_clip_t, 32 bytes: awry_aln_t's fields, then score and clip_left / clip_right.  t_begin / t_end span the aligned
 *   part.  A chain that is not aligned has score 0 and clips 0.
 * Runs.  The encoding of "align chains" plus S = BAM op 4: at most one 'S' run first and one last; an 'S' run never merges with
 *   another run; the 'S' letters plus the query letters of the aligned part are always L.
 * Properties.  (1) Replaying the CIGAR over q and T[t_begin .. t_end) reproduces both strings, edits, score and both clips.
 *   (2) rec(t_begin) == rec(t_end - 1) whenever the chain's pieces lie in one record.  (3) An extension whose letters all match is
 *   never clipped: H <= a i, and ties go to the largest i.  (4) With b, g >= 1 the aligned part of a clipped extension is empty or
 *   ends, at its outer end, with '='.  (5) An extension is clipped iff H* > H_e + E; its score is H* then and H_e otherwise, so it is at
 *   least H* - E and at least H_e, and at least max(0, H_e) when E = 0 (a kept end-to-end extension may score below 0 by up to E).
 * Map level: awry_map_batch's rules except that a candidate must also have score >= T; the rank is ascending by (-score, edits,
 *   strand, t_begin, j); MAPQ of the primary is 0 under AWRY_Q_SEED_CAP, 60 without a second kept candidate, else min(60, 10 (s1 -
 *   s2) / (a + b)) with floor division, s1 and s2 the scores of the first and second kept candidates.  Redundancy, report, the
 *   secondary flag and status are unchanged.  Reverse-strand clips are those computed on rc(read).  Record awry_map_clip_t, 40 bytes:
 *   awry_map_t's fields, then score and clip_left / clip_right.  With R >= 2 a chimeric read comes out as a primary and a secondary
 *   that cover different parts of the read at two loci: that is intended.
 *
 * awry_align_chains_clip_batch and awry_map_clip_batch mirror awry_align_chains_batch and awry_map_batch: the same arguments plus the
 * scalars above, the same CSR output with the clipped records, the same errors and index restrictions.  awry_map_pairs_batch is
 * untouched: pairing clipped records is a later change, awry_map_pairs_clip_batch of "map read pairs, clipped" below. */
enum { AWRY_CLIP_MAX_MATCH = 16, AWRY_CLIP_MAX_PENALTY = 64, AWRY_CLIP_MAX_END_BONUS = 1024 };
enum { AWRY_CIGAR_SOFT_CLIP = 4 };
typedef struct { uint64_t t_begin, t_end; uint32_t edits, status; int32_t score; uint16_t clip_left, clip_right; } awry_aln_clip_t;
typedef struct { uint64_t t_begin, t_end; uint32_t edits, chain_score, chain_index; uint8_t strand, mapq; uint16_t flags; int32_t score; uint16_t clip_left, clip_right; } awry_map_clip_t;
int awry_align_chains_clip_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                                 uint64_t max_hits, uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew,
                                 uint32_t min_score, uint64_t max_alignments, uint32_t band, uint32_t match, uint32_t mismatch,
                                 uint32_t gap, uint32_t end_bonus, uint64_t **aln_off_out, awry_chain_t **chains_out,
                                 awry_aln_clip_t **alns_out, uint64_t **cigar_off_out, uint32_t **cigar_out, uint8_t **status_out);
int awry_map_clip_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                        uint64_t max_hits, uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew,
                        uint32_t min_score, uint64_t chains_per_strand, uint64_t max_report, uint32_t band, uint32_t match,
                        uint32_t mismatch, uint32_t gap, uint32_t end_bonus, uint32_t min_aln_score, uint64_t **map_off_out,
                        awry_map_clip_t **maps_out, awry_pos_t **pos_out, uint64_t **cigar_off_out, uint32_t **cigar_out,
                        uint8_t **status_out);

/* ---- map read pairs: insert-size pairing, mate rescue, proper-pair flag (no counterpart in the reference) --------
 * Short reads come in pairs: two reads from the ends of one fragment, on opposite strands, a known distance apart.  The mate places
 * a read whose own seeds are ambiguous or missing.  This stage joins the ranked candidates of awry_map_batch with the k-edit scan
 * and aligner of awry_locate_edit_batch / awry_align_edit_batch.  Nucleotide indexes only.  Everything is integer arithmetic and
 * every tie is broken explicitly.
 * Input.  n = 2P reads, interleaved: read 2p is mate 0 of pair p, read 2p + 1 is mate 1; odd n => AWRY_ERR_ARG.  Parameters: those
 *   of awry_map_batch without max_report (min_len, max_hits, the five chain parameters, chains_per_strand = A, band), and min_insert
 *   <= max_insert <= AWRY_PAIR_MAX_INSERT = 1 << 20; unpaired_penalty = U, in edits, 0 .. 255; rescue_anchors = G, 0 ..
 *   AWRY_PAIR_MAX_ANCHORS = 4 (0: no rescue); rescue_edits = k, 0 .. AWRY_MAX_EDITS.
 * Kept lists.  K_m, m in {0, 1}, is the list of ALL kept candidates of mate m in rank order, exactly as awry_map_batch defines rank
 *   and redundancy: what max_report = 2 A would report, at most 16 entries.  Each read's status is the one awry_map_batch gives.
 * Proper.  For x in a list of mate 0 and y in a list of mate 1 let f be the one on strand 0 and v the one on strand 1.  proper(x, y)
 *   iff the strands differ and rec(f.t_begin) == rec(v.t_begin) (rec: the record awry_get_seq_location returns) and f.t_begin <=
 *   v.t_begin and f.t_end <= v.t_end and min_insert <= v.t_end - f.t_begin <= max_insert.  FR orientation; the insert is the outer
 *   distance.
 * Rescue (G > 0).  For mate m, each of the first min(|K_m|, G) candidates x of K_m, at rank index a, is an ANCHOR iff no y in
 *   K_{1-m} is proper with it and the other mate's length L' satisfies k < L' <= AWRY_EDIT_MAX_LEN.  An anchor seeks the other mate
 *   on strand 1 - x.strand: query 4p + 2 (1 - m) + (1 - x.strand) of the doubled batch.  Its window of starts, in signed arithmetic,
 *   both ends inclusive: x on strand 0: lo = x.t_begin + max(0, min_insert - L' - k), hi = x.t_begin + max_insert - L' + k; x on
 *   strand 1: lo = x.t_end - max_insert, hi = min(x.t_begin, x.t_end - min_insert).  The window is cut to [0, n_text) and to the
 *   record of x.t_begin, [seq_start[r], seq_start[r+1]) (the last record ends at n_text); it is empty if hi < lo.  The hits in the
 *   window are the hits of awry_locate_edit_batch's rule at max_edits = k -- local minima of D over the whole text: they do not
 *   depend on where the window is cut (the candidate cap plays no part: no pieces are looked up).  The anchor's rescue hit is the hit
 *   with the smallest (D(s), s); its alignment is awry_align_edit_batch's (text_len, runs).  The rescued candidate z: strand 1 -
 *   x.strand, t_begin = s, t_end = s + text_len, edits = D(s), chain_score = 0, chain_index = AWRY_PAIR_NO_CHAIN = 0xFFFFFFFF, flag
 *   AWRY_MAP_RESCUED.
 * Augmented lists.  Only original candidates are anchors.  K'_t is K_t followed by the rescued candidates aimed at mate t = 1 - m,
 *   in anchor order a = 0, 1, ..; each z is appended unless its span intersects (the redundancy rule's test) the span of a
 *   same-strand member already in K'_t, originals and earlier appended ones alike.  z is kept whether or not it turns out proper.
 * Pair choice.  For (x, y) in K'_0 x K'_1: cost = x.edits + y.edits + (proper(x, y) ? 0 : U).  The pairs are ordered ascending by
 *   (cost, !proper, index of x in K'_0, index of y in K'_1); the first is the best pair, the next, if any, the second.  Pair MAPQ: 0
 *   if either read's status is AWRY_Q_SEED_CAP; else 60 if there is no second pair; else min(60, 10 * (cost2 - cost1)).
 * Records.  At most one awry_map_t per read; no secondary or supplementary pair records.  Both K'_0 and K'_1 non-empty: read 2p gets
 *   x and read 2p + 1 gets y of the best pair, both with the pair MAPQ, both with AWRY_MAP_PROPER_PAIR (= 2) iff the pair is proper,
 *   a rescued candidate with AWRY_MAP_RESCUED (= 4), no other flag.  Exactly one non-empty (then it is K_m): that read's record is
 *   K_m[0] exactly as awry_map_batch reports its primary, single-end MAPQ included, plus AWRY_MAP_MATE_UNMAPPED (= 8); the other
 *   read has no record.  Both empty: no records, not an error.  insert[p] = v.t_end - f.t_begin for a proper best pair, else 0.
 *   Reverse-strand spans and CIGARs stay as computed on rc(read) against the forward text; the runs of a rescued record are the edit
 *   aligner's, at most AWRY_ALIGN_MAX_OPS.
 *
 * awry_map_pairs_batch: CSR output like awry_map_batch's -- map_off[2P + 1], maps, pos, cigar_off / cigar, status[2P] -- plus
 * insert[P].  All but map_off_out nullable; cigar_off_out and cigar_out are given or omitted together.  Errors and index
 * restrictions: awry_map_batch's; a bad new argument => AWRY_ERR_ARG; an invalid read fails the batch with AWRY_ERR_INVALID_QUERY
 * and names the read's own index in the interleaved batch.  The out-pointers are written only on success.  Shards, chunks and the
 * capacity fallback cut between pairs, never inside one; a rescue window of more than 64 starts (env AWRY_PAIR_SUB_WINDOW, read per
 * call) is scanned in pieces.  No accelerator, seed-table length, replica count, chunk capacity, sub-batch size, grid cap or window
 * cut changes any output. */
enum { AWRY_PAIR_MAX_INSERT = 1 << 20, AWRY_PAIR_MAX_ANCHORS = 4 };
enum { AWRY_MAP_PROPER_PAIR = 2, AWRY_MAP_RESCUED = 4, AWRY_MAP_MATE_UNMAPPED = 8 };
#define AWRY_PAIR_NO_CHAIN 0xFFFFFFFFu
int awry_map_pairs_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                         uint64_t max_hits, uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew,
                         uint32_t min_score, uint64_t chains_per_strand, uint32_t band, uint64_t min_insert, uint64_t max_insert,
                         uint32_t unpaired_penalty, uint32_t rescue_anchors, int rescue_edits, uint64_t **map_off_out,
                         awry_map_t **maps_out, awry_pos_t **pos_out, uint64_t **cigar_off_out, uint32_t **cigar_out,
                         uint8_t **status_out, uint32_t **insert_out);

/* ---- map read pairs, clipped: clipped pairing and rescue (no counterpart in the reference) ------------------------------
 * The clipped mode of "map read pairs", beside the end-to-end one.  A fragment shorter than the reads makes both mates read through
 * into the adapter: mate 0 is I genomic letters and then L - I adapter letters, rc(mate 1) the same I letters after L - I adapter
 * letters.  End to end both alignments run through the adapter, the forward record ends after the reverse one and begins after it,
 * and the pair that is easiest to place comes out improper.  Here the kept lists are those of "soft-clip read ends", both mates
 * align to the fragment, and the insert is measured between the mates' 5' ends projected through their clips.  No other entry point
 * changes its output.  All arithmetic is signed integer and every tie is broken explicitly.
 * Parameters.  Those of awry_map_pairs_batch and, after rescue_edits, the five clip scalars of awry_map_clip_batch: match = a,
 *   mismatch = b, gap = g, end_bonus = E, min_aln_score = T, with the same ranges and the same AWRY_ERR_ARG.  unpaired_penalty = U is
 *   in score units here, 0 .. AWRY_PAIR_CLIP_MAX_UNPAIRED = 16384: the largest score a read of AWRY_CHAIN_ALIGN_MAX_LEN letters can
 *   reach at a = 16.
 * Kept lists.  K_m is what awry_map_clip_batch would report for mate m at max_report = 2 A: awry_map_clip_t records in that
 *   section's rank order, the threshold T applied, at most 16 entries.  Each read's status is the one awry_map_clip_batch gives.
 * Fragment ends.  For a record x on strand 0, fb(x) = x.t_begin - x.clip_left; for a record on strand 1, ve(x) = x.t_end +
 *   x.clip_right: the 5' ends of the two mates projected through their clips.  Reverse-strand clips are those computed on rc(read), so
 *   clip_left is always the text-left side.  Either value may lie outside the record or below 0; they are used only in differences.
 * Proper.  f the record on strand 0, v the one on strand 1.  proper_clip(x, y) iff the strands differ and rec(f.t_begin) ==
 *   rec(v.t_begin) and f.t_begin <= v.t_begin and f.t_end <= v.t_end (on the aligned spans, as end to end) and min_insert <= ve(v) -
 *   fb(f) <= max_insert.  The insert is ve(v) - fb(f).  With all clips 0 this is proper of the end-to-end section, to the letter.
 * Rescue.  The anchor rule is unchanged, with proper_clip in place of proper.  The windows: x on strand 0: lo = max(x.t_begin, fb(x)
 *   + min_insert - L' - k), hi = fb(x) + max_insert - L' + k; x on strand 1: lo = ve(x) - max_insert, hi = min(x.t_begin, ve(x) -
 *   min_insert); cut to the text and to the record of x.t_begin as there.  Scan and aligner are the existing ones: a rescue hit is a
 *   whole-mate alignment within k edits, exactly as in awry_map_pairs_batch.  The rescued candidate z additionally carries score = a
 *   #'=' - b #'X' - g (#'I' + #'D') of the aligner's runs and clip_left = clip_right = 0, and exists only if score >= T.  A mate
 *   whose junk tail exceeds k edits is therefore not rescuable: a stated limit (scored local rescue is a later change).
 * Augmented lists.  As end to end; the span-intersection test uses the aligned spans.
 * Pair choice.  S(x, y) = x.score + y.score - (proper_clip(x, y) ? 0 : U).  The pairs are ordered ascending by (-S, !proper, index
 *   of x in K'_0, index of y in K'_1).  Pair MAPQ: 0 if either read's status is AWRY_Q_SEED_CAP; else 60 if there is no second pair;
 *   else min(60, 10 (S1 - S2) / (a + b)) with floor division.
 * Records.  At most one awry_map_clip_t per read, with the flags of the end-to-end section.  Exactly one mate with candidates: its
 *   record is the primary of awry_map_clip_batch plus AWRY_MAP_MATE_UNMAPPED.  insert[p] = ve(v) - fb(f) for a proper best pair,
 *   else 0.  The runs of a chain-derived record are the clipped aligner's ('S' runs included), those of a rescued record the edit
 *   aligner's.
 * Properties.  (1) Replaying a record's CIGAR over the read (rc(read) on strand 1) and T[t_begin .. t_end) reproduces edits, score
 *   and both clips; rescued records too.  (2) If every record of both lists has clips 0, the windows and proper_clip are those of
 *   the end-to-end section.  (3) A proper best pair has min_insert <= insert[p] <= max_insert.
 *
 * awry_map_pairs_clip_batch: awry_map_pairs_batch's arguments with the five scalars after rescue_edits, the same CSR output with
 * awry_map_clip_t records, the same errors, index restrictions and invariances. */
enum { AWRY_PAIR_CLIP_MAX_UNPAIRED = 16384 };
int awry_map_pairs_clip_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                              uint64_t max_hits, uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew,
                              uint32_t min_score, uint64_t chains_per_strand, uint32_t band, uint64_t min_insert,
                              uint64_t max_insert, uint32_t unpaired_penalty, uint32_t rescue_anchors, int rescue_edits,
                              uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus, uint32_t min_aln_score,
                              uint64_t **map_off_out, awry_map_clip_t **maps_out, awry_pos_t **pos_out, uint64_t **cigar_off_out,
                              uint32_t **cigar_out, uint8_t **status_out, uint32_t **insert_out);

/* ---- split reads: supplementary alignments by query overlap (no counterpart in the reference) --------------------------
 * A read can come from two places: a chimeric read, a read over a breakpoint, a read that runs across the join of two records.
 * awry_map_clip_batch reports its second half as a secondary with MAPQ 0, and computes the primary's MAPQ against it although it
 * explains other letters.  Here the kept candidates are sorted by the part of the read they explain: SEGMENTS cover different letters
 * (the first is the primary, the later ones are supplementary), SECONDARIES are other places for the letters of a segment, and every
 * segment has a MAPQ of its own against the best competitor for its letters.  No other entry point changes its output.  Everything
 * is integer arithmetic and every tie is broken explicitly.
 * Parameters.  Those of awry_map_clip_batch without max_report, plus max_segments = P, 1 <= P <= AWRY_SPLIT_MAX_SEGMENTS = 4;
 *   max_secondary = R2, 0 <= R2 <= 2 A; max_overlap = O, a percentage, 1 <= O <= 100.  Out of range => AWRY_ERR_ARG.
 * Candidates, threshold and rank are exactly the clipped map level's ("soft-clip read ends"): status AWRY_ALN_OK and score >= T,
 *   among the first A chains of each strand, ordered ascending by (-score, edits, strand, t_begin, j).
 * Query interval, in the read's own orientation, L the read's length: (lo, hi) = (clip_left, clip_right) on strand 0 and
 *   (clip_right, clip_left) on strand 1; q_begin = min(lo, L); q_end = max(q_begin, L - min(hi, L)).  Real alignments never saturate;
 *   the device primitive accepts any records, so the saturation is part of the definition (and a length above 65535 counts as 65535
 *   there: the interval is two 16-bit fields).  A candidate with q_end == q_begin is dropped: it is not kept and plays no part in
 *   redundancy.
 * The walk.  The ranked list is walked once, and for each candidate c: (1) c is dropped if a better-ranked KEPT candidate (segment or
 *   secondary) of the same strand has an intersecting text span -- the redundancy test of awry_map_batch, unchanged.  (2) Otherwise,
 *   with the segments so far g_0, g_1, .. in the order they were accepted, c OVERLAPS g when ov = min(c.q_end, g.q_end) -
 *   max(c.q_begin, g.q_begin) > 0 and 100 ov >= O min(c.q_end - c.q_begin, g.q_end - g.q_begin).  If c overlaps some segment, with g_x
 *   the first such, c is kept as a secondary of g_x, and if g_x has no sub yet, sub(g_x) = c.score: the list is ranked, so this is the
 *   best competitor for those letters.  (3) Otherwise, if fewer than P segments exist, c is kept as a new segment; if P segments
 *   exist already, c is dropped and not kept.
 * Report.  The segments first, in acceptance order: segment 0 is the primary, with flags 0; each later segment carries
 *   AWRY_MAP_SUPPLEMENTARY = 16.  Then the first min(R2, #secondaries) secondaries in rank order, each with AWRY_MAP_SECONDARY.
 *   parent is the index, among this read's records, of the record's segment; a segment's parent is its own index.  The walk always
 *   runs to the end of the list, because a late candidate can be a late segment's sub; only the report is cut.
 * Status and MAPQ.  Status as in awry_map_batch.  Every segment has MAPQ 0 under AWRY_Q_SEED_CAP; otherwise a segment with no sub has
 *   MAPQ 60, and one with a sub has min(60, 10 (score - sub) / (a + b)) with floor division.  Secondaries have MAPQ 0.
 * Record.  awry_map_split_t, 48 bytes: awry_map_clip_t's eleven fields at the same offsets, then uint16_t q_begin, q_end, parent,
 *   reserved (= 0).  Spans, clips and CIGARs of strand-1 records stay those of rc(read) against the forward text.  Soft clips stay
 *   soft: the 'S' letters of a supplementary are the letters the other segments explain.
 * Properties.  (1) q_end - q_begin equals the query letters of the record's CIGAR, and q_begin / q_end follow from strand, clips and
 *   L.  (2) A read whose walk yields one segment with P >= 2 is reported exactly as awry_map_clip_batch reports it at max_report = 1 +
 *   R2: the same records, fields, MAPQ and runs.  (3) No two segments of a read overlap in the sense above.  (4) Every secondary
 *   overlaps its parent, and overlaps no segment accepted before its parent.  (5) At P = 1 the primary's MAPQ never falls below
 *   awry_map_clip_batch's for the same read: the competitor set shrinks and the primary is the same.
 * Not done.  The uncovered part of a read is not seeded again: a split whose second half is not among the first A chains of either
 *   strand is not found (raise A).  awry_map_pairs_clip_batch is untouched.  No hard clips.
 *
 * awry_map_split_batch: awry_map_clip_batch's arguments with max_segments, max_secondary, max_overlap in the place of max_report, the
 * same CSR output with awry_map_split_t records, the same nullability, errors, index restrictions and invariances. */
enum { AWRY_SPLIT_MAX_SEGMENTS = 4 };
enum { AWRY_MAP_SUPPLEMENTARY = 16 };
typedef struct { uint64_t t_begin, t_end; uint32_t edits, chain_score, chain_index; uint8_t strand, mapq; uint16_t flags; int32_t score; uint16_t clip_left, clip_right; uint16_t q_begin, q_end, parent, reserved; } awry_map_split_t;
int awry_map_split_batch(awry_index_t *idx, const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint32_t min_len,
                         uint64_t max_hits, uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew,
                         uint32_t min_score, uint64_t chains_per_strand, uint64_t max_segments, uint64_t max_secondary,
                         uint32_t max_overlap, uint32_t band, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus,
                         uint32_t min_aln_score, uint64_t **map_off_out, awry_map_split_t **maps_out, awry_pos_t **pos_out,
                         uint64_t **cigar_off_out, uint32_t **cigar_out, uint8_t **status_out);

/* releases an array one of the calls above (or awry_locate / awry_read_query_file) returned.  Result arrays are pinned
 * host memory recycled through a process-wide pool (the device writes results straight into them); never pass them to
 * free().  AWRY_PINNED_CACHE_GB (default 4) bounds what the pool keeps between calls. */
void awry_free_buffer(void *p);

/* ---- scalar conveniences (each launches on replica 0) ---------------------------------------------- */
int awry_count(awry_index_t *idx, const uint8_t *q, uint64_t len, uint64_t *count);          /* count_string :499  */
/* get_search_range_for_string (pub(crate) in the reference, :402-438): the row interval of q.  It follows the reference's own
 * step schedule -- no device seed table; for len >= lookup_table_kmer_len the first kmer_len - 1 steps are taken whether or
 * not the range is already empty (src/kmer_lookup_table.rs:90-110) -- so an ABSENT query returns the same (start_ptr, end_ptr)
 * as the reference (start_ptr = end_ptr + 1, not a canonical {1, 0}); pinned against the oracle in tests/test_gpu_parity.py */
int awry_search_range(awry_index_t *idx, const uint8_t *q, uint64_t len, awry_range_t *out);
int awry_locate(awry_index_t *idx, const uint8_t *q, uint64_t len, awry_pos_t **hits_out,
                uint64_t **global_pos_out, uint64_t *n_hits);                                /* locate_string :516 */
int awry_initial_range(const awry_index_t *idx, uint8_t symbol_ascii, awry_range_t *out);    /* :383-385          */
int awry_update_range(awry_index_t *idx, awry_range_t in, uint8_t symbol_ascii, awry_range_t *out); /* :559-582   */
int awry_backstep(awry_index_t *idx, uint64_t row, uint64_t *out);                           /* :585-593          */
int awry_get_seq_location(const awry_index_t *idx, uint64_t global_pos, awry_pos_t *out);    /* sequence_index.rs:108 */

/* ---- accessors (src/fm_index.rs:302-399) ------------------------------------------------------------ */
int awry_alphabet(const awry_index_t *idx);
uint64_t awry_bwt_len(const awry_index_t *idx);
uint64_t awry_version(const awry_index_t *idx);
uint64_t awry_sa_ratio(const awry_index_t *idx);
uint8_t awry_kmer_len(const awry_index_t *idx);
const uint64_t *awry_prefix_sums(const awry_index_t *idx, uint64_t *len);
uint64_t awry_num_sequences(const awry_index_t *idx);
uint64_t awry_sequence_start(const awry_index_t *idx, uint64_t i);
const char *awry_sequence_header(const awry_index_t *idx, uint64_t i);
uint64_t awry_sentinel_row(const awry_index_t *idx);
/* device-layout BWT blocks and packed SA words of the host copy (layout.h); for tests and tooling */
const uint64_t *awry_block_words(const awry_index_t *idx, uint64_t *nwords);
const uint64_t *awry_sa_words(const awry_index_t *idx, uint64_t *nwords);
/* one block converted to the reference layout (planes, then 8 / 24 milestones), src/bwt.rs:12-25 */
int awry_block_reference_layout(const awry_index_t *idx, uint64_t block, uint64_t *out, uint64_t out_words);

const char *awry_last_error(void); /* thread-local message of the last non-zero status */

/* ---- host utilities ----------------------------------------------------------------------------------- */
/* query ingestion: every record of a FASTA / FASTQ file becomes one query; library-allocated CSR arrays
 * (awry_free_buffer) ready for awry_count_batch / awry_locate_batch */
int awry_read_query_file(const char *path, uint8_t **qbytes_out, uint64_t **qoff_out, uint64_t *n_out);
/* suffix array of a byte text ending in '$' (host SA-IS; stands in for libsufr, src/fm_index.rs:156-181) */
int awry_host_suffix_array(const uint8_t *text, uint64_t n, uint64_t *sa_out);
uint8_t awry_symbol_index(int alphabet, uint8_t ascii); /* Symbol::new_ascii(..).index(), src/alphabet.rs:109,152 */
/* the host half of awry_count_batch / awry_locate_batch for nucleotide batches (caller side of src/fm_index.rs:455-487):
 * n ASCII queries -> 2-bit words on the library's worker pool (AVX2), so that 8 B per 31-mer cross PCIe instead of 31.
 * qoff == NULL: n queries of L bytes back to back; else query i = qbytes[qoff[i] .. qoff[i+1]) with 1..L letters and
 * lens_out[i] receives its length.  W = ceil(L / 32) words per query (letter j in word j / 32, bits 2 (j % 32), A0 C1
 * G2 T3, unused bits zero).  Queries holding a byte outside ACGTacgt are listed (ascending) in bad_out[0 .. *nbad_out)
 * (room for n; nullable) -- the batch paths hand those to the generic kernel.  Needs no GPU; searches nothing. */
int awry_host_pack_nt2(const uint8_t *qbytes, const uint64_t *qoff, uint64_t n, uint64_t L, uint64_t *words_out,
                       uint32_t *lens_out, uint32_t *bad_out, uint64_t *nbad_out);
int awry_host_threads(void); /* size of that pool: the CPUs this process may use (cgroup quota / affinity; AWRY_HOST_THREADS) */
void awry_host_memcpy(void *dst, const void *src, uint64_t bytes); /* memcpy cut over that pool (what copies results out) */

/* ---- device-resident API: pointers are device memory on replica `slot`'s GPU, work is queued on
 *      `stream` (a hipStream_t, NULL = default stream) and NOT synchronised.  Scratch (survivor lists, work-queue
 *      heads) is kept per stream, so any number of launches may be in flight across streams.  Query byte buffers
 *      (d_qbytes, d_ascii) are read in aligned 8-byte words: they must be readable up to 8 bytes past the last
 *      query (allocations of awry_dev_malloc and hipMalloc are).
 *      What a caller may do at the same time:
 *      - streams: any number of streams per replica, each with any number of launches queued; a call that has to grow its
 *        stream's scratch first waits for that stream alone (hipStreamSynchronize), then frees and reallocates;
 *      - host threads: any number, on the same or on different streams and replicas, next to threads inside the batch and
 *        scalar entry points above.  The handle is immutable after awry_set_devices; the awry_set_* / awry_debug_* knobs and
 *        awry_set_devices itself are NOT safe beside running queries;
 *      - one stream (the NULL stream included -- what a caller that passes no stream gets) from two host threads: safe for
 *        the library's own state -- an entry point reads, grows and launches with its stream's scratch as one step under
 *        a lock of that stream, and hands out work-queue heads in launch order -- but the two threads' launches are queued
 *        in whatever order the threads arrive, so the buffers a caller passes must not be shared between them unless the
 *        caller orders the threads itself. ----------------------------------------------------------------------- */
int awry_replica_device(const awry_index_t *idx, int slot);
/* fixed-length ACGT reads, ASCII n*L bytes -> n * ceil(L/32) packed u64 words (letter j in word j/32, bits 2(j%32));
 * *d_bad (u64 on device, caller-zeroed) counts queries with other bytes */
int awry_dev_pack_nt2(awry_index_t *idx, int slot, const void *d_ascii, uint64_t n, int L, void *d_words,
                      void *d_bad, void *stream);
/* the hot kernel: count n packed k-mers -> u64 counts.  use_seed != 0 starts from the seed table */
int awry_dev_count_nt2(awry_index_t *idx, int slot, const void *d_words, uint64_t n, int L, void *d_counts,
                       int use_seed, void *stream);
/* same kernel with a work census for the roofline figure: d_tally[6] (u64, caller-zeroed) += {seed probes,
 * executed steps, distinct BWT blocks ranked, SA reads and text windows of seed-and-verify, blocks ranked by steps
 * after a query's first 10 (single-kernel schedule only: the ones whose lines no longer sit in the Infinity Cache), and --
 * caller passes d_tally[8] -- nodes of the left-context index consulted, its (position, row) entries read} --
 * the first three are the tallies SURVEY.md 8(d) prices at 16 B / 104 B each */
int awry_dev_count_nt2_tally(awry_index_t *idx, int slot, const void *d_words, uint64_t n, int L, void *d_counts,
                             int use_seed, void *d_tally, void *stream);
/* generic path: ASCII queries + u64 offsets[n+1] -> counts[n], optional ranges[2n] (start,end) and status[n] bytes */
int awry_dev_count_ascii(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n,
                         void *d_counts, void *d_ranges, void *d_status, void *stream);
/* the count pass of a device-resident parallel_locate: as above, but d_locate_words[2n] receives what awry_dev_locate
 * (range_stride 2) needs per query -- a row interval, or the text position(s) the count pass already verified when the
 * seed-and-verify accelerators are resident -- instead of row intervals, which lets the fast schedules run (amino k-mers:
 * 10x the rate of awry_dev_count_ascii with ranges).  The words are opaque: feed them to awry_dev_locate, nothing else. */
int awry_dev_count_ascii_for_locate(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n,
                                    void *d_counts, void *d_locate_words, void *d_status, void *stream);
/* n ASCII queries of `len` bytes each, back to back (no offsets) -> counts[n], optional status[n].  Nucleotide
 * indexes: packed on the device and served by the packed kernels (queries with letters outside ACGT are redone by the
 * generic kernel).  Amino queries of 8..1024 residues: a two-phase schedule of their own (one query per lane against the
 * seed table and the text -- the last 24 residues in registers, the rest compared with the text for surviving candidates --
 * and the generic kernel on the few it cannot decide).  Every other shape: the generic kernel
 * reading query q at q * len.  Scratch lives in the replica, per stream. */
int awry_dev_count_ascii_uniform(awry_index_t *idx, int slot, const void *d_qbytes, uint64_t n, uint64_t len,
                                 void *d_counts, void *d_status, void *stream);
/* the amino k-mer schedule of awry_dev_count_ascii_uniform with a work census: d_tally[5] (u64, caller-zeroed) +=
 * {seed probes, executed steps, distinct BWT blocks ranked, SA reads, text comparisons} over both of its passes
 * (168 B per block); slower than the plain call (per-event atomics) -- for untimed runs */
int awry_dev_count_ascii_uniform_tally(awry_index_t *idx, int slot, const void *d_qbytes, uint64_t n, uint64_t len,
                                       void *d_counts, void *d_tally, void *stream);
/* substitution-tolerant count (see awry_count_mismatch_batch), device-resident form for timing and device callers (no
 * allocation inside; workspace owned by the replica): ASCII queries + u64 offsets[n+1] -> d_counts[n * (k + 1)], optional
 * d_status[n] bytes (non-zero: rejected query, counts 0) */
int awry_dev_count_mismatch(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n,
                            int max_mismatches, void *d_counts, void *d_status, void *stream);
/* the same with a work census: d_tally[2] (u64, caller-zeroed) += {expansions -- Occ of every symbol at the two rows of one
 * node, two block lines --, queries searched}; per-lane atomics at the end of the launch only */
int awry_dev_count_mismatch_tally(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n,
                                  int max_mismatches, void *d_counts, void *d_status, void *d_tally, void *stream);
/* class-pattern count (see awry_count_pattern_batch), device-resident form (no synchronisation; the stack workspace is owned
 * by the replica, per stream, and grows on first use): ASCII patterns + u64 offsets[n+1] -> d_counts[n * (k + 1)], optional
 * d_status[n] bytes (AWRY_Q_*; non-zero: rejected or abandoned pattern, counts 0) */
int awry_dev_count_pattern(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n,
                           int max_mismatches, void *d_counts, void *d_status, void *stream);
/* the same with a work census: d_tally[3] (u64, caller-zeroed): [0] += expansions, [1] += patterns searched, [2] = max with
 * the deepest stack of the launch, in frames; per-lane atomics at the end of the launch only */
int awry_dev_count_pattern_tally(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n,
                                 int max_mismatches, void *d_counts, void *d_status, void *d_tally, void *stream);
/* anchors (see awry_anchor_batch), device-resident form: no synchronisation, no allocation, any stream.  Two calls with the
 * caller's scan between them: d_anchor_off == NULL is the count pass -- ASCII queries + u64 offsets[n+1] -> d_n_anchors[n]
 * (u64) and optional d_status[n] bytes (non-zero: rejected query, 0 anchors); awry_dev_scan_counts turns d_n_anchors into
 * d_anchor_off[n+1]; the fill pass (d_anchor_off given) repeats the walk and writes the awry_anchor_t records of query q at
 * d_anchors[d_anchor_off[q] ...) (d_n_anchors / d_status nullable there; a slot at or beyond d_anchor_off[q+1] is never
 * written).  Every query must be shorter than 2^32 letters. */
int awry_dev_anchors(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n, uint32_t min_len, int skip,
                     void *d_n_anchors, const void *d_anchor_off, void *d_anchors, void *d_status, void *stream);
/* the same with a work census: d_tally[3] (u64, caller-zeroed) += {LF steps executed (the ones that emptied the range
 * included), seed-table probes that supplied a range, anchors reported}; one atomic per query and counter */
int awry_dev_anchors_tally(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n, uint32_t min_len,
                           int skip, void *d_n_anchors, const void *d_anchor_off, void *d_anchors, void *d_status,
                           void *d_tally, void *stream);
/* SMEMs (see awry_smem_batch), device-resident form: the two-call protocol of awry_dev_anchors, without skip -- d_smem_off ==
 * NULL is the count pass (d_n_smems[n] u64, optional d_status[n]); awry_dev_scan_counts; the fill pass writes the records of
 * query q at d_smems[d_smem_off[q] ...) and never a slot at or beyond d_smem_off[q+1].  The forward extension runs as a
 * search of the dense suffix array against the text where the replica keeps both (the verify accelerators), else as a
 * bisection over backward searches; the records are the same. */
int awry_dev_smems(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n, uint32_t min_len,
                   void *d_n_smems, const void *d_smem_off, void *d_smems, void *d_status, void *stream);
/* the same with a work census: d_tally[4] (u64, caller-zeroed) += {LF steps executed (the ones that emptied the range
 * included), suffixes compared by the suffix-array search, forward extensions performed, SMEMs reported}; one atomic per
 * query and counter */
int awry_dev_smems_tally(awry_index_t *idx, int slot, const void *d_qbytes, const void *d_qoff, uint64_t n, uint32_t min_len,
                         void *d_n_smems, const void *d_smem_off, void *d_smems, void *d_status, void *d_tally, void *stream);
/* The device primitive under awry_locate_edit_batch, for a caller who seeds with SMEMs and verifies candidate loci of their
 * own.  Window w asks for the hits of query d_win_query[w] (u32 index into the CSR d_qbytes / d_qoff) among the starts
 * [d_win_first[w], d_win_first[w] + d_win_count[w]), cut to [0, n); the kernel reads the text it needs around them itself
 * (T[max(first - 1, 0) .. min(last + L + k + 3, n)), last = the last owned start).  Two calls with the caller's scan between
 * them: d_hit_off == NULL is the count pass -> d_n_hits[m] (u64); awry_dev_scan_counts turns it into d_hit_off[m+1]; the
 * fill pass writes window w's hits in ascending position at d_gpos (u64) / d_edits (u8) [d_hit_off[w], d_hit_off[w+1]).
 * Windows of one query must own disjoint starts; keep them adjacent and ascending and the hits of a query are ascending.
 * Values are exact whatever the window cut.  A window whose query is empty, longer than AWRY_EDIT_MAX_LEN or not longer than
 * max_edits has no hits; bytes are mapped as on the exact path ('$' / '#' and bytes >= 0x80 equal no text symbol).  No
 * synchronisation except where the pattern-mask workspace (owned by the replica, per stream) grows, or the text copy is built,
 * on first use; the masks are per window here, at 4 words per column. */
int awry_dev_edit_windows(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff, const uint32_t *d_win_query,
                          const uint64_t *d_win_first, const uint32_t *d_win_count, uint64_t m, int max_edits, uint64_t *d_n_hits,
                          const uint64_t *d_hit_off, uint64_t *d_gpos, uint8_t *d_edits, void *stream);
/* the same with a work census: d_tally[2] (u64, caller-zeroed) += {text columns scanned, windows scanned}; a window without
 * owned starts or without a query the scan takes counts as neither; per-lane atomics at the end of the launch only */
int awry_dev_edit_windows_tally(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff,
                                const uint32_t *d_win_query, const uint64_t *d_win_first, const uint32_t *d_win_count, uint64_t m,
                                int max_edits, uint64_t *d_n_hits, const uint64_t *d_hit_off, uint64_t *d_gpos, uint8_t *d_edits,
                                uint64_t *d_tally, void *stream);
/* The device primitive under awry_align_edit_batch (the definition is stated there), for a caller with hits of their own.
 * Hit h is the triple (d_hit_query[h] (u32 index into the CSR d_qbytes / d_qoff), d_hit_gpos[h] (u64 start), d_hit_edits[h] (u8
 * distance)); output at a fixed stride: d_text_len[m] (u32), d_n_ops[m] (u8) and the runs d_ops[h * AWRY_ALIGN_MAX_OPS ..
 * + d_n_ops[h]) (u32, m * AWRY_ALIGN_MAX_OPS entries; the rest of a hit's slot is unspecified).  A triple that is no alignment
 * at that distance gets d_n_ops = 0 and d_text_len = 0 and nothing else happens: the minimum of row L inside the band of
 * half-width d_hit_edits[h] differs from d_hit_edits[h]; the start is >= n; the distance exceeds max_edits; the query is
 * empty, longer than AWRY_EDIT_MAX_LEN or not longer than max_edits.  A start that is no local minimum of D but has D(s) = the
 * given distance is aligned by the same rule (its script may begin with 'D').  Hits in query order read best.  No
 * synchronisation except where the direction workspace (owned by the replica, per stream, at most 128 MiB) grows, or the text
 * copy is built, on first use. */
int awry_dev_edit_align(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff, const uint32_t *d_hit_query,
                        const uint64_t *d_hit_gpos, const uint8_t *d_hit_edits, uint64_t m, int max_edits, uint32_t *d_text_len,
                        uint8_t *d_n_ops, uint32_t *d_ops, void *stream);
/* the same with a work census: d_tally[2] (u64, caller-zeroed) += {hits aligned (d_n_ops != 0), table cells computed (the cells
 * of rows 0..L with |i - j| <= d and j <= J, of every triple whose query and start the kernel takes)} */
int awry_dev_edit_align_tally(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff,
                              const uint32_t *d_hit_query, const uint64_t *d_hit_gpos, const uint8_t *d_hit_edits, uint64_t m,
                              int max_edits, uint32_t *d_text_len, uint8_t *d_n_ops, uint32_t *d_ops, uint64_t *d_tally,
                              void *stream);
/* Chaining (see awry_chain_batch), device-resident form, for the seeds of any seeder: query q has the seeds d_seeds[d_seed_off[q]
 * .. d_seed_off[q+1]), in any order (the input index is the last sort key); a seed's t_pos at or past bwt_len counts as a position
 * of the last record.  The two-call protocol of awry_dev_smems: d_chain_off == NULL is the count pass -> d_n_chains[n] and
 * d_n_members[n] (u64 each: chains of the query, and seeds in all of them) and optional d_status[n]; awry_dev_scan_counts, twice,
 * turns them into d_chain_off[n+1] and d_member_off[n+1]; the fill pass writes the chains of query q at d_chains[d_chain_off[q]
 * ...) and their members, chain after chain (chain c of the query takes the next d_chains[c].n_seeds), at d_members[d_member_off[q]
 * ...), and never a slot at or beyond the next query's offset (d_n_chains / d_n_members / d_status nullable there).  Each pass
 * computes the chains anew: nothing is kept between the calls.  A group of lanes owns a query -- a wave of 64, or 16 lanes when
 * lookback <= 16 (env AWRY_CHAIN_GROUP=64, read per call, takes the wave there too; the results are the same).  No
 * synchronisation except where the workspace for queries beyond the LDS tile (owned by the replica, per stream, at most 128 MiB)
 * grows, on first use. */
int awry_dev_chain_seeds(awry_index_t *idx, int slot, const uint64_t *d_seed_off, const awry_seed_t *d_seeds, uint64_t n,
                         uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score,
                         uint64_t *d_n_chains, uint64_t *d_n_members, const uint64_t *d_chain_off, const uint64_t *d_member_off,
                         awry_chain_t *d_chains, awry_seed_t *d_members, uint8_t *d_status, void *stream);
/* the same with a work census: d_tally[3] (u64, caller-zeroed) += {seeds chained (of the queries not abandoned), predecessor
 * pairs evaluated (sum over the seeds of min(sorted index, lookback)), chains reported}; one atomic per query and counter */
int awry_dev_chain_seeds_tally(awry_index_t *idx, int slot, const uint64_t *d_seed_off, const awry_seed_t *d_seeds, uint64_t n,
                               uint32_t max_seeds, uint32_t lookback, uint32_t max_gap, uint32_t max_skew, uint32_t min_score,
                               uint64_t *d_n_chains, uint64_t *d_n_members, const uint64_t *d_chain_off,
                               const uint64_t *d_member_off, awry_chain_t *d_chains, awry_seed_t *d_members, uint8_t *d_status,
                               uint64_t *d_tally, void *stream);
/* The device primitive under awry_align_chains_batch (the definition is stated there), for a caller with chains of their own:
 * chain c belongs to query d_chain_query[c] (u32) and has the members d_members[d_member_off[c] .. d_member_off[c+1]); the queries
 * are (d_qbytes, d_qoff), readable as for the other device entry points; m < 2^32.  The two-call protocol of awry_dev_smems:
 * d_cigar_off == NULL is the count pass -> d_alns[m] and d_n_ops[m] (u64, ready for awry_dev_scan_counts); otherwise the fill
 * pass writes the runs of chain c at d_cigar[d_cigar_off[c] ..) and never a slot at or beyond d_cigar_off[c+1] (d_alns / d_n_ops
 * are not written there and may be NULL).  Each pass computes the alignments anew.  One chain per lane; the chains are first
 * sorted into three classes by their widest segment (NB <= 9, 17, 33) and each class runs its own instantiation.  Queued on
 * `stream`; no synchronisation except where the per-stream scratch (class lists, and up to 512 MiB of direction words, sized by
 * the launch) grows. */
int awry_dev_align_chains(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff,
                          const uint32_t *d_chain_query, const uint64_t *d_member_off, const awry_seed_t *d_members, uint64_t m,
                          uint32_t band, awry_aln_t *d_alns, uint64_t *d_n_ops, const uint64_t *d_cigar_off, uint32_t *d_cigar,
                          void *stream);
/* the same with a work census: d_tally[2] (u64, caller-zeroed) += {chains aligned with status AWRY_ALN_OK, table cells computed
 * (the cells of every segment's rows 0..a inside band and table)}, per pass */
int awry_dev_align_chains_tally(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff,
                                const uint32_t *d_chain_query, const uint64_t *d_member_off, const awry_seed_t *d_members,
                                uint64_t m, uint32_t band, awry_aln_t *d_alns, uint64_t *d_n_ops, const uint64_t *d_cigar_off,
                                uint32_t *d_cigar, uint64_t *d_tally, void *stream);
/* The clipped mode of the two entry points above ("soft-clip read ends" states it): the same arguments and protocol plus the four
 * weights after band; d_alns holds awry_aln_clip_t records, and the runs may begin and end with an 'S' run.  The same kernels,
 * instantiated per mode; the classes are cut by the gaps' skew only (an extension needs 2 W + 1 cells).  The census counts the same
 * things; a clipped extension's rows beyond J + W have no cell and do not run. */
int awry_dev_align_chains_clip(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff,
                               const uint32_t *d_chain_query, const uint64_t *d_member_off, const awry_seed_t *d_members, uint64_t m,
                               uint32_t band, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus,
                               awry_aln_clip_t *d_alns, uint64_t *d_n_ops, const uint64_t *d_cigar_off, uint32_t *d_cigar,
                               void *stream);
int awry_dev_align_chains_clip_tally(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff,
                                     const uint32_t *d_chain_query, const uint64_t *d_member_off, const awry_seed_t *d_members,
                                     uint64_t m, uint32_t band, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus,
                                     awry_aln_clip_t *d_alns, uint64_t *d_n_ops, const uint64_t *d_cigar_off, uint32_t *d_cigar,
                                     uint64_t *d_tally, void *stream);
/* The doubled batch of awry_map_batch, device-resident: query 2i of the output is read i as given, query 2i + 1 is rc(read i) (the
 * definition is stated there); d_out_off[2i] = 2 (d_qoff[i] - d_qoff[0]), d_out_off[2i+1] = that + L_i, d_out_off[2n] = 2
 * (d_qoff[n] - d_qoff[0]).  The caller sizes d_out_bytes at 2 x the reads' bytes (plus what the consuming entry point wants
 * readable past the end) and d_out_off at 2 n + 1; nothing is written past either.  A group of 16 lanes owns a read; loads and
 * both stores are contiguous per group.  Nucleotide indexes only (amino => AWRY_ERR_ARG).  Queued on `stream`, no
 * synchronisation. */
int awry_dev_revcomp(awry_index_t *idx, int slot, const uint8_t *d_qbytes, const uint64_t *d_qoff, uint64_t n,
                     uint8_t *d_out_bytes, uint64_t *d_out_off, void *stream);
/* Rank, redundancy, report and MAPQ of awry_map_batch over a caller's alignment records of a doubled batch of n reads: the
 * alignments of query x (strand x & 1 of read x >> 1) are d_alns / d_chains [d_aln_off[x] .. d_aln_off[x+1]) -- d_aln_off has
 * 2 n + 1 entries, of each query the first min(count, chains_per_strand) are candidates, only d_chains[].score is read --
 * and d_chain_status[2n] (nullable) is the chaining status per query.  The two-call protocol of awry_dev_smems: d_map_off ==
 * NULL is the count pass -> d_n_maps[n] (u64, ready for awry_dev_scan_counts) and optional d_read_status[n]; otherwise the fill
 * pass writes the records of read i at d_maps[d_map_off[i] ..) and never a slot at or beyond d_map_off[i+1], and per record
 * (both nullable) d_sel[] = the index of its alignment in d_alns (u32) and d_pos[] = record and offset of t_begin.  One read
 * per lane; the candidates are ranked by repeated selection of the smallest key, so no array lives in registers.  Queued on
 * `stream`, no synchronisation. */
int awry_dev_map_select(awry_index_t *idx, int slot, const uint64_t *d_aln_off, const awry_aln_t *d_alns,
                        const awry_chain_t *d_chains, const uint8_t *d_chain_status, uint64_t n, uint32_t chains_per_strand,
                        uint32_t max_report, uint64_t *d_n_maps, uint8_t *d_read_status, const uint64_t *d_map_off,
                        awry_map_t *d_maps, uint32_t *d_sel, awry_pos_t *d_pos, void *stream);
/* The clipped mode of awry_dev_map_select ("soft-clip read ends", map level): the same arguments and protocol plus the five
 * scalars after max_report (all are checked; MAPQ divides by match + mismatch, min_aln_score is the threshold, gap and end_bonus
 * play no part in the selection); it reads awry_aln_clip_t and writes awry_map_clip_t records. */
int awry_dev_map_select_clip(awry_index_t *idx, int slot, const uint64_t *d_aln_off, const awry_aln_clip_t *d_alns,
                             const awry_chain_t *d_chains, const uint8_t *d_chain_status, uint64_t n, uint32_t chains_per_strand,
                             uint32_t max_report, uint32_t match, uint32_t mismatch, uint32_t gap, uint32_t end_bonus,
                             uint32_t min_aln_score, uint64_t *d_n_maps, uint8_t *d_read_status, const uint64_t *d_map_off,
                             awry_map_clip_t *d_maps, uint32_t *d_sel, awry_pos_t *d_pos, void *stream);
/* The walk, report and MAPQ of awry_map_split_batch ("split reads") over a caller's clipped alignment records: the arguments and the
 * two-call protocol of awry_dev_map_select_clip, with d_qoff -- the reads' own n + 1 offsets, of which only the lengths are read --
 * after d_chain_status, max_segments, max_secondary, max_overlap in the place of max_report, and of the scalars match, mismatch (MAPQ
 * divides by their sum) and min_aln_score (the threshold); all are checked.  It writes awry_map_split_t records.  One read per lane:
 * a first pass classifies the kept candidates (the kept slots in rank order and their segments are two 64-bit words of sixteen
 * 4-bit entries), a second emits, so that the secondaries land behind however many segments there are.  Queued on `stream`, no
 * synchronisation. */
int awry_dev_map_select_split(awry_index_t *idx, int slot, const uint64_t *d_aln_off, const awry_aln_clip_t *d_alns,
                              const awry_chain_t *d_chains, const uint8_t *d_chain_status, const uint64_t *d_qoff, uint64_t n,
                              uint32_t chains_per_strand, uint32_t max_segments, uint32_t max_secondary, uint32_t max_overlap,
                              uint32_t match, uint32_t mismatch, uint32_t min_aln_score, uint64_t *d_n_maps, uint8_t *d_read_status,
                              const uint64_t *d_map_off, awry_map_split_t *d_maps, uint32_t *d_sel, awry_pos_t *d_pos, void *stream);
/* The rescue windows of awry_map_pairs_batch over a caller's kept lists: the candidates of read i (mate i & 1 of pair i >> 1) are
 * d_cands[d_cand_off[i] .. d_cand_off[i+1]) in rank order, d_cand_off and d_qoff (the reads' own offsets: only the lengths are read)
 * have 2 n_pairs + 1 entries.  Output at a fixed stride: slot w = (2p + m) G + a, G = rescue_anchors, is candidate a of mate m.  An
 * anchor's slot gets d_win_query[w] = 4p + 2 (1 - m) + (1 - strand) (u32, the doubled-batch index of what it seeks), d_win_first[w]
 * (u64) and d_win_count[w] (u32) = its window of starts after the cuts; a slot that is no anchor gets query 4p + 2 (1 - m), and it
 * and an anchor with an empty window get first = 0, count = 0.  Nothing is written past 2 G n_pairs slots.  n_pairs < 2^28.  One
 * slot per lane.  Queued on `stream`, no synchronisation. */
int awry_dev_pair_windows(awry_index_t *idx, int slot, const uint64_t *d_cand_off, const awry_map_t *d_cands, const uint64_t *d_qoff,
                          uint64_t n_pairs, uint64_t min_insert, uint64_t max_insert, uint32_t rescue_anchors, int rescue_edits,
                          uint32_t *d_win_query, uint64_t *d_win_first, uint32_t *d_win_count, void *stream);
/* Append and redundancy rule, pair order, MAPQ, flags and insert of awry_map_pairs_batch, a pure function of its arrays: the kept
 * lists as above, d_resc[2 G n_pairs] = slot w's rescued candidate or edits == 0xFFFFFFFF for none (not read when rescue_anchors ==
 * 0), d_read_status[2 n_pairs] (nullable).  The two-call protocol of awry_dev_map_select: d_map_off == NULL is the count pass ->
 * d_n_maps[2 n_pairs]; otherwise the fill pass writes read i's record at d_maps[d_map_off[i]] and never a slot at or beyond
 * d_map_off[i+1], per record (both nullable) d_sel[] (u32: the index into d_cands, or 0x80000000 | w for a rescued record) and
 * d_pos[], and d_insert[n_pairs] (u32, nullable).  One pair per lane; best and second pair are tracked by re-reading the records, so
 * no array lives in registers.  Queued on `stream`, no synchronisation. */
int awry_dev_pair_select(awry_index_t *idx, int slot, const uint64_t *d_cand_off, const awry_map_t *d_cands, const awry_map_t *d_resc,
                         const uint8_t *d_read_status, uint64_t n_pairs, uint64_t min_insert, uint64_t max_insert,
                         uint32_t unpaired_penalty, uint32_t rescue_anchors, uint64_t *d_n_maps, const uint64_t *d_map_off,
                         awry_map_t *d_maps, uint32_t *d_sel, awry_pos_t *d_pos, uint32_t *d_insert, void *stream);
/* The clipped modes of awry_dev_pair_windows and awry_dev_pair_select ("map read pairs, clipped"): the same arguments and protocol
 * over awry_map_clip_t, d_resc included (a slot without a candidate: edits == 0xFFFFFFFF).  The windows are measured from fb and ve;
 * the select takes unpaired_penalty in score units and the five clip scalars after rescue_anchors (all are checked; MAPQ divides by
 * match + mismatch; the others play no part in the choice: the rescued records come with their scores). */
int awry_dev_pair_windows_clip(awry_index_t *idx, int slot, const uint64_t *d_cand_off, const awry_map_clip_t *d_cands,
                               const uint64_t *d_qoff, uint64_t n_pairs, uint64_t min_insert, uint64_t max_insert,
                               uint32_t rescue_anchors, int rescue_edits, uint32_t *d_win_query, uint64_t *d_win_first,
                               uint32_t *d_win_count, void *stream);
int awry_dev_pair_select_clip(awry_index_t *idx, int slot, const uint64_t *d_cand_off, const awry_map_clip_t *d_cands,
                              const awry_map_clip_t *d_resc, const uint8_t *d_read_status, uint64_t n_pairs, uint64_t min_insert,
                              uint64_t max_insert, uint32_t unpaired_penalty, uint32_t rescue_anchors, uint32_t match,
                              uint32_t mismatch, uint32_t gap, uint32_t end_bonus, uint32_t min_aln_score, uint64_t *d_n_maps,
                              const uint64_t *d_map_off, awry_map_clip_t *d_maps, uint32_t *d_sel, awry_pos_t *d_pos,
                              uint32_t *d_insert, void *stream);
/* test hook of the all-symbol rank primitive: d_occ[i * S + s - 1] = Occ(s, d_rows[i]) for every non-sentinel symbol index s
 * (S = 5 nucleotide, 21 amino; inclusive of the row, as awry_update_range uses it); rows >= bwt_len give zeros */
int awry_debug_rank_all(awry_index_t *idx, int slot, const void *d_rows, uint64_t n, void *d_occ, void *stream);
/* exclusive scan of counts[n] -> hit_off[n+1] (d_scratch: awry_dev_scan_scratch_bytes(n) bytes) */
uint64_t awry_dev_scan_scratch_bytes(uint64_t n);
int awry_dev_scan_counts(awry_index_t *idx, int slot, const void *d_counts, uint64_t n, void *d_hit_off,
                         void *d_scratch, void *stream);
/* backtrace `total` hits: d_ranges[q * range_stride] = first row of query q's range (stride 2 = the (start,end)
 * pairs of awry_dev_count_ascii, stride 1 = the starts of awry_dev_count_nt2_long), hit_off[n+1] ->
 * global_pos[total], pos[total] (nullable) */
int awry_dev_locate(awry_index_t *idx, int slot, const void *d_ranges, int range_stride, const void *d_hit_off, uint64_t n,
                    uint64_t total, void *d_global_pos, void *d_pos, void *stream);
/* awry_dev_locate with the walk kernel's census: d_tally[2] (u64, caller-zeroed) += {LF steps taken by the walks, hits
 * that had to walk} -- what SURVEY.md 8(d) prices at 104 B per backstep.  Nucleotide indexes. */
int awry_dev_locate_tally(awry_index_t *idx, int slot, const void *d_ranges, int range_stride, const void *d_hit_off, uint64_t n,
                          uint64_t total, void *d_global_pos, void *d_pos, void *d_tally, void *stream);
/* profiling aid: queues an empty kernel (phase_marker_kernel) of phase_id blocks of 64 threads on `stream`.  rocprofv3
 * counter passes report the grid size of every dispatch, so a run can be cut into named phases without marker tracing. */
int awry_dev_phase_marker(awry_index_t *idx, int slot, int phase_id, void *stream);
/* packed reads of any length: W = ceil(L/32) u64 words per query (letter j in word j/32, bits 2(j%32), as written by
 * awry_dev_pack_nt2); counts[n] and, if non-null, range_start[n] (first BWT row of each range) for awry_dev_locate */
int awry_dev_count_nt2_long(awry_index_t *idx, int slot, const void *d_words, uint64_t n, int L, void *d_counts,
                            void *d_range_start, int use_seed, void *stream);
/* plumbing for callers without a HIP binding of their own */
int awry_dev_malloc(awry_index_t *idx, int slot, uint64_t bytes, void **d_out);
int awry_dev_free(awry_index_t *idx, int slot, void *d);
int awry_dev_memcpy_h2d(awry_index_t *idx, int slot, void *d_dst, const void *h_src, uint64_t bytes);
int awry_dev_memcpy_d2h(awry_index_t *idx, int slot, void *h_dst, const void *d_src, uint64_t bytes);
int awry_dev_memset(awry_index_t *idx, int slot, void *d_dst, int value, uint64_t bytes);
int awry_dev_synchronize(awry_index_t *idx, int slot);
/* measurement aid: copies `bytes` (multiple of 16) from d_src to d_dst with 16-byte loads and stores per lane on `stream` --
 * the streaming rate printed next to the nominal HBM peak */
int awry_dev_stream_copy(awry_index_t *idx, int slot, void *d_dst, const void *d_src, uint64_t bytes, void *stream);
/* time a region on `stream` with HIP events: begin/end record, elapsed synchronises and returns ms */
int awry_dev_timer_begin(awry_index_t *idx, int slot, void *stream);
int awry_dev_timer_end(awry_index_t *idx, int slot, void *stream, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* AWRY_HIP_H */
