// awry.hpp -- header-only C++ host-side mirror of the reference's `FmIndex` surface
// (/root/reference src/fm_index.rs:41-119,142,302-399,455-544) over the C ABI of libawry_hip.so.
// Same names and argument meaning; where the reference panics the calls throw awry::Error.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "awry_hip.h"

namespace awry {

enum class SymbolAlphabet : uint8_t { Nucleotide = AWRY_NUCLEOTIDE, Amino = AWRY_AMINO };  // src/alphabet.rs:28-31

struct Error : std::runtime_error {
  int code;
  Error(int c, const char* msg) : std::runtime_error(msg ? msg : "awry error"), code(c) {}
};
inline void check(int rc) { if (rc != AWRY_OK) throw Error(rc, awry_last_error()); }

struct FmBuildArgs {  // src/fm_index.rs:78-96
  std::string input_file_src;
  std::string suffix_array_output_src;            // Option<PathBuf>: empty = None
  uint64_t suffix_array_compression_ratio = 0;    // Option<u64>: 0 = None (=> 8)
  uint8_t lookup_table_kmer_len = 0;              // Option<u8>: 0 = None (=> 10 / 4)
  SymbolAlphabet alphabet = SymbolAlphabet::Nucleotide;
  uint64_t max_query_len = 0;                     // Option<usize>: 0 = None
  bool remove_intermediate_suffix_array_file = false;
};

struct LocalizedSequencePosition {  // src/sequence_index.rs:31-78
  uint64_t sequence_idx_, local_position_;
  uint64_t sequence_idx() const { return sequence_idx_; }
  uint64_t local_position() const { return local_position_; }
  bool operator<(const LocalizedSequencePosition& o) const {
    return sequence_idx_ != o.sequence_idx_ ? sequence_idx_ < o.sequence_idx_ : local_position_ < o.local_position_;
  }
  bool operator==(const LocalizedSequencePosition& o) const { return sequence_idx_ == o.sequence_idx_ && local_position_ == o.local_position_; }
};

struct SearchRange {  // src/search.rs:25-81
  uint64_t start_ptr = 1, end_ptr = 0;
  static SearchRange zero() { return {}; }
  bool is_empty() const { return start_ptr > end_ptr; }
  uint64_t len() const { return is_empty() ? 0 : end_ptr - start_ptr + 1; }
};

class FmIndex {
 public:
  // FmIndex::new, src/fm_index.rs:142.  `devices`: GPUs that receive a replica (queries need at least one).
  static FmIndex create(const FmBuildArgs& a, const std::vector<int>& devices = {0}) {
    awry_build_args_t c{};
    c.input_path = a.input_file_src.c_str();
    c.sa_tmp_path = a.suffix_array_output_src.empty() ? nullptr : a.suffix_array_output_src.c_str();
    c.sa_ratio = a.suffix_array_compression_ratio;
    c.kmer_len = a.lookup_table_kmer_len;
    c.alphabet = static_cast<uint8_t>(a.alphabet);
    c.max_query_len = a.max_query_len;
    c.remove_tmp = a.remove_intermediate_suffix_array_file;
    awry_index_t* h = nullptr;
    check(awry_build(&c, &h));
    FmIndex ix(h);
    ix.set_devices(devices);
    return ix;
  }
  // FmIndex::load, src/fm_index_file.rs:132
  static FmIndex load(const std::string& path, const std::vector<int>& devices = {0}) {
    awry_index_t* h = nullptr;
    check(awry_load(path.c_str(), &h));
    FmIndex ix(h);
    ix.set_devices(devices);
    return ix;
  }
  void save(const std::string& path) { check(awry_save(h_, path.c_str())); }  // src/fm_index_file.rs:42

  FmIndex(FmIndex&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  FmIndex& operator=(FmIndex&& o) noexcept { if (this != &o) { awry_free(h_); h_ = o.h_; o.h_ = nullptr; } return *this; }
  FmIndex(const FmIndex&) = delete;
  FmIndex& operator=(const FmIndex&) = delete;
  ~FmIndex() { awry_free(h_); }

  void set_devices(const std::vector<int>& ids) { if (!ids.empty()) check(awry_set_devices(h_, ids.data(), (int)ids.size())); }

  // accessors, src/fm_index.rs:302-399
  SymbolAlphabet alphabet() const { return static_cast<SymbolAlphabet>(awry_alphabet(h_)); }
  uint64_t suffix_array_compression_ratio() const { return awry_sa_ratio(h_); }
  uint64_t bwt_len() const { return awry_bwt_len(h_); }
  uint64_t version_number() const { return awry_version(h_); }
  std::vector<uint64_t> prefix_sums() const {
    uint64_t n = 0;
    const uint64_t* p = awry_prefix_sums(h_, &n);
    return std::vector<uint64_t>(p, p + n);
  }
  SearchRange initial_search_range(char symbol) const {
    awry_range_t r;
    check(awry_initial_range(h_, (uint8_t)symbol, &r));
    return {r.start_ptr, r.end_ptr};
  }

  // src/fm_index.rs:499, 516
  uint64_t count_string(std::string_view q) {
    uint64_t c = 0;
    check(awry_count(h_, (const uint8_t*)q.data(), q.size(), &c));
    return c;
  }
  std::vector<LocalizedSequencePosition> locate_string(std::string_view q) {
    awry_pos_t* hits = nullptr;
    uint64_t n = 0;
    check(awry_locate(h_, (const uint8_t*)q.data(), q.size(), &hits, nullptr, &n));
    std::vector<LocalizedSequencePosition> out(n);
    for (uint64_t i = 0; i < n; i++) out[i] = {hits[i].seq_idx, hits[i].local_pos};
    awry_free_buffer(hits);
    return out;
  }
  // src/fm_index.rs:455-460, 479-487 (results in input order; inner order = ascending BWT row)
  template <class StrRange>
  std::vector<uint64_t> parallel_count(const StrRange& queries) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    std::vector<uint64_t> out(off.size() - 1);
    check(awry_count_batch(h_, bytes.data(), off.data(), out.size(), out.data()));
    return out;
  }
  // no counterpart in the reference: k-mers already packed 2 bits per letter (awry_count_packed_kmers)
  std::vector<uint64_t> parallel_count_packed(const std::vector<uint64_t>& words, int L) {
    std::vector<uint64_t> out(words.size());
    check(awry_count_packed_kmers(h_, words.data(), words.size(), L, out.data()));
    return out;
  }
  template <class StrRange>
  std::vector<std::vector<LocalizedSequencePosition>> parallel_locate(const StrRange& queries) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* hoff = nullptr; awry_pos_t* hits = nullptr;
    check(awry_locate_batch(h_, bytes.data(), off.data(), n, &hoff, &hits, nullptr));
    std::vector<std::vector<LocalizedSequencePosition>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = hoff[i]; j < hoff[i + 1]; j++) out[i].push_back({hits[j].seq_idx, hits[j].local_pos});
    awry_free_buffer(hoff); awry_free_buffer(hits);
    return out;
  }
  // substitution-tolerant search (no counterpart in the reference; semantics in awry_hip.h): counts[i * (k + 1) + d] =
  // occurrences of query i at exactly d substitutions
  template <class StrRange>
  std::vector<uint64_t> parallel_count_mismatch(const StrRange& queries, int k) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    std::vector<uint64_t> out((off.size() - 1) * (size_t)(k >= 0 ? k + 1 : 1));
    check(awry_count_mismatch_batch(h_, bytes.data(), off.data(), off.size() - 1, k, out.data()));
    return out;
  }
  struct MismatchHit {
    LocalizedSequencePosition position;
    uint8_t mismatches;
  };
  // hits of each query in ascending BWT-row order, with their distances
  template <class StrRange>
  std::vector<std::vector<MismatchHit>> parallel_locate_mismatch(const StrRange& queries, int k) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* hoff = nullptr; awry_pos_t* hits = nullptr; uint8_t* mm = nullptr;
    check(awry_locate_mismatch_batch(h_, bytes.data(), off.data(), n, k, &hoff, &hits, nullptr, &mm));
    std::vector<std::vector<MismatchHit>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = hoff[i]; j < hoff[i + 1]; j++) out[i].push_back({{hits[j].seq_idx, hits[j].local_pos}, mm[j]});
    awry_free_buffer(hoff); awry_free_buffer(hits); awry_free_buffer(mm);
    return out;
  }
  // locate within k edits (no counterpart in the reference; the definition is in awry_hip.h): per query, the starts whose best
  // alignment has at most k substitutions, insertions and deletions and is not beaten by a neighbouring start, in ascending
  // text position.  A query whose k + 1 pieces occur more than max_candidates times in all is abandoned: no hits, and
  // (*status)[i] == AWRY_Q_CANDIDATE_CAP where the caller asks for the status bytes.
  struct EditHit {
    LocalizedSequencePosition position;
    uint64_t global_position;
    uint8_t edits;
  };
  template <class StrRange>
  std::vector<std::vector<EditHit>> parallel_locate_edit(const StrRange& queries, int k, uint64_t max_candidates, std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* hoff = nullptr; awry_pos_t* hits = nullptr; uint64_t* gp = nullptr; uint8_t* ed = nullptr; uint8_t* st = nullptr;
    check(awry_locate_edit_batch(h_, bytes.data(), off.data(), n, k, max_candidates, &hoff, &hits, &gp, &ed, &st));
    std::vector<std::vector<EditHit>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = hoff[i]; j < hoff[i + 1]; j++) out[i].push_back({{hits[j].seq_idx, hits[j].local_pos}, gp[j], ed[j]});
    if (status) status->assign(st, st + n);
    awry_free_buffer(hoff); awry_free_buffer(hits); awry_free_buffer(gp); awry_free_buffer(ed); awry_free_buffer(st);
    return out;
  }
  // runs (len << 4 | BAM op: I 1, D 2, S 4, = 7, X 8) -> "57=1X43="
  static std::string cigar_text(const std::vector<uint32_t>& runs) {
    std::string out;
    for (uint32_t run : runs) {
      const uint32_t op = run & 15u;
      out += std::to_string(run >> 4);
      out += op == 7 ? '=' : op == 8 ? 'X' : op == 1 ? 'I' : op == 4 ? 'S' : 'D';
    }
    return out;
  }
  // the same hits aligned (awry_hip.h states the canonical script): the length of the text span each matches and its CIGAR,
  // one run per entry, len << 4 | BAM op (I 1, D 2, = 7, X 8)
  struct EditAlignment {
    LocalizedSequencePosition position;
    uint64_t global_position;
    uint8_t edits;
    uint32_t text_len;
    std::vector<uint32_t> cigar;
    std::string cigar_string() const { return cigar_text(cigar); }
  };
  template <class StrRange>
  std::vector<std::vector<EditAlignment>> parallel_align_edit(const StrRange& queries, int k, uint64_t max_candidates,
                                                              std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* hoff = nullptr; awry_pos_t* hits = nullptr; uint64_t* gp = nullptr; uint8_t* ed = nullptr; uint8_t* st = nullptr;
    uint32_t* tl = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr;
    check(awry_align_edit_batch(h_, bytes.data(), off.data(), n, k, max_candidates, &hoff, &hits, &gp, &ed, &st, &tl, &coff, &cg));
    std::vector<std::vector<EditAlignment>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = hoff[i]; j < hoff[i + 1]; j++)
        out[i].push_back({{hits[j].seq_idx, hits[j].local_pos}, gp[j], ed[j], tl[j], std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
    if (status) status->assign(st, st + n);
    awry_free_buffer(hoff); awry_free_buffer(hits); awry_free_buffer(gp); awry_free_buffer(ed); awry_free_buffer(st);
    awry_free_buffer(tl); awry_free_buffer(coff); awry_free_buffer(cg);
    return out;
  }
  // class patterns (no counterpart in the reference; the definition and the limits are in awry_hip.h): IUPAC / residue-class
  // letters with up to k mismatches.  counts[i * (k + 1) + d] = occurrences of pattern i at exactly d mismatches
  template <class StrRange>
  std::vector<uint64_t> parallel_count_pattern(const StrRange& patterns, int k = 0) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(patterns, bytes, off);
    std::vector<uint64_t> out((off.size() - 1) * (size_t)(k >= 0 ? k + 1 : 1));
    check(awry_count_pattern_batch(h_, bytes.data(), off.data(), off.size() - 1, k, out.data()));
    return out;
  }
  // hits of each pattern in ascending BWT-row order (the matched strings in symbol-index order), with their distances
  template <class StrRange>
  std::vector<std::vector<MismatchHit>> parallel_locate_pattern(const StrRange& patterns, int k = 0) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(patterns, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* hoff = nullptr; awry_pos_t* hits = nullptr; uint8_t* mm = nullptr;
    check(awry_locate_pattern_batch(h_, bytes.data(), off.data(), n, k, &hoff, &hits, nullptr, &mm));
    std::vector<std::vector<MismatchHit>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = hoff[i]; j < hoff[i + 1]; j++) out[i].push_back({{hits[j].seq_idx, hits[j].local_pos}, mm[j]});
    awry_free_buffer(hoff); awry_free_buffer(hits); awry_free_buffer(mm);
    return out;
  }
  // class mask of a pattern letter: bit s = symbol index s belongs to the class, 0 = not a class letter (needs no GPU)
  static uint32_t pattern_class(int alphabet, char letter) { return awry_pattern_class(alphabet, (uint8_t)letter); }
  // anchors (no counterpart in the reference; the definition is in awry_hip.h): the greedy longest-match factorisation of
  // every query, found right to left -- q[q_begin .. q_begin + q_len) occupies the BWT rows `rows`
  struct Anchor {
    uint32_t q_begin, q_len;
    SearchRange rows;
  };
  template <class StrRange>
  std::vector<std::vector<Anchor>> parallel_anchors(const StrRange& queries, uint32_t min_len = 1, bool skip_failed_letter = false) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* aoff = nullptr; awry_anchor_t* an = nullptr;
    check(awry_anchor_batch(h_, bytes.data(), off.data(), n, min_len, skip_failed_letter ? 1 : 0, &aoff, &an));
    std::vector<std::vector<Anchor>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = aoff[i]; j < aoff[i + 1]; j++) out[i].push_back({an[j].q_begin, an[j].q_len, {an[j].start_row, an[j].start_row + an[j].count - 1}});
    awry_free_buffer(aoff); awry_free_buffer(an);
    return out;
  }
  // the same with every anchor of at most max_hits (>= 1) occurrences located, in ascending BWT-row order; larger ones keep
  // their record and an empty list
  struct LocatedAnchor {
    Anchor anchor;
    std::vector<LocalizedSequencePosition> hits;
  };
  template <class StrRange>
  std::vector<std::vector<LocatedAnchor>> parallel_locate_anchors(const StrRange& queries, uint64_t max_hits, uint32_t min_len = 1,
                                                                  bool skip_failed_letter = false) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* aoff = nullptr; awry_anchor_t* an = nullptr; uint64_t* hoff = nullptr; awry_pos_t* hits = nullptr;
    check(awry_locate_anchors_batch(h_, bytes.data(), off.data(), n, min_len, skip_failed_letter ? 1 : 0, max_hits, &aoff, &an, &hoff, &hits, nullptr));
    std::vector<std::vector<LocatedAnchor>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = aoff[i]; j < aoff[i + 1]; j++) {
        LocatedAnchor la{{an[j].q_begin, an[j].q_len, {an[j].start_row, an[j].start_row + an[j].count - 1}}, {}};
        for (uint64_t h = hoff[j]; h < hoff[j + 1]; h++) la.hits.push_back({hits[h].seq_idx, hits[h].local_pos});
        out[i].push_back(std::move(la));
      }
    awry_free_buffer(aoff); awry_free_buffer(an); awry_free_buffer(hoff); awry_free_buffer(hits);
    return out;
  }
  // SMEMs (no counterpart in the reference; the definition is in awry_hip.h): every super-maximal exact match of every query
  // of at least min_len letters, in descending q_begin -- the same record as an anchor
  template <class StrRange>
  std::vector<std::vector<Anchor>> parallel_smems(const StrRange& queries, uint32_t min_len = 1) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* soff = nullptr; awry_anchor_t* sm = nullptr;
    check(awry_smem_batch(h_, bytes.data(), off.data(), n, min_len, &soff, &sm));
    std::vector<std::vector<Anchor>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = soff[i]; j < soff[i + 1]; j++) out[i].push_back({sm[j].q_begin, sm[j].q_len, {sm[j].start_row, sm[j].start_row + sm[j].count - 1}});
    awry_free_buffer(soff); awry_free_buffer(sm);
    return out;
  }
  // the same with every SMEM of at most max_hits (>= 1) occurrences located, in ascending BWT-row order
  template <class StrRange>
  std::vector<std::vector<LocatedAnchor>> parallel_locate_smems(const StrRange& queries, uint64_t max_hits, uint32_t min_len = 1) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* soff = nullptr; awry_anchor_t* sm = nullptr; uint64_t* hoff = nullptr; awry_pos_t* hits = nullptr;
    check(awry_locate_smems_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, &soff, &sm, &hoff, &hits, nullptr));
    std::vector<std::vector<LocatedAnchor>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = soff[i]; j < soff[i + 1]; j++) {
        LocatedAnchor la{{sm[j].q_begin, sm[j].q_len, {sm[j].start_row, sm[j].start_row + sm[j].count - 1}}, {}};
        for (uint64_t h = hoff[j]; h < hoff[j + 1]; h++) la.hits.push_back({hits[h].seq_idx, hits[h].local_pos});
        out[i].push_back(std::move(la));
      }
    awry_free_buffer(soff); awry_free_buffer(sm); awry_free_buffer(hoff); awry_free_buffer(hits);
    return out;
  }
  // colinear chaining of the located SMEM seeds (no counterpart in the reference; the definition is in awry_hip.h): per query, its
  // chains, the primary chain first -- a score, the spans it covers in query and text, and its seeds first to last.  A query of
  // more than p.max_seeds seeds is abandoned: no chains, and (*status)[i] == AWRY_Q_SEED_CAP where the caller asks for the status bytes.
  struct ChainParams {
    uint32_t max_seeds = 1024, lookback = 32, max_gap = 1000, max_skew = 100, min_score = 20;
  };
  struct Chain {
    uint32_t score, q_begin, q_end;
    uint64_t t_begin, t_end;
    std::vector<awry_seed_t> seeds;
  };
  template <class StrRange>
  std::vector<std::vector<Chain>> parallel_chains(const StrRange& queries, uint32_t min_len = 12, uint64_t max_hits = 50, ChainParams p = ChainParams(),
                                                  std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* coff = nullptr; awry_chain_t* ch = nullptr; uint64_t* soff = nullptr; awry_seed_t* sd = nullptr; uint8_t* st = nullptr;
    check(awry_chain_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score, &coff, &ch,
                           &soff, &sd, &st));
    std::vector<std::vector<Chain>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = coff[i]; j < coff[i + 1]; j++)
        out[i].push_back({ch[j].score, ch[j].q_begin, ch[j].q_end, ch[j].t_begin, ch[j].t_end, std::vector<awry_seed_t>(sd + soff[j], sd + soff[j + 1])});
    if (status) status->assign(st, st + n);
    awry_free_buffer(coff); awry_free_buffer(ch); awry_free_buffer(soff); awry_free_buffer(sd); awry_free_buffer(st);
    return out;
  }
  // the chains aligned (no counterpart in the reference; the definition is in awry_hip.h): of every query's chains the first
  // max_alignments, the primary first -- the chain's score and spans, the text span the whole read aligns to, the edit count, a
  // status (AWRY_ALN_OK, AWRY_ALN_SKEW, AWRY_ALN_BAD_CHAIN) and the CIGAR, one run per entry, len << 4 | BAM op (I 1, D 2, = 7, X 8)
  struct ChainAlignment {
    awry_chain_t chain;
    uint64_t t_begin, t_end;
    uint32_t edits, status;
    std::vector<uint32_t> cigar;
    std::string cigar_string() const { return cigar_text(cigar); }
  };
  template <class StrRange>
  std::vector<std::vector<ChainAlignment>> parallel_align_chains(const StrRange& queries, uint32_t min_len = 12, uint64_t max_hits = 50,
                                                                 uint64_t max_alignments = 1, uint32_t band = 4, ChainParams p = ChainParams(),
                                                                 std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* aoff = nullptr; awry_chain_t* ch = nullptr; awry_aln_t* al = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr; uint8_t* st = nullptr;
    check(awry_align_chains_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score,
                                  max_alignments, band, &aoff, &ch, &al, &coff, &cg, &st));
    std::vector<std::vector<ChainAlignment>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = aoff[i]; j < aoff[i + 1]; j++)
        out[i].push_back({ch[j], al[j].t_begin, al[j].t_end, al[j].edits, al[j].status, std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
    if (status) status->assign(st, st + n);
    awry_free_buffer(aoff); awry_free_buffer(ch); awry_free_buffer(al); awry_free_buffer(coff); awry_free_buffer(cg); awry_free_buffer(st);
    return out;
  }
  // reads mapped on both strands (no counterpart in the reference; the definition is in awry_hip.h): per read its best alignments
  // over the read as given (strand 0) and its reverse complement (strand 1), the primary first -- where t_begin lies (record and
  // offset), the text span, the edit count, the chain it came from, a mapping quality (0 for the records after the first, which
  // carry AWRY_MAP_SECONDARY in flags) and the CIGAR of the aligned strand against the forward text.  A read that maps nowhere has
  // no records.
  struct Mapping {
    awry_pos_t pos;
    uint64_t t_begin, t_end;
    uint32_t edits, chain_score, chain_index;
    uint8_t strand, mapq;
    uint16_t flags;
    std::vector<uint32_t> cigar;
    std::string cigar_string() const { return cigar_text(cigar); }
  };
  template <class StrRange>
  std::vector<std::vector<Mapping>> parallel_map(const StrRange& queries, uint32_t min_len = 12, uint64_t max_hits = 50, uint64_t chains_per_strand = 4,
                                                 uint64_t max_report = 1, uint32_t band = 4, ChainParams p = ChainParams(),
                                                 std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* moff = nullptr; awry_map_t* mp = nullptr; awry_pos_t* ps = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr; uint8_t* st = nullptr;
    check(awry_map_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score,
                         chains_per_strand, max_report, band, &moff, &mp, &ps, &coff, &cg, &st));
    std::vector<std::vector<Mapping>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = moff[i]; j < moff[i + 1]; j++)
        out[i].push_back({ps[j], mp[j].t_begin, mp[j].t_end, mp[j].edits, mp[j].chain_score, mp[j].chain_index, mp[j].strand, mp[j].mapq, mp[j].flags,
                          std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
    if (status) status->assign(st, st + n);
    awry_free_buffer(moff); awry_free_buffer(mp); awry_free_buffer(ps); awry_free_buffer(coff); awry_free_buffer(cg); awry_free_buffer(st);
    return out;
  }
  // The clipped mode of the two calls above (the definition is in awry_hip.h, "soft-clip read ends"): the end extensions are scored
  // and local, what they leave out is soft-clipped ('S' runs, BAM op 4), and no extension reaches into another record.  t_begin /
  // t_end span the aligned part; score = match #'=' - mismatch #'X' - gap (#'I' + #'D').  In parallel_map_clip a candidate needs
  // score >= min_aln_score, the rank is by score first, and a chimeric read comes out as a primary and a secondary (max_report >= 2).
  struct ClipParams {
    uint32_t match = 1, mismatch = 4, gap = 6, end_bonus = 5, min_aln_score = 0;
  };
  struct ClippedChainAlignment {
    awry_chain_t chain;
    awry_aln_clip_t aln;
    std::vector<uint32_t> cigar;
    std::string cigar_string() const { return cigar_text(cigar); }
  };
  template <class StrRange>
  std::vector<std::vector<ClippedChainAlignment>> parallel_align_chains_clip(const StrRange& queries, uint32_t min_len = 12, uint64_t max_hits = 50,
                                                                             uint64_t max_alignments = 1, uint32_t band = 4, ClipParams c = ClipParams(),
                                                                             ChainParams p = ChainParams(), std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* aoff = nullptr; awry_chain_t* ch = nullptr; awry_aln_clip_t* al = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr; uint8_t* st = nullptr;
    check(awry_align_chains_clip_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score,
                                       max_alignments, band, c.match, c.mismatch, c.gap, c.end_bonus, &aoff, &ch, &al, &coff, &cg, &st));
    std::vector<std::vector<ClippedChainAlignment>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = aoff[i]; j < aoff[i + 1]; j++) out[i].push_back({ch[j], al[j], std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
    if (status) status->assign(st, st + n);
    awry_free_buffer(aoff); awry_free_buffer(ch); awry_free_buffer(al); awry_free_buffer(coff); awry_free_buffer(cg); awry_free_buffer(st);
    return out;
  }
  struct ClippedMapping {
    awry_pos_t pos;
    awry_map_clip_t map;
    std::vector<uint32_t> cigar;
    std::string cigar_string() const { return cigar_text(cigar); }
  };
  template <class StrRange>
  std::vector<std::vector<ClippedMapping>> parallel_map_clip(const StrRange& queries, uint32_t min_len = 12, uint64_t max_hits = 50,
                                                             uint64_t chains_per_strand = 4, uint64_t max_report = 1, uint32_t band = 4,
                                                             ClipParams c = ClipParams(), ChainParams p = ChainParams(),
                                                             std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* moff = nullptr; awry_map_clip_t* mp = nullptr; awry_pos_t* ps = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr; uint8_t* st = nullptr;
    check(awry_map_clip_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score,
                              chains_per_strand, max_report, band, c.match, c.mismatch, c.gap, c.end_bonus, c.min_aln_score, &moff, &mp, &ps, &coff, &cg,
                              &st));
    std::vector<std::vector<ClippedMapping>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = moff[i]; j < moff[i + 1]; j++) out[i].push_back({ps[j], mp[j], std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
    if (status) status->assign(st, st + n);
    awry_free_buffer(moff); awry_free_buffer(mp); awry_free_buffer(ps); awry_free_buffer(coff); awry_free_buffer(cg); awry_free_buffer(st);
    return out;
  }
  template <class Str>
  std::vector<ClippedMapping> map_clip_string(const Str& query, uint32_t min_len = 12, uint64_t max_hits = 50, uint64_t chains_per_strand = 4,
                                              uint64_t max_report = 1, uint32_t band = 4, ClipParams c = ClipParams(), ChainParams p = ChainParams()) {
    return parallel_map_clip(std::vector<std::string_view>{std::string_view(query)}, min_len, max_hits, chains_per_strand, max_report, band, c, p)[0];
  }
  // Split reads (no counterpart in the reference; the definition is in awry_hip.h, "split reads"): parallel_map_clip with the kept
  // candidates sorted by the part of the read they explain.  Per read first its segments -- up to max_segments clipped alignments over
  // different letters [q_begin, q_end) of the read, the primary and then the supplementaries (AWRY_MAP_SUPPLEMENTARY), each with a
  // mapping quality of its own -- then up to max_secondary secondaries, each overlapping the segment map.parent (an index among the
  // read's records) by at least max_overlap percent of the shorter interval.
  struct SplitParams {
    uint64_t max_segments = 2, max_secondary = 0;
    uint32_t max_overlap = 50;
  };
  struct SplitMapping {
    awry_pos_t pos;
    awry_map_split_t map;
    std::vector<uint32_t> cigar;
    std::string cigar_string() const { return cigar_text(cigar); }
    bool secondary() const { return (map.flags & AWRY_MAP_SECONDARY) != 0; }
    bool supplementary() const { return (map.flags & AWRY_MAP_SUPPLEMENTARY) != 0; }
  };
  template <class StrRange>
  std::vector<std::vector<SplitMapping>> parallel_map_split(const StrRange& queries, uint32_t min_len = 12, uint64_t max_hits = 50,
                                                            uint64_t chains_per_strand = 4, SplitParams sp = SplitParams(), uint32_t band = 4,
                                                            ClipParams c = ClipParams(), ChainParams p = ChainParams(),
                                                            std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(queries, bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* moff = nullptr; awry_map_split_t* mp = nullptr; awry_pos_t* ps = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr; uint8_t* st = nullptr;
    check(awry_map_split_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score,
                               chains_per_strand, sp.max_segments, sp.max_secondary, sp.max_overlap, band, c.match, c.mismatch, c.gap, c.end_bonus,
                               c.min_aln_score, &moff, &mp, &ps, &coff, &cg, &st));
    std::vector<std::vector<SplitMapping>> out(n);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t j = moff[i]; j < moff[i + 1]; j++) out[i].push_back({ps[j], mp[j], std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
    if (status) status->assign(st, st + n);
    awry_free_buffer(moff); awry_free_buffer(mp); awry_free_buffer(ps); awry_free_buffer(coff); awry_free_buffer(cg); awry_free_buffer(st);
    return out;
  }
  template <class Str>
  std::vector<SplitMapping> map_split_string(const Str& query, uint32_t min_len = 12, uint64_t max_hits = 50, uint64_t chains_per_strand = 4,
                                             SplitParams sp = SplitParams(), uint32_t band = 4, ClipParams c = ClipParams(), ChainParams p = ChainParams()) {
    return parallel_map_split(std::vector<std::string_view>{std::string_view(query)}, min_len, max_hits, chains_per_strand, sp, band, c, p)[0];
  }
  // read pairs mapped together (no counterpart in the reference; the definition is in awry_hip.h, "map read pairs"): reads1[p] and
  // reads2[p] are the mates of pair p.  Per pair at most one Mapping per mate -- the placements of the best pair, with the pair's
  // mapping quality, AWRY_MAP_PROPER_PAIR when they face each other within [min_insert, max_insert] on one record, AWRY_MAP_RESCUED
  // on a mate found within rescue_edits edits where its partner implies it, AWRY_MAP_MATE_UNMAPPED on a read whose mate has no
  // placement -- and the insert size (0 unless proper).
  struct PairParams {
    uint64_t min_insert = 0, max_insert = 1000;
    uint32_t unpaired_penalty = 4, rescue_anchors = 2;
    int rescue_edits = 4;
  };
  struct PairMapping {
    std::vector<Mapping> mate1, mate2;  // none or one each
    uint32_t insert;
  };
  // reads1[p], reads2[p], reads1[p + 1], ..: the interleaved batch of the pair calls
  template <class StrRange>
  static std::vector<std::string_view> interleave(const StrRange& reads1, const StrRange& reads2) {
    std::vector<std::string_view> inter;
    auto b = std::begin(reads2);
    for (const auto& q : reads1) {
      if (b == std::end(reads2)) throw std::invalid_argument("reads1 and reads2 must have one read per pair each");
      inter.emplace_back(q);
      inter.emplace_back(*b);
      ++b;
    }
    if (b != std::end(reads2)) throw std::invalid_argument("reads1 and reads2 must have one read per pair each");
    return inter;
  }
  template <class StrRange>
  std::vector<PairMapping> parallel_map_pairs(const StrRange& reads1, const StrRange& reads2, uint32_t min_len = 12, uint64_t max_hits = 50,
                                              uint64_t chains_per_strand = 4, uint32_t band = 4, PairParams pp = PairParams(),
                                              ChainParams p = ChainParams(), std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(interleave(reads1, reads2), bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* moff = nullptr; awry_map_t* mp = nullptr; awry_pos_t* ps = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr; uint8_t* st = nullptr;
    uint32_t* ins = nullptr;
    check(awry_map_pairs_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score,
                               chains_per_strand, band, pp.min_insert, pp.max_insert, pp.unpaired_penalty, pp.rescue_anchors, pp.rescue_edits, &moff, &mp, &ps,
                               &coff, &cg, &st, &ins));
    std::vector<PairMapping> out(n / 2);
    for (uint64_t i = 0; i < n; i++) {
      std::vector<Mapping>& to = i % 2 ? out[i / 2].mate2 : out[i / 2].mate1;
      for (uint64_t j = moff[i]; j < moff[i + 1]; j++)
        to.push_back({ps[j], mp[j].t_begin, mp[j].t_end, mp[j].edits, mp[j].chain_score, mp[j].chain_index, mp[j].strand, mp[j].mapq, mp[j].flags,
                      std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
      if (i % 2) out[i / 2].insert = ins[i / 2];
    }
    if (status) status->assign(st, st + n);
    awry_free_buffer(moff); awry_free_buffer(mp); awry_free_buffer(ps); awry_free_buffer(coff); awry_free_buffer(cg); awry_free_buffer(st);
    awry_free_buffer(ins);
    return out;
  }
  // The clipped mode of parallel_map_pairs (the definition is in awry_hip.h, "map read pairs, clipped"): the mates' candidates are
  // parallel_map_clip's, the insert is measured between the mates' 5' ends projected through their clips (map.t_begin - map.clip_left
  // of the forward mate to map.t_end + map.clip_right of the reverse one), so a fragment shorter than the reads comes out proper with
  // its own length as insert; pp.unpaired_penalty is in score units here (0 .. AWRY_PAIR_CLIP_MAX_UNPAIRED), the best pair has the
  // largest score + score - penalty, and a rescued mate is a whole-read alignment with score >= c.min_aln_score.
  struct ClippedPairMapping {
    std::vector<ClippedMapping> mate1, mate2;  // none or one each
    uint32_t insert;
  };
  static PairParams clipped_pair_defaults() {
    PairParams pp;
    pp.unpaired_penalty = 20;
    return pp;
  }
  template <class StrRange>
  std::vector<ClippedPairMapping> parallel_map_pairs_clip(const StrRange& reads1, const StrRange& reads2, uint32_t min_len = 12, uint64_t max_hits = 50,
                                                          uint64_t chains_per_strand = 4, uint32_t band = 4, PairParams pp = clipped_pair_defaults(),
                                                          ClipParams c = ClipParams(), ChainParams p = ChainParams(),
                                                          std::vector<uint8_t>* status = nullptr) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off;
    pack(interleave(reads1, reads2), bytes, off);
    const uint64_t n = off.size() - 1;
    uint64_t* moff = nullptr; awry_map_clip_t* mp = nullptr; awry_pos_t* ps = nullptr; uint64_t* coff = nullptr; uint32_t* cg = nullptr; uint8_t* st = nullptr;
    uint32_t* ins = nullptr;
    check(awry_map_pairs_clip_batch(h_, bytes.data(), off.data(), n, min_len, max_hits, p.max_seeds, p.lookback, p.max_gap, p.max_skew, p.min_score,
                                    chains_per_strand, band, pp.min_insert, pp.max_insert, pp.unpaired_penalty, pp.rescue_anchors, pp.rescue_edits, c.match,
                                    c.mismatch, c.gap, c.end_bonus, c.min_aln_score, &moff, &mp, &ps, &coff, &cg, &st, &ins));
    std::vector<ClippedPairMapping> out(n / 2);
    for (uint64_t i = 0; i < n; i++) {
      std::vector<ClippedMapping>& to = i % 2 ? out[i / 2].mate2 : out[i / 2].mate1;
      for (uint64_t j = moff[i]; j < moff[i + 1]; j++) to.push_back({ps[j], mp[j], std::vector<uint32_t>(cg + coff[j], cg + coff[j + 1])});
      if (i % 2) out[i / 2].insert = ins[i / 2];
    }
    if (status) status->assign(st, st + n);
    awry_free_buffer(moff); awry_free_buffer(mp); awry_free_buffer(ps); awry_free_buffer(coff); awry_free_buffer(cg); awry_free_buffer(st);
    awry_free_buffer(ins);
    return out;
  }
  // src/fm_index.rs:559-582, 585-593
  SearchRange update_range_with_symbol(SearchRange r, char symbol) {
    awry_range_t o;
    check(awry_update_range(h_, awry_range_t{r.start_ptr, r.end_ptr}, (uint8_t)symbol, &o));
    return {o.start_ptr, o.end_ptr};
  }
  uint64_t backstep(uint64_t search_pointer) {
    uint64_t o = 0;
    check(awry_backstep(h_, search_pointer, &o));
    return o;
  }
  awry_index_t* handle() { return h_; }

 private:
  explicit FmIndex(awry_index_t* h) : h_(h) {}
  template <class StrRange>
  static void pack(const StrRange& qs, std::vector<uint8_t>& bytes, std::vector<uint64_t>& off) {
    off.assign(1, 0);
    for (const auto& q : qs) {
      std::string_view v(q);
      bytes.insert(bytes.end(), v.begin(), v.end());
      off.push_back(bytes.size());
    }
    if (bytes.empty()) bytes.push_back(0);
  }
  awry_index_t* h_ = nullptr;
};

}  // namespace awry
