//! `FmIndex` with AWRY 0.3.1's public API (reference: src/fm_index.rs:41-119,142,302-399,455-593 and
//! src/fm_index_file.rs:42,132), backed by `libawry_hip.so`.
//!
//! What differs from the reference, and why:
//! * every search runs on a GPU: `new` / `load` replicate the index onto GPU 0 (or the GPUs listed in
//!   `AWRY_DEVICES`, e.g. `0,1,2,3`); [`FmIndex::set_devices`] chooses others.  Batches are sharded over the replicas.
//! * queries on which the reference panics or is undefined (empty query, `$` / `#`, non-ASCII bytes) panic here too,
//!   with the library's message; the `try_*` variants return the error instead.
//! * hits of a multi-record index are localised with the intended semantics (largest record start <= position); the
//!   reference's `get_seq_location` does not terminate there.
//! * `FmIndex` is `Clone` (a cheap handle copy: the index is immutable) and `PartialEq` (same index content);
//!   `PartialOrd` / `Ord` / `Hash` / `MemSize` of the reference's derive list have no counterpart.
use std::ffi::{CStr, CString};
use std::os::raw::c_char;
use std::path::{Path, PathBuf};
use std::sync::Arc;

use awry_hip_sys::{self as sys, awry_aln_t as RawAln, awry_anchor_t as RawAnchor, awry_chain_t as RawChain, awry_map_clip_t as RawMapClip, awry_map_split_t as RawMapSplit, awry_map_t as RawMap, awry_pos_t as RawPos,
                   awry_seed_t as RawSeed};
use rayon::iter::{IndexedParallelIterator, IntoParallelIterator, IntoParallelRefIterator, ParallelIterator};

use crate::{
    alphabet::{Symbol, SymbolAlphabet},
    search::{SearchPtr, SearchRange},
    sequence_index::LocalizedSequencePosition,
};

/// Error of a library call: the status class and the library's message.
#[derive(Debug, Clone)]
pub struct AwryError {
    pub code: i32,
    pub message: String,
}

impl std::fmt::Display for AwryError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "awry error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for AwryError {}

fn last_error(code: i32) -> AwryError {
    let message = unsafe { CStr::from_ptr(sys::awry_last_error()) }.to_string_lossy().into_owned();
    AwryError { code, message }
}

fn check(code: i32) -> Result<(), AwryError> {
    if code == sys::AWRY_OK {
        Ok(())
    } else {
        Err(last_error(code))
    }
}

fn to_io(e: AwryError) -> std::io::Error {
    let kind = match e.code {
        sys::AWRY_ERR_FORMAT => std::io::ErrorKind::InvalidData,
        sys::AWRY_ERR_ARG => std::io::ErrorKind::InvalidInput,
        _ => std::io::ErrorKind::Other,
    };
    std::io::Error::new(kind, e)
}

fn path_cstring(p: &Path) -> Result<CString, AwryError> {
    #[cfg(unix)]
    {
        use std::os::unix::ffi::OsStrExt;
        CString::new(p.as_os_str().as_bytes()).map_err(|_| AwryError { code: sys::AWRY_ERR_ARG, message: "path contains a NUL byte".into() })
    }
    #[cfg(not(unix))]
    {
        CString::new(p.to_string_lossy().as_bytes()).map_err(|_| AwryError { code: sys::AWRY_ERR_ARG, message: "path contains a NUL byte".into() })
    }
}

/// Owner of the C handle; freed when the last `FmIndex` clone goes away.
struct Handle(*mut sys::awry_index_t);
// The library's query entry points are re-entrant and the index is immutable after build / load / set_devices.
unsafe impl Send for Handle {}
unsafe impl Sync for Handle {}
impl Drop for Handle {
    fn drop(&mut self) {
        unsafe { sys::awry_free(self.0) }
    }
}

/// Primary FM-index struct.
///
/// ```no_run
/// use awry::fm_index::{FmIndex, FmBuildArgs};
/// use awry::alphabet::SymbolAlphabet;
///
/// let build_args = FmBuildArgs {
///     input_file_src: "test.fasta".into(),
///     suffix_array_output_src: None,
///     suffix_array_compression_ratio: None,
///     lookup_table_kmer_len: None,
///     alphabet: SymbolAlphabet::Nucleotide,
///     max_query_len: None,
///     remove_intermediate_suffix_array_file: false,
/// };
/// let fm_index = FmIndex::new(&build_args).expect("unable to build fm index");
/// ```
#[derive(Clone)]
pub struct FmIndex {
    handle: Arc<Handle>,
    prefix_sums: Vec<u64>,
}

impl std::fmt::Debug for FmIndex {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        f.debug_struct("FmIndex")
            .field("alphabet", &self.alphabet())
            .field("bwt_len", &self.bwt_len())
            .field("suffix_array_compression_ratio", &self.suffix_array_compression_ratio())
            .field("version_number", &self.version_number())
            .field("devices", &self.num_devices())
            .finish()
    }
}

impl PartialEq for FmIndex {
    /// Same index content: metadata, prefix sums, BWT blocks, sampled suffix array and sequence records
    /// (what the reference's `save_load_equality_test` compares field by field, src/fm_index.rs:1046-1088).
    fn eq(&self, other: &Self) -> bool {
        if Arc::ptr_eq(&self.handle, &other.handle) {
            return true;
        }
        let (a, b) = (self.raw() as *const sys::awry_index_t, other.raw() as *const sys::awry_index_t);
        unsafe {
            if sys::awry_alphabet(a) != sys::awry_alphabet(b)
                || sys::awry_bwt_len(a) != sys::awry_bwt_len(b)
                || sys::awry_version(a) != sys::awry_version(b)
                || sys::awry_sa_ratio(a) != sys::awry_sa_ratio(b)
                || sys::awry_kmer_len(a) != sys::awry_kmer_len(b)
                || self.prefix_sums != other.prefix_sums
            {
                return false;
            }
            let words = |f: unsafe extern "C" fn(*const sys::awry_index_t, *mut u64) -> *const u64, h: *const sys::awry_index_t| {
                let mut n = 0u64;
                let p = f(h, &mut n);
                std::slice::from_raw_parts(p, n as usize)
            };
            if words(sys::awry_block_words, a) != words(sys::awry_block_words, b) || words(sys::awry_sa_words, a) != words(sys::awry_sa_words, b) {
                return false;
            }
        }
        self.sequence_headers() == other.sequence_headers() && self.sequence_starts() == other.sequence_starts()
    }
}
impl Eq for FmIndex {}

/// Arguments for building an FM-index (reference: src/fm_index.rs:78-119).
#[derive(Debug, Clone)]
#[cfg_attr(feature = "serde", derive(serde::Serialize, serde::Deserialize))]
pub struct FmBuildArgs {
    /// file source for the input, either Fasta or Fastq format
    pub input_file_src: PathBuf,
    /// accepted for signature parity: no intermediate suffix-array file is written (the suffix array is built in memory,
    /// on the GPU when one is present)
    pub suffix_array_output_src: Option<PathBuf>,
    /// how much to downsample the suffix array (default 8)
    pub suffix_array_compression_ratio: Option<u64>,
    /// k-mer length of the lookup table stored in `.awry` files (default 10 nucleotide / 4 amino)
    pub lookup_table_kmer_len: Option<u8>,
    /// alphabet of the input text
    pub alphabet: SymbolAlphabet,
    /// accepted for signature parity: the full suffix array is always built
    pub max_query_len: Option<usize>,
    /// accepted for signature parity: there is no intermediate file to remove
    pub remove_intermediate_suffix_array_file: bool,
}

impl FmBuildArgs {
    pub fn new(
        input_file_src: PathBuf,
        suffix_array_output_src: Option<PathBuf>,
        suffix_array_compression_ratio: Option<u64>,
        lookup_table_kmer_len: Option<u8>,
        alphabet: SymbolAlphabet,
        max_query_len: Option<usize>,
        remove_intermediate_suffix_array_file: bool,
    ) -> Self {
        FmBuildArgs {
            input_file_src,
            suffix_array_output_src,
            suffix_array_compression_ratio,
            lookup_table_kmer_len,
            alphabet,
            max_query_len,
            remove_intermediate_suffix_array_file,
        }
    }
}

/// CSR form of a batch of queries: what `awry_count_batch` / `awry_locate_batch` take.
struct Csr {
    bytes: Vec<u8>,
    offsets: Vec<u64>,
}

/// Parameters of [`FmIndex::parallel_chains`] (include/awry_hip.h, awry_chain_batch): `max_seeds` 1..=4096, `lookback` 1..=64,
/// `max_gap` >= 1, `max_skew` >= 0, `min_score` >= 1.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ChainParams {
    pub max_seeds: u32,
    pub lookback: u32,
    pub max_gap: u32,
    pub max_skew: u32,
    pub min_score: u32,
}

impl Default for ChainParams {
    fn default() -> Self {
        ChainParams { max_seeds: 1024, lookback: 32, max_gap: 1000, max_skew: 100, min_score: 20 }
    }
}

/// Parameters of [`FmIndex::parallel_map_pairs`] (include/awry_hip.h, awry_map_pairs_batch): `min_insert` <= `max_insert` <= 2^20,
/// `unpaired_penalty` 0..=255 edits, `rescue_anchors` 0..=4 (0: no mate rescue), `rescue_edits` 0..=8.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct PairParams {
    pub min_insert: u64,
    pub max_insert: u64,
    pub unpaired_penalty: u32,
    pub rescue_anchors: u32,
    pub rescue_edits: i32,
}

impl Default for PairParams {
    fn default() -> Self {
        PairParams { min_insert: 0, max_insert: 1000, unpaired_penalty: 4, rescue_anchors: 2, rescue_edits: 4 }
    }
}

/// One chain of [`FmIndex::parallel_chains`]: its score, the spans it covers in query and text, and its seeds `(q_begin, q_len,
/// t_pos)` first to last.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct Chain {
    pub score: u32,
    pub q_begin: u32,
    pub q_end: u32,
    pub t_begin: u64,
    pub t_end: u64,
    pub seeds: Vec<(u32, u32, u64)>,
}

/// One aligned chain of [`FmIndex::parallel_align_chains`]: the chain's score, the text span `[t_begin, t_end)` the whole read
/// aligns to, the edit count, the status (0 aligned, 1 `AWRY_ALN_SKEW`, 2 `AWRY_ALN_BAD_CHAIN`) and the CIGAR runs
/// (`len << 4 | op`, see [`cigar_string`]).
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct ChainAlignment {
    pub score: u32,
    pub t_begin: u64,
    pub t_end: u64,
    pub edits: u32,
    pub status: u32,
    pub cigar: Vec<u32>,
}

/// One reported alignment of [`FmIndex::parallel_map`]: where `t_begin` lies, the text span `[t_begin, t_end)`, the edit count, the
/// chain it came from, the strand (0 the read as given, 1 its reverse complement), the mapping quality, the flags
/// (`AWRY_MAP_SECONDARY` on every record after the first) and the CIGAR runs of the aligned strand against the forward text.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct Mapping {
    pub position: LocalizedSequencePosition,
    pub t_begin: u64,
    pub t_end: u64,
    pub edits: u32,
    pub chain_score: u32,
    pub chain_index: u32,
    pub strand: u8,
    pub mapq: u8,
    pub flags: u16,
    pub cigar: Vec<u32>,
}

/// The five scalars of the clipped mode (include/awry_hip.h, "soft-clip read ends"): `match_score` 1..=16 per '=', `mismatch` and `gap`
/// 0..=64 per 'X' and per inserted or deleted letter, `end_bonus` 0..=1024, `min_aln_score` the lowest score a candidate may have.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ClipParams {
    pub match_score: u32,
    pub mismatch: u32,
    pub gap: u32,
    pub end_bonus: u32,
    pub min_aln_score: u32,
}

impl Default for ClipParams {
    fn default() -> Self {
        ClipParams { match_score: 1, mismatch: 4, gap: 6, end_bonus: 5, min_aln_score: 0 }
    }
}

/// One record of [`FmIndex::parallel_map_pairs_clip`]: a [`Mapping`] whose span is the aligned part of the read, with the
/// alignment's score and the letters soft-clipped at either end (of the read's reverse complement on strand 1; 'S' runs in `cigar`).
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct ClippedMapping {
    pub mapping: Mapping,
    pub score: i32,
    pub clip_left: u16,
    pub clip_right: u16,
}

/// The three scalars of the split selection (include/awry_hip.h, "split reads"): at most `max_segments` (1..=4) segments per read, at
/// most `max_secondary` (0..=2 x chains_per_strand) reported secondaries, and `max_overlap` (1..=100), the percentage of the shorter
/// query interval two alignments may share before one counts as another place for the same letters.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct SplitParams {
    pub max_segments: u64,
    pub max_secondary: u64,
    pub max_overlap: u32,
}

impl Default for SplitParams {
    fn default() -> Self {
        SplitParams { max_segments: 2, max_secondary: 0, max_overlap: 50 }
    }
}

/// One record of [`FmIndex::parallel_map_split`]: a [`ClippedMapping`] with the letters `[q_begin, q_end)` of the read (as given) it
/// explains and `parent`, the index among the read's records of its segment (its own for a segment).  The first record is the
/// primary, later segments carry `AWRY_MAP_SUPPLEMENTARY`, secondaries `AWRY_MAP_SECONDARY`.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct SplitMapping {
    pub clipped: ClippedMapping,
    pub q_begin: u16,
    pub q_end: u16,
    pub parent: u16,
}

/// The CIGAR string of the runs [`FmIndex::parallel_align_edit`] returns (`len << 4 | op`, BAM's op codes): `"57=1X43="`.
pub fn cigar_string(runs: &[u32]) -> String {
    let mut out = String::new();
    for &run in runs {
        out.push_str(&(run >> 4).to_string());
        out.push(match run & 15 {
            7 => '=',
            8 => 'X',
            1 => 'I',
            _ => 'D',
        });
    }
    out
}

fn to_csr<'a>(queries: impl ParallelIterator<Item = &'a str>) -> Csr {
    let list: Vec<&'a str> = queries.collect();
    let mut offsets = Vec::with_capacity(list.len() + 1);
    let mut at = 0u64;
    offsets.push(0);
    for q in &list {
        at += q.len() as u64;
        offsets.push(at);
    }
    let mut bytes = vec![0u8; at as usize];
    // disjoint slices of the byte buffer, filled in parallel
    let mut rest: &mut [u8] = &mut bytes;
    let mut parts: Vec<&mut [u8]> = Vec::with_capacity(list.len());
    for q in &list {
        let (head, tail) = std::mem::take(&mut rest).split_at_mut(q.len());
        parts.push(head);
        rest = tail;
    }
    parts.into_par_iter().zip(list.par_iter()).for_each(|(dst, q)| dst.copy_from_slice(q.as_bytes()));
    Csr { bytes, offsets }
}

fn default_devices() -> Vec<i32> {
    match std::env::var("AWRY_DEVICES") {
        Ok(s) => {
            let v: Vec<i32> = s.split(',').filter_map(|t| t.trim().parse().ok()).collect();
            if v.is_empty() { vec![0] } else { v }
        }
        Err(_) => vec![0],
    }
}

impl FmIndex {
    fn raw(&self) -> *mut sys::awry_index_t {
        self.handle.0
    }

    fn from_handle(h: *mut sys::awry_index_t) -> Result<Self, AwryError> {
        let handle = Arc::new(Handle(h));
        let mut n = 0u64;
        let p = unsafe { sys::awry_prefix_sums(h, &mut n) };
        let prefix_sums = unsafe { std::slice::from_raw_parts(p, n as usize) }.to_vec();
        let ix = FmIndex { handle, prefix_sums };
        ix.set_devices(&default_devices())?;
        Ok(ix)
    }

    /// Construct a new FM-index using the supplied build args (reference: src/fm_index.rs:142-268).
    pub fn new(args: &FmBuildArgs) -> Result<Self, anyhow::Error> {
        let input = path_cstring(&args.input_file_src)?;
        let sa_tmp = match &args.suffix_array_output_src {
            Some(p) => Some(path_cstring(p)?),
            None => None,
        };
        let c_args = sys::awry_build_args_t {
            input_path: input.as_ptr(),
            sa_tmp_path: sa_tmp.as_ref().map_or(std::ptr::null(), |s| s.as_ptr()),
            sa_ratio: args.suffix_array_compression_ratio.unwrap_or(0),
            kmer_len: args.lookup_table_kmer_len.unwrap_or(0),
            alphabet: args.alphabet.alphabet_id(),
            max_query_len: args.max_query_len.unwrap_or(0) as u64,
            remove_tmp: args.remove_intermediate_suffix_array_file as u8,
        };
        let mut h: *mut sys::awry_index_t = std::ptr::null_mut();
        check(unsafe { sys::awry_build(&c_args, &mut h) })?;
        Ok(Self::from_handle(h)?)
    }

    /// Loads an FM-index from an `.awry` v1 file (reference: src/fm_index_file.rs:132).
    pub fn load(fm_file_src: &Path) -> Result<FmIndex, std::io::Error> {
        let path = path_cstring(fm_file_src).map_err(to_io)?;
        let mut h: *mut sys::awry_index_t = std::ptr::null_mut();
        check(unsafe { sys::awry_load(path.as_ptr(), &mut h) }).map_err(to_io)?;
        Self::from_handle(h).map_err(to_io)
    }

    /// Saves the FM-index to an `.awry` v1 file, byte-compatible with the reference's (src/fm_index_file.rs:42).
    pub fn save(&self, file_output_src: &Path) -> Result<(), std::io::Error> {
        let path = path_cstring(file_output_src).map_err(to_io)?;
        check(unsafe { sys::awry_save(self.raw(), path.as_ptr()) }).map_err(to_io)
    }

    /// Replicates the index onto the listed GPUs (replacing earlier replicas); batches are sharded contiguously over
    /// them.  Stands in for rayon's global pool of the reference.  Not to be called while queries are running.
    pub fn set_devices(&self, device_ids: &[i32]) -> Result<(), AwryError> {
        check(unsafe { sys::awry_set_devices(self.raw(), device_ids.as_ptr(), device_ids.len() as i32) })
    }

    /// Number of GPU replicas.
    pub fn num_devices(&self) -> usize {
        unsafe { sys::awry_num_devices(self.raw()) as usize }
    }

    /// Gets the alphabet of the index.
    pub fn alphabet(&self) -> SymbolAlphabet {
        SymbolAlphabet::from_id(unsafe { sys::awry_alphabet(self.raw()) })
    }

    /// Gets the suffix array compression ratio.
    pub fn suffix_array_compression_ratio(&self) -> u64 {
        unsafe { sys::awry_sa_ratio(self.raw()) }
    }

    /// Gets the length of the BWT (text length + 1).
    pub fn bwt_len(&self) -> u64 {
        unsafe { sys::awry_bwt_len(self.raw()) }
    }

    /// Gets the version number of the FM-index.
    pub fn version_number(&self) -> u64 {
        unsafe { sys::awry_version(self.raw()) }
    }

    /// Gets a reference to the prefix sums.
    pub fn prefix_sums(&self) -> &Vec<u64> {
        &self.prefix_sums
    }

    /// Headers of the indexed sequences, in file order (the reference keeps them in its crate-private SequenceIndex).
    pub fn sequence_headers(&self) -> Vec<String> {
        let n = unsafe { sys::awry_num_sequences(self.raw()) };
        (0..n)
            .map(|i| unsafe {
                let p: *const c_char = sys::awry_sequence_header(self.raw(), i);
                if p.is_null() { String::new() } else { CStr::from_ptr(p).to_string_lossy().into_owned() }
            })
            .collect()
    }

    /// Start position of every indexed sequence in the concatenated text.
    pub fn sequence_starts(&self) -> Vec<usize> {
        let n = unsafe { sys::awry_num_sequences(self.raw()) };
        (0..n).map(|i| unsafe { sys::awry_sequence_start(self.raw(), i) as usize }).collect()
    }

    /// Gets the initial search range for the given character.
    pub fn initial_search_range(&self, s: Symbol) -> SearchRange {
        SearchRange::new(self, s)
    }

    /// Counts of a batch of queries, in input order (reference: src/fm_index.rs:455-460).  One library call for the
    /// whole batch: the queries are gathered into one byte buffer, packed 2 bits per letter on the library's worker pool
    /// and searched on the GPU replicas.
    pub fn parallel_count<'a>(&self, queries: impl ParallelIterator<Item = &'a str>) -> Vec<u64> {
        self.try_parallel_count(queries).unwrap_or_else(|e| panic!("{}", e))
    }

    /// [`FmIndex::parallel_count`] that returns the library's error instead of panicking.
    pub fn try_parallel_count<'a>(&self, queries: impl ParallelIterator<Item = &'a str>) -> Result<Vec<u64>, AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut counts = vec![0u64; n];
        check(unsafe { sys::awry_count_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, counts.as_mut_ptr()) })?;
        Ok(counts)
    }

    /// Counts of a CSR batch (query i = `bytes[offsets[i]..offsets[i + 1]]`) into a caller-owned slice: the zero-copy
    /// form of [`FmIndex::parallel_count`] for callers that already hold their queries contiguously.
    pub fn count_batch_into(&self, bytes: &[u8], offsets: &[u64], counts_out: &mut [u64]) -> Result<(), AwryError> {
        assert!(!offsets.is_empty() && counts_out.len() == offsets.len() - 1 && *offsets.last().unwrap() as usize <= bytes.len());
        check(unsafe { sys::awry_count_batch(self.raw(), bytes.as_ptr(), offsets.as_ptr(), counts_out.len() as u64, counts_out.as_mut_ptr()) })
    }

    /// Counts of k-mers the caller already holds packed: letter j (0 = leftmost) of k-mer i in bits `[2j, 2j + 2)` of
    /// `words[i]`, A0 C1 G2 T3, `len <= 32` (no counterpart in the reference; nucleotide indexes).
    pub fn count_packed_kmers(&self, words: &[u64], len: usize, counts_out: &mut [u64]) -> Result<(), AwryError> {
        assert_eq!(words.len(), counts_out.len());
        check(unsafe { sys::awry_count_packed_kmers(self.raw(), words.as_ptr(), words.len() as u64, len as i32, counts_out.as_mut_ptr()) })
    }

    /// Locations of a batch of queries (reference: src/fm_index.rs:479-487): outer order = input order, inner order =
    /// ascending BWT row, as `locate_string` returns them.
    pub fn parallel_locate<'a>(&self, queries: impl ParallelIterator<Item = &'a str>) -> Vec<Vec<LocalizedSequencePosition>> {
        self.try_parallel_locate(queries).unwrap_or_else(|e| panic!("{}", e))
    }

    /// [`FmIndex::parallel_locate`] that returns the library's error instead of panicking.
    pub fn try_parallel_locate<'a>(&self, queries: impl ParallelIterator<Item = &'a str>) -> Result<Vec<Vec<LocalizedSequencePosition>>, AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut hit_off: *mut u64 = std::ptr::null_mut();
        let mut hits: *mut sys::awry_pos_t = std::ptr::null_mut();
        check(unsafe {
            sys::awry_locate_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, &mut hit_off, &mut hits, std::ptr::null_mut())
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(hit_off, n + 1);
            let total = off[n] as usize;
            let flat: &[sys::awry_pos_t] = if total == 0 { &[] } else { std::slice::from_raw_parts(hits, total) };
            (0..n)
                .into_par_iter()
                .map(|i| {
                    flat[off[i] as usize..off[i + 1] as usize]
                        .iter()
                        .map(|p| LocalizedSequencePosition::new(p.seq_idx as usize, p.local_pos as usize))
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>()
        };
        unsafe {
            sys::awry_free_buffer(hit_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(hits as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Substitution-tolerant counts (no counterpart in the reference; semantics in include/awry_hip.h): row i of the result
    /// holds the occurrences of query i at exactly 0, 1, .., `max_mismatches` substitutions (Hamming distance over symbol
    /// indices, windows holding '$' never match); `max_mismatches` must be 0, 1 or 2.
    pub fn parallel_count_mismatch<'a>(&self, queries: impl ParallelIterator<Item = &'a str>, max_mismatches: u32) -> Result<Vec<Vec<u64>>, AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let w = max_mismatches as usize + 1;
        let mut counts = vec![0u64; n * w];
        check(unsafe {
            sys::awry_count_mismatch_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, max_mismatches as i32, counts.as_mut_ptr())
        })?;
        Ok(counts.chunks(w).map(|c| c.to_vec()).collect())
    }

    /// Substitution-tolerant locations: per query, `(position, distance)` in ascending BWT-row order.
    pub fn parallel_locate_mismatch<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        max_mismatches: u32,
    ) -> Result<Vec<Vec<(LocalizedSequencePosition, u8)>>, AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut hit_off: *mut u64 = std::ptr::null_mut();
        let mut hits: *mut sys::awry_pos_t = std::ptr::null_mut();
        let mut mm: *mut u8 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_locate_mismatch_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, max_mismatches as i32, &mut hit_off,
                                            &mut hits, std::ptr::null_mut(), &mut mm)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(hit_off, n + 1);
            let total = off[n] as usize;
            let flat: &[sys::awry_pos_t] = if total == 0 { &[] } else { std::slice::from_raw_parts(hits, total) };
            let dist: &[u8] = if total == 0 { &[] } else { std::slice::from_raw_parts(mm, total) };
            (0..n)
                .map(|i| {
                    (off[i] as usize..off[i + 1] as usize)
                        .map(|j| (LocalizedSequencePosition::new(flat[j].seq_idx as usize, flat[j].local_pos as usize), dist[j]))
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>()
        };
        unsafe {
            sys::awry_free_buffer(hit_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(hits as *mut std::os::raw::c_void);
            sys::awry_free_buffer(mm as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Class-pattern counts (no counterpart in the reference; the definition and the limits are in include/awry_hip.h): a pattern
    /// is a string of class letters (nucleotide IUPAC codes, amino B / Z / J / X); row i of the result holds the occurrences of
    /// pattern i at exactly 0, 1, .., `max_mismatches` mismatches (a position mismatches when the text symbol is outside the
    /// letter's class); `max_mismatches` must be 0, 1 or 2.
    pub fn parallel_count_pattern<'a>(&self, patterns: impl ParallelIterator<Item = &'a str>, max_mismatches: u32) -> Result<Vec<Vec<u64>>, AwryError> {
        let csr = to_csr(patterns);
        let n = csr.offsets.len() - 1;
        let w = max_mismatches as usize + 1;
        let mut counts = vec![0u64; n * w];
        check(unsafe {
            sys::awry_count_pattern_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, max_mismatches as i32, counts.as_mut_ptr())
        })?;
        Ok(counts.chunks(w).map(|c| c.to_vec()).collect())
    }

    /// Class-pattern locations: per pattern, `(position, distance)` in ascending BWT-row order (the matched strings in
    /// symbol-index order).
    pub fn parallel_locate_pattern<'a>(
        &self,
        patterns: impl ParallelIterator<Item = &'a str>,
        max_mismatches: u32,
    ) -> Result<Vec<Vec<(LocalizedSequencePosition, u8)>>, AwryError> {
        let csr = to_csr(patterns);
        let n = csr.offsets.len() - 1;
        let mut hit_off: *mut u64 = std::ptr::null_mut();
        let mut hits: *mut sys::awry_pos_t = std::ptr::null_mut();
        let mut mm: *mut u8 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_locate_pattern_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, max_mismatches as i32, &mut hit_off,
                                           &mut hits, std::ptr::null_mut(), &mut mm)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(hit_off, n + 1);
            let total = off[n] as usize;
            let flat: &[sys::awry_pos_t] = if total == 0 { &[] } else { std::slice::from_raw_parts(hits, total) };
            let dist: &[u8] = if total == 0 { &[] } else { std::slice::from_raw_parts(mm, total) };
            (0..n)
                .map(|i| {
                    (off[i] as usize..off[i + 1] as usize)
                        .map(|j| (LocalizedSequencePosition::new(flat[j].seq_idx as usize, flat[j].local_pos as usize), dist[j]))
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>()
        };
        unsafe {
            sys::awry_free_buffer(hit_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(hits as *mut std::os::raw::c_void);
            sys::awry_free_buffer(mm as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Anchors (no counterpart in the reference; the definition is in include/awry_hip.h): per query, its greedy longest-match
    /// factorisation found right to left, as `(q_begin, q_len, SearchRange)` -- the maximal exact matches a mapper chains when a
    /// read does not occur as a whole.  Anchors shorter than `min_len` (>= 1) are left out; `skip_failed_letter` leaves the
    /// letter that ended an anchor out of the next one.
    pub fn parallel_anchors<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        min_len: u32,
        skip_failed_letter: bool,
    ) -> Result<Vec<Vec<(usize, usize, SearchRange)>>, AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut anchor_off: *mut u64 = std::ptr::null_mut();
        let mut anchors: *mut RawAnchor = std::ptr::null_mut();
        check(unsafe {
            sys::awry_anchor_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, skip_failed_letter as i32, &mut anchor_off,
                                   &mut anchors)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(anchor_off, n + 1);
            let total = off[n] as usize;
            let flat: &[RawAnchor] = if total == 0 { &[] } else { std::slice::from_raw_parts(anchors, total) };
            (0..n)
                .map(|i| {
                    flat[off[i] as usize..off[i + 1] as usize]
                        .iter()
                        .map(|a| (a.q_begin as usize, a.q_len as usize, SearchRange { start_ptr: a.start_row, end_ptr: a.start_row + a.count - 1 }))
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>()
        };
        unsafe {
            sys::awry_free_buffer(anchor_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(anchors as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// SMEMs (no counterpart in the reference; the definition is in include/awry_hip.h): per query, every super-maximal exact
    /// match -- a substring that occurs and cannot be extended by one letter on either side and still occur -- of at least
    /// `min_len` (>= 1) letters, in descending begin, as `(q_begin, q_len, SearchRange)`: the seeds of a read mapper.
    pub fn parallel_smems<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        min_len: u32,
    ) -> Result<Vec<Vec<(usize, usize, SearchRange)>>, AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut smem_off: *mut u64 = std::ptr::null_mut();
        let mut smems: *mut RawAnchor = std::ptr::null_mut();
        check(unsafe { sys::awry_smem_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, &mut smem_off, &mut smems) })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(smem_off, n + 1);
            let total = off[n] as usize;
            let flat: &[RawAnchor] = if total == 0 { &[] } else { std::slice::from_raw_parts(smems, total) };
            (0..n)
                .map(|i| {
                    flat[off[i] as usize..off[i + 1] as usize]
                        .iter()
                        .map(|a| (a.q_begin as usize, a.q_len as usize, SearchRange { start_ptr: a.start_row, end_ptr: a.start_row + a.count - 1 }))
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>()
        };
        unsafe {
            sys::awry_free_buffer(smem_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(smems as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// The chains aligned (no counterpart in the reference; the definition is in include/awry_hip.h): of every query's chains the
    /// first `max_alignments`, the primary first, each with the text span of the whole read, its edit count and its CIGAR; `band`
    /// is 0..=8.  And per query whether it was abandoned because it has more than `params.max_seeds` seeds.
    pub fn parallel_align_chains<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        min_len: u32,
        max_hits: u64,
        max_alignments: u64,
        band: u32,
        params: ChainParams,
    ) -> Result<(Vec<Vec<ChainAlignment>>, Vec<bool>), AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut aln_off: *mut u64 = std::ptr::null_mut();
        let mut chains: *mut RawChain = std::ptr::null_mut();
        let mut alns: *mut RawAln = std::ptr::null_mut();
        let mut cigar_off: *mut u64 = std::ptr::null_mut();
        let mut cigar: *mut u32 = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_align_chains_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, max_hits, params.max_seeds, params.lookback,
                                         params.max_gap, params.max_skew, params.min_score, max_alignments, band, &mut aln_off, &mut chains, &mut alns,
                                         &mut cigar_off, &mut cigar, &mut st)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(aln_off, n + 1);
            let total = off[n] as usize;
            let ch: &[RawChain] = if total == 0 { &[] } else { std::slice::from_raw_parts(chains, total) };
            let al: &[RawAln] = if total == 0 { &[] } else { std::slice::from_raw_parts(alns, total) };
            let coff = std::slice::from_raw_parts(cigar_off, total + 1);
            let runs: &[u32] = if coff[total] == 0 { &[] } else { std::slice::from_raw_parts(cigar, coff[total] as usize) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let per = (0..n)
                .map(|i| {
                    (off[i] as usize..off[i + 1] as usize)
                        .map(|j| ChainAlignment {
                            score: ch[j].score,
                            t_begin: al[j].t_begin,
                            t_end: al[j].t_end,
                            edits: al[j].edits,
                            status: al[j].status,
                            cigar: runs[coff[j] as usize..coff[j + 1] as usize].to_vec(),
                        })
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 8).collect::<Vec<_>>())  // AWRY_Q_SEED_CAP
        };
        unsafe {
            sys::awry_free_buffer(aln_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(chains as *mut std::os::raw::c_void);
            sys::awry_free_buffer(alns as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Reads mapped on both strands (no counterpart in the reference; the definition is in include/awry_hip.h): per read its best
    /// alignments over the read and its reverse complement, the primary first, at most `max_report` of them (1..=2 *
    /// `chains_per_strand`, which is 1..=8), each with strand, position, edit count, MAPQ and CIGAR.  And per read whether one of
    /// its strands was abandoned because it has more than `params.max_seeds` seeds (its MAPQ is then 0).
    pub fn parallel_map<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        min_len: u32,
        max_hits: u64,
        chains_per_strand: u64,
        max_report: u64,
        band: u32,
        params: ChainParams,
    ) -> Result<(Vec<Vec<Mapping>>, Vec<bool>), AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut map_off: *mut u64 = std::ptr::null_mut();
        let mut maps: *mut RawMap = std::ptr::null_mut();
        let mut pos: *mut RawPos = std::ptr::null_mut();
        let mut cigar_off: *mut u64 = std::ptr::null_mut();
        let mut cigar: *mut u32 = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_map_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, max_hits, params.max_seeds, params.lookback,
                                params.max_gap, params.max_skew, params.min_score, chains_per_strand, max_report, band, &mut map_off, &mut maps, &mut pos,
                                &mut cigar_off, &mut cigar, &mut st)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(map_off, n + 1);
            let total = off[n] as usize;
            let mp: &[RawMap] = if total == 0 { &[] } else { std::slice::from_raw_parts(maps, total) };
            let ps: &[RawPos] = if total == 0 { &[] } else { std::slice::from_raw_parts(pos, total) };
            let coff = std::slice::from_raw_parts(cigar_off, total + 1);
            let runs: &[u32] = if coff[total] == 0 { &[] } else { std::slice::from_raw_parts(cigar, coff[total] as usize) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let per = (0..n)
                .map(|i| {
                    (off[i] as usize..off[i + 1] as usize)
                        .map(|j| Mapping {
                            position: LocalizedSequencePosition::new(ps[j].seq_idx as usize, ps[j].local_pos as usize),
                            t_begin: mp[j].t_begin,
                            t_end: mp[j].t_end,
                            edits: mp[j].edits,
                            chain_score: mp[j].chain_score,
                            chain_index: mp[j].chain_index,
                            strand: mp[j].strand,
                            mapq: mp[j].mapq,
                            flags: mp[j].flags,
                            cigar: runs[coff[j] as usize..coff[j + 1] as usize].to_vec(),
                        })
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 8).collect::<Vec<_>>())  // AWRY_Q_SEED_CAP
        };
        unsafe {
            sys::awry_free_buffer(map_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(maps as *mut std::os::raw::c_void);
            sys::awry_free_buffer(pos as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Read pairs mapped together (no counterpart in the reference; the definition is in include/awry_hip.h, "map read pairs"):
    /// `reads1[p]` and `reads2[p]` are the mates of pair p.  Per pair the placements of the best pair -- none or one `Mapping` per
    /// mate, with the pair MAPQ, `AWRY_MAP_PROPER_PAIR`, `AWRY_MAP_RESCUED` or `AWRY_MAP_MATE_UNMAPPED` in `flags` -- and the insert
    /// size (0 unless the pair is proper); and per read (interleaved) whether one of its strands was abandoned at `params.max_seeds`.
    pub fn parallel_map_pairs(
        &self,
        reads1: &[&str],
        reads2: &[&str],
        min_len: u32,
        max_hits: u64,
        chains_per_strand: u64,
        band: u32,
        pair: PairParams,
        params: ChainParams,
    ) -> Result<(Vec<(Option<Mapping>, Option<Mapping>, u32)>, Vec<bool>), AwryError> {
        assert_eq!(reads1.len(), reads2.len(), "reads1 and reads2 must have one read per pair each");
        let inter: Vec<&str> = reads1.iter().zip(reads2.iter()).flat_map(|(a, b)| [*a, *b]).collect();
        let csr = to_csr(inter.into_par_iter());
        let n = csr.offsets.len() - 1;
        let mut map_off: *mut u64 = std::ptr::null_mut();
        let mut maps: *mut RawMap = std::ptr::null_mut();
        let mut pos: *mut RawPos = std::ptr::null_mut();
        let mut cigar_off: *mut u64 = std::ptr::null_mut();
        let mut cigar: *mut u32 = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        let mut ins: *mut u32 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_map_pairs_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, max_hits, params.max_seeds, params.lookback,
                                      params.max_gap, params.max_skew, params.min_score, chains_per_strand, band, pair.min_insert, pair.max_insert,
                                      pair.unpaired_penalty, pair.rescue_anchors, pair.rescue_edits, &mut map_off, &mut maps, &mut pos, &mut cigar_off,
                                      &mut cigar, &mut st, &mut ins)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(map_off, n + 1);
            let total = off[n] as usize;
            let mp: &[RawMap] = if total == 0 { &[] } else { std::slice::from_raw_parts(maps, total) };
            let ps: &[RawPos] = if total == 0 { &[] } else { std::slice::from_raw_parts(pos, total) };
            let coff = std::slice::from_raw_parts(cigar_off, total + 1);
            let runs: &[u32] = if coff[total] == 0 { &[] } else { std::slice::from_raw_parts(cigar, coff[total] as usize) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let inserts: &[u32] = if n == 0 { &[] } else { std::slice::from_raw_parts(ins, n / 2) };
            let record = |i: usize| {
                (off[i] as usize..off[i + 1] as usize).next().map(|j| Mapping {
                    position: LocalizedSequencePosition::new(ps[j].seq_idx as usize, ps[j].local_pos as usize),
                    t_begin: mp[j].t_begin,
                    t_end: mp[j].t_end,
                    edits: mp[j].edits,
                    chain_score: mp[j].chain_score,
                    chain_index: mp[j].chain_index,
                    strand: mp[j].strand,
                    mapq: mp[j].mapq,
                    flags: mp[j].flags,
                    cigar: runs[coff[j] as usize..coff[j + 1] as usize].to_vec(),
                })
            };
            let per = (0..n / 2).map(|p| (record(2 * p), record(2 * p + 1), inserts[p])).collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 8).collect::<Vec<_>>())  // AWRY_Q_SEED_CAP
        };
        unsafe {
            sys::awry_free_buffer(map_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(maps as *mut std::os::raw::c_void);
            sys::awry_free_buffer(pos as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
            sys::awry_free_buffer(ins as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// [`FmIndex::parallel_map_pairs`] in the clipped mode (include/awry_hip.h, "map read pairs, clipped"): the mates' candidates are
    /// clipped alignments, the insert is measured between the mates' 5' ends projected through their clips, so a fragment shorter than
    /// the reads comes out proper with its own length as insert; `pair.unpaired_penalty` is in score units here (0..=16384,
    /// `AWRY_PAIR_CLIP_MAX_UNPAIRED`), and a rescued mate is a whole-read alignment with score >= `clip.min_aln_score`.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn parallel_map_pairs_clip(
        &self,
        reads1: &[&str],
        reads2: &[&str],
        min_len: u32,
        max_hits: u64,
        chains_per_strand: u64,
        band: u32,
        pair: PairParams,
        clip: ClipParams,
        params: ChainParams,
    ) -> Result<(Vec<(Option<ClippedMapping>, Option<ClippedMapping>, u32)>, Vec<bool>), AwryError> {
        assert_eq!(reads1.len(), reads2.len(), "reads1 and reads2 must have one read per pair each");
        let inter: Vec<&str> = reads1.iter().zip(reads2.iter()).flat_map(|(a, b)| [*a, *b]).collect();
        let csr = to_csr(inter.into_par_iter());
        let n = csr.offsets.len() - 1;
        let mut map_off: *mut u64 = std::ptr::null_mut();
        let mut maps: *mut RawMapClip = std::ptr::null_mut();
        let mut pos: *mut RawPos = std::ptr::null_mut();
        let mut cigar_off: *mut u64 = std::ptr::null_mut();
        let mut cigar: *mut u32 = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        let mut ins: *mut u32 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_map_pairs_clip_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, max_hits, params.max_seeds,
                                           params.lookback, params.max_gap, params.max_skew, params.min_score, chains_per_strand, band, pair.min_insert,
                                           pair.max_insert, pair.unpaired_penalty, pair.rescue_anchors, pair.rescue_edits, clip.match_score, clip.mismatch,
                                           clip.gap, clip.end_bonus, clip.min_aln_score, &mut map_off, &mut maps, &mut pos, &mut cigar_off, &mut cigar,
                                           &mut st, &mut ins)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(map_off, n + 1);
            let total = off[n] as usize;
            let mp: &[RawMapClip] = if total == 0 { &[] } else { std::slice::from_raw_parts(maps, total) };
            let ps: &[RawPos] = if total == 0 { &[] } else { std::slice::from_raw_parts(pos, total) };
            let coff = std::slice::from_raw_parts(cigar_off, total + 1);
            let runs: &[u32] = if coff[total] == 0 { &[] } else { std::slice::from_raw_parts(cigar, coff[total] as usize) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let inserts: &[u32] = if n == 0 { &[] } else { std::slice::from_raw_parts(ins, n / 2) };
            let record = |i: usize| {
                (off[i] as usize..off[i + 1] as usize).next().map(|j| ClippedMapping {
                    mapping: Mapping {
                        position: LocalizedSequencePosition::new(ps[j].seq_idx as usize, ps[j].local_pos as usize),
                        t_begin: mp[j].t_begin,
                        t_end: mp[j].t_end,
                        edits: mp[j].edits,
                        chain_score: mp[j].chain_score,
                        chain_index: mp[j].chain_index,
                        strand: mp[j].strand,
                        mapq: mp[j].mapq,
                        flags: mp[j].flags,
                        cigar: runs[coff[j] as usize..coff[j + 1] as usize].to_vec(),
                    },
                    score: mp[j].score,
                    clip_left: mp[j].clip_left,
                    clip_right: mp[j].clip_right,
                })
            };
            let per = (0..n / 2).map(|p| (record(2 * p), record(2 * p + 1), inserts[p])).collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 8).collect::<Vec<_>>())  // AWRY_Q_SEED_CAP
        };
        unsafe {
            sys::awry_free_buffer(map_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(maps as *mut std::os::raw::c_void);
            sys::awry_free_buffer(pos as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
            sys::awry_free_buffer(ins as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Split reads (no counterpart in the reference; include/awry_hip.h, "split reads"): per read its segments -- clipped alignments
    /// over different letters of the read, the primary and then the supplementaries, each with a mapping quality of its own -- and then
    /// its reported secondaries; and per read whether one of its strands was abandoned at `params.max_seeds`.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn parallel_map_split<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        min_len: u32,
        max_hits: u64,
        chains_per_strand: u64,
        split: SplitParams,
        band: u32,
        clip: ClipParams,
        params: ChainParams,
    ) -> Result<(Vec<Vec<SplitMapping>>, Vec<bool>), AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut map_off: *mut u64 = std::ptr::null_mut();
        let mut maps: *mut RawMapSplit = std::ptr::null_mut();
        let mut pos: *mut RawPos = std::ptr::null_mut();
        let mut cigar_off: *mut u64 = std::ptr::null_mut();
        let mut cigar: *mut u32 = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_map_split_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, max_hits, params.max_seeds, params.lookback,
                                      params.max_gap, params.max_skew, params.min_score, chains_per_strand, split.max_segments, split.max_secondary,
                                      split.max_overlap, band, clip.match_score, clip.mismatch, clip.gap, clip.end_bonus, clip.min_aln_score, &mut map_off,
                                      &mut maps, &mut pos, &mut cigar_off, &mut cigar, &mut st)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(map_off, n + 1);
            let total = off[n] as usize;
            let mp: &[RawMapSplit] = if total == 0 { &[] } else { std::slice::from_raw_parts(maps, total) };
            let ps: &[RawPos] = if total == 0 { &[] } else { std::slice::from_raw_parts(pos, total) };
            let coff = std::slice::from_raw_parts(cigar_off, total + 1);
            let runs: &[u32] = if coff[total] == 0 { &[] } else { std::slice::from_raw_parts(cigar, coff[total] as usize) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let record = |j: usize| SplitMapping {
                clipped: ClippedMapping {
                    mapping: Mapping {
                        position: LocalizedSequencePosition::new(ps[j].seq_idx as usize, ps[j].local_pos as usize),
                        t_begin: mp[j].t_begin,
                        t_end: mp[j].t_end,
                        edits: mp[j].edits,
                        chain_score: mp[j].chain_score,
                        chain_index: mp[j].chain_index,
                        strand: mp[j].strand,
                        mapq: mp[j].mapq,
                        flags: mp[j].flags,
                        cigar: runs[coff[j] as usize..coff[j + 1] as usize].to_vec(),
                    },
                    score: mp[j].score,
                    clip_left: mp[j].clip_left,
                    clip_right: mp[j].clip_right,
                },
                q_begin: mp[j].q_begin,
                q_end: mp[j].q_end,
                parent: mp[j].parent,
            };
            let per = (0..n).map(|i| (off[i] as usize..off[i + 1] as usize).map(record).collect::<Vec<_>>()).collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 8).collect::<Vec<_>>())  // AWRY_Q_SEED_CAP
        };
        unsafe {
            sys::awry_free_buffer(map_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(maps as *mut std::os::raw::c_void);
            sys::awry_free_buffer(pos as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Colinear chaining of the located SMEM seeds (no counterpart in the reference; the definition is in include/awry_hip.h): per
    /// query its chains, the primary chain first, each with its seeds first to last; and per query whether it was abandoned because
    /// it has more than `params.max_seeds` seeds.
    pub fn parallel_chains<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        min_len: u32,
        max_hits: u64,
        params: ChainParams,
    ) -> Result<(Vec<Vec<Chain>>, Vec<bool>), AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut chain_off: *mut u64 = std::ptr::null_mut();
        let mut chains: *mut RawChain = std::ptr::null_mut();
        let mut seed_off: *mut u64 = std::ptr::null_mut();
        let mut seeds: *mut RawSeed = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_chain_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, min_len, max_hits, params.max_seeds, params.lookback,
                                  params.max_gap, params.max_skew, params.min_score, &mut chain_off, &mut chains, &mut seed_off, &mut seeds, &mut st)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(chain_off, n + 1);
            let total = off[n] as usize;
            let flat: &[RawChain] = if total == 0 { &[] } else { std::slice::from_raw_parts(chains, total) };
            let soff = std::slice::from_raw_parts(seed_off, total + 1);
            let members: &[RawSeed] = if soff[total] == 0 { &[] } else { std::slice::from_raw_parts(seeds, soff[total] as usize) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let per = (0..n)
                .map(|i| {
                    (off[i] as usize..off[i + 1] as usize)
                        .map(|j| Chain {
                            score: flat[j].score,
                            q_begin: flat[j].q_begin,
                            q_end: flat[j].q_end,
                            t_begin: flat[j].t_begin,
                            t_end: flat[j].t_end,
                            seeds: members[soff[j] as usize..soff[j + 1] as usize].iter().map(|m| (m.q_begin, m.q_len, m.t_pos)).collect(),
                        })
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 8).collect::<Vec<_>>())  // AWRY_Q_SEED_CAP
        };
        unsafe {
            sys::awry_free_buffer(chain_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(chains as *mut std::os::raw::c_void);
            sys::awry_free_buffer(seed_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(seeds as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Locate within k edits (no counterpart in the reference; the definition is in include/awry_hip.h): per query, `(position,
    /// distance)` of every start whose best alignment has at most `max_edits` (0..=8) substitutions, insertions and deletions
    /// and is not beaten by a neighbouring start, in ascending text position; and per query whether it was abandoned because
    /// its `max_edits + 1` pieces occur more than `max_candidates` (>= 1) times in all.
    pub fn parallel_locate_edit<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        max_edits: u32,
        max_candidates: u64,
    ) -> Result<(Vec<Vec<(LocalizedSequencePosition, u8)>>, Vec<bool>), AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut hit_off: *mut u64 = std::ptr::null_mut();
        let mut hits: *mut sys::awry_pos_t = std::ptr::null_mut();
        let mut ed: *mut u8 = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_locate_edit_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, max_edits as i32, max_candidates, &mut hit_off,
                                        &mut hits, std::ptr::null_mut(), &mut ed, &mut st)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(hit_off, n + 1);
            let total = off[n] as usize;
            let flat: &[sys::awry_pos_t] = if total == 0 { &[] } else { std::slice::from_raw_parts(hits, total) };
            let dist: &[u8] = if total == 0 { &[] } else { std::slice::from_raw_parts(ed, total) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let per = (0..n)
                .map(|i| {
                    (off[i] as usize..off[i + 1] as usize)
                        .map(|j| (LocalizedSequencePosition::new(flat[j].seq_idx as usize, flat[j].local_pos as usize), dist[j]))
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 7).collect::<Vec<_>>())  // AWRY_Q_CANDIDATE_CAP
        };
        unsafe {
            sys::awry_free_buffer(hit_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(hits as *mut std::os::raw::c_void);
            sys::awry_free_buffer(ed as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// The same hits aligned (the canonical script is defined in include/awry_hip.h): per query, `(position, distance, text_len,
    /// cigar)` in ascending text position -- the hit matches `text_len` text letters from its start by the runs `cigar`, each
    /// `len << 4 | op` with BAM's op codes (I = 1, D = 2, '=' = 7, X = 8; at most 17 runs) -- and per query whether it was
    /// abandoned by the candidate cap.  [`cigar_string`] renders the runs.
    #[allow(clippy::type_complexity)]
    pub fn parallel_align_edit<'a>(
        &self,
        queries: impl ParallelIterator<Item = &'a str>,
        max_edits: u32,
        max_candidates: u64,
    ) -> Result<(Vec<Vec<(LocalizedSequencePosition, u8, u32, Vec<u32>)>>, Vec<bool>), AwryError> {
        let csr = to_csr(queries);
        let n = csr.offsets.len() - 1;
        let mut hit_off: *mut u64 = std::ptr::null_mut();
        let mut hits: *mut sys::awry_pos_t = std::ptr::null_mut();
        let mut ed: *mut u8 = std::ptr::null_mut();
        let mut st: *mut u8 = std::ptr::null_mut();
        let mut tl: *mut u32 = std::ptr::null_mut();
        let mut cigar_off: *mut u64 = std::ptr::null_mut();
        let mut cigar: *mut u32 = std::ptr::null_mut();
        check(unsafe {
            sys::awry_align_edit_batch(self.raw(), csr.bytes.as_ptr(), csr.offsets.as_ptr(), n as u64, max_edits as i32, max_candidates, &mut hit_off,
                                       &mut hits, std::ptr::null_mut(), &mut ed, &mut st, &mut tl, &mut cigar_off, &mut cigar)
        })?;
        let out = unsafe {
            let off = std::slice::from_raw_parts(hit_off, n + 1);
            let total = off[n] as usize;
            let flat: &[sys::awry_pos_t] = if total == 0 { &[] } else { std::slice::from_raw_parts(hits, total) };
            let dist: &[u8] = if total == 0 { &[] } else { std::slice::from_raw_parts(ed, total) };
            let span: &[u32] = if total == 0 { &[] } else { std::slice::from_raw_parts(tl, total) };
            let coff = std::slice::from_raw_parts(cigar_off, total + 1);
            let runs: &[u32] = if coff[total] == 0 { &[] } else { std::slice::from_raw_parts(cigar, coff[total] as usize) };
            let status: &[u8] = if n == 0 { &[] } else { std::slice::from_raw_parts(st, n) };
            let per = (0..n)
                .map(|i| {
                    (off[i] as usize..off[i + 1] as usize)
                        .map(|j| {
                            (LocalizedSequencePosition::new(flat[j].seq_idx as usize, flat[j].local_pos as usize), dist[j], span[j],
                             runs[coff[j] as usize..coff[j + 1] as usize].to_vec())
                        })
                        .collect::<Vec<_>>()
                })
                .collect::<Vec<_>>();
            (per, status.iter().map(|&s| s == 7).collect::<Vec<_>>())  // AWRY_Q_CANDIDATE_CAP
        };
        unsafe {
            sys::awry_free_buffer(hit_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(hits as *mut std::os::raw::c_void);
            sys::awry_free_buffer(ed as *mut std::os::raw::c_void);
            sys::awry_free_buffer(st as *mut std::os::raw::c_void);
            sys::awry_free_buffer(tl as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(cigar as *mut std::os::raw::c_void);
        }
        Ok(out)
    }

    /// Locations of a batch as flat arrays: `(hit_offsets[n + 1], global text positions)`; the hits of query i are
    /// `positions[hit_offsets[i]..hit_offsets[i + 1]]`, `(SA sample + steps) % bwt_len` of src/fm_index.rs:534.
    /// Passes `hits_out = NULL`: 8 bytes per hit cross PCIe instead of 24.
    pub fn locate_batch_positions(&self, bytes: &[u8], offsets: &[u64]) -> Result<(Vec<u64>, Vec<u64>), AwryError> {
        assert!(!offsets.is_empty());
        // the C side reads bytes[offsets[i]..offsets[i + 1]]: a safe fn must not let bad offsets reach it
        assert!(offsets.windows(2).all(|w| w[0] <= w[1]), "query offsets must be non-decreasing");
        assert!(*offsets.last().unwrap() as usize <= bytes.len(), "query offsets run past the byte buffer");
        let n = offsets.len() - 1;
        let mut hit_off: *mut u64 = std::ptr::null_mut();
        let mut gpos: *mut u64 = std::ptr::null_mut();
        check(unsafe { sys::awry_locate_batch(self.raw(), bytes.as_ptr(), offsets.as_ptr(), n as u64, &mut hit_off, std::ptr::null_mut(), &mut gpos) })?;
        let (off, pos) = unsafe {
            let off = std::slice::from_raw_parts(hit_off, n + 1).to_vec();
            let total = off[n] as usize;
            let pos = if total == 0 { Vec::new() } else { std::slice::from_raw_parts(gpos, total).to_vec() };
            sys::awry_free_buffer(hit_off as *mut std::os::raw::c_void);
            sys::awry_free_buffer(gpos as *mut std::os::raw::c_void);
            (off, pos)
        };
        Ok((off, pos))
    }

    /// Finds the count for the given query (reference: src/fm_index.rs:499-501).  One kernel launch per call: batches
    /// are the way to use a GPU.
    pub fn count_string(&self, query: &str) -> u64 {
        self.try_count_string(query).unwrap_or_else(|e| panic!("{}", e))
    }

    pub fn try_count_string(&self, query: &str) -> Result<u64, AwryError> {
        let mut count = 0u64;
        check(unsafe { sys::awry_count(self.raw(), query.as_ptr(), query.len() as u64, &mut count) })?;
        Ok(count)
    }

    /// The search range of the query (the reference's crate-private `get_search_range_for_string`, src/fm_index.rs:402-438).
    pub fn search_range_for_string(&self, query: &str) -> Result<SearchRange, AwryError> {
        let mut r = sys::awry_range_t::default();
        check(unsafe { sys::awry_search_range(self.raw(), query.as_ptr(), query.len() as u64, &mut r) })?;
        Ok(SearchRange { start_ptr: r.start_ptr, end_ptr: r.end_ptr })
    }

    /// Finds the locations in the original text of all instances of the given query (reference: src/fm_index.rs:516-544).
    pub fn locate_string(&self, query: &str) -> Vec<LocalizedSequencePosition> {
        self.try_locate_string(query).unwrap_or_else(|e| panic!("{}", e))
    }

    pub fn try_locate_string(&self, query: &str) -> Result<Vec<LocalizedSequencePosition>, AwryError> {
        let mut hits: *mut sys::awry_pos_t = std::ptr::null_mut();
        let mut n = 0u64;
        check(unsafe { sys::awry_locate(self.raw(), query.as_ptr(), query.len() as u64, &mut hits, std::ptr::null_mut(), &mut n) })?;
        let out = unsafe {
            let flat: &[sys::awry_pos_t] = if n == 0 { &[] } else { std::slice::from_raw_parts(hits, n as usize) };
            let v = flat.iter().map(|p| LocalizedSequencePosition::new(p.seq_idx as usize, p.local_pos as usize)).collect();
            sys::awry_free_buffer(hits as *mut std::os::raw::c_void);
            v
        };
        Ok(out)
    }

    /// Perform a single SearchRange update using a given symbol (reference: src/fm_index.rs:559-582).
    pub fn update_range_with_symbol(&self, search_range: SearchRange, query_symbol: Symbol) -> SearchRange {
        let mut out = sys::awry_range_t::default();
        let rc = unsafe {
            sys::awry_update_range(
                self.raw(),
                sys::awry_range_t { start_ptr: search_range.start_ptr, end_ptr: search_range.end_ptr },
                query_symbol.ascii(),
                &mut out,
            )
        };
        check(rc).unwrap_or_else(|e| panic!("{}", e));
        SearchRange { start_ptr: out.start_ptr, end_ptr: out.end_ptr }
    }

    /// Finds the row of the symbol that precedes the given search pointer (LF-mapping; reference: src/fm_index.rs:585-593).
    pub fn backstep(&self, search_pointer: SearchPtr) -> SearchPtr {
        let mut out = 0u64;
        check(unsafe { sys::awry_backstep(self.raw(), search_pointer, &mut out) }).unwrap_or_else(|e| panic!("{}", e));
        out
    }

    /// Global text position -> (sequence, offset): largest sequence start <= position.
    pub fn get_seq_location(&self, global_position: usize) -> LocalizedSequencePosition {
        let mut p = sys::awry_pos_t::default();
        check(unsafe { sys::awry_get_seq_location(self.raw(), global_position as u64, &mut p) }).unwrap_or_else(|e| panic!("{}", e));
        LocalizedSequencePosition::new(p.seq_idx as usize, p.local_pos as usize)
    }
}

#[cfg(test)]
mod tests {
    //! The reference's own integration tests (src/fm_index.rs:612-743,1046-1088), restated over this crate's API: counts
    //! and sorted locations of every k-mer of a small random text equal brute force; save / load round-trips.
    //! Need an MI355X and libawry_hip.so at run time.
    use super::*;
    use rayon::prelude::*;
    use std::io::Write;

    fn random_text(n: usize, letters: &[u8], mut seed: u64) -> String {
        let mut s = String::with_capacity(n);
        for _ in 0..n {
            seed = seed.wrapping_mul(6364136223846793005).wrapping_add(1442695040888963407);
            s.push(letters[((seed >> 33) % letters.len() as u64) as usize] as char);
        }
        s
    }

    fn brute(text: &str, q: &str) -> Vec<usize> {
        (0..=text.len().saturating_sub(q.len())).filter(|&i| text[i..].starts_with(q)).collect()
    }

    fn check_index(path: &Path, alphabet: SymbolAlphabet, text: &str, k: usize) {
        let args = FmBuildArgs::new(path.into(), None, Some(8), None, alphabet, None, true);
        let ix = FmIndex::new(&args).expect("unable to build fm index");
        let kmers: Vec<&str> = (0..text.len() - k).map(|i| &text[i..i + k]).collect();
        let counts = ix.parallel_count(kmers.par_iter().copied());
        let locs = ix.parallel_locate(kmers.par_iter().copied());
        for (i, q) in kmers.iter().enumerate() {
            let want = brute(text, q);
            assert_eq!(counts[i] as usize, want.len());
            let mut got: Vec<usize> = locs[i].iter().map(|p| p.local_position()).collect();
            got.sort();
            assert_eq!(got, want);
            assert_eq!(ix.count_string(q), counts[i]);
        }
        let saved = path.with_extension("awry");
        ix.save(&saved).expect("save");
        let loaded = FmIndex::load(&saved).expect("load");
        assert!(loaded == ix);
        assert_eq!(loaded.parallel_count(kmers.par_iter().copied()), counts);
    }

    #[test]
    fn nucleotide_index_matches_brute_force() {
        let text = random_text(1847, b"ACGT", 0);
        let path = std::env::temp_dir().join("awry_shim_test_nucleotide.fasta");
        writeln!(std::fs::File::create(&path).unwrap(), ">seq0\n{}", text).unwrap();
        check_index(&path, SymbolAlphabet::Nucleotide, &text, 24);
    }

    #[test]
    fn amino_index_matches_brute_force() {
        let text = random_text(300, b"ACDEFGHIKLMNPQRSTVWY", 999);
        let path = std::env::temp_dir().join("awry_shim_test_amino.fasta");
        writeln!(std::fs::File::create(&path).unwrap(), ">seq0\n{}", text).unwrap();
        check_index(&path, SymbolAlphabet::Amino, &text, 8);
    }
}
