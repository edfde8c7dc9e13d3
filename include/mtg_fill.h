/*
 * mtg_fill.h -- C ABI of libmtgfill.so: the MI355X-native drop-in for the hot path of `MindTheGap fill`.
 *
 * The reference has no plugin / FFI seam; its de-facto boundary for this path is
 *   (i)  the tool entry      Filler::run(argc, argv) -> Filler::execute   (src/main.cpp:105-120, src/Filler.cpp:136)
 *   (ii) the per-gap call    Filler::gapFillFromSource<span>               (src/Filler.hpp:188-189, src/Filler.cpp:854-1026)
 *   (iii) the gatb Graph it queries: Graph::create / Graph::load / successors / predecessors / contains /
 *        queryAbundance (call sites src/Filler.cpp:210,222,415-428,978)
 * Every entry point below names the reference interface it replaces (paths relative to /root/reference).
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain C types only; every function returns an int status (MTG_OK = 0) unless noted; handles are
 * created by the library and released by the matching *_free; result arenas are library-owned until freed; all
 * functions require a HIP device (gfx950) and return MTG_ERR_NO_DEVICE without one -- there is no CPU fallback.
 * k-mer encoding everywhere: 2 bits per nucleotide, A=0 C=1 T=2 G=3 ((ascii>>1)&3, as gatb), first nucleotide in
 * the most significant bits of a uint64_t; k <= 31.
 */
#ifndef MTG_FILL_H
#define MTG_FILL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    MTG_OK = 0,
    MTG_ERR_NO_DEVICE = 1,   /* no HIP device / HIP runtime failure (message via mtg_last_error) */
    MTG_ERR_ARG = 2,         /* invalid argument (k out of range, null pointer, non-ACGT k-mer, ...) */
    MTG_ERR_IO = 3,          /* cannot read / write a file */
    MTG_ERR_NOMEM = 4,       /* device or host allocation failed */
    MTG_ERR_OVERFLOW = 5,    /* a gap exceeded the largest scratch tier (pathological traversal) */
    MTG_ERR_FORMAT = 6       /* unsupported index container (e.g. a GATB HDF5 graph) */
};

const char* mtg_last_error(void);           /* thread-local message of the last failing call */
int mtg_device_count(void);                 /* number of visible HIP devices (0 if none); not a status */
int mtg_set_device(int device);             /* device used by subsequent calls of this thread */

/* ------------------------------------------------------------------------------------------------------------
 * Index = gatb Graph (solid canonical k-mers + abundance), device resident.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct mtg_index mtg_index;

typedef struct mtg_index_info {
    int k;
    int abundance_min;          /* threshold used ("abundance_min (used)", src/Filler.cpp:419-424) */
    int abundance_auto;         /* auto-inferred cut-off or -1 (src/Filler.cpp:415) */
    uint64_t nb_solid_kmers;    /* "kmers_nb_solid"  (src/Filler.cpp:427) */
    uint64_t nb_branching;      /* "nb_branching"    (src/Filler.cpp:428) */
    uint64_t device_bytes;      /* HBM held by the index */
    uint64_t adj_buckets, abnd_buckets;
    uint32_t adj_bucket_bytes, abnd_bucket_bytes; /* one bucket = one read of the walk / of an abundance query */
    uint64_t bloom_blocks;      /* 64-byte blocks of the Bloom filter (0 = not built) */
    uint32_t bloom_minimizer;   /* minimizer length selecting the block */
    uint64_t nb_unitigs;        /* maximal simple paths (>= 2 k-mers) held in the unitig store */
    uint64_t unitig_bytes;      /* HBM held by the unitig store (2-bit sequences + one abundance byte per k-mer) */
    uint64_t nb_saturated;      /* solid k-mers whose abundance exceeds 255 and is stored as 255 (gatb reports discretised values above ~70:
                                   coverage statistics of very deep regions may differ from the reference's) */
    uint32_t sparse;            /* 1: the sparse form -- the ADJ table holds every second junction of a stored unitig (and all others), the ABND
                                   table only the k-mers of no stored unitig; the rest is read off the unitig store */
    uint32_t pad_;
    uint64_t nb_kmers_outside_unitigs;
} mtg_index_info;

/* Graph::create(props) from read files (src/Filler.cpp:172-213): paths_csv = comma separated FASTA/FASTQ(.gz);
 * abundance_min < 0 = "auto" (src/Filler.cpp:106); abundance_max <= 0 = unlimited. */
int mtg_index_create_from_reads(const char* paths_csv, int k, int abundance_min, int abundance_max, mtg_index** out);
/* Graph from an already counted solid set (host arrays; canonical k-mers, abundance >= 1). */
int mtg_index_create_from_kmers(const uint64_t* canon_kmers, const uint32_t* abundance, size_t n, int k, mtg_index** out);
/* Graph whose nodes are all k-mers of the given sequences (2-bit packed, 32 nt per uint64_t word, nt i at bits
 * 2*(i%32); seq s occupies words [word_off[s], ...) and has len[s] nts; arrays in DEVICE memory).  Abundance of a
 * k-mer (deterministic): abund_span > 0: abund_lo + hash(k-mer) % abund_span; abund_span == 0: a Poisson(24) variate drawn from the hash
 * (SURVEY.md 8d), at least abund_lo.  Used for the synthetic benchmark sets.  Sequences of any length (shorter than k: ignored; a donor of a few
 * chromosome-sized sequences is taken in pieces internally); total_kmers_upper_bound >= the sum of max(len - k + 1, 0). */
int mtg_index_create_from_packed_device(const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq,
                                        uint64_t total_kmers_upper_bound, int k, uint32_t abund_lo, uint32_t abund_span, mtg_index** out);
/* Graph::load / save (src/Filler.cpp:222): this library's own container; a GATB .h5 gives MTG_ERR_FORMAT. */
int mtg_index_load(const char* path, mtg_index** out);
int mtg_index_save(const mtg_index* idx, const char* path);
/* A copy of the index on another device of the node (tables and unitig store copied device to device, no rebuild): what the tool uses to
 * run on every GPU, the reference's Dispatcher threads (src/Filler.cpp:824,844) becoming one host thread per device.  The copy is an
 * independent index: free it with mtg_index_free. */
int mtg_index_replicate(const mtg_index* idx, int device, mtg_index** out);
int mtg_index_get_info(const mtg_index* idx, mtg_index_info* info);
/* How Graph::create / Graph::load (src/Filler.cpp:172-226) went on the device: one record per phase of the construction (kernel or group of
 * kernels, in order) with its device time and the bytes the implemented layout has to move for it (0: not accounted), the most device
 * memory the construction held at any moment, and its whole duration.  out may be NULL (n receives the number of phases). */
typedef struct mtg_build_phase {
    char name[32];
    double ms;
    uint64_t bytes;   /* bytes of the implemented layout the phase must read + write (random accesses counted as the lines they touch) */
    uint64_t units;   /* what the phase processed: k-mers, junctions, table slots ... (named in DESIGN.md section 3) */
} mtg_build_phase;
int mtg_index_build_profile(const mtg_index* idx, mtg_build_phase* out, size_t cap, size_t* n, uint64_t* peak_device_bytes, double* total_ms);
void mtg_index_free(mtg_index* idx);

/* Batched graph queries (host arrays in, host arrays out).  kmers[] in any orientation.
 * contains   : Graph::contains            -> 1/0
 * abundance  : Graph::queryAbundance      (src/Filler.cpp:978), 0 if absent, saturates at 255
 * neighbors  : Graph::successors / predecessors: bit nt of succ[i] set iff kmer[1:]+nt is solid (order A,C,T,G) */
int mtg_index_contains(const mtg_index* idx, const uint64_t* kmers, size_t n, uint8_t* out);
int mtg_index_abundance(const mtg_index* idx, const uint64_t* kmers, size_t n, uint32_t* out);
int mtg_index_neighbors(const mtg_index* idx, const uint64_t* kmers, size_t n, uint8_t* succ, uint8_t* pred);

/* Membership of every k-mer along sequences = Graph::contains per position (the access pattern of the reference's `find` scan,
 * src/FindBreakpoints.hpp:851-853,1012-1046).  A rolling 2-bit k-mer per position, probed against the minimizer-blocked Bloom filter
 * of the index (blocks staged in LDS, one coalesced 64-byte read per run of k-mers sharing a minimizer).
 * mode 0: Bloom answer only (no false negatives); mode 1: exact (Bloom pre-filter, positives confirmed in the abundance table).
 * out[s] receives len(seqs[s]) - k + 1 bytes (0/1); k-mers with a non-ACGT character give 0. */
typedef struct mtg_scan_stats {
    uint64_t n_kmers, bloom_positive, confirmed, blocks_staged;
    double kernel_ms;
} mtg_scan_stats;
int mtg_index_scan_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, int mode, uint8_t* const* out, mtg_scan_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (layout of mtg_index_create_from_packed_device);
 * bit (p % 64) of d_out_bits[word_off[s] + p / 64] = membership of the k-mer starting at nt p of sequence s */
int mtg_index_scan_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, int mode,
                                 uint64_t* d_out_bits, mtg_scan_stats* st);

/* Profile of sequences against the graph: per position membership, abundance and degrees, and the maximal runs of absent k-mers -- what the
 * reference's `find` scan reads per reference position (src/FindBreakpoints.hpp:560-622,1012-1046), without its classification rules.
 * One pass of the scan's tile structure (Bloom pre-filter in LDS, positives confirmed exactly); confirmed positions take their abundance and
 * their neighbour masks from the look-ups of mtg_index_abundance / mtg_index_neighbors.  One word per position p of sequence s:
 *   bits  0-7   abundance, saturating at 255 as mtg_index_abundance; 0 if absent
 *   bits  8-11  successor mask of the k-mer as read along the sequence (bit order of mtg_index_neighbors)
 *   bits 12-15  predecessor mask, same convention
 *   bit  16     valid: all k characters are nucleotides (the character rule of mtg_index_scan_sequences)
 *   bit  17     present: valid and in the graph (exact)
 * Absent and invalid positions carry 0 in bits 0-15 (the reference stores nb_in = nb_out = 0 there, :1018-1027).
 * A run is a maximal stretch of consecutive positions of one sequence that are valid and absent.  An invalid position is in no run: it ends
 * one and does not count as a bound.  flags bit 0: position start - 1 exists and is present; bit 1: position start + length exists and is
 * present.  Runs come in ascending (seq, start) order, extracted and ordered on the device.
 * *n_runs is always the total number of runs; when it exceeds runs_cap the first runs_cap runs are written and the call still returns MTG_OK
 * (the snprintf convention).  out[s] receives max(len(seqs[s]) - k + 1, 0) words; out may be NULL (runs and statistics only), runs may be
 * NULL when runs_cap is 0, st may be NULL.  nseq = 0 and sequences shorter than k are legal. */
#define MTG_PROFILE_ABUNDANCE(w) ((w) & 255u)
#define MTG_PROFILE_SUCC(w) (((w) >> 8) & 15u)
#define MTG_PROFILE_PRED(w) (((w) >> 12) & 15u)
#define MTG_PROFILE_VALID(w) (((w) >> 16) & 1u)
#define MTG_PROFILE_PRESENT(w) (((w) >> 17) & 1u)
typedef struct mtg_run { uint32_t seq, start, length, flags; } mtg_run;
typedef struct mtg_profile_stats { uint64_t n_positions, n_valid, n_present, n_runs, longest_run; double kernel_ms; } mtg_profile_stats;
int mtg_index_profile_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, uint32_t* const* out, mtg_run* runs, size_t runs_cap, size_t* n_runs,
                                mtg_profile_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (layout of mtg_index_create_from_packed_device; no invalid positions): the word of
 * position p of sequence s goes to d_out[d_pos_off[s] + p] (d_out and d_pos_off may be NULL), the runs to the device array d_runs */
int mtg_index_profile_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, const uint64_t* d_pos_off,
                                    uint32_t* d_out, mtg_run* d_runs, size_t runs_cap, size_t* n_runs, mtg_profile_stats* st);

/* `find` for homozygous insertions: the gaps of the reference's scan (src/FindBreakpoints.hpp:560-622 -- not the profile's runs: a single
 * present position does not end a gap, see csrc/mtg_find_gaps.h) judged by its gap observers FindSmallCleanInsertion, FindSmallFuzzyInsertion
 * (src/FindSmallInsertion.hpp), FindCleanInsertion and FindFuzzyInsertion (src/FindInsertion.hpp), in that order; no other observer runs.
 * A gap of L positions whose first solid position behind it is e has the repeat r = k - 1 - L; with 0 <= r <= max_repeat and a valid k-mer
 * right before it, it is an insertion of 1-2 nt when one of the 20 strings A, C, G, T, AA .. TT between the left k-mer and the k
 * nucleotides at e + r spells k solid windows (the first such string), else an insertion site.  One record per call:
 *   pos    0-based, as the observers pass it to writeBreakpoint / writeIndel: e - 1 for an insertion, e - 1 + r for a site
 *   kind   0 insertion site, 1 insertion of 1-2 nt
 *   repeat r (the FUZZY / fuzzy_ field)
 *   left, right   positions in the sequence of the two k-mers as written (right = e + r)
 *   ins    index 0..19 of the inserted string in that order; 0 for sites
 * Records come in the order of the scan (ascending seq, then e), ordered on the device.  max_repeat < 0 is refused; values above k - 2 act as k - 2.
 * *n_calls is always the total; when it exceeds cap the first cap records are written and the call still returns MTG_OK.  calls may be NULL
 * when cap is 0, st may be NULL.  The character rule is that of mtg_index_profile_sequences. */
typedef struct mtg_find_call { uint32_t seq, pos, kind, repeat, left, right, ins; } mtg_find_call;
typedef struct mtg_find_stats {
    uint64_t n_positions, n_gaps /* calls of the gap observers */, n_candidates /* of those, r in range and the left k-mer valid */;
    uint64_t n_homo_clean, n_homo_fuzzy /* sites */, n_small_clean, n_small_fuzzy /* insertions of 1-2 nt, r = 0 / r > 0 */;
    double kernel_ms;
} mtg_find_stats;
int mtg_index_find_homo_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, int max_repeat, mtg_find_call* calls, size_t cap, size_t* n_calls,
                                  mtg_find_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (layout of mtg_index_profile_packed_device; no invalid positions); d_calls is a device array */
int mtg_index_find_homo_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, int max_repeat,
                                      mtg_find_call* d_calls, size_t cap, size_t* n_calls, mtg_find_stats* st);

/* `find` for heterozygous insertions: the reference's k-mer observer FindHeteroInsertion (src/FindHeteroInsertion.hpp:46-174) and no other, as
 * it runs under -hete-only and -insert-only.  At a valid position p whose k-mer has in-degree 2 and a prefix (k-1)-mer that is not repeated,
 * it looks for the first i in 0 .. max_repeat whose history slot p - k + i holds a k-mer of out-degree 2 with a suffix (k-1)-mer that is not
 * repeated (the history is the reference's ring of 256 slots, written at valid positions only: see csrc/mtg_find_het.h).  With the k
 * nucleotides at p + i as the right k-mer it is an insertion of 1-2 nt when one of the 20 strings assembles (the rule of
 * mtg_index_find_homo_sequences), else a site unless more than branching_filter of the 100 history slots before the window hold a k-mer with a
 * degree above 1 (branching_filter < 0: no filter).  A site silences the observer for the next max_repeat valid positions.  Records as above:
 *   kind   2 heterozygous site, 3 heterozygous insertion of 1-2 nt
 *   pos    p - 1 for an insertion, p - 1 + i for a site;  repeat = i;  left = position of the left k-mer's text;  right = p + i;  ins as above
 * in the order of the scan (ascending seq, then p).  repeated[s] holds one byte (0 / 1) per (k-1)-mer position of sequence s, len - k + 2 of
 * them -- what mtg_index_scan_sequences returns for an index of k - 1 that holds the repeated (k-1)-mers; repeated == NULL: nothing is
 * repeated (entries of sequences shorter than k are not read).  The reference asks a Bloom filter of the repeated (k-1)-mers; a false positive
 * of it can silence a site there that is called here.  max_repeat, cap, *n_calls, calls, st and the character rule as for
 * mtg_index_find_homo_sequences. */
typedef struct mtg_find_het_stats {
    uint64_t n_positions, n_candidates /* positions where a qualifying i exists, `recent` aside */, n_raw_sites /* of those, sites judged as if nothing were recent */;
    uint64_t n_filtered /* sites refused by the branching filter */, n_suppressed /* sites and insertions silenced by a site before them */;
    uint64_t n_het_clean, n_het_fuzzy /* sites called, i = 0 / i > 0 */, n_het_small /* insertions of 1-2 nt called */;
    double kernel_ms;
} mtg_find_het_stats;
int mtg_index_find_het_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, const uint8_t* const* repeated, int max_repeat, int branching_filter,
                                 mtg_find_call* calls, size_t cap, size_t* n_calls, mtg_find_het_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (no invalid positions); d_repeat_bits: the repeat plane in the layout of
 * mtg_index_scan_packed_device's output for an index of k - 1 (bit q % 64 of d_repeat_bits[word_off[s] + q / 64]), or NULL; d_calls is a device array */
int mtg_index_find_het_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, const uint64_t* d_repeat_bits,
                                     int max_repeat, int branching_filter, mtg_find_call* d_calls, size_t cap, size_t* n_calls, mtg_find_het_stats* st);

/* `find` for homozygous deletions: the reference's gap observer FindDeletion (src/FindDeletion.hpp:58-188) and no other, on the gaps of
 * mtg_index_find_homo_sequences.  A reported gap of L >= k - max_repeat positions (no upper bound) with a valid k-mer right before it (begin,
 * at left) and the k-mer right behind it (end, at right = left + 1 + L): r = the largest i in max_repeat .. 1 with the last i nucleotides of
 * begin equal to the first i of end, else 0.  When every k-mer of begin[0 : k - r] + end is in the graph it is a deletion of
 * del_size = L - k + r + 1 nucleotides; else, with r > 0, when every k-mer of begin + end is: a deletion of L - k + 1 with r = 0 (counted in
 * n_fallback); del_size <= 0 is no deletion.  The observer reads no history and does not change the scan.  Records as above:
 *   kind   4 deletion
 *   pos    0-based position of the nucleotide before the deleted text (left + k - 1 - r; the VCF's POS is pos + 1);  repeat = r
 *   left, right   positions of the two k-mers;  ins = del_size
 * in the order of the scan (ascending seq, then right).  In a combined run the reference asks this observer first: a gap it calls is not
 * seen by the insertion observers (the tool drops their calls with the same (seq, left)).  max_repeat, cap, *n_calls, calls, st and the
 * character rule as for mtg_index_find_homo_sequences. */
typedef struct mtg_find_del_stats {
    uint64_t n_positions, n_gaps /* calls of the gap observers */, n_candidates /* of those, both k-mers valid and L >= k - max_repeat */;
    uint64_t n_del_clean, n_del_fuzzy /* deletions called, r = 0 / r > 0 */, n_fallback /* begin + end held after the shorter text failed */, n_calls;
    double kernel_ms;
} mtg_find_del_stats;
int mtg_index_find_del_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, int max_repeat, mtg_find_call* calls, size_t cap, size_t* n_calls,
                                 mtg_find_del_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (no invalid positions); d_calls is a device array */
int mtg_index_find_del_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, int max_repeat,
                                     mtg_find_call* d_calls, size_t cap, size_t* n_calls, mtg_find_del_stats* st);

/* `find` for isolated homozygous SNPs: the reference's gap observer FindSoloSNP (src/FindSNP.hpp:297-355 with snp_at_end, :139-208) and no
 * other, on the gaps of mtg_index_find_homo_sequences.  A reported gap of exactly k positions from `start` with a valid k-mer right before it:
 * its k k-mers are those that cover the position g = start + k - 1.  With ref the nucleotide at g, the call is the first of the other three
 * nucleotides in the order A, C, T, G for which all k k-mers, g replaced by it, are in the graph; with none there is no call.  The observer
 * leaves the scan alone.  (In the reference a call also corrects the k-mer history that the heterozygous observer reads: not done, the
 * heterozygous entry knows nothing of these calls.)  FindMultiSNP, which takes the longer gaps, is mtg_index_find_msnp_sequences; FindMultiSNPrev is mtg_index_find_msnp_rev_sequences.  Records as above:
 *   kind   5 SNP
 *   pos    g, 0-based (the VCF's POS is pos + 1);  repeat = 0
 *   left, right   start - 1 and start + k, the positions of the two k-mers
 *   ins    ALT's ASCII code in bits 0-7, REF's in bits 8-15, both upper case whatever the text's case is
 * in the order of the scan (ascending seq, then right).  In a combined run the reference asks this observer before the deletion observer: a
 * gap it calls is not seen by the others (the tool drops deletion calls with the same (seq, left); an insertion candidate is shorter than k).
 * max_repeat plays no part in the rule and is checked as elsewhere; cap, *n_calls, calls, st and the character rule as for
 * mtg_index_find_homo_sequences. */
typedef struct mtg_find_snp_stats {
    uint64_t n_positions, n_gaps /* calls of the gap observers */, n_candidates /* of those, both k-mers valid and L = k */, n_calls;
    double kernel_ms;
    uint64_t reserved[3]; /* (the size of mtg_find_del_stats) */
} mtg_find_snp_stats;
int mtg_index_find_snp_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, int max_repeat, mtg_find_call* calls, size_t cap, size_t* n_calls,
                                 mtg_find_snp_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (no invalid positions); d_calls is a device array */
int mtg_index_find_snp_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, int max_repeat,
                                     mtg_find_call* d_calls, size_t cap, size_t* n_calls, mtg_find_snp_stats* st);

/* `find` for close homozygous SNPs: the reference's gap observer FindMultiSNP (src/FindSNP.hpp:435-564 with snp_at_end, :139-208, and
 * correct_history) and no other, on the gaps of mtg_index_find_homo_sequences.  A reported gap of L > k + snp_min_val positions from `start`
 * with a valid k-mer right before it is walked from the left with a cursor c = 0 and a private copy T of its text; while c != L:
 *   g = start + c + k - 1, ref = T[g]; for each of the other three nucleotides a, f(a) = the number of leading windows j = 0, 1, ..
 *   < min(k, L - c + 1) in the graph, window j being the k-mer of T at start + c + j with g replaced by a; M = max f.  The winner is the first
 *   nucleotide in the order A, C, T, G with f = k when M = k, else the last one in that order with f = M.  M < snp_min_val: stop.
 *   c + M > L: stop.  Else a SNP at g, REF ref, ALT the winner; T[g] = winner (the next step reads the corrected text); c += M.
 * consumed = the final c: L = the gap is taken, 0 < c < L = in part, 0 = untouched.  (In the reference a gap taken in part reaches the later
 * observers shortened and with a corrected kmer_begin, and a call corrects the history that the heterozygous observer reads: not done, the
 * other entries know nothing of these calls.)  DEVIATION: the reference keeps the text in a ring of 256 k-mers addressed by unsigned char;
 * from L = 255 on the ring has been overwritten and the reference reports positions it did not look at (23 of 29 such gaps of a random
 * set differ from the rule above).  Gaps of 255 positions and more are not judged: counted in n_long, no call.  FindMultiSNPrev, which
 * walks a gap from the right, is mtg_index_find_msnp_rev_sequences below.  Records as above:
 *   kind   6 SNP of a multi-SNP gap (its VCF line is that of kind 5)
 *   pos    g, 0-based;  repeat = 0
 *   left, right   start - 1 and start + L, the positions of the gap's two k-mers, the same for every SNP of the gap
 *   ins    as for kind 5
 * in the order of the scan (ascending seq, then gap, then pos).  snp_min_val: 1 .. k (the reference's default is 5), else MTG_ERR_ARG.
 * gaps (gap_cap records; may be NULL with gap_cap = 0) receives one record per candidate gap in scan order, the long ones with consumed = 0;
 * *n_gaps (may be NULL) is their total, which can exceed gap_cap as *n_calls can exceed cap.  max_repeat plays no part in the rule and is
 * checked as elsewhere; cap, *n_calls, calls, st and the character rule as for mtg_index_find_homo_sequences. */
typedef struct mtg_find_msnp_gap {
    uint32_t seq, start, length, consumed, n_snps;
} mtg_find_msnp_gap;
typedef struct mtg_find_msnp_stats {
    uint64_t n_positions, n_gaps /* calls of the gap observers */, n_candidates /* of those, both k-mers valid and L > k + snp_min_val */, n_calls;
    double kernel_ms;
    uint64_t n_full /* gaps with consumed = L */, n_partial /* 0 < consumed < L */, n_long /* L >= 255: not judged */;
} mtg_find_msnp_stats;
int mtg_index_find_msnp_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, int max_repeat, int snp_min_val, mtg_find_call* calls, size_t cap, size_t* n_calls,
                                  mtg_find_msnp_gap* gaps, size_t gap_cap, size_t* n_gaps, mtg_find_msnp_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (no invalid positions); d_calls and d_gaps are device arrays */
int mtg_index_find_msnp_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, int max_repeat, int snp_min_val,
                                      mtg_find_call* d_calls, size_t cap, size_t* n_calls, mtg_find_msnp_gap* d_gaps, size_t gap_cap, size_t* n_gaps, mtg_find_msnp_stats* st);

/* The same with the reverse pass: the reference's FindMultiSNPrev (src/FindSNP.hpp:593-709 with snp_at_begin, :219-293), which it asks right
 * behind FindMultiSNP.  passes: 1 = the forward pass alone (calls, statistics and the first five record fields of
 * mtg_index_find_msnp_sequences, bit for bit), 2 = the reverse pass alone, 3 = forward, then reverse on what is left; anything else is
 * MTG_ERR_ARG.  With c what the forward pass consumed (0 when it is not run), the reverse pass is asked only if c != L and
 * L - c > k + snp_min_val, the reference's own entry test on the shrunken gap.  It works on the residual gap start' = start + c, L' = L - c,
 * on the same private text T with the forward substitutions in place, with a cursor d = 0; while d != L':
 *   q = start + L - 1 - d, ref = T[q]; for each of the other three nucleotides a, f(a) = the number of leading windows j = 0, 1, ..
 *   < min(k, L' - d + 1) in the graph, window j being the k-mer of T at q - j with q (its nucleotide j) replaced by a.  Window j = L' - d is
 *   the k-mer at start' - 1, the left anchor, and it decides: if it holds, M = L' - d + 1 and the chain stops without a call; if it fails,
 *   M = L' - d and the gap is taken whole.  M = max f and the winner as in the forward pass.  M < snp_min_val: stop.  d + M > L': stop.  Else
 *   a SNP at q, REF ref, ALT the winner; T[q] = winner; d += M.
 * consumed_rev = the final d.  The gap is full if c + d = L, partial if 0 < c + d < L: n_full and n_partial go by c + d, n_calls counts both
 * passes.  The reverse pass reads the text [start - 1, start + L + k - 1), one nucleotide to the left of the forward text.
 * DEVIATIONS: gaps of 255 positions and more are judged by neither pass (n_long, consumed 0, no call), as above.  THE RING INDICES COUNT AS
 * RESTORED AFTER A GAP: after a partial take the reference subtracts the consumed length from m_position, m_het_kmer_end_index and
 * m_het_kmer_begin_index (:672-674) and restores m_position alone (src/FindBreakpoints.hpp:441-446), so its ring is addressed shifted from
 * then on; a gap that starts exactly two positions behind a gap the reverse pass took in part reads a stale left anchor there (reverse pass
 * alone: 1 of 1 200 random cases differs, one with such a pair of gaps; forward then reverse: none).  The rule here is
 * the pure function of the gap.  (A gap taken in part would reach the deletion and insertion observers shortened on both sides and with a
 * corrected kmer_end: not done.)  Records as above, and
 *   kind   7 SNP of the reverse pass (its VCF line is that of kind 5)
 *   pos    q, 0-based;  repeat = 0
 *   left, right   start + c - 1 and start + L, the two k-mers of the residual gap
 *   ins    as for kind 5
 * in the order of the scan; the calls of one gap in the order they are made: the forward ones ascending, then the reverse ones DESCENDING in
 * pos.  Everything else as for mtg_index_find_msnp_sequences. */
typedef struct mtg_find_msnp_rev_gap {
    uint32_t seq, start, length, consumed, n_snps, consumed_rev, n_snps_rev;
} mtg_find_msnp_rev_gap;
int mtg_index_find_msnp_rev_sequences(const mtg_index* idx, const char* const* seqs, size_t nseq, int max_repeat, int snp_min_val, int passes, mtg_find_call* calls, size_t cap,
                                      size_t* n_calls, mtg_find_msnp_rev_gap* gaps, size_t gap_cap, size_t* n_gaps, mtg_find_msnp_stats* st);
/* same on 2-bit packed sequences already in DEVICE memory (no invalid positions); d_calls and d_gaps are device arrays */
int mtg_index_find_msnp_rev_packed_device(const mtg_index* idx, const uint64_t* d_words, const uint64_t* d_word_off, const uint32_t* d_len, size_t nseq, int max_repeat, int snp_min_val,
                                          int passes, mtg_find_call* d_calls, size_t cap, size_t* n_calls, mtg_find_msnp_rev_gap* d_gaps, size_t gap_cap, size_t* n_gaps,
                                          mtg_find_msnp_stats* st);

/* ------------------------------------------------------------------------------------------------------------
 * Gap filling = Filler::gapFillFromSource over a batch of gaps.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct mtg_params {
    int max_nodes;              /* -max-nodes  (100),   src/Filler.cpp:101 */
    int max_depth;              /* -max-length (10000), src/Filler.cpp:100 */
    int nb_mis_allowed;         /* 2, src/Filler.cpp:56 */
    int end_rule_nonbranching;  /* 0; see SURVEY.md A.5(i) */
    int nb_host_threads;        /* host workers of a batch (0 = the library's pool: the CPUs the process may use, at most 64) */
} mtg_params;
void mtg_default_params(mtg_params* p);

/* one call of gapFillFromSource (arguments as src/Filler.hpp:188-189) */
typedef struct mtg_gap {
    const char* source;               /* sourceSequence (first k nts seed the traversal) */
    const char* target;               /* targetSequence: the early-stop pattern R */
    int n_targets;                    /* targetDictionary, in the caller's iteration order */
    const char* const* target_seqs;   /*   key: k-mer string */
    const char* const* target_names;  /*   value.first */
    const uint8_t* target_is_rc;      /*   value.second */
    int is_anchor_repeated;
    int reverse;
} mtg_gap;

typedef struct mtg_filled {           /* filled_insertion_t, src/Utils.hpp:46-104 */
    const char* seq;                  /* NUL terminated, owned by the result arena */
    int nb_errors_in_anchor;
    int target_index;                 /* index into the gap's targetDictionary */
    float avg_coverage, median_coverage;
    int qual, solution_count, solution_rank;
} mtg_filled;

typedef struct mtg_gap_result {
    int nb_nodes;                     /* infostring fields, src/IGraphOutput.cpp:82-83, src/Filler.cpp:905,1012-1016 */
    int total_nt;
    int nb_terminal;
    int has_solution_counts;          /* whether the two fields below are appended to the infostring */
    int nb_total_filled, nb_reported;
    int n_filled;
    const mtg_filled* filled;         /* appended to filledSequences */
    const char* extension;            /* extensionSequence ("" when solutions exist) */
} mtg_gap_result;

typedef struct mtg_results mtg_results;
int mtg_fill_batch(const mtg_index* idx, const mtg_params* p, const mtg_gap* gaps, size_t n, mtg_results** out);
/* The same, and the filled sequences of the batch also laid out in seq_out: NUL-terminated, in gap order (solution order within a gap),
 * *seq_bytes in total -- the form in which results travel between ranks.  In the common case they are decoded there directly (the
 * results then point into seq_out, which must stay untouched until mtg_results_free); MTG_ERR_ARG when cap is too small (32 bytes per
 * packed word of contig plus one per gap always suffice: a little over the sum of the insert lengths). */
int mtg_fill_batch_serial(const mtg_index* idx, const mtg_params* p, const mtg_gap* gaps, size_t n, char* seq_out, uint64_t cap, uint64_t* seq_bytes,
                          mtg_results** out);
/* A batch marshalled ahead of time and kept in device memory: what a caller that fills the same gaps more than once, or reads its
 * breakpoints while an earlier batch is still on the device, would use instead of mtg_fill_batch (which does exactly this and then
 * forgets the batch).  `gaps` and every string it points to must stay alive and unchanged for as long as the batch is used.  A batch can
 * be filled by several threads at once.  Its device copies live on the device of `idx`: filling it with an index of another device (a
 * replica made by mtg_index_replicate), or with another nb_mis_allowed than it was prepared with, is refused with MTG_ERR_ARG. */
typedef struct mtg_batch mtg_batch;
int mtg_batch_prepare(const mtg_index* idx, const mtg_params* p, const mtg_gap* gaps, size_t n, mtg_batch** out);
void mtg_batch_free(mtg_batch* b);
int mtg_fill_prepared(const mtg_index* idx, const mtg_params* p, const mtg_batch* b, mtg_results** out);
int mtg_fill_prepared_serial(const mtg_index* idx, const mtg_params* p, const mtg_batch* b, char* seq_out, uint64_t cap, uint64_t* seq_bytes, mtg_results** out);
/* The same with the serialised sequences produced in DEVICE memory: d_seq_out is a buffer of `cap` bytes on the index's device (a consumer
 * on the device, or the send buffer of a gather over RCCL / xGMI).  host_copy == NULL: they stay there only -- the ASCII never crosses PCIe, the
 * records come to the host as always and the `seq` pointers of their filled sequences are device addresses into d_seq_out.  host_copy != NULL
 * (cap bytes, page-locked for speed): they are copied there as well, by the batch's own stream, and the records point into host_copy as
 * with mtg_fill_prepared_serial.  Both buffers are complete when the call returns. */
int mtg_fill_prepared_serial_device(const mtg_index* idx, const mtg_params* p, const mtg_batch* b, char* d_seq_out, uint64_t cap, char* host_copy, uint64_t* seq_bytes,
                                    mtg_results** out);
/* The same, and the whole batch -- records AND sequences -- also in relocatable form (mtg_wire_* below), tagged, in DEVICE memory: d_wire is a
 * buffer of `cap` bytes on the index's device, typically the send buffer of a gather over RCCL / xGMI.  The result kernel writes the
 * payload there next to the records (no host pass); the results come to the host as with mtg_fill_prepared.  The payload is complete when
 * the call returns. */
int mtg_fill_prepared_wire_device(const mtg_index* idx, const mtg_params* p, const mtg_batch* b, uint64_t tag, void* d_wire, uint64_t cap, uint64_t* wire_bytes, mtg_results** out);
/* A batch of gapFillFromSource calls whose strings lie in ONE block of text, the way a reader of a breakpoint file has them: strings are
 * (offset, length) pairs into the block, no pointer per string, no NUL terminators.  The library copies the block and the offset arrays into
 * page-locked memory, sends them up and ENCODES ON THE DEVICE (source k-mers, early-stop patterns, dictionary keys: k_marshal_text,
 * k_marshal_targets) -- the host does no per-string work, so a caller with one or two threads feeds the device as fast as a prepared batch
 * does.  Results exactly as mtg_fill_batch for the same strings.  Every offset + length must lie inside the block (MTG_ERR_ARG otherwise);
 * a source shorter than k is MTG_ERR_ARG as in mtg_fill_batch.  The block and the arrays must stay unchanged until the call returns (the
 * rare multi-contig gap reads its strings again). */
typedef struct mtg_text_gaps {
    const char* text;                 /* the block */
    uint64_t text_bytes;
    uint64_t n;                       /* gaps */
    const uint64_t* source_off;       /* sourceSequence of gap i = text[source_off[i], + source_len[i]) */
    const uint32_t* source_len;
    const uint64_t* pattern_off;      /* targetSequence: the early-stop pattern R */
    const uint32_t* pattern_len;
    const uint32_t* dict_first;       /* n + 1 entries: targetDictionary of gap i = entries [dict_first[i], dict_first[i + 1]) of the arrays below, in iteration order */
    const uint64_t* dict_seq_off;     /*   key: k-mer string */
    const uint32_t* dict_seq_len;
    const uint64_t* dict_name_off;    /*   value.first */
    const uint32_t* dict_name_len;
    const uint8_t* dict_is_rc;        /*   value.second (NULL: all 0) */
    const uint8_t* gap_flags;         /* per gap, bit 0: is_anchor_repeated, bit 1: reverse (NULL: all 0) */
} mtg_text_gaps;
int mtg_fill_text(const mtg_index* idx, const mtg_params* p, const mtg_text_gaps* g, mtg_results** out);
/* A caller that keeps its text where it is for many batches (a mapped or fully read breakpoint file) can page-lock it once: the block of a
 * mtg_text_gaps that lies inside a registered range goes to the device straight from the caller's memory, without the copy into the
 * library's page-locked block (13 MB per 100 000 sites).  The offset arrays are still copied (they are small).  The range must stay
 * registered and unchanged while calls that use it run.  MTG_ERR_ARG: the range cannot be page-locked (or overlaps a registered one). */
int mtg_host_register(void* p, size_t bytes);
int mtg_host_unregister(void* p);
/* mtg_fill_text for the gaps of BREAKPOINT sites (one-entry dictionaries), and the text the tool's writers add to its output files for them
 * -- writeFilledBreakpoint (src/Filler.cpp:1029-1093), the info line, writeVcf (:1095-1214) -- FORMATTED ON THE DEVICE from the records and
 * sequences the result kernel has just written there: what crosses PCIe is the files' next bytes, and the host only writes them.
 * name_off / name_len: breakpointName of site i = text[name_off[i], + name_len[i]) (the left record's header up to its first space).
 * The device writes the SIMPLE sites -- one solution, found on the common path of this (forward) attempt; every other site (no solution: the
 * caller's reverse attempt decides; several solutions; a record the host wrote) is listed in complex_sites with the offsets where the
 * caller's own text for it belongs, and its record is in *out as always (the ASCII arena of the simple sites is NOT brought to the host:
 * their records' seq pointers must not be followed).  *text: NULL for a new object, or one to use again (its arenas are page-locked). */
typedef struct mtg_formatted mtg_formatted;
typedef struct mtg_formatted_view {
    const char* text[3];            /* FASTA, info, VCF bytes of the simple sites, in site order */
    uint64_t bytes[3];
    uint64_t n_sites, n_simple;
    const uint32_t* complex_sites;  /* ascending */
    const uint64_t* complex_off[3]; /* complex_off[s][j]: bytes of text[s] that precede the text of site complex_sites[j] */
    uint64_t n_complex;
    double kernel_ms;               /* HIP-event time of the three formatting kernels */
} mtg_formatted_view;
int mtg_fill_text_formatted(const mtg_index* idx, const mtg_params* p, const mtg_text_gaps* g, const uint64_t* name_off, const uint32_t* name_len, mtg_results** out, mtg_formatted** text);
int mtg_formatted_get(const mtg_formatted* t, mtg_formatted_view* v);
void mtg_formatted_free(mtg_formatted* t);
/* and the filled sequences laid out in seq_out as with mtg_fill_batch_serial */
int mtg_fill_text_serial(const mtg_index* idx, const mtg_params* p, const mtg_text_gaps* g, char* seq_out, uint64_t cap, uint64_t* seq_bytes, mtg_results** out);
/* ---- Contig mode at assembly scale: ONE dictionary of all targets, resident on the device, instead of a copy per seed.
 * The reference builds the dictionary of all contig-end k-mers once (src/Filler.cpp:755-829) and hands every seed a copy without the seed's own
 * entries (:522-533).  mtg_fill_seeds gives the same results as mtg_fill_batch with those per-seed dictionaries, with these rules:
 *   - the table: entries [0, n) in the caller's iteration order of the dictionary of all targets (key, value.first, value.second);
 *   - a seed's dictionary: the table without its `excluded` entries, iterating in the order of a fresh std::unordered_map<std::string, ...>
 *     into which the remaining entries were inserted in table order (what the reference's per-seed copy does);
 *   - a seed's early-stop pattern R (targetSequence): the keys of its remaining entries, concatenated in table order;
 *   - keys of any length: a key shorter than k never matches as a target (as with mtg_fill_batch), R is cut at the real key lengths;
 *   - THE ONE DIFFERENCE: target_index of a result is a TABLE entry number, not a position in the seed's dictionary.
 * A table lives on the device of the index it was created with; use it only with that index (a tool with replicas makes one per replica).
 * Keys, names and flags are copied: the caller's arrays may go after mtg_targets_create returns.  Without a device: MTG_ERR_NO_DEVICE. */
typedef struct mtg_targets mtg_targets;
int mtg_targets_create(const mtg_index* idx, const char* const* keys, const char* const* names, const uint8_t* is_rc, size_t n, mtg_targets** out);
void mtg_targets_free(mtg_targets* t);
/* device memory the table holds (encoded keys, packed key text, the piece indexes made so far) */
int mtg_targets_device_bytes(const mtg_targets* t, uint64_t* bytes);
typedef struct mtg_seed {
    const char* source;          /* sourceSequence */
    const uint32_t* excluded;    /* ascending entry numbers of the table this seed leaves out (src/Filler.cpp:527); may be NULL when n_excluded == 0 */
    uint32_t n_excluded;
    int is_anchor_repeated, reverse;
} mtg_seed;
int mtg_fill_seeds(const mtg_index* idx, const mtg_params* p, const mtg_targets* t, const mtg_seed* seeds, size_t n, mtg_results** out);
const mtg_gap_result* mtg_results_get(const mtg_results* r, size_t i);
/* Every pointer obtained from r dies here.  The library keeps the storage of up to six freed result sets (a few hundred bytes per
 * gap plus the sequences) and hands it to the next batches, which then pay no allocation, page fault or memset. */
void mtg_results_free(mtg_results* r);
/* bulk view of a result set (for gathers / checksums): n_filled[i] = number of sequences of gap i (may be NULL);
 * *seq_bytes = size of the concatenation "seq\n" of all filled sequences in gap order, which mtg_results_copy_seqs writes to dst */
int mtg_results_summary(const mtg_results* r, uint32_t* n_filled, uint64_t* seq_bytes, uint64_t* n_gaps_filled);
int mtg_results_copy_seqs(const mtg_results* r, char* dst, uint64_t cap);

/* ------------------------------------------------------------------------------------------------------------
 * A result set in relocatable form (offsets, no pointers): what travels between the ranks of a multi-GPU job -- one process per GPU, every
 * rank fills its shard of the sites, the rank that owns the output files gathers the shards' records AND sequences and writes them in
 * input order (the reference's writers under flockfile, src/Filler.cpp:682-683,1029-1214).  Layout:
 *   mtg_wire_header | n_gaps x mtg_wire_gap | n_filled x mtg_wire_filled | seq_bytes (NUL-terminated fills) | ext_bytes (NUL-terminated extensions)
 * every section 8-byte aligned.  tag is the caller's (the global index of the batch: gathers of several batches in flight arrive in any order).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct mtg_wire_header {
    uint64_t magic;                   /* "MTGWIRE1" */
    uint64_t tag;
    uint64_t n_gaps, n_filled, seq_bytes, ext_bytes;
    uint64_t total_bytes;             /* of the whole payload, header included */
    uint64_t checksum;                /* of everything behind the header (a sum of 64-bit words scrambled by their position) */
} mtg_wire_header;
typedef struct mtg_wire_gap {         /* mtg_gap_result */
    int32_t nb_nodes, total_nt, nb_terminal, has_solution_counts, nb_total_filled, nb_reported, n_filled;
    uint32_t first_filled;            /* index of its first mtg_wire_filled */
    uint64_t ext_off;                 /* offset of its extension sequence in the extension section (the empty string at offset 0) */
} mtg_wire_gap;
typedef struct mtg_wire_filled {      /* mtg_filled */
    uint64_t seq_off;                 /* offset in the sequence section */
    uint32_t seq_len;
    int32_t nb_errors_in_anchor, target_index, qual, solution_count, solution_rank;
    float avg_coverage, median_coverage;
} mtg_wire_filled;
int mtg_results_wire_size(const mtg_results* r, uint64_t* bytes);
int mtg_results_to_wire(const mtg_results* r, uint64_t tag, void* dst, uint64_t cap, uint64_t* bytes);
/* The reverse: a result set whose records point into `wire` (which must stay alive and unchanged until mtg_results_free); the payload is
 * validated (magic, sizes, offsets, checksum: MTG_ERR_FORMAT).  Needs no device. */
int mtg_results_from_wire(const void* wire, uint64_t bytes, mtg_results** out, uint64_t* tag);

/* The tool's writers for a run of breakpoint sites (writeFilledBreakpoint, writeVcf, writeExtensions; src/Filler.cpp:1029-1214,1275-1291)
 * on result sets that may have come over the wire: the text the sites add to <out>.insertions.fasta, .info.txt, .insertions.vcf and
 * .extensions.fasta, in site order.  rev / rev_index: the reverse attempts (src/Filler.cpp:669-680): rev_index[i] = index in `rev` of site
 * i's reverse attempt or -1 (rev may be NULL when there is none).  Needs no device. */
typedef struct mtg_site {
    const char* name;                 /* header of the left k-mer's record up to the first space (src/Filler.cpp:631-636) */
    const char* name_r;               /* the same of the right k-mer's record */
    const char* source;               /* the left k-mer's sequence */
    const char* target;               /* the right k-mer's sequence */
} mtg_site;
typedef struct mtg_text {
    char *fasta, *info, *vcf, *ext;   /* not NUL-terminated */
    uint64_t fasta_bytes, info_bytes, vcf_bytes, ext_bytes;
} mtg_text;
int mtg_format_bkpt(const mtg_site* sites, size_t n, const mtg_results* fwd, const mtg_results* rev, const int64_t* rev_index, int filter, int extend, mtg_text* out);
/* writeVcfHeader (src/Filler.cpp:349-383) into out->vcf: sample = the reads / graph the index came from, prefix = the output prefix */
int mtg_format_vcf_header(const char* sample, const char* prefix, mtg_text* out);
void mtg_text_free(mtg_text* t);

/* Stage A only (gatb IterativeExtensions::construct_linear_seqs, call site src/Filler.cpp:884): contigs of each gap
 * as ASCII, for parity tests and the info file.  sources[i] / targets[i] are NUL terminated strings. */
typedef struct mtg_contigs mtg_contigs;
int mtg_stage_a_batch(const mtg_index* idx, const mtg_params* p, const char* const* sources, const char* const* targets, size_t n,
                      mtg_contigs** out);
size_t mtg_contigs_count(const mtg_contigs* c, size_t gap);
const char* mtg_contigs_get(const mtg_contigs* c, size_t gap, size_t i);
void mtg_contigs_free(mtg_contigs* c);

/* timings / counters of the last fill or stage-A batch on this thread */
typedef struct mtg_batch_stats {
    double kernel_ms;            /* HIP-event time of the traversal kernel (k_stage_a) launches (sum over tiers / attempts) */
    double post_kernel_ms;       /* HIP-event time of the terminal-search / coverage kernel (k_post) and of the two layout scans behind it */
    double total_ms;             /* wall time of the whole call */
    double h2d_ms, d2h_ms, host_ms;
    double marshal_ms, result_ms; /* mtg_fill_batch only: argument marshalling and result-arena construction */
    uint64_t index_lines;        /* 64-byte index lines the kernels actually read */
    uint64_t n_launches;
    uint64_t n_retried_gaps;     /* gaps re-run in a larger scratch tier */
    uint64_t contig_nt;          /* nucleotides of all contigs built */
    uint64_t store_runs;         /* runs of nucleotides the traversal took from the unitig store (one header read each) */
    uint64_t run_nt;             /* nucleotides of the contigs that came out of the unitig store */
    uint64_t post_lines;         /* index buckets read by the coverage pass of k_post */
    uint64_t contig_words;       /* 8-byte words of contig arena the traversal wrote */
    uint64_t coverage_kmers;     /* k-mers whose abundance the coverage pass of k_post needed */
    uint64_t dense_words;        /* 8-byte words of contigs copied back for the multi-contig gaps */
    double emit_kernel_ms;       /* HIP-event time of the result kernel (k_emit: ASCII sequences + records); post_kernel_ms = k_post + the layout scans */
    uint64_t seq_bytes;          /* bytes of ASCII the result kernel wrote into the sequence arena */
    double copy_kernel_ms;       /* HIP-event time of the copy kernel (k_copy: long runs of the contigs out of the unitig store, one wave per gap) */
    uint64_t copy_words;         /* 8-byte words of contig arena it wrote */
    uint64_t copy_cmds;          /* runs it copied (one 24-byte command each) */
    uint64_t coverage_direct_kmers; /* of coverage_kmers: abundance bytes read at places known from the copy commands (no look-up, nothing to verify) */
    double finish_kernel_ms;     /* HIP-event time of the finishing kernel (k_finish: parked gaps resumed by groups of lanes, bubbles resolved from LDS) */
    uint64_t n_parked_gaps;      /* gaps the walk kernel parked at a branching node that is not the strict SNP pattern */
    uint64_t n_rounds;           /* bubble rounds queued between launches of the walk kernel (0: the parked gaps went straight to k_finish) */
    uint64_t n_lean_gaps;        /* gaps whose contig was never materialised: target located in the unitig store, coverage and ASCII read off the store */
    double lean_kernel_ms;       /* of copy_kernel_ms: the decision kernel (k_lean, one gap per lane); the rest is k_copy over the gaps that need it */
    uint64_t copy_words_executed; /* of copy_words: those k_copy really wrote (a lean gap's commands are never executed) */
    uint64_t copy_cmds_executed;
    uint64_t post_scanned_words; /* of contig_words: those k_post's terminal search really read (a lean gap's contig is never scanned) */
    double device_span_ms;       /* first kernel of a launch to its last, summed over the launches */
    uint64_t n_general_device;   /* multi-contig gaps finished on the device (k_general: candidate sequences, de-duplication, coverage, ASCII) */
    uint64_t n_general_host;     /* multi-contig gaps the host's path took (a candidate that does not fit the work areas, an unknown k-mer; HOST_GENERAL) */
    uint64_t n_light_walks;      /* launches whose first walk ran in the light kernel (k_walk: simple paths only; chosen when the previous launch hardly met a branching node) */
    uint64_t n_branching_gaps;   /* gaps whose first walk stood on a branching node at least once */
} mtg_batch_stats;
int mtg_last_batch_stats(mtg_batch_stats* s);

/* ------------------------------------------------------------------------------------------------------------
 * needleman_wunsch (src/Utils.cpp:87-189: match +10, mismatch -5, gap -5, traceback preference diagonal / up / left) for n pairs of
 * NUL-terminated sequences, on the device: matches[i] = matching positions along the traceback of (a[i] = rows, b[i] = columns); the
 * reference's identity is matches / max(strlen(a), strlen(b)).  Used by the fill path to de-duplicate multi-path solutions
 * (remove_almost_identical_solutions, src/Utils.cpp:208-238).
 * ---------------------------------------------------------------------------------------------------------- */
int mtg_nw_matches(const char* const* a, const char* const* b, size_t n, uint32_t* matches);

/* ------------------------------------------------------------------------------------------------------------
 * Whole tool: `MindTheGap fill ...` = Filler::run(argc, argv) (src/main.cpp:105-120).  argv[0] is the first option.
 * Returns the process exit code of the reference (0 / 1).
 * ---------------------------------------------------------------------------------------------------------- */
int mtg_fill_main(int argc, const char* const* argv);
/* The same behind Graph::load / Graph::create (src/Filler.cpp:172-226): the graph is an index that is already resident (options -in / -graph
 * are not expected; the index stays the caller's).  What a long-lived caller uses to run the tool's drivers and writers repeatedly. */
int mtg_fill_main_on_index(mtg_index* idx, int argc, const char* const* argv);
/* `MindTheGap profile (-in reads | -graph container) -ref genome.fa [-kmer-size -abundance-min -abundance-max] -out prefix`: the profile of a
 * reference genome against the graph (not a module of the reference tool).  Writes prefix.absent.bed, one line per run of absent k-mers:
 * name, start, start + length, length, L|R|LR|. (k-mer start positions, 0-based, half-open; name = the FASTA header up to the first blank),
 * and prefix.profile.txt, the statistics as `key : value` lines.  Returns 0 / 1; nothing is written unless the whole profile succeeded. */
int mtg_profile_main(int argc, const char* const* argv);
/* `MindTheGap find (-in reads | -graph container) -ref genome.fa (-homo-insertions | -hete-only | -insert-only | -deletion-only | -homo-only
 * -no-snp | -no-snp | -solo-snps | -homo-only -solo-snps | -multi-snps [-snp-min-val 5] | -solo-snps -multi-snps [-snp-min-val 5] |
 * [-solo-snps] [-multi-snps] -rev-snps [-snp-min-val 5]) [-max-rep 5] [-het-max-occ 1] [-branching-filter 15] [-kmer-size -abundance-min -abundance-max] [-out prefix]`: the part
 * of the reference's `find` that mtg_index_find_homo_sequences (-homo-insertions), mtg_index_find_het_sequences plus the homozygous insertions
 * of 1-2 nt (-hete-only, as the reference's option of that name) or both in full (-insert-only, calls merged in detection order) cover, and with
 * mtg_index_find_del_sequences the reference's -deletion-only (deletions and the homozygous insertions of 1-2 nt), -homo-only -no-snp (those and
 * the homozygous sites) and -no-snp (all three layers: its default find minus the SNP observers); an insertion call on a gap that the deletion
 * observer calls is dropped, as the reference asks that observer first.  -solo-snps (mtg_index_find_snp_sequences alone) and -homo-only -solo-snps
 * (that observer ahead of the deletion observer and the four homozygous insertion observers; a deletion call on a gap it calls is dropped) are
 * not configurations of the reference, which has no way to run FindSoloSNP without its multi-SNP observers; they are refused together with
 * anything that runs the heterozygous observer.  -multi-snps (mtg_index_find_msnp_sequences alone) and -solo-snps -multi-snps (both forward SNP
 * observers, their lists merged in detection order) are not configurations of the reference either; with any flag that runs the deletion, the
 * insertion or the heterozygous observers they are refused: a partially consumed gap would reach those shortened and with a corrected kmer_begin,
 * which is not built.  -rev-snps (mtg_index_find_msnp_rev_sequences with passes 2), -multi-snps -rev-snps (passes 3) and either with -solo-snps
 * are configurations of this tool alone as well; the calls of one gap keep the order in which they are made (forward ascending, then reverse
 * descending), and with the same flags they are refused with a message of their own: the gap would reach the later observers with a
 * corrected kmer_end too.  A SNP is one VCF line of writeVcfVariant's form (TYPE=SNP;LEN=1;FUZZY=0).  The repeat flags of the heterozygous
 * observer come from an index of the genome file at k - 1 with abundance_min = het_max_occ + 1 (k >= 12).  Any other combination of these flags
 * stops with a message that names what is not built (-snp-only, the default find, -bed) and returns 1.  Writes prefix.breakpoints (writeBreakpoint,
 * src/FindBreakpoints.hpp:640-658) and prefix.othervariants.vcf (header of src/Finder.cpp:513-541, records of writeIndel and, for deletions,
 * writeVcfVariant: REF = the genome's text from pos over del_size + 1 characters as it stands, ALT its first); ids bkptN count
 * from 1 in detection order across both files; the REPEATED field stays empty (the reference fills it from a Bloom filter of the genome's
 * (k-1)-mers, whose false positives are not reproducible).  Prints the Results block of the reference's summary.  Returns 0 / 1; nothing is
 * written unless the whole scan succeeded. */
int mtg_find_main(int argc, const char* const* argv);

/* ------------------------------------------------------------------------------------------------------------
 * Tuning: every switch of the library -- capacities, A/B hooks of measured alternatives, hooks the tests use to force rare paths,
 * diagnostics -- is an entry of ONE table (mindthegap_amd/csrc/mtg_tuning.h: name, default, kind, what it does; INTEGRATION.md prints it).
 * An entry NAME starts from the environment variable MTG_NAME (or from MTG_TUNING="NAME=value,NAME=value"), and these calls list, read and
 * set the entries at run time.  A value set here holds for the calls that begin after it; an index keeps the capacities it was built with.
 * There is no equivalent in the reference (its options are all on the command line, src/Filler.cpp:95-135, and are mtg_params here): the
 * table only steers HOW this library computes, never WHAT -- every setting gives the same results, which is what the tests use it for.
 * ---------------------------------------------------------------------------------------------------------- */
size_t mtg_tuning_count(void);
/* entry i: its name (without the MTG_ prefix), default ("" = not set), kind ("cap", "ab", "test", "diag") and description; static strings */
int mtg_tuning_describe(size_t i, const char** name, const char** dflt, const char** kind, const char** what);
/* the current value of an entry, "" when it is not set; MTG_ERR_ARG: no such entry, or cap too small */
int mtg_tuning_get(const char* name, char* value, size_t cap);
/* value NULL or "": "not set" -- overriding the environment and the default (to return to the default, set the default string).  A flag
 * ("" by default) is ON for any value but "0": NAME=0 leaves it off.  An environment variable set to the empty string switches a flag on and
 * leaves a number unset. */
int mtg_tuning_set(const char* name, const char* value);

/* ------------------------------------------------------------------------------------------------------------
 * Bench support: measured ceiling of dependent random reads of line_bytes (16/32/64/128) over a table of the given size.
 * ---------------------------------------------------------------------------------------------------------- */
int mtg_bench_random_lines(uint64_t table_bytes, uint64_t n_chains, uint32_t chain_len, uint32_t line_bytes, double* ms, double* gbps);

#ifdef __cplusplus
}
#endif
#endif
