/* shk.h -- C ABI of libshk.so: the MI355X-native k-mer counting path
 * (CQF-deNoise stage of SH-assembly) as a drop-in for the reference's link-time
 * boundary. Plain pointers and sizes only.
 *
 * What each entry point stands in for in the reference (/root/reference):
 *   shk_create            CQF_mt::CQF_mt(qb,hb,t,seed) -> qf_init          cqf/CQF_mt.h:427-445, cqf/gqf.c:2187-2290
 *                         + CQF_runtime_mt ctor (deNoise trigger/rounds)   cqf/CQF_mt.h:292-305
 *   shk_count_chunks      per-chunk body of fastq_to_uint64kmers_prod:
 *                         reads_to_kmers -> NTPC64 + qf_insert_advance,
 *                         trigger test, DeNoise mode (t = 1 schedule)      cqf/CQF_mt.h:610-731, 821-931; gqf.c:2432
 *   shk_hash_chunks       reads_to_kmers' hashing half only (multi-GPU
 *                         routing: keys go to their owner before insert)   cqf/CQF_mt.h:630-718; base/nthash.hpp:295-309
 *   shk_count_words       qf_insert_advance over a batch of routed keys    cqf/gqf.c:2432-2440
 *   shk_denoise           one DeNoise phase (also --endDeNoise)            cqf/CQF_mt.h:860-914, 999-1039; gqf.c:2792-3040
 *   shk_export_cqf        CQF_mt::save -> qf_serialize                     cqf/CQF_mt.h:521, 986-987; gqf.c:2379-2394
 *   shk_import_cqf        CQF_mt::load -> qf_deserialize                   cqf/CQF_mt.h:514-519; gqf.c:2396-2420
 *   shk_lookup            qf_count_key_value /
 *                         qf_count_key_value_{is,set}_traveled             cqf/gqf.c:2442-2469, 3092-3163
 *   shk_extend_forward    get_unitig_forward, the walk that meets no other
 *                         unitig (Contiger, first slice)                   src/contig_assembly.cpp:3028-3218
 *   shk_unitigs_from_seeds its two calls per seed + median abundance        src/contig_assembly.cpp:1886-1904; base/Utility.cpp:27-40
 *   shk_select_seeds      processDataChunk's seed rule                     src/contig_assembly.cpp:1856-1876
 *   shk_find_unitigs,     find_unitigs_mt_master/worker: seeds walked both ways, work queue of branch neighbours,
 *   shk_unitigs_add_*,    startKmer2unitig with "smaller id wins", known-node stops, pure circles; check_unitig,
 *   shk_unitig_set_write  track_kmer_worker, build_graph_worker, writer -- all on the device (csrc/unitig_kernels.hip)
 *                                                                         src/contig_assembly.cpp:2034-2269, 3018-3218, 935-1084, 600-629
 *   shk_insert_counted    qf_insert_advance(count > 1) -> insert_advance    cqf/gqf.c:2024-2136 (local-QF flush, CQF_mt.h:588-607)
 *   shk_dump              qf_iterator / qfi_get / qfi_next / qfi_end        cqf/gqf.c:2474-2601
 *   shk_merge             qf_merge                                          cqf/gqf.c:2614-2655
 *   shk_multi_merge       qf_multi_merge                                    cqf/gqf.c:2660-2704
 *   shk_inner_product     qf_inner_product                                  cqf/gqf.c:2707-2733
 *   shk_intersect         qf_intersect                                      cqf/gqf.c:2736-2757
 *   shk_magnitude         qf_magnitude                                      cqf/gqf.c:2760-2763
 *   shk_spectrum          (no counterpart: the reference's README sends the user to an outside program for F0, F1, f1, f2, ...)
 *   shk_count_fasta       (no counterpart: the reference reads 4-line FASTQ only, cqf/CQF_mt.h:610-731) FASTA text of any shape
 *   shk_query_fasta       (no counterpart: the reference answers one hashed key at a time, qf_count_key_value) FASTA text against
 *                         the table: per-base counts and per-record totals
 *   shk_query_reads       (no counterpart: the reference answers one hashed key at a time, qf_count_key_value) FASTQ reads
 *                         against the table: per-read k-mer statistics, median count, per-window counts
 *   shk_correct_reads     (no counterpart: CQF-deNoise repairs the table, nothing repairs the reads) substitution errors of
 *                         FASTQ reads against the table: per read the edits that make its weak windows solid
 *   shk_sample_chunks     (no counterpart: the reference's README sends the user to ntCard) -N -n -e from the reads themselves
 *   shk_import_shards     (no counterpart: the reference is one process) quotient-range shards -> the single table
 *   shk_stats             runtime->nelts / ndistinct_elts / num_deNoise    cqf/CQF_mt.h:277-288
 *   shk_destroy           CQF_mt::~CQF_mt -> qf_destroy                    cqf/CQF_mt.h:547-557; gqf.c:2306
 *
 * Errors: every call returns 0 or a negative SHK_ERR_* code; the library never exits
 * the process (the reference perror()+exit()s, gqf.c:2244-2247) and, unlike the
 * reference, detects a full table (SHK_ERR_TABLE_FULL) before the pass that would overflow writes anything.
 * Granularity of an error inside shk_count_chunks / shk_count_words: the call works through its chunks in ranges (a
 * range ends where a deNoise round fires); ranges and rounds completed before the failing range stay committed and
 * `stats` reports them (stats->chunks = chunks consumed), the failing range leaves the table as it was.
 * A context is not re-entrant; use one context per thread / per GPU.
 */
#ifndef SHK_H
#define SHK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct shk_ctx shk_ctx;

enum {
  SHK_OK = 0,
  SHK_ERR_ARG = -1,          /* bad argument / unsupported geometry */
  SHK_ERR_HIP = -2,          /* a HIP runtime call failed (no GPU, out of memory, ...) */
  SHK_ERR_TABLE_FULL = -3,   /* runs would pass xnslots */
  SHK_ERR_REGION = -4,       /* one 256-quotient region exceeded the kernel's LDS image or hash */
  SHK_ERR_CORRUPT = -5,      /* table metadata inconsistent / key outside this context's range */
  SHK_ERR_FASTQ = -6,        /* malformed input: read longer than 65535, too many reads */
  SHK_ERR_BATCH = -7,        /* batch larger than the capacities given at create time */
  SHK_ERR_IO = -8
};

typedef struct shk_config {
  uint32_t qb;                     /* log2(#slots) of the whole filter (all shards) */
  uint32_t hb;                     /* hash bits, must be qb + 8 (src/CQF-deNoise.cpp:161) */
  uint32_t seed;                   /* stored in the .cqf header (src/CQF-deNoise.cpp:83) */
  uint32_t k;                      /* k-mer size, 1..191 */
  uint64_t ndistinct_for_denoise;  /* deNoise trigger (src/CQF-deNoise.cpp:125) */
  uint32_t num_denoise;            /* rounds available (runtime->num_deNoise) */
  uint32_t reserved0;
  uint64_t min_denoise_len;        /* 0 = reference value NUM_SLOTS_TO_LOCK<<4 = 1<<20 (CQF_mt.h:964) */
  uint64_t max_batch_bytes;        /* capacity: FASTQ text bytes per shk_count_chunks call */
  uint64_t max_batch_keys;         /* capacity: k-mers per batch */
  uint64_t max_batch_reads;        /* capacity: reads per batch (0 = max_batch_bytes/16) */
                                   /* Besides the text, read and key buffers these three size, a context keeps the newline
                                    * flags of the text in hand, one bit per text byte: max(max_batch_bytes, 4 * max_batch_keys) / 8
                                    * bytes (+ 16), once more in a context that has used shk_prepare_chunks. Device text of more
                                    * than four bytes per key makes a call grow them to text_bytes / 8 (never back); if that
                                    * allocation fails the call reads the text a second time instead. SHK_PARSE_MASK=0 when the
                                    * context is created: no such buffer.
                                    * The first shk_count_fasta allocates its own: max_batch_bytes / 4 bytes for the piece's bases at
                                    * 2 bits each, max_batch_bytes / 16 for the state in front of every 16 text bytes, and about 70 bytes
                                    * per tile of 4 KiB of text; they stay until shk_destroy */
  int32_t device;                  /* HIP device ordinal */
  uint32_t shard_index;            /* this context owns quotients [shard_index, shard_index+1) * 2^qb / num_shards */
  uint32_t num_shards;             /* 0 or 1 = whole filter; otherwise a power of two */
  uint32_t threads_per_group;      /* 0 = 512; tests may lower it */
  uint32_t hash_groups;            /* 0 = auto; grid of the grid-stride kernels */
  uint32_t max_level_bits;         /* 0 = 10; digit bits per partition level (tests lower it) */
} shk_config;

typedef struct shk_batch_stats {
  uint64_t kmers;            /* k-mers presented to the filter by this call (qf_insert_advance calls) */
  uint64_t new_distinct;     /* keys that were new when inserted (isNew) */
  uint64_t removed;          /* entries removed by deNoise rounds fired inside this call */
  uint32_t denoise_rounds;   /* rounds fired inside this call */
  uint32_t chunks;           /* chunks consumed */
} shk_batch_stats;

typedef struct shk_totals {
  uint64_t nelts;            /* runtime->nelts */
  uint64_t ndistinct;        /* runtime->ndistinct_elts */
  uint32_t rounds_left;      /* runtime->num_deNoise */
  uint32_t rounds_done;
  uint64_t nslots, xnslots, nblocks, table_bytes;  /* this context's (shard's) geometry */
  uint64_t free_pointer;     /* first slot after the last run */
} shk_totals;

int shk_create(const shk_config *cfg, shk_ctx **out);
void shk_destroy(shk_ctx *ctx);

/* Count every k-mer of `nchunks` FASTQ chunks. chunk_off/chunk_len index into `text`
 * (text_on_device != 0: `text` is a device pointer, 16-byte aligned, that stays valid until the call returns; the
 * kernels read the text in aligned 16-byte units, so the allocation must be readable up to the next multiple of 16
 * behind text + text_bytes -- hipMalloc'ed buffers always are. Every call that takes device text answers a pointer
 * that is not 16-byte aligned with SHK_ERR_ARG before it starts anything).
 * The chunks may lie in any order, leave bytes of the text out, be shorter than 16 bytes or empty (chunk_len 0: no
 * reads); lines are counted from each chunk's own first byte. One call takes 1 .. 4096 chunks (SHK_ERR_BATCH otherwise;
 * so do shk_prepare_chunks, shk_hash_chunks and shk_hash_route_chunks, whose labels must stay below 4096 too). A read of
 * more than 65535 bases is SHK_ERR_FASTQ from each of them, the table left as it was.
 * Chunks are the units after which the reference tests its deNoise trigger; rounds fire
 * inside the call exactly where the t = 1 reference would fire them. */
int shk_count_chunks(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes,
                     const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                     shk_batch_stats *stats);

/* The same in two halves, so that the front end of later batches (parse, hash, partition: its own stream and buffers)
 * runs WHILE an earlier batch is rebuilt into the table -- the overlapped form of the reference's producer threads
 * (cqf/CQF_mt.h:821-931 interleaves reading, hashing and inserting across threads). shk_prepare_chunks starts the front
 * end of a batch and returns at once; shk_count_prepared takes the OLDEST prepared batch through the rebuild (deNoise
 * rounds fire inside it exactly as in shk_count_chunks) and returns its statistics. At most two batches may be prepared
 * ahead (SHK_ERR_BATCH beyond). `text` (host or device) must stay valid until the batch has been counted. Device text
 * must be COMPLETE when shk_prepare_chunks is called: the front end runs on a non-blocking stream of its own, which is
 * ordered behind the copy of shk_upload_text that filled `text` and behind nothing else -- not behind work queued on the
 * null stream or any other (synchronise that first). A failure of
 * the front end is returned by the shk_count_prepared of that batch; the table is untouched then. Results are those of
 * shk_count_chunks on the same batches in the same order. Not for sharded contexts (their words go through
 * shk_hash_chunks and the exchange). */
int shk_prepare_chunks(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes,
                       const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks);
int shk_count_prepared(shk_ctx *ctx, shk_batch_stats *stats);
/* Allocates the front end's own buffers and stream now instead of inside the first shk_prepare_chunks (which does it
 * otherwise), and -- for a context with deNoise rounds -- the records of a deNoise point instead of in the first pass
 * that needs them: for callers that want context set-up and steady state apart, e.g. when timing. Idempotent. */
int shk_prepare_reserve(shk_ctx *ctx);

/* Overlapped ingest: start copying host text (pinned memory for full PCIe rate) for a LATER call into one of two
 * context-owned device buffers; the copy runs on its own stream while the context computes. Pass the returned
 * pointer as `text` with text_on_device = 1; that call waits for the copy. Upload batch s+1, then count batch s. */
int shk_upload_text(shk_ctx *ctx, const void *host_text, uint64_t nbytes, void **d_text);
/* page-locked host memory for the text handed to shk_upload_text (pageable memory works, at a fraction of the rate) */
int shk_host_alloc(uint64_t nbytes, void **p);
void shk_host_free(void *p);

/* Hash only: leaves `*nwords` key words (key | chunk_index << hb, reference emission
 * order) in a context-owned device buffer `*d_words`, valid until the next call.
 * In a context that is one of G shards, chunk i of the call is labelled i * G + shard_index:
 * the ranks' chunks interleave like the parts of the reference's round-robin file queue
 * (cqf/CQF_mt.h:364-390, 828-830), and nchunks * G must stay below 4096. */
int shk_hash_chunks(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes,
                    const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                    uint64_t **d_words, uint64_t *nwords);

/* Insert key words that are already on the device (all keys must belong to this context's
 * quotient range). nchunks = 1 + the largest chunk index present. */
int shk_count_words(shk_ctx *ctx, const uint64_t *d_words, uint64_t nwords, uint32_t nchunks,
                    shk_batch_stats *stats);

/* ---- FASTA (no counterpart in the reference). Counts the k-mers of FASTA text: records and lines of any length, one or
 * many records, with or without headers.
 *   - A line whose first byte is '>' or ';' is a header line: nothing in it is sequence, whatever it holds, however long.
 *   - In every other line '\n' and '\r' are skipped, A C G T a c g t are bases, and every other byte is a BREAK: N, the
 *     IUPAC codes, space, tab, '*', '-', NUL, bytes >= 0x80, a '>' that is not at a line start. A header line is a break
 *     too. Text that starts without a header is sequence.
 *   - A k-mer is counted exactly when its k bases follow each other with nothing but line ends between them. Its key is
 *     the one the FASTQ path gives the same k-mer: canonical ntHash masked to hb bits. For reads made of bases only, FASTA
 *     and FASTQ input therefore give identical tables; they differ only where reads_to_kmers hashes windows that hold a
 *     byte that is no base (the first window of a read, and the one behind an 'N'): this path never hashes such a window.
 *   - No limit on the length of a record or a line: a run of bases is cut into segments of SHK_FASTA_SEGMENT k-mers, one
 *     per device thread, which overlap by k - 1 bases.
 * Streaming: consecutive calls are consecutive pieces of ONE stream, cut at any byte (inside a header, between '\r' and
 * '\n', in the middle of a run). The context keeps what the next piece needs: inside a header or not, at a line start or
 * not, whether a break lies behind the last base, and the last <= k - 1 bases of the open run (on the device). first != 0
 * forgets that state: the piece is the start of a file. A k-mer is counted by the call that brings its last base; the table
 * after any sequence of pieces is the table after the whole text in one call.
 * To the table a call is ONE chunk: it behaves as shk_count_words on the call's keys with nchunks = 1 (counters, `stats`,
 * the deNoise trigger tested once, behind the call). fstats (may be NULL): records = header lines begun in this piece,
 * bases, breaks = break BYTES outside header lines (a header counts as a record, not here), kmers = stats->kmers.
 * Errors leave the table and the streaming state as they were, so the call can be repeated with a smaller piece:
 * SHK_ERR_BATCH for text_bytes > max_batch_bytes, more than max_batch_keys k-mers, more segments than max_batch_reads (its
 * default: max_batch_bytes / 16 + 1024), more runs of bases (of any length) than max_batch_keys - 2, more 64-base units of
 * segments than max_batch_keys / 2 - 1, or batches prepared and not yet counted; SHK_ERR_ARG for a sharded context or
 * device text that is not 16-byte aligned (the text contract of shk_count_chunks). 1 <= k <= 191, every geometry. */
#define SHK_FASTA_SEGMENT 256    /* k-mers one device thread hashes of a long run; SHK_FASTA_SEGMENT=n in the
                                    environment of shk_create overrides it (16 <= n, n + k - 1 <= 65535): tests */
typedef struct shk_fasta_stats { uint64_t records, bases, breaks, kmers; } shk_fasta_stats;
int shk_count_fasta(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes, int first,
                    shk_batch_stats *stats, shk_fasta_stats *fstats /* may be NULL */);

/* ---- FASTA text against the table (no counterpart in the reference): how often does the table hold the k-mers of this
 * sequence, position by position and record by record? One streamed pass; the table stays untouched.
 *   - Grammar and k-mers: exactly shk_count_fasta's (header lines, breaks, runs, both cases, '\r', no limit on line or
 *     record length); a k-mer's key is the one the counting paths give it. 1 <= k <= 191, every geometry.
 *   - Streaming: consecutive calls are consecutive pieces of ONE stream, cut at any byte; first != 0 starts a new stream.
 *     A k-mer is answered by the call that brings its last base. The query stream keeps its own state (line state, pending
 *     break, the tail of <= k - 1 bases on the device), apart from shk_count_fasta's: count calls and query calls on one
 *     context may interleave without seeing each other.
 *   - track (may be NULL; a host pointer unless track_on_device != 0): for b in [0, bases of this piece), track[b] belongs to
 *     the k-mer whose last base is the piece's b-th base in text order (bytes that are no bases do not count). Its value is
 *     that k-mer's count in the table, capped at 0xFFFFFFFE, or SHK_QUERY_NONE where no k-mer ends (fewer than k bases lie
 *     behind the last break). The tracks of a stream's pieces, concatenated, are the track of the text in one call. With
 *     track == NULL the call allocates and writes no per-base buffer at all.
 *   - rec (may be NULL; host memory): rec[0] belongs to the record that was open when the piece began (or to text in front
 *     of any header), rec[i], i >= 1, to the i-th header line begun in this piece; *nrec = 1 + records. Each entry holds,
 *     over the k-mers of that record answered by this call: kmers = their number, present = those with count >= 1, solid =
 *     those with count >= min_count, sum = their true (uncapped) counts mod 2^64. A run never crosses a header, so every
 *     k-mer has exactly one record. A caller adds rec[0] to the last record it already has.
 *   - qstats (may be NULL): the same four sums over the whole piece; records, bases, breaks and kmers mean what
 *     shk_fasta_stats means by them.
 *   - It is a reader: it launches the pending lazy placement first, as shk_lookup does, reads with mark mode 2 (traveled
 *     bits are neither read nor set), and changes no byte of the table and no runtime counter.
 * Errors leave the query stream's state as it was: SHK_ERR_ARG for a sharded context or device text that is not 16-byte
 * aligned; SHK_ERR_BATCH for text_bytes > max_batch_bytes, the capacity limits shk_count_fasta states (the call borrows the
 * same batch buffers), batches prepared and not yet counted, track_cap smaller than the piece's bases, or rec_cap <
 * 1 + records -- *nrec is then still set to the number needed, so the call can be repeated.
 * Besides shk_count_fasta's buffers a context that has answered queries keeps 40 bytes per record of the piece with the
 * most records so far and, for host tracks, 4 bytes per base of the piece with the most bases so far. */
#define SHK_QUERY_NONE 0xFFFFFFFFu
typedef struct shk_query_record { uint64_t kmers, present, solid, sum; } shk_query_record;
typedef struct shk_query_stats  { uint64_t records, bases, breaks, kmers, present, solid, sum; } shk_query_stats;
int shk_query_fasta(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes, int first,
                    uint32_t min_count,
                    uint32_t *track, uint64_t track_cap, int track_on_device,      /* track may be NULL */
                    shk_query_record *rec, uint32_t rec_cap, uint32_t *nrec,       /* rec may be NULL; host memory */
                    shk_query_stats *qstats /* may be NULL */);

/* ---- FASTQ reads against the table (no counterpart in the reference): what does the table know about every read? Per read
 * the number of its k-mers, how many of them the table holds, their smallest, largest and median count, and optionally
 * every window's count; the table stays untouched. The job of a decontamination or baiting filter, of abundance
 * filtering by median count, of haplotype binning against two parental tables (one call each).
 *   - Text and chunks: exactly shk_count_chunks' contract (host text, or device text aligned to 16 bytes; 1 .. 4096 chunks
 *     in any order, with gaps, empty or shorter than 16 bytes; lines counted from each chunk's first byte). The reads are
 *     the ones the FASTQ front end finds, in its order: chunk by chunk in the order of the call, text order inside a chunk.
 *     *nreads = their number.
 *   - ext (may be NULL; host memory, rec_cap entries): ext[r] = read r's sequence line as the front end hands it over:
 *     seq_off = the offset of its first byte in `text`, seq_len = its length up to, not including, the line feed (a '\r' in
 *     front of the line feed belongs to it), chunk = the index of its chunk in the call.
 *   - Which k-mers: window j of a read is bytes [j, j + k) of its sequence line, and a window is a k-mer exactly when all k
 *     bytes are one of A C G T a c g t -- shk_query_fasta's rule, so a read answers the same whether asked as FASTQ or as
 *     a two-line FASTA record. Its key is the one the counting paths give that k-mer: canonical ntHash masked to hb bits.
 *     A window that holds any other byte (N, the IUPAC codes, '\r', anything) is no k-mer. This is deliberately NOT the
 *     stream of reads_to_kmers, which hashes the first window of a read and the window behind an 'N' without looking at
 *     them (shk_count_chunks restates that; see shk_count_fasta's comment): for reads made of bases only the two agree.
 *     A read shorter than k has no k-mers. 1 <= k <= 191, every geometry.
 *   - rec[r], over the counts c of read r's k-mers: kmers = their number, present = those with c >= 1, solid = those with
 *     c >= min_count, sum = the true counts added up mod 2^64; min, max and median over the counts capped at 0xFFFFFFFE,
 *     absent k-mers (count 0) included. median is the LOWER median, sorted[(kmers - 1) / 2] -- an integer, unlike the
 *     averaging median of shk_unitigs_from_seeds -- and is computed only with SHK_READS_MEDIAN in flags; without it the
 *     field is SHK_QUERY_NONE. A read without k-mers has min = max = 0 (and median 0 when asked for). rec is host memory
 *     unless rec_on_device != 0.
 *   - track (may be NULL; a host pointer unless track_on_device != 0): entry woff[r] + j belongs to window j of read r,
 *     woff[r] = the sum over earlier reads of max(seq_len - k + 1, 0). Its value is the capped count, or SHK_QUERY_NONE
 *     where the window is no k-mer. *nwindows = the number of windows of the call. With track == NULL and no median
 *     asked for the call writes nothing per window.
 *   - rstats (may be NULL): reads, and the sums of kmers, present, solid and sum over the call.
 *   - It is a reader: it launches the pending lazy placement first, as shk_lookup does, reads with mark mode 2 (traveled
 *     bits are neither read nor set), and changes no byte of the table and no runtime counter.
 * Errors: nothing is written to rec, ext or track, and the table is untouched. SHK_ERR_ARG for a sharded context, device
 * text that is not 16-byte aligned, NULL rec, nreads or chunk arrays, unknown flag bits; SHK_ERR_BATCH for nchunks outside
 * 1 .. 4096, text, reads or windows beyond the context's capacities (windows are bounded by max_batch_keys: the per-window
 * scratch is borrowed from the key-word buffers), batches prepared and not yet counted, track_cap < *nwindows, or rec_cap
 * < *nreads -- *nreads and *nwindows are then still set to what is needed, so the call can be repeated; SHK_ERR_FASTQ
 * for a read of more than 65535 bases.
 * Besides the batch buffers it borrows (the text buffer, the read arrays, the two key-word buffers: 2-bit units in one,
 * the per-window values of a call with a median or a host track in the other), a context that has answered such a query
 * keeps 44 bytes per read of max_batch_reads: the windows of every read and their offsets (pack_stage owns the front
 * end's own pair of arrays for the units' flags and places) and the records of a call whose rec is host memory. */
#define SHK_READS_MEDIAN 1u
typedef struct shk_read_record { uint64_t sum; uint32_t kmers, present, solid, min, median, max; } shk_read_record;   /* 32 bytes */
typedef struct shk_read_extent { uint64_t seq_off; uint32_t seq_len, chunk; } shk_read_extent;                        /* 16 bytes */
typedef struct shk_reads_stats { uint64_t reads, kmers, present, solid, sum; } shk_reads_stats;
int shk_query_reads(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes,
                    const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                    uint32_t min_count, uint32_t flags,
                    shk_read_record *rec, uint64_t rec_cap, int rec_on_device, uint64_t *nreads,
                    shk_read_extent *ext,                                   /* may be NULL; host memory, rec_cap entries */
                    uint32_t *track, uint64_t track_cap, int track_on_device, uint64_t *nwindows,   /* track may be NULL */
                    shk_reads_stats *rstats /* may be NULL */);

/* ---- substitution errors of FASTQ reads repaired against the table (no counterpart in the reference: CQF-deNoise takes
 * the false k-mers out of the table, nothing takes them out of the reads). A read whose k-mers are solid, then weak for k
 * windows, then solid again holds one wrong base, and the table says which base belongs there. The call returns edits,
 * not text: shk/correct.py's apply_edits puts them into a copy of the text.
 *   - Text, chunks, the order of the reads, *nreads and ext: exactly shk_query_reads' contract.
 *   - Candidates: a read is a candidate when its sequence line has k <= seq_len <= 65535 bytes and every byte is one of
 *     A C G T a c g t. A shorter read is flagged SHK_CORRECT_SHORT (whatever it holds), a read of at least k bytes with
 *     any other byte SHK_CORRECT_NONBASE (a '\r' in front of the line feed belongs to the sequence line, so every read of
 *     a CRLF file is one); both are left alone, with edits = unfixable = ambiguous = 0.
 *   - The rule. A window is solid when its k-mer's count is >= min_count; its key is the one the counting paths give it
 *     (canonical ntHash masked to hb bits). W = seq_len - k + 1. S is the read, mutable; budget starts at max_edits.
 *         forward(S): prev = false
 *                     for j in 0 .. W-1:
 *                         solid = count(S[j:j+k]) >= min_count                 (S as it is NOW, earlier edits included)
 *                         if not solid and prev:
 *                             if budget == 0: flags |= SHK_CORRECT_CAPPED
 *                             else: p = j + k - 1                              (the suspect: the base window j adds)
 *                                   valid = the bases b != S[p] for which every window j .. min(j + check, W - 1) of S
 *                                           with S[p] = b is solid
 *                                   one:     S[p] = b, the edit (p, b) is recorded, budget -= 1, solid = true
 *                                   none:    unfixable += 1
 *                                   several: ambiguous += 1                    (no tie-break, no "highest count")
 *                         prev = solid
 *         correct(S): forward(S); forward(the reverse complement of S), its edits recorded in S's coordinates and strand
 *     A larger check is more conservative. 0 <= check <= 255, 1 <= max_edits <= 16, min_count >= 1.
 *   - rec[r] (host memory unless rec_on_device != 0): what the rule did to read r, and the flags above.
 *   - edits (a host pointer unless edits_on_device != 0; rec_cap * max_edits entries): entry edits[r * max_edits + e], for
 *     e < rec[r].edits, is pos | code << 16: pos = the offset in the sequence line, code = the new base, A C G T = 0 1 2 3.
 *     The entries stand in the order the edits were made: those of the forward pass ascending, then those of the backward
 *     pass descending. A position may appear twice; the later entry wins. Entries behind rec[r].edits are unspecified.
 *   - The caller's text is never written: device text is byte for byte what it was.
 *   - cstats (may be NULL): reads = *nreads, and over the candidates: their number, those with an edit, and the sums of
 *     edits, unfixable and ambiguous; capped = the reads flagged SHK_CORRECT_CAPPED.
 *   - It is a reader: it launches the pending lazy placement first, reads with mark mode 2, and changes no byte of the
 *     table and no runtime counter. The 2-bit staging of the batch is consumed (the edits are made there).
 * Errors: nothing is written to rec, ext or edits. SHK_ERR_ARG for a sharded context, device text that is not 16-byte
 * aligned, NULL rec, edits, nreads or chunk arrays, min_count == 0, check > 255, max_edits outside 1 .. 16; SHK_ERR_BATCH
 * for shk_query_reads' reasons (nchunks outside 1 .. 4096, text or reads beyond the context's capacities, batches prepared
 * and not yet counted), for a batch whose 2-bit units the staging buffer cannot hold (text_bytes / 64 + reads + 1 units
 * of 16 bytes against max_batch_keys / 2 - 1: the bound the counting path computes -- SHK_NO_PACK, that path's
 * measurement switch, does not apply here), and for rec_cap < *nreads, with *nreads still set so that the call can be
 * repeated; SHK_ERR_FASTQ for a read of more than 65535 bases.
 * A context that has answered such a call keeps the records and the edit lists of its largest batch on the device (16 +
 * 4 * max_edits bytes per read), only as far as the caller's are host memory. */
#define SHK_CORRECT_SHORT    1u   /* fewer than k bytes: nothing to do */
#define SHK_CORRECT_NONBASE  2u   /* holds a byte that is no base: left alone */
#define SHK_CORRECT_CAPPED   4u   /* a suspect was met with the budget used up */
typedef struct shk_correct_record { uint32_t edits, unfixable, ambiguous, flags; } shk_correct_record;   /* 16 bytes */
typedef struct shk_correct_stats { uint64_t reads, candidates, edited_reads, edits, unfixable, ambiguous, capped; } shk_correct_stats;
int shk_correct_reads(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes,
                      const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                      uint32_t min_count, uint32_t check, uint32_t max_edits,
                      shk_correct_record *rec, uint64_t rec_cap, int rec_on_device, uint64_t *nreads,
                      shk_read_extent *ext,                 /* may be NULL; host memory, rec_cap entries */
                      uint32_t *edits, int edits_on_device, /* rec_cap * max_edits entries */
                      shk_correct_stats *cstats             /* may be NULL */);
/* table lookups of the context's last shk_correct_reads (measurement: tools/bench_correct.py divides them by the windows) */
uint64_t shk_correct_lookups(shk_ctx *ctx);

/* ---- a hash-sampled spectrum of the reads (no counterpart in the reference, whose README sends the user to ntCard for
 * the -N -n -e its command line wants). Hashes every k-mer of the FASTQ chunks exactly as shk_count_chunks does (the
 * reads_to_kmers stream with all its quirks) and KEEPS those whose canonical 64-bit ntHash has bits
 * [hb, hb + sample_bits) equal to zero; the kept k-mers are counted into the table, exactly, under the key the full filter
 * would give them (the hash's low hb bits: the sample bits lie directly above the key bits and share none with them).
 * Whether a k-mer is kept depends on the k-mer alone, so a kept k-mer is kept at every occurrence: the table holds the
 * exact abundances of a 2^-sample_bits sample of the DISTINCT k-mers, and shk_spectrum of it scaled by 2^sample_bits
 * estimates F0, f1, f2, ... of the whole input; F1 is counted exactly on the way (sstats->kmers). sample_bits = 0 keeps
 * everything. (Not the hash's top bits: the canonical hash is the smaller of two, and its leading bits are zero about
 * twice as often as they should be.)
 *   - Text and chunks: the contract of shk_count_chunks (host text, or device text that is 16-byte aligned; 1 .. 4096
 *     chunks in any order, lines counted from each chunk's first byte).
 *   - To the table the call is ONE chunk: it behaves as shk_count_words on the kept keys with nchunks = 1 (counters,
 *     `stats`, the deNoise trigger tested once, behind the call). Every geometry.
 *   - sstats (may be NULL): kmers = every k-mer the text holds (what shk_count_chunks reports as stats->kmers), kept = the
 *     occurrences kept = stats->kmers of this call.
 *   - Calls accumulate: sampling with the same sample_bits over any split of the input into calls gives the table of one
 *     call over all of it. Mixing values of sample_bits in one context is the caller's business; nothing checks it.
 * Errors leave the table as it was: SHK_ERR_ARG for sample_bits > 24, hb + sample_bits > 56, a sharded context or device
 * text that is not 16-byte aligned; SHK_ERR_BATCH for more kept words than max_batch_keys, text or reads beyond the
 * capacities, nchunks outside 1 .. 4096, or batches prepared and not yet counted; SHK_ERR_FASTQ for a read of more than
 * 65535 bases. (Reads are staged at 2 bits per base where their 64-base units fit max_batch_keys / 2 - 1 and are read
 * from the text otherwise: the capacity for keys bounds the kept words only.) */
typedef struct shk_sample_stats { uint64_t kmers, kept; } shk_sample_stats;
int shk_sample_chunks(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes,
                      const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                      uint32_t sample_bits, shk_batch_stats *stats, shk_sample_stats *sstats /* may be NULL */);

/* ---- staged form of shk_count_words for several GPUs. The deNoise trigger is a property of
 * the WHOLE filter, so with quotient-range shards the host reduces each shard's statistics
 * (all-reduce over RCCL/gloo) between these calls and takes the same decisions on every rank
 * (sh-assembly_amd/shk/dist.py mirrors the single-GPU logic of csrc/shk_api.hip merge_stage).
 *   shk_route_words    bin this rank's key words by owner (send buffer of the all-to-all)
 *   shk_stage_words    copy + partition the routed key words (chunk ids are global)
 *   shk_stage_summary  statistics of inserting the words of chunks [lo, hi]; nothing is written
 *   shk_stage_commit   write them; must follow a summary over exactly [lo, hi]
 *   shk_denoise        one round on this shard alone: its range walk (CQF_mt.h:888-895) starts at the shard's first
 *                      slot. The sharded driver uses it only as a last resort -- rounds normally go through
 *                      shk_stage_point_* / shk_stage_round_try below, which continue the walk from shard to shard
 *                      over the single table's layout */
typedef struct shk_summary {
  uint64_t new_distinct, added, removed;
  uint32_t err_bits;       /* raw kernel flags; SHK_SOFT_BITS are meaningless for a speculative range */
  uint32_t reserved;
} shk_summary;
#define SHK_SOFT_BITS 0x0Au     /* table full | region image exceeded: only final for a committed range */
#define SHK_HASH_FULL_BIT 0x04u /* too many distinct new keys in one region: summarise fewer chunks */
/* Group the key words left by shk_hash_chunks by owner shard (owner = top log2(nshards) bits of
 * the quotient): `*d_out` (context-owned, valid until the next call) holds them owner by owner,
 * counts[o] words for owner o -- the send buffer of the all-to-all. Two send buffers alternate: the result of one
 * call stays valid until the SECOND-next call, so batch s can be on the wire while batch s+1 is hashed and routed. */
int shk_route_words(shk_ctx *ctx, uint64_t nwords, uint32_t nshards, uint64_t **d_out, uint64_t *counts);

/* shk_hash_chunks + shk_route_words in one pass over the text: every k-mer is hashed and sent straight to its owner's
 * bin of one of the two alternating send buffers (no key word goes to HBM and back in between). Same results:
 * `*d_out` holds the words binned by owner, counts[s] of them for shard s, `*nwords` in total; chunk i of the call is
 * labelled i * num_shards + shard_index. */
int shk_hash_route_chunks(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes,
                          const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks, uint32_t nshards,
                          uint64_t **d_out, uint64_t *counts, uint64_t *nwords);
int shk_stage_words(shk_ctx *ctx, const uint64_t *d_words, uint64_t nwords);
/* The same from TWO device buffers (a shard's own words, where shk_hash_route_chunks left them, and the words it received):
 * no copy that brings them together first. Neither may lie in the buffer shk_hash_chunks returns (the first partition
 * level writes there): SHK_ERR_ARG. */
int shk_stage_words_pair(shk_ctx *ctx, const uint64_t *d_words_a, uint64_t nwords_a, const uint64_t *d_words_b, uint64_t nwords_b);
/* Allocates the two send buffers of shk_route_words / shk_hash_route_chunks now instead of inside their first two calls,
 * and the records of a deNoise point (for callers that keep set-up and steady state apart). Idempotent. */
int shk_route_reserve(shk_ctx *ctx);
int shk_stage_summary(shk_ctx *ctx, uint32_t chunk_lo, uint32_t chunk_hi, int want_chunks, shk_summary *out);
int shk_stage_commit(shk_ctx *ctx, uint32_t chunk_lo, uint32_t chunk_hi, const shk_summary *s);
/* try/accept form (what sh-assembly_amd/shk/dist.py uses): shk_stage_try computes everything about
 * inserting [lo, hi] that does not depend on the other ranks' decision -- statistics, run lengths and
 * encodings (kept on the device), free pointers, error flags -- and writes nothing to the live table;
 * shk_stage_accept then places the runs into the spare table and makes it the live one (only after a
 * clean try over the same range); a try that is not accepted is simply superseded by the next call */
int shk_stage_try(shk_ctx *ctx, uint32_t chunk_lo, uint32_t chunk_hi, int want_chunks, shk_summary *out);
int shk_stage_accept(shk_ctx *ctx, const shk_summary *s);
/* One deNoise round on this shard fused with the insertion of the staged chunks [lo, hi] that lie behind the deNoise
 * point (one pass over the table instead of two): statistics only; shk_stage_accept writes. out->removed = singletons
 * dropped; a dropped key that reappears in [lo, hi] counts in out->new_distinct. If any rank reports err_bits, or the
 * trigger would be reached again inside [lo, hi], do not accept: run shk_denoise and go on as usual. */
int shk_stage_try_denoise(shk_ctx *ctx, uint32_t chunk_lo, uint32_t chunk_hi, shk_summary *out);
/* want_chunks != 0 in shk_stage_summary / shk_stage_try additionally records the first chunk of every
 * new key; this call returns the exact histogram of that last pass: out[i] = new keys first seen in
 * chunk i, for i < n (n <= chunk_hi + 1 of the pass). With it the ranks find the chunk of a deNoise
 * point in one pass. SHK_ERR_ARG when the last pass has none.
 * (The first such pass allocates nregions KiB of device memory for the first-chunk records, unless
 * the context was created for deNoise rounds or shards, which allocates them up front.) */
int shk_stage_chunk_hist(shk_ctx *ctx, uint64_t *out, uint32_t n);

/* ---- a deNoise point inside the staged batch in ONE rebuild per shard (the sharded form of what shk_count_chunks does
 * on a single table; replaces try(lo..point) + accept + try_denoise + accept). The ranks take the steps together
 * (sh-assembly_amd/shk/dist.py: _one_pass_point); nothing is written before shk_stage_accept.
 *   shk_stage_sample        statistics pass over every n-th region: hist[i] = keys new to the filter first seen in chunk
 *                           i, within the sample (i <= chunk_hi); summed over the shards and scaled by regions / sampled
 *                           it predicts the chunk at which the filter-wide distinct count reaches the trigger
 *   shk_stage_point_try     the rebuild with two counts per key (chunks <= split / behind it): entries whose count at the
 *                           split is 1 are dropped (qf_remove_singletons as run by CQF_mt.h:860-869 after chunk `split`),
 *                           the later chunks added on top. Also records the exact first-chunk histogram
 *                           (shk_stage_chunk_hist) with which the ranks check that `split` IS the chunk of the point.
 *                           out->islots / ifin / first_used describe the shard's table at the split (slots in use, free
 *                           pointer behind its last quotient, run on quotient 0): what the next shard needs to lay its
 *                           own part out as in the single table
 *   shk_stage_point_walk    the round's range walk (CQF_mt.h:888-895) over this shard, continuing the previous shard's:
 *                           carry = slots the earlier shards spill over this shard's first quotient (>= 0), prev_fp = their
 *                           free pointer relative to it (negative when they end before it; -1 for shard 0), state_in/out
 *                           = {0, 0} between two ranges / {1, minimum end of the open range relative to the next shard};
 *                           *nprot singletons on range ends survive the round (kept on the device for _finish)
 *   shk_stage_point_finish  rebuilds the regions holding those; `out` = final statistics, `accept` = what to hand to
 *                           shk_stage_accept when every rank is clean and the trigger is not reached again in the rest */
typedef struct shk_point {
  uint64_t new_after, added_after;   /* keys new to the table after the round / occurrences from the chunks behind the split */
  uint64_t removed, added_before;    /* singletons dropped / occurrences from the chunks up to the split */
  uint64_t islots, ifin;
  uint32_t first_used;
  uint32_t err_bits;                 /* any bit: do not go on with this point (take the three-pass path) */
} shk_point;
int shk_stage_sample(shk_ctx *ctx, uint32_t chunk_lo, uint32_t chunk_hi, uint64_t *hist, uint32_t *regions, uint32_t *sampled,
                     uint32_t *err_bits);
int shk_stage_point_try(shk_ctx *ctx, uint32_t chunk_lo, uint32_t split, uint32_t chunk_hi, shk_point *out);
/* the same for a round on its own (no words: the reference's --endDeNoise round, or a round the batch ends on);
 * followed by shk_stage_point_walk / _finish / shk_stage_accept like a point. split = chunk_lo - 1 in
 * shk_stage_point_try puts the round in front of all the staged chunks [chunk_lo, chunk_hi]. */
int shk_stage_round_try(shk_ctx *ctx, shk_point *out);
int shk_stage_point_walk(shk_ctx *ctx, int64_t carry, int64_t prev_fp, int last, int next_first_used, const uint64_t state_in[2],
                         uint64_t state_out[2], uint64_t *nprot, uint32_t *err_bits);
int shk_stage_point_finish(shk_ctx *ctx, shk_point *out, shk_summary *accept);

/* One deNoise round now (the reference's --endDeNoise round; does not use up num_denoise).
 * Like every round (those fired inside the counting calls, shk_stage_try_denoise, the shk_stage_point_* steps) it drops
 * what qf_remove_singletons drops, whatever traveled marks the table carries (see shk_lookup): the reference's sweep
 * never looks at them, and neither does this one. */
int shk_denoise(shk_ctx *ctx, uint64_t *removed);

/* ---- filter-to-filter utilities
 * shk_insert_counted: add `counts[i]` occurrences of keys[i] (keys < 2^hb inside this context's quotient range), the
 *   batched form of qf_insert_advance(qf, key, 0, count, ...). No deNoise round fires inside (the reference tests its
 *   trigger after a chunk of reads only). stats->kmers = occurrences added, stats->new_distinct = keys that were new.
 * shk_dump: (key, count) of every entry, in the order qf_iterator/qfi_next visit them (ascending key); *n_out = number
 *   of entries; at most `cap` pairs are written; keys == NULL only counts. key = (quotient << 8) | remainder (qfi_get).
 *   The reference's qfi_next ends the iteration when it steps inside a run onto a slot behind nslots (gqf.c:2537-2539),
 *   so entries in the overflow tail that do not open their run, and all behind them, are invisible to its iterator and
 *   to qf_merge: ref_iterator_end != 0 makes *n_out that (smaller) number; 0 = every entry.
 * shk_merge: dst := dst + src -- what qf_merge(a, b, c) leaves in c for a = dst, b = src: the canonical table of the
 *   summed multiset (same geometry, same device). stats->kmers = occurrences added, new_distinct = keys new to dst.
 * shk_multi_merge: the same for several sources (qf_multi_merge).
 * shk_import_shards: replace the table (whole-filter context, num_shards <= 1) by the union of `nshards` quotient-range
 *   shards, each in the layout shk_export_blocks gives for a context with num_shards = nshards (its nslots / nshards
 *   quotients plus its own overflow tail). Device tables need 16 readable bytes behind them. nelts / ndistinct:
 *   the runtime counters for the header (0 = take the sums found in the shards). */
int shk_insert_counted(shk_ctx *ctx, const uint64_t *keys, const uint64_t *counts, uint64_t n, int on_device,
                       shk_batch_stats *stats);
int shk_dump(shk_ctx *ctx, uint64_t *keys, uint64_t *counts, uint64_t cap, int on_device, int ref_iterator_end,
             uint64_t *n_out);
int shk_merge(shk_ctx *dst, shk_ctx *src, shk_batch_stats *stats);
int shk_multi_merge(shk_ctx *dst, shk_ctx *const *srcs, uint32_t n, shk_batch_stats *stats);
int shk_import_shards(shk_ctx *ctx, const void *const *shard_blocks, const uint64_t *shard_bytes, uint32_t nshards,
                      int on_device, uint64_t nelts, uint64_t ndistinct);

/* ---- analytics on resident tables. Readers: like shk_export_blocks they may first launch the pending placement of their
 * operands. They work on a shard context too, over that shard's own quotients and overflow tail: the shards' histograms,
 * totals and inner products add up to the whole filter's (max_count: take the maximum). Traveled bits are ignored.
 * shk_spectrum: the abundance spectrum of the table. hist[i] (i < nbins-1) = entries whose count is i+1; hist[nbins-1] =
 *   entries whose count is >= nbins. hist is a host pointer unless on_device != 0; hist may be NULL with nbins 0 (totals
 *   only). After an error the content of hist is undefined. With F0 = distinct, F1 = total, f1 = hist[0], f2 = hist[1] the
 *   reference README's recipe reads N = F1, n = F0 - f1 - f2, e = 1 - ((F1 - f1 - 2 f2) / F1)^(1/k).
 * shk_inner_product: sum over the keys present in both of count_a * count_b, mod 2^64 (the reference accumulates in uint64_t).
 *   a and b must agree in qb, hb, shard_index, num_shards and device (SHK_ERR_ARG otherwise: the reference's different-sizes
 *   case is not supported); a == b is allowed. For two filters of equal size the reference ITERATES its second operand and
 *   looks each key up in the first (gqf.c:2714-2722), and its qfi_next ends the iteration when it steps inside a run onto a
 *   slot behind nslots (see shk_dump). ref_iterator_end != 0 reproduces that: entries of b at or behind its early-end point
 *   do not contribute, while the lookups into a see everything; apart from this the product is symmetric.
 *   ref_iterator_end == 0: every entry. An empty operand gives 0.
 * shk_magnitude: (uint64_t)sqrt((double)inner_product(ctx, ctx)) -- the reference's expression, gqf.c:2762.
 * shk_intersect: dst := the canonical table of { (key, count_b) : key in a and key in b } -- what qf_intersect(a, b, dst)
 *   inserts into an empty dst: the iterated operand b gives the counts (swap the arguments to keep a's). dst's former
 *   content is discarded, its traveled bits are zero; dst == a or dst == b is SHK_ERR_ARG, geometry as above. With
 *   ref_iterator_end != 0 b's entries behind the early end are left out. An empty operand gives an empty table.
 *   stats->kmers = sum of the counts written, stats->new_distinct = entries written; shk_stats(dst) reports the same as
 *   nelts and ndistinct. A corrupt source table is SHK_ERR_CORRUPT with nothing written. */
typedef struct shk_spectrum_totals {
  uint64_t distinct;   /* F0: entries */
  uint64_t total;      /* F1: sum of counts */
  uint64_t sumsq;      /* sum of count^2 mod 2^64 (= inner product of the filter with itself) */
  uint64_t max_count;  /* largest count present, 0 for an empty table */
} shk_spectrum_totals;
int shk_spectrum(shk_ctx *ctx, uint64_t *hist, uint32_t nbins, int on_device, shk_spectrum_totals *out);
int shk_inner_product(shk_ctx *a, shk_ctx *b, int ref_iterator_end, uint64_t *out);
int shk_magnitude(shk_ctx *ctx, int ref_iterator_end, uint64_t *out);
int shk_intersect(shk_ctx *dst, shk_ctx *a, shk_ctx *b, int ref_iterator_end, shk_batch_stats *stats);

int shk_stats(shk_ctx *ctx, shk_totals *out);
/* 128-byte quotient_filter_metadata image (gqf.h:62-77) for this context */
int shk_header(shk_ctx *ctx, uint8_t out[128]);
/* table bytes (nblocks * 89) to host memory. Counting calls commit lazily: they keep the rebuilt runs as per-region
 * records and leave the table's bytes unwritten until a call reads them, so this call (like every other reader: lookup,
 * dump, export, merge, the Contiger calls, shk_denoise) may first launch the placement kernel, once per build rather than
 * once per batch. SHK_LAZY_PLACE=0 in the environment of shk_create makes every counting call write the table itself. */
int shk_export_blocks(shk_ctx *ctx, void *host_dst, uint64_t cap);
/* device pointer and size of the live table; may launch the placement (see shk_export_blocks) and synchronises. The
 * pointer is valid until the next counting call (any call that rebuilds the table): the two table buffers alternate. */
int shk_table_ptr(shk_ctx *ctx, void **d_table, uint64_t *nbytes);
/* header + blocks, byte-identical to qf_serialize */
int shk_export_cqf(shk_ctx *ctx, const char *path);
/* replace the table by one read from a .cqf (whole filter; num_shards must be 1) */
int shk_import_cqf(shk_ctx *ctx, const char *path);
int shk_import_blocks(shk_ctx *ctx, const void *host_src, uint64_t nbytes, uint64_t nelts, uint64_t ndistinct);

/* mode 0: count + is_traveled, 1: count + set_traveled (returns the bit before), 2: count only.
 * keys/counts/was_traveled are host pointers unless on_device != 0. was_traveled may be NULL. A key outside this
 * context's quotient range answers 0 and marks nothing. One call may hold a key several times: under mode 1 exactly one
 * of them sees the bit unset (which one is not defined; the reference is sequential).
 * Traveled marks -- the contract:
 *   - they belong to readers: shk_lookup mode 1, shk_extend_forward / shk_unitigs_add_seeds with mark_traveled,
 *     shk_unitigs_add_reads and shk_select_seeds(use_traveled) set them on the first slot of an entry, mode 0 and the
 *     marking calls read them, shk_export_* / shk_import_* carry them;
 *   - no mark influences what any writer computes: counts, statistics, what a deNoise round removes and the bytes written
 *     are those of a table nobody marked;
 *   - every call that rebuilds the table leaves all traveled words zero: the counting calls, shk_insert_counted,
 *     shk_merge / shk_multi_merge / shk_import_shards, shk_denoise, shk_stage_commit / shk_stage_accept, shk_intersect.
 *   The reference leaves stale bits at slot positions when an insert shifts slots (its bits do not move with the
 *   entries); that is not reproduced. */
int shk_lookup(shk_ctx *ctx, const uint64_t *keys, uint64_t n, int on_device, int mode,
               uint64_t *counts, uint8_t *was_traveled);

/* ---- Contiger, first slice: forward extension of many open unitig ends at once.
 * For end i: cur_kmers[i*k ..] is the contig's last k-mer, first_kmers[i*k ..] its first (upper-case ACGT). Per
 * step the kernel looks up the 4 successors and the 3 siblings of the current k-mer and applies the reference's
 * rule (stop on a solid sibling or > 1 solid successor; extend on exactly one; stop on none or on a pure
 * circle), for a walk that meets no other unitig (no startKmer2unitig hits). out_bases/out_counts hold up to
 * max_ext appended bases and the filter counts of the k-mers they complete, out_n their number, out_stop why
 * the walk ended (SHK_STOP_*), out_branch (may be NULL) at a SHK_STOP_BRANCH the solid neighbours of the last
 * k-mer s0 s1..s(k-1): bit x = successor s1..s(k-1)+x, bit 4+z = sibling z+s1..s(k-1) (x, z index "ACGT"); out_ncount (may be NULL, 8 per end) their filter counts. mark_traveled != 0 sets the traveled bit of every k-mer looked up, as the
 * reference's count_key_value_set_traveled does. 2 <= k <= 191. All pointers are host pointers. */
#define SHK_STOP_BRANCH 1
#define SHK_STOP_DEAD_END 2
#define SHK_STOP_CIRCLE 3
#define SHK_STOP_BUFFER 4
#define SHK_STOP_BAD_SEED 5
int shk_extend_forward(shk_ctx *ctx, const char *cur_kmers, const char *first_kmers, uint32_t n, uint32_t k,
                       uint64_t abundance_min, int mark_traveled, uint32_t max_ext, char *out_bases,
                       uint32_t *out_counts, uint32_t *out_n, uint8_t *out_stop, uint8_t *out_branch,
                       uint32_t *out_ncount);
/* One maximal unitig per seed k-mer: extend, reverse-complement, extend again; out_seq[i*max_len ..] holds
 * out_len[i] bases, out_median[i] the contig's median abundance as the reference stores it (int),
 * out_stop[2*i], out_stop[2*i+1] the two stop reasons. seed_counts[i] = the seed's filter count. 2 <= k <= 191. */
int shk_unitigs_from_seeds(shk_ctx *ctx, const char *seeds, const uint32_t *seed_counts, uint32_t n, uint32_t k,
                           uint64_t abundance_min, uint32_t max_len, char *out_seq, uint32_t *out_len,
                           int32_t *out_median, uint8_t *out_stop);

/* All unitigs reachable from the seeds, written as FASTA in the reference's record grammar
 * (`>i LN:i:len KC:i:median*(len-k+1) km:f:median L:+:j:+ ... L:-:j:- ...`, successors in A,C,G,T order, predecessors
 * in T,G,C,A order, src/contig_assembly.cpp:606-626, 1012-1084): seeds are extended in both directions, every solid
 * neighbour met at a branch starts a new contig (the reference's work queue), a unitig found more than once is
 * kept once. The reference produces the same set of sequences up to reverse complement; ids and order are its
 * thread schedule's and are not reproduced. 2 <= k <= 191 here and in the unitig set's calls below; the device holds a
 * k-mer in 2, 4 or 6 64-bit words (k <= 64, 128, 191), so k <= 64 costs what it always did. */
typedef struct shk_unitig_stats {
  uint64_t unitigs, total_len;   /* kept unitigs and their summed length */
  uint64_t rounds, extensions;   /* launches of the walk kernel; bases appended by all walks (duplicates included) */
  uint64_t duplicates, truncated;/* unitigs found again and dropped; walks cut at max_len */
} shk_unitig_stats;
int shk_find_unitigs(shk_ctx *ctx, const char *seeds, const uint32_t *seed_counts, uint32_t n, uint32_t k,
                     uint64_t abundance_min, uint32_t max_len, const char *out_path, shk_unitig_stats *stats);
/* The same in pieces, for callers that feed seeds batch by batch (the Contiger command line): a unitig set that
 * accumulates over calls. With mark_traveled != 0 every k-mer an extension looks up is marked, so that
 * shk_select_seeds(use_traveled = 1) on later reads skips seeds inside unitigs that are already known -- the
 * reference's own pruning (contig_assembly.cpp:1871-1873). A set keeps the k of its first call: a later call with
 * another k returns SHK_ERR_ARG. */
typedef struct shk_unitig_set shk_unitig_set;
shk_unitig_set *shk_unitig_set_new(void);
void shk_unitig_set_free(shk_unitig_set *u);
int shk_unitigs_add_seeds(shk_ctx *ctx, shk_unitig_set *u, const char *seeds, const uint32_t *seed_counts, uint32_t n,
                          uint32_t k, uint64_t abundance_min, uint32_t max_len, int mark_traveled);
int shk_unitig_set_write(shk_unitig_set *u, uint32_t k, const char *out_path, shk_unitig_stats *stats);
/* The command line's inner loop without the seeds leaving the device: the seeds of the reads in the given FASTQ chunks
 * (rule of shk_select_seeds with use_traveled = 1) become contigs and are walked at once, every lookup marking the
 * traveled bit as the reference's does. *nseeds (may be NULL) = seeds taken from this batch. */
int shk_unitigs_add_reads(shk_ctx *ctx, shk_unitig_set *u, const void *text, int text_on_device, uint64_t text_bytes,
                          const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks, uint32_t k,
                          uint64_t abundance_min, uint64_t count_min, uint64_t count_max, uint32_t max_len, uint64_t *nseeds);
/* Seeds of the reads in the given FASTQ chunks (processDataChunk, contig_assembly.cpp:1856-1876): the k-mer at
 * len/2 - k/2 of every read, upper-cased, without 'N', whose filter count lies in [count_min, count_max]; with
 * use_traveled != 0 the lookup marks the k-mer and a k-mer that was already marked gives no seed. out_seeds
 * receives *n_out * k bases (capacity cap seeds), out_counts their counts. 2 <= k <= 191. */
int shk_select_seeds(shk_ctx *ctx, const void *text, int text_on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                     const uint64_t *chunk_len, uint32_t nchunks, uint32_t k, uint64_t count_min, uint64_t count_max,
                     int use_traveled, char *out_seeds, uint32_t *out_counts, uint32_t cap, uint32_t *n_out);

/* per-kernel device time measured with HIP events on the context's stream */
typedef struct shk_kernel_time {
  const char *name;
  uint64_t launches;
  double ms;
} shk_kernel_time;
int shk_profile_enable(shk_ctx *ctx, int on);
int shk_profile_get(shk_ctx *ctx, shk_kernel_time *out, int cap);  /* returns #entries */
int shk_profile_reset(shk_ctx *ctx);

const char *shk_strerror(int code);
/* last kernel error bits (diagnostics) */
uint32_t shk_last_error_bits(shk_ctx *ctx);
/* diagnostics: batches since shk_create whose key words left the first partition level as split records (4 + 1 bytes per
 * key instead of 8, between the roll kernels and the middle level of a three-level context that owns the whole filter;
 * SHK_RP_SPLIT=0, read by shk_create, keeps every batch on 8-byte words). The profile's kernel names do not tell. */
uint64_t shk_split_batches(shk_ctx *ctx);
/* diagnostics: launches of the record-sourced rebuild kernels since shk_create that loaded every region's old record and
 * first words up front. They do so when the batch in hand brings eight words per region or more; SHK_MERGE_PREFETCH=0, read
 * by shk_create, keeps every launch on the dependent loads. The results are the same either way. */
uint64_t shk_prefetch_passes(shk_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
