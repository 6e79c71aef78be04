// Host side of libshk.so: context, buffers, launch sequences. See include/shk.h for the
// reference interface each entry point replaces. Everything here runs on one HIP stream
// per context; the only host<->device synchronisations in a batch are the one that reads
// the merge statistics (needed to decide where a deNoise round fires) and the final one.
#include "../../include/shk.h"
#include <thread>

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <string>
#include <algorithm>
#include <unordered_set>
#include <unordered_map>

#include "kmer_kernels.hip"
#include "roll_kernels.hip"
#include "partition_kernels.hip"
#include "cqf_kernels.hip"
#include "merge2_kernels.hip"
#include "walk_kernels.hip"
#include "unitig_kernels.hip"
#include "fasta_kernels.hip"
#include "query_kernels.hip"
#include "reads_kernels.hip"
#include "correct_kernels.hip"

#define SHK_SLACK 256  // bytes of slack behind buffers read with wide loads

enum {
  KP_COUNT_LINES, KP_SCAN_CHUNKS, KP_EMIT_READS, KP_COUNT_KEYS, KP_HASH, KP_SCAN, KP_RP_PREP, KP_RP_HIST,
  KP_RP_SCATTER, KP_MERGE_SUM, KP_REGION_SCAN, KP_MERGE_WRITE, KP_MERGE_SPILL, KP_PLACE, KP_MARKS, KP_LOOKUP, KP_WALK, KP_UG_WALK, KP_UG_FINISH, KP_MERGE_FUSED, KP_MERGE_SAMPLE, KP_MISC, KP_ROLL_HIST, KP_ROLL_SCATTER, KP_PACK, KP_RP_SLOTS, KP_RP_SCATTER_NARROW, KP_SPECTRUM, KP_JOIN, KP_FA_MAPS, KP_FA_STATES, KP_FA_COUNT, KP_FA_COMPACT, KP_FA_SEGMENTS, KP_FA_PACK, KP_ROLL_SAMPLE, KP_ROLL_QUERY, KP_FA_REC_STARTS, KP_READS_QUERY, KP_READS_MEDIAN, KP_READS_CORRECT, KP_N
};
static const char *kp_names[KP_N] = {
  "k_count_lines", "k_scan_chunks", "k_emit_reads", "k_count_keys", "k_hash_reads", "k_scan_*", "k_rp_prep",
  "k_rp_hist", "k_rp_scatter", "k_region_merge<summary>", "k_region_scan", "k_region_merge<write>",
  "k_region_merge<spill>", "k_region_place", "k_denoise_marks", "k_lookup", "k_extend_forward+k_select_seeds", "k_ug_walk", "k_ug_check/emit/median/links", "k_region_merge<fused>", "k_region_merge<sample>", "misc", "k_roll_hist", "k_roll_scatter", "k_pack_reads", "k_rp_slot_cursors", "k_rp_scatter<narrow>", "k_region_spectrum", "k_region_join", "k_fa_maps", "k_fa_states", "k_fa_count", "k_fa_compact", "k_fa_segments+long+tail", "k_fa_pack", "k_roll_sample", "k_roll_query", "k_fa_rec_starts", "k_reads_query", "k_reads_median", "k_reads_correct"};

struct PendingEvent { int id; hipEvent_t a, b; };

// The 64 words of ShkStageBufs::d_scalars. Kernels take pointers to them; an entry point runs alone on its context, so
// slots of different owners are never in flight together.
#define SHK_SCALAR_WORDS 64
enum ShkDevSlot {
  DS_NREADS = 0,       // parse_stage: reads of the batch (k_scan_chunks writes it; the key-count, hash, pack and roll kernels read it)
  DS_NWORDS = 1,       // hash_stage, roll_stage, set_nwords: key words of the batch (the partition kernels read it)
  DS_SCAN_TOTAL = 2,   // run_scan: total of the scan in flight
  DS_MARKS = 3,        // k_denoise_marks, k_denoise_marks_virtual: singletons the range walk protects
  DS_MAX_COUNT = 4,    // shk_insert_counted: largest count of the slice (k_expand_counted<0>)
  DS_DUMP_STOP = 5,    // shk_dump: where the reference's iterator would end
  DS_JOIN_STOP = 6,    // shk_inner_product, shk_intersect: the key at which the reference's iteration of b ends (k_region_iter_end)
  DS_JOIN_ACC = 7,     // shk_inner_product: the sum
  DS_WALK_IN = 8,      // point_walk: state of the range walk entering this shard, 2 words
  DS_WALK_OUT = 10,    // point_walk: ... and leaving it, 2 words
  DS_SPECTRUM = 12,    // shk_spectrum: the totals, SHK_SPEC_WORDS = 4 words
  DS_STAMPS = 16,      // SHK_STAMPS diagnostics: 16 words of cycle counts (ShkMergeArgs::dbg)
  DS_SAMPLE = 32,      // shk_sample_chunks: k_roll_sample's two counters (words kept, k-mers hashed), 2 words
  DS_PAIR_LEN = 40,    // shk_stage_words_pair: lengths of the two sources, 2 words
  DS_PAIR_BASE = 42,   // shk_stage_words_pair: their one-bucket base arrays {0, na} and {0, nb}, 2 + 2 words
  DS_EXTENT = 46,      // a batch with slotted upper levels: positions (all slots) of the roll kernels' output, word 0, and of the
                       // middle level's, word 1 -- what the partition kernels take as their input's length in place of DS_NWORDS
  DS_END = 48
};
// The 64 words of the pinned mirror ShkStageBufs::h_pinned: what the host reads back, and small uploads' sources.
enum ShkHostSlot {
  HP_COUNTERS = 0,     // merge_summary, point_read, merge2_run: d_counters, SHK_NCOUNTERS words (CNT_*, SHK_CNT_*)
  HP_SPECTRUM = 8,     // shk_spectrum: DS_SPECTRUM read back, 4 words
  HP_SAMPLE = 12,      // shk_sample_chunks: DS_SAMPLE read back, 2 words
  HP_ERR = 40,         // err_enqueue / err_take: the error word (4 bytes)
  HP_NREADS = 41,      // parse_stage: DS_NREADS read back
  HP_NWORDS = 42,      // front_end, shk_hash_chunks: DS_NWORDS read back
  HP_NWORDS_IN = 43,   // set_nwords: source of the upload to DS_NWORDS
  HP_FREE_PTR = 44,    // shk_stats: free pointer behind the last region
  HP_TOTAL = 45,       // shk_insert_counted: words of the slice; shk_dump: entries; unitig write: units
  HP_AUX = 46,         // shk_insert_counted: DS_MAX_COUNT read back; shk_dump: DS_DUMP_STOP in and out; unitig write: total length;
                       // shk_inner_product: DS_JOIN_ACC read back
  HP_MARKS = 47,       // point_walk: DS_MARKS read back
  HP_IFIN = 48,        // point_try: free pointer behind the intermediate table's last region
  HP_IFIRST = 49,      // point_try: first length byte of the intermediate table (quotient 0 has a run)
  HP_WALK_IN = 50,     // point_walk: source of the upload to DS_WALK_IN, 2 words
  HP_WALK_OUT = 52,    // point_walk: DS_WALK_OUT read back, 2 words
  HP_PAIR = 56,        // shk_stage_words_pair: source of the upload to DS_PAIR_LEN and DS_PAIR_BASE, 6 words
  HP_END = 62
};
enum { CNT_NEWD, CNT_ADDED, CNT_REMOVED, CNT_ADDED_BEFORE };   // counters[0..3]: the statistics of a pass (ShkMergeArgs::counters)
static_assert(HP_COUNTERS + SHK_NCOUNTERS <= HP_ERR, "the counters mirror ends before the error word");
static_assert(HP_COUNTERS + SHK_NCOUNTERS <= HP_SPECTRUM && DS_SPECTRUM + (int)SHK_SPEC_WORDS <= DS_STAMPS, "the spectrum's totals have four words of their own");
static_assert(DS_END <= SHK_SCALAR_WORDS && HP_END <= SHK_SCALAR_WORDS, "both blocks fit their 64 words");
static_assert(DS_STAMPS + 16 <= DS_SAMPLE && DS_SAMPLE + 2 <= DS_PAIR_LEN && HP_SPECTRUM + (int)SHK_SPEC_WORDS <= HP_SAMPLE && HP_SAMPLE + 2 <= HP_ERR, "the sample counters have two words of their own");
static_assert(DS_PAIR_BASE + 4 == DS_EXTENT && HP_PAIR + (DS_EXTENT - DS_PAIR_LEN) == HP_END, "the pair block is uploaded in one copy");

// How a partition level runs, fixed by the geometry (create_init); a batch adds what its producer has counted already
// (ShkPartInput::counted) and whether region slots are worth trying (slot_capacity).
enum { RP_SCATTER_GROUPED, RP_SCATTER_WIDE, RP_SCATTER_TILE };   // 16384-key windows with window groups; with PMAX 256; 4096-key windows
struct ShkPartLevel {
  uint8_t scatter;     // k_rp_scatter instantiation
  bool pair_hist;      // when this level's words arrive unsorted, its counting pass also counts the next level (k_rp_hist2)
  bool may_slot;       // the last level, of index >= 1, with 4-byte output: region slots instead of a counting pass
  bool may_narrow;     // the k_rp_scatter level in front of the last one: it may hand the last level 4-byte records
                       // (partition_kernels.hip: the narrow record) when the batch's chunk tags fit ShkRpLevel::cb bits
};

// What a front end (parse, hash or roll, partition) works in: its stream, every buffer it writes, the state of its
// partition and the kernel times recorded on its stream. A context is one (the serial front end and everything behind
// it run there); the overlapped front end owns a second (ShkFront). The stage functions take the context for geometry and
// configuration, which they only read, and one of these for everything they change.
struct ShkStageBufs {
  hipStream_t stream = hipStream_t();
  bool lent = false;            // d_words[] and d_base[nlevels] are lent by the owner batch by batch (bufs_alloc, bufs_free)
  uint8_t *d_text = nullptr;
  uint64_t *d_chunk_off = nullptr, *d_chunk_len = nullptr, *d_nlines = nullptr, *d_reads_base = nullptr;
  uint64_t *d_rd_start = nullptr, *d_rd_end = nullptr;
  uint16_t *d_rd_chunk = nullptr;         // chunk (within the call) of every read
  uint16_t *d_nlmask = nullptr;           // newline flags of the text in hand, one word per 16-byte unit (k_count_lines -> k_emit_reads);
  uint64_t nlmask_units = 0;              // its capacity. Null in a context created with SHK_PARSE_MASK=0; parse_stage grows it
  uint32_t *d_nkeys = nullptr;
  uint64_t *d_key_base = nullptr;
  uint64_t *d_words[2] = {};
  uint64_t *d_scalars = nullptr;          // [SHK_SCALAR_WORDS], see ShkDevSlot
  uint64_t *d_block_sums = nullptr;
  uint64_t *d_hist[4] = {};               // per level: nbuckets*P (first level: times its window groups)
  uint64_t *d_base_sub = nullptr;         // first level with window groups: scanned bases of the (digit, group) sub-buckets
  uint64_t *d_base[5] = {};               // base[l]: bucket bases entering level l (base[nlevels] = region_base)
  uint64_t *d_cursor = nullptr;
  uint64_t *d_end[3] = {};                // end[l], l = 1, 2: ends of the slotted buckets entering level l (contexts whose plan has roll_slots)
  uint32_t *d_tfb = nullptr;
  uint32_t *d_err = nullptr;
  uint64_t *h_pinned = nullptr;           // [SHK_SCALAR_WORDS] pinned, see ShkHostSlot
  uint32_t last_err_bits = 0;
  uint32_t region_cap = 0;      // how the partitioned words lie: 0 = d_base[nlevels] holds exact offsets; else region r owns the slot
                                // [r * region_cap, ...) and d_base[nlevels][r] is its END (ShkRpLevel::slot_cap)
  uint32_t slot_overflows = 0;  // consecutive batches whose slotted last level overflowed; at 2 the slots are switched off
  int slots_off = 0;
  uint64_t roll_cap = 0;        // the batch in hand: 0 = roll_stage left exact bucket bases; else digit d owns the slot [d * roll_cap, ...)
                                // of d_words[0] and d_end[1][d] is its end (k_roll_slot_ends)
  bool roll_split = false;      // the batch in hand: d_words[0] holds the split record's two planes (roll_keys), not 8-byte words
  uint64_t split_batches = 0;   // batches that took that form (shk_split_batches)
  uint32_t up_overflows = 0;    // consecutive batches whose slotted upper levels overflowed (SHK_E_SLOT_FULL_UP); at 2 they are
  int up_off = 0;               // switched off. Apart from slot_overflows, which counts the last level's
  // profiling
  double prof_ms[KP_N] = {};
  uint64_t prof_n[KP_N] = {};
  std::vector<PendingEvent> pending;
  std::vector<hipEvent_t> evpool;
};

struct shk_ctx : ShkStageBufs {
  shk_config cfg;
  int dev;
  // geometry of this context (shard)
  uint64_t g_nslots;            // whole filter
  uint64_t q_lo, nslots, xnslots, nblocks, table_bytes;
  uint32_t nregions, rbits;     // regions and ceil(log2(nregions))
  uint32_t nlevels;
  ShkRpLevel lv[4];
  ShkPartLevel part[4];         // the partition plan, level by level
  bool roll_two;                // roll_stage's histogram pass counts the first two levels' digits together (they fit its LDS bins)
  bool roll_slots;              // three levels, all slotted: a narrow batch of text runs without any counting pass (roll_stage)
  uint32_t split_kb;            // 0 = off, else the key bits of the split record between the roll kernels and the middle level
                                // (partition_kernels.hip): three levels, the middle one may be narrow, the whole filter is this context's
  bool parse_mask;              // k_count_lines keeps the newline flags and k_emit_reads reads them, not the text (parse_stage)
  uint32_t threads, hash_groups;
  // state
  uint64_t nelts, ndistinct;
  uint32_t rounds_left, rounds_done;
  // device buffers
  uint8_t *tab[2];
  uint64_t *fin[2];
  int cur;                      // which of tab[]/fin[] is live
  uint8_t *d_up[2];             // shk_upload_text: two alternating buffers filled on a copy stream
  hipStream_t copy_stream;
  hipEvent_t up_done[2];
  int up_next, up_pending[2];
  uint32_t *d_summary;
  long long *d_tile_a, *d_tile_b, *d_tile_f;
  uint64_t *d_dump_offs;        // [nregions + 2] shk_dump: where every region's entries start in the output
  int big_image;                // 1: rebuild kernels run with the SHK_IMG_BLOCKS_BIG image (set after a cluster outgrew the small one)
  // the summary launch spills lengths + encodings per region, k_region_place writes table B from them
  // Lazy placement: a clean pass is committed by keeping its records (and the free pointers of its scan) as the truth;
  // the next pass reads them as its old side (the OLDREC instantiations of k_region_merge) and writes the other buffer;
  // the table's bytes are produced when somebody looks at them (table_sync).
  uint8_t *spill[2];            // a pass writes spill_out(); [1] is allocated by the first lazy commit or a *_reserve call
  int live;                     // which of the two buffers holds the records of the last lazy commit
  int rec_live;                 // 1: spill[live] + fin[cur] describe the live table (a pass may take its old side from them)
  int table_stale;              // 1: tab[cur] has not been written from them yet, or its placement failed (implies rec_live)
  int lazy_ok;                  // 0: every commit places (SHK_LAZY_PLACE=0, or the second record buffer did not fit)
  int foreign_marks;            // 1: tab[cur] may hold traveled bits a reader set (lookup mode 1, the marking Contiger calls) or
                                // an import brought in; a deNoise round zeroes them before its own marks (marks_launch). A
                                // rebuild that makes the other table live clears the flag: rebuilt tables have no marks
  uint32_t *d_over_list;
  // what the spill records currently describe (a write pass may use them only for the same request)
  int spill_valid; const uint64_t *spill_words; uint32_t spill_lo, spill_hi; int spill_denoise, spill_big;
  uint64_t spill_nover;
  uint16_t *d_newchunks;        // first chunks of new keys per region (exact deNoise point in one pass); null without deNoise rounds
  unsigned long long *d_chist;  // [SHK_MAX_CHUNKS]
  uint64_t *h_chist;            // pinned
  uint32_t chist_n;             // entries of h_chist valid from the last summary (0 = none)
  uint32_t sample_stride;       // sampled statistics pass before a deNoise point: every n-th region (<= 1: off)
  uint32_t pt_lo, pt_split, pt_hi; int pt_valid; uint64_t pt_nprot;   // one-pass deNoise point in progress (shk_stage_point_*)
  const uint64_t *pt_words;     // its words (null: a round on its own, shk_stage_round_try)
  unsigned long long *d_counters;  // [SHK_NCOUNTERS]
  uint64_t max_reads;
  int prof_on;                  // profiling: kernel times are recorded (ShkStageBufs::prof_ms)
  double new_frac;              // new distinct keys per presented k-mer in the last committed range (predicts crossings)
  int staged;                   // which d_words[] holds the partitioned words of shk_stage_words
  // The record-sourced rebuild kernels load a region's old record and its first words before they know whether the region
  // has any (ShkMergeArgs::prefetch): right for a dense pass, wasted bytes where most regions are empty and leave at once.
  uint64_t pass_words;          // words of the partitioned batch in hand (merge_stage, shk_stage_words*)
  int prefetch_ok;              // 0: never (SHK_MERGE_PREFETCH=0)
  uint64_t prefetch_passes;     // launches that ran with the early loads (shk_prefetch_passes)
  // one-pass deNoise point (denoise_fused): the intermediate table's (T, c), run lengths and free pointers; protected quotients
  uint32_t *d_isum; uint8_t *d_ilens; uint64_t *d_fin_i; uint64_t *d_prot;
  int counted;                  // 1 while shk_insert_counted runs: the words' chunk field is a multiplicity
  uint64_t *d_send[2];          // shk_route_words: two alternating send buffers (allocated on first use), so that the
  int send_next;                // exchange of one batch can run while the next batch is hashed and routed
  struct ShkFront *front;       // shk_prepare_chunks: the front end (parse, hash, partition) of later batches on its own stream
  struct ShkFasta *fasta;       // shk_count_fasta, shk_query_fasta: their buffers and the states of their streams (allocated by the first call)
  uint32_t fasta_seg;           // k-mers per segment there (SHK_FASTA_SEGMENT)
  struct ShkReads *reads;       // shk_query_reads: its buffers (allocated by the first call)
  struct ShkCorrect *correct;   // shk_correct_reads: its buffers (allocated by the first call)
};

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "libshk: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); return SHK_ERR_HIP; } } while (0)

static hipEvent_t ev_get(ShkStageBufs *c) {
  if (!c->evpool.empty()) { hipEvent_t e = c->evpool.back(); c->evpool.pop_back(); return e; }
  hipEvent_t e; hipEventCreate(&e); return e;
}
struct ProfScope {
  ShkStageBufs *c; int id; bool on; hipEvent_t a, b;
  ProfScope(const shk_ctx *ctx, ShkStageBufs *c_, int id_) : c(c_), id(id_), on(ctx->prof_on != 0) {
    if (on) { a = ev_get(c); b = ev_get(c); hipEventRecord(a, c->stream); }
  }
  ProfScope(shk_ctx *ctx, int id_) : ProfScope(ctx, ctx, id_) {}
  ~ProfScope() {
    if (on) { hipEventRecord(b, c->stream); PendingEvent p = {id, a, b}; c->pending.push_back(p); }
  }
};
static void prof_collect(ShkStageBufs *c) {
  for (size_t i = 0; i < c->pending.size(); i++) {
    float ms = 0;
    hipEventSynchronize(c->pending[i].b);
    hipEventElapsedTime(&ms, c->pending[i].a, c->pending[i].b);
    c->prof_ms[c->pending[i].id] += ms;
    c->prof_n[c->pending[i].id]++;
    c->evpool.push_back(c->pending[i].a);
    c->evpool.push_back(c->pending[i].b);
  }
  c->pending.clear();
}

static int map_err_bits(uint32_t bits) {
  if (!bits) return SHK_OK;
  if (bits & SHK_E_TABLE_FULL) return SHK_ERR_TABLE_FULL;
  if (bits & (SHK_E_OLD_EXTENT | SHK_E_NEW_EXTENT | SHK_E_HASH_FULL | SHK_E_RUN_TOO_LONG)) return SHK_ERR_REGION;
  if (bits & SHK_E_CORRUPT) return SHK_ERR_CORRUPT;
  if (bits & SHK_E_BAD_FASTQ) return SHK_ERR_FASTQ;
  if (bits & SHK_E_KEYS_FULL) return SHK_ERR_BATCH;
  return SHK_ERR_CORRUPT;
}

extern "C" const char *shk_strerror(int code) {
  switch (code) {
    case SHK_OK: return "ok";
    case SHK_ERR_ARG: return "bad argument or unsupported geometry";
    case SHK_ERR_HIP: return "HIP runtime error (is a GPU present?)";
    case SHK_ERR_TABLE_FULL: return "counting quotient filter is full";
    case SHK_ERR_REGION: return "a 256-quotient region exceeds the kernel's on-chip image or hash";
    case SHK_ERR_CORRUPT: return "table metadata inconsistent or key outside this context's range";
    case SHK_ERR_FASTQ: return "malformed FASTQ input";
    case SHK_ERR_BATCH: return "batch exceeds the capacities given to shk_create";
    case SHK_ERR_IO: return "file I/O error";
  }
  return "unknown error";
}
extern "C" uint32_t shk_last_error_bits(shk_ctx *c) { return c ? c->last_err_bits : 0; }

template <typename T> static int dmalloc(T **p, uint64_t n) {
  void *v = nullptr;
  HIPCHK(hipMalloc(&v, n * sizeof(T) + SHK_SLACK));
  *p = (T *)v;
  return 0;
}

// ------------------------------------------------------------------ create / destroy
static int ensure_chist(shk_ctx *c);
static int point_alloc(shk_ctx *c);
// buckets leaving partition level l (= entries of d_hist[l] without window groups, of d_base[l + 1])
static uint64_t level_out(const shk_ctx *c, uint32_t l) { return (uint64_t)c->lv[l].nbuckets << c->lv[l].bits; }

// The stream and the buffers of one front end, sized from the context's geometry. lent: the overlapped front end, whose
// two words buffers and last-level bases are its slots' (set batch by batch; not allocated and not freed here).
// words of every buffer that can be d_words[]: slotted upper levels need room for a full batch plus the slots' slack
// (128 slots of a 6.5 M share: 837.5 M words for 832 M keys)
static uint64_t words_cap(const shk_ctx *c) { return c->cfg.max_batch_keys + (c->roll_slots ? c->cfg.max_batch_keys / 64 : 0); }

// (exactly `units` words, without dmalloc's slack: the 8 units of room behind the text's last unit are part of the count)
static int nlmask_alloc(ShkStageBufs *b, uint64_t units) {
  void *v = nullptr;
  if (hipMalloc(&v, units * sizeof(uint16_t)) != hipSuccess) { (void)hipGetLastError(); return SHK_ERR_HIP; }
  b->d_nlmask = (uint16_t *)v;
  b->nlmask_units = units;
  return 0;
}

static int bufs_alloc(const shk_ctx *c, ShkStageBufs *b, bool lent) {
  const uint64_t capk = c->cfg.max_batch_keys;
  const uint32_t maxch = SHK_MAX_CHUNKS;
  b->lent = lent;
  // (a higher stream priority changes nothing measurable: the rebuild's small workgroups refill every CU as fast as they
  // leave it, whatever the priority of the queue whose big workgroups are waiting)
  if (lent) HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  else HIPCHK(hipStreamCreate(&b->stream));
  if (dmalloc(&b->d_text, c->cfg.max_batch_bytes + 64)) return SHK_ERR_HIP;
  // Host text is at most max_batch_bytes; device text has no configured bound: four text bytes per key cover ordinary
  // short-read FASTQ, so that a fresh context's first batch allocates nothing (parse_stage grows the buffer otherwise)
  if (c->parse_mask) {
    const uint64_t tb = c->cfg.max_batch_bytes > 4 * capk ? c->cfg.max_batch_bytes : 4 * capk;
    if (nlmask_alloc(b, tb / 16 + 8)) return SHK_ERR_HIP;
  }
  if (dmalloc(&b->d_chunk_off, maxch) || dmalloc(&b->d_chunk_len, maxch) || dmalloc(&b->d_nlines, (uint64_t)maxch * SHK_PARSE_SEGS) ||
      dmalloc(&b->d_reads_base, maxch + 1)) return SHK_ERR_HIP;
  if (dmalloc(&b->d_rd_start, c->max_reads + 1) || dmalloc(&b->d_rd_end, c->max_reads + 1) ||
      dmalloc(&b->d_nkeys, c->max_reads + 1) || dmalloc(&b->d_rd_chunk, c->max_reads + 1) || dmalloc(&b->d_key_base, c->max_reads + 2)) return SHK_ERR_HIP;
  if (!lent && (dmalloc(&b->d_words[0], words_cap(c) + 1) || dmalloc(&b->d_words[1], words_cap(c) + 1))) return SHK_ERR_HIP;
  if (dmalloc(&b->d_scalars, SHK_SCALAR_WORDS)) return SHK_ERR_HIP;
  HIPCHK(hipMemsetAsync(b->d_scalars, 0, SHK_SCALAR_WORDS * 8, b->stream));
  {
    uint64_t mx = capk > c->max_reads ? capk : c->max_reads;
    uint64_t pw = 1ULL << c->rbits;
    if (pw > mx) mx = pw;
    if (dmalloc(&b->d_block_sums, mx / SHK_SCAN_TILE + 4 + 8192)) return SHK_ERR_HIP;
  }
  if (dmalloc(&b->d_base[0], 2)) return SHK_ERR_HIP;
  for (uint32_t l = 0; l < c->nlevels; l++) {
    const uint64_t n = level_out(c, l);
    if (dmalloc(&b->d_hist[l], (n << c->lv[l].ng_log2) + 1)) return SHK_ERR_HIP;
    if (!(lent && l + 1 == c->nlevels) && dmalloc(&b->d_base[l + 1], n + 2)) return SHK_ERR_HIP;
    if (l == 0 && dmalloc(&b->d_base_sub, (n << c->lv[0].ng_log2) + 2)) return SHK_ERR_HIP;
  }
  { const uint64_t nb = level_out(c, c->nlevels - 1), first = 1ULL << (c->lv[0].bits + c->lv[0].ng_log2);
    if (dmalloc(&b->d_cursor, (nb > first ? nb : first) + 2)) return SHK_ERR_HIP; }
  // (windows of 4096 positions; a slotted middle level's output is up to two 4-byte records per word of its buffer)
  if (dmalloc(&b->d_tfb, (c->roll_slots ? 2 * words_cap(c) : capk) / SHK_RP_TILE + 2)) return SHK_ERR_HIP;
  if (c->roll_slots && (dmalloc(&b->d_end[1], level_out(c, 0) + 2) || dmalloc(&b->d_end[2], level_out(c, 1) + 2))) return SHK_ERR_HIP;
  if (dmalloc(&b->d_err, 4)) return SHK_ERR_HIP;
  HIPCHK(hipMemsetAsync(b->d_err, 0, 16, b->stream));
  HIPCHK(hipHostMalloc((void **)&b->h_pinned, SHK_SCALAR_WORDS * sizeof(uint64_t), hipHostMallocDefault));
  HIPCHK(hipStreamSynchronize(b->stream));
  return SHK_OK;
}

// (of a partly built object too: whatever bufs_alloc did not reach is null)
static void bufs_free(const shk_ctx *c, ShkStageBufs *b) {
  if (b->stream) hipStreamSynchronize(b->stream);
  prof_collect(b);
  for (size_t i = 0; i < b->evpool.size(); i++) hipEventDestroy(b->evpool[i]);
  b->evpool.clear();
  hipFree(b->d_text); hipFree(b->d_chunk_off); hipFree(b->d_chunk_len); hipFree(b->d_nlines); hipFree(b->d_reads_base);
  hipFree(b->d_nlmask);
  hipFree(b->d_rd_start); hipFree(b->d_rd_end); hipFree(b->d_rd_chunk); hipFree(b->d_nkeys); hipFree(b->d_key_base); hipFree(b->d_scalars);
  hipFree(b->d_block_sums); hipFree(b->d_base_sub); hipFree(b->d_cursor); hipFree(b->d_end[1]); hipFree(b->d_end[2]); hipFree(b->d_tfb); hipFree(b->d_err);
  if (!b->lent) { hipFree(b->d_words[0]); hipFree(b->d_words[1]); }
  for (uint32_t l = 0; l < 4; l++) hipFree(b->d_hist[l]);
  for (uint32_t l = 0; l < 5; l++) if (!(b->lent && l == c->nlevels)) hipFree(b->d_base[l]);
  hipHostFree(b->h_pinned);
  if (b->stream) hipStreamDestroy(b->stream);
  *b = ShkStageBufs();
}

// geometry, buffers and tables of a new context; whatever it leaves behind on failure is shk_destroy's
static int create_init(shk_ctx *c, const shk_config *cfg) {
  const uint32_t ns = cfg->num_shards ? cfg->num_shards : 1;
  c->cfg = *cfg;
  c->dev = cfg->device;
  HIPCHK(hipSetDevice(c->dev));
  c->g_nslots = 1ULL << cfg->qb;
  if (c->g_nslots / ns < 64) return SHK_ERR_ARG;
  c->nslots = c->g_nslots / ns;
  c->q_lo = c->nslots * cfg->shard_index;
  // qf_init geometry, gqf.c:2197-2198 (every shard keeps a full-size overflow tail)
  c->xnslots = c->nslots + (uint64_t)(10 * sqrt((double)c->g_nslots));
  c->nblocks = (c->xnslots + 63) / 64;
  c->table_bytes = c->nblocks * SHK_BLOCK_BYTES;
  c->nregions = (uint32_t)((c->nslots + SHK_REGION - 1) / SHK_REGION);
  c->rbits = 0;
  while ((1u << c->rbits) < c->nregions) c->rbits++;
  const uint32_t mlb = cfg->max_level_bits ? cfg->max_level_bits : 10;
  if (mlb > 10) return SHK_ERR_ARG;
  const uint32_t nlevels = (c->rbits + mlb - 1) / mlb;
  if (nlevels > 4) return SHK_ERR_ARG;
  c->nlevels = nlevels ? nlevels : 1;   // one region: a single pass still converts the words to 32-bit records
  {
    uint32_t left = c->rbits, nb = 1;
    for (uint32_t l = 0; l < c->nlevels; l++) {
      uint32_t bits = (left + (c->nlevels - l) - 1) / (c->nlevels - l);
      left -= bits;
      c->lv[l].shift = left; c->lv[l].bits = bits; c->lv[l].nbuckets = nb; c->lv[l].hb = cfg->hb; c->lv[l].q_lo = c->q_lo;
      c->lv[l].nslots = c->nslots; c->lv[l].cb = 0; c->lv[l].out32 = 0; c->lv[l].ablate = 0; c->lv[l].ng_log2 = 0; c->lv[l].slot_cap = 0;
      c->lv[l].kb = 0; c->lv[l].hi_off = 0;
      nb <<= bits;
    }
    c->lv[c->nlevels - 1].out32 = 1;
    // first level: one cursor per (digit, window group) instead of one per digit (ShkRpLevel::ng_log2)
    if (c->lv[0].bits >= 2 && c->lv[0].bits <= 7 && !getenv("SHK_RP_NO_GROUPS")) c->lv[0].ng_log2 = 3;
  }
  c->threads = cfg->threads_per_group ? cfg->threads_per_group : 512;
  if (c->threads < 64 || c->threads > 1024 || (c->threads & (c->threads - 1))) return SHK_ERR_ARG;
  c->hash_groups = cfg->hash_groups ? cfg->hash_groups : 2048;
  // the partition plan
  const bool words8 = getenv("SHK_RP_WORDS8") && atoi(getenv("SHK_RP_WORDS8")) != 0;
  c->roll_two = c->nlevels >= 2 && c->lv[0].bits + c->lv[1].bits <= 14;   // two levels' digits fit one pass's LDS bins
  for (uint32_t l = 0; l < c->nlevels; l++) {
    const bool last = l + 1 == c->nlevels;
    // a level in the middle: 16384-key windows as at the first level (digit runs of 1 KB instead of 256 bytes: 2.85 ->
    // 2.25 ms per 832 M keys). Not the last level: its 4-byte records in slots gain nothing (3.4 ms either way)
    c->part[l].scatter = l == 0 && c->lv[0].ng_log2 ? RP_SCATTER_GROUPED : c->threads >= 512 && !last && c->lv[l].bits <= 8 ? RP_SCATTER_WIDE : RP_SCATTER_TILE;
    c->part[l].pair_hist = l == 0 && c->roll_two && c->lv[1].ng_log2 == 0;
    c->part[l].may_slot = last && l >= 1 && c->lv[l].out32;
    // (level 0 of a context with two levels or more is the roll kernels'; SHK_RP_WORDS8=1: 8-byte words between all levels)
    c->part[l].may_narrow = l >= 1 && l + 2 == c->nlevels && !words8;
    c->lv[l].cb = 32 - 16 - c->lv[c->nlevels - 1].bits;
  }
  // No counting pass above the last level either (roll_stage): three levels, the middle one may be narrow, the last one may
  // slot, and a bucket of the middle level's output gets so many keys of a full batch that six sigma of a clumpy share,
  // 6 sqrt(8 m), are at most a tenth of it (m >= 28,800): below that the slots spread a bucket over too much empty range.
  // SHK_ROLL_SLOTS=0: every batch takes the histogram pass
  c->roll_slots = c->nlevels == 3 && c->part[1].may_narrow && c->part[2].may_slot &&
                  !(getenv("SHK_ROLL_SLOTS") && atoi(getenv("SHK_ROLL_SLOTS")) == 0) &&
                  cfg->max_batch_keys / (level_out(c, 1)) >= 28800;
  // The split record between k_roll_scatter and the middle level: three levels with a narrow middle one (so SHK_RP_WORDS8=1
  // implies off), the whole filter here (a key masked to hb bits is then in range, which is what lets the middle level drop
  // its SHK_E_CORRUPT check), and the record's fields fit 40 bits. kb <= 32 (the high byte holds chunk bits only) follows
  // from the levels' even split: kb + cb <= 40 means rbits <= 25, and then kb <= 32. SHK_RP_SPLIT=0: every batch on 8-byte words
  c->split_kb = 0;
  if (c->nlevels == 3 && c->part[1].may_narrow && ns == 1 && !(getenv("SHK_RP_SPLIT") && atoi(getenv("SHK_RP_SPLIT")) == 0)) {
    const uint32_t kb = c->rbits + 16 - c->lv[0].bits;
    if (kb + c->lv[1].cb <= 40 && kb <= 32) c->split_kb = kb;
  }
  // SHK_PARSE_MASK=0: k_emit_reads reads the text again
  c->parse_mask = !(getenv("SHK_PARSE_MASK") && atoi(getenv("SHK_PARSE_MASK")) == 0);
  c->fasta_seg = SHK_FASTA_SEGMENT;
  if (const char *e = getenv("SHK_FASTA_SEGMENT")) {
    const long v = atol(e);
    if (v < 16 || v + cfg->k - 1 > 65535) return SHK_ERR_ARG;
    c->fasta_seg = (uint32_t)v;
  }
  c->rounds_left = cfg->num_denoise;
  c->max_reads = cfg->max_batch_reads ? cfg->max_batch_reads : cfg->max_batch_bytes / 16 + 1024;
  { int rc = bufs_alloc(c, c, false); if (rc) return rc; }
  for (int i = 0; i < 2; i++) {
    if (dmalloc(&c->tab[i], c->table_bytes)) return SHK_ERR_HIP;
    if (dmalloc(&c->fin[i], (uint64_t)c->nregions + 2)) return SHK_ERR_HIP;
  }
  if (dmalloc(&c->d_summary, SHK_SUM_STRIDE * (uint64_t)c->nregions + 8)) return SHK_ERR_HIP;
  if (dmalloc(&c->d_dump_offs, (uint64_t)c->nregions + 2)) return SHK_ERR_HIP;
  // the sampled location of a deNoise point needs enough regions for the sample to mean something:
  // every 8th region; every 16th from 2^20 regions on (qb >= 28): a wrong guess costs one more one-pass point (18 ms at
  // qb 29), the sample 1.9 / 1.15 / 0.75 ms at stride 8 / 16 / 32; measured on the 12 points of the qb-29 bench: no wrong
  // guess at 8 and 16, one at 32 (its chance grows with sqrt(stride) / sqrt(new keys per batch))
  c->sample_stride = c->nregions >= (1u << 20) ? 16 : 8;
  if (const char *e = getenv("SHK_SAMPLE_STRIDE")) c->sample_stride = (uint32_t)atoi(e);
  else if (c->nregions < (1u << 14)) c->sample_stride = 0;
  c->lazy_ok = 1;
  c->foreign_marks = 0;
  if (const char *e = getenv("SHK_LAZY_PLACE")) c->lazy_ok = atoi(e) != 0;
  c->prefetch_ok = !(getenv("SHK_MERGE_PREFETCH") && atoi(getenv("SHK_MERGE_PREFETCH")) == 0);
  if (dmalloc(&c->spill[0], (uint64_t)c->nregions * SHK_SPILL_STRIDE) || dmalloc(&c->d_over_list, (uint64_t)c->nregions + 1)) return SHK_ERR_HIP;
  { uint64_t nt = c->nregions / SHK_RSCAN_TILE + 2;
    if (dmalloc(&c->d_tile_a, nt) || dmalloc(&c->d_tile_b, nt) || dmalloc(&c->d_tile_f, nt)) return SHK_ERR_HIP; }
  if (dmalloc(&c->d_counters, SHK_NCOUNTERS)) return SHK_ERR_HIP;
  HIPCHK(hipMemsetAsync(c->tab[0], 0, c->table_bytes + SHK_SLACK, c->stream));
  HIPCHK(hipMemsetAsync(c->tab[1], 0, c->table_bytes + SHK_SLACK, c->stream));
  HIPCHK(hipMemsetAsync(c->fin[0], 0, ((uint64_t)c->nregions + 2) * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->fin[1], 0, ((uint64_t)c->nregions + 2) * 8, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  // A context that is going to take deNoise rounds (its own, or as a shard of a filter that does) gets the buffers of the
  // first-chunk records and of the one-pass point now: allocating gigabytes inside a counting call is a synchronous trip
  // into the driver in the middle of the build (contexts without rounds never pay for them)
  if (cfg->num_denoise > 0 || cfg->num_shards > 1) {
    if (ensure_chist(c) || point_alloc(c)) return SHK_ERR_HIP;
  }
  if (cfg->num_shards > 1) {     // the two send buffers of shk_route_words, for the same reason
    for (int b = 0; b < 2; b++)
      if (dmalloc(&c->d_send[b], c->cfg.max_batch_keys + 1)) return SHK_ERR_HIP;
  }
  return SHK_OK;
}

extern "C" int shk_create(const shk_config *cfg, shk_ctx **out) {
  if (!cfg || !out) return SHK_ERR_ARG;
  if (cfg->qb < 6 || cfg->qb > 40 || cfg->hb != cfg->qb + 8 || cfg->k < 1 || cfg->k > SHK_MAX_K) return SHK_ERR_ARG;
  uint32_t ns = cfg->num_shards ? cfg->num_shards : 1;
  if (ns & (ns - 1)) return SHK_ERR_ARG;
  if (cfg->shard_index >= ns) return SHK_ERR_ARG;
  if (cfg->hb + SHK_CHUNK_BITS > 64) return SHK_ERR_ARG;
  shk_ctx *c = new shk_ctx();
  const int rc = create_init(c, cfg);
  if (rc) { shk_destroy(c); return rc; }
  *out = c;
  return SHK_OK;
}

// (of a partly built context too: shk_create comes here from every failure)
static void front_destroy(shk_ctx *c);
static void fasta_destroy(shk_ctx *c);
static void reads_destroy(shk_ctx *c);
static void correct_destroy(shk_ctx *c);
extern "C" void shk_destroy(shk_ctx *c) {
  if (!c) return;
  hipSetDevice(c->dev);
  front_destroy(c);
  fasta_destroy(c);
  reads_destroy(c);
  correct_destroy(c);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->copy_stream) {
    hipStreamSynchronize(c->copy_stream);
    for (int b = 0; b < 2; b++) { if (c->d_up[b]) hipFree(c->d_up[b]); if (c->up_done[b]) hipEventDestroy(c->up_done[b]); }
    hipStreamDestroy(c->copy_stream);
  }
  if (getenv("SHK_STAMPS") && c->d_scalars) {
    unsigned long long st[16];
    hipMemcpy(st, c->d_scalars + DS_STAMPS, sizeof(st), hipMemcpyDeviceToHost);
    static const char *nm[9] = {"stage+init", "fold keys", "old rank/select", "count sort", "merge pass", "scan+stats", "(unused)", "placement", "stores"};
    unsigned long long tot = 0; for (int i = 0; i < 9; i++) tot += st[i];
    for (int i = 0; i < 9; i++) fprintf(stderr, "SHK_STAMPS %-16s %6.2f %%\n", nm[i], tot ? 100.0 * st[i] / tot : 0.0);
  }
  for (int i = 0; i < 2; i++) { hipFree(c->tab[i]); hipFree(c->fin[i]); hipFree(c->d_send[i]); }
  hipFree(c->d_isum); hipFree(c->d_ilens); hipFree(c->d_fin_i); hipFree(c->d_prot);
  hipFree(c->d_newchunks); hipFree(c->d_chist); hipHostFree(c->h_chist);
  hipFree(c->spill[0]); hipFree(c->spill[1]); hipFree(c->d_over_list); hipFree(c->d_summary); hipFree(c->d_dump_offs); hipFree(c->d_tile_a); hipFree(c->d_tile_b); hipFree(c->d_tile_f); hipFree(c->d_counters);
  bufs_free(c, c);
  delete c;
}

// ------------------------------------------------------------------ helpers
// exclusive scan of in[0..n) (n on the host, or *n_dev on the device with n_max as bound)
template <typename T>
static int run_scan(const shk_ctx *c, ShkStageBufs *b, const T *in, uint64_t n_max, const uint64_t *n_dev, uint64_t *out, uint64_t *sums = nullptr) {
  // sums: n_max / SHK_SCAN_TILE + 2 words of scratch; the context's own fits the batch sizes it was created for
  ProfScope ps(c, b, KP_SCAN);
  if (!sums) sums = b->d_block_sums;
  const uint32_t nb = (uint32_t)(n_max / SHK_SCAN_TILE + 1);
  hipLaunchKernelGGL((k_scan_reduce<T>), dim3(nb), dim3(c->threads), 0, b->stream, in, n_max, n_dev, sums);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(c->threads), 0, b->stream, sums, (uint64_t)nb, b->d_scalars + DS_SCAN_TOTAL);
  hipLaunchKernelGGL((k_scan_apply<T>), dim3(nb), dim3(c->threads), 0, b->stream, in, n_max, n_dev, sums,
                     b->d_scalars + DS_SCAN_TOTAL, out);
  HIPCHK(hipGetLastError());
  return 0;
}

// The error word's read-back in two halves, around the caller's synchronisation. err_take clears the device's word when
// it is set; record: the bits also become last_err_bits (what the big-image retries look at).
static int err_enqueue(ShkStageBufs *b) { HIPCHK(hipMemcpyAsync(b->h_pinned + HP_ERR, b->d_err, 4, hipMemcpyDeviceToHost, b->stream)); return 0; }
static int err_take(ShkStageBufs *b, bool record, uint32_t *bits) {
  *bits = *(uint32_t *)(b->h_pinned + HP_ERR);
  if (*bits && record) b->last_err_bits = *bits;
  if (*bits) HIPCHK(hipMemsetAsync(b->d_err, 0, 16, b->stream));
  return 0;
}
static int fetch_err(ShkStageBufs *b, uint32_t *bits) {
  if (err_enqueue(b)) return SHK_ERR_HIP;
  HIPCHK(hipStreamSynchronize(b->stream));
  return err_take(b, true, bits);
}
// the number of key words of the batch, where the partition kernels read it
static int set_nwords(ShkStageBufs *b, uint64_t n) {
  b->h_pinned[HP_NWORDS_IN] = n;
  HIPCHK(hipMemcpyAsync(b->d_scalars + DS_NWORDS, b->h_pinned + HP_NWORDS_IN, 8, hipMemcpyHostToDevice, b->stream));
  return 0;
}

// Device text that is a buffer of shk_upload_text whose copy may still be running: `stream` waits for it. For the entry
// points, on the caller's thread (the stage functions leave the context alone).
static int upload_wait(shk_ctx *c, const void *text, int on_device, hipStream_t stream) {
  for (int u = 0; on_device && u < 2; u++)
    if (c->d_up[u] && text == (const void *)c->d_up[u] && c->up_pending[u]) { HIPCHK(hipStreamWaitEvent(stream, c->up_done[u], 0)); c->up_pending[u] = 0; }
  return SHK_OK;
}

// chunk i of a call is labelled chunk_first + i * chunk_mul: do the labels of nchunks chunks fit?
static bool chunk_labels_ok(uint32_t nchunks, uint32_t chunk_first, uint32_t chunk_mul) {
  return nchunks != 0 && nchunks <= SHK_MAX_CHUNKS && chunk_first + (uint64_t)(nchunks - 1) * chunk_mul < SHK_MAX_CHUNKS;
}

// text -> extents of every read (d_rd_start, d_rd_end, d_rd_chunk); *dtext_out = where the text is on the device
// (device text: k_count_lines, k_emit_reads and k_count_keys fetch 16-byte units at multiples of 16 from the text's base)
static bool text_aligned(const void *text, int on_device) { return !on_device || ((uintptr_t)text & 15) == 0; }
static int parse_stage(const shk_ctx *c, ShkStageBufs *b, const void *text, int on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                       const uint64_t *chunk_len, uint32_t nchunks, const uint8_t **dtext_out, uint64_t *nreads_out) {
  if (!text_aligned(text, on_device)) return SHK_ERR_ARG;
  uint64_t text_end = 0;
  for (uint32_t i = 0; i < nchunks; i++) {
    if (chunk_off[i] + chunk_len[i] > text_bytes) return SHK_ERR_ARG;
    if (chunk_off[i] + chunk_len[i] > text_end) text_end = chunk_off[i] + chunk_len[i];
  }
  if (!on_device && text_bytes > c->cfg.max_batch_bytes) return SHK_ERR_BATCH;
  // The flags of every unit up to the last chunk's end, and 8 units of room for k_emit_reads' groups of 8. A text beyond the
  // capacity (device text of more than four bytes per key) gets a larger buffer, never a smaller one; when that allocation
  // fails the batch runs on the text-reading emitter
  const uint64_t mask_units = text_end / 16 + 8;
  if (c->parse_mask && mask_units > b->nlmask_units) {
    HIPCHK(hipStreamSynchronize(b->stream));
    hipFree(b->d_nlmask);
    b->d_nlmask = nullptr;
    b->nlmask_units = 0;
    (void)nlmask_alloc(b, mask_units);
  }
  uint16_t *const nlmask = c->parse_mask && mask_units <= b->nlmask_units ? b->d_nlmask : nullptr;
  const uint8_t *dtext;
  if (on_device) {
    dtext = (const uint8_t *)text;
  } else {
    HIPCHK(hipMemcpyAsync(b->d_text, text, text_bytes, hipMemcpyHostToDevice, b->stream));
    dtext = b->d_text;
  }
  HIPCHK(hipMemcpyAsync(b->d_chunk_off, chunk_off, nchunks * 8, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->d_chunk_len, chunk_len, nchunks * 8, hipMemcpyHostToDevice, b->stream));
  { ProfScope ps(c, b, KP_COUNT_LINES);
    hipLaunchKernelGGL(k_count_lines, dim3(nchunks * SHK_PARSE_SEGS), dim3(c->threads), 0, b->stream, dtext, b->d_chunk_off, b->d_chunk_len, b->d_nlines, nlmask); }
  { ProfScope ps(c, b, KP_SCAN_CHUNKS);
    hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(c->threads), 0, b->stream, b->d_nlines, nchunks, b->d_reads_base, b->d_scalars + DS_NREADS); }
  // the read arrays are sized by max_reads: the count is checked on the host below
  HIPCHK(hipMemcpyAsync(b->h_pinned + HP_NREADS, b->d_scalars + DS_NREADS, 8, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  const uint64_t nreads = b->h_pinned[HP_NREADS];
  if (nreads > c->max_reads) return SHK_ERR_BATCH;
  { ProfScope ps(c, b, KP_EMIT_READS);
    hipLaunchKernelGGL(k_emit_reads, dim3(nchunks * SHK_PARSE_SEGS), dim3(c->threads), 0, b->stream, dtext, (const uint16_t *)nlmask, b->d_chunk_off, b->d_chunk_len,
                       b->d_reads_base, b->d_nlines, b->d_rd_start, b->d_rd_end, b->d_rd_chunk); }
  *dtext_out = dtext;
  *nreads_out = nreads;
  return SHK_OK;
}

// text + chunk table -> key words in d_words[0]; d_scalars[DS_NWORDS] = #words
static int hash_stage(const shk_ctx *c, ShkStageBufs *b, const void *text, int on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                      const uint64_t *chunk_len, uint32_t nchunks, uint32_t chunk_first, uint32_t chunk_mul, bool hist0 = false) {
  // chunk i of this call is labelled chunk_first + i * chunk_mul; hist0: the hash kernel also fills the first partition
  // level's histogram (d_hist[0]), see partition_stage
  if (!chunk_labels_ok(nchunks, chunk_first, chunk_mul)) return SHK_ERR_BATCH;
  if (!text_aligned(text, on_device)) return SHK_ERR_ARG;
  if (hist0) HIPCHK(hipMemsetAsync(b->d_hist[0], 0, (1ULL << (c->lv[0].bits + c->lv[0].ng_log2)) * 8, b->stream));
  const uint8_t *dtext;
  uint64_t nreads;
  { int rc = parse_stage(c, b, text, on_device, text_bytes, chunk_off, chunk_len, nchunks, &dtext, &nreads); if (rc) return rc; }
  uint32_t groups = c->hash_groups;
  { uint64_t need = nreads / (c->threads / SHK_WAVE) + 1; if (need < groups) groups = (uint32_t)need; }
  { ProfScope ps(c, b, KP_COUNT_KEYS);       // (one thread per read)
    const uint64_t blocks = nreads / 256 + 1;
    hipLaunchKernelGGL(k_count_keys, dim3((uint32_t)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, b->stream, dtext, b->d_rd_start, b->d_rd_end,
                       b->d_scalars + DS_NREADS, c->cfg.k, b->d_nkeys, b->d_err); }
  if (run_scan<uint32_t>(c, b, b->d_nkeys, nreads, nullptr, b->d_key_base)) return SHK_ERR_HIP;
  HIPCHK(hipMemcpyAsync(b->d_scalars + DS_NWORDS, b->d_key_base + nreads, 8, hipMemcpyDeviceToDevice, b->stream));
  { ProfScope ps(c, b, KP_HASH);
    const uint32_t ht = c->threads < SHK_HASH_WAVES * SHK_WAVE ? c->threads : SHK_HASH_WAVES * SHK_WAVE;
    hipLaunchKernelGGL(k_hash_reads, dim3(groups * (c->threads / ht)), dim3(ht), 0, b->stream, dtext, b->d_rd_start, b->d_rd_end,
                       b->d_scalars + DS_NREADS, b->d_rd_chunk, chunk_first, chunk_mul, b->d_key_base, c->cfg.k, c->cfg.hb,
                       b->d_words[0], c->cfg.max_batch_keys, b->d_err, hist0 ? b->d_hist[0] : nullptr, c->lv[0].shift, c->lv[0].bits, c->q_lo, c->lv[0].ng_log2); }
  HIPCHK(hipGetLastError());
  return SHK_OK;
}

// 2-bit staging of the batch's reads for the roll kernels (k_pack_reads), in `buf` = a buffer of max_batch_keys words that
// nothing else uses until the roll kernels are done. Leaves A.pk null (text path for every read) when the buffer cannot
// hold the batch's units or SHK_NO_PACK is set (measurement; a caller that has no text path passes no_pack_switch = false).
static uint64_t pack_cap_units(const shk_ctx *c) { return c->cfg.max_batch_keys / 2 > 1 ? c->cfg.max_batch_keys / 2 - 1 : 0; }
static int pack_stage(const shk_ctx *c, ShkStageBufs *b, ShkRollArgs &A, uint64_t nreads, uint64_t text_bytes, uint64_t *buf,
                      bool no_pack_switch = true) {
  A.pk = nullptr; A.pk_base = nullptr; A.pk_flag = nullptr;
  // units <= sum over reads of (len / 64 + 1) <= text_bytes / 64 + nreads when no two chunks overlap (k_pack_reads leaves
  // the reads that do not fit on the text path); 16 bytes of slack for the roll kernels' 16-byte fetches
  const uint64_t cap_units = pack_cap_units(c);
  if ((no_pack_switch && getenv("SHK_NO_PACK")) || text_bytes / 64 + nreads + 1 > cap_units) return SHK_OK;
  ProfScope ps(c, b, KP_PACK);
  const uint32_t t = c->threads < 256 ? c->threads : 256;
  { const uint64_t blocks = nreads / t + 1;
    hipLaunchKernelGGL(k_pack_count, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(t), 0, b->stream, (const uint64_t *)b->d_rd_start,
                       (const uint64_t *)b->d_rd_end, (const uint64_t *)(b->d_scalars + DS_NREADS), c->cfg.k, b->d_nkeys); }
  if (run_scan<uint32_t>(c, b, b->d_nkeys, nreads, nullptr, b->d_key_base)) return SHK_ERR_HIP;
  { const uint64_t blocks = nreads * 4 / t + 1;
    hipLaunchKernelGGL(k_pack_reads, dim3((uint32_t)(blocks < 16384 ? blocks : 16384)), dim3(t), 0, b->stream, A.text, A.safe_end,
                       (const uint64_t *)b->d_rd_start, (const uint64_t *)b->d_rd_end, (const uint64_t *)(b->d_scalars + DS_NREADS),
                       (const uint64_t *)b->d_key_base, b->d_nkeys, (ShkQuad *)buf, cap_units); }
  A.pk = (const ShkQuad *)buf; A.pk_base = b->d_key_base; A.pk_flag = b->d_nkeys;
  return SHK_OK;
}

// What the roll kernels take from the parse and the configuration; the caller adds the digits (q_lo, dig_*, hist*), the
// cursors and the output.
static void roll_args(const shk_ctx *c, ShkStageBufs *b, ShkRollArgs &A, const uint8_t *dtext, uint64_t text_bytes,
                      uint32_t chunk_first, uint32_t chunk_mul) {
  A.text = dtext; A.safe_end = (text_bytes + 15) & ~15ULL;
  A.rd_start = b->d_rd_start; A.rd_end = b->d_rd_end; A.nreads_p = b->d_scalars + DS_NREADS; A.rd_chunk = b->d_rd_chunk;
  A.chunk_first = chunk_first; A.chunk_mul = chunk_mul; A.k = c->cfg.k; A.hb = c->cfg.hb;
  A.cap = c->cfg.max_batch_keys; A.err = b->d_err; A.kb = 0; A.sample_bits = 0;
}
// wide: A.hist_bits may exceed 10 (up to 14: two levels' digits together)
static void launch_roll_hist(const shk_ctx *c, ShkStageBufs *b, const ShkRollArgs &A, uint64_t nreads, bool wide) {
  const bool small = c->threads < 512;     // (small workgroups: the CPU emulator build of the tests)
  const uint32_t t = small ? 64 : wide ? 512 : 256, max_blocks = small ? 64 : wide ? 1024 : 4096;
  const uint64_t blocks = nreads / t + 1;
  const dim3 grid((uint32_t)(blocks < max_blocks ? blocks : max_blocks));
  if (small && wide) hipLaunchKernelGGL((k_roll_hist<14, 64>), grid, dim3(64), 0, b->stream, A);
  else if (small) hipLaunchKernelGGL((k_roll_hist<10, 64>), grid, dim3(64), 0, b->stream, A);
  else if (wide) hipLaunchKernelGGL((k_roll_hist<14, 512>), grid, dim3(512), 0, b->stream, A);
  else hipLaunchKernelGGL((k_roll_hist<10, 256>), grid, dim3(256), 0, b->stream, A);
}
static void launch_roll_scatter(const shk_ctx *c, ShkStageBufs *b, const ShkRollArgs &A, uint64_t nreads, bool split = false) {
  ProfScope ps(c, b, KP_ROLL_SCATTER);
  if (c->threads >= 512) {
    const uint64_t blocks = nreads / 1024 + 1;
    const dim3 grid((uint32_t)(blocks < 512 ? blocks : 512));
    if (split) hipLaunchKernelGGL((k_roll_scatter<1024, 1, true>), grid, dim3(1024), 0, b->stream, A);
    else hipLaunchKernelGGL((k_roll_scatter<1024, 1>), grid, dim3(1024), 0, b->stream, A);
  } else {          // (small workgroups: the CPU emulator build of the tests)
    const uint64_t blocks = nreads / 64 + 1;
    const dim3 grid((uint32_t)(blocks < 64 ? blocks : 64));
    if (split) hipLaunchKernelGGL((k_roll_scatter<64, 4, true>), grid, dim3(64), 0, b->stream, A);
    else hipLaunchKernelGGL((k_roll_scatter<64, 4>), grid, dim3(64), 0, b->stream, A);
  }
}

// text + chunk table -> key words in d_words[0], partitioned by the first region digit; d_base[1] = bucket bases,
// d_scalars[DS_NWORDS] = #words (roll_kernels.hip). For contexts with at least two partition levels; whether the histogram
// pass has counted the second level too is the plan's roll_two.
// (the roll kernels take q_lo as a multiple of 256: q_lo = nslots * shard_index with nslots a power of two, so any other
// q_lo needs nslots < 256, which is one region and one level)
static bool roll_path(const shk_ctx *c) { return c->nlevels >= 2; }

// Capacity of a slot above the last level for a mean share of m keys: the mean plus six sigma of a clumpy hash
// distribution (a true k-mer comes ~8 times per batch, as slot_capacity() has it), rounded up to a multiple of `unit`.
// Tight, not buffer-sized: whatever a slot does not use is address range the next level's streams have to cross.
static uint64_t up_slot_capacity(double m, uint64_t unit) {
  const uint64_t cp = (uint64_t)ceil(m + 6.0 * sqrt(8.0 * m + 1.0) + 16.0);
  return (cp + unit - 1) / unit * unit;
}

// The parsed batch as the roll kernels take it: what roll_keys needs to run a second time (front_end, after an overflow)
struct ShkRollBatch {
  const uint8_t *dtext; uint64_t text_bytes, nreads;
  uint32_t nchunks, chunk_first, chunk_mul;
  bool split;           // the batch may leave the roll kernels as split records (split_batch)
  bool staged;          // every read lies in 2-bit units already (shk_count_fasta): d_words[1], d_key_base and d_nkeys are as pack_stage leaves them
};

// The roll kernels over a parsed batch, from the 2-bit staging on. slots: no histogram pass; digit d owns the slot
// [d * roll_cap, (d + 1) * roll_cap) of d_words[0], d_base[1] holds the slots' bases, d_end[1] the buckets' ends and
// d_scalars[DS_EXTENT] the positions of all slots; an overflow raises SHK_E_SLOT_FULL_UP (the caller's read-back).
static int roll_keys(const shk_ctx *c, ShkStageBufs *b, const ShkRollBatch &R, bool slots) {
  const uint64_t P = 1ULL << c->lv[0].bits;
  // the first two levels' digits together, when they fit the histogram pass's LDS bins
  const uint32_t cb = c->lv[0].bits + c->lv[1].bits;
  const bool two = c->roll_two;
  b->roll_cap = 0; b->roll_split = false;
  if (slots) {
    // the host's only bound on the keys before they are hashed: a base needs a quality byte
    const uint64_t U = c->cfg.max_batch_keys < R.text_bytes / 2 ? c->cfg.max_batch_keys : R.text_bytes / 2;
    const uint64_t cap0 = up_slot_capacity((double)U / (double)P, 16);
    if (P * cap0 <= words_cap(c)) b->roll_cap = cap0;
  }
  const uint64_t cap0 = b->roll_cap;
  if (cap0) {
    ProfScope ps(c, b, KP_RP_PREP);
    hipLaunchKernelGGL(k_rp_slot_bases, dim3((uint32_t)(P / 256 + 1)), dim3(256), 0, b->stream, b->d_base[1], b->d_cursor, P, cap0, b->d_scalars + DS_EXTENT);
  } else if (two) HIPCHK(hipMemsetAsync(b->d_hist[1], 0, (1ULL << cb) * 8, b->stream));
  else HIPCHK(hipMemsetAsync(b->d_hist[0], 0, P * 8, b->stream));
  ShkRollArgs A;
  roll_args(c, b, A, R.dtext, R.text_bytes, R.chunk_first, R.chunk_mul);
  A.q_lo = c->q_lo;
  A.dig_shift = c->lv[0].shift; A.dig_bits = c->lv[0].bits;
  A.hist = two ? b->d_hist[1] : b->d_hist[0]; A.hist_shift = two ? c->lv[1].shift : c->lv[0].shift; A.hist_bits = two ? cb : c->lv[0].bits;
  A.cursor = b->d_cursor; A.out = b->d_words[0];
  if (cap0) A.cap = P * cap0;
  // Split records, unless the middle level would have to count them: its counting pass (k_rp_hist) reads 8-byte words. A
  // slotted batch has no counting pass, and one with counted bases has the middle level's counts from k_roll_hist when the
  // two levels' digits fit its bins (`two`); where they do not, the batch stays on 8-byte words
  if (R.split && (cap0 || two)) { b->roll_split = true; b->split_batches++; A.kb = c->split_kb; }
  if (R.staged) { A.pk = (const ShkQuad *)b->d_words[1]; A.pk_base = b->d_key_base; A.pk_flag = b->d_nkeys; }
  else { int rc = pack_stage(c, b, A, R.nreads, R.text_bytes, b->d_words[1]); if (rc) return rc; }     // (d_words[1]: the partition's other buffer, idle until its second level)
  if (cap0) {
    launch_roll_scatter(c, b, A, R.nreads, b->roll_split);
    ProfScope ps(c, b, KP_RP_PREP);
    hipLaunchKernelGGL(k_roll_slot_ends, dim3(1), dim3(c->threads < 256 ? c->threads : 256), 0, b->stream, (const uint64_t *)b->d_cursor, (uint32_t)P, cap0,
                       b->d_end[1], b->d_scalars + DS_NWORDS, b->d_err);
    HIPCHK(hipGetLastError());
    return SHK_OK;
  }
  { ProfScope ps(c, b, KP_ROLL_HIST);
    launch_roll_hist(c, b, A, R.nreads, two);
    if (two) hipLaunchKernelGGL(k_roll_fold, dim3((uint32_t)(P / 256 + 1)), dim3(256), 0, b->stream, (const uint64_t *)b->d_hist[1], (uint32_t)P,
                                1u << c->lv[1].bits, b->d_hist[0]); }
  // bucket bases = exclusive scan of the digit counts; its total is the number of key words
  if (run_scan<uint64_t>(c, b, b->d_hist[0], P, nullptr, b->d_base[1])) return SHK_ERR_HIP;
  HIPCHK(hipMemcpyAsync(b->d_scalars + DS_NWORDS, b->d_base[1] + P, 8, hipMemcpyDeviceToDevice, b->stream));
  HIPCHK(hipMemcpyAsync(b->d_cursor, b->d_base[1], P * 8, hipMemcpyDeviceToDevice, b->stream));
  launch_roll_scatter(c, b, A, R.nreads, b->roll_split);
  HIPCHK(hipGetLastError());
  return SHK_OK;
}

// May this batch of text leave the roll kernels as split records? The plan allows it and the batch is narrow (the rule
// partition_stage applies to the middle level).
static bool split_batch(const shk_ctx *c, uint32_t nchunks) { return c->split_kb && nchunks && nchunks <= (1u << c->lv[1].cb); }
// Does this batch run without counting passes above the last level? The plan allows it, the batch is narrow (the middle
// level's slots hold narrow records) and two overflows in a row have not switched the upper slots off.
static bool roll_slots_batch(const shk_ctx *c, const ShkStageBufs *b, uint32_t nchunks) {
  return c->roll_slots && !b->up_off && nchunks <= (1u << c->lv[1].cb);
}
static int roll_stage(const shk_ctx *c, ShkStageBufs *b, const void *text, int on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                      const uint64_t *chunk_len, uint32_t nchunks, uint32_t chunk_first, uint32_t chunk_mul, ShkRollBatch *R) {
  if (!chunk_labels_ok(nchunks, chunk_first, chunk_mul)) return SHK_ERR_BATCH;
  R->text_bytes = text_bytes; R->nchunks = nchunks; R->chunk_first = chunk_first; R->chunk_mul = chunk_mul;
  R->split = chunk_first == 0 && chunk_mul == 1 && split_batch(c, nchunks);      // (tags below nchunks)
  { int rc = parse_stage(c, b, text, on_device, text_bytes, chunk_off, chunk_len, nchunks, &R->dtext, &R->nreads); if (rc) return rc; }
  return roll_keys(c, b, *R, roll_slots_batch(c, b, nchunks));
}

// What partition_stage reads (the number of words is in d_scalars[DS_NWORDS] as well), and its three producers
struct ShkPartInput {
  const uint64_t *src[2]; uint64_t n[2]; int nsrc;   // one or two sources of words (two: the first level reads both)
  int in_buf;            // which d_words[] src[0] occupies; -1: neither
  uint32_t first_level;  // 1: src[0] is partitioned by the first digit already and d_base[1] holds the bucket bases
  bool counted[2];       // counted[l]: the producer has filled d_hist[l]
  uint32_t nchunks;      // the words' chunk fields are chunk tags below this; 0: not known (or the field is a multiplicity)
  uint64_t slot_cap0;    // first_level = 1 only, 0 = off: src[0] lies in slots of this many words per first digit, d_end[1] holds the
                         // buckets' ends (ShkStageBufs::roll_cap); the middle level is then slotted too
  uint64_t split_ext;    // first_level = 1 only, 0 = 8-byte words: src[0] holds split records, 4-byte plane over this many positions and
                         // the byte plane behind it (ShkStageBufs::roll_split); the batch is narrow then
  bool redo;             // the batch's second time through the partition, after SHK_E_SLOT_FULL_UP: the last level's cursor set-up is
                         // timed with the other preparations, so that k_rp_slot_cursors stays one launch per batch that tried slots
};
// roll_stage: d_words[0] sorted by the first digit; the second level is counted when the two levels' digits fit one pass
static ShkPartInput part_from_roll(const shk_ctx *c, const ShkStageBufs *b, uint64_t n, uint32_t nchunks) {
  return {{b->d_words[0], nullptr}, {n, 0}, 1, 0, 1, {false, c->roll_two && !b->roll_cap}, nchunks, b->roll_cap,
          b->roll_split ? (b->roll_cap ? b->roll_cap << c->lv[0].bits : c->cfg.max_batch_keys) : 0, false};
}
// hash_stage with hist0: d_words[0] in emission order, the first level counted
static ShkPartInput part_from_hash(const ShkStageBufs *b, uint64_t n, uint32_t nchunks) { return {{b->d_words[0], nullptr}, {n, 0}, 1, 0, 0, {true, false}, nchunks, 0, 0, false}; }
// the caller's words, read in place (no staging copy), in one of the context's own buffers or not. w2: a second source
// (shk_stage_words_pair: both are counted into one histogram and scattered with one set of cursors)
static ShkPartInput part_from_words(const ShkStageBufs *b, const uint64_t *w, uint64_t n, const uint64_t *w2 = nullptr, uint64_t n2 = 0) {
  return {{w, w2}, {n, n2}, w2 ? 2 : 1, w == b->d_words[0] ? 0 : w == b->d_words[1] ? 1 : -1, 0, {false, false}, 0, 0, 0, false};
}

// Last level: fixed-capacity region slots instead of a histogram pass over the keys + scan, when the output buffer
// (max_batch_keys 8-byte words = twice as many 4-byte records) gives every region room for its mean share of this
// batch plus six sigma of a clumpy hash distribution (a true k-mer comes ~8 times per batch). A region that gets
// more (repeats: one k-mer a million times) raises SHK_E_SLOT_FULL and the level is redone the exact way; after two
// such batches in a row the context stops trying. 0: no slots for this batch.
static uint32_t slot_capacity(const shk_ctx *c, uint64_t nregions, uint64_t nwords) {
  uint64_t cp = 2 * c->cfg.max_batch_keys / nregions;
  if (cp > (1u << 20)) cp = 1u << 20;
  const double mean = (double)nwords / (double)nregions;
  return cp >= 64 && (double)cp >= mean + 6.0 * sqrt(8.0 * mean + 1.0) + 16.0 ? (uint32_t)cp : 0;
}

// partition_stage's answer when a slotted level above the last one overflowed: nothing of the batch is committed, the
// caller runs its front end again from the 2-bit staging on, with counted bases (front_end). Never leaves the library.
#define SHK_RC_REDO_UP 0x5348

// the words of `in` -> sorted by region in d_words[*dst]; region offsets in d_base[nlevels] (ShkStageBufs::region_cap)
static int partition_stage(const shk_ctx *c, ShkStageBufs *b, const ShkPartInput &in, int *dst) {
  const uint64_t *n_p = b->d_scalars + DS_NWORDS;
  const uint64_t nmax = in.n[0] + in.n[1];
  { ProfScope ps(c, b, KP_RP_PREP);
    hipLaunchKernelGGL(k_rp_base1, dim3(1), dim3(64), 0, b->stream, n_p, b->d_base[0]); }
  int cur = in.in_buf < 0 ? 1 : in.in_buf;   // the buffer the level's input occupies (neither: write to d_words[0] first)
  bool counted[4] = {in.counted[0], in.counted[1], false, false};
  bool narrow = false;   // the level in hand writes narrow records
  bool up_checked = false;   // the error word has been read back behind the slotted upper levels
  // Slotted levels above the last one (in.slot_cap0: a three-level context, so the level in hand is the middle one or the
  // last). A slotted input has an extent in positions, which the window grids and the kernels' bounds take, next to its
  // number of words, which the statistics and the merge take; its buckets end where d_end[l] says.
  uint64_t ext = in.slot_cap0 ? in.slot_cap0 << c->lv[0].bits : nmax;      // positions of the input of the level in hand
  const uint64_t *ext_p = in.slot_cap0 ? b->d_scalars + DS_EXTENT : n_p, *ends = in.slot_cap0 ? b->d_end[1] : nullptr;
  b->region_cap = 0;
  for (uint32_t l = in.first_level; l < c->nlevels; l++) {
    const ShkPartLevel &pl = c->part[l];
    const uint64_t nb = c->lv[l].nbuckets, P = 1ULL << c->lv[l].bits;
    const bool last = l + 1 == c->nlevels;
    // 4-byte records between this level and the next: the plan allows it and every chunk tag of the call fits
    const bool narrow_in = narrow;
    narrow = pl.may_narrow && in.nchunks && in.nchunks <= (1u << c->lv[l].cb);
    const bool split_in = in.split_ext && l == in.first_level;     // this level reads split records
    if (split_in && !(narrow && l == 1)) return SHK_ERR_CORRUPT;   // (roll_keys splits narrow batches only)
    // the sources of this level: (words, their extent on the device, their bucket bases and ends, their extent on the host)
    struct Src { const uint64_t *w, *n_p, *base, *end; uint64_t n; } srcs[2] = {{l == in.first_level ? in.src[0] : b->d_words[cur], ext_p, b->d_base[l], ends, ext}, {}};
    int nsrc = 1;
    if (l == 0 && in.nsrc == 2) {
      srcs[0] = {in.src[0], b->d_scalars + DS_PAIR_LEN, b->d_scalars + DS_PAIR_BASE, nullptr, in.n[0]};
      srcs[1] = {in.src[1], b->d_scalars + DS_PAIR_LEN + 1, b->d_scalars + DS_PAIR_BASE + 2, nullptr, in.n[1]};
      nsrc = 2;
    }
    const uint32_t nwin = (uint32_t)(ext / SHK_RP_TILE + 1);
    // (a level that is counted already gains nothing from slots)
    uint32_t cap = pl.may_slot && !b->slots_off && !counted[l] ? slot_capacity(c, nb * P, nmax) : 0;
    // the middle level behind slotted roll kernels: slots of narrow records for the batch's mean share, as many as its
    // buffer holds (two records per word) at the most
    uint64_t cap_up = 0;
    if (in.slot_cap0 && !last) {
      cap_up = up_slot_capacity((double)nmax / (double)(nb * P), 32);
      const uint64_t room = 2 * words_cap(c) / (nb * P) / 32 * 32;
      if (cap_up > room) cap_up = room;
    }
    { ProfScope ps(c, b, KP_RP_PREP);
      hipLaunchKernelGGL(k_rp_tile_first, dim3(nwin / 256 + 1), dim3(256), 0, b->stream, b->d_base[l], (uint32_t)nb, ext_p, b->d_tfb); }
    for (;;) {
      ShkRpLevel lvl = c->lv[l];
#ifdef SHK_DIAGNOSTICS   // timing ablations give INVALID results: compiled into diagnostic builds only (make DIAG=1)
      if (const char *e = getenv("SHK_RP_ABLATE")) lvl.ablate = (uint32_t)atoi(e);
#endif
      uint64_t *cursor = b->d_cursor;
      if (cap_up) {
        ProfScope ps(c, b, KP_RP_PREP);
        cursor = b->d_end[l + 1];            // (ends up as the buckets' ends)
        lvl.slot_cap = (uint32_t)cap_up;
        hipLaunchKernelGGL(k_rp_slot_bases, dim3((uint32_t)((nb * P) / 256 + 1 < 4096 ? (nb * P) / 256 + 1 : 4096)), dim3(256), 0, b->stream, b->d_base[l + 1],
                           cursor, nb * P, cap_up, b->d_scalars + DS_EXTENT + 1);
      } else if (cap) {
        ProfScope ps(c, b, in.redo ? KP_RP_PREP : KP_RP_SLOTS);
        cursor = b->d_base[l + 1];           // (ends up as the regions' end positions)
        lvl.slot_cap = cap;
        hipLaunchKernelGGL(k_rp_slot_cursors, dim3((uint32_t)((nb * P) / 256 + 1 < 4096 ? (nb * P) / 256 + 1 : 4096)), dim3(256), 0, b->stream, cursor, nb * P, cap);
      } else {
        // histogram, unless the producer or the level in front has counted this level
        if (!counted[l] && pl.pair_hist) {
          HIPCHK(hipMemsetAsync(b->d_hist[0], 0, (P << c->lv[0].ng_log2) * 8, b->stream));
          HIPCHK(hipMemsetAsync(b->d_hist[1], 0, (P << c->lv[1].bits) * 8, b->stream));
          ProfScope ps(c, b, KP_RP_HIST);
          const uint32_t wt = nwin / 1024 + 1;   // windows per workgroup (few workgroups: each flushes up to 2^14 counters)
          for (int si = 0; si < nsrc; si++)
            hipLaunchKernelGGL((k_rp_hist2<14>), dim3(nwin / wt + 1), dim3(c->threads < 512 ? c->threads : 512), 0, b->stream, srcs[si].w, srcs[si].n_p,
                               c->lv[0], c->lv[1], b->d_hist[0], b->d_hist[1], wt);
          counted[1] = true;
        } else if (!counted[l]) {
          if (split_in) return SHK_ERR_CORRUPT;     // (k_rp_hist reads 8-byte words: roll_keys keeps such a batch on them)
          HIPCHK(hipMemsetAsync(b->d_hist[l], 0, ((nb * P) << c->lv[l].ng_log2) * 8, b->stream));
          ProfScope ps(c, b, KP_RP_HIST);
          const uint32_t wt = nwin / 4096 + 1;   // windows per workgroup
          for (int si = 0; si < nsrc; si++)
            if (narrow_in)
              hipLaunchKernelGGL(k_rp_hist<true>, dim3(nwin / wt + 1), dim3(c->threads), 0, b->stream, srcs[si].w, srcs[si].n_p, srcs[si].base, srcs[si].end,
                                 b->d_tfb, c->lv[l], b->d_hist[l], wt);
            else
              hipLaunchKernelGGL(k_rp_hist<false>, dim3(nwin / wt + 1), dim3(c->threads), 0, b->stream, srcs[si].w, srcs[si].n_p, srcs[si].base, srcs[si].end,
                                 b->d_tfb, c->lv[l], b->d_hist[l], wt);
        }
        // bases
        if (c->lv[l].ng_log2) {
          // (first level only: nb = 1) sub-buckets in (digit, group) order; the next level's buckets are the digits
          const uint32_t ng = c->lv[l].ng_log2;
          if (run_scan<uint64_t>(c, b, b->d_hist[l], P << ng, nullptr, b->d_base_sub)) return SHK_ERR_HIP;
          HIPCHK(hipMemcpyAsync(b->d_cursor, b->d_base_sub, (P << ng) * 8, hipMemcpyDeviceToDevice, b->stream));
          ProfScope ps(c, b, KP_RP_PREP);
          hipLaunchKernelGGL(k_rp_group_bases, dim3((uint32_t)(P / 256 + 1)), dim3(256), 0, b->stream, b->d_base_sub, (uint32_t)P, ng, b->d_base[l + 1]);
        } else {
          if (run_scan<uint64_t>(c, b, b->d_hist[l], nb * P, nullptr, b->d_base[l + 1])) return SHK_ERR_HIP;
          HIPCHK(hipMemcpyAsync(b->d_cursor, b->d_base[l + 1], nb * P * 8, hipMemcpyDeviceToDevice, b->stream));
        }
      }
      // scatter
      { ProfScope ps(c, b, narrow || narrow_in ? KP_RP_SCATTER_NARROW : KP_RP_SCATTER);
        for (int si = 0; si < nsrc; si++) {
          const Src &S = srcs[si];
          const dim3 wide((uint32_t)(S.n >> SHK_RP_TILE0_LOG2) + 1);
          if (split_in) {
            lvl.kb = c->split_kb; lvl.hi_off = 4 * in.split_ext;
            if (pl.scatter == RP_SCATTER_WIDE)
              hipLaunchKernelGGL((k_rp_scatter<SHK_RP_TILE0_LOG2, 1024, 256, RP_SPLIT_IN>), wide, dim3(1024), 0, b->stream, S.w, b->d_words[cur ^ 1], S.n_p,
                                 S.base, S.end, b->d_tfb, lvl, cursor, b->d_err);
            else
              hipLaunchKernelGGL((k_rp_scatter<12, SHK_RP_THREADS, SHK_RP_MAXP, RP_SPLIT_IN>), dim3((uint32_t)(S.n / SHK_RP_TILE + 1)), dim3(SHK_RP_THREADS), 0,
                                 b->stream, S.w, b->d_words[cur ^ 1], S.n_p, S.base, S.end, b->d_tfb, lvl, cursor, b->d_err);
          } else if (narrow && pl.scatter == RP_SCATTER_WIDE)
            hipLaunchKernelGGL((k_rp_scatter<SHK_RP_TILE0_LOG2, 1024, 256, RP_NARROW_OUT>), wide, dim3(1024), 0, b->stream, S.w, b->d_words[cur ^ 1], S.n_p,
                               S.base, S.end, b->d_tfb, lvl, cursor, b->d_err);
          else if (narrow)
            hipLaunchKernelGGL((k_rp_scatter<12, SHK_RP_THREADS, SHK_RP_MAXP, RP_NARROW_OUT>), dim3((uint32_t)(S.n / SHK_RP_TILE + 1)), dim3(SHK_RP_THREADS), 0,
                               b->stream, S.w, b->d_words[cur ^ 1], S.n_p, S.base, S.end, b->d_tfb, lvl, cursor, b->d_err);
          else if (narrow_in)
            hipLaunchKernelGGL((k_rp_scatter<12, SHK_RP_THREADS, SHK_RP_MAXP, RP_NARROW_IN>), dim3((uint32_t)(S.n / SHK_RP_TILE + 1)), dim3(SHK_RP_THREADS), 0,
                               b->stream, S.w, b->d_words[cur ^ 1], S.n_p, S.base, S.end, b->d_tfb, lvl, cursor, b->d_err);
          else if (pl.scatter == RP_SCATTER_GROUPED)      // (window groups are defined on the first level's 16384-key windows: SHK_RP_TILE0_LOG2)
            hipLaunchKernelGGL((k_rp_scatter<SHK_RP_TILE0_LOG2, 1024>), wide, dim3(1024), 0, b->stream, S.w, b->d_words[cur ^ 1], S.n_p, S.base, S.end,
                               b->d_tfb, lvl, cursor, b->d_err);
          else if (pl.scatter == RP_SCATTER_WIDE)
            hipLaunchKernelGGL((k_rp_scatter<SHK_RP_TILE0_LOG2, 1024, 256>), wide, dim3(1024), 0, b->stream, S.w, b->d_words[cur ^ 1], S.n_p, S.base, S.end,
                               b->d_tfb, lvl, cursor, b->d_err);
          else
            hipLaunchKernelGGL((k_rp_scatter<12, SHK_RP_THREADS>), dim3((uint32_t)(S.n / SHK_RP_TILE + 1)), dim3(SHK_RP_THREADS), 0, b->stream, S.w,
                               b->d_words[cur ^ 1], S.n_p, S.base, S.end, b->d_tfb, lvl, cursor, b->d_err);
        } }
      // No read-back behind a level without slots, nor behind the slotted middle level (the last level's shows its bit) --
      // unless the last level behind slotted upper ones has no slots of its own this time: then theirs is fetched here
      if (!cap && !(in.slot_cap0 && last && !up_checked)) break;
      uint32_t bits = 0;
      if (fetch_err(b, &bits)) return SHK_ERR_HIP;
      if (bits & SHK_E_SLOT_FULL_UP) return SHK_RC_REDO_UP;
      if (bits & ~SHK_E_SLOT_FULL) return map_err_bits(bits & ~SHK_E_SLOT_FULL);
      if (in.slot_cap0 && !up_checked) { b->up_overflows = 0; up_checked = true; }
      if (!cap) break;
      // slots: did every region fit?
      if (!bits) { b->region_cap = cap; b->slot_overflows = 0; break; }
      if (++b->slot_overflows >= 2) b->slots_off = 1;
      cap = 0;                               // a region overflowed its slot: the same level again with exact bases
    }
    if (cap_up) { ext = (nb * P) * cap_up; ext_p = b->d_scalars + DS_EXTENT + 1; ends = b->d_end[l + 1]; }
    else { ext = nmax; ext_p = n_p; ends = nullptr; }
    cur ^= 1;
  }
  HIPCHK(hipGetLastError());
  *dst = cur;
  return SHK_OK;
}

// One launch per slice of at most 2^24 regions (a HIP grid holds fewer than 2^32 threads; a qb-33 filter has 2^25
// regions): ARGS must name a ShkMergeArgs variable `A`, whose r0 the loop sets.
#define SHK_REGION_SLICE (1u << 24)
#define SHK_FOR_REGION_SLICES(c, A, nblk) \
  for (uint32_t r0_ = 0, nblk = 0; r0_ < (c)->nregions && ((A).r0 = r0_, nblk = (c)->nregions - r0_ < SHK_REGION_SLICE ? (c)->nregions - r0_ : SHK_REGION_SLICE, true); r0_ += SHK_REGION_SLICE)

// rec: the old side comes from the records (no image: the small instantiation serves both image sizes)
template <int MODE>
static void launch_merge(shk_ctx *c, const ShkMergeArgs &A0, bool rec = false) {
  ShkMergeArgs A = A0;
  SHK_FOR_REGION_SLICES(c, A, nblk) {
    // (the write pass, MODE 1, has no record-sourced form: naming MODE 0 in its place keeps launch_merge<1> from
    // instantiating one that the test in front never lets run)
    if (MODE != 1 && rec) {
      c->prefetch_passes += A.prefetch;
      if (A.prefetch) hipLaunchKernelGGL((k_region_merge<MODE == 1 ? 0 : MODE, SHK_IMG_BLOCKS, false, true, true>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else hipLaunchKernelGGL((k_region_merge<MODE == 1 ? 0 : MODE, SHK_IMG_BLOCKS, false, true>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
    } else if (c->big_image)
      hipLaunchKernelGGL((k_region_merge<MODE, SHK_IMG_BLOCKS_BIG>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
    else
      hipLaunchKernelGGL((k_region_merge<MODE, SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
  }
}

struct MergeOut {
  uint64_t newd, added, removed;
  uint32_t err;
};

// where a pass writes its records: never over the ones that describe the live table
static uint8_t *spill_out(const shk_ctx *c) { return c->spill[c->rec_live ? c->live ^ 1 : c->live]; }

// the second record buffer; without it the context places at every commit for the rest of its life (not an error)
static bool lazy_reserve(shk_ctx *c) {
  if (!c->lazy_ok || c->spill[1]) return c->lazy_ok != 0;
  void *v = nullptr;
  if (hipMalloc(&v, (uint64_t)c->nregions * SHK_SPILL_STRIDE + SHK_SLACK) != hipSuccess) {
    (void)hipGetLastError();
    c->lazy_ok = 0;
    return false;
  }
  c->spill[1] = (uint8_t *)v;
  return true;
}

static void fill_args(shk_ctx *c, ShkMergeArgs *A, const uint64_t *words, uint32_t lo, uint32_t hi, int denoise);
// The live table's bytes, if a lazy commit left them unwritten: placement from the records and free pointers that
// describe it. At the top of everything that reads c->tab[c->cur].
static int table_sync(shk_ctx *c) {
  if (!c->table_stale) return SHK_OK;
  ShkMergeArgs A;
  fill_args(c, &A, nullptr, 0, 0, 0);
  A.tabB = c->tab[c->cur]; A.finB = c->fin[c->cur]; A.spill = c->spill[c->live]; A.summary = nullptr;
  HIPCHK(hipMemsetAsync(c->tab[c->cur], 0, c->table_bytes, c->stream));
  { ProfScope ps(c, KP_PLACE);
    SHK_FOR_REGION_SLICES(c, A, nblk)
      hipLaunchKernelGGL((k_region_place<SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A); }
  HIPCHK(hipGetLastError());
  // The table counts as written only once the placement has run without raising an error bit: a reader behind a failed
  // placement must fail again, not read half a table. (One wait per read of a stale table, not per batch.)
  uint32_t bits = 0;
  if (fetch_err(c, &bits)) return SHK_ERR_HIP;
  if (bits) return map_err_bits(bits);
  c->table_stale = 0;
  return SHK_OK;
}

static void fill_args(shk_ctx *c, ShkMergeArgs *A, const uint64_t *words, uint32_t lo, uint32_t hi, int denoise) {
  A->want_hist = 0;
  A->tabA = c->tab[c->cur]; A->tabB = c->tab[c->cur ^ 1];
  A->finA = c->fin[c->cur]; A->finB = c->fin[c->cur ^ 1];
  A->words = reinterpret_cast<const uint32_t *>(words); A->region_base = c->d_base[c->nlevels]; A->region_cap = c->region_cap;
  A->nslots = c->nslots; A->xnslots = c->xnslots; A->nblocks = c->nblocks; A->q_lo = c->q_lo; A->hb = c->cfg.hb;
  A->chunk_lo = lo; A->chunk_hi = hi; A->denoise = denoise;
  A->ablate = 0;
#ifdef SHK_DIAGNOSTICS   // timing ablations give INVALID results: compiled into diagnostic builds only (make DIAG=1)
  { const char *ab = getenv("SHK_ABLATE"); A->ablate = ab ? (uint32_t)atoi(ab) : 0; }
#endif
  { const char *sp = getenv("SHK_STAMPS");    // diagnostics: "fused" = only the one-pass deNoise launches, "plain" = all the others, else all
    A->dbg = (sp && strcmp(sp, "fused") != 0) ? (unsigned long long *)(c->d_scalars + DS_STAMPS) : nullptr; }
  A->spill = spill_out(c); A->orec = c->spill[c->live]; A->over_list = c->d_over_list; A->n_over = c->d_counters + SHK_CNT_NOVER; A->list = nullptr;
  A->newchunks = nullptr; A->chist = nullptr;
  A->counted = c->counted;
  // the early loads: the records are live (a record-sourced launch) and the batch brings eight words per region or more --
  // regions are hash buckets, so fewer than 0.04 % of them are empty then (e^-8)
  A->prefetch = c->prefetch_ok && c->rec_live && words && c->pass_words >= 8ULL * c->nregions;
  A->r0 = 0; A->rstride = 1;
  A->split = ~0u; A->isum = nullptr; A->ilens = nullptr; A->prot_list = nullptr; A->nprot = 0;
  A->summary = c->d_summary; A->counters = c->d_counters; A->err = c->d_err;
}

// first request for the exact first-chunk histogram (contexts that never reach a deNoise point never pay for it)
static int ensure_chist(shk_ctx *c) {
  if (c->d_newchunks) return SHK_OK;
  if (dmalloc(&c->d_newchunks, (uint64_t)c->nregions * SHK_NC_CAP) || dmalloc(&c->d_chist, (uint64_t)SHK_MAX_CHUNKS)) return SHK_ERR_HIP;
  HIPCHK(hipHostMalloc((void **)&c->h_chist, SHK_MAX_CHUNKS * sizeof(uint64_t), hipHostMallocDefault));
  return SHK_OK;
}

// summary launch + free-pointer scan, then read the statistics back (one synchronisation).
// with_chist: the pass also records the first chunk of every new key; c->h_chist[lo..hi] afterwards.
// spill: the summary keeps the runs for k_region_place (a write pass for the same request only places them)
static int merge_summary(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t hi, int denoise, MergeOut *o,
                         bool with_chist, bool spill) {
  // (a deNoise round reads the protection marks k_denoise_marks has just left in the table's traveled words -- and only
  // those: marks_launch has synced the table and zeroed whatever a reader or an import had set before)
  const bool rec = c->rec_live && !denoise;
  if (!rec) { int rc = table_sync(c); if (rc) return rc; }
  ShkMergeArgs A;
  fill_args(c, &A, words, lo, hi, denoise);
  HIPCHK(hipMemsetAsync(c->d_counters, 0, (SHK_CNT_NOVER + 1) * 8, c->stream));
  c->spill_valid = 0;
  if (with_chist) {   // (zeroed in front of the pass: regions whose record overflows add to the histogram themselves)
    int rc = ensure_chist(c);
    if (rc) return rc;
    A.want_hist = 1; A.newchunks = c->d_newchunks; A.chist = c->d_chist;
    HIPCHK(hipMemsetAsync(c->d_chist, 0, SHK_MAX_CHUNKS * 8, c->stream));
  }
  if (spill) { ProfScope ps(c, KP_MERGE_SPILL);
    launch_merge<3>(c, A, rec); }
  else { ProfScope ps(c, KP_MERGE_SUM);
    launch_merge<0>(c, A, rec); }
  { ProfScope ps(c, KP_REGION_SCAN);
    const uint32_t ntiles = (c->nregions + SHK_RSCAN_TILE - 1) / SHK_RSCAN_TILE;
    hipLaunchKernelGGL(k_region_scan_a, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_summary, c->nregions, c->d_tile_a, c->d_tile_b);
    hipLaunchKernelGGL(k_region_scan_b, dim3(1), dim3(c->threads), 0, c->stream, c->d_tile_a, c->d_tile_b, ntiles, c->d_tile_f);
    hipLaunchKernelGGL(k_region_scan_c, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_summary, c->nregions, c->d_tile_f,
                       c->xnslots, (uint32_t)(c->big_image ? SHK_IMG_BLOCKS_BIG * 64 : SHK_IMG_SLOTS), c->fin[c->cur ^ 1], c->d_counters, c->d_err); }
  if (with_chist) {
    ProfScope ps(c, KP_MISC);
    hipLaunchKernelGGL(k_chunk_hist, dim3((c->nregions + SHK_CHIST_REGIONS - 1) / SHK_CHIST_REGIONS), dim3(256), 0, c->stream,
                       c->d_newchunks, c->d_summary, c->nregions, c->d_chist);
    HIPCHK(hipMemcpyAsync(c->h_chist, c->d_chist, ((uint64_t)hi + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipGetLastError());
  const uint64_t *cnt = c->h_pinned + HP_COUNTERS;
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_COUNTERS, c->d_counters, (SHK_CNT_NOVER + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  if (err_enqueue(c)) return SHK_ERR_HIP;
  HIPCHK(hipStreamSynchronize(c->stream));
  o->newd = cnt[CNT_NEWD]; o->added = cnt[CNT_ADDED]; o->removed = cnt[CNT_REMOVED];
  if (err_take(c, true, &o->err)) return SHK_ERR_HIP;
  c->chist_n = with_chist ? hi + 1 : 0;
  if (spill && !o->err) {
    c->spill_valid = 1; c->spill_words = words; c->spill_lo = lo; c->spill_hi = hi; c->spill_denoise = denoise;
    c->spill_big = c->big_image; c->spill_nover = cnt[SHK_CNT_NOVER];
  }
  return SHK_OK;
}

// write launch for the summary that was just computed; then flip the live table
// (the commit point: lazily when the pass left a complete set of records -- nothing on the over list, small image, no
// counted insert -- by making those records and its scan's free pointers the truth; otherwise the table is written now)
static int merge_write(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t hi, int denoise) {
  const bool match = c->spill_valid && c->spill_words == words && c->spill_lo == lo && c->spill_hi == hi && c->spill_denoise == denoise &&
                     c->spill_big == c->big_image;
  if (match && c->spill_nover == 0 && !c->big_image && !c->counted && lazy_reserve(c)) {
    if (c->rec_live) c->live ^= 1;
    c->rec_live = 1; c->table_stale = 1;
    c->spill_valid = 0;
    c->cur ^= 1;
    c->foreign_marks = 0;       // (the placement zeroes the table first)
    return SHK_OK;
  }
  if (!match || c->spill_nover) { int rc = table_sync(c); if (rc) return rc; }   // (the write pass reads table A)
  ShkMergeArgs A;
  fill_args(c, &A, words, lo, hi, denoise);
  HIPCHK(hipMemsetAsync(c->tab[c->cur ^ 1], 0, c->table_bytes, c->stream));
  if (match) {
    // the summary launch left lengths and encodings behind: placement only
    { ProfScope ps(c, KP_PLACE);
      SHK_FOR_REGION_SLICES(c, A, nblk) {
        if (c->big_image) hipLaunchKernelGGL((k_region_place<SHK_IMG_BLOCKS_BIG>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A);
        else hipLaunchKernelGGL((k_region_place<SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A);
      }
      A.r0 = 0; }
    if (c->spill_nover) {
      A.list = c->d_over_list;
      ProfScope ps(c, KP_MERGE_WRITE);
      if (c->big_image)
        hipLaunchKernelGGL((k_region_merge<1, SHK_IMG_BLOCKS_BIG>), dim3((uint32_t)c->spill_nover), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else
        hipLaunchKernelGGL((k_region_merge<1, SHK_IMG_BLOCKS>), dim3((uint32_t)c->spill_nover), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
    }
  } else {
    ProfScope ps(c, KP_MERGE_WRITE);
    launch_merge<1>(c, A);
  }
  c->spill_valid = 0;
  HIPCHK(hipGetLastError());
  c->rec_live = 0; c->table_stale = 0;
  c->cur ^= 1;
  c->foreign_marks = 0;         // (table B was zeroed and its traveled words are never written)
  return SHK_OK;
}

// The protection marks of a deNoise round on the live table (k_denoise_marks): the only traveled bits a writer ever reads.
// Marks belong to readers and influence no writer (include/shk.h), so whatever a marking lookup, a marking Contiger call
// or an import may have left in tab[cur] is zeroed first. A build that never marks launches nothing here but the walk.
static int marks_launch(shk_ctx *c) {
  const uint64_t ml = c->cfg.min_denoise_len ? c->cfg.min_denoise_len : (1ULL << 20);
  { int rc = table_sync(c); if (rc) return rc; }
  ProfScope ps(c, KP_MARKS);
  if (c->foreign_marks) {
    hipLaunchKernelGGL(k_clear_traveled, dim3((uint32_t)((c->nblocks + 255) / 256)), dim3(256), 0, c->stream, c->tab[c->cur], c->nblocks);
    c->foreign_marks = 0;
  }
  hipLaunchKernelGGL(k_denoise_marks, dim3(1), dim3(64), 0, c->stream, c->tab[c->cur], c->nslots, c->xnslots, c->nblocks,
                     ml, (unsigned long long *)(c->d_scalars + DS_MARKS));
  return SHK_OK;
}

static int denoise_round_once(shk_ctx *c, uint64_t *removed) {
  { int rc = marks_launch(c); if (rc) return rc; }
  MergeOut o;
  int rc = merge_summary(c, nullptr, 0, 0, 1, &o, false, true);
  if (rc) return rc;
  if (o.err) return map_err_bits(o.err);
  rc = merge_write(c, nullptr, 0, 0, 1);
  if (rc) return rc;
  c->nelts -= o.removed;        // CQF_mt.h:1037-1038
  c->ndistinct -= o.removed;
  *removed = o.removed;
  return SHK_OK;
}

// deNoise round fused with the insertion of the chunks behind the deNoise point (one pass over the
// table instead of two). Not taken (*done = false) when the pass reports anything unusual or the
// trigger would be reached again inside [lo, hi]: the caller then runs the plain round.
static int denoise_with_rest(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t hi, shk_batch_stats *st, bool *done) {
  *done = false;
  { int rc = marks_launch(c); if (rc) return rc; }
  MergeOut o;
  int rc = merge_summary(c, words, lo, hi, 1, &o, false, true);
  if (rc) return rc;
  if (o.err) return SHK_OK;
  if (c->rounds_left > 0 && c->ndistinct - o.removed + o.newd >= c->cfg.ndistinct_for_denoise) return SHK_OK;
  rc = merge_write(c, words, lo, hi, 1);
  if (rc) return rc;
  c->nelts = c->nelts - o.removed + o.added;        // CQF_mt.h:1037-1038, then the inserts
  c->ndistinct = c->ndistinct - o.removed + o.newd;
  st->removed += o.removed; st->denoise_rounds++;
  st->kmers += o.added; st->new_distinct += o.newd; st->chunks += hi - lo + 1;
  c->big_image = 0;
  *done = true;
  return SHK_OK;
}

// ONE pass for a deNoise point inside a batch (the three-pass form: rebuild the chunks up to the point, mark, fused round +
// rest). The hash keeps two counts per key -- occurrences in the chunks <= cstar and behind it -- so a lane knows every
// key's count at the moment the round runs (cb) and what arrives afterwards (ca): the entry survives with cb when cb >= 2,
// is dropped when cb == 1, and ca is added on top. What the round's range walk needs of the table in between (which never
// exists in memory) leaves the same pass as 8 bytes + 256 length bytes per region; k_denoise_marks_virtual walks those.
// The few singletons the walk protects (one-slot clusters on a range end) are put back by rebuilding their regions with
// the list. Anything unusual (long runs, a cluster beyond the LDS image, a second crossing inside the rest) -> the caller
// takes the three-pass path.
// Three steps, shared by the single-table flow (denoise_fused) and the sharded one (shk_stage_point_*):
//   point_try    the FUSED pass over all regions + both free-pointer scans (+ the exact first-chunk histogram)
//   point_walk   the range walk over the intermediate layout -> protected singletons of this table / shard
//   point_finish their regions once more with the list; final statistics; the spill records are then ready for placement
#define SHK_PROT_CAP 65536u
struct PointOut {
  uint64_t newd_after, added_after, removed, added_before;   // statistics (CQF_mt.h:1037-1038 bookkeeping)
  uint32_t err;                                              // kernel flags: anything set = not this way
  uint64_t islots, ifin;      // intermediate table: slots in use, free pointer behind the last region (local, carry 0)
  int first_used;             // intermediate table: quotient 0 has a run
};

static int point_alloc(shk_ctx *c) {
  if (c->d_isum) return SHK_OK;
  if (dmalloc(&c->d_isum, 2 * (uint64_t)c->nregions + 2) || dmalloc(&c->d_ilens, (uint64_t)c->nregions * SHK_REGION) ||
      dmalloc(&c->d_fin_i, (uint64_t)c->nregions + 2) || dmalloc(&c->d_prot, (uint64_t)SHK_PROT_CAP)) return SHK_ERR_HIP;
  return SHK_OK;
}

static void point_scans(shk_ctx *c, bool final_table, bool inter_table, long long carry) {
  const uint32_t ntiles = (c->nregions + SHK_RSCAN_TILE - 1) / SHK_RSCAN_TILE;
  const uint32_t img_slots = (uint32_t)SHK_IMG_SLOTS;
  ProfScope ps(c, KP_REGION_SCAN);
  if (final_table) {
    hipLaunchKernelGGL(k_region_scan_a, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_summary, c->nregions, c->d_tile_a, c->d_tile_b, (uint32_t)SHK_SUM_STRIDE);
    hipLaunchKernelGGL(k_region_scan_b, dim3(1), dim3(c->threads), 0, c->stream, c->d_tile_a, c->d_tile_b, ntiles, c->d_tile_f, 0LL);
    hipLaunchKernelGGL(k_region_scan_c, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_summary, c->nregions, c->d_tile_f,
                       c->xnslots, img_slots, c->fin[c->cur ^ 1], c->d_counters, c->d_err, (uint32_t)SHK_SUM_STRIDE);
  }
  if (inter_table) {
    // the table in between: free pointers at the region starts (its capacity flags count like the final table's)
    hipLaunchKernelGGL(k_region_scan_a, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_isum, c->nregions, c->d_tile_a, c->d_tile_b, 2u);
    hipLaunchKernelGGL(k_region_scan_b, dim3(1), dim3(c->threads), 0, c->stream, c->d_tile_a, c->d_tile_b, ntiles, c->d_tile_f, carry);
    hipLaunchKernelGGL(k_region_scan_c, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_isum, c->nregions, c->d_tile_f,
                       c->xnslots, img_slots, c->d_fin_i, c->d_counters, c->d_err, 2u);
  }
}

static int point_read(shk_ctx *c, PointOut *po) {
  HIPCHK(hipGetLastError());
  const uint64_t *cnt = c->h_pinned + HP_COUNTERS;
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_COUNTERS, c->d_counters, SHK_NCOUNTERS * 8, hipMemcpyDeviceToHost, c->stream));
  if (err_enqueue(c)) return SHK_ERR_HIP;
  HIPCHK(hipStreamSynchronize(c->stream));
  po->newd_after = cnt[CNT_NEWD]; po->added_after = cnt[CNT_ADDED]; po->removed = cnt[CNT_REMOVED]; po->added_before = cnt[CNT_ADDED_BEFORE];
  return err_take(c, false, &po->err);
}

// with_chist: the pass also records the first chunk of every key the table has not seen; c->h_chist[lo..hi] afterwards
static int point_try(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t split, uint32_t hi, bool with_chist, PointOut *po) {
  int rc = point_alloc(c);
  if (rc) return rc;
  if (with_chist) { rc = ensure_chist(c); if (rc) return rc; }
  ShkMergeArgs A;
  fill_args(c, &A, words, lo, hi, 1);
  A.split = split; A.isum = c->d_isum; A.ilens = c->d_ilens;
  if (with_chist) {
    A.want_hist = 1; A.newchunks = c->d_newchunks; A.chist = c->d_chist;
    HIPCHK(hipMemsetAsync(c->d_chist, 0, SHK_MAX_CHUNKS * 8, c->stream));
  }
  { const char *sp = getenv("SHK_STAMPS");
    A.dbg = (sp && strcmp(sp, "plain") != 0) ? (unsigned long long *)(c->d_scalars + DS_STAMPS) : nullptr; }
  c->spill_valid = 0;
  c->chist_n = 0;
  HIPCHK(hipMemsetAsync(c->d_counters, 0, SHK_NCOUNTERS * 8, c->stream));
  { ProfScope ps(c, KP_MERGE_FUSED);
    SHK_FOR_REGION_SLICES(c, A, nblk) {
      if (c->rec_live) c->prefetch_passes += A.prefetch;
      if (c->rec_live && A.prefetch) hipLaunchKernelGGL((k_region_merge<3, SHK_IMG_BLOCKS, true, true, true>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else if (c->rec_live) hipLaunchKernelGGL((k_region_merge<3, SHK_IMG_BLOCKS, true, true>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else hipLaunchKernelGGL((k_region_merge<3, SHK_IMG_BLOCKS, true>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
    } }
  point_scans(c, true, true, 0);
  if (with_chist) {
    ProfScope ps(c, KP_MISC);
    hipLaunchKernelGGL(k_chunk_hist, dim3((c->nregions + SHK_CHIST_REGIONS - 1) / SHK_CHIST_REGIONS), dim3(256), 0, c->stream,
                       c->d_newchunks, c->d_summary, c->nregions, c->d_chist, 1u);
    HIPCHK(hipMemcpyAsync(c->h_chist, c->d_chist, ((uint64_t)hi + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_IFIN, c->d_fin_i + c->nregions, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_IFIRST, c->d_ilens, 1, hipMemcpyDeviceToHost, c->stream));
  rc = point_read(c, po);
  if (rc) return rc;
  po->islots = c->h_pinned[HP_COUNTERS + SHK_CNT_ISLOTS];
  po->ifin = c->h_pinned[HP_IFIN];
  po->first_used = (c->h_pinned[HP_IFIRST] & 0xff) != 0;
  if (with_chist && !po->err) c->chist_n = hi + 1;
  return SHK_OK;
}

// the range walk of the round over the intermediate layout (k_denoise_marks_virtual). carry: what the shards in front of
// this one spill over the border (slots, >= 0); W/state: see ShkWalkShard. *nprot singletons, their quotients in c->d_prot.
static int point_walk(shk_ctx *c, long long carry, const ShkWalkShard &W, const uint64_t state_in[2], uint64_t state_out[2],
                      uint64_t *nprot, uint32_t *err) {
  const uint64_t ml = c->cfg.min_denoise_len ? c->cfg.min_denoise_len : (1ULL << 20);
  if (carry > 0) point_scans(c, false, true, carry);      // the layout as it is in the single table
  c->h_pinned[HP_WALK_IN] = state_in[0]; c->h_pinned[HP_WALK_IN + 1] = state_in[1];
  HIPCHK(hipMemcpyAsync(c->d_scalars + DS_WALK_IN, c->h_pinned + HP_WALK_IN, 16, hipMemcpyHostToDevice, c->stream));
  { ProfScope ps(c, KP_MARKS);
    hipLaunchKernelGGL(k_denoise_marks_virtual, dim3(1), dim3(64), 0, c->stream, (const uint64_t *)c->d_fin_i, (const uint8_t *)c->d_ilens,
                       (const uint32_t *)c->d_isum, c->nslots, c->xnslots, ml, c->d_prot, SHK_PROT_CAP, (unsigned long long *)(c->d_scalars + DS_MARKS),
                       W, (const uint64_t *)(c->d_scalars + DS_WALK_IN), c->d_scalars + DS_WALK_OUT); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_MARKS, c->d_scalars + DS_MARKS, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_WALK_OUT, c->d_scalars + DS_WALK_OUT, 16, hipMemcpyDeviceToHost, c->stream));
  if (err_enqueue(c)) return SHK_ERR_HIP;
  HIPCHK(hipStreamSynchronize(c->stream));
  *nprot = c->h_pinned[HP_MARKS];
  state_out[0] = c->h_pinned[HP_WALK_OUT]; state_out[1] = c->h_pinned[HP_WALK_OUT + 1];
  return err_take(c, false, err);
}

// the regions that hold a protected singleton, once more with the list; statistics of the whole pass again
static int point_finish(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t split, uint32_t hi, uint64_t nprot, PointOut *po) {
  if (nprot > SHK_PROT_CAP) { po->err |= SHK_E_FUSED; return SHK_OK; }
  if (nprot) {
    std::vector<uint64_t> prot(nprot);
    HIPCHK(hipMemcpyAsync(prot.data(), c->d_prot, nprot * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> regs;
    for (uint64_t q : prot) { const uint32_t r = (uint32_t)(q >> SHK_REGION_LOG2); if (regs.empty() || regs.back() != r) regs.push_back(r); }
    ShkMergeArgs A;
    fill_args(c, &A, words, lo, hi, 1);
    A.split = split; A.isum = c->d_isum; A.ilens = c->d_ilens;
    HIPCHK(hipMemsetAsync(c->d_counters, 0, SHK_NCOUNTERS * 8, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_over_list, regs.data(), regs.size() * 4, hipMemcpyHostToDevice, c->stream));
    A.list = c->d_over_list; A.prot_list = c->d_prot; A.nprot = (uint32_t)nprot;
    { ProfScope ps(c, KP_MISC);   // (the same old side as the first go: its records are untouched)
      if (c->rec_live) c->prefetch_passes += A.prefetch;
      if (c->rec_live && A.prefetch) hipLaunchKernelGGL((k_region_merge<3, SHK_IMG_BLOCKS, true, true, true>), dim3((uint32_t)regs.size()), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else if (c->rec_live) hipLaunchKernelGGL((k_region_merge<3, SHK_IMG_BLOCKS, true, true>), dim3((uint32_t)regs.size()), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else hipLaunchKernelGGL((k_region_merge<3, SHK_IMG_BLOCKS, true>), dim3((uint32_t)regs.size()), dim3(SHK_MERGE_GROUP), 0, c->stream, A); }
    HIPCHK(hipStreamSynchronize(c->stream));   // (regs lives on this stack frame)
    point_scans(c, true, false, 0);
    int rc = point_read(c, po);
    if (rc) return rc;
  }
  if (!po->err) {
    c->spill_valid = 1; c->spill_words = words; c->spill_lo = lo; c->spill_hi = hi; c->spill_denoise = 1; c->spill_big = c->big_image;
    c->spill_nover = 0;
  }
  return SHK_OK;
}

// verify: cstar is a GUESS (sample_locate). The pass then also records the first chunk of every key the table has not seen,
// like the plain pass does; if the exact histogram puts the point at cstar the pass stands, otherwise nothing is committed
// and *exact_ch / *crossing (1: the trigger is reached at chunk *exact_ch, 0: not reached in [lo, hi]) say what is true.
static int denoise_fused(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t cstar, uint32_t hi, uint64_t newd_before,
                         shk_batch_stats *st, bool *done, bool verify = false, uint32_t *exact_ch = nullptr, int *crossing = nullptr) {
  *done = false;
  if (crossing) *crossing = -1;
  if (c->big_image || getenv("SHK_NO_FUSED_POINT")) return SHK_OK;
  PointOut po;
  int rc = point_try(c, words, lo, cstar, hi, verify, &po);
  if (rc) return rc;
  if (po.err) {                                  // not this way: nothing was committed
    if (getenv("SHK_DEBUG_FUSED")) fprintf(stderr, "SHK_DEBUG_FUSED fallback: flags 0x%x\n", po.err);
    return SHK_OK;
  }
  if (verify) {
    // where the running distinct count really reaches the trigger (the loop of merge_stage_from)
    uint64_t run = c->ndistinct;
    uint32_t ch = lo;
    for (; ch < hi; ch++) {
      run += c->h_chist[ch];
      if (run >= c->cfg.ndistinct_for_denoise) break;
    }
    if (ch == hi) run += c->h_chist[ch];
    const bool crosses = run >= c->cfg.ndistinct_for_denoise;
    if (exact_ch) *exact_ch = ch;
    if (crossing) *crossing = crosses ? 1 : 0;
    if (getenv("SHK_DEBUG_FUSED")) fprintf(stderr, "SHK_DEBUG_FUSED guess %u exact %u crossing %d\n", cstar, ch, (int)crosses);
    if (!crosses || ch != cstar) return SHK_OK;
    newd_before = run - c->ndistinct;
  }
  ShkWalkShard W;
  W.prev_fp = -1; W.cap_local = c->nslots; W.last = 1; W.next_first_used = 0;
  const uint64_t s_in[2] = {0, 0};
  uint64_t s_out[2], nprot = 0;
  uint32_t werr = 0;
  rc = point_walk(c, 0, W, s_in, s_out, &nprot, &werr);
  if (rc) return rc;
  if (werr) return SHK_OK;
  rc = point_finish(c, words, lo, cstar, hi, nprot, &po);
  if (rc) return rc;
  if (po.err) {
    c->spill_valid = 0;
    if (getenv("SHK_DEBUG_FUSED")) fprintf(stderr, "SHK_DEBUG_FUSED fallback: flags 0x%x (second go)\n", po.err);
    return SHK_OK;
  }
  // would the trigger be reached again inside the rest? then the rounds have to be taken one by one
  if (c->rounds_left > 1 && c->ndistinct + newd_before - po.removed + po.newd_after >= c->cfg.ndistinct_for_denoise) { c->spill_valid = 0; return SHK_OK; }
  rc = merge_write(c, words, lo, hi, 1);
  if (rc) return rc;
  c->nelts = c->nelts + po.added_before - po.removed + po.added_after;      // inserts, CQF_mt.h:1037-1038, inserts
  c->ndistinct = c->ndistinct + newd_before - po.removed + po.newd_after;
  c->rounds_left--; c->rounds_done++;
  st->removed += po.removed; st->denoise_rounds++;
  st->kmers += po.added_before + po.added_after; st->new_distinct += newd_before + po.newd_after; st->chunks += hi - lo + 1;
  *done = true;
  if (getenv("SHK_DEBUG_FUSED")) fprintf(stderr, "SHK_DEBUG_FUSED one-pass point at chunk %u of [%u, %u]: removed %llu protected %llu\n", cstar, lo, hi,
                                         (unsigned long long)po.removed, (unsigned long long)nprot);
  return SHK_OK;
}

static int denoise_round(shk_ctx *c, uint64_t *removed) {
  int rc = denoise_round_once(c, removed);
  if (rc == SHK_ERR_REGION && !c->big_image && (c->last_err_bits & (SHK_E_OLD_EXTENT | SHK_E_NEW_EXTENT))) {
    c->big_image = 1;
    c->last_err_bits = 0;
    rc = denoise_round_once(c, removed);
  }
  if (!rc) c->big_image = 0;   // the round thinned the table out: back to the small image
  return rc;
}

// Where will the deNoise point of this batch fall? A statistics pass over every sample_stride-th region with the exact
// first-chunk record, scaled up: regions are hash buckets, so the sample's per-chunk counts of new keys are the whole
// table's divided by the stride, up to Poisson noise (variance of the scaled sum = stride x sum). The answer is only a
// guess -- the one-pass point that is run with it checks it against the full histogram it produces itself.
// sample_pass: c->h_chist[lo..hi] = the sample's histogram; *ns regions of c->nregions were looked at
static int sample_pass(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t hi, uint32_t *ns_out, uint32_t *err_out) {
  int rc = ensure_chist(c);
  if (rc) return rc;
  const uint32_t stride = c->sample_stride > 1 ? c->sample_stride : 1;
  const uint32_t ns = (c->nregions + stride - 1) / stride;
  ShkMergeArgs A;
  fill_args(c, &A, words, lo, hi, 0);
  A.want_hist = 1; A.newchunks = c->d_newchunks; A.chist = c->d_chist; A.rstride = stride;
  c->spill_valid = 0;
  c->chist_n = 0;
  HIPCHK(hipMemsetAsync(c->d_chist, 0, SHK_MAX_CHUNKS * 8, c->stream));
  { ProfScope ps(c, KP_MERGE_SAMPLE);
    for (uint32_t r0 = 0; r0 < ns; r0 += SHK_REGION_SLICE) {
      A.r0 = r0;
      const uint32_t nblk = ns - r0 < SHK_REGION_SLICE ? ns - r0 : SHK_REGION_SLICE;
      if (c->rec_live) c->prefetch_passes += A.prefetch;
      if (c->rec_live && A.prefetch) hipLaunchKernelGGL((k_region_merge<0, SHK_IMG_BLOCKS, false, true, true>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else if (c->rec_live) hipLaunchKernelGGL((k_region_merge<0, SHK_IMG_BLOCKS, false, true>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
      else hipLaunchKernelGGL((k_region_merge<0, SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_MERGE_GROUP), 0, c->stream, A);
    }
    hipLaunchKernelGGL(k_chunk_hist, dim3((ns + SHK_CHIST_REGIONS - 1) / SHK_CHIST_REGIONS), dim3(256), 0, c->stream,
                       c->d_newchunks, c->d_summary, c->nregions, c->d_chist, stride); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_chist, c->d_chist, ((uint64_t)hi + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  if (err_enqueue(c)) return SHK_ERR_HIP;
  HIPCHK(hipStreamSynchronize(c->stream));
  *ns_out = ns;
  return err_take(c, false, err_out);   // (cleared: whatever it is, the full pass will meet it again and deal with it)
}

// verdict 0: no point expected in [lo, hi]; 1: expected at chunk *guess; 2: cannot tell
static int sample_locate(shk_ctx *c, const uint64_t *words, uint32_t lo, uint32_t hi, int *verdict, uint32_t *guess) {
  *verdict = 2;
  if (c->ndistinct >= c->cfg.ndistinct_for_denoise) return SHK_OK;
  uint32_t ns = 0, err = 0;
  int rc = sample_pass(c, words, lo, hi, &ns, &err);
  if (rc) return rc;
  if (err) return SHK_OK;
  const double F = (double)c->nregions / (double)ns;
  const double need = (double)(c->cfg.ndistinct_for_denoise - c->ndistinct);
  double cum = 0;
  uint32_t at = hi + 1;
  for (uint32_t ch = lo; ch <= hi; ch++) {
    cum += F * (double)c->h_chist[ch];
    if (at > hi && cum >= need) at = ch;
  }
  const double margin = 6.0 * sqrt(F * cum + 1.0);
  if (cum + margin < need) *verdict = 0;
  else if (cum - margin >= need && at <= hi) { *verdict = 1; *guess = at; }
  if (getenv("SHK_DEBUG_FUSED")) fprintf(stderr, "SHK_DEBUG_FUSED sample: need %.0f predicted %.0f +- %.0f -> verdict %d at %u of [%u, %u]\n", need, cum, margin / 6.0, *verdict, at, lo, hi);
  return SHK_OK;
}

// Insert the words of chunks [0, nchunks) (already partitioned in `words`), firing deNoise
// rounds where the t = 1 reference would: after the first chunk at which
// ndistinct >= trigger while rounds are left (CQF_mt.h:837, 860-869).
static int merge_stage_from(shk_ctx *c, const uint64_t *words, uint32_t nchunks, uint64_t nwords, shk_batch_stats *st,
                            uint32_t *lo_io) {
  // A summary over chunks that will turn out to lie behind a deNoise point is speculative:
  // "table full"/"extent" raised by its free-pointer scan mean nothing then.
  const uint32_t soft = SHK_E_TABLE_FULL | SHK_E_NEW_EXTENT;
  uint32_t &lo = *lo_io;
  while (lo < nchunks) {
    uint32_t hi = nchunks - 1;
    const bool watch = c->rounds_left > 0;
    MergeOut o;
    int rc;
    // When the trigger is within reach of this batch the summary launch also records the first chunk of every new key,
    // so that a pass which turns out to contain the deNoise point already yields its exact position.
    // (with a known rate of new keys per k-mer, "within reach" means within twice the predicted gain; a
    // point that is missed this way only costs one more statistics pass)
    const double reach = c->new_frac > 0 ? 2.0 * c->new_frac * (double)nwords * (double)(hi - lo + 1) / (double)nchunks : (double)nwords;
    const bool possible = watch && (double)c->ndistinct + reach >= (double)c->cfg.ndistinct_for_denoise;
    int sv = 2;
    if (possible && c->sample_stride > 1 && !c->big_image && !c->counted) {
      // guess the chunk of the deNoise point from a sample of the regions and run the one-pass point with it; the pass
      // verifies the guess against the exact histogram it collects itself and, when it was wrong, is run once more
      uint32_t guess = 0;
      rc = sample_locate(c, words, lo, hi, &sv, &guess);
      if (rc) return rc;
      if (sv == 1 && guess + 1 < nchunks) {
        bool fused = false;
        uint32_t ech = 0;
        int crossing = -1;
        rc = denoise_fused(c, words, lo, guess, nchunks - 1, 0, st, &fused, true, &ech, &crossing);
        if (rc) return rc;
        if (fused) { lo = nchunks; continue; }
        if (crossing == 1 && ech != guess && ech + 1 < nchunks) {
          uint64_t run = 0;
          for (uint32_t ch = lo; ch <= ech; ch++) run += c->h_chist[ch];
          rc = denoise_fused(c, words, lo, ech, nchunks - 1, run, st, &fused);
          if (rc) return rc;
          if (fused) { lo = nchunks; continue; }
        }
        // (anything else: the general path below)
      }
    }
    const bool with_chist = possible && sv != 0;   // (sv == 0: the sample rules a point out)
    bool have_chist = false;
    for (;;) {
      rc = merge_summary(c, words, lo, hi, 0, &o, with_chist, true);
      if (rc) return rc;
      if (with_chist && !(o.err & ~soft)) have_chist = true;
      if (o.err & ~(soft | SHK_E_HASH_FULL)) return map_err_bits(o.err & ~(soft | SHK_E_HASH_FULL));
      if (o.err & SHK_E_HASH_FULL) {
        // more distinct new keys in one region than its LDS hash holds: take fewer chunks at once
        if (hi == lo) return SHK_ERR_REGION;
        hi = lo + (hi - lo) / 2;
        continue;
      }
      break;
    }
    bool fire = false;
    if (watch && c->ndistinct + o.newd >= c->cfg.ndistinct_for_denoise) {
      // locate the first chunk at which the running distinct count reaches the trigger:
      // only now is the per-chunk histogram of first occurrences needed
      if (!have_chist) {
        rc = merge_summary(c, words, lo, hi, 0, &o, true, false);
        if (rc) return rc;
        if (o.err & ~soft) return map_err_bits(o.err & ~soft);
      }
      uint64_t run = c->ndistinct;
      uint32_t ch = lo;
      for (; ch < hi; ch++) {
        run += c->h_chist[ch];
        if (run >= c->cfg.ndistinct_for_denoise) break;
      }
      if (ch == hi) run += c->h_chist[ch];      // (the loop leaves the last chunk's keys out)
      if (ch + 1 < nchunks) {
        // the point lies inside the batch: everything -- the chunks up to it, the round, the chunks behind it -- in one pass
        bool fused = false;
        rc = denoise_fused(c, words, lo, ch, nchunks - 1, run - c->ndistinct, st, &fused);
        if (rc) return rc;
        if (fused) { lo = nchunks; continue; }
      }
      hi = ch;
      fire = true;
      // rebuild for exactly the chunks [lo, hi]
      rc = merge_summary(c, words, lo, hi, 0, &o, false, true);
      if (rc) return rc;
      if (o.err) return map_err_bits(o.err);
      rc = merge_write(c, words, lo, hi, 0);
      if (rc) return rc;
    } else {
      if (o.err) return map_err_bits(o.err);
      rc = merge_write(c, words, lo, hi, 0);
      if (rc) return rc;
    }
    if (o.added && !fire) c->new_frac = (double)o.newd / (double)o.added;
    c->ndistinct += o.newd;
    c->nelts += o.added;
    st->kmers += o.added;
    st->new_distinct += o.newd;
    st->chunks += hi - lo + 1;
    if (fire) {
      uint64_t removed = 0;
      c->rounds_left--;
      c->rounds_done++;
      if (hi + 1 < nchunks) {
        bool done = false;
        rc = denoise_with_rest(c, words, hi + 1, nchunks - 1, st, &done);
        if (rc) return rc;
        if (done) { lo = nchunks; continue; }
      }
      rc = denoise_round(c, &removed);
      if (rc) return rc;
      st->removed += removed;
      st->denoise_rounds++;
    }
    lo = hi + 1;
  }
  return SHK_OK;
}

// A cluster longer than the small LDS image makes a pass fail with an extent flag before anything is
// committed: the remaining chunks are then rebuilt with the big image (until the next deNoise round
// thins the table out again).
static int merge_stage(shk_ctx *c, const uint64_t *words, uint32_t nchunks, uint64_t nwords, shk_batch_stats *st) {
  uint32_t lo = 0;
  c->pass_words = nwords;
  int rc = merge_stage_from(c, words, nchunks, nwords, st, &lo);
  if (rc == SHK_ERR_REGION && !c->big_image && (c->last_err_bits & (SHK_E_OLD_EXTENT | SHK_E_NEW_EXTENT))) {
    c->big_image = 1;
    c->last_err_bits = 0;
    rc = merge_stage_from(c, words, nchunks, nwords, st, &lo);
  }
  return rc;
}

static int finish(shk_ctx *c, int rc) {
  uint32_t bits = 0;
  int rc2 = fetch_err(c, &bits);
  prof_collect(c);
  if (rc) return rc;
  if (rc2) return rc2;
  return map_err_bits(bits);
}

// The front end of one batch: text + chunk table -> key words partitioned by region in b->d_words[*dst], *nwords of them;
// the regions' offsets are in b->d_base[nlevels] and lie as *region_cap says (ShkStageBufs::region_cap). Errors the
// partition's kernels raise are left in b->d_err for the caller's next fetch_err.
static int front_end(const shk_ctx *c, ShkStageBufs *b, const void *text, int on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                     const uint64_t *chunk_len, uint32_t nchunks, uint64_t *nwords, int *dst, uint32_t *region_cap) {
  const bool roll = roll_path(c);
  ShkRollBatch R = {};
  bool part_redo = false;
  // (one-level contexts: the hash kernel, which counts the level's digits as it goes)
  int rc = roll ? roll_stage(c, b, text, on_device, text_bytes, chunk_off, chunk_len, nchunks, 0, 1, &R)
                : hash_stage(c, b, text, on_device, text_bytes, chunk_off, chunk_len, nchunks, 0, 1, true);
  for (;;) {
    if (rc) return rc;
    uint32_t bits = 0;
    HIPCHK(hipMemcpyAsync(b->h_pinned + HP_NWORDS, b->d_scalars + DS_NWORDS, 8, hipMemcpyDeviceToHost, b->stream));
    if (fetch_err(b, &bits)) return SHK_ERR_HIP;
    if (!(bits & SHK_E_SLOT_FULL_UP)) {
      if (bits) return map_err_bits(bits);
      *nwords = b->h_pinned[HP_NWORDS];
      if (*nwords > c->cfg.max_batch_keys) return SHK_ERR_BATCH;
      ShkPartInput in = roll ? part_from_roll(c, b, *nwords, nchunks) : part_from_hash(b, *nwords, nchunks);
      in.redo = part_redo;
      rc = partition_stage(c, b, in, dst);
      if (rc != SHK_RC_REDO_UP) break;
      part_redo = true;
    }
    // A slotted level above the last one overflowed (the roll kernels' level: seen in the read-back above; the middle one:
    // in the read-back behind the last level). Nothing is committed, the parse results are intact, the pack buffer is
    // not (the middle level wrote over it): the batch again from the 2-bit staging on, with counted bases. Two such
    // batches in a row switch the upper slots off for this front end.
    if (++b->up_overflows >= 2) b->up_off = 1;
    rc = roll_keys(c, b, R, false);
  }
  *region_cap = b->region_cap;
  return rc;
}

extern "C" int shk_count_chunks(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes,
                                const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                                shk_batch_stats *stats) {
  if (!c || !text || !chunk_off || !chunk_len) return SHK_ERR_ARG;
  shk_batch_stats st;
  memset(&st, 0, sizeof(st));
  HIPCHK(hipSetDevice(c->dev));
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  uint64_t nwords = 0;
  int dst = 0;
  uint32_t cap = 0;
  // (the error word behind the partition is finish()'s, after the rebuild: no synchronisation in between)
  int rc = front_end(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, &nwords, &dst, &cap);
  if (rc) return finish(c, rc);
  rc = merge_stage(c, c->d_words[dst], nchunks, nwords, &st);
  if (stats) *stats = st;
  return finish(c, rc);
}

// ------------------------------------------------------------------ overlapped front end
// shk_count_chunks = front end (parse, hash, partition: bound by HBM and instruction issue in turn) + rebuild (bound by
// the CUs' LDS pipelines and instruction issue), one after the other on one stream. The two halves of DIFFERENT batches
// have nothing to do with each other until the rebuild reads the partitioned words, so the front end of batch s+1 can
// run on a second stream while batch s is rebuilt: shk_prepare_chunks starts it and returns, shk_count_prepared takes
// the oldest prepared batch through the rebuild. Two batches may be prepared ahead. The overlapped front end has a
// ShkStageBufs of its own (a non-blocking stream, scalars, error word, scan scratch, partition buffers, kernel times) and
// reads the context for geometry and configuration only; two slots of (partitioned words, region bases) alternate
// between "being prepared" and "being rebuilt". It runs the same front_end as the serial path (host synchronisations
// included) in a helper thread, so the caller's thread is free to drive the rebuild.
struct ShkFrontSlot {
  uint64_t *words = nullptr;    // the buffer the last partition level writes into (and the roll kernels, two levels earlier)
  uint64_t *base = nullptr;     // region bases of that batch (region ENDS when cap != 0)
  uint32_t cap = 0;             // ShkStageBufs::region_cap of that batch
  std::thread th;
  bool busy = false;
  int rc = 0;
  uint64_t nwords = 0;
  uint32_t nchunks = 0;
};
struct ShkFront {
  ShkStageBufs b;               // (lent: d_words[] are a slot's words and scratch, d_base[nlevels] the slot's base)
  ShkFrontSlot slot[2];
  int head = 0, count = 0;      // oldest prepared slot, prepared slots
  int par = 0;                  // index of d_words[] the last level writes into
  uint64_t *scratch = nullptr;  // the other d_words[] of every batch
};

static int front_init(shk_ctx *c) {
  ShkFront *F = new ShkFront();
  c->front = F;
  { int rc = bufs_alloc(c, &F->b, true); if (rc) return rc; }
  // the roll kernels write d_words[0]; every further level flips: the last one lands in d_words[(nlevels - 1) & 1]
  F->par = roll_path(c) ? (int)((c->nlevels - 1) & 1) : (int)(c->nlevels & 1);
  const uint64_t capk = c->cfg.max_batch_keys;
  if (dmalloc(&F->scratch, words_cap(c) + 1)) return SHK_ERR_HIP;
  for (int k2 = 0; k2 < 2; k2++)
    if (dmalloc(&F->slot[k2].words, words_cap(c) + 1) || dmalloc(&F->slot[k2].base, level_out(c, c->nlevels - 1) + 2)) return SHK_ERR_HIP;
  return SHK_OK;
}
static void front_destroy(shk_ctx *c) {
  ShkFront *F = c->front;
  if (!F) return;
  for (int k2 = 0; k2 < 2; k2++) if (F->slot[k2].th.joinable()) F->slot[k2].th.join();
  bufs_free(c, &F->b);
  hipFree(F->scratch);
  for (int k2 = 0; k2 < 2; k2++) { hipFree(F->slot[k2].words); hipFree(F->slot[k2].base); }
  delete F;
  c->front = nullptr;
}

// the front end of one batch in the front's own buffers; runs in the helper thread
static void front_run(const shk_ctx *c, ShkFrontSlot *S, const void *text, int on_device, uint64_t text_bytes, std::vector<uint64_t> off,
                      std::vector<uint64_t> len) {
  ShkFront *F = c->front;
  ShkStageBufs *b = &F->b;
  hipSetDevice(c->dev);
  b->d_words[F->par] = S->words; b->d_words[F->par ^ 1] = F->scratch;
  b->d_base[c->nlevels] = S->base;
  S->nwords = 0; S->nchunks = (uint32_t)off.size();
  int dst = 0;
  int rc = front_end(c, b, text, on_device, text_bytes, off.data(), len.data(), S->nchunks, &S->nwords, &dst, &S->cap);
  if (!rc) {
    uint32_t bits = 0;
    if (fetch_err(b, &bits)) rc = SHK_ERR_HIP;            // (synchronises the front's stream: the batch is ready)
    else if (bits) rc = map_err_bits(bits);
    else if (dst != F->par) rc = SHK_ERR_CORRUPT;         // (the slot's buffer must be the one the last level wrote)
  }
  if (rc) hipStreamSynchronize(b->stream);
  S->rc = rc;
}

extern "C" int shk_prepare_chunks(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                                  const uint64_t *chunk_len, uint32_t nchunks) {
  if (!c || !text || !chunk_off || !chunk_len || !text_aligned(text, text_on_device)) return SHK_ERR_ARG;
  if (!chunk_labels_ok(nchunks, 0, 1)) return SHK_ERR_BATCH;   // (as shk_count_chunks answers it)
  if (c->cfg.num_shards > 1) return SHK_ERR_ARG;          // (a shard's words go through the exchange: shk_hash_chunks)
  HIPCHK(hipSetDevice(c->dev));
  if (!c->front) { int rc = front_init(c); if (rc) { front_destroy(c); return rc; } }
  ShkFront *F = c->front;
  if (F->count == 2) return SHK_ERR_BATCH;                // two batches are prepared already: count one first
  ShkFrontSlot *S = &F->slot[(F->head + F->count) & 1];
  // one front end at a time: the previous one (the other slot's) must have left the front's buffers
  ShkFrontSlot *O = &F->slot[(F->head + F->count + 1) & 1];
  if (O->th.joinable()) O->th.join();
  if (upload_wait(c, text, text_on_device, F->b.stream)) return SHK_ERR_HIP;
  std::vector<uint64_t> off(chunk_off, chunk_off + nchunks), len(chunk_len, chunk_len + nchunks);
  S->busy = true;
  F->count++;
#if defined(__HIPCC__)
  S->th = std::thread(front_run, c, S, text, text_on_device, text_bytes, std::move(off), std::move(len));
#else     // (the CPU emulator build of the tests keeps its kernels on the calling thread)
  front_run(c, S, text, text_on_device, text_bytes, std::move(off), std::move(len));
#endif
  return SHK_OK;
}

extern "C" int shk_prepare_reserve(shk_ctx *c) {
  if (!c || c->cfg.num_shards > 1) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  if (!c->front) { int rc = front_init(c); if (rc) { front_destroy(c); return rc; } }
  lazy_reserve(c);               // (the second record buffer, otherwise allocated by the first lazy commit)
  if (c->cfg.num_denoise) {      // (the records of a deNoise point, otherwise allocated by the first pass that needs them)
    int rc = ensure_chist(c);
    if (!rc) rc = point_alloc(c);
    if (rc) return rc;
  }
  return SHK_OK;
}

extern "C" int shk_count_prepared(shk_ctx *c, shk_batch_stats *stats) {
  if (!c || !c->front || c->front->count == 0) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  ShkFront *F = c->front;
  ShkFrontSlot *S = &F->slot[F->head];
  if (S->th.joinable()) S->th.join();
  F->head ^= 1; F->count--;
  S->busy = false;
  ShkStageBufs *f = &F->b;
  shk_batch_stats st;
  memset(&st, 0, sizeof(st));
  if (stats) *stats = st;
  // the front end's kernel times join the context's (its events were recorded on the front's stream)
  { // (the other slot's front end may be running: it only appends to f->pending from its own thread, so collect
    // what THIS batch left only when nobody else is inside the front's buffers)
    ShkFrontSlot *O = &F->slot[F->head];
    if (!(O->busy && O->th.joinable())) {
      prof_collect(f);
      for (int i = 0; i < KP_N; i++) { c->prof_ms[i] += f->prof_ms[i]; c->prof_n[i] += f->prof_n[i]; f->prof_ms[i] = 0; f->prof_n[i] = 0; }
    } }
  if (S->rc) return S->rc;
  uint64_t *saved = c->d_base[c->nlevels];
  const uint32_t saved_cap = c->region_cap;
  c->d_base[c->nlevels] = S->base; c->region_cap = S->cap;
  int rc = merge_stage(c, S->words, S->nchunks, S->nwords, &st);
  c->d_base[c->nlevels] = saved; c->region_cap = saved_cap;
  if (stats) *stats = st;
  return finish(c, rc);
}

// Start copying host text for a later call into one of two context-owned device buffers (they alternate). The copy
// runs on its own stream, next to whatever the context is computing; the call that is handed the returned pointer
// (text_on_device = 1) waits for it. A buffer is reused by the second-next upload, i.e. after the call that read it.
extern "C" int shk_upload_text(shk_ctx *c, const void *host_text, uint64_t nbytes, void **d_text) {
  if (!c || !host_text || !d_text || nbytes > c->cfg.max_batch_bytes) return c && host_text && d_text ? SHK_ERR_BATCH : SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  if (!c->copy_stream) {
    HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) HIPCHK(hipEventCreateWithFlags(&c->up_done[b], hipEventDisableTiming));
  }
  const int b = c->up_next;
  if (!c->d_up[b] && dmalloc(&c->d_up[b], c->cfg.max_batch_bytes + 64)) return SHK_ERR_HIP;
  HIPCHK(hipMemcpyAsync(c->d_up[b], host_text, nbytes, hipMemcpyHostToDevice, c->copy_stream));
  HIPCHK(hipEventRecord(c->up_done[b], c->copy_stream));
  c->up_pending[b] = 1;
  c->up_next ^= 1;
  *d_text = c->d_up[b];
  return SHK_OK;
}

// page-locked host memory for shk_upload_text sources (callers that do not link the HIP runtime themselves)
extern "C" int shk_host_alloc(uint64_t nbytes, void **p) {
  if (!p) return SHK_ERR_ARG;
  HIPCHK(hipHostMalloc(p, nbytes, hipHostMallocDefault));
  return SHK_OK;
}
extern "C" void shk_host_free(void *p) { if (p) hipHostFree(p); }

extern "C" int shk_hash_chunks(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes,
                               const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                               uint64_t **d_words, uint64_t *nwords) {
  if (!c || !text || !d_words || !nwords) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  int rc = hash_stage(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, c->cfg.shard_index, c->cfg.num_shards ? c->cfg.num_shards : 1);
  if (rc) return finish(c, rc);
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_NWORDS, c->d_scalars + DS_NWORDS, 8, hipMemcpyDeviceToHost, c->stream));
  rc = finish(c, 0);
  *d_words = c->d_words[0];
  *nwords = c->h_pinned[HP_NWORDS];
  return rc;
}

// external words -> partitioned by region in d_words[*dst]
static int partition_words(shk_ctx *c, const uint64_t *d_words, uint64_t nwords, int *dst) {
  if (set_nwords(c, nwords)) return SHK_ERR_HIP;
  return partition_stage(c, c, part_from_words(c, d_words, nwords), dst);
}

extern "C" int shk_count_words(shk_ctx *c, const uint64_t *d_words, uint64_t nwords, uint32_t nchunks,
                               shk_batch_stats *stats) {
  if (!c || (!d_words && nwords) || nchunks == 0 || nchunks > SHK_MAX_CHUNKS) return SHK_ERR_ARG;
  if (nwords > c->cfg.max_batch_keys) return SHK_ERR_BATCH;
  shk_batch_stats st;
  memset(&st, 0, sizeof(st));
  HIPCHK(hipSetDevice(c->dev));
  int dst = 0;
  int rc = partition_words(c, d_words, nwords, &dst);
  if (rc) return finish(c, rc);
  rc = merge_stage(c, c->d_words[dst], nchunks, nwords, &st);
  if (stats) *stats = st;
  return finish(c, rc);
}

// ------------------------------------------------------------------ sampling front end (roll_kernels.hip: k_roll_sample)
static void launch_roll_sample(const shk_ctx *c, ShkStageBufs *b, const ShkRollArgs &A, uint64_t nreads) {
  ProfScope ps(c, b, KP_ROLL_SAMPLE);
  if (c->threads >= 512) {
    const uint64_t blocks = nreads / 256 + 1;
    hipLaunchKernelGGL((k_roll_sample<256, 4>), dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, b->stream, A);
  } else {          // (small workgroups: the CPU emulator build of the tests)
    const uint64_t blocks = nreads / 64 + 1;
    hipLaunchKernelGGL((k_roll_sample<64, 4>), dim3((uint32_t)(blocks < 64 ? blocks : 64)), dim3(64), 0, b->stream, A);
  }
}

// The kept k-mers' key words go through the path of a caller's words (partition_words, merge_stage), so every geometry
// works, the one-level contexts that have no roll path included.
extern "C" int shk_sample_chunks(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes,
                                 const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks,
                                 uint32_t sample_bits, shk_batch_stats *stats, shk_sample_stats *sstats) {
  if (!c || !text) return SHK_ERR_ARG;
  if (sample_bits > 24 || c->cfg.hb + sample_bits > 56 || c->cfg.num_shards > 1 || !text_aligned(text, text_on_device)) return SHK_ERR_ARG;
  if (c->front && c->front->count) return SHK_ERR_BATCH;     // (their words are partitioned against the table as it is now)
  if (!chunk_labels_ok(nchunks, 0, 1)) return SHK_ERR_BATCH;
  if (!chunk_off || !chunk_len) return SHK_ERR_ARG;
  shk_batch_stats st;
  memset(&st, 0, sizeof(st));
  HIPCHK(hipSetDevice(c->dev));
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  const uint8_t *dtext;
  uint64_t nreads;
  int rc = parse_stage(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, &dtext, &nreads);
  if (rc) return finish(c, rc);
  ShkRollArgs A;
  roll_args(c, c, A, dtext, text_bytes, 0, 1);
  A.q_lo = c->q_lo; A.dig_shift = 0; A.dig_bits = 0; A.hist = nullptr; A.hist_shift = 0; A.hist_bits = 0;
  A.cursor = c->d_scalars + DS_SAMPLE; A.out = c->d_words[0]; A.sample_bits = sample_bits;
  HIPCHK(hipMemsetAsync(c->d_scalars + DS_SAMPLE, 0, 16, c->stream));
  // (the 2-bit units lie in d_words[1] and are read for the last time before the partition starts)
  rc = pack_stage(c, c, A, nreads, text_bytes, c->d_words[1]);
  if (rc) return finish(c, rc);
  launch_roll_sample(c, c, A, nreads);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_SAMPLE, c->d_scalars + DS_SAMPLE, 16, hipMemcpyDeviceToHost, c->stream));
  uint32_t bits = 0;
  if (fetch_err(c, &bits)) { prof_collect(c); return SHK_ERR_HIP; }
  const uint64_t kept = c->h_pinned[HP_SAMPLE], kmers = c->h_pinned[HP_SAMPLE + 1];
  if (bits) { prof_collect(c); return map_err_bits(bits); }
  if (kept > c->cfg.max_batch_keys) { prof_collect(c); return SHK_ERR_BATCH; }
  int dst = 0;
  rc = partition_words(c, c->d_words[0], kept, &dst);
  if (rc) return finish(c, rc);
  // to the table the call is one chunk: the trigger is tested once, behind it
  rc = merge_stage(c, c->d_words[dst], 1, kept, &st);
  if (stats) *stats = st;
  if (sstats) { sstats->kmers = kmers; sstats->kept = kept; }
  return finish(c, rc);
}

// ------------------------------------------------------------------ FASTA front end (fasta_kernels.hip)
// What shk_count_fasta keeps besides the context's buffers. Of those it borrows d_text (host text), d_words[0] (the list of
// run starts, until the roll kernels write their keys there), d_words[1] (the segments' 2-bit units, where pack_stage
// puts a FASTQ batch's) and the read arrays (one "read" per segment).
struct ShkFasta {
  uint32_t *stream = nullptr;       // the piece's bases behind the tail, 2 bits each
  uint64_t stream_words = 0;
  uint8_t *unit_state = nullptr;    // the state in front of every 16 text bytes
  uint32_t *tile_map = nullptr, *tile_state = nullptr;
  uint64_t *tile_cnt = nullptr, *tile_off = nullptr;
  uint64_t *long_runs = nullptr;    // k_fa_segments -> k_fa_long_segments: one record per run of many segments
  uint64_t cap_long = 0;
  uint64_t *counters = nullptr;     // [FA_NCOUNTERS] on the device
  uint64_t *h = nullptr;            // pinned: [0, FA_NCOUNTERS) the counters read back, [FA_NCOUNTERS] the scan's total
  // Two streams of pieces that do not see each other: [0] shk_count_fasta's, [1] shk_query_fasta's
  struct Stream {
    ShkQuad *tail[2] = {};          // the open run's last <= k - 1 bases (three units); tail[cur] is the committed one
    int cur = 0;
    uint32_t state = SHK_FA_STATE_START;
    uint64_t tail_len = 0;
  } s[2];
  // shk_query_fasta only
  uint64_t *tile_rec = nullptr, *rec_off = nullptr;   // header lines begun per tile, and their scan
  uint64_t *q_rec = nullptr;        // the piece's records: four sums each (record 0 = the one open when the piece began), then
  uint64_t q_rec_cap = 0;           // their first base ordinals; grown to the most records a piece has had
  uint32_t *q_track = nullptr;      // a host caller's track, grown to the most bases a piece with a track has had
  uint64_t q_track_cap = 0;
};
enum { FA_COUNT_STREAM = 0, FA_QUERY_STREAM = 1 };
static uint32_t fasta_threads(const shk_ctx *c) { return c->threads < 256 ? c->threads : 256; }
static void fasta_destroy(shk_ctx *c);
static int fasta_alloc(shk_ctx *c);
static int fasta_init(shk_ctx *c) {
  if (c->fasta) return SHK_OK;
  const int rc = fasta_alloc(c);
  if (rc) fasta_destroy(c);      // (the next call tries again)
  return rc;
}
static int fasta_alloc(shk_ctx *c) {
  ShkFasta *F = new ShkFasta();
  c->fasta = F;
  const uint64_t nb = c->cfg.max_batch_bytes, ntiles = nb / (16 * fasta_threads(c)) + 2;
  F->stream_words = (nb + 192) / 16 + 16;     // (two quads of room behind the last base: shk_fa_unit loads a unit's neighbour)
  if (dmalloc(&F->stream, F->stream_words) || dmalloc(&F->unit_state, nb / 16 + 2) || dmalloc(&F->tile_map, ntiles) || dmalloc(&F->tile_state, ntiles) ||
      dmalloc(&F->tile_cnt, ntiles) || dmalloc(&F->tile_off, ntiles + 1) || dmalloc(&F->counters, FA_NCOUNTERS) || dmalloc(&F->tile_rec, ntiles) ||
      dmalloc(&F->rec_off, ntiles + 1)) return SHK_ERR_HIP;
  for (int i = 0; i < 2; i++)
    if (dmalloc(&F->s[i].tail[0], 3) || dmalloc(&F->s[i].tail[1], 3)) return SHK_ERR_HIP;
  F->cap_long = ntiles;
  if (dmalloc(&F->long_runs, SHK_FA_LONG_WORDS * F->cap_long)) return SHK_ERR_HIP;
  HIPCHK(hipHostMalloc((void **)&F->h, (FA_NCOUNTERS + 1) * sizeof(uint64_t), hipHostMallocDefault));
  return SHK_OK;
}
static void fasta_destroy(shk_ctx *c) {
  ShkFasta *F = c->fasta;
  if (!F) return;
  if (c->stream) hipStreamSynchronize(c->stream);
  hipFree(F->stream); hipFree(F->unit_state); hipFree(F->tile_map); hipFree(F->tile_state); hipFree(F->tile_cnt); hipFree(F->tile_off);
  hipFree(F->counters); hipFree(F->long_runs); hipFree(F->tile_rec); hipFree(F->rec_off); hipFree(F->q_rec); hipFree(F->q_track);
  for (int i = 0; i < 2; i++) { hipFree(F->s[i].tail[0]); hipFree(F->s[i].tail[1]); }
  hipHostFree(F->h);
  delete F;
  c->fasta = nullptr;
}

// The piece's segments -> key words partitioned by region in d_words[*dst]. Two levels and more: roll_keys behind
// pack_stage, with counted bases. One level (roll_path() is false): the same scatter kernel with a single digit leaves the
// words in d_words[0], and they go through the partition as a caller's words do.
static int fasta_keys(shk_ctx *c, uint64_t nseg, uint64_t nkmers, int *dst) {
  if (!nseg) return partition_words(c, c->d_words[0], 0, dst);
  c->h_pinned[HP_NREADS] = nseg;
  HIPCHK(hipMemcpyAsync(c->d_scalars + DS_NREADS, c->h_pinned + HP_NREADS, 8, hipMemcpyHostToDevice, c->stream));
  ShkRollBatch R = {};
  R.nreads = nseg; R.nchunks = 1; R.chunk_mul = 1; R.staged = true; R.split = split_batch(c, 1);
  if (roll_path(c)) {
    { int rc = roll_keys(c, c, R, false); if (rc) return rc; }
    uint32_t bits = 0;
    HIPCHK(hipMemcpyAsync(c->h_pinned + HP_NWORDS, c->d_scalars + DS_NWORDS, 8, hipMemcpyDeviceToHost, c->stream));
    if (fetch_err(c, &bits)) return SHK_ERR_HIP;
    if (bits) return map_err_bits(bits);
    if (c->h_pinned[HP_NWORDS] != nkmers) return SHK_ERR_CORRUPT;
    const int rc = partition_stage(c, c, part_from_roll(c, c, nkmers, 1), dst);
    return rc == SHK_RC_REDO_UP ? SHK_ERR_CORRUPT : rc;
  }
  ShkRollArgs A;
  roll_args(c, c, A, nullptr, 0, 0, 1);
  A.q_lo = c->q_lo; A.dig_shift = 0; A.dig_bits = 0; A.hist = nullptr; A.hist_shift = 0; A.hist_bits = 0;
  A.cursor = c->d_cursor; A.out = c->d_words[0];
  A.pk = (const ShkQuad *)c->d_words[1]; A.pk_base = c->d_key_base; A.pk_flag = c->d_nkeys;
  HIPCHK(hipMemsetAsync(c->d_cursor, 0, 8, c->stream));
  launch_roll_scatter(c, c, A, nseg);
  HIPCHK(hipGetLastError());
  if (set_nwords(c, nkmers)) return SHK_ERR_HIP;
  return partition_stage(c, c, part_from_words(c, c->d_words[0], nkmers), dst);
}

// What shk_query_fasta wants of the front end besides the segments (null: shk_count_fasta)
struct ShkFaQuery {
  bool want_track; uint64_t track_cap;
  bool want_rec; uint32_t rec_cap; uint32_t *nrec_out;
};
// One piece of a stream through the front end
struct ShkFaPiece {
  uint64_t tail, nbases, nbreaks, nrec, nseg, nkmers, new_tail;
  uint32_t end_state;
};
// Stages (a) to (d) of a piece of stream S: classes, stream and run list, segments and their 2-bit units, the new tail
// (written to the stream's spare tail buffer: the caller commits it, with P's end state, once the piece has been taken).
// Leaves the segments as staged reads: the read arrays, d_key_base, d_nkeys, and the units in d_words[1].
static int fasta_front(shk_ctx *c, ShkFasta::Stream *S, const void *text, int text_on_device, uint64_t text_bytes, int first, const ShkFaQuery *Q,
                       ShkFaPiece *P) {
  ShkFasta *F = c->fasta;
  const uint32_t st0 = first ? SHK_FA_STATE_START : S->state, k = c->cfg.k, t = fasta_threads(c);
  const uint64_t tail = first ? 0 : S->tail_len;
  const uint8_t *dtext = (const uint8_t *)text;
  if (!text_on_device && text_bytes) {
    HIPCHK(hipMemcpyAsync(c->d_text, text, text_bytes, hipMemcpyHostToDevice, c->stream));
    dtext = c->d_text;
  }
  const uint64_t safe_end = (text_bytes + 15) & ~15ULL, ntiles = (text_bytes + 16 * t - 1) / (16 * t);
  const dim3 tiles((uint32_t)(ntiles ? ntiles : 1));
  // (a) the classes: maps, the tiles' states, counts; the tiles' bases and run starts through one scan
  HIPCHK(hipMemsetAsync(F->counters, 0, FA_NCOUNTERS * 8, c->stream));
  if (ntiles) { ProfScope ps(c, KP_FA_MAPS);
    hipLaunchKernelGGL(k_fa_maps, tiles, dim3(t), 0, c->stream, dtext, text_bytes, safe_end, F->tile_map); }
  { ProfScope ps(c, KP_FA_STATES);
    hipLaunchKernelGGL(k_fa_states, dim3(1), dim3(c->threads), 0, c->stream, (const uint32_t *)F->tile_map, ntiles, st0, F->tile_state, F->counters + FA_END_STATE); }
  if (ntiles) { ProfScope ps(c, KP_FA_COUNT);
    hipLaunchKernelGGL(k_fa_count, tiles, dim3(t), 0, c->stream, dtext, text_bytes, safe_end, (const uint32_t *)F->tile_state, F->unit_state,
                       F->tile_cnt, F->counters, Q ? F->tile_rec : (uint64_t *)nullptr); }
  if (run_scan<uint64_t>(c, c, F->tile_cnt, ntiles, nullptr, F->tile_off)) return SHK_ERR_HIP;
  // (the header lines per tile need a scan of their own: the tile word's 36 + 28 bits are taken)
  if (Q && run_scan<uint64_t>(c, c, F->tile_rec, ntiles, nullptr, F->rec_off)) return SHK_ERR_HIP;
  HIPCHK(hipMemcpyAsync(F->h, F->counters, FA_NCOUNTERS * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(F->h + FA_NCOUNTERS, F->tile_off + ntiles, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint64_t nbases = F->h[FA_NCOUNTERS] & SHK_FA_COUNT_MASK, nruns = 1 + (F->h[FA_NCOUNTERS] >> SHK_FA_COUNT_BITS);
  const uint64_t nrec = F->h[FA_NREC];
  const uint32_t end_state = (uint32_t)F->h[FA_END_STATE];
  P->tail = tail; P->nbases = nbases; P->nbreaks = F->h[FA_NBREAK]; P->nrec = nrec; P->end_state = end_state;
  const uint64_t cap_runs = words_cap(c), cap_units = c->cfg.max_batch_keys / 2 > 1 ? c->cfg.max_batch_keys / 2 - 1 : 0;
  if (nruns + 1 > cap_runs) { prof_collect(c); return SHK_ERR_BATCH; }
  if (Q) {
    // what the caller's arrays must hold is known here, before anything of the stream's has moved
    if (nrec + 1 > 0xFFFFFFFFull) { prof_collect(c); return SHK_ERR_BATCH; }
    if (Q->nrec_out) *Q->nrec_out = (uint32_t)(nrec + 1);
    if ((Q->want_track && Q->track_cap < nbases) || (Q->want_rec && Q->rec_cap < nrec + 1)) { prof_collect(c); return SHK_ERR_BATCH; }
    if (nrec + 1 > F->q_rec_cap) {
      hipFree(F->q_rec); F->q_rec = nullptr; F->q_rec_cap = 0;
      const uint64_t want = nrec + 1 + (nrec + 1) / 2;
      if (dmalloc(&F->q_rec, 5 * want)) { prof_collect(c); return SHK_ERR_HIP; }
      F->q_rec_cap = want;
    }
    if (nrec) { ProfScope ps(c, KP_FA_REC_STARTS);
      hipLaunchKernelGGL(k_fa_rec_starts, tiles, dim3(t), 0, c->stream, dtext, text_bytes, safe_end, (const uint8_t *)F->unit_state, (const uint64_t *)F->tile_off,
                         (const uint64_t *)F->rec_off, ntiles, tail, F->q_rec + 4 * (nrec + 1), nrec); }
  }
  // (b) the stream and the run list, (c) the segments, (d) the tail
  uint64_t *run_start = c->d_words[0];
  { const uint64_t used = ((tail + nbases + 15) / 16 + 12) * 4;
    HIPCHK(hipMemsetAsync(F->stream, 0, used < F->stream_words * 4 ? used : F->stream_words * 4, c->stream));
    if (tail) HIPCHK(hipMemcpyAsync(F->stream, S->tail[S->cur], 48, hipMemcpyDeviceToDevice, c->stream)); }
  ShkFaSegArgs G;
  G.run_start = run_start; G.nruns = nruns; G.k = k; G.seg = c->fasta_seg;
  G.rd_start = c->d_rd_start; G.rd_end = c->d_rd_end; G.rd_chunk = c->d_rd_chunk; G.flag = c->d_nkeys; G.pk_base = c->d_key_base;
  G.cap_seg = c->max_reads; G.cap_units = cap_units; G.long_runs = F->long_runs; G.cap_long = F->cap_long; G.counters = F->counters; G.err = c->d_err;
  { ProfScope ps(c, KP_FA_COMPACT);
    hipLaunchKernelGGL(k_fa_compact, tiles, dim3(t), 0, c->stream, dtext, text_bytes, safe_end, (const uint8_t *)F->unit_state, (const uint64_t *)F->tile_off,
                       ntiles, tail, F->stream, F->stream_words, run_start, cap_runs, c->d_err); }
  { ProfScope ps(c, KP_FA_SEGMENTS);
    const uint64_t blocks = nruns / t + 1;
    hipLaunchKernelGGL(k_fa_segments, dim3((uint32_t)(blocks < 2048 ? blocks : 2048)), dim3(t), 0, c->stream, G);
    hipLaunchKernelGGL(k_fa_long_segments, dim3(c->threads < 512 ? 2 : 512), dim3(t), 0, c->stream, G);     // (small workgroups: the CPU emulator build of the tests)
    hipLaunchKernelGGL(k_fa_tail, dim3(1), dim3(64), 0, c->stream, (const uint32_t *)F->stream, (const uint64_t *)run_start, nruns, end_state, k,
                       S->tail[S->cur ^ 1], F->counters); }
  HIPCHK(hipMemcpyAsync(F->h, F->counters, FA_NCOUNTERS * 8, hipMemcpyDeviceToHost, c->stream));
  uint64_t nseg = 0, nkmers = 0;
  { uint32_t bits = 0;
    if (fetch_err(c, &bits)) return SHK_ERR_HIP;
    nseg = F->h[FA_NSEG]; nkmers = F->h[FA_NKMERS];
    if (nkmers > c->cfg.max_batch_keys || nseg > c->max_reads || F->h[FA_NUNITS] > cap_units) { prof_collect(c); return SHK_ERR_BATCH; }
    if (bits) { prof_collect(c); return map_err_bits(bits); } }
  if (nseg) {
    ProfScope ps(c, KP_FA_PACK);
    const uint64_t pb = nseg * 4 / t + 1;
    hipLaunchKernelGGL(k_fa_pack, dim3((uint32_t)(pb < 16384 ? pb : 16384)), dim3(t), 0, c->stream, (const uint32_t *)F->stream, nseg, (const uint64_t *)c->d_rd_start,
                       (const uint64_t *)c->d_rd_end, (const uint64_t *)c->d_key_base, (const uint32_t *)c->d_nkeys, (ShkQuad *)c->d_words[1], cap_units, c->d_err);
  }
  HIPCHK(hipGetLastError());
  P->nseg = nseg; P->nkmers = nkmers; P->new_tail = F->h[FA_TAIL_LEN];
  return SHK_OK;
}

extern "C" int shk_count_fasta(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes, int first,
                               shk_batch_stats *stats, shk_fasta_stats *fstats) {
  if (!c || (!text && text_bytes) || c->cfg.num_shards > 1 || !text_aligned(text, text_on_device)) return SHK_ERR_ARG;
  if (c->front && c->front->count) return SHK_ERR_BATCH;     // (their words are partitioned against the table as it is now)
  if (text_bytes > c->cfg.max_batch_bytes) return SHK_ERR_BATCH;
  shk_batch_stats st;
  memset(&st, 0, sizeof(st));
  HIPCHK(hipSetDevice(c->dev));
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  { int rc = fasta_init(c); if (rc) return rc; }
  ShkFasta::Stream *S = &c->fasta->s[FA_COUNT_STREAM];
  ShkFaPiece P;
  { int rc = fasta_front(c, S, text, text_on_device, text_bytes, first, nullptr, &P); if (rc) return rc; }
  int dst = 0;
  int rc = fasta_keys(c, P.nseg, P.nkmers, &dst);
  if (rc) return finish(c, rc);
  // to the table the piece is one chunk: the trigger is tested once, behind it
  rc = merge_stage(c, c->d_words[dst], 1, P.nkmers, &st);
  rc = finish(c, rc);
  if (rc == SHK_OK || st.chunks) {       // (the chunk is in the table: the stream has moved on, whatever a round behind it did)
    S->cur ^= 1; S->state = P.end_state; S->tail_len = P.new_tail;
  }
  if (stats) *stats = st;
  if (fstats) { fstats->records = P.nrec; fstats->bases = P.nbases; fstats->breaks = P.nbreaks; fstats->kmers = st.kmers; }
  return rc;
}

// ------------------------------------------------------------------ FASTA text against the table (query_kernels.hip)
extern "C" int shk_query_fasta(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes, int first, uint32_t min_count,
                               uint32_t *track, uint64_t track_cap, int track_on_device, shk_query_record *rec, uint32_t rec_cap, uint32_t *nrec,
                               shk_query_stats *qstats) {
  if (!c || (!text && text_bytes) || c->cfg.num_shards > 1 || !text_aligned(text, text_on_device)) return SHK_ERR_ARG;
  if (c->front && c->front->count) return SHK_ERR_BATCH;     // (the call borrows the batch buffers their words may lie in)
  if (text_bytes > c->cfg.max_batch_bytes) return SHK_ERR_BATCH;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  { int rc = fasta_init(c); if (rc) return rc; }
  ShkFasta *F = c->fasta;
  ShkFasta::Stream *S = &F->s[FA_QUERY_STREAM];
  ShkFaQuery Q;
  Q.want_track = track != nullptr; Q.track_cap = track_cap; Q.want_rec = rec != nullptr; Q.rec_cap = rec_cap; Q.nrec_out = nrec;
  ShkFaPiece P;
  { int rc = fasta_front(c, S, text, text_on_device, text_bytes, first, &Q, &P); if (rc) return rc; }
  const uint64_t nr = P.nrec + 1;
  uint32_t *dtrack = nullptr;
  if (track && P.nbases) {
    dtrack = track;
    if (!track_on_device) {
      if (P.nbases > F->q_track_cap) {
        hipFree(F->q_track); F->q_track = nullptr; F->q_track_cap = 0;
        if (dmalloc(&F->q_track, P.nbases)) return finish(c, SHK_ERR_HIP);
        F->q_track_cap = P.nbases;
      }
      dtrack = F->q_track;
    }
    HIPCHK(hipMemsetAsync(dtrack, 0xFF, P.nbases * 4, c->stream));
  }
  HIPCHK(hipMemsetAsync(F->q_rec, 0, nr * 32, c->stream));
  if (P.nseg) {
    ShkQueryArgs A;
    A.rd_start = c->d_rd_start; A.rd_end = c->d_rd_end; A.pk_base = c->d_key_base; A.pk = (const ShkQuad *)c->d_words[1]; A.nseg = P.nseg;
    A.k = c->cfg.k; A.hb = c->cfg.hb; A.tab = c->tab[c->cur]; A.q_lo = c->q_lo; A.nslots = c->nslots;
    A.rec_start = F->q_rec + 4 * nr; A.nrec = P.nrec; A.tail = P.tail; A.min_count = min_count;
    A.track = dtrack; A.track_len = P.nbases; A.acc = F->q_rec;
    ProfScope ps(c, KP_ROLL_QUERY);
    const uint32_t t = fasta_threads(c);
    const uint64_t blocks = P.nseg / t + 1, most = c->threads < 512 ? 4 : 4096;      // (small workgroups: the CPU emulator build of the tests)
    hipLaunchKernelGGL(k_roll_query, dim3((uint32_t)(blocks < most ? blocks : most)), dim3(t), 0, c->stream, A);
  }
  HIPCHK(hipGetLastError());
  std::vector<shk_query_record> own;
  shk_query_record *hr = rec;
  if (!hr) { own.resize(nr); hr = own.data(); }
  static_assert(sizeof(shk_query_record) == 32, "a record is the kernel's four sums");
  HIPCHK(hipMemcpyAsync(hr, F->q_rec, nr * 32, hipMemcpyDeviceToHost, c->stream));
  if (dtrack && !track_on_device) HIPCHK(hipMemcpyAsync(track, dtrack, P.nbases * 4, hipMemcpyDeviceToHost, c->stream));
  const int rc = finish(c, SHK_OK);
  if (rc) return rc;
  shk_query_stats q = {P.nrec, P.nbases, P.nbreaks, 0, 0, 0, 0};
  for (uint64_t i = 0; i < nr; i++) { q.kmers += hr[i].kmers; q.present += hr[i].present; q.solid += hr[i].solid; q.sum += hr[i].sum; }
  if (q.kmers != P.nkmers) return SHK_ERR_CORRUPT;      // (every k-mer the segments hold has been answered, once)
  S->cur ^= 1; S->state = P.end_state; S->tail_len = P.new_tail;
  if (qstats) *qstats = q;
  return SHK_OK;
}

// ------------------------------------------------------------------ FASTQ reads against the table (reads_kernels.hip)
// What shk_query_reads keeps besides the context's buffers. Of those it borrows d_text (host text), the read arrays,
// d_words[1] (the reads' 2-bit units, where pack_stage puts a counting batch's) and d_words[0] (the per-window values of
// a call that wants a median or a host track). pack_stage owns d_nkeys and d_key_base (the units' flags and places), so
// the windows of every read and their offsets have arrays of their own.
struct ShkReads {
  uint32_t *nwin = nullptr;         // [max_reads + 1] windows of every read
  uint64_t *woff = nullptr;         // [max_reads + 2] ... scanned
  shk_read_record *rec = nullptr;   // [max_reads] the records of a call whose rec is host memory
  uint64_t *totals = nullptr;       // [4] kmers, present, solid, sum of the call
};
static void reads_destroy(shk_ctx *c) {
  ShkReads *R = c->reads;
  if (!R) return;
  if (c->stream) hipStreamSynchronize(c->stream);
  hipFree(R->nwin); hipFree(R->woff); hipFree(R->rec); hipFree(R->totals);
  delete R;
  c->reads = nullptr;
}
static int reads_init(shk_ctx *c) {
  if (c->reads) return SHK_OK;
  ShkReads *R = new ShkReads();
  c->reads = R;
  if (dmalloc(&R->nwin, c->max_reads + 1) || dmalloc(&R->woff, c->max_reads + 2) || dmalloc(&R->rec, c->max_reads + 1) || dmalloc(&R->totals, 4)) {
    reads_destroy(c);      // (the next call tries again)
    return SHK_ERR_HIP;
  }
  return SHK_OK;
}

extern "C" int shk_query_reads(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                               const uint64_t *chunk_len, uint32_t nchunks, uint32_t min_count, uint32_t flags, shk_read_record *rec,
                               uint64_t rec_cap, int rec_on_device, uint64_t *nreads_out, shk_read_extent *ext, uint32_t *track,
                               uint64_t track_cap, int track_on_device, uint64_t *nwindows, shk_reads_stats *rstats) {
  static_assert(sizeof(shk_read_record) == 32 && sizeof(shk_read_extent) == 16, "the kernel stores a record as two 16-byte halves");
  if (!c || !text || !rec || !nreads_out || (flags & ~SHK_READS_MEDIAN)) return SHK_ERR_ARG;
  if (c->cfg.num_shards > 1 || !text_aligned(text, text_on_device)) return SHK_ERR_ARG;
  if (c->front && c->front->count) return SHK_ERR_BATCH;     // (the call borrows the batch buffers their words may lie in)
  if (!chunk_labels_ok(nchunks, 0, 1)) return SHK_ERR_BATCH;
  if (!chunk_off || !chunk_len) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  { int rc = reads_init(c); if (rc) return rc; }
  ShkReads *R = c->reads;
  const uint8_t *dtext;
  uint64_t nreads;
  int rc = parse_stage(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, &dtext, &nreads);
  if (rc) return finish(c, rc);
  const uint32_t t = c->threads < 256 ? c->threads : 256;
  const bool small = c->threads < 512;      // (small workgroups: the CPU emulator build of the tests)
  { ProfScope ps(c, KP_MISC);
    const uint64_t blocks = nreads / t + 1;
    hipLaunchKernelGGL(k_reads_windows, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(t), 0, c->stream, (const uint64_t *)c->d_rd_start,
                       (const uint64_t *)c->d_rd_end, nreads, c->cfg.k, R->nwin, c->d_err); }
  if (run_scan<uint32_t>(c, c, R->nwin, nreads, nullptr, R->woff)) return finish(c, SHK_ERR_HIP);
  uint64_t nwin = 0;
  HIPCHK(hipMemcpyAsync(&nwin, R->woff + nreads, 8, hipMemcpyDeviceToHost, c->stream));
  rc = finish(c, SHK_OK);      // (malformed text, a read of more than 65535 bases: nothing has been written yet)
  if (rc) return rc;
  *nreads_out = nreads;
  if (nwindows) *nwindows = nwin;
  if (rec_cap < nreads || nwin > c->cfg.max_batch_keys || (track && track_cap < nwin)) return SHK_ERR_BATCH;
  shk_reads_stats q = {nreads, 0, 0, 0, 0};
  if (nreads == 0) { if (rstats) *rstats = q; return SHK_OK; }
  const bool median = (flags & SHK_READS_MEDIAN) != 0;
  // the per-window values: straight into a device track; else, for a host track or the median, into d_words[0]
  // (max_batch_keys words of 8 bytes for at most max_batch_keys entries of 4)
  uint32_t *dwin = nullptr;
  if (nwin && (track || median)) dwin = track && track_on_device ? track : (uint32_t *)c->d_words[0];
  shk_read_record *drec = rec_on_device ? rec : R->rec;
  ShkRollArgs P;
  roll_args(c, c, P, dtext, text_bytes, 0, 1);
  rc = pack_stage(c, c, P, nreads, text_bytes, c->d_words[1]);
  if (rc) return finish(c, rc);
  HIPCHK(hipMemsetAsync(R->totals, 0, 32, c->stream));
  {
    ShkReadsArgs A;
    A.text = dtext; A.rd_start = c->d_rd_start; A.rd_end = c->d_rd_end; A.nreads = nreads;
    A.pk = P.pk; A.pk_base = P.pk_base; A.pk_flag = P.pk_flag; A.woff = R->woff;
    A.k = c->cfg.k; A.hb = c->cfg.hb; A.tab = c->tab[c->cur]; A.q_lo = c->q_lo; A.nslots = c->nslots; A.min_count = min_count;
    A.median = median ? 0 : SHK_QUERY_NONE; A.win = dwin; A.rec = drec; A.totals = R->totals;
    ProfScope ps(c, KP_READS_QUERY);
    const uint64_t blocks = nreads / t + 1, most = small ? 4 : 4096;
    hipLaunchKernelGGL(k_reads_query, dim3((uint32_t)(blocks < most ? blocks : most)), dim3(t), 0, c->stream, A);
  }
  if (median && nwin) {
    ProfScope ps(c, KP_READS_MEDIAN);
    const uint64_t blocks = nreads / (t / SHK_READS_GROUP) + 1, most = small ? 4 : 16384;
    hipLaunchKernelGGL(k_reads_median, dim3((uint32_t)(blocks < most ? blocks : most)), dim3(t), 0, c->stream, (const uint32_t *)dwin,
                       (const uint64_t *)R->woff, nreads, drec);
  }
  HIPCHK(hipGetLastError());
  // (every capacity has been compared above: from here on only the runtime itself can fail)
  std::vector<uint64_t> hst, hen;
  std::vector<uint16_t> hch;
  uint64_t tot[4] = {0, 0, 0, 0};
  if (!rec_on_device) HIPCHK(hipMemcpyAsync(rec, R->rec, nreads * 32, hipMemcpyDeviceToHost, c->stream));
  if (track && !track_on_device && nwin) HIPCHK(hipMemcpyAsync(track, dwin, nwin * 4, hipMemcpyDeviceToHost, c->stream));
  if (ext) {
    hst.resize(nreads); hen.resize(nreads); hch.resize(nreads);
    HIPCHK(hipMemcpyAsync(hst.data(), c->d_rd_start, nreads * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hen.data(), c->d_rd_end, nreads * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hch.data(), c->d_rd_chunk, nreads * 2, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipMemcpyAsync(tot, R->totals, 32, hipMemcpyDeviceToHost, c->stream));
  rc = finish(c, SHK_OK);
  if (rc) return rc;
  if (ext)
    for (uint64_t r = 0; r < nreads; r++) { ext[r].seq_off = hst[r]; ext[r].seq_len = (uint32_t)(hen[r] - hst[r]); ext[r].chunk = hch[r]; }
  q.kmers = tot[0]; q.present = tot[1]; q.solid = tot[2]; q.sum = tot[3];
  if (rstats) *rstats = q;
  return SHK_OK;
}

// ------------------------------------------------------------------ FASTQ reads repaired against the table (correct_kernels.hip)
// What shk_correct_reads keeps besides the context's buffers. It borrows what shk_query_reads borrows (d_text for host
// text, the read arrays, d_words[1] for the reads' 2-bit units, into which the kernel writes its edits); the records and
// the edit lists of a call whose arrays are host memory have buffers here that grow with the largest batch.
struct ShkCorrect {
  shk_correct_record *rec = nullptr; uint64_t rec_cap = 0;
  uint32_t *edits = nullptr; uint64_t edits_cap = 0;
  uint64_t *totals = nullptr;       // [SHK_CORRECT_TOTALS]
  uint64_t lookups = 0;             // of the last call (shk_correct_lookups)
};
static void correct_destroy(shk_ctx *c) {
  ShkCorrect *R = c->correct;
  if (!R) return;
  if (c->stream) hipStreamSynchronize(c->stream);
  hipFree(R->rec); hipFree(R->edits); hipFree(R->totals);
  delete R;
  c->correct = nullptr;
}
template <typename T>
static int correct_grow(shk_ctx *c, T **buf, uint64_t *cap, uint64_t want) {
  if (want <= *cap) return SHK_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  hipFree(*buf); *buf = nullptr; *cap = 0;
  if (dmalloc(buf, want + want / 2)) return SHK_ERR_HIP;
  *cap = want + want / 2;
  return SHK_OK;
}

extern "C" uint64_t shk_correct_lookups(shk_ctx *c) { return c && c->correct ? c->correct->lookups : 0; }

extern "C" int shk_correct_reads(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                                 const uint64_t *chunk_len, uint32_t nchunks, uint32_t min_count, uint32_t check, uint32_t max_edits,
                                 shk_correct_record *rec, uint64_t rec_cap, int rec_on_device, uint64_t *nreads_out, shk_read_extent *ext,
                                 uint32_t *edits, int edits_on_device, shk_correct_stats *cstats) {
  static_assert(sizeof(shk_correct_record) == 16, "the kernel stores a record as one 16-byte store");
  if (!c || !text || !rec || !edits || !nreads_out || min_count == 0 || check > 255 || max_edits < 1 || max_edits > 16) return SHK_ERR_ARG;
  if (c->cfg.num_shards > 1 || !text_aligned(text, text_on_device)) return SHK_ERR_ARG;
  if (c->front && c->front->count) return SHK_ERR_BATCH;     // (the call borrows the batch buffers their words may lie in)
  if (!chunk_labels_ok(nchunks, 0, 1)) return SHK_ERR_BATCH;
  if (!chunk_off || !chunk_len) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  if (!c->correct) {
    c->correct = new ShkCorrect();
    if (dmalloc(&c->correct->totals, SHK_CORRECT_TOTALS)) { correct_destroy(c); return SHK_ERR_HIP; }      // (the next call tries again)
  }
  ShkCorrect *R = c->correct;
  const uint8_t *dtext;
  uint64_t nreads;
  int rc = parse_stage(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, &dtext, &nreads);
  if (rc) return finish(c, rc);
  const uint32_t t = c->threads < 256 ? c->threads : 256;
  const bool small = c->threads < 512;      // (small workgroups: the CPU emulator build of the tests)
  { ProfScope ps(c, KP_MISC);
    const uint64_t blocks = nreads / t + 1;
    hipLaunchKernelGGL(k_correct_check, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(t), 0, c->stream, (const uint64_t *)c->d_rd_start,
                       (const uint64_t *)c->d_rd_end, nreads, c->d_err); }
  // the units go into library memory only, so they are packed before the text has been judged: one wait for both answers
  ShkRollArgs P;
  roll_args(c, c, P, dtext, text_bytes, 0, 1);
  P.pk = nullptr;
  if (nreads) { rc = pack_stage(c, c, P, nreads, text_bytes, c->d_words[1], false); if (rc) return finish(c, rc); }
  uint64_t units = 0;
  if (P.pk) HIPCHK(hipMemcpyAsync(&units, c->d_key_base + nreads, 8, hipMemcpyDeviceToHost, c->stream));
  rc = finish(c, SHK_OK);      // (malformed text, a read of more than 65535 bases: nothing has been written yet)
  if (rc) return rc;
  *nreads_out = nreads;
  if (rec_cap < nreads || (nreads && (!P.pk || units > pack_cap_units(c)))) return SHK_ERR_BATCH;
  shk_correct_stats q = {nreads, 0, 0, 0, 0, 0, 0};
  R->lookups = 0;
  if (nreads == 0) { if (cstats) *cstats = q; return SHK_OK; }
  if (!rec_on_device) { rc = correct_grow(c, &R->rec, &R->rec_cap, nreads); if (rc) return rc; }
  if (!edits_on_device) { rc = correct_grow(c, &R->edits, &R->edits_cap, nreads * max_edits); if (rc) return rc; }
  shk_correct_record *drec = rec_on_device ? rec : R->rec;
  uint32_t *dedits = edits_on_device ? edits : R->edits;
  HIPCHK(hipMemsetAsync(R->totals, 0, SHK_CORRECT_TOTALS * 8, c->stream));
  {
    ShkCorrectArgs A;
    A.rd_start = c->d_rd_start; A.rd_end = c->d_rd_end; A.nreads = nreads;
    A.pk = (ShkQuad *)c->d_words[1]; A.pk_base = P.pk_base; A.pk_flag = P.pk_flag;
    A.k = c->cfg.k; A.hb = c->cfg.hb; A.tab = c->tab[c->cur]; A.q_lo = c->q_lo; A.nslots = c->nslots;
    A.min_count = min_count; A.check = check; A.max_edits = max_edits;
    A.rec = drec; A.edits = dedits; A.totals = R->totals;
    ProfScope ps(c, KP_READS_CORRECT);
    const uint64_t blocks = nreads / t + 1, most = small ? 4 : 4096;
    hipLaunchKernelGGL(k_reads_correct, dim3((uint32_t)(blocks < most ? blocks : most)), dim3(t), 0, c->stream, A);
  }
  HIPCHK(hipGetLastError());
  // (every capacity has been compared above: from here on only the runtime itself can fail)
  std::vector<uint64_t> hst, hen;
  std::vector<uint16_t> hch;
  uint64_t tot[SHK_CORRECT_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
  if (!rec_on_device) HIPCHK(hipMemcpyAsync(rec, R->rec, nreads * 16, hipMemcpyDeviceToHost, c->stream));
  if (!edits_on_device) HIPCHK(hipMemcpyAsync(edits, R->edits, nreads * max_edits * 4, hipMemcpyDeviceToHost, c->stream));
  if (ext) {
    hst.resize(nreads); hen.resize(nreads); hch.resize(nreads);
    HIPCHK(hipMemcpyAsync(hst.data(), c->d_rd_start, nreads * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hen.data(), c->d_rd_end, nreads * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hch.data(), c->d_rd_chunk, nreads * 2, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipMemcpyAsync(tot, R->totals, SHK_CORRECT_TOTALS * 8, hipMemcpyDeviceToHost, c->stream));
  rc = finish(c, SHK_OK);
  if (rc) return rc;
  if (ext)
    for (uint64_t r = 0; r < nreads; r++) { ext[r].seq_off = hst[r]; ext[r].seq_len = (uint32_t)(hen[r] - hst[r]); ext[r].chunk = hch[r]; }
  q.candidates = tot[CT_CANDIDATES]; q.edited_reads = tot[CT_EDITED]; q.edits = tot[CT_EDITS]; q.unfixable = tot[CT_UNFIXABLE];
  q.ambiguous = tot[CT_AMBIGUOUS]; q.capped = tot[CT_CAPPED];
  R->lookups = tot[CT_LOOKUPS];
  if (cstats) *cstats = q;
  return SHK_OK;
}

// where routed words go: one of two alternating send buffers (allocated on first use)
static int send_buffer(shk_ctx *c, uint64_t **send) {
  const int b = c->send_next;
  if (!c->d_send[b] && dmalloc(&c->d_send[b], c->cfg.max_batch_keys + 1)) return SHK_ERR_HIP;
  *send = c->d_send[b];
  c->send_next ^= 1;
  return SHK_OK;
}

// Owner bins of the two routing calls, in d_block_sums (nbins <= 1024): the counters a histogram pass fills at ROUTE_HIST,
// the cursors its scatter pass takes at ROUTE_CURSOR. Zeroes the counters, has `count` launch the histogram pass, and
// turns the counts into the words per owner (per_owner consecutive bins each), the bins' bases (base[nbins] = all words;
// the caller's, so that it outlives the copy) and the cursors. Kernel errors so far are the return code.
enum { ROUTE_HIST = 0, ROUTE_CURSOR = 4096 };
template <typename F>
static int owner_bins(shk_ctx *c, uint32_t nbins, uint32_t per_owner, F count, uint64_t *counts, std::vector<uint64_t> &base) {
  uint64_t *hist = c->d_block_sums + ROUTE_HIST;
  HIPCHK(hipMemsetAsync(hist, 0, nbins * 8, c->stream));
  count();
  std::vector<uint64_t> hh(nbins);
  HIPCHK(hipMemcpyAsync(hh.data(), hist, nbins * 8, hipMemcpyDeviceToHost, c->stream));
  uint32_t bits = 0;
  if (fetch_err(c, &bits)) return SHK_ERR_HIP;
  if (bits) return map_err_bits(bits);
  base.assign(nbins + 1, 0);
  std::fill(counts, counts + nbins / per_owner, 0);
  for (uint32_t i = 0; i < nbins; i++) { counts[i / per_owner] += hh[i]; base[i + 1] = base[i] + hh[i]; }
  HIPCHK(hipMemcpyAsync(c->d_block_sums + ROUTE_CURSOR, base.data(), nbins * 8, hipMemcpyHostToDevice, c->stream));
  return SHK_OK;
}

extern "C" int shk_route_words(shk_ctx *c, uint64_t nwords, uint32_t nshards, uint64_t **d_out, uint64_t *counts) {
  if (!c || !d_out || !counts || nshards == 0 || (nshards & (nshards - 1)) || nshards > SHK_RP_MAXP) return SHK_ERR_ARG;
  if (nwords > c->cfg.max_batch_keys) return SHK_ERR_BATCH;
  HIPCHK(hipSetDevice(c->dev));
  uint32_t lg = 0;
  while ((1u << lg) < nshards) lg++;
  uint64_t *send;
  if (send_buffer(c, &send)) return SHK_ERR_HIP;
  if (lg == 0) {
    HIPCHK(hipMemcpyAsync(send, c->d_words[0], nwords * 8, hipMemcpyDeviceToDevice, c->stream));
    *d_out = send; counts[0] = nwords;
    return finish(c, 0);
  }
  if (c->cfg.qb < SHK_REGION_LOG2 + lg) return SHK_ERR_ARG;
  // one partition level over the WHOLE filter's regions: digit = owner
  ShkRpLevel lv;
  lv.shift = (c->cfg.qb - SHK_REGION_LOG2) - lg; lv.bits = lg; lv.nbuckets = 1; lv.hb = c->cfg.hb; lv.q_lo = 0;
  lv.nslots = ~0ULL; lv.cb = 0; lv.out32 = 0; lv.ablate = 0; lv.ng_log2 = 0; lv.slot_cap = 0; lv.kb = 0; lv.hi_off = 0;
  if (set_nwords(c, nwords)) return SHK_ERR_HIP;
  const uint64_t *n_p = c->d_scalars + DS_NWORDS;
  const uint32_t nwin = (uint32_t)(nwords / SHK_RP_TILE + 1);
  { ProfScope ps(c, KP_RP_PREP);
    hipLaunchKernelGGL(k_rp_base1, dim3(1), dim3(64), 0, c->stream, n_p, c->d_base[0]);
    hipLaunchKernelGGL(k_rp_tile_first, dim3(nwin / 256 + 1), dim3(256), 0, c->stream, c->d_base[0], 1u, n_p, c->d_tfb); }
  std::vector<uint64_t> base;
  int rc = owner_bins(c, nshards, 1, [&] {
    ProfScope ps(c, KP_RP_HIST);
    const uint32_t wt = nwin / 4096 + 1;
    hipLaunchKernelGGL(k_rp_hist<false>, dim3(nwin / wt + 1), dim3(c->threads), 0, c->stream, c->d_words[0], n_p, c->d_base[0], (const uint64_t *)nullptr, c->d_tfb, lv, c->d_block_sums + ROUTE_HIST, wt);
  }, counts, base);
  if (rc) return finish(c, rc);
  { ProfScope ps(c, KP_RP_SCATTER);
    hipLaunchKernelGGL((k_rp_scatter<12, SHK_RP_THREADS>), dim3(nwin), dim3(SHK_RP_THREADS), 0, c->stream, c->d_words[0], send, n_p,
                       c->d_base[0], (const uint64_t *)nullptr, c->d_tfb, lv, c->d_block_sums + ROUTE_CURSOR, c->d_err); }
  HIPCHK(hipGetLastError());
  *d_out = send;
  return finish(c, 0);
}

// shk_hash_chunks + shk_route_words in one: the roll kernels (roll_kernels.hip) hash every k-mer and send it straight
// to its OWNER's bin of the send buffer (digit = the top log2(nshards) bits of the whole filter's regions) -- no key word
// is written to HBM and read back before the exchange. Chunk i is labelled i * num_shards + shard_index as in
// shk_hash_chunks.
extern "C" int shk_hash_route_chunks(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                                     const uint64_t *chunk_len, uint32_t nchunks, uint32_t nshards, uint64_t **d_out, uint64_t *counts,
                                     uint64_t *nwords) {
  if (!c || !text || !chunk_off || !chunk_len || !d_out || !counts || !nwords) return SHK_ERR_ARG;
  if (nshards == 0 || (nshards & (nshards - 1)) || nshards > SHK_RP_MAXP) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  uint32_t lg = 0;
  while ((1u << lg) < nshards) lg++;
  if (c->cfg.qb < SHK_REGION_LOG2 + lg) return SHK_ERR_ARG;
  const uint32_t chunk_first = c->cfg.shard_index, chunk_mul = c->cfg.num_shards ? c->cfg.num_shards : 1;
  if (!chunk_labels_ok(nchunks, chunk_first, chunk_mul)) return SHK_ERR_BATCH;
  uint64_t *send;
  if (send_buffer(c, &send)) return SHK_ERR_HIP;
  const uint8_t *dtext;
  uint64_t nreads;
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  int rc = parse_stage(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, &dtext, &nreads);
  if (rc) return finish(c, rc);
  // The words are binned by MORE bits than the owner's (7, when the filter has them): with a handful of bins every
  // lane's LDS atomic lands on the same few counters (one rank: 64-way serialised, the kernels took 3.3 and 8.3 ms
  // instead of 1.3 and 4.7). An owner's bin is then 2^(bits - lg) consecutive sub-bins, contiguous in the send buffer.
  const uint32_t rb = c->cfg.qb - SHK_REGION_LOG2;
  const uint32_t db = lg > 7 ? lg : (rb < 7 ? (rb > lg ? rb : lg) : 7);
  const uint32_t nbins = 1u << db, per_owner = nbins / nshards;
  ShkRollArgs A;
  roll_args(c, c, A, dtext, text_bytes, chunk_first, chunk_mul);
  A.q_lo = 0;                                   // (owners are ranges of the WHOLE filter's quotients)
  A.dig_shift = rb - db; A.dig_bits = db;
  A.hist_shift = A.dig_shift; A.hist_bits = db;
  A.hist = c->d_block_sums + ROUTE_HIST; A.cursor = c->d_block_sums + ROUTE_CURSOR; A.out = send;
  rc = pack_stage(c, c, A, nreads, text_bytes, c->d_words[0]);      // (d_words[0]: filled by shk_stage_words, after this call)
  if (rc) return finish(c, rc);
  // (the bins are zeroed behind pack_stage, whose scan uses the head of d_block_sums too)
  std::vector<uint64_t> base;
  rc = owner_bins(c, nbins, per_owner, [&] {
    ProfScope ps(c, KP_ROLL_HIST);
    launch_roll_hist(c, c, A, nreads, false);
  }, counts, base);
  if (rc) return finish(c, rc);
  *nwords = base[nbins];
  if (base[nbins] > c->cfg.max_batch_keys) return finish(c, SHK_ERR_BATCH);
  launch_roll_scatter(c, c, A, nreads);
  HIPCHK(hipGetLastError());
  *d_out = send;
  return finish(c, 0);
}

extern "C" int shk_route_reserve(shk_ctx *c) {
  if (!c) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  for (int b = 0; b < 2; b++)
    if (!c->d_send[b] && dmalloc(&c->d_send[b], c->cfg.max_batch_keys + 1)) return SHK_ERR_HIP;
  // (and the records of a deNoise point: a shard's rounds are decided outside the context)
  { int rc = ensure_chist(c); if (!rc) rc = point_alloc(c); if (rc) return rc; }
  lazy_reserve(c);               // (the second record buffer, otherwise allocated by the first lazy commit)
  return SHK_OK;
}

extern "C" int shk_stage_words_pair(shk_ctx *c, const uint64_t *d_a, uint64_t na, const uint64_t *d_b, uint64_t nb) {
  if (!c || (!d_a && na) || (!d_b && nb)) return SHK_ERR_ARG;
  if (na == 0) return shk_stage_words(c, d_b, nb);
  if (nb == 0) return shk_stage_words(c, d_a, na);
  if (na + nb > c->cfg.max_batch_keys) return SHK_ERR_BATCH;
  // (the first level writes d_words[0] while it reads both sources)
  { const uint64_t *o0 = c->d_words[0], *o1 = c->d_words[0] + c->cfg.max_batch_keys + 1;
    if ((d_a + na > o0 && d_a < o1) || (d_b + nb > o0 && d_b < o1)) return SHK_ERR_ARG; }
  if (c->nlevels == 0) return SHK_ERR_ARG;       // (a single region has no partition to read two sources: concatenate)
  HIPCHK(hipSetDevice(c->dev));
  if (set_nwords(c, na + nb)) return SHK_ERR_HIP;
  // the sources' lengths (DS_PAIR_LEN) and their one-bucket base arrays (DS_PAIR_BASE)
  const uint64_t pair[DS_END - DS_PAIR_LEN] = {na, nb, 0, na, 0, nb};
  memcpy(c->h_pinned + HP_PAIR, pair, sizeof(pair));
  HIPCHK(hipMemcpyAsync(c->d_scalars + DS_PAIR_LEN, c->h_pinned + HP_PAIR, sizeof(pair), hipMemcpyHostToDevice, c->stream));
  int dst = 0;
  int rc = partition_stage(c, c, part_from_words(c, d_a, na, d_b, nb), &dst);
  c->staged = dst; c->pass_words = na + nb;
  return finish(c, rc);
}

extern "C" int shk_stage_words(shk_ctx *c, const uint64_t *d_words, uint64_t nwords) {
  if (!c || (!d_words && nwords)) return SHK_ERR_ARG;
  if (nwords > c->cfg.max_batch_keys) return SHK_ERR_BATCH;
  HIPCHK(hipSetDevice(c->dev));
  int dst = 0;
  int rc = partition_words(c, d_words, nwords, &dst);
  c->staged = dst; c->pass_words = nwords;
  return finish(c, rc);
}

static void summary_out(const MergeOut &o, shk_summary *out) {
  out->new_distinct = o.newd; out->added = o.added; out->removed = o.removed;
  out->err_bits = o.err; out->reserved = 0;
}

extern "C" int shk_stage_summary(shk_ctx *c, uint32_t lo, uint32_t hi, int want_chunks, shk_summary *out) {
  if (!c || !out || hi < lo || hi >= SHK_MAX_CHUNKS) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  MergeOut o;
  int rc = merge_summary(c, c->d_words[c->staged], lo, hi, 0, &o, want_chunks != 0, true);
  if (!rc && !c->big_image && (o.err & (SHK_E_OLD_EXTENT | SHK_E_NEW_EXTENT)) && !(o.err & SHK_E_TABLE_FULL)) {
    c->big_image = 1;   // a cluster outgrew the small LDS image: same range with the big one
    rc = merge_summary(c, c->d_words[c->staged], lo, hi, 0, &o, want_chunks != 0, true);
  }
  prof_collect(c);
  if (rc) return rc;
  summary_out(o, out);
  return SHK_OK;
}

extern "C" int shk_stage_commit(shk_ctx *c, uint32_t lo, uint32_t hi, const shk_summary *s) {
  if (!c || !s || hi < lo) return SHK_ERR_ARG;
  if (s->err_bits) return map_err_bits(s->err_bits);
  HIPCHK(hipSetDevice(c->dev));
  int rc = merge_write(c, c->d_words[c->staged], lo, hi, 0);
  if (!rc) { c->ndistinct += s->new_distinct; c->nelts += s->added; }
  return finish(c, rc);
}

extern "C" int shk_stage_try(shk_ctx *c, uint32_t lo, uint32_t hi, int want_chunks, shk_summary *out) {
  if (!c || !out || hi < lo || hi >= SHK_MAX_CHUNKS) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  MergeOut o;
  int rc;
  for (int attempt = 0; attempt < 2; attempt++) {
    rc = merge_summary(c, c->d_words[c->staged], lo, hi, 0, &o, want_chunks != 0, true);
    if (rc || c->big_image || !(o.err & (SHK_E_OLD_EXTENT | SHK_E_NEW_EXTENT)) || (o.err & SHK_E_TABLE_FULL)) break;
    c->big_image = 1;
  }
  prof_collect(c);
  if (rc) return rc;
  summary_out(o, out);
  return SHK_OK;
}

extern "C" int shk_stage_accept(shk_ctx *c, const shk_summary *s) {
  if (!c || !s) return SHK_ERR_ARG;
  if (s->err_bits) return map_err_bits(s->err_bits);
  HIPCHK(hipSetDevice(c->dev));
  if (!c->spill_valid) return SHK_ERR_ARG;   // nothing was tried
  const int dn = c->spill_denoise;
  int rc = merge_write(c, c->spill_words, c->spill_lo, c->spill_hi, dn);
  if (rc) return finish(c, rc);
  if (dn) { c->big_image = 0; c->rounds_done++; }
  c->ndistinct += s->new_distinct; c->nelts += s->added;
  c->ndistinct -= s->removed; c->nelts -= s->removed;     // (only a deNoise try removes anything)
  return finish(c, SHK_OK);
}

// deNoise round on this shard fused with the insertion of the staged chunks [lo, hi] (the chunks behind the deNoise
// point): marks + statistics pass; nothing is written until shk_stage_accept. s->removed = singletons dropped,
// s->new_distinct counts dropped keys that reappear in [lo, hi] as new.
extern "C" int shk_stage_try_denoise(shk_ctx *c, uint32_t lo, uint32_t hi, shk_summary *out) {
  if (!c || !out || hi < lo || hi >= SHK_MAX_CHUNKS) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = marks_launch(c); if (rc) return rc; }
  MergeOut o;
  int rc = merge_summary(c, c->d_words[c->staged], lo, hi, 1, &o, false, true);
  prof_collect(c);
  if (rc) return rc;
  summary_out(o, out);
  return SHK_OK;
}

extern "C" int shk_stage_chunk_hist(shk_ctx *c, uint64_t *out, uint32_t n) {
  if (!c || !out || !c->chist_n || n > c->chist_n) return SHK_ERR_ARG;
  memcpy(out, c->h_chist, (size_t)n * sizeof(uint64_t));
  return SHK_OK;
}

// ---- one-pass deNoise point on a shard (shk/dist.py: the ranks take the steps together)
extern "C" int shk_stage_sample(shk_ctx *c, uint32_t lo, uint32_t hi, uint64_t *hist, uint32_t *regions, uint32_t *sampled,
                                uint32_t *err_bits) {
  if (!c || !hist || !regions || !sampled || !err_bits || hi < lo || hi >= SHK_MAX_CHUNKS) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  uint32_t ns = 0, err = 0;
  int rc = sample_pass(c, c->d_words[c->staged], lo, hi, &ns, &err);
  prof_collect(c);
  if (rc) return rc;
  memcpy(hist, c->h_chist, ((size_t)hi + 1) * sizeof(uint64_t));
  *regions = c->nregions; *sampled = ns; *err_bits = err;
  return SHK_OK;
}

extern "C" int shk_stage_point_try(shk_ctx *c, uint32_t lo, uint32_t split, uint32_t hi, shk_point *out) {
  if (!c || !out || hi < lo || split + 1 < lo || split > hi || hi >= SHK_MAX_CHUNKS) return SHK_ERR_ARG;   // (split = lo - 1: the round comes first)
  HIPCHK(hipSetDevice(c->dev));
  c->pt_valid = 0;
  memset(out, 0, sizeof(*out));
  // (the retry image is not instantiated for this pass: the caller takes another path)
  if (c->big_image) { out->err_bits = SHK_E_FUSED; return SHK_OK; }
  PointOut po;
  int rc = point_try(c, c->d_words[c->staged], lo, split, hi, true, &po);
  prof_collect(c);
  if (rc) return rc;
  out->new_after = po.newd_after; out->added_after = po.added_after; out->removed = po.removed; out->added_before = po.added_before;
  out->err_bits = po.err; out->first_used = (uint32_t)po.first_used; out->islots = po.islots; out->ifin = po.ifin;
  if (!po.err) { c->pt_lo = lo; c->pt_split = split; c->pt_hi = hi; c->pt_valid = 1; c->pt_nprot = 0; c->pt_words = c->d_words[c->staged]; }
  return SHK_OK;
}

// a deNoise round on its own (no words), taken the same way: the range walk then runs over the single table's layout
extern "C" int shk_stage_round_try(shk_ctx *c, shk_point *out) {
  if (!c || !out) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  c->pt_valid = 0;
  memset(out, 0, sizeof(*out));
  // (the retry image is not instantiated for this pass: the caller takes another path)
  if (c->big_image) { out->err_bits = SHK_E_FUSED; return SHK_OK; }
  PointOut po;
  int rc = point_try(c, nullptr, 0, 0, 0, false, &po);
  prof_collect(c);
  if (rc) return rc;
  out->new_after = po.newd_after; out->added_after = po.added_after; out->removed = po.removed; out->added_before = po.added_before;
  out->err_bits = po.err; out->first_used = (uint32_t)po.first_used; out->islots = po.islots; out->ifin = po.ifin;
  if (!po.err) { c->pt_lo = 1; c->pt_split = 0; c->pt_hi = 0; c->pt_valid = 1; c->pt_nprot = 0; c->pt_words = nullptr; }
  return SHK_OK;
}

extern "C" int shk_stage_point_walk(shk_ctx *c, int64_t carry, int64_t prev_fp, int last, int next_first_used,
                                    const uint64_t state_in[2], uint64_t state_out[2], uint64_t *nprot, uint32_t *err_bits) {
  if (!c || !state_in || !state_out || !nprot || !err_bits || carry < 0 || !c->pt_valid) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  ShkWalkShard W;
  W.prev_fp = prev_fp; W.cap_local = c->g_nslots - c->q_lo; W.last = last; W.next_first_used = next_first_used;
  int rc = point_walk(c, carry, W, state_in, state_out, nprot, err_bits);
  prof_collect(c);
  if (rc) return rc;
  c->pt_nprot = *nprot;
  return SHK_OK;
}

extern "C" int shk_stage_point_finish(shk_ctx *c, shk_point *out, shk_summary *accept) {
  if (!c || !out || !accept || !c->pt_valid || (c->pt_words && !c->chist_n)) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  PointOut po;
  po.newd_after = out->new_after; po.added_after = out->added_after; po.removed = out->removed; po.added_before = out->added_before;
  po.err = 0;
  const bool round_only = c->pt_words == nullptr;
  int rc = point_finish(c, c->pt_words, round_only ? 0 : c->pt_lo, c->pt_split, c->pt_hi, c->pt_nprot, &po);
  prof_collect(c);
  c->pt_valid = 0;
  if (rc) return rc;
  out->new_after = po.newd_after; out->added_after = po.added_after; out->removed = po.removed; out->added_before = po.added_before;
  out->err_bits = po.err;
  uint64_t newd_before = 0;
  if (!round_only) for (uint32_t ch = c->pt_lo; ch <= c->pt_split; ch++) newd_before += c->h_chist[ch];
  memset(accept, 0, sizeof(*accept));
  accept->new_distinct = newd_before + po.newd_after; accept->added = po.added_before + po.added_after; accept->removed = po.removed;
  accept->err_bits = po.err;
  return SHK_OK;
}

extern "C" int shk_denoise(shk_ctx *c, uint64_t *removed) {
  if (!c) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  uint64_t r = 0;
  int rc = table_sync(c);
  if (!rc) rc = denoise_round(c, &r);
  if (!rc) c->rounds_done++;
  if (removed) *removed = r;
  return finish(c, rc);
}

extern "C" int shk_stats(shk_ctx *c, shk_totals *o) {
  if (!c || !o) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  o->nelts = c->nelts; o->ndistinct = c->ndistinct; o->rounds_left = c->rounds_left; o->rounds_done = c->rounds_done;
  o->nslots = c->nslots; o->xnslots = c->xnslots; o->nblocks = c->nblocks; o->table_bytes = c->table_bytes;
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_FREE_PTR, c->fin[c->cur] + c->nregions, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  o->free_pointer = c->h_pinned[HP_FREE_PTR];
  return SHK_OK;
}

// quotient_filter_metadata, gqf.h:62-77 (field offsets checked against the compiled
// reference: see oracle/cqf_oracle.c orc_qf_header)
extern "C" int shk_header(shk_ctx *c, uint8_t out[128]) {
  if (!c || !out) return SHK_ERR_ARG;
  memset(out, 0, 128);
  uint64_t v;
#define PUT(off, val) do { v = (val); memcpy(out + (off), &v, 8); } while (0)
  PUT(0, c->table_bytes);
  memcpy(out + 8, &c->cfg.seed, 4);
  PUT(16, c->nslots); PUT(24, c->xnslots); PUT(32, (uint64_t)c->cfg.hb); PUT(40, 0);
  PUT(48, 8); PUT(56, 8);
  { unsigned __int128 range = (unsigned __int128)c->nslots << 8; memcpy(out + 64, &range, 16); }
  PUT(80, c->nblocks); PUT(88, c->nelts); PUT(96, c->ndistinct); PUT(104, 0);
  PUT(112, c->xnslots / (1ULL << 16) + 2);
#undef PUT
  return SHK_OK;
}

extern "C" int shk_export_blocks(shk_ctx *c, void *dst, uint64_t cap) {
  if (!c || !dst || cap < c->table_bytes) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(dst, c->tab[c->cur], c->table_bytes, hipMemcpyDeviceToHost, c->stream));
  { uint32_t bits = 0; if (fetch_err(c, &bits)) return SHK_ERR_HIP; if (bits) return map_err_bits(bits); }
  HIPCHK(hipStreamSynchronize(c->stream));
  return SHK_OK;
}

// device pointer and size of the live table (valid until the next call that rebuilds it): lets a caller move a
// shard's table to the GPU that stitches them without a trip through host memory
extern "C" int shk_table_ptr(shk_ctx *c, void **d_table, uint64_t *nbytes) {
  if (!c || !d_table || !nbytes) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  { uint32_t bits = 0; if (fetch_err(c, &bits)) return SHK_ERR_HIP; if (bits) return map_err_bits(bits); }   // (synchronises)
  *d_table = c->tab[c->cur]; *nbytes = c->table_bytes;
  return SHK_OK;
}

extern "C" int shk_export_cqf(shk_ctx *c, const char *path) {
  if (!c || !path) return SHK_ERR_ARG;
  std::vector<uint8_t> buf(c->table_bytes);
  int rc = shk_export_blocks(c, buf.data(), buf.size());
  if (rc) return rc;
  uint8_t hdr[128];
  shk_header(c, hdr);
  FILE *f = fopen(path, "wb+");
  if (!f) return SHK_ERR_IO;
  size_t ok = fwrite(hdr, 128, 1, f);
  ok += fwrite(buf.data(), buf.size(), 1, f);
  fclose(f);
  return ok == 2 ? SHK_OK : SHK_ERR_IO;
}

extern "C" int shk_import_blocks(shk_ctx *c, const void *src, uint64_t nbytes, uint64_t nelts, uint64_t ndistinct) {
  if (!c || !src || nbytes != c->table_bytes) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  c->rec_live = 0; c->table_stale = 0; c->spill_valid = 0;   // (the table is the truth again)
  c->foreign_marks = 1;         // (a .cqf written behind Contiger carries its traveled words; they are kept for the readers)
  HIPCHK(hipMemcpyAsync(c->tab[c->cur], src, nbytes, hipMemcpyHostToDevice, c->stream));
  { ProfScope ps(c, KP_MISC);
    hipLaunchKernelGGL(k_build_fin, dim3(c->nregions / 256 + 1), dim3(256), 0, c->stream, c->tab[c->cur], c->nslots,
                       c->nregions, c->fin[c->cur]); }
  HIPCHK(hipGetLastError());
  c->nelts = nelts; c->ndistinct = ndistinct;
  return finish(c, 0);
}

extern "C" int shk_import_cqf(shk_ctx *c, const char *path) {
  if (!c || !path) return SHK_ERR_ARG;
  FILE *f = fopen(path, "rb");
  if (!f) return SHK_ERR_IO;
  uint8_t hdr[128];
  if (fread(hdr, 128, 1, f) != 1) { fclose(f); return SHK_ERR_IO; }
  uint64_t size, nslots, key_bits, bps, nelts, nd;
  memcpy(&size, hdr + 0, 8); memcpy(&nslots, hdr + 16, 8); memcpy(&key_bits, hdr + 32, 8); memcpy(&bps, hdr + 56, 8);
  memcpy(&nelts, hdr + 88, 8); memcpy(&nd, hdr + 96, 8);
  if (bps != 8 || nslots != c->nslots || key_bits != c->cfg.hb || size != c->table_bytes || c->q_lo != 0) { fclose(f); return SHK_ERR_ARG; }
  std::vector<uint8_t> buf(size);
  if (fread(buf.data(), size, 1, f) != 1) { fclose(f); return SHK_ERR_IO; }
  fclose(f);
  return shk_import_blocks(c, buf.data(), size, nelts, nd);
}

extern "C" int shk_lookup(shk_ctx *c, const uint64_t *keys, uint64_t n, int on_device, int mode, uint64_t *counts,
                          uint8_t *was_traveled) {
  if (!c || (n && (!keys || !counts)) || mode < 0 || mode > 2) return SHK_ERR_ARG;
  if (n == 0) return SHK_OK;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  uint64_t *dk = nullptr, *dc = nullptr; uint8_t *dt = nullptr;
  if (mode == 1) c->foreign_marks = 1;
  if (on_device) { dk = (uint64_t *)keys; dc = counts; dt = was_traveled; }
  else {
    HIPCHK(hipMalloc((void **)&dk, n * 8)); HIPCHK(hipMalloc((void **)&dc, n * 8)); HIPCHK(hipMalloc((void **)&dt, n));
    HIPCHK(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, c->stream));
  }
  { ProfScope ps(c, KP_LOOKUP);
    hipLaunchKernelGGL(k_lookup, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, c->tab[c->cur], dk, n, c->q_lo,
                       c->nslots, mode, dc, dt); }
  HIPCHK(hipGetLastError());
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(counts, dc, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (was_traveled) HIPCHK(hipMemcpyAsync(was_traveled, dt, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hipFree(dk); hipFree(dc); hipFree(dt);
  }
  return finish(c, 0);
}

// ------------------------------------------------------------------ counted inserts, iterator dump, merge, stitch
// (insert_advance with count > 1 gqf.c:2024-2136; qf_iterator/qfi_* :2474-2601; qf_merge/qf_multi_merge :2614-2704)

// rebuild with the words of a counted insert; nothing is committed unless the pass is clean
static int merge_plain(shk_ctx *c, const uint64_t *words, MergeOut *o) {
  for (int attempt = 0; attempt < 2; attempt++) {
    int rc = merge_summary(c, words, 0, SHK_MAX_CHUNKS - 1, 0, o, false, true);
    if (rc) return rc;
    if (!c->big_image && (o->err & (SHK_E_OLD_EXTENT | SHK_E_NEW_EXTENT)) && !(o->err & SHK_E_TABLE_FULL)) { c->big_image = 1; continue; }
    break;
  }
  if (o->err) return SHK_OK;   // the caller looks at o->err
  return merge_write(c, words, 0, SHK_MAX_CHUNKS - 1, 0);
}

extern "C" int shk_insert_counted(shk_ctx *c, const uint64_t *keys, const uint64_t *counts, uint64_t n, int on_device,
                                  shk_batch_stats *stats) {
  if (!c || (n && (!keys || !counts))) return SHK_ERR_ARG;
  shk_batch_stats st;
  memset(&st, 0, sizeof(st));
  if (stats) *stats = st;
  if (n == 0) return SHK_OK;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  uint64_t *dk = nullptr, *dc = nullptr, *doff = nullptr;
  uint32_t *dnw = nullptr;
  int rc = SHK_OK;
  struct Free { uint64_t *&a, *&b, *&o; uint32_t *&w; bool own; ~Free() { if (own) { hipFree(a); hipFree(b); } hipFree(o); hipFree(w); } } fr{dk, dc, doff, dnw, !on_device};
  if (on_device) { dk = (uint64_t *)keys; dc = (uint64_t *)counts; }
  else {
    if (dmalloc(&dk, n) || dmalloc(&dc, n)) return SHK_ERR_HIP;
    HIPCHK(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dc, counts, n * 8, hipMemcpyHostToDevice, c->stream));
  }
  // pairs are inserted slice by slice (bounded by the key-word capacity; halved when one region would receive more
  // distinct new keys than its LDS hash holds); occurrences beyond `take` of one key go into further passes
  const uint64_t take = 1ULL << 22;
  const uint64_t key_lo = c->q_lo << 8, key_hi = (c->q_lo + c->nslots) << 8;
  uint64_t slice = n;
  { const uint64_t cap = c->cfg.max_batch_keys / 2 > 0 ? c->cfg.max_batch_keys / 2 : 1; if (slice > cap) slice = cap; }
  if (dmalloc(&doff, slice + 2) || dmalloc(&dnw, slice + 2)) return SHK_ERR_HIP;
  c->counted = 1;
  struct CountedScope { shk_ctx *c; ~CountedScope() { c->counted = 0; } } counted_scope{c};   // every exit, incl. HIPCHK's
  uint64_t done = 0;
  while (done < n && !rc) {
    const uint64_t m = n - done < slice ? n - done : slice;
    uint64_t skip = 0, maxc = 0;
    bool halve = false;
    do {
      HIPCHK(hipMemsetAsync(c->d_scalars + DS_MAX_COUNT, 0, 8, c->stream));
      const uint32_t nb = (uint32_t)((m + 255) / 256);
      { ProfScope ps(c, KP_MISC);
        hipLaunchKernelGGL(k_expand_counted<0>, dim3(nb), dim3(256), 0, c->stream, dk + done, dc + done, m, skip, take, c->cfg.hb, dnw,
                           (const uint64_t *)nullptr, (uint64_t *)nullptr, c->d_err, key_lo, key_hi, (unsigned long long *)(c->d_scalars + DS_MAX_COUNT)); }
      if (run_scan<uint32_t>(c, c, dnw, m, nullptr, doff)) { rc = SHK_ERR_HIP; break; }
      HIPCHK(hipMemcpyAsync(c->h_pinned + HP_TOTAL, doff + m, 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(c->h_pinned + HP_AUX, c->d_scalars + DS_MAX_COUNT, 8, hipMemcpyDeviceToHost, c->stream));
      uint32_t bits = 0;
      if (fetch_err(c, &bits)) { rc = SHK_ERR_HIP; break; }
      if (bits) { rc = map_err_bits(bits); break; }
      const uint64_t nwords = c->h_pinned[HP_TOTAL];
      maxc = c->h_pinned[HP_AUX];
      if (nwords > c->cfg.max_batch_keys) { halve = true; break; }
      if (nwords) {
        { ProfScope ps(c, KP_MISC);
          hipLaunchKernelGGL(k_expand_counted<1>, dim3(nb), dim3(256), 0, c->stream, dk + done, dc + done, m, skip, take, c->cfg.hb, dnw,
                             doff, c->d_words[0], c->d_err, key_lo, key_hi, (unsigned long long *)nullptr); }
        if (set_nwords(c, nwords)) return SHK_ERR_HIP;
        int dst = 0;
        rc = partition_stage(c, c, part_from_words(c, c->d_words[0], nwords), &dst);
        if (rc) break;
        c->pass_words = nwords;
        MergeOut o;
        rc = merge_plain(c, c->d_words[dst], &o);
        if (rc) break;
        if (o.err & SHK_E_HASH_FULL) { if (skip) { rc = SHK_ERR_REGION; break; } halve = true; break; }
        if (o.err) { rc = map_err_bits(o.err); break; }
        c->nelts += o.added; c->ndistinct += o.newd;
        st.kmers += o.added; st.new_distinct += o.newd;
      }
      skip += take;
    } while (maxc > skip);
    if (rc) break;
    if (halve) {
      if (slice == 1) { rc = SHK_ERR_REGION; break; }
      slice = (slice + 1) / 2;
      continue;
    }
    done += m;
  }
  c->counted = 0;
  if (stats) *stats = st;
  return finish(c, rc);
}

// (key, count) of every entry in the order of the reference's iterator. keys == NULL: only the number of entries.
// ref_iterator_end != 0: *n_out is where the reference's own iteration would END (see k_region_dump).
extern "C" int shk_dump(shk_ctx *c, uint64_t *keys, uint64_t *counts, uint64_t cap, int on_device, int ref_iterator_end,
                        uint64_t *n_out) {
  if (!c || !n_out || (keys && !counts)) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  ShkMergeArgs A;
  fill_args(c, &A, nullptr, 0, 0, 0);
  uint32_t *nper = c->d_over_list;                       // scratch of the spill scheme: [nregions + 1]
  uint64_t *offs = c->d_dump_offs;                       // [nregions + 2]
  unsigned long long *stop = (unsigned long long *)(c->d_scalars + DS_DUMP_STOP);
  const uint64_t *no_offs = nullptr;
  uint64_t *no_out = nullptr;
  c->spill_valid = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    { ProfScope ps(c, KP_MISC);
      SHK_FOR_REGION_SLICES(c, A, nblk) {
        if (c->big_image) hipLaunchKernelGGL((k_region_dump<0, SHK_IMG_BLOCKS_BIG>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, nper, no_offs, no_out, no_out, 0ULL, (unsigned long long *)nullptr);
        else hipLaunchKernelGGL((k_region_dump<0, SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, nper, no_offs, no_out, no_out, 0ULL, (unsigned long long *)nullptr);
      } }
    uint32_t bits = 0;
    if (fetch_err(c, &bits)) return SHK_ERR_HIP;
    if ((bits & SHK_E_OLD_EXTENT) && !c->big_image) { c->big_image = 1; c->last_err_bits = 0; continue; }
    if (bits) { prof_collect(c); return map_err_bits(bits); }
    break;
  }
  if (run_scan<uint32_t>(c, c, nper, c->nregions, nullptr, offs)) return SHK_ERR_HIP;
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_TOTAL, offs + c->nregions, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint64_t total = c->h_pinned[HP_TOTAL];
  *n_out = total;
  if (!keys && !ref_iterator_end) return finish(c, 0);
  const uint64_t m = keys ? (total < cap ? total : cap) : 0;
  uint64_t *dk = keys, *dc = counts;
  if (!on_device && m) { if (dmalloc(&dk, m) || dmalloc(&dc, m)) return SHK_ERR_HIP; }
  c->h_pinned[HP_AUX] = ~0ULL;
  HIPCHK(hipMemcpyAsync(stop, c->h_pinned + HP_AUX, 8, hipMemcpyHostToDevice, c->stream));
  if (total) {
    ProfScope ps(c, KP_MISC);
    unsigned long long *sp = ref_iterator_end ? stop : nullptr;
    SHK_FOR_REGION_SLICES(c, A, nblk) {
      if (c->big_image) hipLaunchKernelGGL((k_region_dump<1, SHK_IMG_BLOCKS_BIG>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, nper, (const uint64_t *)offs, m ? dk : no_out, m ? dc : no_out, m, sp);
      else hipLaunchKernelGGL((k_region_dump<1, SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, nper, (const uint64_t *)offs, m ? dk : no_out, m ? dc : no_out, m, sp);
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_AUX, stop, 8, hipMemcpyDeviceToHost, c->stream));
  if (!on_device && m) {
    HIPCHK(hipMemcpyAsync(keys, dk, m * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(counts, dc, m * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!on_device && m) { hipFree(dk); hipFree(dc); }
  if (ref_iterator_end && c->h_pinned[HP_AUX] < total) *n_out = c->h_pinned[HP_AUX];
  return finish(c, 0);
}

// Where the reference's iteration of the table A.tabA ends early: *stop = the first key it does not reach, ~0 when it reaches
// all. Only the regions whose image reaches behind nslots can hold such an entry.
static int launch_iter_end(shk_ctx *c, ShkMergeArgs A, unsigned long long *stop) {
  HIPCHK(hipMemsetAsync(stop, 0xFF, 8, c->stream));
  const uint64_t img_slots = c->big_image ? SHK_IMG_BLOCKS_BIG * 64 : SHK_IMG_SLOTS;
  A.r0 = c->nslots > img_slots ? (uint32_t)((c->nslots - img_slots) / SHK_REGION) : 0;
  const uint32_t nblk = c->nregions - A.r0;
  ProfScope ps(c, KP_JOIN);
  if (c->big_image) hipLaunchKernelGGL((k_region_iter_end<SHK_IMG_BLOCKS_BIG>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, stop);
  else hipLaunchKernelGGL((k_region_iter_end<SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, stop);
  return SHK_OK;
}

template <bool WRITE>
static void launch_rebuild2(shk_ctx *c, ShkMergeArgs &A, const ShkSrc2 &S, bool join) {
  constexpr int JM = WRITE ? SHK_JOIN_WRITE : SHK_JOIN_LENGTHS;
  unsigned long long *none = nullptr;
  SHK_FOR_REGION_SLICES(c, A, nblk) {
    if (join) {
      if (c->big_image) hipLaunchKernelGGL((k_region_join<JM, SHK_IMG_BLOCKS_BIG>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, S, none);
      else hipLaunchKernelGGL((k_region_join<JM, SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, S, none);
    } else {
      if (c->big_image) hipLaunchKernelGGL((k_region_merge2<WRITE, SHK_IMG_BLOCKS_BIG>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, S);
      else hipLaunchKernelGGL((k_region_merge2<WRITE, SHK_IMG_BLOCKS>), dim3(nblk), dim3(SHK_WAVE), 0, c->stream, A, S);
    }
  }
}

// The two-launch layout of a table walked from two: table 1 = (tab1, fin1), table 2 = S; the result replaces c's table.
// join = false (merge2_run): every entry of either, counts of equal keys added. join = true (intersect_run): the entries of
// table 1 whose key table 2 holds too, with table 1's counts; S.stop != null: those behind the reference's early end take no
// part. Nothing of c changes unless the lengths pass is clean.
static int rebuild2_run(shk_ctx *c, const uint8_t *tab1, const uint64_t *fin1, const ShkSrc2 &S, bool join, uint64_t *newd_out,
                        uint64_t *added_out) {
  ShkMergeArgs A;
  uint64_t newd = 0, added = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    fill_args(c, &A, nullptr, 0, 0, 0);
    A.tabA = tab1; A.finA = fin1;
    HIPCHK(hipMemsetAsync(c->d_counters, 0, (SHK_CNT_NOVER + 1) * 8, c->stream));
    c->spill_valid = 0;
    if (join && S.stop) { int rc = launch_iter_end(c, A, (unsigned long long *)S.stop); if (rc) return rc; }
    { ProfScope ps(c, KP_MERGE_SUM);
      launch_rebuild2<false>(c, A, S, join); }
    { ProfScope ps(c, KP_REGION_SCAN);
      const uint32_t ntiles = (c->nregions + SHK_RSCAN_TILE - 1) / SHK_RSCAN_TILE;
      hipLaunchKernelGGL(k_region_scan_a, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_summary, c->nregions, c->d_tile_a, c->d_tile_b);
      hipLaunchKernelGGL(k_region_scan_b, dim3(1), dim3(c->threads), 0, c->stream, c->d_tile_a, c->d_tile_b, ntiles, c->d_tile_f);
      hipLaunchKernelGGL(k_region_scan_c, dim3(ntiles), dim3(c->threads), 0, c->stream, c->d_summary, c->nregions, c->d_tile_f,
                         c->xnslots, (uint32_t)(c->big_image ? SHK_IMG_BLOCKS_BIG * 64 : SHK_IMG_SLOTS), c->fin[c->cur ^ 1], c->d_counters, c->d_err); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_pinned + HP_COUNTERS, c->d_counters, 4 * 8, hipMemcpyDeviceToHost, c->stream));
    uint32_t bits = 0;
    if (fetch_err(c, &bits)) return SHK_ERR_HIP;
    if (!c->big_image && (bits & (SHK_E_OLD_EXTENT | SHK_E_NEW_EXTENT)) && !(bits & SHK_E_TABLE_FULL)) { c->big_image = 1; c->last_err_bits = 0; continue; }
    if (bits) return map_err_bits(bits);
    newd = (c->h_pinned + HP_COUNTERS)[CNT_NEWD]; added = (c->h_pinned + HP_COUNTERS)[CNT_ADDED];
    break;
  }
  HIPCHK(hipMemsetAsync(c->tab[c->cur ^ 1], 0, c->table_bytes, c->stream));
  { ProfScope ps(c, KP_MERGE_WRITE);
    launch_rebuild2<true>(c, A, S, join); }
  HIPCHK(hipGetLastError());
  c->rec_live = 0; c->table_stale = 0;
  c->cur ^= 1;
  c->foreign_marks = 0;
  *newd_out = newd; *added_out = added;
  return SHK_OK;
}

// dst := canonical table of (dst's entries + the second source's entries), counts of equal keys added
static int merge2_run(shk_ctx *c, const ShkSrc2 &S, uint64_t *newd_out, uint64_t *added_out) {
  { int rc = table_sync(c); if (rc) return rc; }
  return rebuild2_run(c, c->tab[c->cur], c->fin[c->cur], S, false, newd_out, added_out);
}
// dst := canonical table of { (key, count_b) : key in a and in b }; dst's own content is not read (nor its placement run)
static int intersect_run(shk_ctx *dst, const shk_ctx *b, const ShkSrc2 &a, uint64_t *newd_out, uint64_t *added_out) {
  return rebuild2_run(dst, b->tab[b->cur], b->fin[b->cur], a, true, newd_out, added_out);
}

extern "C" int shk_merge(shk_ctx *dst, shk_ctx *src, shk_batch_stats *stats) {
  if (!dst || !src || dst == src) return SHK_ERR_ARG;
  if (dst->dev != src->dev || dst->cfg.qb != src->cfg.qb || dst->cfg.hb != src->cfg.hb || dst->q_lo != src->q_lo || dst->nslots != src->nslots)
    return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(dst->dev));
  { int rc = table_sync(src); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(src->stream));   // the source's table must be at rest
  ShkSrc2 S;
  memset(&S, 0, sizeof(S));
  S.tab[0] = src->tab[src->cur]; S.fin[0] = src->fin[src->cur]; S.nblocks = src->nblocks; S.regions_per_src = dst->nregions; S.nsrc = 1;
  uint64_t newd = 0, added = 0;
  int rc = merge2_run(dst, S, &newd, &added);
  if (!rc) {
    dst->nelts += added; dst->ndistinct += newd;
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->kmers = added; stats->new_distinct = newd; }
  }
  return finish(dst, rc);
}

extern "C" int shk_multi_merge(shk_ctx *dst, shk_ctx *const *srcs, uint32_t n, shk_batch_stats *stats) {
  if (!dst || (n && !srcs)) return SHK_ERR_ARG;
  shk_batch_stats tot;
  memset(&tot, 0, sizeof(tot));
  for (uint32_t i = 0; i < n; i++) {
    shk_batch_stats st;
    int rc = shk_merge(dst, srcs[i], &st);
    if (rc) return rc;
    tot.kmers += st.kmers; tot.new_distinct += st.new_distinct;
  }
  if (stats) *stats = tot;
  return SHK_OK;
}

// ------------------------------------------------------------------ analytics on resident tables: spectrum, inner product, intersect
// (qf_inner_product gqf.c:2707-2733, qf_intersect :2736-2757, qf_magnitude :2760-2763; the spectrum has no counterpart)

static bool same_geometry(const shk_ctx *x, const shk_ctx *y) {
  return x->dev == y->dev && x->cfg.qb == y->cfg.qb && x->cfg.hb == y->cfg.hb && x->q_lo == y->q_lo && x->nslots == y->nslots;
}
// the grid of the grid-stride analytics kernels: at most every wave slot of the device once (256 CUs x 32 one-wave workgroups
// with the default hash_groups), so that a workgroup's one flush pays for many regions
static uint32_t analytics_grid(const shk_ctx *c) {
  const uint64_t cap = 4ull * c->hash_groups;
  return (uint32_t)(c->nregions < cap ? c->nregions : cap);
}

extern "C" int shk_spectrum(shk_ctx *c, uint64_t *hist, uint32_t nbins, int on_device, shk_spectrum_totals *out) {
  if (!c || (nbins && !hist) || (!nbins && !out)) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  ShkMergeArgs A;
  fill_args(c, &A, nullptr, 0, 0, 0);
  unsigned long long *dh = (unsigned long long *)hist, *dt = (unsigned long long *)(c->d_scalars + DS_SPECTRUM);
  if (nbins && !on_device) { uint64_t *p = nullptr; if (dmalloc(&p, nbins)) return SHK_ERR_HIP; dh = (unsigned long long *)p; }
  struct Free { void *p; ~Free() { if (p) hipFree(p); } } fr{(nbins && !on_device) ? dh : nullptr};
  if (!nbins) dh = nullptr;
  const uint32_t grid = analytics_grid(c);
  for (int attempt = 0; attempt < 2; attempt++) {
    if (nbins) HIPCHK(hipMemsetAsync(dh, 0, (uint64_t)nbins * 8, c->stream));
    HIPCHK(hipMemsetAsync(dt, 0, SHK_SPEC_WORDS * 8, c->stream));
    { ProfScope ps(c, KP_SPECTRUM);
      if (c->big_image) hipLaunchKernelGGL((k_region_spectrum<SHK_IMG_BLOCKS_BIG>), dim3(grid), dim3(SHK_WAVE), 0, c->stream, A, dh, nbins, dt);
      else hipLaunchKernelGGL((k_region_spectrum<SHK_IMG_BLOCKS>), dim3(grid), dim3(SHK_WAVE), 0, c->stream, A, dh, nbins, dt); }
    HIPCHK(hipGetLastError());
    uint32_t bits = 0;
    if (fetch_err(c, &bits)) return SHK_ERR_HIP;
    if ((bits & SHK_E_OLD_EXTENT) && !c->big_image) { c->big_image = 1; c->last_err_bits = 0; continue; }
    if (bits) { prof_collect(c); return map_err_bits(bits); }
    break;
  }
  HIPCHK(hipMemcpyAsync(c->h_pinned + HP_SPECTRUM, dt, SHK_SPEC_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
  if (nbins && !on_device) HIPCHK(hipMemcpyAsync(hist, dh, (uint64_t)nbins * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (out) {
    const uint64_t *t = c->h_pinned + HP_SPECTRUM;
    out->distinct = t[SHK_SPEC_DISTINCT]; out->total = t[SHK_SPEC_TOTAL]; out->sumsq = t[SHK_SPEC_SUMSQ]; out->max_count = t[SHK_SPEC_MAX];
  }
  return finish(c, 0);
}

// both operands' tables written and at rest (the join runs on the stream of the context that launches it)
static int join_operands(shk_ctx *a, shk_ctx *b) {
  { int rc = table_sync(a); if (rc) return rc; }
  if (b != a) { int rc = table_sync(b); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(a->stream));
  if (b != a) HIPCHK(hipStreamSynchronize(b->stream));
  return SHK_OK;
}
// a as the looked-up operand of a join launched by `run`
static ShkSrc2 join_source(const shk_ctx *a, shk_ctx *run, int ref_iterator_end) {
  ShkSrc2 S;
  memset(&S, 0, sizeof(S));
  S.tab[0] = a->tab[a->cur]; S.fin[0] = a->fin[a->cur]; S.nblocks = a->nblocks; S.regions_per_src = a->nregions; S.nsrc = 1;
  S.stop = ref_iterator_end ? (const unsigned long long *)(run->d_scalars + DS_JOIN_STOP) : nullptr;
  return S;
}

extern "C" int shk_inner_product(shk_ctx *a, shk_ctx *b, int ref_iterator_end, uint64_t *out) {
  if (!a || !b || !out || !same_geometry(a, b)) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(a->dev));
  { int rc = join_operands(a, b); if (rc) return rc; }
  const ShkSrc2 S = join_source(a, a, ref_iterator_end);
  unsigned long long *acc = (unsigned long long *)(a->d_scalars + DS_JOIN_ACC);
  const uint32_t grid = analytics_grid(a);
  for (int attempt = 0; attempt < 2; attempt++) {
    ShkMergeArgs A;
    fill_args(a, &A, nullptr, 0, 0, 0);
    A.tabA = b->tab[b->cur]; A.finA = b->fin[b->cur];     // the iterated operand
    HIPCHK(hipMemsetAsync(acc, 0, 8, a->stream));
    if (S.stop) { int rc = launch_iter_end(a, A, (unsigned long long *)S.stop); if (rc) return rc; }
    { ProfScope ps(a, KP_JOIN);
      if (a->big_image) hipLaunchKernelGGL((k_region_join<SHK_JOIN_DOT, SHK_IMG_BLOCKS_BIG>), dim3(grid), dim3(SHK_WAVE), 0, a->stream, A, S, acc);
      else hipLaunchKernelGGL((k_region_join<SHK_JOIN_DOT, SHK_IMG_BLOCKS>), dim3(grid), dim3(SHK_WAVE), 0, a->stream, A, S, acc); }
    HIPCHK(hipGetLastError());
    uint32_t bits = 0;
    if (fetch_err(a, &bits)) return SHK_ERR_HIP;
    if ((bits & SHK_E_OLD_EXTENT) && !a->big_image) { a->big_image = 1; a->last_err_bits = 0; continue; }
    if (bits) { prof_collect(a); return map_err_bits(bits); }
    break;
  }
  HIPCHK(hipMemcpyAsync(a->h_pinned + HP_AUX, acc, 8, hipMemcpyDeviceToHost, a->stream));
  HIPCHK(hipStreamSynchronize(a->stream));
  *out = a->h_pinned[HP_AUX];
  return finish(a, 0);
}

extern "C" int shk_magnitude(shk_ctx *c, int ref_iterator_end, uint64_t *out) {
  if (!c || !out) return SHK_ERR_ARG;
  uint64_t ip = 0;
  int rc = shk_inner_product(c, c, ref_iterator_end, &ip);
  if (rc) return rc;
  *out = (uint64_t)sqrt((double)ip);
  return SHK_OK;
}

extern "C" int shk_intersect(shk_ctx *dst, shk_ctx *a, shk_ctx *b, int ref_iterator_end, shk_batch_stats *stats) {
  if (!dst || !a || !b || dst == a || dst == b || !same_geometry(dst, a) || !same_geometry(dst, b)) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(dst->dev));
  { int rc = join_operands(a, b); if (rc) return rc; }
  uint64_t newd = 0, added = 0;
  int rc = intersect_run(dst, b, join_source(a, dst, ref_iterator_end), &newd, &added);
  if (!rc) {
    dst->nelts = added; dst->ndistinct = newd;
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->kmers = added; stats->new_distinct = newd; }
  }
  return finish(dst, rc);
}

// The whole filter from its quotient-range shards: shard s (a table in the layout shk_export_blocks gives for a context
// with num_shards = nshards, shard_index = s: its nslots / nshards quotients plus its own overflow tail) supplies the
// runs of its quotients; they are laid out again in the single table, where a cluster may now run across a shard border.
extern "C" int shk_import_shards(shk_ctx *c, const void *const *shard_blocks, const uint64_t *shard_bytes, uint32_t nshards,
                                 int on_device, uint64_t nelts, uint64_t ndistinct) {
  if (!c || !shard_blocks || !shard_bytes || nshards == 0 || nshards > SHK_MAX_SRC || (nshards & (nshards - 1))) return SHK_ERR_ARG;
  if (c->cfg.num_shards > 1 || c->q_lo != 0) return SHK_ERR_ARG;
  const uint64_t s_nslots = c->nslots / nshards;
  if (s_nslots < SHK_REGION || s_nslots % SHK_REGION) return SHK_ERR_ARG;
  const uint64_t s_xnslots = s_nslots + (uint64_t)(10 * sqrt((double)c->g_nslots));
  const uint64_t s_nblocks = (s_xnslots + 63) / 64, s_bytes = s_nblocks * SHK_BLOCK_BYTES;
  const uint32_t s_nregions = (uint32_t)(s_nslots / SHK_REGION);
  for (uint32_t s = 0; s < nshards; s++) if (shard_bytes[s] != s_bytes || !shard_blocks[s]) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  // start from an empty table
  c->rec_live = 0; c->table_stale = 0; c->spill_valid = 0;
  HIPCHK(hipMemsetAsync(c->tab[c->cur], 0, c->table_bytes + SHK_SLACK, c->stream));
  HIPCHK(hipMemsetAsync(c->fin[c->cur], 0, ((uint64_t)c->nregions + 2) * 8, c->stream));
  c->nelts = 0; c->ndistinct = 0;
  ShkSrc2 S;
  memset(&S, 0, sizeof(S));
  S.nblocks = s_nblocks; S.regions_per_src = s_nregions; S.nsrc = nshards;
  std::vector<uint8_t *> own;
  std::vector<uint64_t *> fins;
  int rc = SHK_OK;
  for (uint32_t s = 0; s < nshards && !rc; s++) {
    uint8_t *dt = (uint8_t *)shard_blocks[s];
    if (!on_device) {
      if (dmalloc(&dt, s_bytes)) { rc = SHK_ERR_HIP; break; }
      own.push_back(dt);
      if (hipMemcpyAsync(dt, shard_blocks[s], s_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = SHK_ERR_HIP; break; }
      if (hipMemsetAsync(dt + s_bytes, 0, SHK_SLACK, c->stream) != hipSuccess) { rc = SHK_ERR_HIP; break; }
    }
    uint64_t *df = nullptr;
    if (dmalloc(&df, (uint64_t)s_nregions + 2)) { rc = SHK_ERR_HIP; break; }
    fins.push_back(df);
    hipLaunchKernelGGL(k_build_fin, dim3(s_nregions / 256 + 1), dim3(256), 0, c->stream, dt, s_nslots, s_nregions, df);
    S.tab[s] = dt; S.fin[s] = df;
  }
  uint64_t newd = 0, added = 0;
  if (!rc) rc = merge2_run(c, S, &newd, &added);
  hipStreamSynchronize(c->stream);
  for (auto p : own) hipFree(p);
  for (auto p : fins) hipFree(p);
  if (!rc) { c->nelts = nelts ? nelts : added; c->ndistinct = ndistinct ? ndistinct : newd; }
  // (the shards' tables are laid out again by the merge, which writes no traveled word: nothing foreign comes in here)
  return finish(c, rc);
}

// ------------------------------------------------------------------ Contiger: seeds (processDataChunk, contig_assembly.cpp:1839-1884)
extern "C" int shk_select_seeds(shk_ctx *c, const void *text, int text_on_device, uint64_t text_bytes, const uint64_t *chunk_off,
                                const uint64_t *chunk_len, uint32_t nchunks, uint32_t k, uint64_t count_min, uint64_t count_max,
                                int use_traveled, char *out_seeds, uint32_t *out_counts, uint32_t cap, uint32_t *n_out) {
  if (!c || !text || !out_seeds || !out_counts || !n_out || nchunks == 0 || nchunks > SHK_MAX_CHUNKS) return SHK_ERR_ARG;
  if (k < 2 || k > SHK_WALK_MAX_K) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc = table_sync(c); if (rc) return rc; }
  const uint8_t *dtext;
  uint64_t nreads;
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  int rc = parse_stage(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, &dtext, &nreads);
  if (rc) return finish(c, rc);
  *n_out = 0;
  if (nreads == 0) return finish(c, 0);
  struct Scratch { char *s = nullptr; uint32_t *c = nullptr; ~Scratch() { hipFree(s); hipFree(c); } } w;
  if (dmalloc(&w.s, nreads * k) || dmalloc(&w.c, nreads)) return SHK_ERR_HIP;
  char *ds = w.s; uint32_t *dc = w.c;
  if (use_traveled) c->foreign_marks = 1;
  { ProfScope ps(c, KP_WALK);
    hipLaunchKernelGGL(k_select_seeds, dim3((uint32_t)((nreads + 255) / 256)), dim3(256), 0, c->stream, c->tab[c->cur], c->q_lo, c->nslots,
                       c->cfg.hb, dtext, c->d_rd_start, c->d_rd_end, (uint64_t)0, nreads, k, count_min, count_max, use_traveled ? 1 : 2, ds, dc); }
  HIPCHK(hipGetLastError());
  std::vector<char> hs(nreads * k);
  std::vector<uint32_t> hc(nreads);
  HIPCHK(hipMemcpyAsync(hs.data(), ds, nreads * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hc.data(), dc, nreads * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  uint32_t n = 0;
  for (uint64_t r = 0; r < nreads; r++)
    if (hc[r]) {                       // 0 = no seed from this read
      if (n >= cap) return finish(c, SHK_ERR_BATCH);
      memcpy(out_seeds + (size_t)n * k, &hs[r * k], k);
      out_counts[n++] = hc[r];
    }
  *n_out = n;
  return finish(c, 0);
}

// ------------------------------------------------------------------ Contiger: unitig extension (first slice)
// The Contiger kernels that hold k-mers are instantiated for W = 2, 4, 6 words per k-mer (shk_walk_words(k)): the
// statement runs with the constexpr KW set to the instantiation's W
#define SHK_BY_WORDS(w, ...) do {                                  \
    switch (w) {                                                   \
      case 2: { constexpr int KW = 2; __VA_ARGS__; } break;        \
      case 4: { constexpr int KW = 4; __VA_ARGS__; } break;        \
      default: { constexpr int KW = 6; __VA_ARGS__; } break;       \
    }                                                              \
  } while (0)

extern "C" int shk_extend_forward(shk_ctx *c, const char *cur_kmers, const char *first_kmers, uint32_t n, uint32_t k,
                                  uint64_t abundance_min, int mark_traveled, uint32_t max_ext, char *out_bases,
                                  uint32_t *out_counts, uint32_t *out_n, uint8_t *out_stop, uint8_t *out_branch,
                                  uint32_t *out_ncount) {
  if (!c || (n && (!cur_kmers || !first_kmers || !out_bases || !out_counts || !out_n || !out_stop))) return SHK_ERR_ARG;
  if (k < 2 || k > SHK_WALK_MAX_K || max_ext == 0) return SHK_ERR_ARG;
  if (n == 0) return SHK_OK;
  HIPCHK(hipSetDevice(c->dev));
  { int rc_ = table_sync(c); if (rc_) return rc_; }
  // scratch of this call, released on every way out
  struct Scratch {
    char *dk = nullptr, *df = nullptr, *db = nullptr;
    uint32_t *dc = nullptr, *dn = nullptr, *dnc = nullptr;
    uint8_t *ds = nullptr, *dbr = nullptr;
    ~Scratch() { hipFree(dk); hipFree(df); hipFree(db); hipFree(dc); hipFree(dn); hipFree(dnc); hipFree(ds); hipFree(dbr); }
  } w;
  const size_t nk = (size_t)n * k, ne = (size_t)n * max_ext;
  if (dmalloc(&w.dk, nk) || dmalloc(&w.df, nk) || dmalloc(&w.db, ne) || dmalloc(&w.dc, ne) || dmalloc(&w.dn, (size_t)n) || dmalloc(&w.ds, (size_t)n) ||
      dmalloc(&w.dbr, (size_t)n) || dmalloc(&w.dnc, (size_t)n * 8))
    return SHK_ERR_HIP;
  HIPCHK(hipMemcpyAsync(w.dk, cur_kmers, nk, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(w.df, first_kmers, nk, hipMemcpyHostToDevice, c->stream));
  if (mark_traveled) c->foreign_marks = 1;
  { ProfScope ps(c, KP_WALK);
    char *dk = w.dk, *df = w.df, *db = w.db;          // (plain pointers: the launch must not capture the owning struct)
    uint32_t *dc = w.dc, *dn = w.dn, *dnc = w.dnc;
    uint8_t *ds = w.ds, *dbr = w.dbr;
    SHK_BY_WORDS(shk_walk_words(k),
      hipLaunchKernelGGL(k_extend_forward<KW>, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->tab[c->cur], c->q_lo, c->nslots,
                         c->cfg.hb, dk, df, n, k, abundance_min, mark_traveled ? 1 : 2, max_ext, db, dc, dn, ds, dbr, dnc)); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_bases, w.db, ne, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(out_counts, w.dc, ne * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(out_n, w.dn, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(out_stop, w.ds, n, hipMemcpyDeviceToHost, c->stream));
  if (out_branch) HIPCHK(hipMemcpyAsync(out_branch, w.dbr, n, hipMemcpyDeviceToHost, c->stream));
  if (out_ncount) HIPCHK(hipMemcpyAsync(out_ncount, w.dnc, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return finish(c, 0);
}

// median() of base/Utility.cpp:27-40 stored into Contig::median_abundance, an int (truncation)
static int walk_median(std::vector<int> &v) {
  if (v.empty()) return 0;
  if (v.size() == 1) return v[0];
  std::sort(v.begin(), v.end());
  const size_t t = v.size() / 2;
  return v.size() % 2 == 0 ? (int)((v[t - 1] + v[t]) / 2.0) : v[t];
}

// One maximal unitig per seed k-mer: extend forward, reverse-complement, extend forward again -- the two
// get_unitig_forward calls of processDataChunk (contig_assembly.cpp:1886-1904) in the case where no
// other unitig is met. seeds: n * k upper-case bases; seed_counts: their filter counts (Contig(kmer, count)).
extern "C" int shk_unitigs_from_seeds(shk_ctx *c, const char *seeds, const uint32_t *seed_counts, uint32_t n, uint32_t k,
                                      uint64_t abundance_min, uint32_t max_len, char *out_seq, uint32_t *out_len,
                                      int32_t *out_median, uint8_t *out_stop) {
  if (!c || (n && (!seeds || !seed_counts || !out_seq || !out_len || !out_median || !out_stop))) return SHK_ERR_ARG;
  if (k < 2 || k > SHK_WALK_MAX_K || max_len < k + 1) return SHK_ERR_ARG;
  const uint32_t max_ext = max_len - k;
  std::vector<std::string> seq(n);
  std::vector<int> med(n);
  for (uint32_t i = 0; i < n; i++) { seq[i].assign(seeds + (size_t)i * k, k); med[i] = (int)seed_counts[i]; }
  std::vector<char> cur((size_t)n * k), first((size_t)n * k), ext((size_t)n * max_ext);
  std::vector<uint32_t> cnt((size_t)n * max_ext), en(n);
  std::vector<uint8_t> st(n);
  for (int pass = 0; pass < 2; pass++) {
    for (uint32_t i = 0; i < n; i++) {
      memcpy(&first[(size_t)i * k], seq[i].data(), k);
      memcpy(&cur[(size_t)i * k], seq[i].data() + seq[i].size() - k, k);
    }
    int rc = shk_extend_forward(c, cur.data(), first.data(), n, k, abundance_min, 0, max_ext, ext.data(), cnt.data(), en.data(), st.data(), nullptr, nullptr);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) {
      // abundances start as (length - K + 1) copies of the contig's current median (contig_assembly.cpp:3049)
      std::vector<int> ab(seq[i].size() - k + 1, med[i]);
      uint32_t take = en[i];
      if (seq[i].size() + take > max_len) { take = max_len - (uint32_t)seq[i].size(); st[i] = SHK_STOP_BUFFER; }
      for (uint32_t j = 0; j < take; j++) ab.push_back((int)cnt[(size_t)i * max_ext + j]);
      seq[i].append(&ext[(size_t)i * max_ext], take);
      med[i] = walk_median(ab);
      out_stop[(size_t)i * 2 + pass] = st[i];
      if (pass == 0) {   // DNAString::RC
        std::string r(seq[i].rbegin(), seq[i].rend());
        for (auto &ch : r) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
        seq[i].swap(r);
      }
    }
  }
  for (uint32_t i = 0; i < n; i++) {
    memcpy(out_seq + (size_t)i * max_len, seq[i].data(), seq[i].size());
    out_len[i] = (uint32_t)seq[i].size();
    out_median[i] = med[i];
  }
  return SHK_OK;
}

// ------------------------------------------------------------------ Contiger: the unitig set on the device
// (unitig_kernels.hip; the reference's find_unitigs_mt_master/worker, check_unitig, track_kmer_worker,
// build_graph_worker and the writer, src/contig_assembly.cpp:2034-2269, 935-1084, 600-629)
template <typename T> static int ug_grow(T **p, uint64_t old_n, uint64_t new_n, hipStream_t st, bool zero_new) {
  T *q = nullptr;
  if (dmalloc(&q, new_n)) return SHK_ERR_HIP;
  if (zero_new) HIPCHK(hipMemsetAsync(q, 0, new_n * sizeof(T), st));
  if (*p && old_n) HIPCHK(hipMemcpyAsync(q, *p, old_n * sizeof(T), hipMemcpyDeviceToDevice, st));
  if (*p) { HIPCHK(hipStreamSynchronize(st)); hipFree(*p); }
  *p = q;
  return SHK_OK;
}

struct shk_unitig_set {
  shk_ctx *c = nullptr;
  ShkUG G;
  uint32_t cap = 0, mcap = 0, ccap = 0, lcap = 0;     // contigs, map slots, circle slots, list entries
  uint32_t *d_list[2] = {nullptr, nullptr};
  uint32_t *d_scal = nullptr;                          // [0] ncontigs [1] next_n [2] flags [3] nactive (seeds from reads)
  unsigned long long *d_stats = nullptr;
  uint32_t *h_scal = nullptr;                          // pinned mirror (4 u32 + 4 u64)
  char *d_seeds = nullptr; uint32_t *d_counts = nullptr; uint64_t seeds_cap = 0;
  uint32_t ncontigs = 1;                               // next free id (the reference starts with contigs.resize(1))
  uint32_t k = 0, max_len = 0;
  uint32_t W = 0;                                      // words per packed k-mer (shk_walk_words(k)): planes per k-mer array and map key
  uint64_t amin = 0;
  shk_unitig_stats st;
  shk_unitig_set() { memset(&st, 0, sizeof(st)); memset(&G, 0, sizeof(G)); }
};
extern "C" shk_unitig_set *shk_unitig_set_new(void) { return new shk_unitig_set(); }
// every device array of a set's ShkUG (unallocated planes are null)
static void ug_free_arrays(ShkUG &G) {
  for (int j = 0; j < SHK_KM_WMAX; j++) { hipFree(G.first[j]); hipFree(G.cur[j]); hipFree(G.rc[j]); hipFree(G.mk[j]); }
  hipFree(G.fh); hipFree(G.rh); hipFree(G.hmin); hipFree(G.len); hipFree(G.l1); hipFree(G.cnt0); hipFree(G.state); hipFree(G.kind);
  hipFree(G.stop); hipFree(G.mv); hipFree(G.ck); hipFree(G.cv);
}
extern "C" void shk_unitig_set_free(shk_unitig_set *u) {
  if (!u) return;
  if (u->c) {
    hipSetDevice(u->c->dev);
    hipStreamSynchronize(u->c->stream);
    ug_free_arrays(u->G);
    hipFree(u->d_list[0]); hipFree(u->d_list[1]); hipFree(u->d_scal); hipFree(u->d_stats); hipFree(u->d_seeds); hipFree(u->d_counts);
    if (u->h_scal) hipHostFree(u->h_scal);
  }
  delete u;
}

// capacities for `ncontigs_after` contig ids and `nlist` list entries
static int ug_reserve(shk_unitig_set *u, uint64_t ncontigs_after, uint64_t nlist) {
  shk_ctx *c = u->c;
  ShkUG &G = u->G;
  if (ncontigs_after + 1 > u->cap) {
    uint64_t nc = u->cap ? u->cap : 1024;
    while (nc < ncontigs_after + 1) nc *= 2;
    if (nc > 0x7FFFFFF0ull) return SHK_ERR_BATCH;
    const uint64_t o = u->cap;
    for (uint32_t j = 0; j < u->W; j++)
      if (ug_grow(&G.first[j], o, nc, c->stream, false) || ug_grow(&G.cur[j], o, nc, c->stream, false) || ug_grow(&G.rc[j], o, nc, c->stream, false))
        return SHK_ERR_HIP;
    if (ug_grow(&G.fh, o, nc, c->stream, false) || ug_grow(&G.rh, o, nc, c->stream, false) || ug_grow(&G.hmin, o, nc, c->stream, false) ||
        ug_grow(&G.len, o, nc, c->stream, true) || ug_grow(&G.l1, o, nc, c->stream, true) || ug_grow(&G.cnt0, o, nc, c->stream, true) ||
        ug_grow(&G.state, o, nc, c->stream, true) || ug_grow(&G.kind, o, nc, c->stream, true) || ug_grow(&G.stop, o, nc, c->stream, true))
      return SHK_ERR_HIP;
    u->cap = (uint32_t)nc; G.cap = (uint32_t)nc;
  }
  if (nlist > u->lcap) {
    uint64_t nl = u->lcap ? u->lcap : 1024;
    while (nl < nlist) nl *= 2;
    if (ug_grow(&u->d_list[0], u->lcap, nl, c->stream, false) || ug_grow(&u->d_list[1], u->lcap, nl, c->stream, false)) return SHK_ERR_HIP;
    u->lcap = (uint32_t)nl;
  }
  // every contig owns at most two keys; the table stays at most a quarter full
  if (ncontigs_after * 8 > u->mcap) {
    uint64_t nm = u->mcap ? u->mcap : 4096;
    while (nm < ncontigs_after * 8) nm *= 2;
    if (nm > 0x80000000ull) return SHK_ERR_BATCH;
    const ShkUG old = G;                      // (its mk / mv: the table being replaced)
    const uint32_t ocap = u->mcap;
    for (int j = 0; j < SHK_KM_WMAX; j++) G.mk[j] = nullptr;
    G.mv = nullptr;
    // (a failure here leaves the old table with `old` and the new planes in G: both released below / by the caller)
    int rc = dmalloc(&G.mv, nm) ? SHK_ERR_HIP : SHK_OK;
    for (uint32_t j = 0; j < u->W && !rc; j++) if (dmalloc(&G.mk[j], nm)) rc = SHK_ERR_HIP;
    if (!rc && hipMemsetAsync(G.mv, 0, nm * 4, c->stream) != hipSuccess) rc = SHK_ERR_HIP;
    if (!rc) {
      G.mmask = (uint32_t)(nm - 1); u->mcap = (uint32_t)nm;
      if (ocap) {
        SHK_BY_WORDS(u->W, hipLaunchKernelGGL(k_ug_rehash<KW>, dim3((ocap + 255) / 256), dim3(256), 0, c->stream, G, old, ocap));
        if (hipStreamSynchronize(c->stream) != hipSuccess) rc = SHK_ERR_HIP;
      }
    }
    for (int j = 0; j < SHK_KM_WMAX; j++) hipFree(old.mk[j]);
    hipFree(old.mv);
    if (rc) return rc;
  }
  if (!u->ccap) {
    const uint64_t ncs = 1 << 16;
    if (dmalloc(&G.ck, ncs) || dmalloc(&G.cv, ncs)) return SHK_ERR_HIP;
    HIPCHK(hipMemsetAsync(G.cv, 0, ncs * 4, c->stream));
    G.cmask = (uint32_t)(ncs - 1); u->ccap = (uint32_t)ncs;
  }
  return SHK_OK;
}

static int ug_bind(shk_unitig_set *u, shk_ctx *c, uint32_t k, uint64_t amin, uint32_t max_len) {
  { int rc = table_sync(c); if (rc) return rc; }
  if (u->c) {
    if (u->c != c || u->k != k || u->amin != amin || u->max_len != max_len) return SHK_ERR_ARG;   // one filter, one set of rules
    return SHK_OK;
  }
  // bound only once everything is allocated: a set whose first bind failed stays unbound (and can be bound again)
  uint32_t *d_scal = nullptr, *h_scal = nullptr;
  unsigned long long *d_stats = nullptr;
  if (dmalloc(&d_scal, 16) || dmalloc(&d_stats, 8) || hipHostMalloc((void **)&h_scal, 64, hipHostMallocDefault) != hipSuccess ||
      hipMemsetAsync(d_scal, 0, 16 * 4, c->stream) != hipSuccess || hipMemsetAsync(d_stats, 0, 8 * 8, c->stream) != hipSuccess) {
    hipFree(d_scal); hipFree(d_stats); if (h_scal) hipHostFree(h_scal);
    return SHK_ERR_HIP;
  }
  u->c = c; u->k = k; u->amin = amin; u->max_len = max_len; u->W = shk_walk_words(k);
  u->d_scal = d_scal; u->d_stats = d_stats; u->h_scal = h_scal;
  u->G.ncontigs = u->d_scal; u->G.next_n = u->d_scal + 1; u->G.flags = u->d_scal + 2; u->G.stats = u->d_stats;
  int rc = ug_reserve(u, 1024, 1024);
  if (rc) {           // release what the half-made set holds and unbind it
    hipStreamSynchronize(c->stream);
    ug_free_arrays(u->G);
    hipFree(u->d_list[0]); hipFree(u->d_list[1]); hipFree(u->d_scal); hipFree(u->d_stats); hipHostFree(u->h_scal);
    memset(&u->G, 0, sizeof(u->G));
    u->d_list[0] = u->d_list[1] = nullptr; u->d_scal = nullptr; u->d_stats = nullptr; u->h_scal = nullptr;
    u->cap = u->mcap = u->ccap = u->lcap = 0;
    u->c = nullptr; u->W = 0;
  }
  return rc;
}

// rounds of k_ug_walk until no contig is open; d_list[0] holds `nactive` ids
static int ug_run(shk_unitig_set *u, uint32_t nactive, int mark) {
  shk_ctx *c = u->c;
  { int rc = table_sync(c); if (rc) return rc; }
  if (mark) c->foreign_marks = 1;
  // Extensions per contig and launch. A launch lasts as long as its longest walk while the neighbours that the short
  // ones queued wait for the next one: with many contigs open, short launches keep the frontier moving (2 M unitigs of a
  // 100x C. elegans graph, 126 M extensions: 1.25 s at 2048 steps per launch, 0.92 at 512, 0.56 at 128, 0.49 at 64, 0.47 at
  // 32, 0.48 at 16 with 2675 launches; longer launches while fewer than 4096 / 64 contigs are open: 0.73 / 0.55). The price
  // is paid by a graph that is one long unitig: a launch and its synchronisation (~70 us) per 64 extensions (~100 us)
  uint32_t fixed = 0;
  if (const char *e = getenv("SHK_WALK_STEP")) { int v = atoi(e); if (v > 0) fixed = (uint32_t)v; }   // tests: force continuations
  int cur = 0;
  while (nactive) {
    const uint32_t step = fixed ? fixed : 64u;
    // a contig may queue up to 7 neighbours; every open contig may come back once
    int rc = ug_reserve(u, (uint64_t)u->ncontigs + 8ull * nactive + 16, 8ull * nactive + 16);
    if (rc) return rc;
    u->h_scal[0] = u->ncontigs; u->h_scal[1] = 0; u->h_scal[2] = 0;
    HIPCHK(hipMemcpyAsync(u->d_scal, u->h_scal, 12, hipMemcpyHostToDevice, c->stream));
    u->G.next = u->d_list[cur ^ 1];
    { ProfScope ps(c, KP_UG_WALK);
      SHK_BY_WORDS(u->W,
        hipLaunchKernelGGL(k_ug_walk<KW>, dim3((nactive + 7) / 8), dim3(64), 0, c->stream, u->G, (const uint32_t *)u->d_list[cur], nactive, c->tab[c->cur],
                           c->q_lo, c->nslots, c->cfg.hb, u->k, u->amin, mark ? 1 : 2, step, u->max_len)); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(u->h_scal, u->d_scal, 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (u->h_scal[2]) return u->h_scal[2] & SHK_UG_E_MAP ? SHK_ERR_CORRUPT : SHK_ERR_BATCH;
    u->ncontigs = u->h_scal[0];
    nactive = u->h_scal[1];
    cur ^= 1;
    u->st.rounds++;
  }
  // (the lists may have been swapped an odd number of times: nothing depends on which one is list 0 between calls)
  return SHK_OK;
}

extern "C" int shk_unitigs_add_seeds(shk_ctx *c, shk_unitig_set *u, const char *seeds, const uint32_t *seed_counts, uint32_t n,
                                     uint32_t k, uint64_t abundance_min, uint32_t max_len, int mark_traveled) {
  if (!c || !u || (n && (!seeds || !seed_counts))) return SHK_ERR_ARG;
  if (k < 2 || k > SHK_WALK_MAX_K || max_len < k + 1) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc_ = table_sync(c); if (rc_) return rc_; }
  int rc = ug_bind(u, c, k, abundance_min, max_len);
  if (rc || n == 0) return rc;
  if ((uint64_t)n > u->seeds_cap) {
    hipFree(u->d_seeds); hipFree(u->d_counts); u->d_seeds = nullptr; u->d_counts = nullptr;
    if (dmalloc(&u->d_seeds, (uint64_t)n * k) || dmalloc(&u->d_counts, (uint64_t)n)) return SHK_ERR_HIP;
    u->seeds_cap = n;
  }
  rc = ug_reserve(u, (uint64_t)u->ncontigs + n + 16, (uint64_t)n + 16);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(u->d_seeds, seeds, (size_t)n * k, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(u->d_counts, seed_counts, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  SHK_BY_WORDS(u->W,
    hipLaunchKernelGGL(k_ug_add_seeds<KW>, dim3((n + 255) / 256), dim3(256), 0, c->stream, u->G, (const char *)u->d_seeds, (const uint32_t *)u->d_counts, n, k,
                       u->ncontigs, u->d_list[0]));
  HIPCHK(hipGetLastError());
  u->ncontigs += n;
  rc = ug_run(u, n, mark_traveled);
  return finish(c, rc);
}

// Seeds straight from FASTQ chunks (processDataChunk's rule, contig_assembly.cpp:1856-1876) and their walks, without
// the seeds leaving the device: parse -> k_select_seeds (lookup that marks) -> new contigs -> rounds.
extern "C" int shk_unitigs_add_reads(shk_ctx *c, shk_unitig_set *u, const void *text, int text_on_device, uint64_t text_bytes,
                                     const uint64_t *chunk_off, const uint64_t *chunk_len, uint32_t nchunks, uint32_t k,
                                     uint64_t abundance_min, uint64_t count_min, uint64_t count_max, uint32_t max_len,
                                     uint64_t *nseeds) {
  if (!c || !u || !text || !chunk_off || !chunk_len || nchunks == 0 || nchunks > SHK_MAX_CHUNKS) return SHK_ERR_ARG;
  if (k < 2 || k > SHK_WALK_MAX_K || max_len < k + 1) return SHK_ERR_ARG;
  HIPCHK(hipSetDevice(c->dev));
  { int rc_ = table_sync(c); if (rc_) return rc_; }
  int rc = ug_bind(u, c, k, abundance_min, max_len);
  if (rc) return rc;
  const uint8_t *dtext;
  uint64_t nreads;
  if (upload_wait(c, text, text_on_device, c->stream)) return SHK_ERR_HIP;
  rc = parse_stage(c, c, text, text_on_device, text_bytes, chunk_off, chunk_len, nchunks, &dtext, &nreads);
  if (rc) return finish(c, rc);
  if (nseeds) *nseeds = 0;
  if (nreads == 0) return finish(c, 0);
  if (nreads > 0x7FFFFFF0ull) return SHK_ERR_BATCH;
  if (nreads > u->seeds_cap) {
    hipFree(u->d_seeds); hipFree(u->d_counts); u->d_seeds = nullptr; u->d_counts = nullptr;
    if (dmalloc(&u->d_seeds, nreads * k) || dmalloc(&u->d_counts, nreads)) return SHK_ERR_HIP;
    u->seeds_cap = nreads;
  }
  // The reference takes its seeds read by read: a read whose middle k-mer an earlier walk has already marked gives none
  // (:1871-1873). Selecting all seeds of a batch at once would walk every unitig once per read that covers it, so the
  // reads are taken in slices that grow geometrically: the walks of one slice mark their unitigs before the next, four
  // times larger, slice looks at its reads -- the duplicates stay a small multiple of the number of unitigs.
  c->foreign_marks = 1;
  uint64_t total_seeds = 0, lo = 0, slice = 16384;
  if (const char *e = getenv("SHK_SEED_SLICE")) { long long v = atoll(e); if (v > 0) slice = (uint64_t)v; }
  while (lo < nreads) {
    const uint64_t hi = nreads - lo < slice ? nreads : lo + slice;
    const uint64_t m = hi - lo;
    rc = ug_reserve(u, (uint64_t)u->ncontigs + m + 16, m + 16);
    if (rc) return finish(c, rc);
    { ProfScope ps(c, KP_WALK);
      hipLaunchKernelGGL(k_select_seeds, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, c->tab[c->cur], c->q_lo, c->nslots,
                         c->cfg.hb, dtext, c->d_rd_start, c->d_rd_end, lo, hi, k, count_min, count_max, 1, u->d_seeds, u->d_counts); }
    u->h_scal[0] = u->ncontigs; u->h_scal[1] = 0; u->h_scal[2] = 0; u->h_scal[3] = 0;
    HIPCHK(hipMemcpyAsync(u->d_scal, u->h_scal, 16, hipMemcpyHostToDevice, c->stream));
    SHK_BY_WORDS(u->W,
      hipLaunchKernelGGL(k_ug_seeds_from_reads<KW>, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, c->stream, u->G, (const char *)u->d_seeds,
                         (const uint32_t *)u->d_counts, lo, hi, k, u->d_list[0], u->d_scal + 3));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(u->h_scal, u->d_scal, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (u->h_scal[2]) return finish(c, SHK_ERR_BATCH);
    u->ncontigs = u->h_scal[0];
    const uint32_t n = u->h_scal[3];
    total_seeds += n;
    rc = ug_run(u, n, 1);
    if (rc) return finish(c, rc);
    lo = hi;
    slice *= 4;
  }
  if (nseeds) *nseeds = total_seeds;
  return finish(c, SHK_OK);
}

extern "C" int shk_unitig_set_write(shk_unitig_set *u, uint32_t k, const char *out_path, shk_unitig_stats *stats) {
  if (!u || !out_path) return SHK_ERR_ARG;
  FILE *fo = fopen(out_path, "w");
  if (!fo) return SHK_ERR_IO;
  if (!u->c) {          // nothing was ever added
    fclose(fo);
    if (stats) *stats = u->st;
    return SHK_OK;
  }
  if (k != u->k) { fclose(fo); return SHK_ERR_ARG; }
  shk_ctx *c = u->c;
  HIPCHK(hipSetDevice(c->dev));
  { int rc_ = table_sync(c); if (rc_) return rc_; }
  const uint32_t n = u->ncontigs;
  uint32_t *d_keep = nullptr, *d_lens = nullptr, *d_ulen = nullptr, *d_ul1 = nullptr, *d_cnt = nullptr;
  uint64_t *d_newid = nullptr, *d_off = nullptr, *d_uoff = nullptr, *d_sums = nullptr;
  char *d_bases = nullptr;
  int32_t *d_med = nullptr, *d_links = nullptr;
  uint64_t *m_k[SHK_KM_WMAX] = {}; uint32_t *m_v = nullptr;
  int rc = SHK_OK;
  std::vector<char> bases;
  std::vector<uint64_t> uoff;
  std::vector<uint32_t> ulen;
  std::vector<int32_t> med, links;
  uint64_t nunits = 0, total = 0;
  do {
    // the scans run over all contig ids (seeds, queued neighbours, duplicates): their block sums get scratch of their own,
    // sized from n (the context's is sized for its key batches -- a graph of more than 16.7 M ids used to be refused here,
    // after all the walks)
    if (dmalloc(&d_sums, (uint64_t)n / SHK_SCAN_TILE + 8)) { rc = SHK_ERR_HIP; break; }
    if (dmalloc(&d_keep, (uint64_t)n + 1) || dmalloc(&d_lens, (uint64_t)n + 1) || dmalloc(&d_newid, (uint64_t)n + 2) || dmalloc(&d_off, (uint64_t)n + 2)) { rc = SHK_ERR_HIP; break; }
    SHK_BY_WORDS(u->W, hipLaunchKernelGGL(k_ug_check<KW>, dim3((n + 255) / 256), dim3(256), 0, c->stream, u->G, n, d_keep, d_lens));
    if (getenv("SHK_UG_DEBUG")) {   // diagnostics: contigs by kind, state and last stop reason
      std::vector<uint8_t> hs(n), hk(n), hp(n);
      std::vector<uint32_t> hkeep(n);
      hipMemcpy(hs.data(), u->G.state, n, hipMemcpyDeviceToHost); hipMemcpy(hk.data(), u->G.kind, n, hipMemcpyDeviceToHost);
      hipMemcpy(hp.data(), u->G.stop, n, hipMemcpyDeviceToHost); hipMemcpy(hkeep.data(), d_keep, (size_t)n * 4, hipMemcpyDeviceToHost);
      unsigned long long h[2][4][8] = {{{0}}}, kept[2] = {0, 0};
      for (uint32_t i = 1; i < n; i++) { h[hk[i] & 1][hs[i] & 3][hp[i] & 7]++; kept[hk[i] & 1] += hkeep[i]; }
      for (int kd = 0; kd < 2; kd++) for (int stt = 0; stt < 4; stt++) for (int sp = 0; sp < 8; sp++)
        if (h[kd][stt][sp]) fprintf(stderr, "SHK_UG_DEBUG %s state %d stop %d: %llu\n", kd ? "seed" : "cand", stt, sp, h[kd][stt][sp]);
      fprintf(stderr, "SHK_UG_DEBUG kept seeds %llu candidates %llu\n", kept[1], kept[0]);
      std::vector<uint64_t> hh(n);
      std::vector<uint32_t> hl(n);
      hipMemcpy(hh.data(), u->G.hmin, (size_t)n * 8, hipMemcpyDeviceToHost); hipMemcpy(hl.data(), u->G.len, (size_t)n * 4, hipMemcpyDeviceToHost);
      for (uint32_t i = 1; i < n; i++)
        if ((hp[i] & 15) == SHK_STOP_CIRCLE) fprintf(stderr, "SHK_UG_DEBUG circle id %u state %d keep %u len %u hmin %016llx\n", i, hs[i], hkeep[i], hl[i], (unsigned long long)hh[i]);
    }
    if (run_scan<uint32_t>(c, c, d_keep, n, nullptr, d_newid, d_sums) || run_scan<uint32_t>(c, c, d_lens, n, nullptr, d_off, d_sums)) { rc = SHK_ERR_HIP; break; }
    if (hipMemcpyAsync(c->h_pinned + HP_TOTAL, d_newid + n, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->h_pinned + HP_AUX, d_off + n, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { rc = SHK_ERR_HIP; break; }
    nunits = c->h_pinned[HP_TOTAL]; total = c->h_pinned[HP_AUX];
    if (nunits == 0) break;
    if (dmalloc(&d_bases, total + 16) || dmalloc(&d_cnt, total + 16) || dmalloc(&d_uoff, nunits + 1) || dmalloc(&d_ulen, nunits + 1) ||
        dmalloc(&d_ul1, nunits + 1) || dmalloc(&d_med, nunits + 1) || dmalloc(&d_links, nunits * 8 + 8)) { rc = SHK_ERR_HIP; break; }
    { ProfScope ps(c, KP_UG_FINISH);
      SHK_BY_WORDS(u->W,
        hipLaunchKernelGGL(k_ug_emit<KW>, dim3((n + 63) / 64), dim3(64), 0, c->stream, u->G, n, (const uint32_t *)d_keep, (const uint64_t *)d_newid,
                           (const uint64_t *)d_off, c->tab[c->cur], c->q_lo, c->nslots, c->cfg.hb, k, u->amin, d_bases, d_cnt, d_uoff, d_ulen, d_ul1)); }
    hipLaunchKernelGGL(k_ug_median, dim3((uint32_t)nunits), dim3(SHK_WAVE), 0, c->stream, (uint32_t)nunits, (const uint64_t *)d_uoff, (const uint32_t *)d_ulen,
                       (const uint32_t *)d_ul1, (const uint32_t *)d_cnt, k, d_med);
    // the graph pass's own map: first k-mer -> +number, RC(last k-mer) -> -number
    uint64_t nm = 4096;
    while (nm < nunits * 8) nm *= 2;
    if (dmalloc(&m_v, nm)) { rc = SHK_ERR_HIP; break; }
    for (uint32_t j = 0; j < u->W && !rc; j++) if (dmalloc(&m_k[j], nm)) rc = SHK_ERR_HIP;
    if (rc) break;
    if (hipMemsetAsync(m_v, 0, nm * 4, c->stream) != hipSuccess) { rc = SHK_ERR_HIP; break; }
    ShkUG G2 = u->G;
    for (int j = 0; j < SHK_KM_WMAX; j++) G2.mk[j] = m_k[j];
    G2.mv = m_v; G2.mmask = (uint32_t)(nm - 1);
    SHK_BY_WORDS(u->W,
      hipLaunchKernelGGL(k_ug_map2<KW>, dim3((n + 255) / 256), dim3(256), 0, c->stream, G2, n, (const uint32_t *)d_keep, (const uint64_t *)d_newid);
      hipLaunchKernelGGL(k_ug_links<KW>, dim3((n + 255) / 256), dim3(256), 0, c->stream, G2, n, (const uint32_t *)d_keep, (const uint64_t *)d_newid, k, d_links));
    if (hipGetLastError() != hipSuccess) { rc = SHK_ERR_HIP; break; }
    bases.resize(total); uoff.resize(nunits); ulen.resize(nunits); med.resize(nunits); links.resize(nunits * 8);
    if (hipMemcpyAsync(bases.data(), d_bases, total, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(uoff.data(), d_uoff, nunits * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(ulen.data(), d_ulen, nunits * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(med.data(), d_med, nunits * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(links.data(), d_links, nunits * 32, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(u->h_scal + 4, u->d_stats, 32, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { rc = SHK_ERR_HIP; break; }
  } while (0);
  hipStreamSynchronize(c->stream);
  hipFree(d_keep); hipFree(d_lens); hipFree(d_newid); hipFree(d_off); hipFree(d_bases); hipFree(d_cnt); hipFree(d_uoff); hipFree(d_ulen);
  hipFree(d_ul1); hipFree(d_med); hipFree(d_links); hipFree(m_v); hipFree(d_sums);
  for (int j = 0; j < SHK_KM_WMAX; j++) hipFree(m_k[j]);
  if (rc) { fclose(fo); return finish(c, rc); }
  // the records as the reference writes them (:606-626): ids 0-based in final numbering, successors then predecessors.
  // Formatted in slices by a few host threads (two million records are ~6 M numbers to print), written in order
  {
    const auto put_num = [](std::string &o, long long v) {
      char t[24]; int n = 0;
      unsigned long long a = v < 0 ? 0ULL - (unsigned long long)v : (unsigned long long)v;
      do { t[n++] = (char)('0' + a % 10); a /= 10; } while (a);
      if (v < 0) o.push_back('-');
      while (n) o.push_back(t[--n]);
    };
    const auto format = [&](uint64_t a, uint64_t b, std::string &o) {
      o.clear();
      for (uint64_t i = a; i < b; i++) {
        const long long len = ulen[i];
        o.push_back('>'); put_num(o, (long long)i);
        o.append(" LN:i:"); put_num(o, len);
        o.append(" KC:i:"); put_num(o, (long long)med[i] * (len - (long long)k + 1));
        o.append(" km:f:"); put_num(o, med[i]);
        for (int x = 0; x < 8; x++) {
          const int32_t v = links[i * 8 + x];
          if (!v) continue;
          o.append(x < 4 ? " L:+:" : " L:-:"); put_num(o, (v > 0 ? v : -v) - 1);
          o.append(v > 0 ? ":+" : ":-");
        }
        o.push_back('\n');
        o.append(bases.data() + uoff[i], (size_t)len);
        o.push_back('\n');
      }
    };
    const uint64_t slice = 1u << 15;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 8 ? 8 : nt;
    std::vector<std::string> outs(nt);
    for (uint64_t a0 = 0; a0 < nunits; a0 += slice * nt) {
      std::vector<std::thread> th;
      unsigned used = 0;
      for (unsigned t = 0; t < nt && a0 + t * slice < nunits; t++, used++) {
        const uint64_t a = a0 + t * slice, b = a + slice < nunits ? a + slice : nunits;
        if (nt == 1) format(a, b, outs[0]);
        else th.emplace_back(format, a, b, std::ref(outs[t]));
      }
      for (auto &x : th) x.join();
      for (unsigned t = 0; t < used; t++)
        if (fwrite(outs[t].data(), 1, outs[t].size(), fo) != outs[t].size()) rc = SHK_ERR_IO;
    }
  }
  if (fclose(fo) != 0) rc = SHK_ERR_IO;
  if (rc) return finish(c, rc);
  const unsigned long long *ds = reinterpret_cast<const unsigned long long *>(u->h_scal + 4);
  u->st.unitigs = nunits; u->st.total_len = total;
  if (nunits) { u->st.extensions = ds[0]; u->st.duplicates = ds[1]; u->st.truncated = ds[2]; }
  if (stats) *stats = u->st;
  return finish(c, SHK_OK);
}

extern "C" int shk_find_unitigs(shk_ctx *c, const char *seeds, const uint32_t *seed_counts, uint32_t n, uint32_t k,
                                uint64_t abundance_min, uint32_t max_len, const char *out_path, shk_unitig_stats *stats) {
  if (!out_path) return SHK_ERR_ARG;
  shk_unitig_set *u = shk_unitig_set_new();
  int rc = shk_unitigs_add_seeds(c, u, seeds, seed_counts, n, k, abundance_min, max_len, 0);
  if (!rc) rc = shk_unitig_set_write(u, k, out_path, stats);
  shk_unitig_set_free(u);
  return rc;
}

// batches whose first-level output took the split record (either front end), since the context was created
extern "C" uint64_t shk_prefetch_passes(shk_ctx *c) { return c ? c->prefetch_passes : 0; }
extern "C" uint64_t shk_split_batches(shk_ctx *c) { return c ? c->split_batches + (c->front ? c->front->b.split_batches : 0) : 0; }
extern "C" int shk_profile_enable(shk_ctx *c, int on) { if (!c) return SHK_ERR_ARG; c->prof_on = on; return SHK_OK; }
extern "C" int shk_profile_reset(shk_ctx *c) {
  if (!c) return SHK_ERR_ARG;
  for (int i = 0; i < KP_N; i++) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
  return SHK_OK;
}
extern "C" int shk_profile_get(shk_ctx *c, shk_kernel_time *out, int cap) {
  if (!c || !out) return SHK_ERR_ARG;
  prof_collect(c);              // (a placement launched by a reader such as shk_export_blocks is still pending)
  int n = 0;
  for (int i = 0; i < KP_N && n < cap; i++) {
    out[n].name = kp_names[i]; out[n].launches = c->prof_n[i]; out[n].ms = c->prof_ms[i]; n++;
  }
  return n;
}
