// Key-word partition by quotient region (MSD radix, one digit per level) and the
// device-wide exclusive scan the pipeline uses.
//
// The reference has no such step: it takes a region lock per k-mer and shifts slots in
// place (cqf/gqf.c:174-264, 1614-1915). Here every key of a batch is first routed to the
// 2048-quotient region that owns it, so that one workgroup can rebuild that region in LDS
// (cqf_kernels.hip). Order inside a region is irrelevant: the filter's bytes depend only
// on the key multiset.
#include "shk_device.h"
#include <type_traits>

#define SHK_RP_TILE 4096     // keys per window
#define SHK_RP_MAXP 1024     // at most 10 digit bits per level
#define SHK_SCAN_TILE 2048   // elements per workgroup in the scan kernels

struct ShkRpLevel {
  uint32_t shift;     // digit = (region >> shift) & (P-1)
  uint32_t bits;      // P = 1 << bits
  uint32_t nbuckets;  // buckets entering this level (= product of earlier P's)
  uint32_t hb;
  uint64_t q_lo;      // first quotient this context owns (multi-GPU shards)
  uint64_t nslots;    // quotients this context owns
  uint32_t cb;        // chunk bits of the narrow record between the level in front of the last one and the last one (below)
  uint32_t out32;     // 1 (last level): write 32-bit records (quotient in region << 8 | remainder) << SHK_CHUNK_BITS | chunk
  uint32_t ablate;    // diagnostics only (SHK_RP_ABLATE): 1 = no reservation atomics, all windows write the same few KB per digit (results invalid)
  uint32_t slot_cap;  // last level only, 0 = off: bucket (region) i owns the fixed slot [i * slot_cap, (i + 1) * slot_cap) of the
                      // output instead of an exact range from a histogram pass + scan (the keys are hash values: a
                      // region's share of a batch is its mean +- a few sigma); `cursor` starts at the slots' first
                      // positions and ends as the regions' END positions. A region that gets more raises SHK_E_SLOT_FULL.
                      // The level in front of the last one may be slotted the same way (narrow records out, the slots of a
                      // batch whose first level came slotted out of k_roll_scatter); there the bit is SHK_E_SLOT_FULL_UP
  uint32_t ng_log2;   // first level only: every digit's bucket is laid out as 2^ng_log2 sub-buckets, one per window group
                      // (window index mod 2^ng_log2), each with its own cursor, so that the windows of a batch do not all
                      // reserve from the same P addresses. Measured on 832 M keys: the scatter itself is unchanged (its
                      // first level stays at 4.7 ms against 3.2 for the second: not the atomics), the hash kernel's
                      // histogram flush gets 5 % off that kernel
  uint32_t kb;        // RP_SPLIT_IN only: key bits of the split record (below)
  uint64_t hi_off;    // RP_SPLIT_IN only: bytes from the input's 4-byte plane to its byte plane = 4 * (positions of the input's extent)
};

__device__ __forceinline__ uint32_t shk_word_region(uint64_t w, uint32_t hb, uint64_t q_lo) {
  uint64_t key = hb >= 64 ? w : (w & ((1ULL << hb) - 1));
  return (uint32_t)(((key >> 8) - q_lo) >> SHK_REGION_LOG2);
}

// The narrow record: what the level in front of the last one hands to the last one when the call's chunk tags fit cb =
// 32 - 16 - (last level's digit bits) bits. Behind all levels but the last a word's bucket is its region's high digits, so
//   rec32 = ((last digit << 16 | quotient in region << 8 | remainder) << cb) | chunk
// is all that anybody still reads of it: half the bytes of the key word. (The digit and the quotient in the region are
// adjacent bits of the quotient: the upper field is the low 16 + b_last bits of key - (q_lo << 8).)
enum { RP_WORDS = 0, RP_NARROW_OUT = 1, RP_NARROW_IN = 2, RP_SPLIT_IN = 3 };   // k_rp_scatter: 8-byte words in and out (the last
                                                              // level: 4-byte records out); writes the narrow record; reads it;
                                                              // reads the split record and writes the narrow one
__device__ __forceinline__ uint32_t shk_narrow_rec(uint64_t w, uint32_t hb, uint64_t q_lo, uint32_t cb) {
  const uint64_t key = hb >= 64 ? w : (w & ((1ULL << hb) - 1));
  const uint32_t up = (uint32_t)(key - (q_lo << 8)) & ((1u << (32 - cb)) - 1);
  return (up << cb) | ((uint32_t)(w >> hb) & ((1u << cb) - 1));
}

// The split record: what k_roll_scatter hands to the middle level of a three-level context that owns the whole filter, for
// the batches that are narrow. Behind the first level a word's bucket is its first digit, so all that is still read of it
// are the kb = rbits + 16 - bits0 bits of key - (q_lo << 8) below that digit and the chunk tag (< 2^cb, cb as above):
//   rec40 = chunk << kb | ((key - (q_lo << 8)) & (2^kb - 1)),      kb + cb <= 40 and kb <= 32 (create_init)
// kept as two planes in the buffer the 8-byte words would use: lo32 = its low 32 bits at positions [0, E) of a uint32_t
// array, hi8 = rec40 >> 32 at byte 4 * E + position, E = the extent in positions the 8-byte form has (all slots of a
// slotted batch, the buffer's capacity otherwise): 5 bytes per key written and read instead of 8. With kb <= 32 the high
// byte holds bits of the chunk only, so it is one value per read for the kernel that writes it. The middle level
// (RP_SPLIT_IN) takes its digit from the key bits and builds the narrow record from the two planes, bit for bit
// shk_narrow_rec's; a key masked to hb bits cannot lie outside a context that owns the whole filter, so that form has no
// SHK_E_CORRUPT check.
__device__ __forceinline__ uint32_t shk_split_to_narrow(uint32_t lo32, uint32_t hi8, uint32_t kb, uint32_t cb) {
  const uint32_t chunk = (uint32_t)((((uint64_t)hi8 << 32) | lo32) >> kb) & ((1u << cb) - 1);
  return ((lo32 & ((1u << (32 - cb)) - 1)) << cb) | chunk;
}

// ---------------------------------------------------------------- exclusive scan (3 kernels)
template <typename T>
__global__ void k_scan_reduce(const T *in, uint64_t n_host, const uint64_t *n_dev, uint64_t *block_sums) {
  __shared__ uint64_t scratch[SHK_MAX_WAVES + 1];
  const uint64_t n = n_dev ? *n_dev : n_host;
  const uint64_t base = (uint64_t)blockIdx.x * SHK_SCAN_TILE;
  uint64_t s = 0;
  for (uint64_t i = base + threadIdx.x; i < base + SHK_SCAN_TILE && i < n; i += blockDim.x) s += in[i];
  uint64_t tot = shk_block_sum64(s, scratch);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}
// single workgroup: exclusive scan of the block sums in place; total to *total
__global__ void k_scan_top(uint64_t *block_sums, uint64_t nblocks, uint64_t *total) {
  __shared__ uint64_t scratch[SHK_MAX_WAVES + 1];
  __shared__ uint64_t carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint64_t b = 0; b < nblocks; b += blockDim.x) {
    uint64_t i = b + threadIdx.x;
    uint64_t v = i < nblocks ? block_sums[i] : 0, tot;
    uint64_t ex = shk_block_exscan64(v, &tot, scratch);
    uint64_t carry = carry_s;
    if (i < nblocks) block_sums[i] = carry + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry_s = carry + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry_s;
}
// out[i] = exclusive prefix; out[n] = total (written by the workgroup that owns index n)
template <typename T>
__global__ void k_scan_apply(const T *in, uint64_t n_host, const uint64_t *n_dev, const uint64_t *block_sums,
                             const uint64_t *total, uint64_t *out) {
  __shared__ uint64_t scratch[SHK_MAX_WAVES + 1];
  const uint64_t n = n_dev ? *n_dev : n_host;
  const uint64_t base = (uint64_t)blockIdx.x * SHK_SCAN_TILE;
  if (base > n) return;
  const unsigned per = SHK_SCAN_TILE / blockDim.x;  // blockDim.x divides the tile
  const uint64_t my = base + (uint64_t)threadIdx.x * per;
  uint64_t s = 0;
  for (unsigned j = 0; j < per; j++)
    if (my + j < n) s += in[my + j];
  uint64_t tot;
  uint64_t ex = shk_block_exscan64(s, &tot, scratch) + block_sums[blockIdx.x];
  for (unsigned j = 0; j < per; j++) {
    if (my + j < n) { out[my + j] = ex; ex += in[my + j]; }
  }
  if (threadIdx.x == 0 && n >= base && n < base + SHK_SCAN_TILE) out[n] = *total;
}

// ---------------------------------------------------------------- partition
// bucket_base for level 1 = {0, n}
__global__ void k_rp_base1(const uint64_t *n_p, uint64_t *bucket_base) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { bucket_base[0] = 0; bucket_base[1] = *n_p; }
}

// first bucket that has a key in window w (windows are SHK_RP_TILE keys of the input)
__global__ void k_rp_tile_first(const uint64_t *bucket_base, uint32_t nbuckets, const uint64_t *n_p, uint32_t *tfb) {
  const uint64_t n = *n_p;
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t pos = w * SHK_RP_TILE;
  if (pos >= n) return;
  uint32_t lo = 0, hi = nbuckets;  // last b with bucket_base[b] <= pos
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) / 2;
    if (bucket_base[mid] <= pos) lo = mid; else hi = mid;
  }
  tfb[w] = lo;
}

// Histogram of the next digit. One workgroup takes `wtiles` consecutive windows, so that the global
// counters of a (bucket, digit) see one atomic per workgroup and bucket, not one per window
// (at the first level every window would hit the same P addresses).
// NARROW: the input is the narrow record (the exact redo of a slotted last level behind a narrow level).
// Slotted input (here and in k_rp_scatter): bucket b is [bucket_base[b], bucket_end[b]) and a gap may follow it; *n_p is
// then the input's EXTENT in positions (all slots), not the number of words. bucket_end null: bucket_base[b + 1].
template <bool NARROW>
__global__ void k_rp_hist(const uint64_t *words_, const uint64_t *n_p, const uint64_t *bucket_base, const uint64_t *bucket_end,
                          const uint32_t *tfb, ShkRpLevel lv, uint64_t *hist, uint32_t wtiles) {
  __shared__ uint32_t lh[SHK_RP_MAXP];
  using W = typename std::conditional<NARROW, uint32_t, uint64_t>::type;
  const W *words = reinterpret_cast<const W *>(words_);
  const uint64_t n = *n_p;
  const uint64_t wstart = (uint64_t)blockIdx.x * wtiles * SHK_RP_TILE;
  if (wstart >= n) return;
  const uint64_t wend = wstart + (uint64_t)wtiles * SHK_RP_TILE < n ? wstart + (uint64_t)wtiles * SHK_RP_TILE : n;
  const uint32_t P = 1u << lv.bits;
  for (uint32_t b = tfb[(uint64_t)blockIdx.x * wtiles]; b < lv.nbuckets && bucket_base[b] < wend; b++) {
    const uint64_t lo = bucket_base[b] > wstart ? bucket_base[b] : wstart;
    const uint64_t be = bucket_end ? bucket_end[b] : bucket_base[b + 1];
    const uint64_t hi = be < wend ? be : wend;
    if (hi <= lo) continue;
    for (uint32_t d = threadIdx.x; d < (P << lv.ng_log2); d += blockDim.x) lh[d] = 0;
    __syncthreads();
    // four loads in flight per thread
    for (uint64_t i0 = lo; i0 < hi; i0 += 4ull * blockDim.x) {
      W w[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint64_t i = i0 + (uint64_t)u * blockDim.x + threadIdx.x;
        w[u] = i < hi ? words[i] : 0;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint64_t i = i0 + (uint64_t)u * blockDim.x + threadIdx.x;
        if (i < hi) {
          const uint32_t dg = NARROW ? (uint32_t)(w[u] >> (16 + lv.cb)) : (shk_word_region(w[u], lv.hb, lv.q_lo) >> lv.shift) & (P - 1);
          const uint32_t grp = (uint32_t)(i >> SHK_RP_TILE0_LOG2) & ((1u << lv.ng_log2) - 1);     // the (first-level) scatter window this key lies in
          atomicAdd(&lh[(dg << lv.ng_log2) | grp], 1u);
        }
      }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < (P << lv.ng_log2); d += blockDim.x)
      if (lh[d]) atomicAdd((unsigned long long *)&hist[(((uint64_t)b * P) << lv.ng_log2) + d], (unsigned long long)lh[d]);
    __syncthreads();
  }
}

// bucket bases of the next level from the scanned sub-bucket bases of a grouped first level: base[d] = sub[d << ng_log2]
__global__ void k_rp_group_bases(const uint64_t *sub, uint32_t nd, uint32_t ng_log2, uint64_t *base) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d <= nd) base[d] = sub[(uint64_t)d << ng_log2];
}

// cursor[b*P+d] starts at the scanned base of (b,d) and is advanced by reservations.
// One window of SHK_RP_TILE keys per workgroup of SHK_RP_THREADS threads: the keys stay in
// registers; ONE LDS atomic per key yields both the digit count and the key's rank inside
// its digit (the order of keys inside a bucket is free: the rebuild folds them into a hash);
// after the scan the keys are staged digit by digit in LDS and leave as contiguous runs.
#define SHK_RP_THREADS 512
#define SHK_RP_KPT (SHK_RP_TILE / SHK_RP_THREADS)
// (TILE_LOG2, THREADS) = (12, 512) for all levels but the first of a context's own partition: (SHK_RP_TILE0_LOG2, 1024)
// Level 0 of a partition that starts from unsorted words (the sharded flow's received words): the first level's digit
// counts per window group as k_rp_hist gives them and, from the same pass over the keys, the SECOND level's counts
// (hist1[d0 * P1 + d1], the layout k_rp_hist would fill for level 1 with its buckets = the first level's digits) -- the
// second level then needs no counting pass of its own (1.7-2.0 ms per 832 M keys). For bits0 + bits1 <= LB2.
template <int LB2>
__global__ void k_rp_hist2(const uint64_t *words, const uint64_t *n_p, ShkRpLevel lv0, ShkRpLevel lv1, uint64_t *hist0, uint64_t *hist1,
                           uint32_t wtiles) {
  __shared__ uint32_t lh0[SHK_RP_MAXP];
  __shared__ uint32_t lh1[1u << LB2];
  const uint64_t n = *n_p;
  const uint64_t wstart = (uint64_t)blockIdx.x * wtiles * SHK_RP_TILE;
  if (wstart >= n) return;
  const uint64_t wend = wstart + (uint64_t)wtiles * SHK_RP_TILE < n ? wstart + (uint64_t)wtiles * SHK_RP_TILE : n;
  const uint32_t P0 = 1u << lv0.bits, C = 1u << (lv0.bits + lv1.bits);
  for (uint32_t d = threadIdx.x; d < (P0 << lv0.ng_log2); d += blockDim.x) lh0[d] = 0;
  for (uint32_t d = threadIdx.x; d < C; d += blockDim.x) lh1[d] = 0;
  __syncthreads();
  for (uint64_t i0 = wstart; i0 < wend; i0 += 4ull * blockDim.x) {
    uint64_t w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t i = i0 + (uint64_t)u * blockDim.x + threadIdx.x;
      w[u] = i < wend ? words[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t i = i0 + (uint64_t)u * blockDim.x + threadIdx.x;
      if (i < wend) {
        const uint32_t region = shk_word_region(w[u], lv0.hb, lv0.q_lo);
        const uint32_t d0 = (region >> lv0.shift) & (P0 - 1);
        const uint32_t grp = (uint32_t)(i >> SHK_RP_TILE0_LOG2) & ((1u << lv0.ng_log2) - 1);
        atomicAdd(&lh0[(d0 << lv0.ng_log2) | grp], 1u);
        atomicAdd(&lh1[(region >> lv1.shift) & (C - 1)], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < (P0 << lv0.ng_log2); d += blockDim.x)
    if (lh0[d]) atomicAdd((unsigned long long *)&hist0[d], (unsigned long long)lh0[d]);
  for (uint32_t d = threadIdx.x; d < C; d += blockDim.x)
    if (lh1[d]) atomicAdd((unsigned long long *)&hist1[d], (unsigned long long)lh1[d]);
}

// fixed-capacity region slots: cursor[i] = i * cap
__global__ void k_rp_slot_cursors(uint64_t *cursor, uint64_t n, uint32_t cap) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) cursor[i] = i * cap;
}
// the slots of a level above the last one: the n buckets' bases (base[n] = all slots), their cursors, and the extent
// in positions that the next level's windows cover
__global__ void k_rp_slot_bases(uint64_t *base, uint64_t *cursor, uint64_t n, uint64_t cap, uint64_t *extent) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
    base[i] = i * cap;
    if (i < n) cursor[i] = i * cap; else *extent = n * cap;
  }
}

// FORM (RP_WORDS, RP_NARROW_OUT, RP_NARROW_IN): which of `in` and `out` holds narrow records. A narrow record is made
// from the key word as it is loaded (the last place the whole key exists: the SHK_E_CORRUPT check of a narrow batch is
// here), so that the registers and the LDS stage of those instantiations hold 4 bytes per key. RP_SPLIT_IN is RP_NARROW_OUT
// behind another load: the split record's two planes (lv.kb, lv.hi_off) instead of the 8-byte word.
template <int TILE_LOG2, int THREADS, int PMAX = SHK_RP_MAXP, int FORM = RP_WORDS>
__global__ void __launch_bounds__(THREADS) k_rp_scatter(const uint64_t *in_, uint64_t *out, const uint64_t *n_p,
                                                        const uint64_t *bucket_base, const uint64_t *bucket_end, const uint32_t *tfb,
                                                        ShkRpLevel lv, uint64_t *cursor, uint32_t *err) {
  constexpr uint32_t SHK_RP_TILE_ = 1u << TILE_LOG2;
  constexpr int KPT_ = (int)(SHK_RP_TILE_ / THREADS);   // keys per thread (registers)
  static_assert(SHK_RP_TILE_ <= 65536, "a rank inside a digit takes 16 bits");
  using WIN = typename std::conditional<FORM == RP_NARROW_IN || FORM == RP_SPLIT_IN, uint32_t, uint64_t>::type;    // what is loaded
  constexpr bool NOUT = FORM == RP_NARROW_OUT || FORM == RP_SPLIT_IN;                         // narrow records leave
  using WST = typename std::conditional<FORM == RP_WORDS, uint64_t, uint32_t>::type;        // what is held and staged
  const WIN *in = reinterpret_cast<const WIN *>(in_);
  __shared__ uint32_t lh[PMAX];      // digit counts (= next rank while counting); PMAX >= 2^lv.bits (the host's choice)
  __shared__ uint32_t lbase[PMAX];   // local exclusive base of each digit
  __shared__ uint64_t gbase[PMAX];   // reserved global base of each digit
  __shared__ WST stage[SHK_RP_TILE_];
  __shared__ uint32_t scratch[SHK_MAX_WAVES + 1];
  const uint64_t n = *n_p;
  const uint64_t wstart = (uint64_t)blockIdx.x * SHK_RP_TILE_;
  if (wstart >= n) return;
  const uint64_t wend = wstart + SHK_RP_TILE_ < n ? wstart + SHK_RP_TILE_ : n;
  const uint32_t P = 1u << lv.bits;
  // (tfb is indexed by 4096-key windows)
  for (uint32_t b = (lv.nbuckets > 1 ? tfb[(uint64_t)blockIdx.x << (TILE_LOG2 - 12)] : 0u); b < lv.nbuckets && bucket_base[b] < wend; b++) {
    const uint64_t lo = bucket_base[b] > wstart ? bucket_base[b] : wstart;
    const uint64_t be = bucket_end ? bucket_end[b] : bucket_base[b + 1];
    const uint64_t hi = be < wend ? be : wend;
    if (hi <= lo) continue;
    const uint32_t cnt = (uint32_t)(hi - lo);
    for (uint32_t d = threadIdx.x; d < P; d += THREADS) lh[d] = 0;
    WIN w[KPT_];
    uint32_t h8[KPT_];               // RP_SPLIT_IN: the byte plane
#pragma unroll
    for (int u = 0; u < KPT_; u++) {
      const uint32_t i = threadIdx.x + (uint32_t)u * THREADS;
      w[u] = i < cnt ? in[lo + i] : 0;
      if (FORM == RP_SPLIT_IN) h8[u] = i < cnt ? reinterpret_cast<const uint8_t *>(in_)[lv.hi_off + lo + i] : 0;
    }
    __syncthreads();
    uint32_t dr[KPT_];               // digit << 16 | rank inside the digit (rank < SHK_RP_TILE)
    WST x[KPT_];                     // the key as it is staged
#pragma unroll
    for (int u = 0; u < KPT_; u++) {
      const uint32_t i = threadIdx.x + (uint32_t)u * THREADS;
      dr[u] = 0;
      x[u] = (WST)w[u];
      if (i < cnt) {
        uint32_t d;
        if (FORM == RP_NARROW_IN) d = (uint32_t)(w[u] >> (16 + lv.cb));
        else if (FORM == RP_SPLIT_IN) {
          // (the digit's top bit is bit kb - 1 of the record: no chunk bit gets into it)
          d = ((uint32_t)w[u] >> (16 + lv.shift)) & (P - 1);
          x[u] = (WST)shk_split_to_narrow((uint32_t)w[u], h8[u], lv.kb, lv.cb);
        } else d = (shk_word_region(w[u], lv.hb, lv.q_lo) >> lv.shift) & (P - 1);
        if (FORM == RP_NARROW_OUT) {
          const uint64_t key = lv.hb >= 64 ? w[u] : (w[u] & ((1ULL << lv.hb) - 1));
          if ((key >> 8) - lv.q_lo >= lv.nslots) atomicOr(err, SHK_E_CORRUPT);
          x[u] = (WST)shk_narrow_rec(w[u], lv.hb, lv.q_lo, lv.cb);
        }
        dr[u] = (d << 16) | atomicAdd(&lh[d], 1u);
      }
    }
    __syncthreads();
    // exclusive scan of the digit counts (P <= 1024)
    uint32_t carry = 0;
    for (uint32_t d0 = 0; d0 < P; d0 += THREADS) {
      uint32_t d = d0 + threadIdx.x;
      uint32_t v = d < P ? lh[d] : 0, tot;
      uint32_t ex = shk_block_exscan(v, &tot, scratch);
      if (d < P) {
        lbase[d] = carry + ex;
        if (lv.ablate & 1) gbase[d] = cursor[((uint64_t)b * P + d) << lv.ng_log2] + (uint64_t)(blockIdx.x % 1024) * 24;
        else gbase[d] = v ? atomicAdd((unsigned long long *)&cursor[((((uint64_t)b * P) + d) << lv.ng_log2) | (blockIdx.x & ((1u << lv.ng_log2) - 1))], (unsigned long long)v) : 0;
        if (lv.slot_cap && v && gbase[d] + v > ((uint64_t)b * P + d + 1) * lv.slot_cap) {
          atomicOr(err, lv.out32 ? SHK_E_SLOT_FULL : SHK_E_SLOT_FULL_UP);
          gbase[d] = ~0ULL;              // (nothing of this run is written)
        }
      }
      carry += tot;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < KPT_; u++) {
      const uint32_t i = threadIdx.x + (uint32_t)u * THREADS;
      if (i < cnt) stage[lbase[dr[u] >> 16] + (dr[u] & 0xFFFFu)] = x[u];
    }
    __syncthreads();
    if (NOUT) {
      // the staged record no longer holds this level's digit: a wave takes whole digit runs (lh[] still holds their lengths).
      // This trades balance for not keeping the digit: a run that is no multiple of 64 records leaves lanes idle (hash
      // values: 128 runs of ~128 records over 16 waves here), and a batch whose keys crowd into one digit is written by one
      // wave. Staging dr >> 16 next to the record would restore the flat loop for 1-2 more bytes of LDS per key.
      uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
      for (uint32_t d = threadIdx.x / SHK_WAVE; d < P; d += THREADS / SHK_WAVE) {
        const uint32_t l0 = lbase[d], len = lh[d];
        const uint64_t g0 = gbase[d];
        if (g0 == ~0ULL) continue;     // (a slotted level: the run did not fit)
        for (uint32_t j = threadIdx.x % SHK_WAVE; j < len; j += SHK_WAVE) out32[g0 + j] = stage[l0 + j];
      }
    } else {
      for (uint32_t i = threadIdx.x; i < cnt; i += THREADS) {
        const WST xs = stage[i];
        if (FORM == RP_NARROW_IN) {
          // the record the rebuild reads, bit for bit the one the 8-byte path writes below
          const uint32_t d = xs >> (16 + lv.cb);
          const uint32_t rec = (((uint32_t)(xs >> lv.cb) & 0xFFFFu) << SHK_CHUNK_BITS) | ((uint32_t)xs & ((1u << lv.cb) - 1));
          if (gbase[d] != ~0ULL) reinterpret_cast<uint32_t *>(out)[gbase[d] + (i - lbase[d])] = rec;
          continue;
        }
        const uint64_t x64 = xs;
        uint32_t d = (shk_word_region(x64, lv.hb, lv.q_lo) >> lv.shift) & (P - 1);
        if (lv.out32) {
          // behind the last level a word's region is its bucket: the rebuild kernel only needs the
          // quotient inside the region, the remainder and the chunk -- half the bytes, no 64-bit arithmetic
          const uint64_t key = lv.hb >= 64 ? x64 : (x64 & ((1ULL << lv.hb) - 1));
          const uint64_t q = (key >> 8) - lv.q_lo;
          if (q >= lv.nslots) atomicOr(err, SHK_E_CORRUPT);
          const uint32_t rec = ((((uint32_t)q & (SHK_REGION - 1)) << 8 | (uint32_t)(key & 0xff)) << SHK_CHUNK_BITS) |
                               ((uint32_t)(x64 >> lv.hb) & (SHK_MAX_CHUNKS - 1));
          if (gbase[d] != ~0ULL) reinterpret_cast<uint32_t *>(out)[gbase[d] + (i - lbase[d])] = rec;
        } else {
          out[gbase[d] + (i - lbase[d])] = x64;
        }
      }
    }
    shk_lds_barrier();             // (LDS only: the runs just written drain to HBM behind it)
  }
}
