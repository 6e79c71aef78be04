// Device-side helpers shared by the kernels: wave/workgroup scans, unaligned
// access to the packed 89-byte qfblock image, the counter codec.
// gfx950 only: wavefront = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SHK_WAVE 64
#define SHK_MAX_WAVES 16      // workgroups are at most 1024 threads
#define SHK_BLOCK_BYTES 89    // reference qfblock at bits_per_slot = 8: cqf/gqf.c:63-86
#define SHK_OFF_OCC 1         // occupieds word
#define SHK_OFF_RUN 9         // runends word
#define SHK_OFF_TRAV 17       // traveled word
#define SHK_OFF_SLOTS 25      // 64 one-byte slots

// One region = the quotients one workgroup owns in the merge kernels.
#define SHK_REGION_LOG2 8
#define SHK_REGION (1u << SHK_REGION_LOG2)             // 256 quotients = 4 blocks, rebuilt by ONE wave
#define SHK_REGION_BLOCKS (SHK_REGION / 64)
#define SHK_IMG_BLOCKS 24                              // LDS image: own 4 blocks + 20 spill blocks
#define SHK_IMG_SLOTS (SHK_IMG_BLOCKS * 64)            // 1536 slots
#define SHK_IMG_BLOCKS_BIG 64                          // retry size for longer clusters (4096 slots)
#define SHK_IMG_BYTES (SHK_IMG_BLOCKS * SHK_BLOCK_BYTES)
#define SHK_HCAP_LOG2 9
#define SHK_HCAP (1u << SHK_HCAP_LOG2)                 // LDS hash capacity (distinct new keys per region)
#define SHK_MERGE_THREADS 64                           // the rebuild kernels run one wave per region ...
#define SHK_MERGE_GROUP 128                            // ... helped by one more wave while staging and folding the batch keys (the kernel is bound by instruction issue: more helpers only add instructions)
#define SHK_CHUNK_BITS 12                              // chunk index field of a key word
#define SHK_MAX_CHUNKS (1u << SHK_CHUNK_BITS)

// error bits raised by kernels (ctx->d_err), reported through the C ABI
#define SHK_E_OLD_EXTENT   (1u << 0)   // a region's old runs spill further than the LDS image
#define SHK_E_NEW_EXTENT   (1u << 1)   // a region's new runs spill further than the LDS image
#define SHK_E_HASH_FULL    (1u << 2)   // more distinct new keys in one region than SHK_HCAP
#define SHK_E_TABLE_FULL   (1u << 3)   // runs would pass xnslots
#define SHK_E_CORRUPT      (1u << 4)   // occupieds/runends disagree
#define SHK_E_BAD_FASTQ    (1u << 5)   // read longer than 65535 / k out of range
#define SHK_E_KEYS_FULL    (1u << 6)   // batch produced more keys than the key buffer holds
#define SHK_E_RUN_TOO_LONG (1u << 7)
#define SHK_E_SLOT_FULL_UP (1u << 8)   // a slotted level ABOVE the last one (k_roll_scatter, the middle k_rp_scatter): a bucket got more words than its
                                       // slot holds (host runs the batch's front end again with counted bases). Apart from SHK_E_SLOT_FULL, whose redo
                                       // is the last level alone. (The flags keep their numbers: shk/__init__.py hard-codes some)
#define SHK_E_FUSED        (1u << 9)   // the one-pass deNoise point met a region it does not handle (host takes the three-pass path)
#define SHK_E_SLOT_FULL    (1u << 10)  // last partition level with fixed-capacity region slots: a region got more words (host redoes the level with exact bases)

__device__ __forceinline__ unsigned shk_lane() { return threadIdx.x & (SHK_WAVE - 1); }
__device__ __forceinline__ unsigned shk_wave() { return threadIdx.x / SHK_WAVE; }

__device__ __forceinline__ uint64_t shk_rol64(uint64_t v, unsigned s) {
  s &= 63;
  return s ? (v << s) | (v >> (64 - s)) : v;
}
__device__ __forceinline__ uint64_t shk_ror64(uint64_t v, unsigned s) {
  s &= 63;
  return s ? (v >> s) | (v << (64 - s)) : v;
}

// keys per window of the FIRST partition level: 16384 = what one workgroup can stage in LDS. Its 128 output streams lie
// pages apart and three of four digit-run stores of a 4096-key window missed the first-level TLB (19.5 M misses per
// launch against 30 k in the later levels, whose streams stay inside one bucket): longer runs = fewer misses per key.
// Measured on 832 M keys: 4.7 ms (4096) -> 3.6 (8192) -> 2.7 ms (16384). The later levels keep 4096-key windows
// (SHK_RP_TILE): 8192 made them slower.
#define SHK_RP_TILE0_LOG2 14

// Workgroup barrier that orders LDS accesses only: global stores issued before it may still be in flight behind it (a
// __syncthreads() waits for them too: vmcnt(0)). For the scatter kernels, whose windows reuse LDS buffers while the runs
// they have just written drain to HBM.
__device__ __forceinline__ void shk_lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#else
  __syncthreads();
#endif
}

// ---- wave scans (64 lanes, shuffle based)
// LDS writes of this wave's lanes become visible to its other lanes (a barrier among the 64 lanes only)
__device__ __forceinline__ void shk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Inclusive scans over the 64 lanes with DPP moves (VALU only: __shfl_up would be a ds_bpermute per step, and the LDS
// pipeline is what the rebuild kernel keeps busiest): Hillis-Steele inside each row of 16 lanes (row_shr 1,2,4,8), then
// row_bcast15 / row_bcast31 carry the row totals across rows (GFX9 DPP modes, present on gfx950). A lane without a source
// (or in a row the step does not touch) receives the operation's identity.
#define SHK_DPP_STEPS(STEP) STEP(0x111, 0xf) STEP(0x112, 0xf) STEP(0x114, 0xf) STEP(0x118, 0xf) STEP(0x142, 0xa) STEP(0x143, 0xc)
__device__ __forceinline__ uint32_t shk_wave_incl_add(uint32_t x) {
#define SHK_STEP_(ctrl, rows) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, rows, 0xf, true);
  SHK_DPP_STEPS(SHK_STEP_)
#undef SHK_STEP_
  return x;
}
__device__ __forceinline__ uint64_t shk_wave_incl_add64(uint64_t x) {
#define SHK_STEP_(ctrl, rows) { const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, ctrl, rows, 0xf, true); \
                              const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), ctrl, rows, 0xf, true); \
                              x += ((uint64_t)hi_ << 32) | lo_; }
  SHK_DPP_STEPS(SHK_STEP_)
#undef SHK_STEP_
  return x;
}
// Inclusive XOR scan over the 64 lanes with DPP moves (no LDS crossbar): Hillis-Steele inside
// each row of 16 lanes (row_shr 1,2,4,8), then row_bcast15 / row_bcast31 carry the row totals
// across rows (GFX9 DPP modes, present on gfx950).
__device__ __forceinline__ uint32_t shk_dpp_xor_scan32(uint32_t x) {
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);  // row_shr:1
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);  // row_shr:2
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);  // row_shr:4
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);  // row_shr:8
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, true);  // row_bcast:15 -> rows 1,3
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, true);  // row_bcast:31 -> rows 2,3
  return x;
}
__device__ __forceinline__ uint64_t shk_wave_incl_xor64(uint64_t x) {
  const uint32_t lo = shk_dpp_xor_scan32((uint32_t)x), hi = shk_dpp_xor_scan32((uint32_t)(x >> 32));
  return ((uint64_t)hi << 32) | lo;
}
// value of lane 63, as a wave-uniform scalar
__device__ __forceinline__ uint64_t shk_last_lane64(uint64_t x) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}

// ---- workgroup exclusive scan of one u32 per thread. `scratch` is SHK_MAX_WAVES+1 words of LDS.
// Returns the exclusive prefix; *total gets the workgroup sum. Ends with a barrier.
__device__ __forceinline__ uint32_t shk_block_exscan(uint32_t v, uint32_t *total, uint32_t *scratch) {
  unsigned lane = shk_lane(), wave = shk_wave(), nw = blockDim.x / SHK_WAVE;
  uint32_t incl = shk_wave_incl_add(v);
  if (lane == SHK_WAVE - 1) scratch[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    uint32_t w = lane < nw ? scratch[lane] : 0;
    uint32_t wi = shk_wave_incl_add(w);
    if (lane < nw) scratch[lane] = wi - w;
    if (lane == nw - 1) scratch[SHK_MAX_WAVES] = wi;
  }
  __syncthreads();
  uint32_t res = scratch[wave] + incl - v;
  *total = scratch[SHK_MAX_WAVES];
  __syncthreads();
  return res;
}
__device__ __forceinline__ uint64_t shk_block_exscan64(uint64_t v, uint64_t *total, uint64_t *scratch) {
  unsigned lane = shk_lane(), wave = shk_wave(), nw = blockDim.x / SHK_WAVE;
  uint64_t incl = shk_wave_incl_add64(v);
  if (lane == SHK_WAVE - 1) scratch[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    uint64_t w = lane < nw ? scratch[lane] : 0;
    uint64_t wi = shk_wave_incl_add64(w);
    if (lane < nw) scratch[lane] = wi - w;
    if (lane == nw - 1) scratch[SHK_MAX_WAVES] = wi;
  }
  __syncthreads();
  uint64_t res = scratch[wave] + incl - v;
  *total = scratch[SHK_MAX_WAVES];
  __syncthreads();
  return res;
}
// workgroup sum of one u64 per thread (result valid in every thread). Ends with a barrier.
__device__ __forceinline__ uint64_t shk_block_sum64(uint64_t v, uint64_t *scratch) {
  uint64_t t;
  shk_block_exscan64(v, &t, scratch);
  return t;
}

// ---- "free pointer" functions f -> max(f + a, b): how a sequence of runs moves the
// first free slot (a = total run length, b = where it ends when nothing spills in).
// Composition is associative; identity is (0, -inf).
#define SHK_NEG_INF (-(1LL << 60))
struct ShkMP {
  long long a, b;
};
__device__ __forceinline__ ShkMP shk_mp_compose(ShkMP first, ShkMP second) {
  ShkMP r;
  r.a = first.a + second.a;
  long long t = first.b + second.a;
  r.b = t > second.b ? t : second.b;
  if (r.b < SHK_NEG_INF) r.b = SHK_NEG_INF;
  return r;
}
__device__ __forceinline__ long long shk_mp_apply(ShkMP m, long long f) {
  long long t = f + m.a;
  return t > m.b ? t : m.b;
}

// the same in 32 bits, for values relative to a region start (k_region_merge: a <= slots of one region's runs, b <= 256 + a)
#define SHK_NEG_INF_W (-(1 << 28))
struct ShkMPw {
  int a, b;
};
__device__ __forceinline__ ShkMPw shk_mpw_compose(ShkMPw first, ShkMPw second) {
  ShkMPw r;
  r.a = first.a + second.a;
  const int t = first.b + second.a;
  r.b = t > second.b ? t : second.b;
  if (r.b < SHK_NEG_INF_W) r.b = SHK_NEG_INF_W;
  return r;
}

// inclusive scan of f -> max(f + a, b) functions over the 64 lanes in lane order (lane 0's function is applied first)
__device__ __forceinline__ ShkMPw shk_mpw_wave_scan(ShkMPw x) {
#define SHK_STEP_(ctrl, rows) { ShkMPw y_; y_.a = __builtin_amdgcn_update_dpp(0, x.a, ctrl, rows, 0xf, true); \
                              y_.b = __builtin_amdgcn_update_dpp(SHK_NEG_INF_W, x.b, ctrl, rows, 0xf, false); \
                              x = shk_mpw_compose(y_, x); }
  SHK_DPP_STEPS(SHK_STEP_)
#undef SHK_STEP_
  return x;
}

// ---- bytes of the packed block image (global or LDS): unaligned little-endian access
__device__ __forceinline__ uint64_t shk_ld64(const uint8_t *p) {
  uint64_t v = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
__device__ __forceinline__ void shk_st64(uint8_t *p, uint64_t v) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// position of the n-th (0-based) set bit of w; 64 when there are not that many
__device__ __forceinline__ unsigned shk_select64(uint64_t w, unsigned n) {
  if ((unsigned)__popcll(w) <= n) return 64;
  unsigned pos = 0;
#pragma unroll
  for (int width = 32; width >= 1; width >>= 1) {
    uint64_t low = w & ((1ULL << width) - 1);
    unsigned c = (unsigned)__popcll(low);
    if (n >= c) { n -= c; w >>= width; pos += width; } else { w = low; }
  }
  return pos;
}

// ---- counter codec, cqf/gqf.c:1225-1255 (encode_counter) at bits_per_slot = 8:
// count 1 -> [r]; count c+1 >= 2 -> [r, (0 if top digit > r), d_m|0x80 .. d_1|0x80, d_0],
// base-128 digits of c.
__device__ __forceinline__ unsigned shk_enc_len(unsigned rem, uint64_t count) {
  if (count <= 1) return (unsigned)count;
  uint64_t c = count - 1;
  unsigned nd = 1;
  uint64_t t = c >> 7;
  while (t) { nd++; t >>= 7; }
  unsigned top = (unsigned)((c >> (7 * (nd - 1))) & 0x7f);
  if (nd > 1) top |= 0x80;
  return 1 + nd + (top > rem ? 1 : 0);
}
// writes the encoding to dst[0..len) and returns len
__device__ __forceinline__ unsigned shk_enc_write(uint8_t *dst, unsigned rem, uint64_t count) {
  dst[0] = (uint8_t)rem;
  if (count <= 1) return 1;
  uint64_t c = count - 1;
  unsigned nd = 1;
  uint64_t t = c >> 7;
  while (t) { nd++; t >>= 7; }
  unsigned top = (unsigned)((c >> (7 * (nd - 1))) & 0x7f);
  if (nd > 1) top |= 0x80;
  unsigned n = 1;
  if (top > rem) dst[n++] = 0;
  for (int i = (int)nd - 1; i >= 1; i--) dst[n++] = (uint8_t)(((c >> (7 * i)) & 0x7f) | 0x80);
  dst[n++] = (uint8_t)(c & 0x7f);
  return n;
}
// decode_counter, cqf/gqf.c:1259-1299, over a byte image of slots. `is_last` = the
// entry's first slot carries the runend bit. Returns the number of slots the entry takes.
__device__ __forceinline__ unsigned shk_dec(const uint8_t *s, bool first_is_runend, uint64_t *count) {
  unsigned rem = s[0];
  if (first_is_runend) { *count = 1; return 1; }
  unsigned digit = s[1];
  if (digit > rem) { *count = 1; return 1; }
  unsigned n = 1;
  uint64_t cnt = 0;
  if (digit == 0) { n++; digit = s[n]; }
  while (digit & 0x80) { cnt = cnt * 128 + (digit & 0x7f); n++; digit = s[n]; }
  cnt = cnt * 128 + digit;
  *count = cnt + 1;
  return n + 1;
}

// ---- Contiger's k-mers: 2 bits per base (A,C,G,T = 0..3) in W 64-bit words, the value of the base-4 number
// s0 s1 .. s(k-1), so the first base sits in the highest used bits, at bit 2(k-1); word 0 holds the lowest 64 bits.
// W = 2 holds k <= 64 (the unsigned __int128 of earlier versions, word for word), 4 k <= 128, 6 k <= 192. k stays a runtime
// value: every loop over the words unrolls on the compile-time W, and what depends on k (the first base's word, the mask,
// the shift of the reverse complement) is a select per word inside those loops -- no per-thread array is ever indexed at
// run time, so the windows live in registers.
#define SHK_KM_WMAX 6
template <int W> struct ShkKmer { uint64_t w[W]; };

template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_zero() {
  ShkKmer<W> a;
#pragma unroll
  for (int j = 0; j < W; j++) a.w[j] = 0;
  return a;
}
// the 2k low bits set
template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_mask(uint32_t k) {
  ShkKmer<W> m;
#pragma unroll
  for (int j = 0; j < W; j++) {
    const int bits = 2 * (int)k - 64 * j;
    m.w[j] = bits >= 64 ? ~0ULL : bits <= 0 ? 0ULL : ((1ULL << bits) - 1);
  }
  return m;
}
// (a << 2) | c, not masked (packing from text: the value never exceeds 2k bits)
template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_push(const ShkKmer<W> &a, unsigned c) {
  ShkKmer<W> r;
#pragma unroll
  for (int j = W - 1; j > 0; j--) r.w[j] = (a.w[j] << 2) | (a.w[j - 1] >> 62);
  r.w[0] = (a.w[0] << 2) | c;
  return r;
}
// append a base: ((a << 2) | c) & mask
template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_append(const ShkKmer<W> &a, unsigned c, const ShkKmer<W> &mask) {
  ShkKmer<W> r = shk_km_push(a, c);
#pragma unroll
  for (int j = 0; j < W; j++) r.w[j] &= mask.w[j];
  return r;
}
// the base at 2-bit position p (0 = the last base, k - 1 = the first)
template <int W> __device__ __forceinline__ unsigned shk_km_base(const ShkKmer<W> &a, uint32_t p) {
  const uint32_t wi = p >> 5, sh = 2 * (p & 31);
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < W; j++) c = (uint32_t)j == wi ? (unsigned)(a.w[j] >> sh) & 3u : c;
  return c;
}
// (a >> 2) with base c inserted at position k - 1 (the first base)
template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_push_top(const ShkKmer<W> &a, unsigned c, uint32_t k) {
  const uint32_t wi = (k - 1) >> 5, sh = 2 * ((k - 1) & 31);
  ShkKmer<W> r;
#pragma unroll
  for (int j = 0; j < W - 1; j++) r.w[j] = (a.w[j] >> 2) | (a.w[j + 1] << 62);
  r.w[W - 1] = a.w[W - 1] >> 2;
#pragma unroll
  for (int j = 0; j < W; j++) r.w[j] |= (uint32_t)j == wi ? (uint64_t)c << sh : 0ULL;
  return r;
}
// the last base replaced by c
template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_set_last(ShkKmer<W> a, unsigned c) {
  a.w[0] = (a.w[0] & ~3ULL) | c;
  return a;
}
template <int W> __device__ __forceinline__ bool shk_km_eq(const ShkKmer<W> &a, const ShkKmer<W> &b) {
  bool e = true;
#pragma unroll
  for (int j = 0; j < W; j++) e = e && a.w[j] == b.w[j];
  return e;
}
// reverse complement: complement, reverse the 2-bit groups of every word and the order of the words (the k-mer then
// fills the top 2k bits), then shift right by 64 W - 2k
template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_rc(const ShkKmer<W> &a, uint32_t k) {
  uint64_t t[W];
#pragma unroll
  for (int j = 0; j < W; j++) {
    uint64_t x = ~a.w[W - 1 - j];
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
    t[j] = __builtin_bswap64(x);
  }
  const uint32_t s = 64 * W - 2 * k, q = s >> 6, b = s & 63;
  ShkKmer<W> r;
#pragma unroll
  for (int j = 0; j < W; j++) {
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int qq = 0; qq < W; qq++) {
      if ((uint32_t)qq == q) {
        lo = j + qq < W ? t[j + qq] : 0ULL;
        hi = j + qq + 1 < W ? t[j + qq + 1] : 0ULL;
      }
    }
    r.w[j] = b ? (lo >> b) | (hi << (64 - b)) : lo;
  }
  return r;
}
// the start-k-mer map's hash; at W = 2 the mix of the two halves that the 128-bit keys always had (same probe order)
__device__ __forceinline__ uint64_t shk_ug_mix(uint64_t lo, uint64_t hi) {
  uint64_t h = lo * 0x9E3779B97F4A7C15ULL ^ (hi + 0x7F4A7C159E3779B9ULL) * 0xC2B2AE3D27D4EB4FULL;
  h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ULL; h ^= h >> 32;
  return h;
}
template <int W> __device__ __forceinline__ uint64_t shk_km_mix(const ShkKmer<W> &a) {
  static_assert(W % 2 == 0, "pairs of words");
  uint64_t h = shk_ug_mix(a.w[0], a.w[1]);
#pragma unroll
  for (int j = 2; j < W; j += 2) h = shk_ug_mix(h ^ a.w[j], a.w[j + 1]);
  return h;
}
// word planes: plane j holds word j of every entry (neighbouring entries stay coalesced)
template <int W> __device__ __forceinline__ ShkKmer<W> shk_km_load(uint64_t *const (&p)[SHK_KM_WMAX], size_t i) {
  ShkKmer<W> a;
#pragma unroll
  for (int j = 0; j < W; j++) a.w[j] = p[j][i];
  return a;
}
template <int W> __device__ __forceinline__ void shk_km_store(uint64_t *const (&p)[SHK_KM_WMAX], size_t i, const ShkKmer<W> &a) {
#pragma unroll
  for (int j = 0; j < W; j++) p[j][i] = a.w[j];
}
