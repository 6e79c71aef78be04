// FASTA text of any shape -> the input of the packed roll form (roll_kernels.hip: pk, pk_base, pk_flag, read extents),
// so that shk_count_fasta hashes with the kernels shk_count_chunks uses and adds no hash kernel of its own.
//
// The grammar (include/shk.h, shk_count_fasta): a line whose first byte is '>' or ';' is a header line; in every other
// line '\n' and '\r' are skipped, A C G T (either case) are bases and every other byte is a break; a header line is a
// break too. A RUN is a maximal sequence of bases with nothing but line ends between them; the k-mers counted are those of
// the runs. Nothing here looks for records: a piece of text may begin and end anywhere, what it needs to know about the
// text in front of it is one of six states,
//     line state (0 inside a header line, 1 at a line start, 2 inside a sequence line)  x  pending (a break lies behind
//     the last base, so the next base opens a run)
// plus the last <= k-1 bases of the run that is still open (the TAIL, kept on the device by the host side).
//
// Stages; every dependency between tiles is a kernel boundary (no workgroup ever waits for another):
//   k_fa_maps      a thread takes 16 text bytes (one aligned load), turns them into bit masks (shk_fa_masks: no loop over
//                  the bytes, no branch on them) and finds the MAP they are over the six states; the maps
//                  of a tile (blockDim x 16 bytes) are composed -- composition of maps is associative -- into one word
//   k_fa_states    one workgroup composes the tiles' maps in text order: the state in which every tile begins
//   k_fa_count     the tile pass proper: states of the threads, classes of the bytes; per tile the number of bases and of
//                  run starts (summed by the host side's run_scan), per thread its state (one byte per 16 of text)
//   k_fa_compact   the bases as one 2-bit stream behind the tail, and the list of run starts in base coordinates
//   k_fa_segments (+ k_fa_long_segments)  every run of >= k bases is cut into segments of `seg` k-mers (seg + k - 1 bases, overlapping by k - 1):
//                  one segment = one "read" of the roll kernels, i.e. one thread's work there
//   k_fa_pack      the segments' 64-base units, funnel-shifted out of the stream (a segment starts at any 2-bit offset)
//   k_fa_tail      the new tail
#include "shk_device.h"

#define SHK_FA_STATES 6
#define SHK_FA_MAP_ID 0x2C688u                 // state s -> s: sum of s << 3s
#define SHK_FA_STATE_START 3u                  // line start, pending: where a file begins
#define SHK_FA_COUNT_BITS 36                   // a tile's word: bases | run starts << 36 (and their sums over a piece)
#define SHK_FA_COUNT_MASK ((1ULL << SHK_FA_COUNT_BITS) - 1)
#define SHK_FA_LONG_RUN 8                      // k_fa_segments: a run of more segments is left to k_fa_long_segments (the whole grid)
#define SHK_FA_LONG_WORDS 5                    // ... as a record of this many words: start, length, first segment, first unit, segments
enum { FA_NBREAK, FA_NREC, FA_END_STATE, FA_NSEG, FA_NUNITS, FA_NKMERS, FA_TAIL_LEN, FA_NLONG, FA_NCOUNTERS };

__device__ __forceinline__ uint32_t shk_fa_apply(uint32_t m, uint32_t s) { return (m >> (3 * s)) & 7u; }
// first a, then b
__device__ __forceinline__ uint32_t shk_fa_compose(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t s = 0; s < SHK_FA_STATES; s++) r |= shk_fa_apply(b, shk_fa_apply(a, s)) << (3 * s);
  return r;
}

// What a thread's 16 bytes are, one bit per byte (bits from nvalid on are clear): line feeds, carriage returns, bytes that
// would open a header at a line start ('>' ';'), bases (either case)
struct ShkFaMasks { uint32_t nl, cr, hd, base, valid; };
// the 0x80 flags of shk_zero_bytes, one per byte of a word, as four neighbouring bits
__device__ __forceinline__ uint32_t shk_fa_gather(uint32_t x) { return (((x >> 7) * 0x204081u) >> 21) & 0xFu; }
__device__ __forceinline__ ShkFaMasks shk_fa_masks(const ShkQuad &v, uint32_t nvalid) {
  const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
  ShkFaMasks M = {0, 0, 0, 0, nvalid >= 16 ? 0xFFFFu : (1u << nvalid) - 1};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t w = wd[q], y = w & 0xDFDFDFDFu;
    M.nl |= shk_fa_gather(shk_zero_bytes(w ^ 0x0A0A0A0Au)) << (4 * q);
    M.cr |= shk_fa_gather(shk_zero_bytes(w ^ 0x0D0D0D0Du)) << (4 * q);
    M.hd |= shk_fa_gather(shk_zero_bytes(w ^ 0x3E3E3E3Eu) | shk_zero_bytes(w ^ 0x3B3B3B3Bu)) << (4 * q);
    M.base |= shk_fa_gather(shk_zero_bytes(y ^ 0x41414141u) | shk_zero_bytes(y ^ 0x43434343u) | shk_zero_bytes(y ^ 0x47474747u) |
                            shk_zero_bytes(y ^ 0x54545454u)) << (4 * q);
  }
  M.nl &= M.valid; M.cr &= M.valid; M.hd &= M.valid; M.base &= M.valid;
  return M;
}

struct ShkFaWalk {
  uint32_t nbase, nbreak, nrec;   // bases, break bytes, header lines begun
  uint32_t basemask, startmask;   // bytes that are bases; those of them that open a run
  uint32_t openmask;              // first bytes of the header lines begun (query_kernels.hip: the records' starts)
};
// The bytes behind M from state st on; returns the state behind them. All 16 bytes at once, on the masks:
//   header bytes   a header opens at a line start (behind a line feed, or byte 0 in state "line start") that holds '>' or
//                  ';', or is open already (state "header": as if byte 0 opened one), and runs up to the next line feed.
//                  Subtracting the openers from the line feeds (and one more behind the last byte) borrows through exactly
//                  those bytes; line feeds that close nothing stay set and are masked away;
//   run starts     a base opens a run when the event in front of it is a break (a break byte, a header's first byte, or
//                  `pending` for the first event). Adding the breaks, shifted up by one, to the bytes that are no events
//                  carries each break through the gap behind it onto the next event.
__device__ __forceinline__ uint32_t shk_fa_walk(const ShkFaMasks &M, uint32_t st, ShkFaWalk *out) {
  const uint32_t ls = st >> 1, pend = st & 1u;
  ShkFaWalk r = {0, 0, 0, 0, 0, 0};
  *out = r;
  if (!M.valid) return st;
  const uint32_t opens = ((M.nl << 1) | (uint32_t)(ls == 1)) & M.hd;
  const uint32_t hdr = (((M.nl | 0x10000u) - (opens | (uint32_t)(ls == 0))) & ~M.nl) & M.valid;
  const uint32_t seq = M.valid & ~hdr & ~M.nl & ~M.cr;
  const uint32_t e = seq & M.base, b = seq & ~M.base, bev = b | opens, ev = e | bev;
  const uint32_t gaps = ~ev & 0x1FFFFu;
  r.nbase = (uint32_t)__popc(e); r.nbreak = (uint32_t)__popc(b); r.nrec = (uint32_t)__popc(opens);
  r.basemask = e; r.openmask = opens;
  r.startmask = (((bev << 1) | pend) + gaps) & e;
  *out = r;
  const uint32_t last = M.valid ^ (M.valid >> 1);      // the last byte
  const uint32_t ls_out = (M.nl & last) ? 1u : (hdr & last) ? 0u : 2u;
  return ls_out * 2 + (ev ? (uint32_t)(bev > e) : pend);
}
// the 2-bit codes of the bytes in basemask, first base lowest
__device__ __forceinline__ uint32_t shk_fa_codes(const ShkQuad &v, uint32_t basemask) {
  const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
  uint32_t codes = 0, n = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t c = wd[j >> 2] >> (8 * (j & 3)), bit = (basemask >> j) & 1u;
    codes |= ((((c >> 1) ^ (c >> 2)) & 3u) & (0u - bit)) << (2 * n);
    n += bit;
  }
  return codes;
}
// the map of 16 bytes: one walk per line state; the pending bit passes through bytes that hold no base, no break and no
// header start, and is the walk's own behind any other
__device__ __forceinline__ uint32_t shk_fa_map16(const ShkFaMasks &M) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t ls = 0; ls < 3; ls++) {
    ShkFaWalk w;
    const uint32_t o = shk_fa_walk(M, ls * 2, &w);
    const bool touched = (w.nbase | w.nbreak | w.nrec) != 0;
    m |= o << (6 * ls);
    m |= (touched ? o : (o | 1u)) << (6 * ls + 3);
  }
  return m;
}
// inclusive scan of one map per thread in thread order: Hillis-Steele over the wave's 64 lanes by shuffles, the waves'
// maps through LDS (`arr` = SHK_MAX_WAVES words); *excl = the map of all threads in front of this one. Every thread of the
// workgroup calls it; ends with a barrier.
__device__ __forceinline__ uint32_t shk_fa_scan_maps(uint32_t m, uint32_t *arr, uint32_t *excl) {
  const uint32_t lane = shk_lane(), wave = shk_wave();
  uint32_t v = m;
#pragma unroll
  for (uint32_t d = 1; d < SHK_WAVE; d <<= 1) {
    const uint32_t u = __shfl_up(v, d);
    if (lane >= d) v = shk_fa_compose(u, v);
  }
  const uint32_t before = __shfl_up(v, 1u);
  if (lane == SHK_WAVE - 1) arr[wave] = v;
  __syncthreads();
  uint32_t wp = SHK_FA_MAP_ID;
  for (uint32_t w = 0; w < wave; w++) wp = shk_fa_compose(wp, arr[w]);
  *excl = lane ? shk_fa_compose(wp, before) : wp;
  __syncthreads();
  return shk_fa_compose(wp, v);
}
// this thread's 16 bytes of tile blockIdx.x
__device__ __forceinline__ ShkQuad shk_fa_load(const uint8_t *text, uint64_t n, uint64_t safe_end, uint32_t *nvalid) {
  const uint64_t at = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  *nvalid = at >= n ? 0 : n - at < 16 ? (uint32_t)(n - at) : 16;
  return *nvalid ? shk_load16(text, at, safe_end) : shk_quad(0, 0, 0, 0);
}

__global__ void __launch_bounds__(256) k_fa_maps(const uint8_t *text, uint64_t n, uint64_t safe_end, uint32_t *tile_map) {
  __shared__ uint32_t arr[SHK_MAX_WAVES];
  uint32_t nvalid, ex;
  const ShkQuad v = shk_fa_load(text, n, safe_end, &nvalid);
  const uint32_t incl = shk_fa_scan_maps(shk_fa_map16(shk_fa_masks(v, nvalid)), arr, &ex);
  if (threadIdx.x == blockDim.x - 1) tile_map[blockIdx.x] = incl;
}

// One workgroup: thread t composes its share of the tiles, the shares are scanned, and every thread walks its share again
// from the state it now knows. end_state = the state behind the last tile (st0 for an empty text).
__global__ void __launch_bounds__(1024) k_fa_states(const uint32_t *tile_map, uint64_t ntiles, uint32_t st0, uint32_t *tile_state, uint64_t *end_state) {
  __shared__ uint32_t arr[SHK_MAX_WAVES];
  const uint64_t per = (ntiles + blockDim.x - 1) / blockDim.x;
  const uint64_t lo = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
  uint32_t m = SHK_FA_MAP_ID, ex;
  for (uint64_t i = lo; i < hi; i++) m = shk_fa_compose(m, tile_map[i]);
  shk_fa_scan_maps(m, arr, &ex);
  uint32_t s = shk_fa_apply(ex, st0);
  for (uint64_t i = lo; i < hi; i++) { tile_state[i] = s; s = shk_fa_apply(tile_map[i], s); }
  if (threadIdx.x == blockDim.x - 1) *end_state = s;
}

// tile_rec (null: not wanted) = the header lines begun in every tile, for the scan of shk_query_fasta's record starts
__global__ void __launch_bounds__(256) k_fa_count(const uint8_t *text, uint64_t n, uint64_t safe_end, const uint32_t *tile_state, uint8_t *unit_state,
                                                   uint64_t *tile_cnt, uint64_t *counters, uint64_t *tile_rec) {
  __shared__ uint32_t arr[SHK_MAX_WAVES];
  __shared__ uint64_t scratch[SHK_MAX_WAVES + 1];
  uint32_t nvalid, ex;
  const ShkQuad v = shk_fa_load(text, n, safe_end, &nvalid);
  const ShkFaMasks M = shk_fa_masks(v, nvalid);
  shk_fa_scan_maps(shk_fa_map16(M), arr, &ex);
  const uint32_t st = shk_fa_apply(ex, tile_state[blockIdx.x]);
  if (nvalid) unit_state[(uint64_t)blockIdx.x * blockDim.x + threadIdx.x] = (uint8_t)st;
  ShkFaWalk w;
  shk_fa_walk(M, st, &w);
  // (four sums in one: a tile has at most 1024 x 16 of anything)
  const uint64_t tot = shk_block_sum64((uint64_t)w.nbase | (uint64_t)__popc(w.startmask) << 16 | (uint64_t)w.nbreak << 32 | (uint64_t)w.nrec << 48, scratch);
  if (threadIdx.x == 0) {
    tile_cnt[blockIdx.x] = (tot & 0xFFFFu) | ((tot >> 16) & 0xFFFFu) << SHK_FA_COUNT_BITS;
    if ((tot >> 32) & 0xFFFFu) atomicAdd((unsigned long long *)&counters[FA_NBREAK], (unsigned long long)((tot >> 32) & 0xFFFFu));
    if (tot >> 48) atomicAdd((unsigned long long *)&counters[FA_NREC], (unsigned long long)(tot >> 48));
    if (tile_rec) tile_rec[blockIdx.x] = tot >> 48;
  }
}

// The stream (zeroed by the host side, the tail's `tail` bases in front) takes the tile's bases at tail + tile_off; run
// i >= 1 of the piece starts at run_start[i], run 0 is the one the tail belongs to and starts at 0 (empty when the piece
// opens with a run start and there is no tail), run_start[nruns] = the end of the stream. cap_runs = words of run_start.
__global__ void __launch_bounds__(256) k_fa_compact(const uint8_t *text, uint64_t n, uint64_t safe_end, const uint8_t *unit_state, const uint64_t *tile_off,
                                                     uint64_t ntiles, uint64_t tail, uint32_t *stream, uint64_t stream_words, uint64_t *run_start,
                                                     uint64_t cap_runs, uint32_t *err) {
  __shared__ uint32_t scratch[SHK_MAX_WAVES + 1];
  uint32_t nvalid, tot;
  const ShkQuad v = shk_fa_load(text, n, safe_end, &nvalid);
  ShkFaWalk w = {0, 0, 0, 0, 0, 0};
  if (nvalid) shk_fa_walk(shk_fa_masks(v, nvalid), unit_state[(uint64_t)blockIdx.x * blockDim.x + threadIdx.x], &w);
  const uint32_t ex = shk_block_exscan(w.nbase | (uint32_t)__popc(w.startmask) << 16, &tot, scratch);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t all = tile_off[ntiles], nruns = 1 + (all >> SHK_FA_COUNT_BITS);
    run_start[0] = 0;
    if (nruns < cap_runs) run_start[nruns] = tail + (all & SHK_FA_COUNT_MASK); else atomicOr(err, SHK_E_KEYS_FULL);
  }
  if (blockIdx.x >= ntiles || !w.nbase) return;
  const uint64_t off = tile_off[blockIdx.x];
  const uint64_t g = tail + (off & SHK_FA_COUNT_MASK) + (ex & 0xFFFFu);
  const uint64_t wi = g >> 4;
  const uint64_t bits = (uint64_t)shk_fa_codes(v, w.basemask) << (2 * (uint32_t)(g & 15));
  if (wi + 1 < stream_words) {
    atomicOr(&stream[wi], (uint32_t)bits);
    if (bits >> 32) atomicOr(&stream[wi + 1], (uint32_t)(bits >> 32));
  } else atomicOr(err, SHK_E_KEYS_FULL);
  uint64_t ri = 1 + (off >> SHK_FA_COUNT_BITS) + (ex >> 16);
  for (uint32_t sm = w.startmask; sm; sm &= sm - 1) {
    const uint32_t j = (uint32_t)__ffs((int)sm) - 1;
    if (ri < cap_runs) run_start[ri] = g + (uint32_t)__popc(w.basemask & ((1u << j) - 1));
    ri++;
  }
}

struct ShkFaSegArgs {
  const uint64_t *run_start; uint64_t nruns;
  uint32_t k, seg;
  uint64_t *rd_start, *rd_end; uint16_t *rd_chunk; uint32_t *flag; uint64_t *pk_base;
  uint64_t cap_seg, cap_units;
  uint64_t *long_runs; uint64_t cap_long;      // records of the long runs (SHK_FA_LONG_WORDS words each)
  uint64_t *counters; uint32_t *err;
};
// segment j of a run of `len` bases at `start`, as read A.* [sb + j] with its units from ub + j * (units of a full segment)
__device__ __forceinline__ void shk_fa_put_segment(const ShkFaSegArgs &A, uint64_t start, uint64_t len, uint64_t sb, uint64_t ub, uint64_t j) {
  const uint32_t full = A.seg + A.k - 1;
  const uint64_t left = len - j * A.seg;
  const uint32_t sl = left < full ? (uint32_t)left : full;
  A.rd_start[sb + j] = start + j * A.seg;
  A.rd_end[sb + j] = start + j * A.seg + sl;
  A.rd_chunk[sb + j] = 0;
  A.flag[sb + j] = (sl + 63) >> 6;
  A.pk_base[sb + j] = ub + j * ((full + 63) >> 6);
}
// One run per thread and turn. Segments and units are handed out by one atomic per workgroup and turn (their order is
// free: a bucket's keys are a multiset); a run that does not fit the read arrays or the unit buffer raises
// SHK_E_KEYS_FULL and writes nothing -- the host compares the totals with the capacities anyway. A thread writes the
// segments of a short run itself; a long run (a chromosome: 10^5 segments) becomes a record for k_fa_long_segments, or,
// when the records' buffer is full, is written by this workgroup together.
__global__ void __launch_bounds__(256) k_fa_segments(ShkFaSegArgs A) {
  __shared__ uint64_t scratch[SHK_MAX_WAVES + 1];
  __shared__ uint64_t alloc[2];
  __shared__ uint64_t l_start[256], l_len[256], l_sb[256], l_ub[256], l_ns[256];
  __shared__ uint32_t nlong;
  const uint32_t full = A.seg + A.k - 1, ufull = (full + 63) >> 6;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t turns = (A.nruns + stride - 1) / stride;
  uint64_t kmers = 0;
  for (uint64_t turn = 0; turn < turns; turn++) {
    const uint64_t r = turn * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t start = 0, len = 0, ns = 0, units = 0;
    if (r < A.nruns) {
      start = A.run_start[r];
      len = A.run_start[r + 1] - start;
      if (len >= A.k) {
        const uint64_t nk = len - A.k + 1;
        kmers += nk;
        ns = (nk + A.seg - 1) / A.seg;
        units = (ns - 1) * ufull + ((len - (ns - 1) * A.seg + 63) >> 6);
      }
    }
    uint64_t tot_s, tot_u;
    const uint64_t ex_s = shk_block_exscan64(ns, &tot_s, scratch);
    const uint64_t ex_u = shk_block_exscan64(units, &tot_u, scratch);
    if (threadIdx.x == 0) {
      nlong = 0;
      alloc[0] = tot_s ? atomicAdd((unsigned long long *)&A.counters[FA_NSEG], (unsigned long long)tot_s) : 0;
      alloc[1] = tot_u ? atomicAdd((unsigned long long *)&A.counters[FA_NUNITS], (unsigned long long)tot_u) : 0;
    }
    __syncthreads();
    const uint64_t sb = alloc[0] + ex_s, ub = alloc[1] + ex_u;
    if (ns && (sb + ns > A.cap_seg || ub + units > A.cap_units)) { atomicOr(A.err, SHK_E_KEYS_FULL); ns = 0; }
    if (ns > SHK_FA_LONG_RUN) {
      const uint64_t gi = atomicAdd((unsigned long long *)&A.counters[FA_NLONG], 1ULL);
      if (gi < A.cap_long) {
        uint64_t *rec = A.long_runs + SHK_FA_LONG_WORDS * gi;
        rec[0] = start; rec[1] = len; rec[2] = sb; rec[3] = ub; rec[4] = ns;
      } else {
        const uint32_t i = atomicAdd(&nlong, 1u);
        l_start[i] = start; l_len[i] = len; l_sb[i] = sb; l_ub[i] = ub; l_ns[i] = ns;
      }
    } else {
      for (uint64_t j = 0; j < ns; j++) shk_fa_put_segment(A, start, len, sb, ub, j);
    }
    __syncthreads();
    const uint32_t nl = nlong;
    for (uint32_t i = 0; i < nl; i++)
      for (uint64_t j = threadIdx.x; j < l_ns[i]; j += blockDim.x) shk_fa_put_segment(A, l_start[i], l_len[i], l_sb[i], l_ub[i], j);
    __syncthreads();
  }
  const uint64_t tot_k = shk_block_sum64(kmers, scratch);
  if (threadIdx.x == 0 && tot_k) atomicAdd((unsigned long long *)&A.counters[FA_NKMERS], (unsigned long long)tot_k);
}

// the segments of the long runs, spread over the grid
__global__ void k_fa_long_segments(ShkFaSegArgs A) {
  const uint64_t have = A.counters[FA_NLONG], nl = have < A.cap_long ? have : A.cap_long;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t i = 0; i < nl; i++) {
    const uint64_t *rec = A.long_runs + SHK_FA_LONG_WORDS * i;
    for (uint64_t j = me; j < rec[4]; j += stride) shk_fa_put_segment(A, rec[0], rec[1], rec[2], rec[3], j);
  }
}

// 64 bases of the stream from base `pos` on, as one unit; bases from `nv` on read as zero. The unit lies across two
// neighbouring 16-byte quads of the stream: both are loaded whole and shifted as one 256-bit value.
__device__ __forceinline__ ShkQuad shk_fa_unit(const uint32_t *stream, uint64_t pos, uint32_t nv) {
  const ShkQuad *q = reinterpret_cast<const ShkQuad *>(stream) + (pos >> 6);
  const ShkQuad a = q[0], b = q[1];
  const uint32_t sh = 2 * (uint32_t)(pos & 63), ws = sh >> 5, bs = sh & 31;
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t x[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (uint32_t c = 0; c < 4; c++)
    if (ws == c) {
#pragma unroll
      for (uint32_t i = 0; i < 5; i++) x[i] = w[c + i];
    }
  uint32_t o[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) {
    o[i] = bs ? (x[i] >> bs) | (x[i + 1] << (32 - bs)) : x[i];
    const uint32_t have = 2 * nv > 32 * i ? 2 * nv - 32 * i : 0;      // bits of this word inside the segment
    if (have < 32) o[i] &= (1u << have) - 1;
  }
  return shk_quad(o[0], o[1], o[2], o[3]);
}
// four lanes per segment, one unit per lane and turn (as k_pack_reads)
__global__ void k_fa_pack(const uint32_t *stream, uint64_t nseg, const uint64_t *rd_start, const uint64_t *rd_end, const uint64_t *pk_base,
                          const uint32_t *flag, ShkQuad *pk, uint64_t cap_units, uint32_t *err) {
  const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) >> 2;
  for (uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; r < nseg; r += stride) {
    const uint32_t units = flag[r];
    const uint64_t base = pk_base[r], st = rd_start[r];
    if (base + units > cap_units) { atomicOr(err, SHK_E_KEYS_FULL); continue; }
    const uint32_t len = (uint32_t)(rd_end[r] - st);
    for (uint32_t u = threadIdx.x & 3; u < units; u += 4) pk[base + u] = shk_fa_unit(stream, st + 64 * u, len - 64 * u < 64 ? len - 64 * u : 64);
  }
}

// The tail for the next piece: the last min(k - 1, length) bases of the run the stream ends in, or nothing when a break
// lies behind its last base. Three units (k - 1 <= 190 bases), bases from the tail's length on zero. One wave.
__global__ void k_fa_tail(const uint32_t *stream, const uint64_t *run_start, uint64_t nruns, uint32_t end_state, uint32_t k, ShkQuad *tail_out,
                          uint64_t *counters) {
  const uint64_t total = run_start[nruns], len = total - run_start[nruns - 1];
  const uint32_t tl = (end_state & 1u) ? 0 : len < k - 1 ? (uint32_t)len : k - 1;
  if (threadIdx.x < 3) {
    const uint32_t u = threadIdx.x, nv = tl > 64 * u ? (tl - 64 * u < 64 ? tl - 64 * u : 64) : 0;
    tail_out[u] = nv ? shk_fa_unit(stream, total - tl + 64 * u, nv) : shk_quad(0, 0, 0, 0);
  }
  if (threadIdx.x == 0) counters[FA_TAIL_LEN] = tl;
}
