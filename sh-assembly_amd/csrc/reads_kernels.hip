// shk_query_reads: FASTQ reads against the table -- per read how many of its k-mers the table holds, their smallest,
// largest and (lower) median count, and optionally every window's count. The front end is shk_count_chunks' (parse_stage:
// the reads' extents; pack_stage: the 2-bit units of the reads that are all bases); what is added here:
//   k_reads_windows  windows of every read, max(len - k + 1, 0): scanned, they say where a read's per-window values lie
//   k_reads_query    one thread per read rolls its windows (k_roll_query's recurrence, one base per turn, ONE copy of the
//                    probe loop behind it) and reads every k-mer's count (shk_lookup_one, mark mode 2)
//   k_reads_median   eight lanes per read select the rank-(kmers - 1) / 2 value of the read's window values bit by bit
// The grammar is shk_query_fasta's, not reads_to_kmers': a window is a k-mer exactly when its k bytes are bases.
#include "shk_device.h"

struct ShkReadsArgs {
  const uint8_t *text;
  const uint64_t *rd_start, *rd_end;   // the reads, as k_emit_reads left them (text offsets)
  uint64_t nreads;
  const ShkQuad *pk;                   // 2-bit staging as in ShkRollArgs; null: every read takes its bases from the text
  const uint64_t *pk_base;
  const uint32_t *pk_flag;
  const uint64_t *woff;                // [nreads + 1] windows in front of every read; woff[nreads] <= the entries `win` holds (the host has compared)
  uint32_t k, hb;
  uint8_t *tab; uint64_t q_lo, nslots;
  uint32_t min_count;
  uint32_t median;                     // what the record's median field starts as: 0 (k_reads_median follows) or SHK_QUERY_NONE
  uint32_t *win;                       // null: nothing is written per window. Entry woff[r] + j = window j of read r
  shk_read_record *rec;
  uint64_t *totals;                    // [4] kmers, present, solid, sum of the call, zeroed
};

// A read of more than 65535 bases (SHK_MAX_READ) raises SHK_E_BAD_FASTQ: the host looks before anything else runs
__global__ void k_reads_windows(const uint64_t *rd_start, const uint64_t *rd_end, uint64_t nreads, uint32_t k, uint32_t *nwin, uint32_t *err) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += stride) {
    const uint64_t len = rd_end[r] - rd_start[r];
    if (len > 65535) { atomicOr(err, SHK_E_BAD_FASTQ); nwin[r] = 0; continue; }
    nwin[r] = len >= k ? (uint32_t)(len - k + 1) : 0;
  }
}

// Grid-stride over the reads, a wave's 64 lanes on 64 neighbouring reads. As k_roll_query, the kernel waits for the
// lookups' scattered loads and for nothing else, so it keeps the registers few: the roll runs one base per turn and the
// probe loop is instantiated once. A read whose pk_flag says "all bases" takes its bases from its 2-bit units (no byte of
// it can be anything else, so fill = min(i + 1, k)); every other read -- flagged, a batch whose units did not fit,
// SHK_NO_PACK -- reads its text bytes: a byte that is no base empties the window (fill = 0, fh = rh = 0), and a window is
// emitted only when k bases lie behind it, so the base that leaves is always one that went in.
// kmers, present, solid, sum, min and max stay in registers and leave as the lane's own record (two 16-byte stores, no
// atomics per read); the call's totals are added up per workgroup behind the loop: four atomics per workgroup.
// The per-window values (the track, or the scratch k_reads_median reads): a wave's lanes are a read apart, so they are
// staged as k_roll_query stages its track -- sixteen entries per lane in LDS, whole 64-byte groups as four 16-byte
// stores, the partial groups at a read's two ends entry by entry (the neighbour reads own the rest of those groups).
// SHK_READS_SGPRS: with the text path's branches next to the packed one the kernel wants 102 scalar registers, six more
// than eight waves per SIMD leave each of them; capped at 96 the compiler parks seven in lanes of one more VGPR (63).
#if defined(__HIPCC__)
#define SHK_READS_SGPRS __attribute__((amdgpu_num_sgpr(96)))
#else
#define SHK_READS_SGPRS
#endif
__global__ void __launch_bounds__(256) SHK_READS_SGPRS k_reads_query(ShkReadsArgs A) {
  __shared__ ShkRollRow in4[4], out4[4];      // shk_roll_tabs_init's rows by 2-bit code
  __shared__ uint32_t stage[SHK_QUERY_STAGE][256];
  __shared__ uint64_t scratch[SHK_MAX_WAVES + 1];
  if (threadIdx.x < 4) {
    const uint64_t f = shk_code_seed(threadIdx.x), c = shk_code_seed_rc(threadIdx.x);
    in4[threadIdx.x].f = f; in4[threadIdx.x].r = shk_rol64(c, A.k - 1);
    out4[threadIdx.x].f = shk_rol64(f, A.k); out4[threadIdx.x].r = shk_ror64(c, 1);
  }
  __syncthreads();
  const uint64_t mask = A.hb >= 64 ? ~0ULL : ((1ULL << A.hb) - 1);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t goff = (uint32_t)(reinterpret_cast<uintptr_t>(A.win) >> 2) & (SHK_QUERY_STAGE - 1);      // entry 0's place in its 64 bytes
  uint64_t tk = 0, tp = 0, ts = 0, tsum = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.nreads; r += stride) {
    const uint64_t st = A.rd_start[r];
    const uint32_t len = (uint32_t)(A.rd_end[r] - st);
    uint32_t nk = 0, np = 0, ns = 0, mn = SHK_QUERY_NONE, mx = 0;
    uint64_t sum = 0;
    if (len >= A.k) {
      const uint32_t flag = A.pk ? A.pk_flag[r] : 0;
      const bool packed = flag != 0 && !(flag >> 31);
      const uint32_t *words = packed ? reinterpret_cast<const uint32_t *>(A.pk + A.pk_base[r]) : nullptr;      // sixteen bases a word, the first lowest
      const uint8_t *tx = A.text + st;
      const uint64_t w0 = A.woff[r];
      uint64_t fh = 0, rh = 0;
      uint32_t fill = 0, zin = 0, zout = 0;
      uint32_t first = SHK_QUERY_STAGE;      // the first staged entry's place in its group (SHK_QUERY_STAGE: none is staged)
      for (uint32_t i = 0; i < len; i++) {
        uint32_t ci;
        bool base = true;
        if (packed) {
          if (!(i & 15)) zin = words[i >> 4];
          ci = zin & 3u;
          zin >>= 2;
        } else {
          const uint32_t b = tx[i], u = b & 0xDFu;
          ci = ((b >> 1) ^ (b >> 2)) & 3u;
          base = u == 'A' || u == 'C' || u == 'G' || u == 'T';
        }
        if (!base) {
          fill = 0; fh = 0; rh = 0;
        } else {
          const ShkRollRow ri = in4[ci];
          fh = shk_rol1(fh) ^ ri.f; rh = shk_ror1(rh) ^ ri.r;
          if (fill == A.k) {
            uint32_t co;
            if (packed) {
              const uint32_t o = i - A.k;
              if (!(o & 15)) zout = words[o >> 4];
              co = zout & 3u;
              zout >>= 2;
            } else {
              const uint32_t b = tx[i - A.k];
              co = ((b >> 1) ^ (b >> 2)) & 3u;
            }
            const ShkRollRow ro = out4[co];
            fh ^= ro.f; rh ^= ro.r;
          } else {
            fill++;
          }
        }
        if (i + 1 < A.k) continue;
        uint32_t v = SHK_QUERY_NONE;
        if (fill == A.k) {
          uint8_t trav;
          const uint64_t cnt = shk_lookup_one(A.tab, (fh < rh ? fh : rh) & mask, A.q_lo, A.nslots, 2, &trav);
          v = cnt > SHK_QUERY_CAP ? SHK_QUERY_CAP : (uint32_t)cnt;
          nk++; np += cnt != 0; ns += cnt >= A.min_count; sum += cnt;
          mn = v < mn ? v : mn; mx = v > mx ? v : mx;
        }
        const uint64_t at = w0 + (i + 1 - A.k);
        if (A.win) {
          const uint32_t slot = (uint32_t)(at + goff) & (SHK_QUERY_STAGE - 1);
          stage[slot][threadIdx.x] = v;
          if (first == SHK_QUERY_STAGE) first = slot;
          if (slot == SHK_QUERY_STAGE - 1 || i + 1 == len) {
            uint32_t *g = A.win + (at - slot);      // (slot <= at + goff; entries below `first` are not touched)
            if (first == 0 && slot == SHK_QUERY_STAGE - 1) {
#pragma unroll
              for (uint32_t q = 0; q < SHK_QUERY_STAGE; q += 4)
                *reinterpret_cast<uint4 *>(g + q) = make_uint4(stage[q][threadIdx.x], stage[q + 1][threadIdx.x], stage[q + 2][threadIdx.x], stage[q + 3][threadIdx.x]);
            } else {
              for (uint32_t q = first; q <= slot; q++) g[q] = stage[q][threadIdx.x];
            }
            first = SHK_QUERY_STAGE;
          }
        }
      }
    }
    shk_read_record out;
    out.sum = sum; out.kmers = nk; out.present = np; out.solid = ns;
    out.min = nk ? mn : 0; out.median = A.median; out.max = mx;
    A.rec[r] = out;
    tk += nk; tp += np; ts += ns; tsum += sum;
  }
  tk = shk_block_sum64(tk, scratch); tp = shk_block_sum64(tp, scratch);
  ts = shk_block_sum64(ts, scratch); tsum = shk_block_sum64(tsum, scratch);
  if (threadIdx.x == 0 && tk) {
    unsigned long long *a = (unsigned long long *)A.totals;
    atomicAdd(a, (unsigned long long)tk);
    if (tp) atomicAdd(a + 1, (unsigned long long)tp);
    if (ts) atomicAdd(a + 2, (unsigned long long)ts);
    if (tsum) atomicAdd(a + 3, (unsigned long long)tsum);
  }
}

// The lower median of every read's counts: the value of rank (kmers - 1) / 2 among the read's window values. The entries
// of windows that are no k-mers are SHK_QUERY_NONE, the largest value there is, so they sort last and the rank is taken
// over all windows as they lie. A bitwise radix select from the top set bit of the read's max downwards: per bit one pass
// over the read's values counts those that share the prefix found so far and have the bit clear -- windows x bits loads,
// never a sort and never quadratic (a 65535-base read has 65 k windows). SHK_READS_GROUP lanes share a read (their loads
// are neighbours), add their counts with three shuffles per bit, and a wave's groups walk the bits in step from the
// highest top bit among them (a group above its own top bit only takes part in the shuffles).
#define SHK_READS_GROUP 8
__global__ void __launch_bounds__(256) k_reads_median(const uint32_t *win, const uint64_t *woff, uint64_t nreads, shk_read_record *rec) {
  const uint32_t lane = shk_lane(), g = lane & (SHK_READS_GROUP - 1);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x / SHK_READS_GROUP;
  for (uint64_t r0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane) / SHK_READS_GROUP; r0 < nreads; r0 += stride) {
    const uint64_t r = r0 + lane / SHK_READS_GROUP;
    uint32_t kmers = 0, mx = 0, n = 0;
    uint64_t w0 = 0;
    if (r < nreads) { kmers = rec[r].kmers; mx = rec[r].max; w0 = woff[r]; n = (uint32_t)(woff[r + 1] - w0); }
    const int top = kmers && mx ? 31 - __clz((int)mx) : -1;
    int wtop = top;
    for (int m = SHK_READS_GROUP; m < SHK_WAVE; m <<= 1) { const int o = __shfl_xor(wtop, m); wtop = o > wtop ? o : wtop; }
    uint32_t rank = kmers ? (kmers - 1) / 2 : 0, prefix = 0;
    for (int b = wtop; b >= 0; b--) {
      uint32_t zeros = 0;
      if (b <= top) {
        const uint64_t hi = (uint64_t)prefix >> (b + 1);
        for (uint32_t i = g; i < n; i += SHK_READS_GROUP) {
          const uint32_t v = win[w0 + i];
          zeros += ((uint64_t)v >> (b + 1)) == hi && !((v >> b) & 1u);
        }
      }
      for (int m = 1; m < SHK_READS_GROUP; m <<= 1) zeros += __shfl_xor(zeros, m);
      if (b <= top && rank >= zeros) { rank -= zeros; prefix |= 1u << b; }
    }
    if (g == 0 && kmers) rec[r].median = prefix;
  }
}
