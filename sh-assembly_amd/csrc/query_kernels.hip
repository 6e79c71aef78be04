// shk_query_fasta: FASTA text against the table -- per base the count of the k-mer that ends there, per record and per
// piece how many k-mers the table holds. The front end is shk_count_fasta's (fasta_kernels.hip: the text becomes 2-bit
// segments, one "read" of the packed roll form each); what is added here:
//   k_fa_rec_starts  the base ordinal at which every header line of the piece begins, in text order. A run never crosses
//                    a header, so a segment's record is the number of headers whose ordinal is <= the segment's first
//                    base ordinal (a binary search per segment); ordinals are stream coordinates (the tail's bases in
//                    front), so a segment that starts inside the carried tail finds no header and belongs to record 0
//   k_roll_query     one thread per segment rolls its k-mers (shk_roll_round_pk's recurrence) and reads every key's count from the
//                    table (shk_lookup_one, mark mode 2: traveled bits are neither read nor set)
#include "shk_device.h"

// As k_fa_compact finds the run starts: the thread's bases and openers in front of it by one scan over the tile, the
// tile's by the two scans of the host side (tile_off: bases, low SHK_FA_COUNT_BITS; rec_off: header lines).
__global__ void __launch_bounds__(256) k_fa_rec_starts(const uint8_t *text, uint64_t n, uint64_t safe_end, const uint8_t *unit_state, const uint64_t *tile_off,
                                                        const uint64_t *rec_off, uint64_t ntiles, uint64_t tail, uint64_t *rec_start, uint64_t nrec) {
  __shared__ uint32_t scratch[SHK_MAX_WAVES + 1];
  uint32_t nvalid, tot;
  const ShkQuad v = shk_fa_load(text, n, safe_end, &nvalid);
  ShkFaWalk w = {0, 0, 0, 0, 0, 0};
  if (nvalid) shk_fa_walk(shk_fa_masks(v, nvalid), unit_state[(uint64_t)blockIdx.x * blockDim.x + threadIdx.x], &w);
  // (a tile has at most 256 x 16 bases and half as many header lines)
  const uint32_t ex = shk_block_exscan(w.nbase | w.nrec << 16, &tot, scratch);
  if (blockIdx.x >= ntiles || !w.openmask) return;
  const uint64_t g = tail + (tile_off[blockIdx.x] & SHK_FA_COUNT_MASK) + (ex & 0xFFFFu);
  uint64_t ri = rec_off[blockIdx.x] + (ex >> 16);
  for (uint32_t om = w.openmask; om; om &= om - 1) {
    const uint32_t j = (uint32_t)__ffs((int)om) - 1;
    if (ri < nrec) rec_start[ri] = g + (uint32_t)__popc(w.basemask & ((1u << j) - 1));
    ri++;
  }
}

#define SHK_QUERY_CAP 0xFFFFFFFEu      // a track entry's largest value (SHK_QUERY_NONE = 0xFFFFFFFF: no k-mer ends here)
struct ShkQueryArgs {
  const uint64_t *rd_start, *rd_end;   // the segments, as k_fa_segments left them (stream coordinates)
  const uint64_t *pk_base; const ShkQuad *pk;
  uint64_t nseg;
  uint32_t k, hb;
  uint8_t *tab; uint64_t q_lo, nslots;
  const uint64_t *rec_start; uint64_t nrec;
  uint64_t tail;                       // bases of the carried tail in front of the piece's own
  uint32_t min_count;
  uint32_t *track; uint64_t track_len; // null: no track. Pre-filled with 0xFF bytes; entry b = the piece's b-th base
  uint64_t *acc;                       // [4 * (nrec + 1)]: kmers, present, solid, sum of every record, zeroed
};

__device__ __forceinline__ uint64_t shk_wave_sum64(uint64_t x) { return shk_last_lane64(shk_wave_incl_add64(x)); }

#define SHK_QUERY_STAGE 16             // track entries a lane collects before it stores them: one aligned 64-byte run
// Grid-stride over the segments, a wave's 64 lanes on 64 neighbouring segments and in step from segment to segment (the
// loop's bound is the wave's, so that its lanes meet for the sums below). The kernel waits for the lookups' scattered
// loads and for nothing else, so what it has is waves per SIMD, i.e. few registers and one copy of the probe loop:
// shk_roll_round_pk's recurrence (roll_kernels.hip, the staged form: the rows of its in4 / out4 tables, the segment's
// 2-bit units as k_fa_pack left them) runs here ONE BASE PER TURN with the lookup behind it. The sixteen-step rounds of
// shk_roll_round_pk themselves instantiate their emitter 48 times: with the lookup in it the kernel is 190 KB of code at
// 122 VGPRs (4 waves per SIMD), with the round's keys parked in registers for one lookup loop behind it 152 VGPRs (3 waves).
// This form keeps 8 waves, and its thirty-odd operations per base disappear behind a probe's loads either way.
// The track: a wave's lanes are a segment apart, so a lane's 4-byte store per base is a memory transaction of its own
// (measured: the kernel 20 to 45% slower with a track than without). A lane therefore collects the entries of one
// 64-byte-aligned group of sixteen in LDS (entry-major: no bank conflicts) and stores a whole group as four 16-byte
// stores; the partial groups at a segment's two ends go out entry by entry (the neighbour segment owns the rest of them).
// The four sums of a segment stay in registers; behind the segment the lanes that share a record add theirs up across the
// wave, and one lane sends the record's four 64-bit atomics (a wave inside a chromosome: four atomics per 64 segments).
__global__ void __launch_bounds__(256) k_roll_query(ShkQueryArgs A) {
  __shared__ ShkRollRow in4[4], out4[4];      // shk_roll_tabs_init's rows by 2-bit code
  __shared__ uint32_t stage[SHK_QUERY_STAGE][256];
  if (threadIdx.x < 4) {
    const uint64_t f = shk_code_seed(threadIdx.x), c = shk_code_seed_rc(threadIdx.x);
    in4[threadIdx.x].f = f; in4[threadIdx.x].r = shk_rol64(c, A.k - 1);
    out4[threadIdx.x].f = shk_rol64(f, A.k); out4[threadIdx.x].r = shk_ror64(c, 1);
  }
  __syncthreads();
  const uint64_t mask = A.hb >= 64 ? ~0ULL : ((1ULL << A.hb) - 1);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t lane = shk_lane();
  const uint32_t goff = (uint32_t)(reinterpret_cast<uintptr_t>(A.track) >> 2) & (SHK_QUERY_STAGE - 1);      // entry 0's place in its 64 bytes
  for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; r0 < A.nseg; r0 += stride) {
    const uint64_t r = r0 + lane;
    const bool have = r < A.nseg;
    uint64_t nk = 0, np = 0, ns = 0, sum = 0, rec = 0;
    if (have) {
      const uint64_t st = A.rd_start[r];
      uint64_t lo = 0, hi = A.nrec;
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (A.rec_start[mid] <= st) lo = mid + 1; else hi = mid;
      }
      rec = lo;
      const uint32_t len = (uint32_t)(A.rd_end[r] - st);
      const uint32_t *words = reinterpret_cast<const uint32_t *>(A.pk + A.pk_base[r]);      // sixteen bases a word, the first lowest
      // a k-mer's last base is base st + i of the stream, i >= k - 1, and the tail holds <= k - 1 bases: never negative
      const uint64_t tb = st - A.tail;
      uint64_t fh = 0, rh = 0;
      uint32_t zin = 0, zout = 0;
      uint32_t first = SHK_QUERY_STAGE;      // the first staged entry's place in its group (SHK_QUERY_STAGE: none is staged)
      for (uint32_t i = 0; i < len; i++) {
        if (!(i & 15)) zin = words[i >> 4];
        const ShkRollRow ri = in4[zin & 3u];
        zin >>= 2;
        fh = shk_rol1(fh) ^ ri.f; rh = shk_ror1(rh) ^ ri.r;
        if (i >= A.k) {
          const uint32_t o = i - A.k;
          if (!(o & 15)) zout = words[o >> 4];
          const ShkRollRow ro = out4[zout & 3u];
          zout >>= 2;
          fh ^= ro.f; rh ^= ro.r;
        }
        if (i + 1 < A.k) continue;
        uint8_t trav;
        const uint64_t cnt = shk_lookup_one(A.tab, (fh < rh ? fh : rh) & mask, A.q_lo, A.nslots, 2, &trav);
        nk++; np += cnt != 0; ns += cnt >= A.min_count; sum += cnt;
        const uint64_t at = tb + i;
        if (A.track && at < A.track_len) {
          const uint32_t slot = (uint32_t)(at + goff) & (SHK_QUERY_STAGE - 1);
          stage[slot][threadIdx.x] = cnt > SHK_QUERY_CAP ? SHK_QUERY_CAP : (uint32_t)cnt;
          if (first == SHK_QUERY_STAGE) first = slot;
          if (slot == SHK_QUERY_STAGE - 1 || i + 1 == len) {
            uint32_t *g = A.track + (at - slot);      // (slot <= at + goff; entries below `first` are not touched)
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
    for (uint64_t left = __ballot(have && nk != 0); left;) {
      const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1;
      const uint64_t lrec = __shfl(rec, (int)leader);
      const bool mine = have && nk != 0 && rec == lrec;
      const uint64_t t0 = shk_wave_sum64(mine ? nk : 0), t1 = shk_wave_sum64(mine ? np : 0), t2 = shk_wave_sum64(mine ? ns : 0),
                     t3 = shk_wave_sum64(mine ? sum : 0);
      if (lane == leader) {
        unsigned long long *a = (unsigned long long *)A.acc + 4 * lrec;
        atomicAdd(a, (unsigned long long)t0);
        if (t1) atomicAdd(a + 1, (unsigned long long)t1);
        if (t2) atomicAdd(a + 2, (unsigned long long)t2);
        if (t3) atomicAdd(a + 3, (unsigned long long)t3);
      }
      left &= ~__ballot(mine);
    }
  }
}
