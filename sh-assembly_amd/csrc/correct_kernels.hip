// shk_correct_reads: substitution errors of FASTQ reads repaired against the table. The front end is shk_query_reads'
// (parse_stage: the reads' extents; pack_stage: the 2-bit units of the reads that are all bases); what is added here:
//   k_correct_check  a read of more than 65535 bases raises SHK_E_BAD_FASTQ before anything else runs
//   k_reads_correct  one thread per read scans the read's windows on both strands (k_reads_query's roll, one base per
//                    turn, ONE copy of the probe loop behind it), tries the three other bases where a weak window follows
//                    a solid one, and writes the single base that makes the next check + 1 windows solid into the read's
//                    units and into the read's edit list
// The rule is include/shk.h's (shk_correct_reads); DESIGN.md 4 has the reasons.
#include "shk_device.h"

struct ShkCorrectArgs {
  const uint64_t *rd_start, *rd_end;   // the reads, as k_emit_reads left them (text offsets)
  uint64_t nreads;
  ShkQuad *pk;                         // 2-bit staging as in ShkRollArgs, never null here; the kernel writes its edits into it
  const uint64_t *pk_base;
  const uint32_t *pk_flag;
  uint32_t k, hb;
  uint8_t *tab; uint64_t q_lo, nslots;
  uint32_t min_count, check, max_edits;
  shk_correct_record *rec;
  uint32_t *edits;                     // [nreads * max_edits]
  uint64_t *totals;                    // [SHK_CORRECT_TOTALS] of the call, zeroed
};
enum { CT_CANDIDATES, CT_EDITED, CT_EDITS, CT_UNFIXABLE, CT_AMBIGUOUS, CT_CAPPED, CT_LOOKUPS, SHK_CORRECT_TOTALS };

__global__ void k_correct_check(const uint64_t *rd_start, const uint64_t *rd_end, uint64_t nreads, uint32_t *err) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += stride)
    if (rd_end[r] - rd_start[r] > 65535) atomicOr(err, SHK_E_BAD_FASTQ);
}

// Grid-stride over the reads, a wave's 64 lanes on 64 neighbouring reads, as k_reads_query -- and like it the kernel waits
// for the lookups' scattered loads and for little else, so the whole rule is ONE loop around ONE lookup: a turn either
// scans (t == 0: base i of the pass goes in, base i - k goes out, window i - k + 1 is judged) or tries (t = 1 .. 3: the
// suspect at i reads as (orig + t) & 3, and window i - k + 1 + d is judged, d = 0 .. dmax), and both kinds of turn meet at
// the same call of shk_lookup_one. Lanes that scan and lanes that try share the loop; a wave runs at the pace of the lane
// with the most turns (its longest read, or the one with the most suspects).
// A pass is a direction: pass 1 walks the read from its last base with the codes complemented (3 - code = code ^ 3),
// which IS the forward rule on the reverse complement; the canonical key does not know the strand. A first pass that
// met no weak window leaves nothing for the second to find, which is then skipped.
// Bases come from the read's 2-bit units through two one-word caches (the incoming and the leaving base's word, each
// with the index of the word it holds): a turn costs a global load only when it crosses into another word. An edit is a
// 32-bit read-modify-write of the word that holds the base -- the units of a read are its own, so no atomics -- and patches
// the caches; this is how later windows, the other pass included, see it. The hash of window j - 1 (pfh, prh) is kept from
// turn to turn: every trial starts there, and so does the window that is left behind when the trials are over.
// The record leaves as one 16-byte store, an edit as one store into the lane's own max_edits words when it is made; the
// call's totals are added up per workgroup behind the loop: at most seven atomics per workgroup.
__global__ void __launch_bounds__(256) k_reads_correct(ShkCorrectArgs A) {
  __shared__ ShkRollRow in4[4], out4[4];      // shk_roll_tabs_init's rows by 2-bit code
  __shared__ uint64_t scratch[SHK_MAX_WAVES + 1];
  if (threadIdx.x < 4) {
    const uint64_t f = shk_code_seed(threadIdx.x), c = shk_code_seed_rc(threadIdx.x);
    in4[threadIdx.x].f = f; in4[threadIdx.x].r = shk_rol64(c, A.k - 1);
    out4[threadIdx.x].f = shk_rol64(f, A.k); out4[threadIdx.x].r = shk_ror64(c, 1);
  }
  __syncthreads();
  const uint64_t mask = A.hb >= 64 ? ~0ULL : ((1ULL << A.hb) - 1);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t tot[SHK_CORRECT_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.nreads; r += stride) {
    const uint32_t len = (uint32_t)(A.rd_end[r] - A.rd_start[r]);
    const uint32_t flag = A.pk_flag[r];
    uint32_t ne = 0, unf = 0, amb = 0, fl = 0;
    if (len < A.k) {
      fl = SHK_CORRECT_SHORT;
    } else if (flag == 0 || (flag >> 31)) {
      fl = SHK_CORRECT_NONBASE;
    } else {
      uint32_t *words = reinterpret_cast<uint32_t *>(A.pk + A.pk_base[r]);      // sixteen bases a word, the first lowest
      uint32_t *ed = A.edits + r * A.max_edits;
      const uint32_t top = len - 1;
      uint32_t budget = A.max_edits, looks = 0;
      uint32_t win = 0, tin = ~0u, wout = 0, tout = ~0u;      // the two cached words and which ones they are
      for (uint32_t pass = 0; pass < 2; pass++) {
        const uint32_t flip = pass ? 3u : 0u;
        const auto code_in = [&](uint32_t pos) -> uint32_t {
          const uint32_t own = pass ? top - pos : pos;
          if ((own >> 4) != tin) { tin = own >> 4; win = words[tin]; }
          return ((win >> (2 * (own & 15))) & 3u) ^ flip;
        };
        const auto code_out = [&](uint32_t pos) -> uint32_t {
          const uint32_t own = pass ? top - pos : pos;
          if ((own >> 4) != tout) { tout = own >> 4; wout = words[tout]; }
          return ((wout >> (2 * (own & 15))) & 3u) ^ flip;
        };
        uint64_t fh = 0, rh = 0, pfh = 0, prh = 0;
        uint32_t i = 0, d = 0, t = 0, dmax = 0, nvalid = 0, vcode = 0, orig = 0;
        bool prev = false, weak = false;
        while (i < len) {
          const uint32_t pos = i + d;
          uint32_t ci;
          if (t && d == 0) { fh = pfh; rh = prh; ci = (orig + t) & 3u; }
          else { if (!t) { pfh = fh; prh = rh; } ci = code_in(pos); }
          { const ShkRollRow ri = in4[ci]; fh = shk_rol1(fh) ^ ri.f; rh = shk_ror1(rh) ^ ri.r; }
          if (pos >= A.k) {
            const uint32_t co = t && pos - A.k == i ? (orig + t) & 3u : code_out(pos - A.k);
            const ShkRollRow ro = out4[co]; fh ^= ro.f; rh ^= ro.r;
          }
          if (pos + 1 < A.k) { i++; continue; }      // (a scanning turn: a trial has i >= k)
          uint8_t trav;
          const bool solid = shk_lookup_one(A.tab, (fh < rh ? fh : rh) & mask, A.q_lo, A.nslots, 2, &trav) >= A.min_count;
          looks++;
          if (!t) {
            weak |= !solid;
            if (!solid && prev) {
              if (budget) { orig = ci; t = 1; nvalid = 0; dmax = A.check < top - i ? A.check : top - i; continue; }
              fl |= SHK_CORRECT_CAPPED;
            }
            prev = solid; i++;
            continue;
          }
          if (solid && d < dmax) { d++; continue; }
          if (solid) { nvalid++; vcode = (orig + t) & 3u; }
          d = 0;
          if (t < 3 && nvalid < 2) { t++; continue; }      // (a second valid base settles it: ambiguous)
          uint32_t now = orig;
          if (nvalid == 1) {
            now = vcode;
            const uint32_t own = pass ? top - i : i, sh = 2 * (own & 15);
            const uint32_t w = (words[own >> 4] & ~(3u << sh)) | ((now ^ flip) << sh);
            words[own >> 4] = w;
            if (tin == (own >> 4)) win = w;
            if (tout == (own >> 4)) wout = w;
            ed[ne++] = own | ((now ^ flip) << 16);
            budget--;
          } else if (nvalid == 0) {
            unf++;
          } else {
            amb++;
          }
          // the window the scan goes on from: j - 1's hash, the base the suspect now is, and the one that leaves (i >= k)
          { const ShkRollRow ri = in4[now], ro = out4[code_out(i - A.k)];
            fh = shk_rol1(pfh) ^ ri.f ^ ro.f; rh = shk_ror1(prh) ^ ri.r ^ ro.r; }
          prev = nvalid == 1; t = 0; i++;
        }
        if (!weak) break;
      }
      tot[CT_CANDIDATES]++; tot[CT_EDITED] += ne != 0; tot[CT_EDITS] += ne; tot[CT_UNFIXABLE] += unf; tot[CT_AMBIGUOUS] += amb;
      tot[CT_CAPPED] += (fl & SHK_CORRECT_CAPPED) != 0; tot[CT_LOOKUPS] += looks;
    }
    shk_correct_record out;
    out.edits = ne; out.unfixable = unf; out.ambiguous = amb; out.flags = fl;
    A.rec[r] = out;
  }
#pragma unroll
  for (int z = 0; z < SHK_CORRECT_TOTALS; z++) {
    const uint64_t s = shk_block_sum64(tot[z], scratch);
    if (threadIdx.x == 0 && s) atomicAdd((unsigned long long *)A.totals + z, (unsigned long long)s);
  }
}
