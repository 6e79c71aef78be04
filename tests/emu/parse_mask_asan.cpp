// TEST INFRASTRUCTURE ONLY: a program of its own (CPU, AddressSanitizer) around the emulator build of the kernel sources,
// for the one buffer whose stores are new: the newline flags k_count_lines leaves for k_emit_reads (ShkStageBufs::d_nlmask,
// allocated without slack). It calls shk_hash_chunks and shk_count_chunks on "device" text that lies in allocations ending
// exactly at the next multiple of 16 behind the text:
//   chunk edges   one or two records per chunk, starts and ends on every residue mod 128, gaps of newlines between them,
//                 chunks shorter than 16 units; the last chunk ends on the text's last byte
//   growth        max_batch_bytes = 64 and max_batch_keys = the keys of the big text: a small text, one whose flags do not
//                 fit the buffer the context was created with, the small one again
// Built by parse_mask_asan.mk, run by tests/test_parse_mask.py, with and without SHK_PARSE_MASK=0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/shk.h"

static const uint32_t K = 21;
static uint64_t rng_state = 88172645463325252ULL;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}

struct Text {
  std::string fq;
  std::vector<uint64_t> off, len;
  uint64_t keys = 0;
};

// a record of a header of `h` bytes and a read of `r` bases
static void add_record(Text &t, uint32_t h, uint32_t r) {
  t.fq += '@';
  t.fq.append(h - 1, 'h');
  t.fq += '\n';
  for (uint32_t i = 0; i < r; i++) t.fq += "ACGT"[rnd(4)];
  t.fq += "\n+\n";
  t.fq.append(r, 'I');
  t.fq += '\n';
  if (r >= K) t.keys += r - K + 1;
}

static Text chunk_edges() {
  Text t;
  t.fq = "@front\nACGT\n+\nIIII\n\n";
  for (uint32_t c = 0; c < 128; c++) {
    // chunk c starts on residue 5 c and ends on residue 7 c + 3 (mod 128): a gap of newlines in front, the header's length
    t.fq.append((128 + 5 * c % 128 - t.fq.size() % 128) % 128, '\n');
    const uint64_t a = t.fq.size();
    if (c % 4 == 0) add_record(t, 2 + rnd(130), K + rnd(5));
    const uint32_t r = K + rnd(5);
    add_record(t, 2 + (uint32_t)((128 + 7 * c + 3 - (t.fq.size() + 2 + 2 * r + 5) % 128) % 128), r);
    t.off.push_back(a);
    t.len.push_back(t.fq.size() - a);
    if (a % 128 != 5 * c % 128 || t.fq.size() % 128 != (7 * c + 3) % 128) { fprintf(stderr, "chunk_edges: residues\n"); exit(2); }
  }
  return t;                                                          // (nothing behind the last chunk)
}

static Text tiled(uint32_t nrec, uint32_t hmin, uint32_t hspan, uint32_t per) {
  Text t;
  for (uint32_t i = 0; i < nrec; i++) {
    if (i % per == 0) { if (i) t.len.push_back(t.fq.size() - t.off.back()); t.off.push_back(t.fq.size()); }
    add_record(t, hmin + rnd(hspan), K + rnd(5));
  }
  t.len.push_back(t.fq.size() - t.off.back());
  return t;
}

// the text in an allocation that ends at the next multiple of 16 behind it
static uint8_t *exact_copy(const Text &t) {
  void *p = nullptr;
  if (posix_memalign(&p, 16, (t.fq.size() + 15) & ~(size_t)15)) exit(2);
  memcpy(p, t.fq.data(), t.fq.size());
  return (uint8_t *)p;
}

static shk_ctx *make(uint32_t qb, uint64_t bytes, uint64_t keys, uint64_t reads) {
  shk_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.qb = qb; cfg.hb = qb + 8; cfg.seed = 2038074761u; cfg.k = K;
  cfg.ndistinct_for_denoise = 1ULL << 62;
  cfg.max_batch_bytes = bytes; cfg.max_batch_keys = keys; cfg.max_batch_reads = reads;
  cfg.threads_per_group = 64; cfg.hash_groups = 2;
  shk_ctx *c = nullptr;
  const int rc = shk_create(&cfg, &c);
  if (rc) { fprintf(stderr, "shk_create: %s\n", shk_strerror(rc)); exit(2); }
  return c;
}

static void run(shk_ctx *c, const Text &t, const char *what) {
  uint8_t *p = exact_copy(t);
  uint64_t *words = nullptr, nwords = 0;
  int rc = shk_hash_chunks(c, p, 1, t.fq.size(), t.off.data(), t.len.data(), (uint32_t)t.off.size(), &words, &nwords);
  if (rc || nwords != t.keys) { fprintf(stderr, "%s: shk_hash_chunks rc %d, %llu words, expected %llu\n", what, rc, (unsigned long long)nwords, (unsigned long long)t.keys); exit(1); }
  shk_batch_stats st;
  rc = shk_count_chunks(c, p, 1, t.fq.size(), t.off.data(), t.len.data(), (uint32_t)t.off.size(), &st);
  if (rc || st.kmers != t.keys) { fprintf(stderr, "%s: shk_count_chunks rc %d, %llu k-mers, expected %llu\n", what, rc, (unsigned long long)st.kmers, (unsigned long long)t.keys); exit(1); }
  free(p);
}

int main() {
  {
    const Text t = chunk_edges();
    shk_ctx *c = make(16, t.fq.size() + 16, t.keys + 64 > (1u << 14) ? t.keys + 64 : (1u << 14), t.fq.size() / 8 + 4096);
    run(c, t, "chunk edges");
    shk_destroy(c);
  }
  {
    const Text small = tiled(6, 20, 9, 2), big = tiled(60, 300, 200, 7);
    // the flags of `big` do not fit the buffer of a context created for its keys; those of `small` do
    const uint64_t initial = (4 * big.keys > 64 ? 4 * big.keys : 64) / 16 + 8;
    if (!(small.fq.size() / 16 + 8 <= initial && initial < big.fq.size() / 16 + 8) || small.keys > big.keys) { fprintf(stderr, "growth: sizes\n"); return 2; }
    shk_ctx *c = make(12, 64, big.keys, 1024);
    run(c, small, "growth: small");
    run(c, big, "growth: big");
    run(c, small, "growth: small again");
    shk_destroy(c);
  }
  printf("PARSE_MASK_ASAN_OK\n");
  return 0;
}
