"""Cases for shk_sample_chunks (include/shk.h), shared by the emulator and the GPU tests of tests/test_sample.py.

Expected values never come from the library: cqflibs.oracle().chunk_keys(chunk, k, 64) gives the full canonical hashes of
a chunk in emission order (the oracle's reads_to_kmers with its mask all ones), the kept ones are those whose bits
[hb, hb + s) are zero, masked to hb bits, and the expected table is the oracle's qf_new + qf_insert of each. Every
comparison is for equality. Every case asserts its own guard conditions (the oracle's table is not full, something is
kept, for s > 0 something is dropped), so that a vacuous case fails instead of passing."""
import random

import cqflibs
import synth
from fastq_util import chunks_by_records

# k_roll_sample (roll_kernels.hip): every wave of 64 threads stages its kept keys in an LDS list of 64 * 16 + 64 * 4 words
# and flushes it when it holds more than 64 * 4 behind a window; test_sample.test_constants_mirror_the_kernel keeps these
# in step. The library launches workgroups of GPU_THREADS on gfx950 and of EMU_THREADS in the emulator build.
ROLL_STEPS, WAVE = 16, 64
GPU_THREADS, EMU_THREADS = 256, 64
LIST_CAPACITY = WAVE * ROLL_STEPS + WAVE * ROLL_STEPS // 4


def hashes_of(fq, offs, lens, k):
    O = cqflibs.oracle()
    out = []
    for a, n in zip(offs, lens):
        out += O.chunk_keys(fq[a:a + n], k, 64)
    return out


def kept_of(hashes, hb, s):
    return [h & ((1 << hb) - 1) for h in hashes if (h >> hb) & ((1 << s) - 1) == 0]


class Expect:
    """the oracle's table of everything sampled so far, with the guards"""

    def __init__(self, qb):
        self.qb, self.hb = qb, qb + 8
        self.q = cqflibs.oracle().new(qb)

    def add(self, hashes, s, times=1):
        kept = kept_of(hashes, self.hb, s)
        assert kept, "vacuous: nothing is kept"
        assert s == 0 or len(kept) < len(hashes), "vacuous: everything is kept"
        assert s > 0 or len(kept) == len(hashes)
        for _ in range(times):
            for x in kept:
                self.q.insert(x)
        assert not self.q.full(), "the oracle's table is full: raise qb"
        return kept

    def check(self, ctx, what=""):
        assert not self.q.full()
        assert ctx.blocks() == self.q.blocks(), "table bytes differ " + str(what)
        t = ctx.totals()
        assert (t.nelts, t.ndistinct) == (self.q.nelts(), self.q.ndistinct()), what

    def free(self):
        self.q.free()


def sample_and_check(ctx, exp, fq, offs, lens, k, s, what=""):
    """one call over the chunks; its statistics and the table against the oracle's. Returns the kept keys."""
    hashes = hashes_of(fq, offs, lens, k)
    d0 = exp.q.ndistinct()
    kept = exp.add(hashes, s)
    st, ss = ctx.sample_chunks(fq, offs, lens, s)
    assert ss == {"kmers": len(hashes), "kept": len(kept)}, (what, ss, len(hashes), len(kept))
    assert (st["kmers"], st["chunks"], st["denoise_rounds"]) == (len(kept), 1, 0), (what, st)
    assert st["new_distinct"] == exp.q.ndistinct() - d0, (what, st)
    exp.check(ctx, what)
    return kept


# ---------------------------------------------------------------- inputs
def read_mix(k, seed=7):
    """the read mix of roll_cases.run: lengths around k, the 16-base rounds and the 64-base units, lower case, 'N' at the
    ends and inside, IUPAC and other bytes"""
    rnd = random.Random(seed)
    recs = []
    lens_ = [1, k - 1, k, k + 1, k + 15, k + 16, k + 17, 63, 64, 65, 127, 128, 129, 150, 191, 192, 193, 2 * k + 64, 300, 517]
    for i, L in enumerate(lens_ + [rnd.randrange(k, 400) for _ in range(30)]):
        L = max(1, L)
        s = [rnd.choice("ACGT") for _ in range(L)]
        m = i % 6
        if m == 1:
            for _ in range(3):
                p = rnd.randrange(L)
                s[p] = s[p].lower()
        elif m == 2:
            s[rnd.randrange(L)] = "N"
        elif m == 3:
            s[rnd.randrange(L)] = rnd.choice("nRYKSWDMB.-*")
        elif m == 4 and L > 2:
            s[0] = "N"
            s[-1] = "N"
            s[L // 2] = "n"
        recs.append("@r%d\n%s\n+\n%s\n" % (i, "".join(s), "I" * L))
    rnd.shuffle(recs)
    return "".join(recs).encode()


def plain_reads(n, length, seed):
    rnd = random.Random(seed)
    return "".join("@p%d\n%s\n+\n%s\n" % (i, "".join(rnd.choice("ACGT") for _ in range(length)), "I" * length) for i in range(n)).encode()


K_LIST = [5, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 129]
S_LIST = [0, 1, 3]
GEOMETRIES = [(12, 0, 1), (12, 2, 2), (14, 2, 3)]       # qb, max_level_bits, partition levels (fasta_cases.GEOMETRIES)


# ---------------------------------------------------------------- runners (mk = context factory of the build under test)
def run_shapes(mk, k, no_pack):
    """case 1: the read mix in chunks of 7 records, s = 0, 1, 3, once with the reads staged at 2 bits per base and once
    with every read on the text path; both give the oracle's table, hence the same one.
    The text path is reached in two ways. A key capacity too small for the 2-bit units (they need text / 64 + reads + 1 <=
    max_batch_keys / 2 - 1) is also too small for the kept words of this mix at s <= 3 (a read of 150 bases gives 5 units
    and 120 k-mers), so that form runs at s = 5, where the kept words fit below the units' need; at s = 0, 1, 3 the
    library's own SHK_NO_PACK switch (pack_stage) takes the staging away instead. no_pack: context manager setting it."""
    fq = read_mix(k)
    offs, lens = chunks_by_records(fq, 7)
    hashes = hashes_of(fq, offs, lens, k)
    nreads = fq.count(b"\n") // 4
    for s in S_LIST:
        qb = 12 if s == 3 else 14
        blocks = []
        for pack in (True, False):
            exp = Expect(qb)
            ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 20, max_batch_keys=1 << 16)
            ctx.profile(True)
            if pack:
                sample_and_check(ctx, exp, fq, offs, lens, k, s, (k, s, "staged"))
            else:
                with no_pack():
                    sample_and_check(ctx, exp, fq, offs, lens, k, s, (k, s, "text"))
            prof = ctx.profile_get()
            assert ("k_pack_reads" in prof) == pack and "k_roll_sample" in prof, (k, s, pack, sorted(prof))
            blocks.append(ctx.blocks())
            ctx.close()
            exp.free()
        assert blocks[0] == blocks[1]
    # a key capacity below the units' need: the fallback of pack_stage itself
    s, qb = 5, 12
    kept = kept_of(hashes, qb + 8, s)
    need_units = len(fq) // 64 + nreads + 1
    cap = max(2 * len(kept), 64)
    assert cap // 2 - 1 < need_units, "the capacity would hold the units: nothing is tested"
    exp = Expect(qb)
    ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 20, max_batch_keys=cap)
    ctx.profile(True)
    sample_and_check(ctx, exp, fq, offs, lens, k, s, (k, s, "capacity below the units"))
    prof = ctx.profile_get()
    assert "k_pack_reads" not in prof and "k_roll_sample" in prof
    ctx.close()
    exp.free()


def run_anchor(mk, k=31, qb=14):
    """case 2: on one-chunk input, sample_chunks(.., 0) leaves the table count_chunks leaves"""
    fq = synth.make_fastq(synth.make_genome(2000, 2), 60, 100, 0.01, seed=4, n_frac=0.05)
    a, b = (mk(qb=qb, k=k, max_batch_bytes=1 << 20, max_batch_keys=1 << 16) for _ in range(2))
    st, ss = a.sample_chunks(fq, [0], [len(fq)], 0)
    st2 = b.count_chunks(fq, [0], [len(fq)])
    assert ss["kmers"] == ss["kept"] == st["kmers"] == st2["kmers"] > 0
    assert st == st2
    assert a.blocks() == b.blocks()
    ta, tb = a.totals(), b.totals()
    assert (ta.nelts, ta.ndistinct) == (tb.nelts, tb.ndistinct)
    a.close()
    b.close()


def run_flush_full(mk, threads):
    """case 3a: s = 0 on 150-base reads, enough of them that every wave of two whole workgroups keeps more than twice its
    list's capacity: every window fills the list past its threshold and the list is flushed window after window.
    threads = workgroup size of k_roll_sample in the build under test."""
    k, qb, length = 31, 18, 150
    nreads = 2 * threads + 88                  # two workgroups with a read for every thread, a third partly filled
    assert WAVE * (length - k + 1) > 2 * LIST_CAPACITY
    assert WAVE * ROLL_STEPS > LIST_CAPACITY - WAVE * ROLL_STEPS      # one full window crosses the threshold
    fq = plain_reads(nreads, length, 17)
    offs, lens = chunks_by_records(fq, 100)
    exp = Expect(qb)
    ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 20, max_batch_keys=1 << 18)
    sample_and_check(ctx, exp, fq, offs, lens, k, 0, "full windows")
    ctx.close()
    exp.free()


SPARSE_SEED = 12         # (chosen so that the sample is not empty: it keeps 3 of the 100 k-mers)


def run_flush_sparse(mk):
    """case 3b: s = 7 on a batch of about 100 k-mers: whole windows keep nothing, the list is flushed once, at the end"""
    k, qb, s = 31, 12, 7
    fq = plain_reads(1, 130, SPARSE_SEED)
    exp = Expect(qb)
    ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 16, max_batch_keys=1 << 12)
    kept = sample_and_check(ctx, exp, fq, [0], [len(fq)], k, s, "sparse")
    assert 1 <= len(kept) <= 10
    ctx.close()
    exp.free()


def run_accumulate(mk, k=31, s=2, qb=13):
    """case 4: three calls over thirds of the chunks give the bytes of one call over all of them; a second identical call
    doubles every count"""
    fq = synth.make_fastq(synth.make_genome(3000, 9), 120, 100, 0.01, seed=12, n_frac=0.05)
    offs, lens = chunks_by_records(fq, 10)
    assert len(offs) == 12
    one, three = (mk(qb=qb, k=k, max_batch_bytes=1 << 20, max_batch_keys=1 << 16, max_level_bits=2) for _ in range(2))
    exp = Expect(qb)
    sample_and_check(one, exp, fq, offs, lens, k, s, "one call")
    tot = {"kmers": 0, "kept": 0}
    for i in range(0, 12, 4):
        _, ss = three.sample_chunks(fq, offs[i:i + 4], lens[i:i + 4], s)
        for key in tot:
            tot[key] += ss[key]
    hashes = hashes_of(fq, offs, lens, k)
    assert tot == {"kmers": len(hashes), "kept": len(kept_of(hashes, qb + 8, s))}
    assert three.blocks() == one.blocks()
    exp.check(three, "three calls")
    three.close()
    # the same call again: every kept key twice
    st, ss = one.sample_chunks(fq, offs, lens, s)
    assert st["new_distinct"] == 0 and ss["kept"] == tot["kept"]
    exp.add(hashes, s)
    exp.check(one, "second identical call")
    dump = dict(one.dump())
    assert dump and all(c % 2 == 0 for c in dump.values())
    one.close()
    exp.free()


def run_geometry(mk, qb, mlb, k=47, s=1):
    """case 5: one-, two- and three-level contexts on the same input"""
    fq = synth.make_fastq(synth.make_genome(1500, 4), 50, 110, 0.01, seed=6, n_frac=0.05)
    offs, lens = chunks_by_records(fq, 9)
    exp = Expect(qb)
    ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 20, max_batch_keys=1 << 16, max_level_bits=mlb)
    sample_and_check(ctx, exp, fq, offs, lens, k, s, ("geometry", qb, mlb))
    sample_and_check(ctx, exp, fq, offs[:3], lens[:3], k, s, ("geometry, second call", qb, mlb))
    ctx.close()
    exp.free()


def run_trigger(mk, k=31, s=1, qb=13):
    """case 6: a context with one round and a trigger below the kept distinct count fires exactly one round, behind the call"""
    fq = synth.make_fastq(synth.make_genome(2500, 8), 100, 100, 0.01, seed=3)
    offs, lens = chunks_by_records(fq, 20)
    hashes = hashes_of(fq, offs, lens, k)
    exp = Expect(qb)
    kept = exp.add(hashes, s)
    ndist = exp.q.ndistinct()
    removed = exp.q.denoise_round(64)
    assert removed > 0
    ctx = mk(qb=qb, k=k, trigger=ndist // 2, num_denoise=1, min_denoise_len=64, max_batch_bytes=1 << 20, max_batch_keys=1 << 16,
             max_level_bits=2)
    st, ss = ctx.sample_chunks(fq, offs, lens, s)
    assert (st["denoise_rounds"], st["removed"], st["kmers"], st["chunks"]) == (1, removed, len(kept), 1), st
    assert ss == {"kmers": len(hashes), "kept": len(kept)}
    assert ctx.blocks() == exp.q.blocks()
    assert ctx.totals().rounds_left == 0
    ctx.close()
    exp.free()


def run_errors(mk, dev_bytes):
    """case 7: every error of the contract; after each the table bytes are unchanged and a good call gives the right table.
    dev_bytes(b) -> (pointer the library can read, keep-alive)"""
    import shk
    k, qb = 31, 12
    fq = synth.make_fastq(synth.make_genome(800, 3), 30, 90, 0.01, seed=5, n_frac=0.05)
    offs, lens = chunks_by_records(fq, 10)
    more = plain_reads(12, 100, 23)

    def expect_err(ctx, code, *a, **kw):
        before = ctx.blocks()
        try:
            ctx.sample_chunks(*a, **kw)
        except shk.ShkError as e:
            assert e.code == code, (e.code, code)
        else:
            raise AssertionError("no error %d" % code)
        assert ctx.blocks() == before

    exp = Expect(qb)
    ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 18, max_batch_keys=1 << 14, max_level_bits=2)
    sample_and_check(ctx, exp, fq, offs, lens, k, 1, "before the errors")
    expect_err(ctx, -1, fq, offs, lens, 25)                             # sample_bits > 24
    expect_err(ctx, -1, fq, offs, lens, 37)                             # hb + sample_bits = 57 (and > 24)
    ptr, keep = dev_bytes(b"\n" * 16 + fq)
    expect_err(ctx, -1, ptr + 1, [o + 15 for o in offs], lens, 1, on_device=True, text_bytes=len(fq) + 15)      # unaligned device text
    expect_err(ctx, -7, fq, [], [], 1)                                  # nchunks 0
    expect_err(ctx, -7, fq, [0] * 4097, [0] * 4097, 1)                  # nchunks 4097
    long_read = b"@long\n" + b"ACGT" * 16384 + b"\n+\n" + b"I" * 65536 + b"\n"
    expect_err(ctx, -6, fq + long_read, [0], [len(fq) + len(long_read)], 1)      # one read of 65536 bases
    ctx.prepare_chunks(more, [0], [len(more)])
    expect_err(ctx, -7, fq, offs, lens, 1)                              # a batch prepared and not yet counted
    ctx.count_prepared()
    for x in kept_of(hashes_of(more, [0], [len(more)], k), qb + 8, 0):
        exp.q.insert(x)
    exp.check(ctx, "the prepared batch")
    # aligned device text works, and the table is right after all of the above
    hashes = hashes_of(fq, offs, lens, k)
    kept = exp.add(hashes, 1)
    st, ss = ctx.sample_chunks(ptr + 16, offs, lens, 1, on_device=True, text_bytes=len(fq))
    assert ss == {"kmers": len(hashes), "kept": len(kept)}
    exp.check(ctx, "device text after the errors")
    ctx.close()
    exp.free()
    # hb + sample_bits = 57 with sample_bits <= 24: a filter of 2^25 slots (hb = 33)
    big = mk(qb=25, k=k, max_batch_bytes=1 << 16, max_batch_keys=1 << 12)
    try:
        big.sample_chunks(fq[:lens[0]], [0], [lens[0]], 24)
    except shk.ShkError as e:
        assert e.code == -1
    else:
        raise AssertionError("hb + sample_bits = 57 was taken")
    assert (big.totals().nelts, big.totals().ndistinct) == (0, 0)
    big.close()
    # kept words beyond max_batch_keys, reached with s = 0; the same context takes the batch at s = 3
    exp = Expect(qb)
    ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 18, max_batch_keys=1024, max_level_bits=2)
    assert len(hashes) > 1024 > len(kept_of(hashes, qb + 8, 3))
    expect_err(ctx, -7, fq, offs, lens, 0)
    sample_and_check(ctx, exp, fq, offs, lens, k, 3, "after too many kept words")
    ctx.close()
    exp.free()
    # a sharded context
    sh = mk(qb=qb, k=k, max_batch_bytes=1 << 18, max_batch_keys=1 << 14, num_shards=2, shard_index=1)
    expect_err(sh, -1, fq, offs, lens, 1)
    sh.close()


# ---------------------------------------------------------------- the tool
def format_case():
    """hand-written numbers for format_estimate: (hist, totals, sstats_sum, s, k, false_max, text)"""
    hist = [40, 10, 0, 5]
    totals = {"distinct": 55, "total": 80, "sumsq": 0, "max_count": 4}
    sstats = {"kmers": 700, "kept": 80}
    # scaled by 2^3: F0 = 440, f1 = 320, f2 = 80, f4 = 40; n = 440 - 320 - 80 = 40; e = 1 - ((700 - 320 - 160) / 700)^(1/10)
    e = 1.0 - (220 / 700.0) ** (1.0 / 10)
    want = "sampled\t1/2^3\t55\nF1\t700\nF0\t440\nf1\t320\nf2\t80\nf4\t40\nsuggested: -N 700 -n 40 -e %.5f\n" % e
    return hist, totals, sstats, 3, 10, 2, want


def oracle_estimate(path, k, qb, s, part_size, overhead, bins):
    """(hist, totals, sstats_sum) the tool must find for a plain FASTQ file cut into the chunker's parts"""
    import numpy as np
    O = cqflibs.oracle()
    fq = open(path, "rb").read()
    sizes = O.chunk_sizes(path, part_size, overhead)
    assert sum(sizes) == len(fq) and len(sizes) > 1
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    hashes = hashes_of(fq, offs, sizes, k)
    kept = kept_of(hashes, qb + 8, s)
    assert 0 < len(kept) < len(hashes)
    uniq, cnt = np.unique(np.array(kept, dtype=np.uint64), return_counts=True)
    hist = [int(((cnt == i + 1) if i < bins - 1 else (cnt >= bins)).sum()) for i in range(bins)]
    totals = {"distinct": len(uniq), "total": len(kept), "max_count": int(cnt.max())}
    return hist, totals, {"kmers": len(hashes), "kept": len(kept)}
