"""The 4-byte record between the level in front of the last partition level and the last one (csrc/partition_kernels.hip:
the narrow record; csrc/shk_api.hip: ShkPartLevel::may_narrow, partition_stage). Shared by the emulator tests and the GPU
tests of tests/test_narrow_records.py. The yardstick is the oracle throughout; `k_rp_scatter<narrow>` in profile_get() is the
observable for which path ran.

The rule: a batch is narrow when its context has at least three levels, its words come from text (shk_count_chunks,
shk_prepare_chunks: the host knows the chunk count) and the call's chunks are at most 1 << cb, cb = 16 - (last level's digit
bits). Then the level in front of the last one and the last one both run under the narrow key, the levels in front of
them under `k_rp_scatter`. SHK_RP_WORDS8=1, read when a context is created, keeps every batch on 8-byte words: every group
below runs in a fresh child process, once as built and once with the variable set (python narrow_cases.py BACKEND GROUP),
and asserts there; the parent test only looks at the exit status (and, for `corrupt`, compares the two error codes).

| geometry | qb | max_level_bits | levels    | cb | narrow                        | emulator |
|----------|----|----------------|-----------|----|-------------------------------|----------|
| one      | 12 | 0              | (4)       |    | never                         | yes      |
| two      | 14 | 3              | (3,3)     |    | never                         | yes      |
| three    | 16 | 3              | (3,3,2)   | 14 | every chunk count             | yes      |
| four     | 18 | 3              | (3,3,2,2) | 14 | levels 2 and 3; level 1 wide  | GPU only |
| edge     | 23 | 7              | (5,5,5)   | 11 | 2048 chunks yes, 2049 no; with a deNoise point behind chunk 1535 the tags decide the result | GPU only |
| shard    | 16 | 3, shard 1 of 2| (3,2,2)   | 14 | yes                           | yes      |

Texts: ~2,000 reads of 100 bases, k = 31, max_batch_keys = 2^20, as tests/partition_cases.py has them."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NARROW, WIDE = "k_rp_scatter<narrow>", "k_rp_scatter"
K = 31
MAX_KEYS = 1 << 20
#          qb  max_level_bits  levels
GEOM = {
    "one":   (12, 0, (4,)),
    "two":   (14, 3, (3, 3)),
    "three": (16, 3, (3, 3, 2)),
    "four":  (18, 3, (3, 3, 2, 2)),
    "edge":  (23, 7, (5, 5, 5)),
}
EMU_GROUPS = ["three", "three-4096", "never", "words", "slots", "corrupt", "windows"]
GPU_GROUPS = ["three", "three-4096", "four", "edge", "edge-point", "never", "words", "slots", "corrupt", "windows"]


def words8():
    return os.environ.get("SHK_RP_WORDS8", "") not in ("", "0")


def cb_of(levels):
    return 16 - levels[-1]


def expect_narrow(levels, nchunks):
    """the rule, for a batch of text"""
    return not words8() and len(levels) >= 3 and nchunks <= (1 << cb_of(levels))


def _rec(i, seq):
    return b"@r%d\n%s\n+\n%s\n" % (i, seq, b"I" * len(seq))


def _reads(rnd, lens):
    return [_rec(i, bytes(rnd.choices(b"ACGT", k=L))) for i, L in enumerate(lens)]


def _tile(recs, per):
    offs, lens, pos = [], [], 0
    for i in range(0, len(recs), per):
        n = sum(len(r) for r in recs[i:i + per])
        offs.append(pos)
        lens.append(n)
        pos += n
    return offs, lens


def _oracle(fq, offs, lens, k, qb):
    from fastq_util import oracle_header, oracle_t1
    q, _, _ = oracle_t1(fq, offs, lens, k, qb)
    assert not q.full()
    want = (q.blocks(), oracle_header(q), q.nelts(), q.ndistinct())
    q.free()
    return want


def _state(ctx):
    t = ctx.totals()
    return ctx.blocks(), ctx.header(), t.nelts, t.ndistinct


def _check_profile(prof, levels, nchunks, batches, what):
    """the narrow key exactly where the rule says: both of the last two levels under it, the levels in front of them (level
    0 of a context of two levels or more is the roll kernels') under the wide key"""
    nrp = len(levels) - 1 if len(levels) >= 2 else 1          # k_rp_scatter levels per batch
    narrow = expect_narrow(levels, nchunks)
    got_n = prof.get(NARROW, (0, 0.0))[0]
    got_w = prof.get(WIDE, (0, 0.0))[0]
    assert got_n == (2 * batches if narrow else 0), (what, "narrow launches", got_n, prof)
    assert got_w == (nrp - 2 if narrow else nrp) * batches, (what, "wide launches", got_w, prof)


def run_text(mk, geom, fq, offs, lens, k=K, flows=("count", "prepared"), want=None):
    """the text through shk_count_chunks and through shk_prepare_chunks + shk_count_prepared, a context each: table blocks,
    header, nelts and ndistinct equal the oracle's, and the narrow key is in the profile exactly where the rule says"""
    qb, mlb, levels = GEOM[geom]
    want = want or _oracle(fq, offs, lens, k, qb)
    for flow in flows:
        ctx = mk(qb=qb, k=k, max_level_bits=mlb, max_batch_bytes=len(fq) + 1024, max_batch_keys=MAX_KEYS,
                 max_batch_reads=fq.count(b"\n") + 4096 + 16)
        ctx.profile(True)
        if flow == "count":
            st = ctx.count_chunks(fq, offs, lens)
        else:
            ctx.prepare_chunks(fq, offs, lens)
            st = ctx.count_prepared()
        assert st["kmers"] == want[2], (geom, flow)
        assert _state(ctx) == want, (geom, flow)
        _check_profile(ctx.profile_get(), levels, len(offs), 1, (geom, flow, len(offs)))
        ctx.close()
    return want


def _genome_text(nchunks_of=100, nreads=2000, genome=8000, err=0.001, seed=33):
    import synth
    from fastq_util import chunks_by_records
    fq = synth.make_fastq(synth.make_genome(genome, 5), nreads, 100, err, seed=seed, n_frac=0.03, short_frac=0.02)
    return (fq,) + tuple(chunks_by_records(fq, nchunks_of))


# ------------------------------------------------------------------------------------------------------------ groups
def group_three(mk, emu):
    """(3, 3, 2), cb = 14 >= 12: 20 chunks, both flows"""
    fq, offs, lens = _genome_text()
    assert len(offs) == 20
    run_text(mk, "three", fq, offs, lens)


def group_three_4096(mk, emu):
    """(3, 3, 2) with a table of 4096 tiny chunks (tests/text_cases.py: k = 5, one record each), so that the chunk tags use
    all 12 bits: still narrow. (The emulator: shk_count_chunks only, as the existing suite does with this text.)"""
    import text_cases as TC
    big = TC._tiny_records(random.Random(52), TC.MAX_CHUNKS)
    offs, lens = TC._tile(big, 1)
    assert len(offs) == 4096 and cb_of(GEOM["three"][2]) >= 12
    run_text(mk, "three", b"".join(big), offs, lens, k=5, flows=("count",) if emu else ("count", "prepared"))


def group_four(mk, emu):
    """(3, 3, 2, 2): only the level in front of the last one writes narrow records, the one before it 8-byte words"""
    fq, offs, lens = _genome_text(genome=12000, err=0.01)
    run_text(mk, "four", fq, offs, lens)


def group_edge(mk, emu):
    """(5, 5, 5), cb = 11: a call of exactly 2048 chunks is narrow, one of 2049 is wide; reads in the last chunk carry the
    highest tag (one record per chunk: the last read's keys are the only ones with it)"""
    rnd = random.Random(61)
    recs = _reads(rnd, [100] * 2049)
    assert cb_of(GEOM["edge"][2]) == 11
    for n in (2048, 2049):
        offs, lens = _tile(recs[:n], 1)
        assert len(offs) == n and lens[-1] > 0
        assert expect_narrow(GEOM["edge"][2], n) == (n == 2048 and not words8())
        run_text(mk, "edge", b"".join(recs[:n]), offs, lens)


def group_edge_point(mk, emu):
    """the chunk field of the narrow record: (5, 5, 5), cb = 11, 2048 chunks of one read each, and ONE deNoise round whose
    trigger is the oracle's ndistinct behind chunk 1535 -- a tag with the field's top bit set. The library finds the point
    from the chunk tags of the partitioned records (the keys of chunks 0 .. 1535 are in the table when the round runs,
    the others are not), so rounds, removed count and table equal the oracle's only if every record carries its chunk's
    whole tag: a tag that lost its top bit would put the reads of chunks 1024 .. 2047 in front of the point."""
    import cqflibs
    from fastq_util import chunks_by_records, oracle_header, oracle_t1
    import synth
    qb, mlb, levels = GEOM["edge"]
    point = 1535
    assert point >= 1 << (cb_of(levels) - 1)
    fq = synth.make_fastq(synth.make_genome(60000, 9), 2048, 100, 0.01, seed=34, n_frac=0.03)
    offs, lens = chunks_by_records(fq, 1)
    assert len(offs) == 2048 == 1 << cb_of(levels)
    O = cqflibs.oracle()
    q = O.new(qb)
    nd = []
    for a, n in zip(offs, lens):
        q.reads_to_kmers(fq[a:a + n], K)
        nd.append(q.ndistinct())
    q.free()
    trigger = nd[point]
    assert nd[point - 1] < trigger            # the round fires behind chunk `point`, not earlier
    q, rounds, removed = oracle_t1(fq, offs, lens, K, qb, trigger, 1, False, 1 << 20)
    assert rounds == 1 and removed > 0 and not q.full()
    want = (q.blocks(), oracle_header(q), q.nelts(), q.ndistinct())
    q.free()
    for flow in ("count", "prepared"):
        ctx = mk(qb=qb, k=K, max_level_bits=mlb, trigger=trigger, num_denoise=1, min_denoise_len=1 << 20,
                 max_batch_bytes=len(fq) + 1024, max_batch_keys=MAX_KEYS, max_batch_reads=2048 + 4096 + 16)
        ctx.profile(True)
        if flow == "count":
            st = ctx.count_chunks(fq, offs, lens)
        else:
            ctx.prepare_chunks(fq, offs, lens)
            st = ctx.count_prepared()
        assert (st["denoise_rounds"], st["removed"]) == (rounds, removed), (flow, st, rounds, removed)
        assert _state(ctx) == want, flow
        prof = ctx.profile_get()
        assert (prof.get(NARROW, (0, 0.0))[0] == 2) == (not words8()) and (WIDE in prof) == words8(), (flow, prof)
        ctx.close()


def group_never(mk, emu):
    """one level and two levels: never narrow"""
    fq, offs, lens = _genome_text(genome=400, err=0.0)
    run_text(mk, "one", fq, offs, lens)
    fq, offs, lens = _genome_text(genome=2000, err=0.0)
    run_text(mk, "two", fq, offs, lens)


def group_words(mk, emu, tmp):
    """part_from_words on the three-level geometry: shk_stage_words (the sharded flow's received words) and a counted insert
    (its words carry a multiplicity in the chunk field). Never narrow; results equal the oracle's (the checker's).
    On the GPU the counted insert also runs at (5, 5, 5), cb = 11, with multiplicities of 3000 > 1 << cb: read as chunk tags
    of a narrow record they would lose their top bit."""
    import pathlib
    import partition_cases as PC
    import f4_scenarios as F
    seen = []

    def recording(**kw):
        ctx = mk(**kw)
        ctx.profile(True)
        close = ctx.close

        def close_and_record():
            if getattr(ctx, "h", None):
                seen.append(ctx.profile_get())
            close()
        ctx.close = close_and_record
        return ctx
    import torch
    from shk import dist as shkdist

    def factory(**kw):
        ctx = recording(**kw)
        ctx.device = torch.device("cpu") if emu else torch.device("cuda", 0)
        return ctx
    PC.run_words(factory, "e", "gloo" if emu else "nccl", pathlib.Path(tmp), ("words",))
    assert len(seen) == 1 and NARROW not in seen[0] and seen[0][WIDE][0] == 3 * 3, seen      # three batches, three levels
    for geom, maxc in (("three", 4000),) + (() if emu else (("edge", 3001),)):
        qb, mlb, levels = GEOM[geom]
        held = []

        def mk_counted(qb_):
            held.append(recording(qb=qb_, k=21, max_batch_keys=1 << 14, max_level_bits=mlb))
            return held[-1]
        rng = random.Random(12)
        kc = F.pairs(rng, qb, 150, maxc) + [((rng.randrange(1 << qb) << 8) | 7, maxc - 1)]
        assert max(c for _, c in kc) == maxc - 1 and (emu or geom != "edge" or maxc - 1 > (1 << cb_of(levels)))
        F.check_counted_and_dump(mk_counted, qb, kc)
        held[0].close()             # (records the profile, unless the check has closed the context already)
        prof = seen[-1]
        assert len(held) == 1 and NARROW not in prof and prof.get(WIDE, (0, 0.0))[0] > 0, (geom, prof)


def group_slots(mk, emu):
    """a slotted last level that overflows on narrow input: one k-mer repeated until its region overflows the slot, as
    roll_cases.run_slots does, on (3, 3, 2). SHK_E_SLOT_FULL stays inside the library, the redo (k_rp_hist over the narrow
    records, then the last level again) gives the oracle's table; after two such batches in a row the slots are off."""
    import cqflibs
    import synth
    from fastq_util import chunks_by_records
    k = 21
    qb, mlb, levels = GEOM["three"]
    uni = synth.make_fastq(synth.make_genome(3000, 5), 250, 100, 0.005, seed=8, n_frac=0.02)
    poly = "".join("@p%d\n%s\n+\n%s\n" % (i, "A" * 100, "I" * 100) for i in range(60)).encode()
    ctx = mk(qb=qb, k=k, max_batch_bytes=1 << 20, max_batch_keys=1 << 16, max_level_bits=mlb)
    ctx.profile(True)
    O = cqflibs.oracle()
    q = O.new(qb)
    narrow = expect_narrow(levels, 5)
    key, other = (NARROW, WIDE) if narrow else (WIDE, NARROW)
    assert narrow == (not words8())

    def batch(fq, per, redo):
        offs, lens = chunks_by_records(fq, per)
        ctx.profile_reset()
        ctx.count_chunks(fq, offs, lens)          # (an SHK_E_SLOT_FULL that left the library would raise here)
        q.reads_to_kmers(fq, k)
        assert ctx.blocks() == q.blocks()
        p = ctx.profile_get()
        assert other not in p and p[key][0] == (3 if redo else 2), p     # the last level runs again after an overflow
        return p

    p = batch(uni, 50, False)
    assert p["k_rp_slot_cursors"][0] == 1 and "k_rp_hist" not in p
    p = batch(poly, 20, True)              # 4800 times one key: 512 fit its slot
    assert p["k_rp_slot_cursors"][0] == 1 and p["k_rp_hist"][0] == 1
    p = batch(uni, 50, False)              # one overflow does not switch the slots off
    assert p["k_rp_slot_cursors"][0] == 1 and "k_rp_hist" not in p
    batch(poly, 20, True)
    batch(poly, 20, True)                  # the second overflow in a row does
    p = batch(uni, 50, False)
    assert "k_rp_slot_cursors" not in p and p["k_rp_hist"][0] == 1
    assert (ctx.totals().nelts, ctx.totals().ndistinct) == (q.nelts(), q.ndistinct())
    ctx.close()
    q.free()


def group_corrupt(mk, emu):
    """shard 1 of 2 at qb 16 (2^15 quotients, 128 regions, levels (3, 2, 2)) fed text whose keys fall anywhere in the whole
    filter: about half lie outside the shard. The check `q >= nslots` sits in the last level for 8-byte words and in the
    level in front of it for narrow batches; both must refuse the batch with the same error and leave the table as it
    was. Through shk_count_chunks (shk_prepare_chunks refuses a shard's context before anything runs). Prints
    {"code": ..} for the parent to compare between the two runs."""
    fq, offs, lens = _genome_text()
    ctx = mk(qb=16, k=K, max_level_bits=3, max_batch_bytes=len(fq) + 1024, max_batch_keys=MAX_KEYS, shard_index=1, num_shards=2)
    ctx.profile(True)
    before = _state(ctx)
    code = 0
    try:
        ctx.count_chunks(fq, offs, lens)
    except Exception as e:
        code = getattr(e, "code", None)
    assert code not in (0, None), code
    assert _state(ctx) == before
    prof = ctx.profile_get()
    assert (prof.get(NARROW, (0, 0.0))[0] == 2) == (not words8()) and (WIDE in prof) == words8(), prof
    ctx.close()
    print(json.dumps({"code": code}))


def group_windows(mk, emu):
    """16384 * m - 1, 16384 * m and 16384 * m + 1 keys entering the level in front of the last one, m = 1, 2 (the edges of
    its 16384-key windows on the GPU): reads of 100 bases give 70 keys each, one longer read lands the total"""
    rnd = random.Random(71)
    for m in (1, 2):
        for d in (-1, 0, 1):
            nkeys = 16384 * m + d
            full, rest = divmod(nkeys, 100 - K + 1)
            recs = _reads(rnd, [100] * (full - 1) + [100 + rest])
            fq = b"".join(recs)
            offs, lens = _tile(recs, 40)
            want = _oracle(fq, offs, lens, K, GEOM["three"][0])
            assert want[2] == nkeys, (want[2], nkeys)
            run_text(mk, "three", fq, offs, lens, flows=("count",), want=want)


GROUPS = {"three": group_three, "three-4096": group_three_4096, "four": group_four, "edge": group_edge, "edge-point": group_edge_point, "never": group_never,
          "words": group_words, "slots": group_slots, "corrupt": group_corrupt, "windows": group_windows}


def main(argv):
    backend, group = argv[1], argv[2]
    for p in (HERE, ROOT, os.path.join(ROOT, "sh-assembly_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    emu = backend == "emu"
    if not emu or group == "words":
        import torch  # noqa: F401  (before libshk.so: one HIP runtime per process, see tests/conftest.py)
    import shk
    if emu:
        lib = os.path.join(HERE, "emu", "libshk_emu.so")

        def mk(**kw):
            return shk.Context(threads_per_group=64, hash_groups=2, lib_path=lib, **kw)
    else:
        mk = shk.Context
    if group == "words":
        GROUPS[group](mk, emu, argv[3])
    else:
        GROUPS[group](mk, emu)
    print("NARROW_GROUP_OK")


if __name__ == "__main__":
    main(sys.argv)
