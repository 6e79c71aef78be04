"""Slots instead of counting passes above the last partition level (csrc/shk_api.hip: shk_ctx::roll_slots, roll_keys,
partition_stage; csrc/roll_kernels.hip: k_roll_slot_ends; csrc/partition_kernels.hip: bucket ends). Shared by the
emulator tests and the GPU tests of tests/test_roll_slots.py. The yardstick is the oracle throughout; `k_roll_hist` and
`k_rp_hist` in profile_get() are the observables for which path ran.

The rule: a context of three levels whose middle level may be narrow and whose last level may slot, with
max_batch_keys / (P0 * P1) >= 28,800, runs a narrow batch of text (shk_count_chunks, shk_prepare_chunks) without
k_roll_hist: k_roll_scatter writes into level-0 slots, the middle level into level-1 slots of narrow records, the last
level into region slots as before. A slot above the last level that overflows raises SHK_E_SLOT_FULL_UP inside the
library; the batch's front end then runs again from the 2-bit staging on with the histogram pass (`k_roll_hist` once in
that batch's profile), and two such batches in a row switch the upper slots off. SHK_ROLL_SLOTS=0, read when a context
is created, keeps every batch on the histogram pass: every group below runs in a fresh child process, once as built and
once with the variable set (python roll_slots_cases.py BACKEND GROUP), and asserts there.

Common shape: (3, 3, 2) at qb 16, k = 31, max_batch_keys = 2^21 (a level-1 bucket's share of a full batch: 32,768),
about 2,000 reads of 100 bases (a level-1 share of ~2,200 keys against a slot of ~3,000; level 0: ~18,000 against
~30,000)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NARROW, WIDE, ROLL_HIST, RP_HIST, SLOT_CURSORS = "k_rp_scatter<narrow>", "k_rp_scatter", "k_roll_hist", "k_rp_hist", "k_rp_slot_cursors"
K = 31
QB, MLB = 16, 3
MAX_KEYS = 1 << 21
ERR_CORRUPT, ERR_FASTQ, ERR_BATCH = -5, -6, -7           # include/shk.h
EMU_GROUPS = ["clean", "point", "sparse", "overflow1", "overflow0", "twice", "long-read", "shard"]
GPU_GROUPS = EMU_GROUPS + ["wide", "too-many"]


def slots_on():
    return os.environ.get("SHK_ROLL_SLOTS", "") != "0"


def _uniform(nreads=2000, genome=8000, seed=33, gseed=5, prefix="r"):
    import synth
    return synth.make_fastq(synth.make_genome(genome, gseed), nreads, 100, 0.001, seed=seed, n_frac=0.03, short_frac=0.02, name_prefix=prefix)


def _poly(n, L=100):
    return "".join("@p%d\n%s\n+\n%s\n" % (i, "A" * L, "I" * L) for i in range(n)).encode()


def _state(ctx):
    t = ctx.totals()
    return ctx.blocks(), ctx.header(), t.nelts, t.ndistinct


def _ostate(q):
    from fastq_util import oracle_header
    return q.blocks(), oracle_header(q), q.nelts(), q.ndistinct()


def _mk_ctx(mk, fq_bytes, k=K, **kw):
    kw.setdefault("qb", QB)
    kw.setdefault("max_level_bits", MLB)
    kw.setdefault("max_batch_keys", MAX_KEYS)
    ctx = mk(k=k, max_batch_bytes=fq_bytes + 1024, max_batch_reads=fq_bytes // 8 + 4096, **kw)
    ctx.profile(True)
    return ctx


def _hist_free(p, batches=1):
    """a batch that ran on slots at all three levels: no counting pass, two narrow launches"""
    assert ROLL_HIST not in p and RP_HIST not in p, p
    assert p[NARROW][0] == 2 * batches and WIDE not in p and p[SLOT_CURSORS][0] == batches, p


def _hist_path(p, batches=1):
    """the histogram pass, the last level on its own slots"""
    assert p[ROLL_HIST][0] == batches and RP_HIST not in p, p
    assert p[NARROW][0] == 2 * batches and WIDE not in p and p[SLOT_CURSORS][0] == batches, p


def _clean(p, batches=1):
    (_hist_free if slots_on() else _hist_path)(p, batches)


# ------------------------------------------------------------------------------------------------------------ groups
def group_clean(mk, emu):
    """shk_count_chunks in one call and in three, shk_prepare_chunks + shk_count_prepared: table, header, nelts, ndistinct
    and kmers equal the oracle's; no k_roll_hist, no k_rp_hist, two narrow launches per batch (with the switch at 0:
    k_roll_hist once per batch, the same table)"""
    from fastq_util import chunks_by_records, oracle_t1
    fq = _uniform()
    offs, lens = chunks_by_records(fq, 100)
    assert len(offs) == 20
    q, _, _ = oracle_t1(fq, offs, lens, K, QB)
    want = _ostate(q)
    q.free()
    for flow in ("count", "count3", "prepared"):
        ctx = _mk_ctx(mk, len(fq))
        if flow == "count":
            kmers, batches = ctx.count_chunks(fq, offs, lens)["kmers"], 1
        elif flow == "count3":
            kmers, batches = 0, 3
            for a, b in ((0, 7), (7, 13), (13, 20)):
                lo, hi = offs[a], offs[b - 1] + lens[b - 1]
                kmers += ctx.count_chunks(fq[lo:hi], [o - lo for o in offs[a:b]], lens[a:b])["kmers"]
        else:
            ctx.prepare_chunks(fq, offs, lens)
            kmers, batches = ctx.count_prepared()["kmers"], 1
        assert kmers == want[2], (flow, kmers, want[2])
        assert _state(ctx) == want, flow
        _clean(ctx.profile_get(), batches)
        ctx.close()


def group_point(mk, emu):
    """a deNoise point inside the batch: the trigger is the oracle's ndistinct behind chunk 11 of 20, so the round fires
    between two chunks of one slotted batch. Rounds, removed count and table equal the oracle's."""
    import cqflibs
    from fastq_util import chunks_by_records, oracle_t1
    fq = _uniform(genome=12000)
    offs, lens = chunks_by_records(fq, 100)
    point = 11
    O = cqflibs.oracle()
    q = O.new(QB)
    nd = []
    for a, n in zip(offs, lens):
        q.reads_to_kmers(fq[a:a + n], K)
        nd.append(q.ndistinct())
    q.free()
    trigger = nd[point]
    assert nd[point - 1] < trigger
    q, rounds, removed = oracle_t1(fq, offs, lens, K, QB, trigger, 1, False, 1 << 20)
    assert rounds == 1 and removed > 0 and not q.full()
    want = _ostate(q)
    q.free()
    for flow in ("count", "prepared"):
        ctx = _mk_ctx(mk, len(fq), trigger=trigger, num_denoise=1, min_denoise_len=1 << 20)
        if flow == "count":
            st = ctx.count_chunks(fq, offs, lens)
        else:
            ctx.prepare_chunks(fq, offs, lens)
            st = ctx.count_prepared()
        assert (st["denoise_rounds"], st["removed"]) == (rounds, removed), (flow, st, rounds, removed)
        assert _state(ctx) == want, flow
        _clean(ctx.profile_get())
        ctx.close()


def group_sparse(mk, emu):
    """a batch of one read (most level-0 buckets are empty), a batch whose reads are all shorter than k (no words at all),
    and a normal batch behind them in the same context"""
    import random
    import cqflibs
    from fastq_util import chunks_by_records
    uni = _uniform()
    one = b"@one\n" + bytes(random.Random(3).choices(b"ACGT", k=100)) + b"\n+\n" + b"I" * 100 + b"\n"
    short = "".join("@s%d\n%s\n+\n%s\n" % (i, "ACGTTGCA" * 3, "I" * 24) for i in range(40)).encode()
    ctx = _mk_ctx(mk, len(uni))
    q = cqflibs.oracle().new(QB)
    for fq, per, nk in ((one, 1, 100 - K + 1), (short, 10, 0), (uni, 100, None)):
        offs, lens = chunks_by_records(fq, per)
        ctx.profile_reset()
        st = ctx.count_chunks(fq, offs, lens)
        before = q.nelts()
        q.reads_to_kmers(fq, K)
        assert st["kmers"] == q.nelts() - before and (nk is None or st["kmers"] == nk), (st, nk)
        assert _state(ctx) == _ostate(q), len(fq)
        _clean(ctx.profile_get())
    ctx.close()
    q.free()


def _batches(mk, k, plan):
    """plan: (text, records per chunk, check(profile)) in turn through one context, the oracle alongside"""
    import cqflibs
    from fastq_util import chunks_by_records
    ctx = _mk_ctx(mk, max(len(fq) for fq, _, _ in plan), k=k)
    q = cqflibs.oracle().new(QB)
    for i, (fq, per, check) in enumerate(plan):
        offs, lens = chunks_by_records(fq, per)
        ctx.profile_reset()
        ctx.count_chunks(fq, offs, lens)            # (an SHK_E_SLOT_FULL_UP that left the library would raise here)
        q.reads_to_kmers(fq, k)
        assert _state(ctx) == _ostate(q), i
        check(ctx.profile_get())
    ctx.close()
    q.free()


def _redone(p):
    """a batch whose upper slots overflowed: the histogram pass once, no k_rp_hist (the last level's slots hold)"""
    if not slots_on():
        return _hist_path(p)
    assert p[ROLL_HIST][0] == 1 and RP_HIST not in p and p[SLOT_CURSORS][0] == 1 and WIDE not in p, p


def group_overflow1(mk, emu):
    """level-1 overflow only: the uniform text plus 60 poly-A reads gives one k-mer 4,200 times (k = 31) on top of a level-1
    share of ~2,250 against a slot of ~3,100; its level-0 bucket (~22,000 of ~30,000) and its region's slot (16,384) hold.
    Seen in the read-back behind the last level, so that batch runs the partition twice: four narrow launches. Then the
    same with 20 poly-A reads: 1,400 copies put that bucket at ~3,600, behind its slot's end and inside the next slot, so
    an overflow test that is off by one slot lets the run overwrite the neighbour's records."""
    uni, uni2 = _uniform(), _uniform(seed=34, prefix="u")

    def redone(p):
        _redone(p)
        assert p[NARROW][0] == (4 if slots_on() else 2), p
    _batches(mk, K, [(uni2 + _poly(60), 103, redone), (uni, 100, _clean), (uni2 + _poly(20), 101, redone)])


def group_overflow0(mk, emu):
    """level-0 overflow: 3,400 poly-A reads at k = 21 give one key 272,000 times against a level-0 slot of ~75,000. Seen in
    the read-back behind the roll stage: the partition runs once. That key's region overflows the last level's slot as
    well (16,384), which is the last level's own redo (k_rp_hist once) on either path."""
    uni = _uniform()

    def redone(p):
        assert p[ROLL_HIST][0] == 1 and p[RP_HIST][0] == 1 and p[SLOT_CURSORS][0] == 1 and p[NARROW][0] == 3 and WIDE not in p, p
    _batches(mk, 21, [(uni, 100, _clean), (uni + _poly(3400), 270, redone), (uni, 100, _clean)])


def group_twice(mk, emu):
    """two overflow batches in a row switch the upper slots off: a uniform batch afterwards runs the histogram pass (one
    overflow does not: group_overflow1). The last level's own slots and their counter are unaffected (no k_rp_hist anywhere), and
    k_rp_slot_cursors stays one launch per batch throughout."""
    uni, uni2 = _uniform(), _uniform(seed=34, prefix="u")
    over = uni2 + _poly(60)
    _batches(mk, K, [(over, 103, _redone), (over, 103, _redone), (uni, 100, _hist_path)])


def group_long_read(mk, emu):
    """a read of 65,536 bases is SHK_ERR_FASTQ and leaves the state as it was (a slotted batch has no histogram pass to
    find it: k_roll_scatter does); the same batch with the read cut to 65,535 bases then counts"""
    import random
    import cqflibs
    import shk
    from fastq_util import chunks_by_records
    uni = _uniform(nreads=400)
    unit = bytes(random.Random(5).choices(b"ACGT", k=4000))          # (4,000 distinct k-mers 16 times each: the table holds them)
    seq = (unit * 17)[:65536]
    rec = lambda s: b"@long\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"          # noqa: E731
    ctx = _mk_ctx(mk, len(uni) + 2 * 65536 + 64)
    before = _state(ctx)
    fq = uni + rec(seq)
    offs, lens = chunks_by_records(fq, 101)
    code = 0
    try:
        ctx.count_chunks(fq, offs, lens)
    except shk.ShkError as e:
        code = e.code
    assert code == ERR_FASTQ, code
    assert _state(ctx) == before
    fq = uni + rec(seq[:65535])
    offs, lens = chunks_by_records(fq, 101)
    ctx.profile_reset()
    ctx.count_chunks(fq, offs, lens)
    q = cqflibs.oracle().new(QB)
    q.reads_to_kmers(fq, K)
    assert _state(ctx) == _ostate(q)
    _clean(ctx.profile_get())
    ctx.close()
    q.free()


def group_shard(mk, emu):
    """shard 1 of 2 at qb 16 (levels (3, 2, 2), a level-1 share of a full batch of 65,536) fed text whose keys fall anywhere
    in the whole filter: refused with SHK_ERR_CORRUPT, as with the switch at 0, and the table is unchanged. Prints
    {"code": ..} for the parent to compare between the two runs."""
    import shk
    from fastq_util import chunks_by_records
    fq = _uniform()
    offs, lens = chunks_by_records(fq, 100)
    ctx = _mk_ctx(mk, len(fq), shard_index=1, num_shards=2)
    before = _state(ctx)
    code = 0
    try:
        ctx.count_chunks(fq, offs, lens)
    except shk.ShkError as e:
        code = e.code
    assert code == ERR_CORRUPT, code
    assert _state(ctx) == before
    p = ctx.profile_get()
    assert (ROLL_HIST in p) == (not slots_on()) and p[NARROW][0] == 2, p
    ctx.close()
    print(json.dumps({"code": code}))


def group_wide(mk, emu):
    """GPU only, the wide instantiation of the middle level: (5, 5, 5) at qb 23, max_batch_keys = 2^25 (a level-1 share of
    32,768), 50,000 reads: level-0 slots of ~171,000 words under 16384-key windows, so buckets end inside a window and a
    gap follows them"""
    from fastq_util import chunks_by_records, oracle_t1
    fq = _uniform(nreads=50000, genome=400000)
    offs, lens = chunks_by_records(fq, 500)
    q, _, _ = oracle_t1(fq, offs, lens, K, 23)
    want = _ostate(q)
    q.free()
    for flow in ("count", "prepared"):
        ctx = _mk_ctx(mk, len(fq), qb=23, max_level_bits=7, max_batch_keys=1 << 25)
        if flow == "count":
            st = ctx.count_chunks(fq, offs, lens)
        else:
            ctx.prepare_chunks(fq, offs, lens)
            st = ctx.count_prepared()
        assert st["kmers"] == want[2] and _state(ctx) == want, flow
        _clean(ctx.profile_get())
        ctx.close()


def group_too_many(mk, emu):
    """GPU only: a batch of more keys than max_batch_keys (k = 5: 96 keys per read of 100 bases) is SHK_ERR_BATCH, as with
    the switch at 0, and the table is unchanged"""
    import shk
    from fastq_util import chunks_by_records
    fq = _uniform(nreads=23000, genome=100000)
    assert 22000 * 96 > MAX_KEYS
    offs, lens = chunks_by_records(fq, 1000)
    ctx = _mk_ctx(mk, len(fq), k=5)
    before = _state(ctx)
    code = 0
    try:
        ctx.count_chunks(fq, offs, lens)
    except shk.ShkError as e:
        code = e.code
    assert code == ERR_BATCH, code
    assert _state(ctx) == before
    ctx.close()


GROUPS = {"clean": group_clean, "point": group_point, "sparse": group_sparse, "overflow1": group_overflow1, "overflow0": group_overflow0,
          "twice": group_twice, "long-read": group_long_read, "shard": group_shard, "wide": group_wide, "too-many": group_too_many}


def main(argv):
    backend, group = argv[1], argv[2]
    for p in (HERE, ROOT, os.path.join(ROOT, "sh-assembly_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    emu = backend == "emu"
    if not emu:
        import torch  # noqa: F401  (before libshk.so: one HIP runtime per process, see tests/conftest.py)
    import shk
    if emu:
        lib = os.path.join(HERE, "emu", "libshk_emu.so")

        def mk(**kw):
            return shk.Context(threads_per_group=64, hash_groups=2, lib_path=lib, **kw)
    else:
        mk = shk.Context
    GROUPS[group](mk, emu)
    print("ROLL_SLOTS_GROUP_OK")


if __name__ == "__main__":
    main(sys.argv)
