"""Lazy placement: a clean rebuild pass is committed by keeping its run records; the next pass reads them as its old side
(the OLDREC instantiations of k_region_merge) and the table's bytes are produced when somebody looks at them. Shared by the
emulator tests and the GPU tests of tests/test_lazy_place.py. The yardstick is the oracle throughout.

mk_ctx(**kw) -> context with ctx.dev_words(list of key words) -> pointer the library can read (kept alive by the context)."""
import contextlib
import ctypes as C
import os
import random

import cqflibs
import synth
import unitig_compare as UC
from fastq_util import chunks_by_records, oracle_header, oracle_t1

K = 21


@contextlib.contextmanager
def env(**kw):
    """switches the library reads when a context is created / a pass is planned (None = unset)"""
    old = {n: os.environ.get(n) for n in kw}
    try:
        for n, v in kw.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
        yield
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def _ctx(mk_ctx, qb, **kw):
    kw.setdefault("max_batch_bytes", 1 << 21)
    kw.setdefault("max_batch_keys", 1 << 17)
    ctx = mk_ctx(qb=qb, k=K, max_level_bits=2, **kw)
    ctx.profile(True)
    return ctx


def _n(ctx, name):
    return ctx.profile_get().get(name, (0, 0.0))[0]


def _places(ctx):
    return _n(ctx, "k_region_place")


def _reads(seed, nreads=360, G=2800):
    return synth.make_fastq(synth.make_genome(G, seed), nreads, 100, 0.005, seed=seed + 1)


def _batches(fq, per, nb):
    offs, lens = chunks_by_records(fq, per)
    step = (len(offs) + nb - 1) // nb
    return offs, lens, [(offs[i:i + step], lens[i:i + step]) for i in range(0, len(offs), step)]


def _same_totals(ctx, q):
    t = ctx.totals()
    assert (t.nelts, t.ndistinct) == (q.nelts(), q.ndistinct())


def run_chain(mk_ctx):
    """six batches, nobody looks in between: no placement until the first read, exactly one for it, none for the second"""
    qb = 13
    fq = _reads(31)
    offs, lens, bs = _batches(fq, 20, 6)
    assert len(bs) == 6
    ctx = _ctx(mk_ctx, qb)
    for o, l in bs:
        ctx.count_chunks(fq, o, l)
    assert _places(ctx) == 0
    q, _, _ = oracle_t1(fq, offs, lens, K, qb)
    assert not q.full()
    assert ctx.blocks() == q.blocks() and ctx.header() == oracle_header(q)
    _same_totals(ctx, q)
    assert _places(ctx) == 1
    assert ctx.blocks() == q.blocks()
    assert _places(ctx) == 1
    ctx.close()
    q.free()


def run_alternating(mk_ctx):
    """a read after every batch: the synced table and the live records alternate as what a pass and a reader use; with
    SHK_LAZY_PLACE=0 every batch places on its own and the bytes are the same"""
    qb = 13
    fq = _reads(33)
    offs, lens, bs = _batches(fq, 20, 6)
    outs = []
    for lazy in (True, False):
        with env(SHK_LAZY_PLACE=None if lazy else "0"):
            ctx = _ctx(mk_ctx, qb)
        q = cqflibs.oracle().new(qb)
        got = []
        for i, (o, l) in enumerate(bs):
            ctx.count_chunks(fq, o, l)
            assert _places(ctx) == (i if lazy else i + 1)
            for a, n in zip(o, l):
                q.reads_to_kmers(fq[a:a + n], K)
            got.append(ctx.blocks())
            assert got[-1] == q.blocks(), (lazy, i)
            assert _places(ctx) == i + 1
        _same_totals(ctx, q)
        outs.append(got)
        ctx.close()
        q.free()
    assert outs[0] == outs[1]


# (the oracle's points fall on chunks 8 and 11 of 30: behind the fourth chunk of batch 2 and the second of batch 3, five chunks each)
POINT = dict(qb=14, trigger=3000, num_denoise=2, ml=1 << 20, per=12, nb=6)


def point_reads():
    return b"".join(synth.make_fastq(synth.make_genome(2000, 15 + i), 90, 100, 0.005, seed=18 + i, name_prefix="r%d" % i) for i in range(4))


def run_points(mk_ctx, scheme):
    """deNoise points inside batches 2..5 whose old side is the records. scheme "fused": the one-pass point (exact
    position from the general path); "two-pass": SHK_NO_FUSED_POINT, whose k_denoise_marks needs the table's bytes;
    "guess": the sampled guess (every 4th of 64 regions), wrong at least once: the retry reads the untouched old record"""
    P = POINT
    fq = point_reads()
    # (finer chunks for the guess: with 20 to a batch the sample of 16 regions puts the second point one chunk early)
    offs, lens, bs = _batches(fq, 3 if scheme == "guess" else P["per"], P["nb"])
    assert len(bs) == 6
    q, orounds, oremoved = oracle_t1(fq, offs, lens, K, P["qb"], P["trigger"], P["num_denoise"], False, P["ml"])
    assert not q.full() and orounds >= 2
    sw = dict(SHK_NO_FUSED_POINT="1" if scheme == "two-pass" else None, SHK_SAMPLE_STRIDE="4" if scheme == "guess" else None)
    with env(**sw):
        ctx = _ctx(mk_ctx, P["qb"], trigger=P["trigger"], num_denoise=P["num_denoise"], min_denoise_len=P["ml"])
        per_batch = []
        for o, l in bs:
            st = ctx.count_chunks(fq, o, l)
            per_batch.append((st["denoise_rounds"], st["removed"]))
    assert (sum(r for r, _ in per_batch), sum(x for _, x in per_batch)) == (orounds, oremoved)
    assert per_batch[0][0] == 0 and sum(r for r, _ in per_batch[1:5]) >= 2, per_batch      # the points lie in batches 2..5
    nfused = _n(ctx, "k_region_merge<fused>")
    if scheme == "two-pass":
        assert nfused == 0 and _n(ctx, "k_denoise_marks") >= orounds and _places(ctx) >= 1
    else:
        assert nfused >= 2
    if scheme == "guess":
        assert _n(ctx, "k_region_merge<sample>") >= 2 and nfused > orounds, (nfused, orounds)    # a guess was wrong
    assert ctx.blocks() == q.blocks() and ctx.header() == oracle_header(q)
    _same_totals(ctx, q)
    ctx.close()
    q.free()


def _words(ctx, q, pairs):
    """counted keys -> one word per occurrence, shuffled; the oracle gets the same"""
    ws = [k for k, c in pairs for _ in range(c)]
    random.Random(len(ws)).shuffle(ws)
    ctx.count_words(ctx.dev_words(ws), len(ws), 1)
    for k, c in pairs:
        q.insert(k, c)


def run_over_list(mk_ctx):
    """what makes a commit eager, and what follows it. A counted insert places at once; the batch after it rebuilds from the
    table and is lazy again, as is the one after that. A region whose runs do not fit a record (more than
    SHK_SPILL_PACK_MAX bytes) goes to the over list and is written by the write pass from the table -- in that batch and,
    because the region stays as full as it is, in every batch after it; likewise a run of more than 255 slots."""
    qb = 12
    rnd = random.Random(3)

    def scatter(n):
        return [(((rnd.randrange(1 << qb)) << 8) | rnd.randrange(256), rnd.choice([1, 1, 2, 5])) for _ in range(n)]
    # ~300 distinct keys of region 3, three slots each (count 120 behind a remainder < 100: [r, 0, 119]): 900 bytes
    fat = list({(((3 * 256 + rnd.randrange(256)) << 8) | rnd.randrange(100)): 120 for _ in range(330)}.items())
    assert len(fat) >= 300
    # one quotient with 100 remainders of three slots: a run of 300 slots
    long_run = [(((9 * 256 + 17) << 8) | r, 120) for r in range(100)]
    counted = [(k, c + 300) for k, c in scatter(50)]
    # (pairs, counted insert?, placements: 0 = a lazy commit, 1 = at least one, write passes over the list)
    mixed = [(scatter(300), False, 0, 0), (scatter(200), False, 0, 0), (counted, True, 1, 0), (scatter(200), False, 0, 0),
             (scatter(200), False, 0, 0), (fat, False, 1, 1), (scatter(200), False, 1, 1), (long_run, False, 1, 1),
             (scatter(100), False, 1, 1)]
    # the order of the case as it was asked for: the fat region in the first batch (no old side at all), the long run in
    # the second (its old side is the table the first batch placed), plain batches behind them. They cannot turn lazy
    # again: nothing but a deNoise round empties the fat region, so it is on the over list of every later pass
    fat_first = [(fat, False, 1, 1), (long_run, False, 1, 1), (scatter(200), False, 1, 1), (scatter(200), False, 1, 1)]
    for plan, read_every in ((mixed, False), (mixed, True), (fat_first, False), (fat_first, True)):
        ctx = _ctx(mk_ctx, qb)
        q = cqflibs.oracle().new(qb)
        for i, (pairs, is_counted, nplace, nwrite) in enumerate(plan):
            before = _places(ctx), _n(ctx, "k_region_merge<write>")
            if is_counted:
                ctx.insert_counted([k for k, _ in pairs], [c for _, c in pairs])
                for k, c in pairs:
                    q.insert(k, c)
            else:
                _words(ctx, q, pairs)
            got = _places(ctx) - before[0]
            assert (got >= 1) if nplace else (got == 0), (i, got)
            assert _n(ctx, "k_region_merge<write>") - before[1] == nwrite, i
            if read_every:
                assert ctx.blocks() == q.blocks(), i
        assert not q.full()
        assert ctx.blocks() == q.blocks() and ctx.header() == oracle_header(q)
        _same_totals(ctx, q)
        ctx.close()
        q.free()


def run_failed_pass(mk_ctx):
    """a batch that overfills the table fails before anything is committed: records, free pointers and totals stay"""
    import shk
    qb = 10
    rnd = random.Random(5)
    ctx = _ctx(mk_ctx, qb)
    q = cqflibs.oracle().new(qb)

    def some(n):
        return [((rnd.randrange(1 << qb) << 8) | rnd.randrange(256), rnd.choice([1, 2, 3])) for _ in range(n)]
    too_many = [(k, 1) for k in {(rnd.randrange(1 << qb) << 8) | rnd.randrange(256) for _ in range(1700)}]
    _words(ctx, q, some(120))
    _words(ctx, q, some(120))
    for read_first in (False, True):
        try:
            ws = [k for k, _ in too_many]
            ctx.count_words(ctx.dev_words(ws), len(ws), 1)
            raise AssertionError("the batch fits?")
        except shk.ShkError as e:
            assert e.code in (-3, -4), e.code      # SHK_ERR_TABLE_FULL / SHK_ERR_REGION
        _same_totals(ctx, q)
        if read_first:
            assert ctx.blocks() == q.blocks()
        _words(ctx, q, some(60))
        assert ctx.blocks() == q.blocks()
        _same_totals(ctx, q)
    ctx.close()
    q.free()


def _select_seeds(ctx, text):
    L = ctx.L
    L.shk_select_seeds.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.POINTER(C.c_uint32),
                                   C.c_uint32, C.POINTER(C.c_uint32)]
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(text))
    buf = C.create_string_buffer(text, len(text))
    cap = 4096
    seeds, counts, n = C.create_string_buffer(cap * K), (C.c_uint32 * cap)(), C.c_uint32()
    assert L.shk_select_seeds(ctx.h, C.cast(buf, C.c_void_p), 0, len(text), off, ln, 1, K, 2, 1000000, 0, seeds, counts, cap, C.byref(n)) == 0
    return seeds.raw[:n.value * K], list(counts[:n.value])


def run_readers(mk_ctx, UnitigSet, tmp_path):
    """every reader of the table, each directly behind lazy batches: what an eager context gives for the same calls (and
    what the oracle gives, where it has the call)"""
    qb = 14
    fq = _reads(37, 240)
    offs, lens, bs = _batches(fq, 20, 3)
    fq2 = _reads(39, 120)
    offs2, lens2, bs2 = _batches(fq2, 20, 2)
    q, _, _ = oracle_t1(fq, offs, lens, K, qb)
    q2, _, _ = oracle_t1(fq2, offs2, lens2, K, qb)

    def built(lazy, text=fq, batches=bs):
        with env(SHK_LAZY_PLACE=None if lazy else "0"):
            ctx = _ctx(mk_ctx, qb)
        for o, l in batches:
            ctx.count_chunks(text, o, l)
        assert _places(ctx) == (0 if lazy else len(batches))
        return ctx

    def lookup(ctx):
        keys = [kc[0] for kc in q.dump()[:200]] + [12345, (1 << (qb + 8)) - 1]
        got = ctx.lookup(keys, mode=2)[0]
        assert got == [q.count(x) for x in keys]
        return got

    def dump(ctx):
        got = ctx.dump()
        assert got == q.dump()
        return got

    def export_import(ctx):
        p = str(tmp_path / "x.cqf")
        ctx.export_cqf(p)
        c2 = _ctx(mk_ctx, qb)
        c2.import_cqf(p)
        c2.count_chunks(fq2, offs2, lens2)      # (and a pass on top of the imported table)
        got = (open(p, "rb").read(), c2.blocks())
        c2.close()
        assert got[0][128:] == q.blocks()
        return got

    def merge(ctx):
        other = built(ctx.lazy, fq2, bs2)
        ctx.merge(other)
        other.close()
        qm = cqflibs.oracle().new(qb)
        for kk, cc in q.dump() + q2.dump():
            qm.insert(kk, cc)
        got = ctx.blocks()
        assert got == qm.blocks()
        qm.free()
        return got

    def seeds(ctx):
        return _select_seeds(ctx, fq)

    def contiger(ctx):
        # read by read, the schedule under which the device's result is determined (tests/contiger_cases.py: all chunks in
        # one call leave who finds a unitig first, and with it km, to the order the waves run in), and compared as that
        # file compares: canonical sequences with km and KC, and the canonical link set
        u = UnitigSet(ctx)
        o1, l1 = chunks_by_records(fq, 1)
        n = sum(u.add_reads(fq[a:a + b], [0], [b], K, 2, 2, 1000000, 1 << 16) for a, b in zip(o1, l1))
        out = str(tmp_path / "u.fa")
        st = u.write(K, out)
        u.close()
        assert st["truncated"] == 0 and st["unitigs"] > 0
        units, links, invalid = UC.canonical(UC.parse(open(out, "rb").read(), K), K)
        assert invalid == 0
        return n, st["unitigs"], units, links

    for reader in (lookup, dump, export_import, merge, seeds, contiger):
        res = []
        for lazy in (True, False):
            ctx = built(lazy)
            ctx.lazy = lazy
            res.append(reader(ctx))
            assert _places(ctx) >= 1
            assert ctx.blocks() == ctx.blocks()
            ctx.close()
        assert res[0] == res[1], reader.__name__
    q.free()
    q2.free()


def run_prepared(mk_ctx):
    """the overlapped front end: prepare_chunks / count_prepared over four batches, read at the end"""
    qb = 13
    fq = _reads(41, 320)
    offs, lens, bs = _batches(fq, 20, 4)
    ctx = _ctx(mk_ctx, qb)
    ctx.prepare_reserve()
    ctx.prepare_chunks(fq, *bs[0])
    for i in range(4):
        if i + 1 < 4:
            ctx.prepare_chunks(fq, *bs[i + 1])
        ctx.count_prepared()
    assert _places(ctx) == 0
    q, _, _ = oracle_t1(fq, offs, lens, K, qb)
    assert ctx.blocks() == q.blocks() and ctx.header() == oracle_header(q)
    assert _places(ctx) == 1
    ctx.close()
    q.free()


def run_partial_region(mk_ctx):
    """tables whose last (only) region has fewer than 256 quotients: qb 6 and 7, and a shard of 128 quotients"""
    for qb in (6, 7):
        fq = synth.make_fastq(synth.make_genome(50, 3 + qb), 6, 40, 0.0, seed=2)
        offs, lens, bs = _batches(fq, 2, 3)
        ctx = _ctx(mk_ctx, qb, max_batch_bytes=1 << 16, max_batch_keys=1 << 12)
        q = cqflibs.oracle().new(qb)
        for o, l in bs:
            ctx.count_chunks(fq, o, l)
            for a, n in zip(o, l):
                q.reads_to_kmers(fq[a:a + n], K)
        assert not q.full() and _places(ctx) == 0
        assert ctx.blocks() == q.blocks() and ctx.header() == oracle_header(q)
        assert _places(ctx) == 1
        ctx.close()
        q.free()
    # shard 2 of 4 of a 512-slot filter: quotients [256, 384); against an eager context of the same shape
    rnd = random.Random(9)
    res = []
    batches = [[(((256 + rnd.randrange(128)) << 8) | rnd.randrange(256)) for _ in range(40)] for _ in range(3)]
    for lazy in (True, False):
        with env(SHK_LAZY_PLACE=None if lazy else "0"):
            ctx = _ctx(mk_ctx, 9, shard_index=2, num_shards=4, max_batch_bytes=64, max_batch_keys=1 << 10)
        for ws in batches:
            ctx.count_words(ctx.dev_words(ws), len(ws), 1)
        assert _places(ctx) == (0 if lazy else 3)
        res.append((ctx.blocks(), ctx.dump()))
        ctx.close()
    assert res[0] == res[1]
    want = {}
    for ws in batches:
        for w in ws:
            want[w] = want.get(w, 0) + 1
    assert dict(res[0][1]) == want


def run_sparse(mk_ctx):
    """batches that leave most regions without old runs and without words: the early return must still zero the lengths
    of the record the NEXT pass reads (both record buffers start as whatever the allocator left in them)"""
    qb = 14
    rnd = random.Random(13)
    ctx = _ctx(mk_ctx, qb)
    q = cqflibs.oracle().new(qb)
    for regions in ((1, 5), (5, 9), (1, 20), (33,), (63, 0), (9,)):
        pairs = [(((r * 256 + rnd.randrange(256)) << 8) | rnd.randrange(256), rnd.choice([1, 2, 200])) for r in regions for _ in range(30)]
        _words(ctx, q, pairs)
    assert _places(ctx) == 0
    assert ctx.blocks() == q.blocks() and ctx.header() == oracle_header(q)
    _same_totals(ctx, q)
    ctx.close()
    q.free()
