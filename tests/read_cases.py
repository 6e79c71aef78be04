"""The read side on hard tables: shk_lookup in its three modes, the contract for traveled marks (they belong to readers;
no writer sees them), and the walk kernels on low-complexity sequence. Shared by the emulator tests and the GPU tests of
tests/test_read_side.py. Every table here is a valid table.

mk_ctx(**kw) -> context with
  ctx.dev_words(list of 64-bit words) -> pointer the library can read as device memory (kept alive by the context)
  ctx.dev_out(nbytes) -> (pointer the library can write as device memory, fetch() -> its bytes)"""
import contextlib
import ctypes as C
import os
import random

import cqflibs
import f4_scenarios as F
import synth
from cqf_canon import build_blocks, build_shard_blocks
from fastq_util import chunks_by_records, oracle_t1

BLOCK, OFF_TRAV, OFF_SLOTS = 89, 17, 25


@contextlib.contextmanager
def env(**kw):
    """switches the library reads when a context is created (None = unset)"""
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


# ---------------------------------------------------------------- reading a table's bytes

def _bit(blocks, off, pos):
    return (blocks[(pos >> 6) * BLOCK + off + ((pos & 63) >> 3)] >> (pos & 7)) & 1


def _slot(blocks, pos):
    return blocks[(pos >> 6) * BLOCK + OFF_SLOTS + (pos & 63)]


def runs_of(blocks, nslots):
    """{quotient: (first slot, bytes of its run)} of a valid table: runs lie in quotient order, each at
    max(quotient, end of the run before + 1), and end on the next runend bit"""
    out, free = {}, 0
    total = len(blocks) // BLOCK * 64
    for q in range(nslots):
        if not _bit(blocks, 1, q):
            continue
        start = max(q, free)
        e = start
        while not _bit(blocks, 9, e):
            e += 1
            assert e < total
        out[q] = (start, bytes(_slot(blocks, p) for p in range(start, e + 1)))
        free = e + 1
    return out


def entries_of(run):
    """[(remainder, count, offset of the entry's first slot in the run)] -- the decoder of gqf.c:1263-1313 on one run"""
    out, i = [], 0
    while i < len(run):
        r, c, j = run[i], 1, i + 1
        if j < len(run) and run[j] <= r:
            if run[j] == 0:
                j += 1
            cc = 0
            while run[j] & 0x80:
                cc = cc * 128 + (run[j] & 0x7F)
                j += 1
            c = cc * 128 + run[j] + 1
            j += 1
        out.append((r, c, i))
        i = j
    return out


def set_marks(blocks, nslots, keys, q_lo=0):
    """the table's bytes with the traveled bit of every key in `keys` set on the first slot of its entry"""
    out = bytearray(blocks)
    runs = runs_of(blocks, nslots)
    where = {}
    for q, (start, run) in runs.items():
        for r, _, off in entries_of(run):
            where[((q + q_lo) << 8) | r] = start + off
    for k in keys:
        p = where[k]
        out[(p >> 6) * BLOCK + OFF_TRAV + ((p & 63) >> 3)] |= 1 << (p & 7)
    return bytes(out)


class ShardModel:
    """what the checker is for a whole table, for one quotient-range shard (the checkers have no shard geometry): counts
    from the key multiset, marks as a set, bytes from the canonical layout of tests/cqf_canon.py"""

    def __init__(self, qb, g, nshards, counts):
        self.per = (1 << qb) // nshards
        self.q_lo = self.per * g
        self.mine = {k: c for k, c in counts.items() if self.q_lo <= (k >> 8) < self.q_lo + self.per}
        self.clean = build_shard_blocks(qb, g, nshards, counts)
        self.marked = set()

    def count(self, key):
        return self.mine.get(key, 0)

    def count_is_traveled(self, key):
        return (1 if key in self.marked else 0), self.count(key)

    def count_set_traveled(self, key):
        t = 1 if key in self.marked else 0
        if key in self.mine:
            self.marked.add(key)
        return t, self.count(key)

    def blocks(self):
        return set_marks(self.clean, self.per, self.marked, self.q_lo)

    def free(self):
        pass


# ---------------------------------------------------------------- 1. lookups on hard tables

def table_a():
    """the clump of test_dense_clusters_and_saturated_offsets: 250-400 keys inside 64 quotients, 1500 background keys"""
    rnd = random.Random(7)
    qb, tot = 13, {}
    base = rnd.randrange(0, 5000)
    for _ in range(rnd.choice([250, 400])):
        key = ((base + rnd.randrange(0, 64)) << 8) | rnd.randrange(256)
        tot[key] = tot.get(key, 0) + rnd.choice([1, 1, 2, 3, 200, 20000])
    for _ in range(1500):
        key = (rnd.randrange(1 << qb) << 8) | rnd.randrange(256)
        tot[key] = tot.get(key, 0) + rnd.choice([1, 1, 1, 2])
    canon = build_blocks(qb, qb + 8, tot)
    assert max(canon[b * BLOCK] for b in range(len(canon) // BLOCK)) == 255      # a block offset saturates
    return qb, tot, (base, 64)


def table_b():
    """runs in the overflow tail: 80 keys on the last 24 quotients of a qb-10 filter"""
    qb = 10
    tot = dict(F.pairs(random.Random(10), qb, 80, 300, cluster=(1000, 24)))
    return qb, tot, (1000, 24)


def table_c():
    """entries on quotient 0 and on quotient nslots - 1, remainders 0 and 255 among them; a little background"""
    qb, tot = 10, {}
    rnd = random.Random(12)
    for q in (0, (1 << qb) - 1):
        for i, r in enumerate([0, 1, 0x7F, 0x80, 0xFE, 0xFF]):
            tot[(q << 8) | r] = [1, 2, 129, r + 1, 1, 300][i]
    for _ in range(150):
        tot.setdefault((rnd.randrange(1, (1 << qb) - 1) << 8) | rnd.randrange(256), rnd.choice([1, 1, 2, 7]))
    return qb, tot, (0, 2)


def table_d():
    """codec edges: every remainder of F.REMS with every count of {1, 2, 3, r, r+1, r+2, 128, 129, 16384, 16385, 2^32+5},
    on eleven adjacent quotients (six entries of different lengths in each run)"""
    qb, tot = 10, {}
    for j in range(11):
        for i, r in enumerate(F.REMS):
            c = [1, 2, 3, r, r + 1, r + 2, 128, 129, 16384, 16385, (1 << 32) + 5][(i + j) % 11]
            tot[((500 + j) << 8) | r] = c or 1
    assert {(k & 0xFF, c) for k, c in tot.items()} >= {(r, r + 1) for r in F.REMS}
    return qb, tot, (500, 12)


TABLES = {"clump": table_a, "tail": table_b, "borders": table_c, "codec": table_d}


def queries(qb, tot, clump, blocks, nslots, q_lo, rnd):
    """(present keys, absent keys) of one table. Absent: for every occupied quotient the bytes stored in its run that are
    no remainder of it (counter digits, the 0 escape) and a remainder below, between and above its entries; remainders 0
    and 255 on occupied quotients and on an unoccupied quotient inside the clump; 200 random keys"""
    present = sorted(tot)
    absent = set()
    runs = runs_of(blocks, nslots)
    for q, (_, run) in runs.items():
        rems = [r for r, _, _ in entries_of(run)]
        assert rems == sorted(k & 0xFF for k in tot if (k >> 8) == q + q_lo), q
        cand = set(run) - set(rems)                                   # counter digits, the 0 escape
        if rems[0] > 0:
            cand.add(rems[0] - 1)
        if rems[-1] < 255:
            cand.add(rems[-1] + 1)
        for a, b in zip(rems, rems[1:]):
            if b - a > 1:
                cand.add(a + 1)
                break
        absent |= {((q + q_lo) << 8) | r for r in cand}
    occupied = {k >> 8 for k in tot}
    lo, width = clump
    # an unoccupied quotient inside the clump (a shard that does not hold the clump: its first unoccupied quotient)
    hole = next(q for q in list(range(lo, lo + width)) + list(range(q_lo, q_lo + nslots)) if q not in occupied and q_lo <= q < q_lo + nslots)
    absent |= {(hole << 8) | 0, (hole << 8) | 255, (hole << 8) | 77}
    for q in sorted(occupied)[:3]:
        absent |= {(q << 8) | 0, (q << 8) | 255}
    absent |= {rnd.randrange(1 << (qb + 8)) for _ in range(200)}
    absent -= set(present)
    return present, sorted(absent)


def check_lookups(ctx, q, qb, tot, present, absent, rnd):
    """every mode of shk_lookup on one table against the checker q (whose marks follow the calls made here)"""
    keys = present + absent
    rnd.shuffle(keys)
    assert ctx.lookup([], mode=2) == ([], [])                                              # n = 0 is SHK_OK
    cnt, _ = ctx.lookup(keys, mode=2)
    assert cnt == [q.count(x) for x in keys] == [tot.get(x, 0) for x in keys]
    c0, t0 = ctx.lookup(keys, mode=0)
    assert c0 == cnt and t0 == [q.count_is_traveled(x)[0] for x in keys] and not any(t0)
    # one marking call that holds 50 present keys three times each, scattered among absent ones
    trip = rnd.sample(present, min(50, len(present)))
    call = trip * 3 + absent[:100]
    rnd.shuffle(call)
    c1, t1 = ctx.lookup(call, mode=1)
    assert c1 == [tot.get(x, 0) for x in call]
    for x in trip:
        assert sorted(t for y, t in zip(call, t1) if y == x) == [0, 1, 1], x               # the first to arrive sees 0
        assert q.count_set_traveled(x) == (0, tot[x])
    assert not any(t for y, t in zip(call, t1) if y not in tot)
    # a subset, then an overlapping one; 257 keys (one more than a workgroup) in the second when the table has them
    sub1 = [x for x in keys if x not in trip][::3] + trip[:10]
    sub2 = list(dict.fromkeys(sub1[::2] + keys[1::5] + keys))[:257]      # (no key twice: the order inside a call is free)
    assert len(set(sub1)) == len(sub1)
    for sub in (sub1, sub2):
        c, t = ctx.lookup(sub, mode=1)
        exp = [q.count_set_traveled(x) for x in sub]
        assert (t, c) == ([e[0] for e in exp], [e[1] for e in exp])
    if len(keys) >= 257:
        assert len(sub2) == 257
    # keys, counts and flags in device memory
    dk = ctx.dev_words(keys)
    (pc, fc), (pt, ft) = ctx.dev_out(8 * len(keys)), ctx.dev_out(len(keys))
    ctx._chk(ctx.L.shk_lookup(ctx.h, dk, len(keys), 1, 0, pc, pt))
    exp = [q.count_is_traveled(x) for x in keys]
    assert list((C.c_uint64 * len(keys)).from_buffer_copy(fc())) == [e[1] for e in exp]
    assert list(ft()) == [e[0] for e in exp] and any(e[0] for e in exp)
    # was_traveled = NULL
    arr, out = (C.c_uint64 * len(keys))(*keys), (C.c_uint64 * len(keys))()
    for mode in (0, 1):
        ctx._chk(ctx.L.shk_lookup(ctx.h, C.cast(arr, C.c_void_p), len(keys), 0, mode, C.cast(out, C.c_void_p), None))
        assert list(out) == cnt
    for x in keys:
        q.count_set_traveled(x)
    # bits on the first slot of every marked entry and nowhere else
    assert ctx.blocks() == q.blocks()


def _tail_in_use(blocks, nslots):
    runs = runs_of(blocks, nslots)
    start, run = runs[max(runs)]
    return start + len(run) > nslots


def run_lookups(mk_ctx, name, huge_by_import=False):
    """huge_by_import: a counted insert takes one rebuild per 2^22 occurrences of its largest count, 1025 for 2^32 + 5 --
    a fraction of a second on the card, minutes on the emulator. There the six entries with that count come in as the
    checker's table of them (shk_import_blocks) and every other entry is inserted on top, which rebuilds them too."""
    qb, tot, clump = TABLES[name]()
    lib = F.checker()
    F.fits(qb, list(tot.items()))
    rnd = random.Random(len(tot))
    ctx = mk_ctx(qb=qb, k=21, max_batch_bytes=64, max_batch_keys=1 << 12)
    q = lib.new(qb)
    items = list(tot.items())
    rnd.shuffle(items)
    huge = [(k, c) for k, c in items if c >> 32]
    if huge_by_import and huge:
        for k, c in huge:
            q.insert(k, c)
        ctx.import_blocks(q.blocks(), q.nelts(), q.ndistinct())
        items = [kc for kc in items if kc not in huge]
    for part in (items[::2], items[1::2]):
        ctx.insert_counted([k for k, _ in part], [c for _, c in part])
        for k, c in part:
            q.insert(k, c)
    blocks = q.blocks()
    assert ctx.blocks() == blocks
    if name == "tail":
        assert _tail_in_use(blocks, 1 << qb)               # the free pointer lies behind nslots: runs sit in the tail
    if name == "borders":
        occ = {k >> 8 for k in tot}
        assert 0 in occ and (1 << qb) - 1 in occ
    present, absent = queries(qb, tot, clump, blocks, 1 << qb, 0, rnd)
    check_lookups(ctx, q, qb, tot, present, absent, rnd)
    ctx.close()
    q.free()


def run_lookups_sharded(mk_ctx):
    """table (a)'s keys over four shard contexts: each answers for its own quotients only"""
    qb, tot, clump = table_a()
    G = 4
    per = (1 << qb) // G
    rnd = random.Random(4)
    for g in range(G):
        m = ShardModel(qb, g, G, tot)
        ctx = mk_ctx(qb=qb, k=21, shard_index=g, num_shards=G, max_batch_bytes=64, max_batch_keys=1 << 12)
        ctx.insert_counted(list(m.mine), list(m.mine.values()))
        assert ctx.blocks() == m.clean
        present, absent = queries(qb, m.mine, clump, m.clean, per, m.q_lo, rnd)
        # keys of the shards before and behind, and the quotients just outside on both sides (present there or not)
        foreign = [k for k in tot if (k >> 8) // per in ((g - 1) % G, (g + 1) % G)][:300]
        edge = [((x % (1 << qb)) << 8) | r for x in (m.q_lo - 1, m.q_lo - 2, m.q_lo + per, m.q_lo + per + 1) for r in (0, 1, 128, 255)]
        absent = sorted((set(absent) | set(foreign) | set(edge)) - set(present))
        assert all(m.count(x) == 0 for x in absent)
        check_lookups(ctx, m, qb, m.mine, present, absent, rnd)
        assert m.marked == set(m.mine)
        ctx.close()


# ---------------------------------------------------------------- 2. marks belong to readers

DN = dict(qb=13, k=21, ml=1 << 10)


def denoise_reads():
    return synth.make_fastq(synth.make_genome(1500, 61), 200, 100, 0.004, seed=62)


def denoise_table():
    """(reads, chunk table, unmarked oracle of all the reads, the keys the cases mark: every third present key)"""
    fq = denoise_reads()
    offs, lens = chunks_by_records(fq, 20)
    q, _, _ = oracle_t1(fq, offs, lens, DN["k"], DN["qb"])
    assert not q.full()
    return fq, offs, lens, q, [kc[0] for kc in q.dump()][::3]


def _dn_ctx(mk_ctx, **kw):
    kw.setdefault("min_denoise_len", DN["ml"])
    return mk_ctx(qb=DN["qb"], k=DN["k"], max_batch_bytes=1 << 20, max_batch_keys=1 << 16, **kw)


def _same(ctx, q):
    t = ctx.totals()
    assert (t.nelts, t.ndistinct) == (q.nelts(), q.ndistinct())
    assert ctx.blocks() == q.blocks()


def _mark(ctx, marks):
    _, t = ctx.lookup(marks, mode=1)
    assert not any(t)
    assert all(ctx.lookup(marks, mode=0)[1])


def run_denoise_after_lookup(mk_ctx):
    """(f) mode-1 lookups, then shk_denoise: the round of an oracle nobody marked"""
    fq, offs, lens, q, marks = denoise_table()
    ctx = _dn_ctx(mk_ctx)
    ctx.count_chunks(fq, offs, lens)
    _mark(ctx, marks)
    got, want = ctx.denoise(), q.denoise_round(DN["ml"])
    print("denoise after lookup: removed", got, "expected", want)
    assert got == want
    _same(ctx, q)
    assert not any(ctx.lookup(marks, mode=0)[1])
    ctx.close()
    q.free()


def run_denoise_after_import(mk_ctx):
    """(g) the table comes in through shk_import_blocks with traveled bits set (as a .cqf written behind Contiger has them)"""
    fq, offs, lens, q, marks = denoise_table()
    qm, _, _ = oracle_t1(fq, offs, lens, DN["k"], DN["qb"])
    for x in marks:
        assert qm.count_set_traveled(x)[0] == 0
    ctx = _dn_ctx(mk_ctx)
    ctx.import_blocks(qm.blocks(), qm.nelts(), qm.ndistinct())
    assert ctx.blocks() == qm.blocks() != q.blocks()
    assert all(ctx.lookup(marks, mode=0)[1])                       # the import keeps the marks for the readers
    got, want = ctx.denoise(), q.denoise_round(DN["ml"])
    print("denoise after import: removed", got, "expected", want)
    assert got == want
    _same(ctx, q)
    ctx.close()
    q.free()
    qm.free()


DN_SCHED = dict(trigger=2200, num_denoise=3)      # (test_denoise_schedule_matches_oracle's 8000 of qb 15, scaled to qb 13)


FLOWS = {"default": {}, "lazy_place_0": dict(SHK_LAZY_PLACE="0"), "two_pass": dict(SHK_NO_FUSED_POINT="1")}


def run_denoise_inside_count(mk_ctx, flow):
    """(h) marks, then a counting call inside which a round fires: with the default flow (the one-pass point, whose
    protections are a list), with every commit placing at once, and with the two-pass point (k_denoise_marks). Inside a
    counting call a round always follows the rebuild of the chunks in front of it, so it never meets a reader's marks"""
    fq, offs, lens, q0, _ = denoise_table()
    q0.free()
    P = DN_SCHED
    first = 3
    with env(**FLOWS[flow]):
        ctx = _dn_ctx(mk_ctx, trigger=P["trigger"], num_denoise=P["num_denoise"])
        s1 = ctx.count_chunks(fq, offs[:first], lens[:first])
        assert s1["denoise_rounds"] == 0
        part, _, _ = oracle_t1(fq, offs[:first], lens[:first], DN["k"], DN["qb"])
        _mark(ctx, [kc[0] for kc in part.dump()][::3])
        part.free()
        s2 = ctx.count_chunks(fq, offs[first:], lens[first:])
    q, rounds, removed = oracle_t1(fq, offs, lens, DN["k"], DN["qb"], P["trigger"], P["num_denoise"], False, DN["ml"])
    assert not q.full() and rounds >= 1
    print("denoise inside count (%s): removed" % flow, s2["removed"], "expected", removed)
    assert (s2["denoise_rounds"], s2["removed"]) == (rounds, removed)
    _same(ctx, q)
    ctx.close()
    q.free()


def run_denoise_staged(mk_ctx, path):
    """(i) marks, then the staged rounds on a one-shard context. "try": shk_stage_try_denoise + shk_stage_accept with
    forty staged words behind the round; "point": shk_stage_round_try / _point_walk / _point_finish / shk_stage_accept"""
    fq, offs, lens, q, marks = denoise_table()
    ctx = _dn_ctx(mk_ctx)
    ctx.count_chunks(fq, offs, lens)
    _mark(ctx, marks)
    want = q.denoise_round(DN["ml"])
    if path == "try":
        rnd = random.Random(8)
        words = [rnd.randrange(1 << (DN["qb"] + 8)) for _ in range(40)]
        ctx.stage_words(ctx.dev_words(words), len(words))
        s = ctx.stage_try_denoise(0, 0)
        assert not s.err_bits
        new = sum(q.insert(w, 1) for w in words)
        print("staged try_denoise: removed", s.removed, "expected", want)
        assert (s.removed, s.added, s.new_distinct) == (want, len(words), new)
        ctx.stage_accept(s)
    else:
        p = ctx.stage_round_try()
        assert not p.err_bits
        _, nprot, web = ctx.stage_point_walk(0, -1, True, 0, (0, 0))
        assert not web
        acc = ctx.stage_point_finish(p)
        assert not acc.err_bits
        print("staged round: removed", p.removed, "expected", want, "protected", nprot)
        assert p.removed == want
        ctx.stage_accept(acc)
    _same(ctx, q)
    ctx.close()
    q.free()


def run_writers_drop_marks(mk_ctx, writer):
    """(j) marks, then a plain writer: afterwards no key is marked and the bytes are an unmarked checker's"""
    lib = F.checker()
    qb = 12
    rnd = random.Random(21)
    kc = F.pairs(rnd, qb, 500, 400) + F.pairs(rnd, qb, 120, 400, cluster=(700, 40))
    kc = list(dict(kc).items())
    more = list(dict(F.pairs(rnd, qb, 200, 50) + [(k, 3) for k, _ in kc[::7]]).items())
    F.fits(qb, kc + more)
    ctx = mk_ctx(qb=qb, k=21, max_batch_bytes=1 << 16, max_batch_keys=1 << 14)
    ctx.insert_counted([k for k, _ in kc], [c for _, c in kc])
    q = F.build(lib, qb, kc)
    assert ctx.blocks() == q.blocks()
    _mark(ctx, [k for k, _ in kc][::2])
    assert ctx.blocks() != q.blocks()
    if writer == "count_words":
        ws = [k for k, c in more for _ in range(c)]
        rnd.shuffle(ws)
        ctx.count_words(ctx.dev_words(ws), len(ws), 1)
    elif writer == "insert_counted":
        ctx.insert_counted([k for k, _ in more], [c for _, c in more])
    else:
        other = mk_ctx(qb=qb, k=21, max_batch_bytes=1 << 16, max_batch_keys=1 << 14)
        other.insert_counted([k for k, _ in more], [c for _, c in more])
        _mark(other, [k for k, _ in more][::2])                        # (nor do the source's marks travel)
        ctx.merge(other)
        other.close()
    for k, c in more:
        q.insert(k, c)
    keys = [k for k, _ in kc + more]
    cnt, trav = ctx.lookup(keys, mode=0)
    assert not any(trav) and cnt == [q.count(k) for k in keys]
    assert ctx.blocks() == q.blocks()
    ctx.close()
    q.free()


def contiger_reads():
    import contiger_cases as CC
    return CC.reads(G=1500, nreads=300, L=100, err=0.004, plasmid=0, seed=41)


def run_denoise_after_contiger(mk_ctx, UnitigSet):
    """(k) the unitig engine marks what it looks up; the round behind it is the unmarked oracle's"""
    fq = contiger_reads()
    offs, lens = chunks_by_records(fq, 40)
    q, _, _ = oracle_t1(fq, offs, lens, DN["k"], DN["qb"])
    assert not q.full()
    ctx = _dn_ctx(mk_ctx)
    ctx.count_chunks(fq, offs, lens)
    u = UnitigSet(ctx)
    assert u.add_reads(fq, offs, lens, DN["k"], 2, 2, 1000000, 1 << 14) >= 3
    u.close()
    assert ctx.blocks() != q.blocks()                              # marks were set
    got, want = ctx.denoise(), q.denoise_round(DN["ml"])
    print("denoise after add_reads: removed", got, "expected", want)
    assert got == want and want >= 100
    _same(ctx, q)
    ctx.close()
    q.free()


# ---------------------------------------------------------------- 3. walks on low-complexity sequence

STOP_BRANCH, STOP_DEAD_END, STOP_CIRCLE, STOP_BUFFER = 1, 2, 3, 4
WALK_QB = 12
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def low_complexity_reads(k, seed=5):
    """(FASTQ text, the reads). Five shapes, each once between random 60-base flanks and once free-standing (reads made of
    the shape alone; other letters than the flanked form, so that the two do not share k-mers), every read three times
    and without errors: all k-mers are solid at abundance_min = 2.
      homopolymer of k + 15 bases; (AC) x k; (AT) x k -- at even k the k-mer is its own reverse complement, at odd k its
      successor is; (ACG) x k; a hairpin S + rc(S), |S| = 2k."""
    rnd = random.Random(seed * 1000 + k)

    def rand(n):
        return bytes(rnd.choice(b"ACGT") for _ in range(n))
    flanked = [b"A" * (k + 15), b"AC" * k, b"AT" * k, b"ACG" * k]
    free = [b"C" * (k + 15), b"AG" * k, b"CG" * k, b"ATC" * k]
    s1, s2 = rand(2 * k), rand(2 * k)
    seqs = [rand(60) + s + rand(60) for s in flanked + [s1 + rc(s1)]] + free + [s2 + rc(s2)]
    reads = [s for s in seqs for _ in range(3)]
    return _fastq(reads), reads


def _fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads))


class WalkTable:
    """the filter of a read set on the oracle, with the k-mer -> count function every restatement here uses:
    ntHash from scratch, min(fh, rh) & mask into the oracle's count"""

    def __init__(self, fq, k, qb=WALK_QB):
        self.fq, self.k, self.qb = fq, k, qb
        self.offs, self.lens = chunks_by_records(fq, 8)
        self.q, _, _ = oracle_t1(fq, self.offs, self.lens, k, qb)
        assert not self.q.full()
        self.O = cqflibs.oracle()
        self.mask = (1 << (qb + 8)) - 1
        self._key, self._step = {}, {}

    def key(self, km):
        v = self._key.get(km)
        if v is None:
            fh, rh = self.O.nthash(km, self.k)
            v = self._key[km] = min(fh, rh) & self.mask
        return v

    def count(self, km):
        return self.q.count(self.key(km))

    def fresh(self):
        """an oracle of the same reads whose marks nobody has touched"""
        return oracle_t1(self.fq, self.offs, self.lens, self.k, self.qb)[0]

    def ctx(self, mk_ctx):
        ctx = mk_ctx(qb=self.qb, k=self.k, max_batch_bytes=2 * len(self.fq) + 4096, max_batch_keys=1 << 15)
        ctx.count_chunks(self.fq, self.offs, self.lens)
        assert ctx.blocks() == self.q.blocks()
        return ctx

    # -- shk_extend_forward as include/shk.h states it
    def step(self, win, amin):
        """one step at the window: (stop or 0, base index, its count, branch mask, neighbour counts[8], keys looked up)"""
        v = self._step.get((win, amin))
        if v is None:
            nc, mask, keys = [0] * 8, 0, []
            for j, x in enumerate((b"A", b"C", b"G", b"T")):
                for slot, km in ((j, win[1:] + x), (4 + j, x + win[1:])):
                    if slot >= 4 and x == win[:1]:
                        continue                               # the sibling with my own first base is me
                    keys.append(self.key(km))
                    c = self.count(km)
                    if c >= amin:
                        mask |= 1 << slot
                        nc[slot] = min(c, 0xFFFFFFFF)
            succ = [j for j in range(4) if mask >> j & 1]
            if mask >> 4 or len(succ) > 1:
                v = (STOP_BRANCH, 0, 0, mask, nc, keys)
            elif not succ:
                v = (STOP_DEAD_END, 0, 0, 0, [0] * 8, keys)
            else:
                v = (0, succ[0], nc[succ[0]], 0, [0] * 8, keys)
            self._step[(win, amin)] = v
        return v

    def extend_forward(self, cur, first, amin, max_ext, looked=None):
        """(bases, counts, stop, branch mask, neighbour counts[8])"""
        win, bases, counts = cur, b"", []
        while True:
            stop, x, c, mask, nc, keys = self.step(win, amin)
            if looked is not None:
                looked.update(keys)
            if stop:
                return bases, counts, stop, mask, nc
            nxt = win[1:] + b"ACGT"[x:x + 1]
            if nxt == first:
                return bases, counts, STOP_CIRCLE, 0, [0] * 8
            if len(bases) >= max_ext:
                return bases, counts, STOP_BUFFER, 0, [0] * 8
            bases += b"ACGT"[x:x + 1]
            counts.append(c)
            win = nxt

    def free(self):
        self.q.free()


def _extend_forward(ctx, ends, k, amin, mark, max_ext):
    n = len(ends)
    cur = b"".join(ends)
    ext, cnt = C.create_string_buffer(n * max_ext), (C.c_uint32 * (n * max_ext))()
    en, st, br, nc = (C.c_uint32 * n)(), (C.c_uint8 * n)(), (C.c_uint8 * n)(), (C.c_uint32 * (8 * n))()
    ctx._chk(ctx.L.shk_extend_forward(ctx.h, cur, cur, n, k, amin, mark, max_ext, ext, cnt, en, st, br, nc))
    raw = ext.raw
    return [(raw[i * max_ext:i * max_ext + en[i]], list(cnt[i * max_ext:i * max_ext + en[i]]), st[i], br[i], list(nc[8 * i:8 * i + 8]))
            for i in range(n)]


def _kmers(reads, k):
    return list(dict.fromkeys(s[i:i + k] for s in reads for i in range(len(s) - k + 1)))


def run_extend_forward(mk_ctx, k):
    """shk_extend_forward on every distinct k-mer of the reads and its reverse complement (first = cur) against the
    definition: bases, counts, number, stop reason, branch mask, the eight neighbour counts; with max_ext = 5; and with
    marking, after which the marked slots are those of every key the definition looked up"""
    fq, reads = low_complexity_reads(k)
    T = WalkTable(fq, k)
    kms = _kmers(reads, k)
    ends = list(dict.fromkeys(kms + [rc(x) for x in kms]))
    ctx = T.ctx(mk_ctx)
    for max_ext, mark in ((512, 0), (5, 0), (512, 1)):
        looked = set()
        want = [T.extend_forward(e, e, 2, max_ext, looked) for e in ends]
        stops = {(w[2], len(w[0])) for w in want}
        if max_ext == 5:
            assert (STOP_BUFFER, 5) in stops
        else:
            # the inputs reach: a pure circle that appends nothing (free-standing homopolymer), one that appends one base
            # (free-standing two-letter repeat), a branch and a dead end
            # (k <= 64. Beyond, ntHash rotates by (k - 1 - i) mod 64, so equal bases 64 apart cancel and the k-mers of a
            # periodic sequence share keys with one another: at k = 66 the definition itself finds "solid" neighbours next
            # to the free-standing repeats and stops there on a branch. The comparison below drops nothing at any k.)
            kinds = {s for s, _ in stops}
            assert kinds >= {STOP_BRANCH, STOP_DEAD_END} and STOP_BUFFER not in kinds
            if k <= 64:
                assert T.extend_forward(b"C" * k, b"C" * k, 2, max_ext)[2:4] == (STOP_CIRCLE, 0) and (STOP_CIRCLE, 0) in stops
                ag = (b"AG" * k)[:k]
                assert T.extend_forward(ag, ag, 2, max_ext)[:3] == ((b"GA" * k)[k - 1:k], [T.count((b"GA" * k)[:k])], STOP_CIRCLE)
                assert (STOP_CIRCLE, 1) in stops
        got = _extend_forward(ctx, ends, k, 2, mark, max_ext)
        bad = [(e, g, w) for e, g, w in zip(ends, got, want) if g != w]
        assert not bad, (len(bad), bad[:3])
        if mark:
            qm = T.fresh()
            for key in looked:
                qm.count_set_traveled(key)
            assert ctx.blocks() == qm.blocks() != T.q.blocks()
            qm.free()
        else:
            assert ctx.blocks() == T.q.blocks()
    ctx.close()
    T.free()


def run_unitigs_from_seeds(mk_ctx, k):
    """one maximal unitig per distinct k-mer of the reads against the oracle's two get_unitig_forward calls: sequence,
    median abundance, both stops"""
    fq, reads = low_complexity_reads(k)
    T = WalkTable(fq, k)
    seeds = _kmers(reads, k)
    counts = [T.count(s) for s in seeds]
    assert min(counts) >= 2
    ctx = T.ctx(mk_ctx)
    max_len = 1024
    got = ctx.unitigs_from_seeds(seeds, counts, k, 2, max_len)
    want = [T.q.unitig_from_seed(s, c, k, 2, max_len) for s, c in zip(seeds, counts)]
    bad = [(s, g, w) for s, g, w in zip(seeds, got, want) if g != w]
    assert not bad, (len(bad), bad[:2])
    assert {st for _, _, sts in want for st in sts} >= {STOP_BRANCH, STOP_DEAD_END, STOP_CIRCLE}
    ctx.close()
    T.free()


def _select_seeds(ctx, text, k, cmin, cmax, use_traveled):
    L = ctx.L
    L.shk_select_seeds.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.POINTER(C.c_uint32),
                                   C.c_uint32, C.POINTER(C.c_uint32)]
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(text))
    buf = C.create_string_buffer(text, len(text))
    cap = text.count(b"\n") // 4 + 1
    seeds, counts, n = C.create_string_buffer(cap * k), (C.c_uint32 * cap)(), C.c_uint32()
    ctx._chk(L.shk_select_seeds(ctx.h, C.cast(buf, C.c_void_p), 0, len(text), off, ln, 1, k, cmin, cmax, use_traveled, seeds, counts, cap,
                                C.byref(n)))
    return [(seeds.raw[i * k:(i + 1) * k], counts[i]) for i in range(n.value)]


def run_select_seeds(mk_ctx, k):
    """shk_select_seeds against its rule in include/shk.h: the k-mer at len/2 - k/2, upper-cased, without N, count within
    [count_min, count_max]; with use_traveled every k-mer looked up is marked and one that an earlier read of the call
    marked gives no seed (of several reads with one seed exactly one survives; which one is the schedule's)"""
    fq, reads = low_complexity_reads(k)
    T = WalkTable(fq, k)
    body = reads[0]
    mid = len(body) // 2 - k // 2
    with_n = body[:mid + 3] + b"N" + body[mid + 4:]
    lower = body[:mid + 2] + body[mid + 2:mid + 9].lower() + body[mid + 9:]
    sel = reads + [body[:k], body[7:7 + k + 1], body[:k - 1], with_n, lower, reads[3][5:5 + k], b"acgt" * k]
    text = _fastq(sel)
    valid = []                                   # per read with a seed k-mer: (k-mer, key, count)
    for s in sel:
        m = len(s) // 2 - k // 2
        if len(s) < k or m < 0 or m > len(s) - k:
            continue
        km = s[m:m + k].upper()
        if set(km) <= set(b"ACGT"):
            valid.append((km, T.key(km), T.count(km)))
    cmin, cmax = 4, max(c for _, _, c in valid) - 1            # (both ends of the range leave some read out)
    want = [(km, c) for km, _, c in valid if cmin <= c <= cmax]
    assert len(want) >= 12 and any(c < cmin for _, _, c in valid) and any(c > cmax for _, _, c in valid)
    assert len(valid) == len(sel) - 2             # (the read of k - 1 bases and the one with N give nothing)
    ctx = T.ctx(mk_ctx)
    assert _select_seeds(ctx, text, k, cmin, cmax, 0) == want          # read order
    assert ctx.blocks() == T.q.blocks()
    got = _select_seeds(ctx, text, k, cmin, cmax, 1)
    by_key = {}
    for km, key, c in valid:
        if cmin <= c <= cmax:
            by_key.setdefault(key, set()).add((km, c))
    assert sorted(T.key(km) for km, _ in got) == sorted(by_key)         # one survivor per key
    assert all((km, c) in by_key[T.key(km)] for km, c in got)
    assert max(len(v) for v in by_key.values()) >= 1 and len(got) < len(want)
    qm = T.fresh()
    for _, key, _ in valid:
        qm.count_set_traveled(key)
    assert ctx.blocks() == qm.blocks()
    assert _select_seeds(ctx, text, k, cmin, cmax, 1) == []            # everything is marked now
    assert ctx.blocks() == qm.blocks()
    qm.free()
    ctx.close()
    T.free()


def run_pipeline(mk_ctx, UnitigSet, tmp_path, k):
    """the whole of Contiger read by read on these reads == the sequential restatement"""
    import contiger_cases as CC
    fq, _ = low_complexity_reads(k)
    r = CC.run_case(mk_ctx, UnitigSet, tmp_path, k=k, qb=WALK_QB, fq=fq, chunk_reads=8, per_read=True, max_len=1 << 12)
    assert r["unitigs"] >= 8 and r["seeds"] >= 5, r
    return r
