"""One case per branch of the front end's partition plan (csrc/shk_api.hip: create_init fills it, partition_stage reads it).
Shared by the emulator tests and the GPU tests of tests/test_partition_plan.py. The yardstick is the oracle throughout.

Geometry as create_init derives it: rbits = qb - 8 region bits, nlevels = ceil(rbits / max_level_bits) (0 = the default, 10),
the bits split evenly with the larger shares first. Every case: ~2,000 reads of 100 bases, k = 31, chunks of 100 records,
no deNoise rounds, max_batch_keys = 2^20 (so that the slot capacity rule admits region slots wherever the plan allows them).

| case | qb | max_level_bits | levels    | what it reaches                                                                   | emulator |
|------|----|----------------|-----------|-----------------------------------------------------------------------------------|----------|
| a    | 8  | 0              | 1 region  | the single-pass conversion to 32-bit records                                      | yes      |
| b    | 9  | 0              | (1)       | one level, ungrouped, hash front end with d_hist[0] counted                       | yes      |
| c    | 12 | 0              | (4)       | one level, grouped                                                                | yes      |
| d    | 14 | 3              | (3,3)     | roll front end; level 1 counted by the roll histogram, so no slots                | yes      |
| e    | 16 | 3              | (3,3,2)   | roll; a middle level; last level with region slots                                | yes      |
| f    | 18 | 3              | (3,3,2,2) | four levels                                                                       | GPU only |
| g    | 23 | 8              | (8,7)     | roll with cb = 15 > 14: one-level roll histogram, level 1 counts for itself       | GPU only |
| h    | 24 | 0              | (8,8)     | external words only: ungrouped first level, no paired histogram                   | GPU only |

(f, g and h hold 2^10, 2^15 and 2^16 regions: the emulator runs a workgroup per region one after another, which takes
ten seconds per context for f and minutes for the other two. The emulator runs one flow of a case per test.)

The genome, the error rate and the share of reads with an 'N' run are sized to a case's table, not to the plan: every k-mer
next to an 'N' run hashes to a key of its own, and the table of case a holds 256 slots (its genome repeats every 30 bases).
`slots`: whether the last level may use region slots (k_rp_slot_cursors in profile_get(), the suite's only observable for
"which path"): it must where the plan allows them and the capacity rule admits them, and cannot anywhere else.

mk_ctx(**kw) -> context with ctx.split(ptr, n, m) -> (pa, m, pb, n - m): copies of words [0, m) and [m, n) of the buffer at
ptr that the library can read (kept alive by the context), and ctx.device = where torch puts the ranks' statistics."""
import contextlib

import numpy as np

import synth
from fastq_util import chunks_by_records, oracle_header, oracle_t1

K = 31
NREADS, READ_LEN, PER_CHUNK = 2000, 100, 100
MAX_KEYS = 1 << 20

#        qb  max_level_bits  levels        genome  period  err    n_frac  slots  emulator
CASES = {
    "a": (8,  0,             (0,),         120,    30,     0.0,   0.003,  False, True),
    "b": (9,  0,             (1,),         110,    110,    0.0,   0.01,   False, True),
    "c": (12, 0,             (4,),         400,    400,    0.0,   0.03,   False, True),
    "d": (14, 3,             (3, 3),       2000,   2000,   0.0,   0.03,   False, True),
    "e": (16, 3,             (3, 3, 2),    8000,   8000,   0.001, 0.03,   True,  True),
    "f": (18, 3,             (3, 3, 2, 2), 12000,  12000,  0.01,  0.03,   True,  False),
    "g": (23, 8,             (8, 7),       12000,  12000,  0.01,  0.03,   True,  False),
    "h": (24, 0,             (8, 8),       12000,  12000,  0.01,  0.03,   False, False),
}
EMU_CASES = [n for n in sorted(CASES) if CASES[n][8]]


def levels(qb, max_level_bits):
    """create_init's split of the region bits"""
    rbits, mlb = qb - 8, max_level_bits or 10
    n = max(1, -(-rbits // mlb))
    out, left = [], rbits
    for l in range(n):
        bits = -(-left // (n - l))
        left -= bits
        out.append(bits)
    return tuple(out)


_REF = {}


def reference(name):
    """(fq, offs, lens, (blocks, header, nelts, ndistinct) of the oracle): computed once per case, never changed"""
    if name not in _REF:
        qb, _, _, G, period, err, n_frac, _, _ = CASES[name]
        genome = np.tile(synth.make_genome(period, 5), -(-G // period))[:G]
        fq = synth.make_fastq(genome, NREADS, READ_LEN, err, seed=33, n_frac=n_frac, short_frac=0.02)
        offs, lens = chunks_by_records(fq, PER_CHUNK)
        q, _, _ = oracle_t1(fq, offs, lens, K, qb)
        assert not q.full()
        _REF[name] = (fq, offs, lens, (q.blocks(), oracle_header(q), q.nelts(), q.ndistinct()))
        q.free()
    return _REF[name]


def _new(mk_ctx, name, fq, **kw):
    qb, mlb = CASES[name][:2]
    ctx = mk_ctx(qb=qb, k=K, max_level_bits=mlb, max_batch_bytes=len(fq) + 1024, max_batch_keys=MAX_KEYS, **kw)
    ctx.profile(True)
    return ctx


def _check(ctx, name, want, flow):
    blocks, header, nelts, ndistinct = want
    t = ctx.totals()
    assert (t.nelts, t.ndistinct) == (nelts, ndistinct), (name, flow)
    assert ctx.header() == header, (name, flow)
    assert ctx.blocks() == blocks, (name, flow)
    ran = ctx.profile_get().get("k_rp_slot_cursors", (0, 0.0))[0]
    assert (ran > 0) == CASES[name][7], (name, flow, ran)
    ctx.close()


def _thirds(n):
    t = n // 3
    return ((0, t), (t, 2 * t), (2 * t, n))


TEXT_FLOWS = ("one call", "three calls", "prepared")
WORD_FLOWS = ("words", "pair")


def run_text(mk_ctx, name, flows=TEXT_FLOWS):
    """count_chunks in one call and in three; prepare_chunks + count_prepared (a context each)"""
    assert levels(*CASES[name][:2]) == CASES[name][2]
    fq, offs, lens, want = reference(name)
    parts = [(offs[a:b], lens[a:b]) for a, b in _thirds(len(offs))]
    for flow in flows:
        ctx = _new(mk_ctx, name, fq)
        if flow == "one call":
            ctx.count_chunks(fq, offs, lens)
        elif flow == "three calls":
            for o, l in parts:
                ctx.count_chunks(fq, o, l)
        else:
            assert flow == "prepared"
            ctx.prepare_chunks(fq, *parts[0])
            for i in range(3):
                if i + 1 < 3:
                    ctx.prepare_chunks(fq, *parts[i + 1])
                ctx.count_prepared()
        _check(ctx, name, want, flow)


@contextlib.contextmanager
def one_rank_group(backend, tmp_path):
    """a process group of one rank (the collectives of shk/dist.py need one), unless the caller's process has one already"""
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        dist.init_process_group(backend, init_method="file://%s" % (tmp_path / "pg"), rank=0, world_size=1)
    try:
        yield
    finally:
        if own:
            dist.destroy_process_group()


def run_words(mk_ctx, name, backend, tmp_path, flows=WORD_FLOWS):
    """the external-words path with one rank: hash_chunks -> stage_words -> sharded_count in three batches ("words"), and
    the same with the words staged from two buffers cut at n // 3 + 17 ("pair", shk_stage_words_pair)"""
    from shk import dist as shkdist
    fq, offs, lens, want = reference(name)
    with one_rank_group(backend, tmp_path):
        for flow in flows:
            assert flow in WORD_FLOWS
            ctx = _new(mk_ctx, name, fq, shard_index=0, num_shards=1)
            st = shkdist.ShardState(1 << 62, 0, ctx.device)
            for a, b in _thirds(len(offs)):
                dp, nw = ctx.hash_chunks(fq, offs[a:b], lens[a:b])
                if flow == "pair":
                    ctx.stage_words_pair(*ctx.split(dp, nw, nw // 3 + 17))
                else:
                    ctx.stage_words(dp, nw)
                shkdist.sharded_count(ctx, st, b - a)
            assert (st.nelts, st.ndistinct) == want[2:]
            _check(ctx, name, want, flow)
