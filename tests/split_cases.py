"""The split record between k_roll_scatter and the middle partition level (csrc/partition_kernels.hip: the split record;
csrc/roll_kernels.hip: k_roll_scatter's SPLIT form; csrc/shk_api.hip: shk_ctx::split_kb, roll_keys, partition_stage). Shared
by the emulator tests and the GPU tests of tests/test_split_records.py. The yardstick is the oracle throughout: table
blocks, header, nelts and ndistinct.

Which path ran: the profile keys are the same for both forms, so the observable is Context.split_batches()
(shk_split_batches, include/shk.h): the number of batches since the context was created whose first-level output took the
split form. Existing callers ignore it. A batch that runs its front end twice (the redo with counted bases behind an
overflowing upper slot) counts once per run.

The rule: a batch is split when its context has three levels whose middle one may be narrow, owns the whole filter
(num_shards = 1), its words come from text (shk_count_chunks, shk_prepare_chunks, shk_count_fasta), the call's chunks are at
most 1 << cb, and kb + cb <= 40 with kb = rbits + 16 - bits0. SHK_RP_SPLIT=0, read when a context is created, keeps every
batch on 8-byte words (SHK_RP_WORDS8=1 implies it): every group below runs in a fresh child process, once as built and once
with the variable set (python split_cases.py BACKEND GROUP), and asserts there; the parent test only looks at the exit
status (and, for `rule`, compares the shard's two error codes).

| geometry | qb | max_level_bits | levels    | kb | cb | kb + cb | split                          | emulator |
|----------|----|----------------|-----------|----|----|---------|--------------------------------|----------|
| two      | 14 | 3              | (3,3)     |    |    |         | never                          | yes      |
| three    | 16 | 3              | (3,3,2)   | 21 | 14 | 35      | every chunk count              | yes      |
| four     | 18 | 3              | (3,3,2,2) |    |    |         | never                          | GPU only |
| edge     | 23 | 7              | (5,5,5)   | 26 | 11 | 37      | 2048 chunks yes, 2049 no       | GPU only |
| shard    | 16 | 3, shard 1 of 2| (3,2,2)   |    |    |         | never                          | yes      |
| fasta    | 14 | 2              | (2,2,2)   | 20 | 14 | 34      | every piece                    | yes      |

The high plane holds rec40 >> 32 = chunk >> (32 - kb): `three` needs a chunk tag of 2048 or more to set a bit there (the
4096 tiny chunks of tests/text_cases.py), `edge` one of 64 or more (its 2048 chunks); a call of one chunk leaves the plane
zero. Texts: ~2,000 reads of 100 bases, k = 31, max_batch_keys = 2^20, as tests/narrow_cases.py has them; the slot groups
take the batches of tests/roll_slots_cases.py with its max_batch_keys = 2^21, so that the slot conditions hold (the levels
(3, 3, 2) at qb 16 come from max_level_bits = 3 there and here)."""
import json
import os
import random
import sys

import narrow_cases as NC
import roll_slots_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = NC.K
MAX_KEYS = NC.MAX_KEYS
GEOM = dict(NC.GEOM)
EMU_GROUPS = ["planes", "rule", "windows", "slots", "fasta"]
GPU_GROUPS = ["planes", "edge", "edge-point", "rule", "rule-four", "windows", "slots", "slots0", "fasta"]


def split_on():
    return os.environ.get("SHK_RP_SPLIT", "") != "0" and not NC.words8()


def kb_of(qb, levels):
    return (qb - 8) + 16 - levels[0]


def expect_split(geom, nchunks):
    """the rule, for a batch of text on a context that owns the whole filter"""
    qb, _, levels = GEOM[geom]
    return split_on() and len(levels) == 3 and nchunks <= (1 << NC.cb_of(levels)) and kb_of(qb, levels) + NC.cb_of(levels) <= 40


def run_text(mk, geom, fq, offs, lens, k=K, flows=("count", "prepared"), want=None):
    """the text through shk_count_chunks and through shk_prepare_chunks + shk_count_prepared, a context each: the oracle's
    table, and the split form exactly where the rule says"""
    qb, mlb, levels = GEOM[geom]
    want = want or NC._oracle(fq, offs, lens, k, qb)
    for flow in flows:
        ctx = mk(qb=qb, k=k, max_level_bits=mlb, max_batch_bytes=len(fq) + 1024, max_batch_keys=MAX_KEYS,
                 max_batch_reads=fq.count(b"\n") + 4096 + 16)
        assert ctx.split_batches() == 0
        if flow == "count":
            st = ctx.count_chunks(fq, offs, lens)
        else:
            ctx.prepare_chunks(fq, offs, lens)
            st = ctx.count_prepared()
        assert st["kmers"] == want[2], (geom, flow)
        assert NC._state(ctx) == want, (geom, flow)
        assert ctx.split_batches() == (1 if expect_split(geom, len(offs)) else 0), (geom, flow, len(offs), ctx.split_batches())
        ctx.close()
    return want


# ------------------------------------------------------------------------------------------------------------ groups
def group_planes(mk, emu):
    """(3, 3, 2), kb = 21: 4096 tiny chunks put chunk bits 11 and up into the byte plane (tags 2048 .. 4095 set it); 20
    chunks leave it zero but for nothing; ONE chunk leaves both the tag bits of the low word and the byte plane zero"""
    import text_cases as TC
    assert kb_of(16, GEOM["three"][2]) == 21 and NC.cb_of(GEOM["three"][2]) == 14
    big = TC._tiny_records(random.Random(52), TC.MAX_CHUNKS)
    offs, lens = TC._tile(big, 1)
    assert len(offs) == 4096 and (len(offs) - 1) >> (32 - 21) > 0
    run_text(mk, "three", b"".join(big), offs, lens, k=5, flows=("count",) if emu else ("count", "prepared"))
    fq, offs, lens = NC._genome_text()
    assert len(offs) == 20
    run_text(mk, "three", fq, offs, lens)
    run_text(mk, "three", fq, [0], [len(fq)])


def group_edge(mk, emu):
    """(5, 5, 5), kb = 26, cb = 11, kb + cb = 37: a call of exactly 2048 chunks is split (tags of 64 and more reach the byte
    plane, one record per chunk), one of 2049 is not narrow, hence not split"""
    rnd = random.Random(61)
    recs = NC._reads(rnd, [100] * 2049)
    assert kb_of(23, GEOM["edge"][2]) == 26 and NC.cb_of(GEOM["edge"][2]) == 11
    for n in (2048, 2049):
        offs, lens = NC._tile(recs[:n], 1)
        assert expect_split("edge", n) == (n == 2048 and split_on())
        run_text(mk, "edge", b"".join(recs[:n]), offs, lens)


def group_edge_point(mk, emu):
    """narrow_cases' edge-point shape: (5, 5, 5), 2048 chunks of one read each and ONE deNoise round behind chunk 1535. The
    chunk tags decide the result, and their bits 6 and up travel in the byte plane: a record that lost them would put its
    read in front of the point."""
    import cqflibs
    from fastq_util import chunks_by_records, oracle_header, oracle_t1
    import synth
    qb, mlb, levels = GEOM["edge"]
    point = 1535
    fq = synth.make_fastq(synth.make_genome(60000, 9), 2048, 100, 0.01, seed=34, n_frac=0.03)
    offs, lens = chunks_by_records(fq, 1)
    assert len(offs) == 2048 == 1 << NC.cb_of(levels) and point >> (32 - kb_of(qb, levels)) > 0
    O = cqflibs.oracle()
    q = O.new(qb)
    nd = []
    for a, n in zip(offs, lens):
        q.reads_to_kmers(fq[a:a + n], K)
        nd.append(q.ndistinct())
    q.free()
    trigger = nd[point]
    assert nd[point - 1] < trigger
    q, rounds, removed = oracle_t1(fq, offs, lens, K, qb, trigger, 1, False, 1 << 20)
    assert rounds == 1 and removed > 0 and not q.full()
    want = (q.blocks(), oracle_header(q), q.nelts(), q.ndistinct())
    q.free()
    for flow in ("count", "prepared"):
        ctx = mk(qb=qb, k=K, max_level_bits=mlb, trigger=trigger, num_denoise=1, min_denoise_len=1 << 20,
                 max_batch_bytes=len(fq) + 1024, max_batch_keys=MAX_KEYS, max_batch_reads=2048 + 4096 + 16)
        if flow == "count":
            st = ctx.count_chunks(fq, offs, lens)
        else:
            ctx.prepare_chunks(fq, offs, lens)
            st = ctx.count_prepared()
        assert (st["denoise_rounds"], st["removed"]) == (rounds, removed), (flow, st, rounds, removed)
        assert NC._state(ctx) == want, flow
        assert ctx.split_batches() == (1 if split_on() else 0), flow
        ctx.close()


def group_rule(mk, emu):
    """the rule's edges that never split: two levels; a counted insert on (3, 3, 2) (its words do not come from text); shard
    1 of 2 at qb 16, which refuses the text's out-of-range keys with the error it gave before (printed as {"code": ..} for
    the parent to compare between the two runs) and leaves the table as it was"""
    import f4_scenarios as F
    fq, offs, lens = NC._genome_text(genome=2000, err=0.0)
    run_text(mk, "two", fq, offs, lens)
    qb, mlb, levels = GEOM["three"]
    held = []

    def mk_counted(qb_):
        held.append(mk(qb=qb_, k=21, max_batch_keys=1 << 14, max_level_bits=mlb))
        close = held[-1].close

        def close_and_look():
            if getattr(held[-1], "h", None):
                assert held[-1].split_batches() == 0
            close()
        held[-1].close = close_and_look
        return held[-1]
    rng = random.Random(12)
    F.check_counted_and_dump(mk_counted, qb, F.pairs(rng, qb, 150, 4000))
    held[0].close()
    assert len(held) == 1
    fq, offs, lens = NC._genome_text()
    ctx = mk(qb=16, k=K, max_level_bits=3, max_batch_bytes=len(fq) + 1024, max_batch_keys=MAX_KEYS, shard_index=1, num_shards=2)
    before = NC._state(ctx)
    code = 0
    try:
        ctx.count_chunks(fq, offs, lens)
    except Exception as e:
        code = getattr(e, "code", None)
    assert code not in (0, None), code
    assert NC._state(ctx) == before and ctx.split_batches() == 0
    ctx.close()
    print(json.dumps({"code": code}))


def group_rule_four(mk, emu):
    """(3, 3, 2, 2): four levels, not split (the level behind the roll kernels is a wide one)"""
    fq, offs, lens = NC._genome_text(genome=12000, err=0.01)
    run_text(mk, "four", fq, offs, lens)


def group_windows(mk, emu):
    """k_roll_scatter's windows are one round (16 bases) of every thread, the middle level's 16384 positions of a bucket
    (4096 on the emulator build). One read alone: its rounds are windows of 2 to 16 keys, the last one of 4, and most digits
    get no key in any of them. Reads of 100 bases next to short ones end inside windows. 250 reads of poly-A give one digit
    whole windows of 16 equal keys per thread (17,500 copies of one k-mer: more than a 16384-key window of either level),
    which the wave-per-run drain must neither lose nor duplicate; the oracle's count of that key says so. Then the window
    edges of narrow_cases: 16384 - 1, 16384 and 16384 + 1 keys."""
    rnd = random.Random(71)
    one = NC._reads(rnd, [100])
    run_text(mk, "three", one[0], [0], [len(one[0])], flows=("count",))
    recs = NC._reads(rnd, [100, 40, 31, 100, 30, 47] * 20) + [NC._rec(1000 + i, b"A" * 100) for i in range(250)]
    rnd.shuffle(recs)
    offs, lens = NC._tile(recs, 37)
    run_text(mk, "three", b"".join(recs), offs, lens, flows=("count",) if emu else ("count", "prepared"))
    for d in (-1, 0, 1):
        nkeys = 16384 + d
        full, rest = divmod(nkeys, 100 - K + 1)
        recs = NC._reads(rnd, [100] * (full - 1) + [100 + rest])
        fq = b"".join(recs)
        offs, lens = NC._tile(recs, 40)
        want = NC._oracle(fq, offs, lens, K, GEOM["three"][0])
        assert want[2] == nkeys, (want[2], nkeys)
        run_text(mk, "three", fq, offs, lens, flows=("count",), want=want)


def _slot_batches(mk, k, plan):
    """roll_slots_cases' batches through one context of its shape ((3, 3, 2) at qb 16, max_batch_keys = 2^21: the slot
    conditions hold), the oracle alongside; plan: (text, records per chunk, check(profile), front-end runs)"""
    import cqflibs
    from fastq_util import chunks_by_records
    ctx = RC._mk_ctx(mk, max(len(p[0]) for p in plan), k=k)
    q = cqflibs.oracle().new(RC.QB)
    for i, (fq, per, check, runs) in enumerate(plan):
        offs, lens = chunks_by_records(fq, per)
        ctx.profile_reset()
        n0 = ctx.split_batches()
        ctx.count_chunks(fq, offs, lens)
        q.reads_to_kmers(fq, k)
        assert RC._state(ctx) == RC._ostate(q), i
        check(ctx.profile_get())
        assert ctx.split_batches() - n0 == (runs if split_on() else 0), (i, ctx.split_batches() - n0, runs)
    ctx.close()
    q.free()


def group_slots(mk, emu):
    """the slotted flow (no counting pass at any level) writes and reads split records; a level-1 slot that overflows sends
    the batch through the front end again with counted bases, split again (the two levels' digits fit k_roll_hist's bins, so
    no k_rp_hist meets the planes); two overflows in a row switch the upper slots off and the next batch takes the histogram
    pass, still split. All against the oracle."""
    assert RC.slots_on()
    uni, uni2 = RC._uniform(), RC._uniform(seed=34, prefix="u")
    over = uni2 + RC._poly(60)
    _slot_batches(mk, K, [(uni, 100, RC._clean, 1), (over, 103, RC._redone, 2), (over, 103, RC._redone, 2), (uni, 100, RC._hist_path, 1)])


def group_slots0(mk, emu):
    """the overflow of a k_roll_scatter slot (roll_slots_cases' overflow0: one key 272,000 times against a slot of ~75,000):
    the split run's records past the slot are never read, the redo with counted bases is split too"""
    uni = RC._uniform()

    def redone(p):
        assert p[RC.ROLL_HIST][0] == 1 and p[RC.RP_HIST][0] == 1 and p[RC.NARROW][0] == 3 and RC.WIDE not in p, p
    _slot_batches(mk, 21, [(uni, 100, RC._clean, 1), (uni + RC._poly(3400), 270, redone, 2), (uni, 100, RC._clean, 1)])


def group_fasta(mk, emu):
    """shk_count_fasta on a three-level context ((2, 2, 2) at qb 14, the geometry case of tests/fasta_cases.py): every piece
    that holds a k-mer is one batch of one chunk, split"""
    import fasta_cases as FC
    k, seg, qb, mlb = 31, 16, 14, 2
    ctx, exp = FC.ctx_for(mk, qb, k, seg, max_level_bits=mlb), FC.Expect(qb)
    text, _ = FC.stream_text(k)
    FC.count_stream(ctx, exp, [FC.run_length_text(k, seg, 31)], k, "split, one call")
    n1 = ctx.split_batches()
    assert (n1 >= 1) == split_on(), n1
    FC.count_stream(ctx, exp, [text[:100], text[100:101], text[101:]], k, "split, pieces")
    assert (ctx.split_batches() > n1) == split_on()
    ctx.close()
    exp.free()


GROUPS = {"planes": group_planes, "edge": group_edge, "edge-point": group_edge_point, "rule": group_rule, "rule-four": group_rule_four,
          "windows": group_windows, "slots": group_slots, "slots0": group_slots0, "fasta": group_fasta}


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
    print("SPLIT_GROUP_OK")


if __name__ == "__main__":
    main(sys.argv)
