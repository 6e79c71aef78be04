"""The early loads of the record-sourced rebuild kernels (csrc/cqf_kernels.hip, k_region_merge with OLDREC and PF: a dense
pass asks for a region's old record and for its first round of words before it knows anything about the region). Shared by
the emulator tests and the GPU tests of tests/test_merge_prefetch.py: every group runs in a fresh child process (python
prefetch_cases.py BACKEND GROUP), asserts there and prints PREFETCH_GROUP_OK.

Key words go in through shk_count_words at qb 11 / hb 19: 8 regions of 256 quotients, so a pass is dense -- the host's gate --
from 64 words on. A context's first batch rebuilds from the (empty) table; it leaves records, and the batches behind it take
the record-sourced kernels. Every case runs twice, with the gate as the library sets it and with SHK_MERGE_PREFETCH=0: table
bytes, header and totals must be the same, and equal to cqf_canon.build_blocks (the oracle where a deNoise point is
involved). shk_prefetch_passes says which of the two ran."""
import ctypes as C
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QB, HB = 11, 19
NREG = 8
PACK_MAX = 512                 # SHK_SPILL_PACK_MAX: packed run bytes a region's record holds
GROUPS = ["slots", "rounds", "records", "over", "empty", "unslotted", "sample", "point", "gate"]


def key(tag, region):
    """tag = local quotient << 8 | remainder"""
    return (region << 16) | tag


def _mk(backend):
    """-> (make context, make a pointer the library can read from a list of words)"""
    for p in (HERE, ROOT, os.path.join(ROOT, "sh-assembly_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    held = []
    if backend == "emu":
        import shk
        lib = os.path.join(HERE, "emu", "libshk_emu.so")

        def mk(**kw):
            return shk.Context(threads_per_group=64, hash_groups=2, lib_path=lib, **kw)

        def dev(ws):
            arr = (C.c_uint64 * max(len(ws), 1))(*ws)
            held.append(arr)
            return C.addressof(arr)
    else:
        import torch  # (before libshk.so: one HIP runtime per process, see tests/conftest.py)
        import shk
        mk = shk.Context

        def dev(ws):
            t = torch.tensor(ws if ws else [0], dtype=torch.int64).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            held.append(t)
            return t.data_ptr()
    return mk, dev


def singles(region, n, first=0):
    """n distinct keys of the region, once each: n packed bytes in its record (remainders >= 2, at most two keys per
    quotient from 256 keys on, so that no length byte saturates)"""
    return {key(((first + i) % 256) << 8 | (2 + (first + i) // 256), region): 1 for i in range(n)}


def repeats(region, nwords, ndistinct=40, seed=0):
    """nwords words of the region over at most ndistinct keys"""
    rnd = random.Random(1000 * region + seed)
    ks = [key(t, region) for t in rnd.sample(range(1 << 16), min(ndistinct, max(nwords, 1)))]
    out = {}
    for i in range(nwords):
        k = ks[(i * i + i) % len(ks)]
        out[k] = out.get(k, 0) + 1
    return out


def merged(*ds):
    out = {}
    for d in ds:
        for k, c in d.items():
            out[k] = out.get(k, 0) + c
    return out


def _words(counts, seed, chunk=0):
    ws = [k | (chunk << HB) for k, c in counts.items() for _ in range(c)]
    random.Random(seed).shuffle(ws)
    return ws


def both_gates(fn):
    """fn() with the gate as the library sets it, then with SHK_MERGE_PREFETCH=0 (read when a context is created); fn
    returns (what must be equal, prefetch passes). -> the passes of the first run"""
    os.environ.pop("SHK_MERGE_PREFETCH", None)
    a, pa = fn()
    os.environ["SHK_MERGE_PREFETCH"] = "0"
    try:
        b, pb = fn()
    finally:
        os.environ.pop("SHK_MERGE_PREFETCH", None)
    assert (sum(pb) if isinstance(pb, list) else pb) == 0, pb
    assert a == b, "the early loads change the result"
    return pa


def run_batches(mk, dev, batches, seed=1, slotted=None, **kw):
    """the batches (key -> occurrences) one after the other into one context, the canonical table after each.
    slotted: None, or per batch whether its last partition level must have run with region slots
    -> ([(blocks, header, nelts, ndistinct) per batch], prefetch passes per batch)"""
    from cqf_canon import build_blocks
    kw.setdefault("max_batch_keys", 1 << 13)
    ctx = mk(qb=QB, k=21, max_batch_bytes=64, **kw)
    ctx.profile(True)
    have = {}
    out, passes = [], []
    for bi, counts in enumerate(batches):
        ws = _words(counts, seed + bi)
        before = ctx.prefetch_passes()
        ctx.profile_reset()
        st = ctx.count_words(dev(ws), len(ws), 1)
        assert st["kmers"] == len(ws), (bi, st)
        prof = ctx.profile_get()
        if slotted is not None:
            assert ("k_rp_slot_cursors" in prof) == slotted[bi] or (slotted[bi] == "redo" and "k_rp_slot_cursors" in prof and "k_rp_hist" in prof), (bi, prof)
        passes.append(ctx.prefetch_passes() - before)
        have = merged(have, counts)
        t = ctx.totals()
        assert (t.nelts, t.ndistinct) == (sum(have.values()), len(have)), bi
        blocks = ctx.blocks()
        assert blocks == build_blocks(QB, HB, have), bi
        out.append((blocks, ctx.header(), t.nelts, t.ndistinct))
    ctx.close()
    return out, passes


def group_slots(mk, dev):
    """region slots of 256 records (three levels of one bit, max_batch_keys 1024), less than the 512 indices the two waves
    load up front: a region with few words next to regions whose slots are full of other keys, the last region of the
    buffer among them. Nothing of a neighbour is counted and nothing behind the buffer is read"""
    old = merged(*[repeats(r, 12, 6, seed=1) for r in range(NREG)])
    nw = [5, 256, 3, 90, 0, 40, 9, 256]       # (a mean above 84 words would make the library do without slots of 256)
    assert 64 <= sum(nw) <= 660
    new = merged(*[repeats(r, n, 30, seed=2) for r, n in enumerate(nw)])

    def go():
        out, passes = run_batches(mk, dev, [old, new], max_level_bits=1, max_batch_keys=1024, slotted=[True, True])
        return out, sum(passes)
    assert both_gates(go) >= 1


def group_rounds(mk, dev):
    """regions with 0, 1, 127, 128, 129, 511, 512, 513 and 1,100 words in slots of 2048: the edges of the first round (four
    words per lane of two waves, loaded up front) and of the later rounds, which keep their dependent loads"""
    old = merged(*[repeats(r, 10, 5, seed=3) for r in range(1, NREG)])      # (region 0: no old runs either)
    a = merged(*[repeats(r, n, 50, seed=4) for r, n in enumerate([0, 1, 127, 128, 129, 511, 512, 513])])
    b = merged(repeats(3, 1100, 60, seed=5), repeats(6, 70, 20, seed=5))

    def go():
        out, passes = run_batches(mk, dev, [old, a, b], max_level_bits=1, slotted=[True, True, True])
        assert passes[0] == 0
        return out, min(passes[1:])
    assert both_gates(go) >= 1


def group_records(mk, dev):
    """old records with 0, 1, 2, 3, 4, 255, 256 and 257 packed bytes (a sub-dword tail; the border between the dwords the
    first and the second wave load), then 511 and 512 (the record's capacity), each read by a dense pass that adds a second
    occurrence to some of the keys and new keys to others"""
    for sizes in ([0, 1, 2, 3, 4, 255, 256, 257], [511, 0, 5, 0, 512, 0, 4, 3]):
        old = merged(*[singles(r, n) for r, n in enumerate(sizes)])
        # a dense pass that keeps every region's runs inside its record: second occurrences only where it is full
        new = {}
        for r, n in enumerate(sizes):
            ks = list(singles(r, n))
            for k in ks[:: max(1, n // 7)] if n < 500 else []:
                new[k] = new.get(k, 0) + 1
            for k in (singles(r, 4, first=n) if n < 250 else {}):
                new[k] = 2
        new = merged(new, repeats(1, 40, 8, seed=6))
        third = merged(*[repeats(r, 9, 3, seed=7) for r in (1, 3, 5)], singles(0, 3))

        def go():
            out, passes = run_batches(mk, dev, [old, new, third])
            return out, passes[1]
        assert both_gates(go) >= 1


def group_over(mk, dev):
    """a region whose record is full (512 packed bytes) gets one more key: its runs no longer fit the record and it takes
    the over-list route (the write pass); the batches behind it read the table, which that region keeps them on"""
    old = merged(singles(2, PACK_MAX), singles(5, 30), singles(6, 100))
    new = merged(singles(2, 1, first=PACK_MAX), repeats(5, 50, 10, seed=8), repeats(0, 30, 10, seed=8))
    third = merged(repeats(2, 20, 5, seed=9), repeats(7, 60, 10, seed=9))
    fourth = merged(*[repeats(r, 10, 4, seed=10) for r in range(NREG)])

    def go():
        return run_batches(mk, dev, [old, new, third, fourth])
    passes = both_gates(go)
    assert passes[1] >= 1 and passes[2] == 0 and passes[3] == 0, passes      # (records, then the table: the over list made the pass write)


def group_empty(mk, dev):
    """a dense pass in which one region has old runs and no words, one has words and an empty old record, and one has
    neither (it leaves behind the issued loads: its summary and its new record must say "nothing"); the pass behind it
    reads all three records and puts keys into each of the regions"""
    old = merged(singles(0, 40), singles(1, 17), repeats(3, 30, 9, seed=11), repeats(4, 25, 9, seed=11), singles(6, 3), singles(7, 60))
    new = merged(repeats(0, 40, 9, seed=12), repeats(2, 50, 12, seed=12), repeats(3, 33, 9, seed=12), repeats(4, 20, 30, seed=12),
                 repeats(6, 21, 4, seed=12), repeats(7, 19, 4, seed=12))
    assert not any((k >> 16) in (1, 5) for k in new) and not any((k >> 16) in (2, 5) for k in old)
    third = merged(*[repeats(r, 12, 5, seed=13) for r in range(NREG)])
    for kw in ({}, {"max_level_bits": 1}):      # unslotted and slotted words

        def go():
            out, passes = run_batches(mk, dev, [old, new, third], **kw)
            return out, min(passes[1:])
        assert both_gates(go) >= 1


def group_unslotted(mk, dev):
    """words without slots under the gate: a one-level context (exact bases always), and a slotted context in which a region
    gets more words than its slot holds, so that the last level is redone with exact bases (SHK_E_SLOT_FULL inside the
    library). The records are loaded up front, the words are not"""
    old = merged(*[repeats(r, 12, 6, seed=14) for r in range(NREG)])
    new = merged(repeats(2, 300, 40, seed=15), *[repeats(r, 20, 10, seed=15) for r in (0, 1, 5, 7)])
    again = merged(*[repeats(r, 15, 10, seed=16) for r in range(NREG)])

    def go():
        out, passes = run_batches(mk, dev, [old, new, again], max_level_bits=1, max_batch_keys=1024, slotted=[True, "redo", True])
        return out, min(passes[1:])
    assert both_gates(go) >= 1

    def go1():
        out, passes = run_batches(mk, dev, [old, new, again], slotted=[False, False, False])
        return out, min(passes[1:])
    assert both_gates(go1) >= 1


def _point(mk, dev, ml, env, want_profile, slotted):
    """a deNoise point inside a dense batch of four chunks on top of live records, against the oracle's t = 1 schedule:
    rounds, removed, table, header, totals. -> what the library printed about the point (SHK_DEBUG_FUSED)"""
    import cqflibs
    from fastq_util import oracle_header
    rnd = random.Random(21)
    pool = [key(rnd.randrange(1 << 16), r) for r in range(NREG) for _ in range(70)]
    rnd.shuffle(pool)
    batch0 = pool[:120] + pool[:50]
    chunks = [pool[120:220] + pool[60:100], pool[220:300] + pool[120:160] + pool[:20], pool[300:380] + pool[200:240],
              pool[380:460] + pool[300:330] + pool[100:120]]
    O = cqflibs.oracle()
    q = O.new(QB)
    for k in batch0:
        q.insert(k, 1)
    nd = []
    for ch in chunks:
        for k in ch:
            q.insert(k, 1)
        nd.append(q.ndistinct())
    q.free()
    trigger = nd[1]
    assert nd[0] < trigger < nd[3]
    q = O.new(QB)
    for k in batch0:
        q.insert(k, 1)
    rounds = removed = 0
    for ch in chunks:
        for k in ch:
            q.insert(k, 1)
        if rounds == 0 and q.ndistinct() >= trigger:
            removed += q.denoise_round(ml)
            rounds += 1
    assert rounds == 1 and removed > 0 and not q.full()
    want = q.blocks(), oracle_header(q), q.nelts(), q.ndistinct()
    q.free()
    kw = {"max_level_bits": 1} if slotted else {}
    log = []

    def go():
        ctx = mk(qb=QB, k=21, max_batch_bytes=64, max_batch_keys=1 << 13, trigger=trigger, num_denoise=1, min_denoise_len=ml, **kw)
        ctx.profile(True)
        ws = list(batch0)
        random.Random(5).shuffle(ws)
        ctx.count_words(dev(ws), len(ws), 1)
        ws = [k | (ci << HB) for ci, ch in enumerate(chunks) for k in ch]
        random.Random(6).shuffle(ws)
        ctx.profile_reset()
        before = ctx.prefetch_passes()
        # the library's own words about the point go to stderr: keep them
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile() as tf:
            os.dup2(tf.fileno(), 2)
            try:
                st = ctx.count_words(dev(ws), len(ws), len(chunks))
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tf.seek(0)
            log.append(tf.read().decode())
        assert (st["denoise_rounds"], st["removed"]) == (rounds, removed), (st, removed, log[-1])
        prof = ctx.profile_get()
        for name in want_profile:
            assert prof.get(name, (0, 0.0))[0] >= 1, (name, prof, log[-1])
        t = ctx.totals()
        got = (ctx.blocks(), ctx.header(), t.nelts, t.ndistinct)
        assert got == want
        passes = ctx.prefetch_passes() - before
        ctx.close()
        return got, passes

    os.environ["SHK_DEBUG_FUSED"] = "1"
    for k, v in env.items():
        os.environ[k] = v
    try:
        assert both_gates(go) >= 1
    finally:
        for k in list(env) + ["SHK_DEBUG_FUSED"]:
            os.environ.pop(k, None)
    return log[0]


def group_sample(mk, dev):
    """the sampled statistics pass in front of a deNoise point (every second of the 8 regions: SHK_SAMPLE_STRIDE=2) runs
    the plain record-sourced instantiation on a strided grid, the one-pass point behind it the fused one"""
    log = _point(mk, dev, 1 << 20, {"SHK_SAMPLE_STRIDE": "2"}, ["k_region_merge<sample>", "k_region_merge<fused>"], slotted=True)
    assert "sample:" in log, log


def group_point(mk, dev):
    """the one-pass deNoise point with ranges of 64 slots: the range walk protects singletons at range ends, and the regions
    that hold one are rebuilt once more from a list (the second go of the fused instantiation); and a full point with one
    range, slotted and unslotted"""
    log = _point(mk, dev, 64, {}, ["k_region_merge<fused>"], slotted=True)
    prot = [int(ln.rsplit("protected", 1)[1]) for ln in log.splitlines() if "one-pass point at chunk" in ln]
    assert prot and prot[0] > 0, log           # (the listed launch ran)
    _point(mk, dev, 1 << 20, {}, ["k_region_merge<fused>"], slotted=False)


def group_gate(mk, dev):
    """the gate: the first batch of a context (no records yet) and a batch of fewer than 8 words per region leave the
    counter alone, a dense batch on live records raises it, SHK_MERGE_PREFETCH=0 keeps it at 0 (both_gates)"""
    old = merged(*[repeats(r, 30, 6, seed=17) for r in range(NREG)])                # dense, but nothing to read records from
    sparse = merged(*[repeats(r, 7, 3, seed=18) for r in range(NREG)], singles(4, 7))  # 63 words
    dense = merged(*[repeats(r, 7, 3, seed=19) for r in range(NREG)], singles(4, 8))   # 64 words
    assert sum(sparse.values()) == 8 * NREG - 1 and sum(dense.values()) == 8 * NREG

    def go():
        return run_batches(mk, dev, [old, sparse, dense, sparse])
    passes = both_gates(go)
    assert passes[0] == 0 and passes[1] == 0 and passes[2] >= 1 and passes[3] == 0, passes


RUN = {"slots": group_slots, "rounds": group_rounds, "records": group_records, "over": group_over, "empty": group_empty,
       "unslotted": group_unslotted, "sample": group_sample, "point": group_point, "gate": group_gate}


def main(argv):
    backend, group = argv[1], argv[2]
    mk, dev = _mk(backend)
    RUN[group](mk, dev)
    print("PREFETCH_GROUP_OK")


if __name__ == "__main__":
    main(sys.argv)
