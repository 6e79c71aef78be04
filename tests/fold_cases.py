"""The fold of a region's batch words into its LDS hash (csrc/cqf_kernels.hip, k_region_merge: first probe of a lane's four
words side by side, then the collided words from one queue per lane). Shared by the emulator tests and the GPU tests of
tests/test_fold_probe.py: every group runs in a fresh child process (python fold_cases.py BACKEND GROUP), asserts there and
prints FOLD_GROUP_OK.

Key words go in through shk_count_words at qb 11 / hb 19 (8 regions of 256 quotients). A word's tag is
`local quotient << 8 | remainder`; its home entry in the hash of 512 is ((tag * 40503) & 0xFFFF) >> 7, so 128 tags share
every entry and a chain is a set of tags chosen by entry. The caller does not control the order in which a region's words
reach the kernel (the partition scatters them): every group runs under several seeded shuffles. The yardstick is
cqf_canon.build_blocks, and the oracle where a deNoise round is involved."""
import ctypes as C
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
QB, HB = 11, 19
HCAP = 512
REGION = 1                     # the region the chains live in: quotients 256 .. 511
SEEDS = (1, 2, 3)
GROUPS = ["chain", "wrap", "capacity", "overflow", "rounds", "point", "counted"]


def entry(tag):
    """the kernel's formula"""
    return ((tag * 40503) & 0xFFFF) >> 7


def tags_of(e):
    """the 128 tags whose home entry is e"""
    return [t for t in range(1 << 16) if entry(t) == e]


def key(tag, region=REGION):
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


def _ctx(mk, **kw):
    ctx = mk(qb=QB, k=21, max_batch_bytes=64, max_batch_keys=1 << 13, **kw)
    ctx.profile(True)
    return ctx


def _words(counts, seed, chunk=0):
    ws = [k | (chunk << HB) for k, c in counts.items() for _ in range(c)]
    random.Random(seed).shuffle(ws)
    return ws


def _check_counts(mk, dev, counts, min_words=0, nchunks=1):
    """one batch of `counts` (key -> occurrences) into an empty filter, under every shuffle: the canonical table"""
    from cqf_canon import build_blocks
    want = build_blocks(QB, HB, counts)
    total = sum(counts.values())
    assert total >= min_words
    for seed in SEEDS:
        ctx = _ctx(mk)
        ws = _words(counts, seed)
        st = ctx.count_words(dev(ws), len(ws), nchunks)
        assert st["kmers"] == total, (seed, st)
        t = ctx.totals()
        assert (t.nelts, t.ndistinct) == (total, len(counts)), seed
        assert ctx.blocks() == want, seed
        ctx.close()


def group_chain(mk, dev):
    """100 distinct keys of one region in ONE chain: all share entry 200, each 1..5 times, 400+ words -- the lanes hold
    several collided words at once, the last key of the chain is 99 entries from home"""
    rnd = random.Random(11)
    tags = rnd.sample(tags_of(200), 100)
    counts = {key(t): 1 + i % 5 for i, t in enumerate(tags)}
    counts[key(tags[0])] += 110                    # (so that the words are more than 400 whatever the draw)
    _check_counts(mk, dev, counts, min_words=400)


def group_wrap(mk, dev):
    """chains that start at entries 505 .. 511 and go on at entry 0: 12 keys per entry, 84 keys for 7 entries, so that
    the last ones land 70 entries and more behind the end of the table"""
    rnd = random.Random(12)
    counts = {}
    for e in range(505, 512):
        for i, t in enumerate(rnd.sample(tags_of(e), 12)):
            counts[key(t)] = 1 + (i + e) % 4
    assert len(counts) == 84
    _check_counts(mk, dev, counts)


def _distinct(n, seed):
    """n distinct keys of the region, any entry"""
    rnd = random.Random(seed)
    return [key(t) for t in rnd.sample(range(1 << 16), n)]


def group_capacity(mk, dev):
    """exactly SHK_HCAP distinct keys of one region in one chunk fill the hash to the last entry: the canonical table"""
    keys = _distinct(HCAP + 1, 13)
    _check_counts(mk, dev, {k: 1 for k in keys[:HCAP]})


def group_overflow(mk, dev):
    """one key more than the hash holds (the keys of the capacity group and one more) in one chunk cannot be folded: an
    error, and the table keeps its bytes. The same 513 over two chunks: the host halves the chunk range and succeeds."""
    import shk
    from cqf_canon import build_blocks
    keys = _distinct(HCAP + 1, 13)
    want513 = build_blocks(QB, HB, {k: 1 for k in keys})
    for seed in SEEDS[:2]:       # (two passes and a retry per shuffle: two shuffles keep the group under a second)
        # 513 in one chunk, on top of a small table
        ctx = _ctx(mk)
        first = {key(5 + i, region=3): 2 for i in range(20)}
        ws = _words(first, seed)
        ctx.count_words(dev(ws), len(ws), 1)
        before = ctx.blocks()
        assert before == build_blocks(QB, HB, first)
        ws = _words({k: 1 for k in keys}, seed)
        try:
            ctx.count_words(dev(ws), len(ws), 1)
            raise AssertionError("513 distinct keys of one region in one chunk were folded")
        except shk.ShkError:
            pass
        assert ctx.blocks() == before, seed
        ctx.close()
        # 513 over two chunks
        ctx = _ctx(mk)
        half = len(keys) // 2
        ws = [k | (0 << HB) for k in keys[:half]] + [k | (1 << HB) for k in keys[half:]]
        random.Random(seed).shuffle(ws)
        st = ctx.count_words(dev(ws), len(ws), 2)
        assert st["kmers"] == len(keys)
        assert ctx.blocks() == want513, seed
        ctx.close()


def group_rounds(mk, dev):
    """2000 words of 100 keys in one region: several rounds of four words per lane, the later ones against a hash that
    holds every key already; 60 of the keys in two chains"""
    rnd = random.Random(14)
    tags = rnd.sample(tags_of(77), 30) + rnd.sample(tags_of(300), 30)
    tags += [t for t in rnd.sample(range(1 << 16), 60) if entry(t) not in (77, 300)][:40]
    assert len(set(tags)) == 100
    counts = {key(t): 1 for t in tags}
    ks = list(counts)
    for i in range(2000 - 100):
        counts[ks[(i * i + 3 * i) % 100]] += 1
    assert sum(counts.values()) == 2000
    _check_counts(mk, dev, counts)


def group_point(mk, dev):
    """a deNoise point inside the batch, taken by the one-pass instantiation: the trigger is the oracle's ndistinct behind
    chunk 1 of 4. Keys of one chain (entry 150) and of a chain across the end of the table (entry 510) sit on both sides of
    the split: singletons in front of it, which go; keys seen twice in front of it, which stay; singletons in front of it
    that return behind it; keys that only come behind it; old keys of the table with one occurrence that get their second
    in front of the point or only behind it. Against the oracle's t = 1 schedule: rounds, removed, table, header."""
    import cqflibs
    from fastq_util import oracle_header
    rnd = random.Random(15)
    chain = rnd.sample(tags_of(150), 70) + rnd.sample(tags_of(510), 30)
    rnd.shuffle(chain)
    go, stay, back, late, old_a, old_b = (chain[0:20], chain[20:40], chain[40:60], chain[60:80], chain[80:90], chain[90:100])
    filler = [key(rnd.randrange(1 << 16), region=rnd.choice([0, 2, 3, 4, 5, 6, 7])) for _ in range(400)]
    batch0 = [key(t) for t in old_a + old_b] + filler[:150] + filler[:60]
    chunks = [
        [key(t) for t in go[:10] + stay + back[:10] + old_a] + filler[150:230],
        [key(t) for t in go[10:] + stay + back[10:]] + filler[230:300] + filler[150:170],
        [key(t) for t in back + late[:10] + old_b] + filler[300:350],
        [key(t) for t in late + late[:5] + back[:5]] + filler[350:400],
    ]
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
    assert q.ndistinct() < trigger
    rounds = removed = 0
    for ch in chunks:
        for k in ch:
            q.insert(k, 1)
        if rounds == 0 and q.ndistinct() >= trigger:
            removed += q.denoise_round(1 << 20)
            rounds += 1
    assert rounds == 1 and removed >= len(go) + len(back) and not q.full()
    want = q.blocks(), oracle_header(q), q.nelts(), q.ndistinct()
    q.free()
    for seed in SEEDS:
        ctx = _ctx(mk, trigger=trigger, num_denoise=1, min_denoise_len=1 << 20)
        ws = list(batch0)
        random.Random(seed).shuffle(ws)
        ctx.count_words(dev(ws), len(ws), 1)
        ws = [k | (ci << HB) for ci, ch in enumerate(chunks) for k in ch]
        random.Random(seed).shuffle(ws)
        ctx.profile_reset()
        st = ctx.count_words(dev(ws), len(ws), len(chunks))
        assert (st["denoise_rounds"], st["removed"]) == (rounds, removed), (seed, st, removed)
        prof = ctx.profile_get()
        assert prof.get("k_region_merge<fused>", (0, 0.0))[0] >= 1, (seed, prof)          # the one-pass point ran ...
        # ... and stood: handed back to the general path, the chunks on either side of the point take a plain pass each
        assert prof.get("k_region_merge<spill>", (0, 0.0))[0] <= 1, (seed, prof)
        t = ctx.totals()
        assert (ctx.blocks(), ctx.header(), t.nelts, t.ndistinct) == want, seed
        ctx.close()


def group_counted(mk, dev):
    """shk_insert_counted: the words carry a multiplicity where a batch word has its chunk. Keys of one chain with
    multiplicities above 1, some keys twice in the call"""
    from cqf_canon import build_blocks
    rnd = random.Random(16)
    tags = rnd.sample(tags_of(411), 60) + rnd.sample(tags_of(511), 20)
    for seed in SEEDS:
        r = random.Random(seed)
        pairs = [(key(t), r.choice([1, 2, 3, 7, 250, 3000])) for t in tags]
        pairs += [(key(t), r.choice([1, 4, 90])) for t in tags[:25]]           # a second time, to be added up
        r.shuffle(pairs)
        counts = {}
        for k, c in pairs:
            counts[k] = counts.get(k, 0) + c
        ctx = _ctx(mk)
        st = ctx.insert_counted([k for k, _ in pairs], [c for _, c in pairs])
        assert st["kmers"] == sum(counts.values()), (seed, st)
        assert ctx.blocks() == build_blocks(QB, HB, counts), seed
        ctx.close()


RUN = {"chain": group_chain, "wrap": group_wrap, "capacity": group_capacity, "overflow": group_overflow, "rounds": group_rounds, "point": group_point,
       "counted": group_counted}


def main(argv):
    backend, group = argv[1], argv[2]
    mk, dev = _mk(backend)
    RUN[group](mk, dev)
    print("FOLD_GROUP_OK")


if __name__ == "__main__":
    main(sys.argv)
