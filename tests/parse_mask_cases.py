"""The newline flags between k_count_lines and k_emit_reads (csrc/kmer_kernels.hip; parse_stage in csrc/shk_api.hip): the
cases that only the flags path can get wrong. Shared by the emulator tests and the GPU tests of tests/test_parse_mask.py;
tests/test_text_shapes.py already sends every line structure and chunk table of tests/text_cases.py through the same path.
The yardstick is the oracle throughout. SHK_PARSE_MASK=0, read when a context is created, keeps the text-reading emitter
and stores no flags: every group below runs in a fresh child process, once as built and once with the variable set
(python parse_mask_cases.py BACKEND GROUP), asserts there, and prints a digest of the words and tables it saw, which the
parent compares between the two runs.

The geometry the cases are built around: one uint16_t of flags per 16-byte unit of the text, indexed from the text's base;
k_emit_reads takes groups of 8 units = 128 bytes of text per thread, aligned by absolute unit index, in rounds of
threads * 8 units; a chunk is cut into SHK_PARSE_SEGS = 16 segments of whole units; the flags buffer of a fresh context
holds max(max_batch_bytes, 4 * max_batch_keys) / 16 + 8 units."""
import ctypes as C
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEGS = 16
K = 21
GROUPS = ["group-edges", "chunk-edges", "rounds", "growth", "stale"]
EMU_GROUPS = GROUPS
GPU_GROUPS = GROUPS + ["rounds-1024"]
COUNT_LINES, EMIT_READS = "k_count_lines", "k_emit_reads"


def _bases(rnd, n):
    return bytes(rnd.choices(b"ACGT", k=n))


def _rec(head, seq, qual=None):
    return head + b"\n" + seq + b"\n+\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"


def _pad_rec(rnd, i, total, empty_quality=False):
    """a record of exactly `total` >= 60 bytes: a read of 21 .. 25 bases, the header takes the rest. empty_quality: the
    newline behind the read is among the record's last four bytes"""
    r = 21 + i % 5
    h = total - (r + 5 if empty_quality else 2 * r + 5)
    assert h >= 2
    rec = _rec(b"@" + b"h" * (h - 1), _bases(rnd, r), b"" if empty_quality else None)
    assert len(rec) == total
    return rec


def _mask_units(nbytes):
    """units of flags a text whose last chunk ends at nbytes needs (parse_stage)"""
    return nbytes // 16 + 8


def _initial_units(max_batch_bytes, max_batch_keys):
    return max(max_batch_bytes, 4 * max_batch_keys) // 16 + 8


# ---------------------------------------------------------------------------------------------------------- the texts
def group_edge_text():
    """one chunk, k = 21; record lengths step through 128 consecutive values (four times), so that the newline behind the
    header, the read, the '+' and the quality line each fall on every byte residue mod 128: 15/16 is a unit's edge, 127/0 a
    group's"""
    from text_cases import Text
    rnd = random.Random(71)
    recs = [_pad_rec(rnd, i, 61 + i % 128) for i in range(512)]
    fq = b"".join(recs)
    res = [set(), set(), set(), set()]
    line = 0
    for p, b in enumerate(fq):
        if b == 10:
            res[line % 4].add(p % 128)
            line += 1
    for kind in range(4):
        assert res[kind] == set(range(128)), (kind, sorted(set(range(128)) - res[kind]))
        assert {15, 16, 127, 0} <= res[kind]
    return Text("group-edges", K, 14, fq, [0], [len(fq)])


def chunk_edge_text():
    """one or two records per chunk; chunk starts and ends on every residue mod 128 from the text's base; two chunks share a
    16-byte unit; two chunks share a group of 8 units but no unit; gaps between chunks hold newlines that belong to no
    chunk; chunks shorter than SHK_PARSE_SEGS units (empty segments)"""
    from text_cases import Text
    rnd = random.Random(72)
    text, offs, lens = bytearray(b"@front\nACGT\n+\nIIII\n\n"), [], []
    i = 0
    for c in range(128):
        # chunk c starts on residue 5 c and ends on residue 7 c + 3 (mod 128): the gap in front of it (newlines, or a line
        # of junk) and the length of its last record see to that; the gaps take every even length from 0 to 126
        gap = (5 * c - len(text)) % 128
        text += b"\n" * gap if c % 2 else (b"x" * (gap - 1) + b"\n")[:gap]
        offs.append(len(text))
        if c % 3 == 0:
            text += _pad_rec(rnd, i, rnd.randrange(60, 190))
            i += 1
        # (every fourth chunk ends four bytes behind its last read: the flags of a chunk's last unit matter to the extents)
        text += _pad_rec(rnd, i, 60 + (7 * c + 3 - (len(text) + 60)) % 128, empty_quality=c % 4 == 1)
        i += 1
        lens.append(len(text) - offs[-1])
    text += b"\n@back\nACGT\n+\nIIII\n"
    ends = [a + n for a, n in zip(offs, lens)]
    assert {a % 128 for a in offs} == set(range(128)) and {e % 128 for e in ends} == set(range(128))
    pairs = list(zip(ends[:-1], offs[1:]))
    assert any((e - 1) // 16 == a // 16 for e, a in pairs), "no two chunks share a unit"
    assert any((e - 1) // 128 == a // 128 and (e - 1) // 16 < a // 16 for e, a in pairs), "no two chunks share a group but no unit"
    assert any(b"\n" in text[e:a] for e, a in pairs), "no gap with newlines"
    assert any((a % 16 + n + 15) // 16 < SEGS for a, n in zip(offs, lens)), "no chunk shorter than SHK_PARSE_SEGS units"
    return Text("chunk-edges", K, 15, bytes(text), offs, lens)


def rounds_text(threads):
    """one chunk just over 2 * SHK_PARSE_SEGS * threads * 128 bytes: every segment takes more than two rounds of
    threads * 8 units, the line index is carried from round to round, the last group of a segment is partial. Few keys per
    byte (reads of 21 .. 25 bases under long or empty headers), so that the oracle and the card are done in seconds."""
    from text_cases import Text
    rnd = random.Random(73 + threads)
    target = 2 * SEGS * threads * 128
    parts, n, i = [], 0, 0
    while True:
        s = _bases(rnd, 21 + i % 5)
        rec = _rec(b"", s, b"") if i % 3 == 0 else _rec(b"@" + b"h" * ((i * 37) % 300), s)
        parts.append(rec)
        n += len(rec)
        i += 1
        units = (n + 15) // 16
        per = (units + SEGS - 1) // SEGS          # units per segment: no multiple of 8 either, so segments end inside a group
        if n > target + 2000 and units % 8 and units % SEGS and per % 8:
            break
    assert target < n < target + 20000 and per > 2 * threads * 8
    nk = sum(len(p.split(b"\n")[1]) - K + 1 for p in parts)
    qb = 12
    while (1 << qb) < 3 * nk:
        qb += 1
    return Text("rounds-%d" % threads, K, qb, b"".join(parts), [0], [n])


def growth_texts():
    """(small, big): big has so few keys per byte that a context made for its keys starts with a flags buffer smaller than
    big needs"""
    from text_cases import Text
    rnd = random.Random(74)
    small = [_pad_rec(rnd, i, 70 + i % 9) for i in range(6)]
    big = [_rec(b"@" + b"h" * (300 + (i * 53) % 200), _bases(rnd, 21 + i % 5)) for i in range(60)]

    def tile(recs, per):
        offs, lens, pos = [], [], 0
        for j in range(0, len(recs), per):
            m = sum(len(r) for r in recs[j:j + per])
            offs.append(pos)
            lens.append(m)
            pos += m
        return offs, lens
    return (Text("growth-small", K, 12, b"".join(small), *tile(small, 2)), Text("growth-big", K, 12, b"".join(big), *tile(big, 7)))


def stale_texts():
    """(first, second) of equal length: the first of short lines, the second of long ones, so that the first has newlines
    where the second has bases"""
    from text_cases import Text
    rnd = random.Random(75)
    long_ = [_rec(b"@long%d" % i, _bases(rnd, 280 + i % 7)) for i in range(12)]
    second = b"".join(long_)
    short, n, i = [], 0, 0
    while len(second) - n >= 140:
        short.append(_pad_rec(rnd, i, 60 + i % 5))
        n += len(short[-1])
        i += 1
    short.append(_pad_rec(rnd, i, len(second) - n))
    first = b"".join(short)
    assert len(first) == len(second)
    # newlines of the first text inside sequence lines of the second
    seq = bytearray(len(second))
    pos = 0
    for r in long_:
        a = pos + r.index(b"\n") + 1
        seq[a:a + len(r.split(b"\n")[1])] = b"\x01" * len(r.split(b"\n")[1])
        pos += len(r)
    hits = sum(1 for p, b in enumerate(first) if b == 10 and seq[p])
    assert hits >= 100, hits

    def tile(recs, per):
        offs, lens, p = [], [], 0
        for j in range(0, len(recs), per):
            m = sum(len(r) for r in recs[j:j + per])
            offs.append(p)
            lens.append(m)
            p += m
        return offs, lens
    return Text("stale-first", K, 13, first, *tile(short, 9)), Text("stale-second", K, 13, second, *tile(long_, 5))


# ---------------------------------------------------------------------------------------------------------- the checks
class _Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, *objs):
        for o in objs:
            self.h.update(o if isinstance(o, (bytes, bytearray)) else repr(o).encode())


def _state(ctx):
    t = ctx.totals()
    return ctx.blocks(), ctx.header(), t.nelts, t.ndistinct


def _kernels(ctx, D):
    p = ctx.profile_get()
    assert COUNT_LINES in p and EMIT_READS in p, p
    assert p[COUNT_LINES][0] == p[EMIT_READS][0], p
    D.add(sorted(n for n in p if n in (COUNT_LINES, EMIT_READS)))


def _words_and_table(mk, T, D, **kw):
    """shk_hash_chunks on device text (an allocation that ends at the next multiple of 16 behind the text): the oracle's
    words in stream order with chunk tags; shk_count_chunks on host text: the oracle's table"""
    import text_cases as TC
    exp, blocks, header, nelts, ndistinct = T.expected()
    ctx = TC._ctx_for(lambda **k2: mk(**dict(k2, **kw)), T)
    ctx.profile(True)
    dp, nw = ctx.hash_chunks(ctx.dev_text(T.fq), T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
    words = ctx.read_words(dp, nw)
    assert nw == len(exp) and words == exp, T.name
    st = ctx.count_chunks(T.fq, T.offs, T.lens)
    assert st["kmers"] == nelts and _state(ctx) == (blocks, header, nelts, ndistinct), T.name
    _kernels(ctx, D)
    D.add(words, *_state(ctx))
    ctx.close()


def group_group_edges(mk, emu, D):
    _words_and_table(mk, group_edge_text(), D)


def group_chunk_edges(mk, emu, D):
    _words_and_table(mk, chunk_edge_text(), D)


def group_rounds(mk, emu, D):
    _words_and_table(mk, rounds_text(64 if emu else 512), D)


def group_rounds_1024(mk, emu, D):
    _words_and_table(mk, rounds_text(1024), D, threads_per_group=1024)


def group_growth(mk, emu, D):
    """device text on a context with max_batch_bytes = 64 and max_batch_keys = the big text's keys: small, big (over the
    initial capacity of the flags buffer), small again; then the same through the overlapped pair, two batches ahead"""
    import cqflibs
    small, big = growth_texts()
    nk = len(big.expected()[0])
    assert len(small.expected()[0]) <= nk
    assert _mask_units(len(small.fq)) <= _initial_units(64, nk) < _mask_units(len(big.fq)), (len(small.fq), nk, len(big.fq))
    nreads = big.fq.count(b"\n") + 64
    O = cqflibs.oracle()

    def oracle_after(seq):
        from fastq_util import oracle_header
        q = O.new(12)
        for T in seq:
            for c in T.chunks():
                q.reads_to_kmers(c, K)
        st = (q.blocks(), oracle_header(q), q.nelts(), q.ndistinct())
        q.free()
        return st

    ctx = mk(qb=12, k=K, max_batch_bytes=64, max_batch_keys=nk, max_batch_reads=nreads)
    ctx.profile(True)
    seq = []
    for T in (small, big, small):
        p = ctx.dev_text(T.fq)
        dp, nw = ctx.hash_chunks(p, T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
        words = ctx.read_words(dp, nw)
        assert words == T.expected()[0], T.name
        st = ctx.count_chunks(p, T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
        seq.append(T)
        assert st["kmers"] == len(words) and _state(ctx) == oracle_after(seq), T.name
        D.add(words, *_state(ctx))
    _kernels(ctx, D)
    ctx.close()

    ctx = mk(qb=12, k=K, max_batch_bytes=64, max_batch_keys=nk, max_batch_reads=nreads)
    ctx.profile(True)
    ptrs = [ctx.dev_text(T.fq) for T in (small, big)]
    for T, p in zip((small, big), ptrs):
        ctx.prepare_chunks(p, T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
    for n, T in enumerate((small, big)):
        st = ctx.count_prepared()
        assert st["kmers"] == len(T.expected()[0]), T.name
        assert _state(ctx) == oracle_after((small, big)[:n + 1]), T.name
    D.add(*_state(ctx))
    _kernels(ctx, D)
    ctx.close()


def group_stale(mk, emu, D):
    """two texts of equal length on one context, device text and host text: the second text's words are the oracle's
    whatever flags the first left behind"""
    import text_cases as TC
    first, second = stale_texts()
    for on_device in (True, False):
        ctx = TC._ctx_for(mk, first if len(first.expected()[0]) > len(second.expected()[0]) else second)
        ctx.profile(True)
        for T in (first, second):
            if on_device:
                dp, nw = ctx.hash_chunks(ctx.dev_text(T.fq), T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
            else:
                dp, nw = ctx.hash_chunks(T.fq, T.offs, T.lens)
            words = ctx.read_words(dp, nw)
            assert words == T.expected()[0], (T.name, on_device)
            D.add(words)
        ctx.count_chunks(first.fq, first.offs, first.lens)
        ctx.count_chunks(second.fq, second.offs, second.lens)
        import cqflibs
        from fastq_util import oracle_header
        q = cqflibs.oracle().new(13)
        for T in (first, second):
            for c in T.chunks():
                q.reads_to_kmers(c, K)
        assert _state(ctx) == (q.blocks(), oracle_header(q), q.nelts(), q.ndistinct()), on_device
        q.free()
        D.add(*_state(ctx))
        _kernels(ctx, D)
        ctx.close()


RUN = {"group-edges": group_group_edges, "chunk-edges": group_chunk_edges, "rounds": group_rounds, "rounds-1024": group_rounds_1024,
       "growth": group_growth, "stale": group_stale}


# ---------------------------------------------------------------------------------------------------------- factories
def _emu_factory(shk):
    """contexts on the emulator build; their "device" text is host memory of exactly the documented extent"""
    lib = os.path.join(HERE, "emu", "libshk_emu.so")
    libc = C.CDLL(None)
    libc.posix_memalign.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t]
    libc.free.argtypes = [C.c_void_p]

    def mk(**kw):
        kw.setdefault("threads_per_group", 64)
        ctx = shk.Context(hash_groups=2, lib_path=lib, **kw)
        ctx.read_words = lambda dp, n: list((C.c_uint64 * max(n, 1)).from_address(dp)[:n])
        held = []

        def dev_text(data, offset=0):
            p = C.c_void_p()
            assert libc.posix_memalign(C.byref(p), 16, offset + ((len(data) + 15) & ~15)) == 0
            C.memmove(p.value + offset, data, len(data))
            held.append(p)
            return p.value + offset
        ctx.dev_text = dev_text
        close = ctx.close

        def close_and_free():
            close()
            while held:
                libc.free(held.pop())
        ctx.close = close_and_free
        return ctx
    return mk


def _gpu_factory(shk):
    import torch
    from shk import dist as shkdist
    dev = torch.device("cuda", 0)

    def mk(**kw):
        ctx = shk.Context(**kw)
        ctx.read_words = lambda dp, n: [x & 0xFFFFFFFFFFFFFFFF for x in shkdist.wrap_words(dp, n, dev).cpu().tolist()] if n else []
        held = []

        def dev_text(data, offset=0):
            t = torch.empty(offset + ((len(data) + 15) & ~15), dtype=torch.uint8, device=dev)
            t[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            torch.cuda.synchronize()
            held.append(t)
            assert t.data_ptr() % 16 == 0
            return t.data_ptr() + offset
        ctx.dev_text = dev_text
        return ctx
    return mk


def main(argv):
    backend, group = argv[1], argv[2]
    for p in (HERE, ROOT, os.path.join(ROOT, "sh-assembly_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    emu = backend == "emu"
    if not emu:
        import torch  # noqa: F401  (before libshk.so: one HIP runtime per process, see tests/conftest.py)
    import shk
    D = _Digest()
    RUN[group]((_emu_factory if emu else _gpu_factory)(shk), emu, D)
    print(json.dumps({"digest": D.h.hexdigest()}))
    print("PARSE_MASK_GROUP_OK")


if __name__ == "__main__":
    main(sys.argv)
