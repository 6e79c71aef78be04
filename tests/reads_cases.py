"""Cases for shk_query_reads (include/shk.h), shared by the emulator and the GPU tests of tests/test_reads.py.

Expected values never come from the library: reads_of and windows below read the chunks byte by byte (a read is the second of every
four lines counted from a chunk's first byte; window j is a k-mer exactly when its k bytes are bases), the keys come from
cqflibs.oracle().seq_keys, the counts from a Python dict from hashed key to count that is filled next to the table
(Context.insert_counted), the median from sorted(). All comparisons are exact."""
import contextlib
import ctypes as C
import os
import random

import numpy as np

import cqflibs
import fasta_cases as FC
import query_cases as QC

NONE, CAP, M64 = QC.NONE, QC.CAP, QC.M64
REC_FIELDS = ("sum", "kmers", "present", "solid", "min", "median", "max")
NOT_BASES = (b"N", b"n", b"R", b".", b"-")


def fastq(seqs, eol=b"\n", quals=None, last_eol=True):
    """four-line records; quals: None (all 'I') or one quality line per read"""
    out = []
    for i, s in enumerate(seqs):
        q = quals[i] if quals is not None else b"I" * len(s)
        out.append(b"@r%d some words" % i + eol + s + eol + b"+" + eol + q + eol)
    text = b"".join(out)
    return text if last_eol else text[:len(text) - len(eol)]


def reads_of(text, chunk_off, chunk_len):
    """[(seq_off, seq_len, chunk)] as the front end finds them: in a chunk, the line behind every line feed of index
    0 mod 4 that is itself ended by a line feed inside the chunk"""
    out = []
    for c, (o, n) in enumerate(zip(chunk_off, chunk_len)):
        nl = [o + i for i, b in enumerate(text[o:o + n]) if b == 10]
        for i in range(0, len(nl) - 1, 4):
            out.append((nl[i] + 1, nl[i + 1] - nl[i] - 1, c))
    return out


def windows(seq, k):
    """per window of the sequence line the k-mer's bytes, or None where it holds a byte that is no base"""
    out, last_bad = [], -1
    for i, b in enumerate(seq):
        if b not in FC.BASES:
            last_bad = i
        if i + 1 >= k:
            out.append(bytes(seq[i + 1 - k:i + 1]) if i - last_bad >= k else None)
    return out


def all_keys(text, chunk_off, chunk_len, k, hb):
    kmers = [w for o, n, _ in reads_of(text, chunk_off, chunk_len) for w in windows(text[o:o + n], k) if w is not None]
    return cqflibs.oracle().seq_keys(kmers, k, hb) if kmers else np.zeros(0, dtype=np.uint64)


def expect(text, chunk_off, chunk_len, k, hb, table, min_count, median):
    """(rstats, records as rows of REC_FIELDS, extents, track) the call must answer"""
    reads = reads_of(text, chunk_off, chunk_len)
    wins = [windows(text[o:o + n], k) for o, n, _ in reads]
    kmers = [w for ws in wins for w in ws if w is not None]
    keys = cqflibs.oracle().seq_keys(kmers, k, hb) if kmers else []
    counts = iter(table.get(int(x), 0) for x in keys)
    rec, track = [], []
    for ws in wins:
        cs = [next(counts) if w is not None else None for w in ws]
        track += [NONE if c is None else min(c, CAP) for c in cs]
        cs = [c for c in cs if c is not None]
        capped = sorted(min(c, CAP) for c in cs)
        med = (capped[(len(cs) - 1) // 2] if cs else 0) if median else NONE
        rec.append((sum(cs) & M64, len(cs), sum(c >= 1 for c in cs), sum(c >= min_count for c in cs),
                    capped[0] if cs else 0, med, capped[-1] if cs else 0))
    rs = {"reads": len(reads)}
    for name, col in (("kmers", 1), ("present", 2), ("solid", 3)):
        rs[name] = sum(r[col] for r in rec)
    rs["sum"] = sum(r[0] for r in rec) & M64
    return rs, rec, reads, np.array(track, dtype=np.uint32)


def rows(rec):
    return [tuple(int(r[f]) for f in REC_FIELDS) for r in rec]


def ask(ctx, text, chunk_off, chunk_len, table, min_count=2, median=True, want_track=True, what="", **kw):
    """one call against the model's answer; returns what the call answered"""
    want_rs, want_rec, want_ext, want_track_ = expect(text, chunk_off, chunk_len, ctx.cfg.k, ctx.cfg.hb, table, min_count, median)
    rs, rec, ext, track = ctx.query_reads(kw.pop("call_text", text), chunk_off, chunk_len, min_count=min_count, median=median,
                                          want_track=want_track, want_extents=True, **kw)
    assert rs == want_rs, (what, rs, want_rs)
    got = rows(rec)
    assert len(got) == len(want_rec), (what, len(got), len(want_rec))
    bad = [i for i, (a, b) in enumerate(zip(got, want_rec)) if a != b]
    assert not bad, (what, "read %d" % bad[0], dict(zip(REC_FIELDS, got[bad[0]])), dict(zip(REC_FIELDS, want_rec[bad[0]])))
    assert [tuple(int(x) for x in e) for e in ext.tolist()] == want_ext, what
    if want_track:
        assert track.dtype == np.uint32 and len(track) == len(want_track_), (what, len(track), len(want_track_))
        bad = np.flatnonzero(track != want_track_)
        assert len(bad) == 0, (what, "track differs first at window %d" % bad[0], int(track[bad[0]]), int(want_track_[bad[0]]))
    else:
        assert track is None
    return rs, rec, ext, track


def ctx_for(mk, qb, k, text_cap=1 << 16, **kw):
    kw.setdefault("max_batch_keys", text_cap)
    return mk(qb=qb, k=k, max_batch_bytes=text_cap, **kw)


def one_chunk(text):
    return [0], [len(text)]


@contextlib.contextmanager
def no_pack():
    os.environ["SHK_NO_PACK"] = "1"
    try:
        yield
    finally:
        del os.environ["SHK_NO_PACK"]


# ---------------------------------------------------------------- texts
def shape_reads(k, seed):
    """the read lengths and the bytes that are no bases of the issue's list, on one genome so that k-mers repeat"""
    rng = random.Random(seed)
    g = FC.dna(1500, seed)

    def piece(n):
        at = rng.randrange(0, len(g) - n) if n < len(g) else 0
        return bytearray(g[at:at + n])
    lens = sorted(set(n for n in (k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 200, 2 * k + 3) if n >= 0))
    seqs = [bytes(piece(n)) for n in lens]
    seqs.append(b"")                                    # an empty sequence line
    seqs.append(bytes(piece(2 * k + 3)).lower())        # lower case
    mixed = piece(130)
    mixed[::3] = bytes(mixed[::3]).lower()
    seqs.append(bytes(mixed))
    n = max(2 * k + 3, 70)
    spots = sorted(set(p for p in (0, k - 1, k, n - k - 1, n - k, n - 1) if 0 <= p < n))
    for j, p in enumerate(spots):
        s = piece(n)
        s[p:p + 1] = NOT_BASES[j % len(NOT_BASES)]
        seqs.append(bytes(s))
    s = piece(n)
    for j, p in enumerate(spots):
        s[p:p + 1] = NOT_BASES[(j + 2) % len(NOT_BASES)]
    seqs.append(bytes(s))
    return seqs


def shape_text(k, seed, eol=b"\n"):
    seqs = shape_reads(k, seed)
    quals = [(b"@" if i % 2 else b"+") + b"I" * (len(s) - 1) if s else b"" for i, s in enumerate(seqs)]
    return fastq(seqs, eol=eol, quals=quals)


def half_table(ctx, text, chunk_off, chunk_len):
    table = {}
    QC.fill(ctx, table, QC.half_of(all_keys(text, chunk_off, chunk_len, ctx.cfg.k, ctx.cfg.hb)))
    return table


# ---------------------------------------------------------------- runners (mk = context factory of the build under test)
def run_shapes(mk, k, qb=12):
    """2. shapes of a read, LF and CRLF"""
    for eol in (b"\n", b"\r\n"):
        text = shape_text(k, 300 + k, eol)
        ctx = ctx_for(mk, qb, k, max_level_bits=3)
        table = half_table(ctx, text, *one_chunk(text))
        rs, rec, ext, track = ask(ctx, text, *one_chunk(text), table, what="k=%d eol=%r" % (k, eol))
        assert int((track == NONE).sum()) > 0 and 0 < rs["present"] < rs["kmers"]
        if eol == b"\r\n":      # the '\r' belongs to the sequence line, and no window that holds it is a k-mer
            assert all(text[int(e["seq_off"]) + int(e["seq_len"]) - 1] == 13 for e in ext)
            assert all(int(r["kmers"]) <= max(int(e["seq_len"]) - k, 0) for r, e in zip(rec, ext))
        ctx.close()


def run_sources(mk, k=31, qb=12):
    """3. both sources of the bases: the 2-bit units, SHK_NO_PACK=1, a context too small for the units"""
    text = shape_text(k, 17) + fastq([FC.dna(n, 40 + n) for n in (150, 151, 100, 64, 31)] + [FC.dna(560, 3)[i:i + k] for i in range(500)])
    ctx = ctx_for(mk, qb, k, max_level_bits=3)
    table = half_table(ctx, text, *one_chunk(text))
    a = ask(ctx, text, *one_chunk(text), table, what="as it is")
    with no_pack():
        b = ask(ctx, text, *one_chunk(text), table, what="SHK_NO_PACK=1")
    nwin, nreads = len(a[3]), len(a[1])
    keys = nwin + 8
    assert len(text) // 64 + nreads + 1 > keys // 2 - 1, "the units must not fit"
    small = ctx_for(mk, qb, k, max_batch_keys=keys, max_level_bits=3)
    QC.fill(small, {}, sorted(table.items()))
    c = ask(small, text, *one_chunk(text), table, what="max_batch_keys too small for the units")
    for other in (b, c):
        assert rows(other[1]) == rows(a[1]) and np.array_equal(other[3], a[3])
    small.close()
    ctx.close()


def chunk_text(k, nrec, seed):
    rng = random.Random(seed)
    g = FC.dna(600, seed)
    recs = []
    for i in range(nrec):
        n = rng.randrange(k - 2, k + 60)
        at = rng.randrange(0, len(g) - n)
        s = bytearray(g[at:at + n])
        if i % 7 == 3 and n:
            s[rng.randrange(n)] = ord("N")
        recs.append(fastq([bytes(s)]))
    return recs


def run_chunks(mk, dev_bytes, k=21, qb=12):
    """4. chunk tables"""
    recs = chunk_text(k, 40, 9)
    text = b"".join(recs)
    bounds = np.cumsum([0] + [len(r) for r in recs]).tolist()
    # 17 chunks in reverse order: two records each with a record nobody asked for between them, an empty chunk, three bytes
    offs, lens = [], []
    for i in range(15):
        a = 2 * i + (i // 2)
        offs.append(bounds[a])
        lens.append(bounds[a + 2] - bounds[a])
    offs, lens = offs[::-1], lens[::-1]
    offs[5:5] = [bounds[3]]
    lens[5:5] = [0]
    offs.append(bounds[39])
    lens.append(3)
    assert len(offs) == 17
    ctx = ctx_for(mk, qb, k, max_level_bits=3)
    table = half_table(ctx, text, [0], [len(text)])
    rs, rec, ext, _ = ask(ctx, text, offs, lens, table, what="17 chunks")
    assert rs["reads"] == 30 and [int(e["chunk"]) for e in ext] == sorted(int(e["chunk"]) for e in ext)
    ask(ctx, text, [bounds[4]], [bounds[9] - bounds[4]], table, what="1 chunk")
    rs, rec, ext, track = ctx.query_reads(text, [5, 40, len(text)], [0, 0, 0], want_track=True, want_extents=True, median=True)
    assert rs == {"reads": 0, "kmers": 0, "present": 0, "solid": 0, "sum": 0} and len(rec) == 0 and len(ext) == 0 and len(track) == 0
    # device text: 16-byte aligned answers as host text does, unaligned is SHK_ERR_ARG
    ptr, keep = dev_bytes(b"\n" * 16 + text)
    ask(ctx, text, offs, lens, table, what="device text", call_text=ptr + 16, on_device=True, text_bytes=len(text))
    assert raw_query(ctx, ptr + 1, offs, lens, 64, 0, on_device=True, text_bytes=len(text))["rc"] == -1
    ctx.close()


def run_hard_table(mk, k=31, qb=10):
    """5. counts that are hard: min, median and max capped at 0xFFFFFFFE, sum not"""
    fa, pairs = QC.hard_case(k, qb)
    seqs = [ln for ln in fa.split(b"\n") if ln and not ln.startswith(b">")]
    text = fastq(seqs)
    big = [p for p in pairs if p[1] >= 1 << 22]
    ctx, table = ctx_for(mk, qb, k, max_level_bits=2), dict(big)
    q = cqflibs.oracle().new(qb)
    for key, c in big:
        q.insert(key, c)
    ctx.import_blocks(q.blocks(), q.nelts(), q.ndistinct())
    q.free()
    rest = [p for p in pairs if p[1] < 1 << 22]
    for i in range(0, len(rest), 97):
        QC.fill(ctx, table, rest[i:i + 97])
    rs, rec, _, track = ask(ctx, text, *one_chunk(text), table, min_count=128, what="hard table")
    assert int((track == CAP).sum()) >= 4 * len(QC.SPECIAL_REMS) and int(rec["max"].max()) == CAP
    assert rs["sum"] >= len(QC.SPECIAL_REMS) * (1 << 35) and int(rec["sum"].max()) > CAP
    ctx.close()


def run_median(mk, k=21, qb=12):
    """6. reads on which the answer turns on the definition; the counts are put into the table k-mer by k-mer"""
    O = cqflibs.oracle()
    hb = qb + 8
    g = FC.dna(4000, 61)
    plans = {      # name -> counts of the read's k-mers in order; None = a window that is no k-mer
        "even": [1, 2, 3, 4], "odd": [5, 1, 3, 2, 4], "half absent": [0, 3, 0, 7, 9, 0], "all equal": [6] * 9, "all absent": [0] * 8,
        "one k-mer": [11], "top bit": [1 << 31, 0, 1 << 31, 0, 1 << 31], "bit 0": [6, 7, 6, 7, 7, 6, 7],
        "top bit and bit 0": [(1 << 31) + 1, 1 << 31, 1, 0, (1 << 31) + 1, 1],
        "interleaved": [2, None, 9, 9, None, None, 1, 4, None, 3],
    }
    # Every planned k-mer is a stretch of the genome of its own, the parts of a read are joined by an 'N', and a None is a
    # part whose last base is an 'N' too: every window across a seam holds an 'N', so the read's k-mers are exactly the
    # planned ones, in order, with windows that are no k-mers between any two of them.
    reads, pairs, at = [], {}, 0
    for plan in plans.values():
        parts = []
        for c in plan:
            kmer = g[at:at + k]
            at += k + 1
            parts.append(kmer if c is not None else kmer[:k - 1] + b"N")
            if c is not None:
                key = int(O.seq_keys([kmer], k, hb)[0])
                assert key not in pairs, "two k-mers of the test's genome share a key"
                pairs[key] = c
        reads.append(b"N".join(parts))
    text = fastq(reads)
    # counts of 2^31 go through the oracle's table, as the hard table's do; insert_counted puts the rest on top
    bigs = [(a, b) for a, b in pairs.items() if b >= 1 << 22]
    ctx, table = ctx_for(mk, qb, k, max_level_bits=3), dict(bigs)
    q = O.new(qb)
    for key, c in bigs:
        q.insert(key, c)
    ctx.import_blocks(q.blocks(), q.nelts(), q.ndistinct())
    q.free()
    QC.fill(ctx, table, [(a, b) for a, b in pairs.items() if 0 < b < 1 << 22])
    rs, rec, _, track = ask(ctx, text, *one_chunk(text), table, what="median")
    med = dict(zip(plans, (int(x) for x in rec["median"])))
    assert med == {"even": 2, "odd": 3, "half absent": 0, "all equal": 6, "all absent": 0, "one k-mer": 11, "top bit": 1 << 31,
                   "bit 0": 7, "top bit and bit 0": 1, "interleaved": 3}, med
    for name, r in zip(plans, rec):
        assert int(r["kmers"]) == sum(c is not None for c in plans[name]), name
    # without the flag the field is SHK_QUERY_NONE and everything else is unchanged
    _, rec2, _, track2 = ask(ctx, text, *one_chunk(text), table, median=False, what="no median")
    assert all(int(x) == NONE for x in rec2["median"]) and np.array_equal(track, track2)
    for f in REC_FIELDS:
        assert f == "median" or np.array_equal(rec[f], rec2[f]), f
    ctx.close()


def run_longest(mk, k=47, qb=14):
    """7. one read of 65535 bases with an N every ~700 among 100 short ones; 65536 bases are SHK_ERR_FASTQ"""
    rng = random.Random(5)
    g = FC.dna(3000, 71)
    long_read = bytearray((g * 22)[:65535])
    for p in range(350, 65535, 701):
        long_read[p] = ord("N")
    shorts = []
    for i in range(100):
        n = rng.randrange(30, 301)
        at = rng.randrange(0, len(g) - n)
        shorts.append(g[at:at + n])
    seqs = shorts[:50] + [bytes(long_read)] + shorts[50:]
    text = fastq(seqs)
    ctx = ctx_for(mk, qb, k, text_cap=1 << 18, max_level_bits=3)
    table = half_table(ctx, text, *one_chunk(text))
    rs, rec, ext, track = ask(ctx, text, *one_chunk(text), table, what="65535 bases")
    assert int(ext[50]["seq_len"]) == 65535 and int(rec[50]["kmers"]) > 50000 and int(rec[50]["max"]) > 0
    text = fastq(shorts[:3] + [bytes(long_read) + b"A"] + shorts[3:6])
    got = raw_query(ctx, text, *one_chunk(text), 64, 1 << 17, flags=1)
    assert got["rc"] == -6 and not got["rec"].view(np.uint8).any() and int((got["track"] != 0x55555555).sum()) == 0
    ctx.close()


def run_many(mk, nreads, k=31, qb=14):
    """8. more reads than one launch has lanes"""
    rng = random.Random(nreads)
    g = FC.dna(700, 81)
    seqs = []
    for i in range(nreads):
        at = rng.randrange(0, len(g) - 40)
        s = g[at:at + 40]
        seqs.append(s[:17] + b"N" + s[18:] if i % 97 == 5 else s)
    text = b"".join(b"@%d\n%s\n+\n%s\n" % (i, s, b"I" * 40) for i, s in enumerate(seqs))
    ctx = ctx_for(mk, qb, k, text_cap=len(text) + 64, max_batch_keys=nreads * 10 + 64, max_batch_reads=nreads + 8, max_level_bits=3)
    table = {}
    QC.fill(ctx, table, QC.half_of(cqflibs.oracle().seq_keys([g], k, ctx.cfg.hb)))
    rs, rec, _, _ = ask(ctx, text, *one_chunk(text), table, what="%d reads" % nreads)
    assert rs["reads"] == nreads and rs["kmers"] == 10 * nreads - 10 * len(range(5, nreads, 97))
    ctx.close()


def run_against_fasta(mk, k=31, qb=14):
    """9. per read the four sums shk_query_fasta answers for the same reads as two-line FASTA records"""
    rng = random.Random(19)
    g = FC.dna(5000, 91)
    seqs = []
    for i in range(2000):
        n = rng.randrange(100, 152)
        at = rng.randrange(0, len(g) - n)
        s = bytearray(g[at:at + n])
        if i % 100 == 7:
            s[rng.randrange(n)] = ord("N")
        seqs.append(bytes(s))
    fq = fastq(seqs)
    fa = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    ctx = ctx_for(mk, qb, k, text_cap=1 << 20, max_level_bits=3)
    table = {}
    QC.fill(ctx, table, QC.half_of(cqflibs.oracle().seq_keys([g], k, ctx.cfg.hb)))
    rs, rec, _, _ = ctx.query_reads(fq, *one_chunk(fq), min_count=3)
    qs, frec, _ = ctx.query_fasta(fa, first=True, min_count=3)
    assert len(frec) == 1 + len(seqs) and not frec[0].any() and len(rec) == len(seqs)
    for j, f in enumerate(("kmers", "present", "solid", "sum")):
        assert np.array_equal(rec[f].astype(np.uint64), frec[1:, j]), f
    assert {f: rs[f] for f in ("kmers", "present", "solid", "sum")} == {f: qs[f] for f in ("kmers", "present", "solid", "sum")}
    assert rs["present"] > 0 and rs["present"] < rs["kmers"]
    ctx.close()


def run_against_counting(mk, k=31, qb=13):
    """10. the first reader behind the counting call, against the table it built"""
    g = FC.dna(900, 33)
    rng = random.Random(3)
    seqs = [g[a:a + rng.randrange(k, 140)] for a in (rng.randrange(0, 700) for _ in range(150))]
    text = fastq(seqs, last_eol=False)
    cut = text.index(b"@r75 ")
    offs, lens = [0, cut], [cut, len(text) - cut]
    ctx = ctx_for(mk, qb, k, max_level_bits=3)
    st = ctx.count_chunks(text, offs, lens)
    rs, rec, _, _ = ctx.query_reads(text, offs, lens, median=True)
    assert rs["reads"] == len(seqs) and rs["kmers"] == st["kmers"] == sum(len(s) - k + 1 for s in seqs)
    assert np.array_equal(rec["present"], rec["kmers"]) and int(rec["min"].min()) >= 1 and int(rec["median"].min()) >= 1
    uniq, cnt = np.unique(all_keys(text, offs, lens, k, ctx.cfg.hb), return_counts=True)
    ask(ctx, text, offs, lens, {int(a): int(b) for a, b in zip(uniq, cnt)}, what="behind count_chunks")
    ctx.close()


def raw_query(ctx, text, chunk_off, chunk_len, rec_cap, track_cap, flags=0, min_count=2, on_device=False, text_bytes=None,
              with_track=True):
    """the C call itself with capacities of the caller's choosing"""
    import shk
    if on_device:
        ptr, n = C.c_void_p(int(text)), int(text_bytes)
    else:
        buf = (C.c_char * max(len(text), 1)).from_buffer_copy(bytes(text) or b"\0")
        ptr, n = C.cast(buf, C.c_void_p), len(text)
    rec = np.zeros(max(rec_cap, 1), dtype=shk._struct_dtype(shk.ReadRecord))
    ext = np.zeros(max(rec_cap, 1), dtype=shk._struct_dtype(shk.ReadExtent))
    track = np.full(max(track_cap, 1), 0x55555555, dtype=np.uint32)
    nreads, nwin, rs = C.c_uint64(0), C.c_uint64(0), shk.ReadsStats()
    rc = ctx.L.shk_query_reads(ctx.h, ptr, 1 if on_device else 0, n, ctx._tab(chunk_off), ctx._tab(chunk_len), len(chunk_off), min_count,
                               flags, C.c_void_p(rec.ctypes.data), rec_cap, 0, C.byref(nreads), C.c_void_p(ext.ctypes.data),
                               C.c_void_p(track.ctypes.data) if with_track else None, track_cap, 0, C.byref(nwin), C.byref(rs))
    return {"rc": rc, "nreads": nreads.value, "nwin": nwin.value, "rs": rs.as_dict(), "rec": rec, "ext": ext, "track": track}


def run_reader_contract(mk, k=31, qb=11):
    """11. the reader contract and the errors"""
    g = FC.dna(500, 5)
    reads = [g[a:a + 120] for a in range(0, 380, 20)]
    text = fastq([g[50:200], g[210:330][:60] + b"N" + g[271:330], FC.dna(120, 6), g[300:420]])
    ctx = ctx_for(mk, qb, k, max_level_bits=2)
    fq = fastq(reads)
    ctx.count_chunks(fq, *one_chunk(fq))
    uniq, cnt = np.unique(all_keys(fq, *one_chunk(fq), k, qb + 8), return_counts=True)
    table = {int(a): int(b) for a, b in zip(uniq, cnt)}
    first = ask(ctx, text, *one_chunk(text), table, what="directly behind count_chunks")
    assert first[0]["present"] > 0 and first[0]["solid"] > 0
    before, tb = ctx.blocks(), ctx.totals()
    ctx.lookup([int(x) for x in uniq[::3]], mode=1)
    marked = ctx.blocks()
    assert marked != before
    again = ask(ctx, text, *one_chunk(text), table, what="behind lookup(mode=1)")
    assert rows(again[1]) == rows(first[1]) and np.array_equal(again[3], first[3])
    assert ctx.blocks() == marked
    ta = ctx.totals()
    assert all(getattr(ta, f) == getattr(tb, f) for f, _ in ta._fields_)
    # rec_cap one too small: *nreads says how many, nothing is written, and the repeated call answers
    nr, nw = len(first[1]), len(first[3])
    got = raw_query(ctx, text, *one_chunk(text), nr - 1, nw, flags=1)
    assert (got["rc"], got["nreads"], got["nwin"]) == (-7, nr, nw)
    assert not got["rec"].view(np.uint8).any() and not got["ext"].view(np.uint8).any() and int((got["track"] != 0x55555555).sum()) == 0
    got = raw_query(ctx, text, *one_chunk(text), nr, nw - 1, flags=1)
    assert (got["rc"], got["nreads"], got["nwin"]) == (-7, nr, nw)
    assert not got["rec"].view(np.uint8).any() and int((got["track"] != 0x55555555).sum()) == 0
    got = raw_query(ctx, text, *one_chunk(text), nr, nw, flags=1)
    assert got["rc"] == 0 and rows(got["rec"]) == rows(first[1]) and np.array_equal(got["track"], first[3])
    # without a track its capacity does not matter; unknown flag bits, NULL chunk arrays, no chunks, too many
    assert raw_query(ctx, text, *one_chunk(text), nr, 0, with_track=False)["rc"] == 0
    assert raw_query(ctx, text, *one_chunk(text), nr, nw, flags=2)["rc"] == -1
    assert raw_query(ctx, text, [], [], nr, nw)["rc"] == -7
    assert raw_query(ctx, text, [0] * 4097, [0] * 4097, nr, nw)["rc"] == -7
    # a prepared, uncounted batch
    one = fastq([FC.dna(60, 1)])
    ctx.prepare_chunks(one, [0], [len(one)])
    assert raw_query(ctx, text, *one_chunk(text), nr, nw)["rc"] == -7
    ctx.count_prepared()
    ctx.close()
    # windows beyond max_batch_keys; text beyond max_batch_bytes; reads beyond max_batch_reads
    small = ctx_for(mk, qb, k, max_batch_keys=nw - 1, max_level_bits=2)
    assert raw_query(small, text, *one_chunk(text), nr, nw)["rc"] == -7
    small.close()
    small = ctx_for(mk, qb, k, text_cap=len(text) - 1, max_level_bits=2)
    assert raw_query(small, text, *one_chunk(text), nr, nw)["rc"] == -7
    small.close()
    small = ctx_for(mk, qb, k, max_batch_reads=nr - 1, max_level_bits=2)
    assert raw_query(small, text, *one_chunk(text), nr, nw)["rc"] == -7
    small.close()
    # a sharded context
    sh = mk(qb=12, k=k, max_batch_bytes=4096, max_batch_keys=4096, num_shards=2, shard_index=1)
    assert raw_query(sh, text, *one_chunk(text), nr, nw)["rc"] == -1
    sh.close()


# ---------------------------------------------------------------- command line
def cli_case():
    """(the reads file's text, the FASTA the table is built from, k, qb): 800 reads, a third from the table's genome, a
    third foreign, the rest half and half, some with an N, some shorter than k, CRLF in a few records"""
    rng = random.Random(44)
    own, foreign = FC.dna(1500, 45), FC.dna(1500, 46)
    recs = []
    for i in range(800):
        n = rng.randrange(20, 151)
        a, b = rng.randrange(0, 1500 - n), rng.randrange(0, 1500 - n)
        s = bytearray(own[a:a + n] if i % 3 == 0 else foreign[b:b + n] if i % 3 == 1 else own[a:a + n // 2] + foreign[b:b + n - n // 2])
        if i % 23 == 4:
            s[rng.randrange(n)] = ord("N")
        eol = b"\r\n" if i % 50 == 9 else b"\n"
        recs.append(b"@read_%d/1 lane=%d" % (i, i % 4) + eol + bytes(s) + eol + b"+" + eol + b"I" * n + eol)
    return b"".join(recs), b">own\n" + FC.wrap(own, 70), 31, 12


def cli_expected(fq, fa, k, qb, min_count, rules, min_kmers, keep_short, path):
    """(report, kept bytes, rejected bytes, table text, mask) python -m shk.reads must produce, from the model alone"""
    from shk.reads import format_report, select
    import shk
    uniq, cnt = np.unique(QC.text_keys(fa, k, qb + 8), return_counts=True)
    table = {int(a): int(b) for a, b in zip(uniq, cnt)}
    rs, rec, reads, _ = expect(fq, [0], [len(fq)], k, qb + 8, table, min_count, True)
    arr = np.zeros(len(rec), dtype=shk._struct_dtype(shk.ReadRecord))
    for j, f in enumerate(REC_FIELDS):
        arr[f] = [r[j] for r in rec]
    keep = select(arr, min_kmers=min_kmers, keep_short=keep_short, **rules)
    lines = fq.split(b"\n")
    assert lines[-1] == b""
    records = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]
    assert len(records) == len(rec)
    kept = b"".join(r for r, m in zip(records, keep) if m)
    rest = b"".join(r for r, m in zip(records, keep) if not m)
    tsv = "".join("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((r.split()[0][1:].decode(), e[1]) + t[1:] + t[:1])
                  for r, e, t in zip(records, reads, rec))
    return format_report(rs, int(keep.sum()), k, min_count, path, rules, min_kmers, keep_short), kept, rest, tsv, keep.astype(np.uint8)


def report_case():
    stats = {"reads": 1000, "kmers": 120000, "present": 90000, "solid": 60000, "sum": 987654}
    rules = {"min_solid": 0.5, "max_solid": None, "min_present": None, "max_present": 0.95, "min_median": 2, "max_median": None}
    want = ("reads\t1000\nkept\t250\t25.00%\nk-mers\t120000\nagainst\thost.cqf\npresent\t90000\t75.00%\ncount>=3\t60000\t50.00%\n"
            "rules\tmin-solid=0.5 max-present=0.95 min-median=2 min-kmers=10 keep-short\n")
    return stats, rules, want
