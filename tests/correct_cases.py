"""Cases for shk_correct_reads (include/shk.h), shared by the emulator and the GPU tests of tests/test_correct.py.

Expected values never come from the library: `correct` below is the header's rule in plain Python over a function that
says which windows of a sequence are solid. For the device cases that function is built from reads_cases.reads_of (the
reads), cqflibs.oracle().seq_keys (the keys) and a Python dict from hashed key to count that is filled next to the table
(Context.insert_counted) -- keyed by hashed key, so hash collisions are answered the way the filter answers them; for the
single-error property it is a set of canonical k-mer strings. All comparisons are exact."""
import ctypes as C
import random

import numpy as np

import cqflibs
import fasta_cases as FC
import query_cases as QC
import reads_cases as RC

SHORT, NONBASE, CAPPED = 1, 2, 4
REC_FIELDS = ("edits", "unfixable", "ambiguous", "flags")
STAT_FIELDS = ("reads", "candidates", "edited_reads", "edits", "unfixable", "ambiguous", "capped")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
BIG = 1 << 33      # a count above what a track entry or a 32-bit comparison could hold


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


# ---------------------------------------------------------------- the rule
class _State:
    def __init__(self, budget):
        self.budget, self.edits, self.unfixable, self.ambiguous, self.flags = budget, [], 0, 0, 0


def _forward(S, solid_of, k, check, st, back):
    """one pass over S (a bytearray of upper-case bases, edited in place); solid_of(seq) = [is window j of seq solid].
    back: S is the reverse complement of the read, and the edits are recorded in the read's coordinates and strand"""
    W = len(S) - k + 1
    sol = solid_of(bytes(S))
    prev = False
    for j in range(W):
        solid = sol[j]
        if not solid and prev:
            if st.budget == 0:
                st.flags |= CAPPED
            else:
                p = j + k - 1
                hi = min(j + check, W - 1)
                valid = []
                for b in b"ACGT":
                    if b == S[p]:
                        continue
                    T = bytes(S[j:p]) + bytes([b]) + bytes(S[p + 1:hi + k])
                    if all(solid_of(T)):
                        valid.append(b)
                if len(valid) == 1:
                    S[p] = valid[0]
                    b = bytes([valid[0]])
                    st.edits.append((len(S) - 1 - p, b"ACGT".index(b.translate(COMP))) if back else (p, b"ACGT".index(b)))
                    st.budget -= 1
                    solid = True
                    sol = solid_of(bytes(S))      # (only windows >= j have changed, and none of them has been judged)
                elif not valid:
                    st.unfixable += 1
                else:
                    st.ambiguous += 1
        prev = solid


def correct(seq, solid_of, k, check=4, max_edits=8):
    """the rule on one sequence line: ((edits, unfixable, ambiguous, flags), [(pos, code)] in the order made)"""
    if len(seq) < k:
        return (0, 0, 0, SHORT), []
    if any(b not in FC.BASES for b in seq):
        return (0, 0, 0, NONBASE), []
    assert len(seq) <= 65535
    st = _State(max_edits)
    S = bytearray(bytes(seq).upper())
    _forward(S, solid_of, k, check, st, False)
    R = bytearray(revcomp(S))
    _forward(R, solid_of, k, check, st, True)
    return (len(st.edits), st.unfixable, st.ambiguous, st.flags), st.edits


def corrected(seq, edits):
    """seq with the edits in it, case kept (the model's own apply_edits for one read)"""
    out = bytearray(seq)
    for p, code in edits:
        out[p] = b"ACGT"[code] | (out[p] & 0x20)
    return bytes(out)


def solid_by_strings(kmers, k):
    """solid_of over a set of canonical k-mer strings"""
    def solid_of(seq):
        out = []
        for j in range(len(seq) - k + 1):
            w = seq[j:j + k]
            out.append(min(w, revcomp(w)) in kmers)
        return out
    return solid_of


def canonical_kmers(g, k):
    return [min(g[j:j + k], revcomp(g[j:j + k])) for j in range(len(g) - k + 1)]


def solid_by_table(table, k, hb, min_count):
    """solid_of over the dict from hashed key to count"""
    O = cqflibs.oracle()

    def solid_of(seq):
        if len(seq) < k:
            return []
        return [table.get(int(x), 0) >= min_count for x in O.seq_keys([seq], k, hb)]
    return solid_of


def expect(text, chunk_off, chunk_len, k, hb, table, min_count, check, max_edits):
    """(cstats, records as rows of REC_FIELDS, extents, the edit list of every read) the call must answer"""
    reads = RC.reads_of(text, chunk_off, chunk_len)
    solid_of = solid_by_table(table, k, hb, min_count)
    rec, eds = [], []
    for o, n, _ in reads:
        r, e = correct(text[o:o + n], solid_of, k, check, max_edits)
        rec.append(r)
        eds.append(e)
    cand = [r for r in rec if not r[3] & (SHORT | NONBASE)]
    cs = {"reads": len(reads), "candidates": len(cand), "edited_reads": sum(r[0] != 0 for r in cand), "edits": sum(r[0] for r in cand),
          "unfixable": sum(r[1] for r in cand), "ambiguous": sum(r[2] for r in cand), "capped": sum((r[3] & CAPPED) != 0 for r in cand)}
    return cs, rec, reads, eds


def model_text(text, reads, eds):
    """the text with the model's edits in it"""
    out = bytearray(text)
    for (o, n, _), e in zip(reads, eds):
        out[o:o + n] = corrected(text[o:o + n], e)
    return bytes(out)


def rows(rec):
    return [tuple(int(r[f]) for f in REC_FIELDS) for r in rec]


def edit_lists(rec, edits):
    return [[(int(w) & 0xFFFF, int(w) >> 16) for w in row[:int(r["edits"])]] for r, row in zip(rec, edits)]


def ask(ctx, text, chunk_off, chunk_len, table, min_count=2, check=4, max_edits=8, what="", **kw):
    """one call against the model's answer; returns (what the call answered, the model's answer)"""
    want = expect(text, chunk_off, chunk_len, ctx.cfg.k, ctx.cfg.hb, table, min_count, check, max_edits)
    cs, rec, ext, edits = ctx.correct_reads(kw.pop("call_text", text), chunk_off, chunk_len, min_count=min_count, check=check,
                                            max_edits=max_edits, want_extents=True, **kw)
    got = rows(rec)
    assert len(got) == len(want[1]), (what, len(got), len(want[1]))
    bad = [i for i, (a, b) in enumerate(zip(got, want[1])) if a != b]
    assert not bad, (what, "read %d" % bad[0], dict(zip(REC_FIELDS, got[bad[0]])), dict(zip(REC_FIELDS, want[1][bad[0]])))
    assert edits.shape == (len(got), max_edits) and edits.dtype == np.uint32
    lists = edit_lists(rec, edits)
    bad = [i for i, (a, b) in enumerate(zip(lists, want[3])) if a != b]
    assert not bad, (what, "edits of read %d" % bad[0], lists[bad[0]], want[3][bad[0]])
    assert cs == want[0], (what, cs, want[0])
    assert [tuple(int(x) for x in e) for e in ext.tolist()] == want[2], what
    return (cs, rec, ext, edits), want


# ---------------------------------------------------------------- tables and texts
def graded_table(ctx, g, s):
    """the k-mers of g in the table, their counts 1, s - 1, s, 5 and BIG spread over them: one in six is weak"""
    keys = sorted(set(int(x) for x in cqflibs.oracle().seq_keys([g], ctx.cfg.k, ctx.cfg.hb)))
    plan = [s, 5, BIG, s, 5, 1, s, 5, s, 5, s - 1, s]
    pairs = [(key, plan[i % len(plan)]) for i, key in enumerate(keys)]
    return fill_table(ctx, pairs)


def fill_table(ctx, pairs):
    """(key, count) pairs into the table and its dict; counts of 2^22 and more go in through the oracle's table"""
    bigs = [(a, b) for a, b in pairs if b >= 1 << 22]
    table = dict(bigs)
    if bigs:
        q = cqflibs.oracle().new(ctx.cfg.qb)
        for key, c in bigs:
            q.insert(key, c)
        ctx.import_blocks(q.blocks(), q.nelts(), q.ndistinct())
        q.free()
    QC.fill(ctx, table, [(a, b) for a, b in pairs if 0 < b < 1 << 22])
    return table


def flat_table(ctx, seqs, count=3):
    """every k-mer of the sequences, `count` times"""
    keys = sorted(set(int(x) for x in cqflibs.oracle().seq_keys(list(seqs), ctx.cfg.k, ctx.cfg.hb)))
    table = {}
    QC.fill(ctx, table, [(key, count) for key in keys])
    return table


def sub(s, p, rng=None, to=None):
    """s with another base at p (the next one in ACGT, or a drawn one); case kept"""
    s = bytearray(s)
    at = b"ACGT".index(bytes([s[p] & 0xDF]))
    new = b"ACGT"[(at + (rng.randrange(1, 4) if rng else 1)) % 4] if to is None else to
    s[p] = new | (s[p] & 0x20)
    return bytes(s)


def shape_reads(k, check, seed):
    """the issue's list on one genome: lengths, one error at each listed position, two errors, the reverse strand, lower
    and mixed case, reads that are left alone"""
    rng = random.Random(seed)
    g = FC.dna(1500, seed)

    def piece(n):
        at = rng.randrange(0, len(g) - n)
        return g[at:at + n]
    lens = sorted(set(n for n in (k - 1, k, k + 1, 2 * k - 1, 2 * k, 63, 64, 65, 127, 128, 129, 200, 2 * k + 3) if n >= 0))
    seqs = []
    for n in lens:
        s = piece(n)
        seqs.append(s)
        spots = sorted(set(p for p in (0, 1, k - 2, k - 1, k, 15, 16, 63, 64, n - k - 1, n - k, n - 1) if 0 <= p < n))
        if n >= k:
            seqs += [sub(s, p) for p in spots]
    n = max(3 * k + 2 * check + 8, 200) if 3 * k + 2 * check + 8 <= 1400 else 1400
    a = k + 3
    for gap in (check, check + 1, k):
        if a + gap < n:
            seqs.append(sub(sub(piece(n), a), a + gap))
    seqs.append(sub(sub(piece(n), max(k - 3, 0)), n - max(k - 3, 0) - 1))      # one in the head, one in the tail
    for p in (k + 5, n - k - 7, n // 2):
        seqs.append(revcomp(sub(piece(n), p % n)))
    seqs.append(sub(piece(n), n // 2).lower())
    mixed = bytearray(sub(piece(n), n // 3))
    mixed[::3] = bytes(mixed[::3]).lower()
    seqs.append(bytes(mixed))
    for j, bad in enumerate((b"N", b"n", b"R")):
        s = bytearray(sub(piece(n), n // 2))
        s[(5 + 37 * j) % n:(5 + 37 * j) % n + 1] = bad
        seqs.append(bytes(s))
    seqs.append(b"")
    return g, seqs


def run_shapes(mk, k, qb=12, s=3):
    """2. shapes of a read; check and min_count at their listed values; a CRLF file"""
    g, seqs = shape_reads(k, 4, 500 + k)
    text = RC.fastq(seqs)
    ctx = RC.ctx_for(mk, qb, k, text_cap=1 << 18, max_level_bits=3)
    table = graded_table(ctx, g, s)
    (cs, rec, _, _), _ = ask(ctx, text, *RC.one_chunk(text), table, min_count=s, what="k=%d" % k)
    # (the case must have all outcomes in it: the weak k-mers of the genome itself make many suspects unfixable, and at
    # k = 5 a suspect often has several valid bases)
    assert cs["edited_reads"] > cs["candidates"] // 4 and cs["unfixable"] > 0 and cs["candidates"] < cs["reads"]
    assert cs["ambiguous"] > 100 if k == 5 else cs["edits"] < 2 * cs["edited_reads"]
    flags = [int(r["flags"]) for r in rec]
    assert flags[-1] == SHORT and flags[-4:-1] == [NONBASE] * 3
    for check in sorted(set((0, 1, min(k - 1, 255), 255))):
        _, seqs_c = shape_reads(k, check, 500 + k)
        text_c = RC.fastq(seqs_c)
        ask(ctx, text_c, *RC.one_chunk(text_c), table, min_count=s, check=check, what="k=%d check=%d" % (k, check))
    for m in (1, s + 1):
        ask(ctx, text, *RC.one_chunk(text), table, min_count=m, what="k=%d min_count=%d" % (k, m))
    crlf = RC.fastq(seqs[:40], eol=b"\r\n")
    (cs, rec, _, _), _ = ask(ctx, crlf, *RC.one_chunk(crlf), table, min_count=s, what="k=%d CRLF" % k)
    assert cs["candidates"] == 0 and all(int(r["flags"]) in (NONBASE, SHORT) for r in rec)      # (the '\r' is no base)
    ctx.close()


def _one(ctx, seq, table, what, **kw):
    text = RC.fastq([seq])
    (cs, rec, _, edits), want = ask(ctx, text, *RC.one_chunk(text), table, what=what, **kw)
    return rows(rec)[0], edit_lists(rec, edits)[0]


def run_constructed(mk, k=21, qb=12, check=4):
    """3. reads built for one outcome each"""
    g = FC.dna(600, 77)
    read = g[100:190]
    code = lambda s, p: b"ACGT".index(s[p:p + 1])      # noqa: E731
    # ambiguous: the suspect in the tail (only the forward pass meets it), both other bases solid in every window
    ctx = RC.ctx_for(mk, qb, k, max_level_bits=3)
    p = len(read) - 6
    bad = sub(read, p)
    other = sub(bad, p)
    assert len({read[p], bad[p], other[p]}) == 3
    table = flat_table(ctx, [g, other[p - k + 1:]])
    got = _one(ctx, bad, table, "ambiguous", check=check)
    assert got == ((0, 0, 1, 0), []), got
    ctx.close()
    ctx = RC.ctx_for(mk, qb, k, max_level_bits=3)
    table = flat_table(ctx, [g])
    # unfixable: two errors inside check + 1 windows -- the forward pass meets the left one, the backward pass the right one
    got = _one(ctx, sub(sub(read, 40), 40 + check), table, "unfixable", check=check)
    assert got == ((0, 2, 0, 0), []), got
    # ... one base further apart both are repaired, by the forward pass
    got = _one(ctx, sub(sub(read, 40), 40 + check + 1), table, "check + 1 apart", check=check)
    assert got[0] == (2, 0, 0, 0) and sorted(got[1]) == [(40, code(read, 40)), (40 + check + 1, code(read, 40 + check + 1))], got
    # capped: three errors far apart, two edits allowed; the third suspect is met from both sides
    three = sub(sub(sub(read, 25), 50), 75)
    got = _one(ctx, three, table, "capped", check=check, max_edits=2)
    assert got == ((2, 0, 0, CAPPED), [(25, code(read, 25)), (50, code(read, 50))]), got
    got = _one(ctx, three, table, "not capped", check=check, max_edits=3)
    assert got == ((3, 0, 0, 0), [(25, code(read, 25)), (50, code(read, 50)), (75, code(read, 75))]), got
    # the last window is the suspect: nothing lies behind it, check shrinks to 0
    got = _one(ctx, sub(read, len(read) - 1), table, "last window", check=check)
    assert got == ((1, 0, 0, 0), [(len(read) - 1, code(read, len(read) - 1))]), got
    # ... and the first base is met by the backward pass alone
    got = _one(ctx, sub(read, 0), table, "first base", check=check)
    assert got == ((1, 0, 0, 0), [(0, code(read, 0))]), got
    ctx.close()
    # a position edited by both passes: two genomes that differ at one base, p. Of the first the table holds the windows
    # that end at p .. p + check (what the forward pass looks at), of the second those that begin at p - check .. p (what the
    # backward pass looks at), of both everything that does not hold p. The read has a third base there: the forward
    # pass writes the first genome's base, the backward pass finds the window that begins at p weak and writes the second's.
    # Each pass then runs out of the windows it was given and meets one suspect it cannot repair.
    p = 45
    one, two = read, sub(read, p)
    bad = sub(two, p)
    ctx = RC.ctx_for(mk, qb, k, max_level_bits=3)
    table = flat_table(ctx, [read[:p], read[p + 1:], one[p - k + 1:p + check + 1], two[p - check:p + k]])
    got = _one(ctx, bad, table, "both passes", check=check)
    assert got == ((2, 2, 0, 0), [(p, code(one, p)), (p, code(two, p))]), got
    ctx.close()


def batch_text(k, nreads, seed, every=3):
    """reads of mixed lengths from one genome, an error or two in every third; (genome, reads)"""
    rng = random.Random(seed)
    g = FC.dna(2500, seed)
    seqs = []
    for i in range(nreads):
        n = rng.randrange(k - 2, 3 * k + 40)
        at = rng.randrange(0, len(g) - n)
        s = g[at:at + n]
        if i % every == 1 and n:
            s = sub(s, rng.randrange(n), rng)
            if i % 2 and n > k:
                s = sub(s, rng.randrange(n), rng)
        if i % 41 == 7 and n:
            s = s[:n // 2] + b"N" + s[n // 2 + 1:]
        seqs.append(revcomp(s) if i % 5 == 0 and b"N" not in s else s)
    return g, seqs


def run_batch(mk, dev_bytes, k=21, qb=14):
    """4. 600 reads in one call, lanes with and without suspects side by side; chunk tables; device text"""
    g, seqs = batch_text(k, 600, 13)
    recs = [RC.fastq([s]).replace(b"@r0 ", b"@r%d " % i) for i, s in enumerate(seqs)]
    text = b"".join(recs)
    ctx = RC.ctx_for(mk, qb, k, text_cap=1 << 17, max_level_bits=3)
    table = flat_table(ctx, [g])
    (cs, rec, _, _), _ = ask(ctx, text, *RC.one_chunk(text), table, min_count=2, what="600 reads")
    assert cs["reads"] == 600 and cs["edited_reads"] > 100 and cs["candidates"] < 600
    # chunks in reverse order, with a gap, an empty chunk and one shorter than 16 bytes
    bounds = np.cumsum([0] + [len(r) for r in recs]).tolist()
    offs, lens = [], []
    for a in range(0, 560, 45):
        offs.append(bounds[a])
        lens.append(bounds[a + 40] - bounds[a])
    offs, lens = offs[::-1], lens[::-1]
    offs[3:3] = [bounds[7]]
    lens[3:3] = [0]
    offs.append(bounds[599])
    lens.append(9)
    (cs2, _, ext, _), _ = ask(ctx, text, offs, lens, table, what="chunks")
    assert cs2["reads"] == 40 * len(range(0, 560, 45)) and [int(e["chunk"]) for e in ext] == sorted(int(e["chunk"]) for e in ext)
    # device text answers as host text does, and is not written
    ptr, keep = dev_bytes(b"\n" * 16 + text)
    before = snapshot(keep)
    ask(ctx, text, offs, lens, table, what="device text", call_text=ptr + 16, on_device=True, text_bytes=len(text))
    assert snapshot(keep) == before
    ctx.close()


def snapshot(keep):
    """the bytes of what a dev_bytes factory handed out (a ctypes buffer, or a tensor on the device)"""
    return keep.cpu().numpy().tobytes() if hasattr(keep, "cpu") else bytes(keep)


def error_text(k, nreads, seed, rate=0.01):
    rng = random.Random(seed)
    g = FC.dna(3000, seed)
    seqs = []
    for _ in range(nreads):
        n = rng.randrange(2 * k, 4 * k)
        at = rng.randrange(0, len(g) - n)
        s = g[at:at + n]
        for p in range(n):
            if rng.random() < rate:
                s = sub(s, p, rng)
        seqs.append(s)
    return g, seqs


def run_reader_contract(mk, dev_bytes, k=21, qb=14):
    """5. the reader contract: the table, later calls, and what the edits do to the reads"""
    g, seqs = error_text(k, 200, 23, rate=0.02)
    text = RC.fastq(seqs)
    more = RC.fastq([g[i:i + 90] for i in range(0, 900, 30)])
    ctx, twin = (RC.ctx_for(mk, qb, k, max_level_bits=3) for _ in range(2))
    table = flat_table(ctx, [g])
    flat_table(twin, [g])
    ctx.lookup(sorted(table)[::3], mode=1)       # traveled bits the call must neither read nor touch
    twin.lookup(sorted(table)[::3], mode=1)
    before, tb = ctx.blocks(), ctx.totals()
    (cs, rec, ext, edits), want = ask(ctx, text, *RC.one_chunk(text), table, what="contract")
    assert cs["edits"] > 50
    assert ctx.blocks() == before == twin.blocks()
    ta = ctx.totals()
    assert all(getattr(ta, f) == getattr(tb, f) for f, _ in ta._fields_)
    # the readers and the counting call behind it answer what they answer without it
    a, b = ctx.query_reads(text, *RC.one_chunk(text), median=True, want_track=True), twin.query_reads(text, *RC.one_chunk(text), median=True, want_track=True)
    assert a[0] == b[0] and RC.rows(a[1]) == RC.rows(b[1]) and np.array_equal(a[3], b[3])
    # the corrected text is at least as solid, read by read
    from shk.correct import apply_edits
    fixed = apply_edits(text, ext, rec, edits)
    assert fixed == model_text(text, want[2], want[3]) and fixed != text
    again = ctx.query_reads(fixed, *RC.one_chunk(fixed))
    assert len(again[1]) == len(a[1]) and bool((again[1]["solid"] >= a[1]["solid"]).all())
    assert int(again[1]["solid"].sum()) > int(a[1]["solid"].sum())
    assert ctx.count_chunks(more, *RC.one_chunk(more)) == twin.count_chunks(more, *RC.one_chunk(more))
    assert ctx.blocks() == twin.blocks()
    ctx.close()
    twin.close()


def raw_correct(ctx, text, chunk_off, chunk_len, rec_cap, min_count=2, check=4, max_edits=8, on_device=False, text_bytes=None,
                null=()):
    """the C call itself with capacities and NULLs of the caller's choosing; the arrays start as 0x55 bytes"""
    import shk
    if on_device:
        ptr, n = C.c_void_p(int(text)), int(text_bytes)
    else:
        buf = (C.c_char * max(len(text), 1)).from_buffer_copy(bytes(text) or b"\0")
        ptr, n = C.cast(buf, C.c_void_p), len(text)
    rec = np.full(max(rec_cap, 1) * 16, 0x55, dtype=np.uint8)
    ext = np.full(max(rec_cap, 1) * 16, 0x55, dtype=np.uint8)
    edits = np.full(max(rec_cap, 1) * 16 * 4, 0x55, dtype=np.uint8)
    nreads, cs = C.c_uint64(0), shk.CorrectStats()
    rc = ctx.L.shk_correct_reads(ctx.h, ptr, 1 if on_device else 0, n,
                                 None if "chunk_off" in null else ctx._tab(chunk_off), None if "chunk_len" in null else ctx._tab(chunk_len),
                                 len(chunk_off), min_count, check, max_edits, None if "rec" in null else C.c_void_p(rec.ctypes.data), rec_cap, 0,
                                 None if "nreads" in null else C.byref(nreads), C.c_void_p(ext.ctypes.data),
                                 None if "edits" in null else C.c_void_p(edits.ctypes.data), 0, C.byref(cs))
    untouched = bool((rec == 0x55).all() and (ext == 0x55).all() and (edits == 0x55).all())
    return {"rc": rc, "nreads": nreads.value, "untouched": untouched, "cs": cs.as_dict(),
            "rec": rec.view(shk._struct_dtype(shk.CorrectRecord)), "edits": edits.view(np.uint32)}


def run_errors(mk, dev_bytes, k=21, qb=14):
    """6. every error of the header, each leaving rec, ext and edits as they were"""
    g, seqs = error_text(k, 200, 29)
    text = RC.fastq(seqs)
    assert len(text) < 1 << 16
    one = RC.one_chunk(text)
    ctx = RC.ctx_for(mk, qb, k, text_cap=1 << 18, max_level_bits=3)
    table = flat_table(ctx, [g])
    (_, rec, _, edits), _ = ask(ctx, text, *one, table, what="errors: the call itself")
    nr = len(rec)

    def fails(code, what, *a, **kw):
        got = raw_correct(*a, **kw)
        assert got["rc"] == code and got["untouched"], (what, got["rc"])
        return got
    ok = raw_correct(ctx, text, *one, nr)
    assert ok["rc"] == 0 and ok["nreads"] == nr and rows(ok["rec"][:nr]) == rows(rec)
    assert edit_lists(ok["rec"][:nr], ok["edits"][:nr * 8].reshape(nr, 8)) == edit_lists(rec, edits)
    # SHK_ERR_ARG
    for name in ("rec", "edits", "nreads", "chunk_off", "chunk_len"):
        fails(-1, "NULL " + name, ctx, text, *one, nr, null=(name,))
    fails(-1, "min_count 0", ctx, text, *one, nr, min_count=0)
    fails(-1, "check 256", ctx, text, *one, nr, check=256)
    fails(-1, "max_edits 0", ctx, text, *one, nr, max_edits=0)
    fails(-1, "max_edits 17", ctx, text, *one, nr, max_edits=17)
    assert raw_correct(ctx, text, *one, nr, check=255, max_edits=16)["rc"] == 0
    ptr, keep = dev_bytes(b"\n" * 16 + text)
    fails(-1, "unaligned device text", ctx, ptr + 17, [0], [len(text) - 1], nr, on_device=True, text_bytes=len(text) - 1)
    sh = mk(qb=12, k=k, max_batch_bytes=1 << 16, max_batch_keys=1 << 16, num_shards=2, shard_index=1)
    fails(-1, "sharded", sh, text, *one, nr)
    sh.close()
    # SHK_ERR_BATCH
    got = fails(-7, "rec_cap", ctx, text, *one, nr - 1)
    assert got["nreads"] == nr      # ... says how many, and the repeated call answers
    fails(-7, "no chunks", ctx, text, [], [], nr)
    fails(-7, "4097 chunks", ctx, text, [0] * 4097, [0] * 4097, nr)
    tiny = RC.fastq([FC.dna(60, 1)])
    ctx.prepare_chunks(tiny, [0], [len(tiny)])
    fails(-7, "a prepared batch", ctx, text, *one, nr)
    ctx.count_prepared()
    # SHK_ERR_FASTQ
    long_text = RC.fastq(seqs[:3] + [(g * 22)[:65536]] + seqs[3:6])
    fails(-6, "65536 bases", ctx, long_text, *RC.one_chunk(long_text), 64)
    long_text = RC.fastq(seqs[:3] + [(g * 22)[:65535]] + seqs[3:6])
    assert raw_correct(ctx, long_text, *RC.one_chunk(long_text), 64)["rc"] == 0
    ctx.close()
    small = RC.ctx_for(mk, qb, k, text_cap=len(text) - 1, max_level_bits=3)
    fails(-7, "text beyond max_batch_bytes", small, text, *one, nr)
    small.close()
    small = RC.ctx_for(mk, qb, k, max_batch_reads=nr - 1, max_level_bits=3)
    fails(-7, "reads beyond max_batch_reads", small, text, *one, nr)
    small.close()
    keys = 2 * (len(text) // 64 + nr + 1)      # one unit short of what pack_stage asks for
    small = RC.ctx_for(mk, qb, k, max_batch_keys=keys, max_level_bits=3)
    fails(-7, "the units do not fit", small, text, *one, nr)
    small.close()
    small = RC.ctx_for(mk, qb, k, max_batch_keys=keys + 4, max_level_bits=3)
    assert raw_correct(small, text, *one, nr)["rc"] == 0
    small.close()


# ---------------------------------------------------------------- the single-error property (no library)
def unique_genome(n, k, seed):
    """a random genome in which no canonical k-mer repeats"""
    while True:
        g = FC.dna(n, seed)
        if len(set(canonical_kmers(g, k))) == n - k + 1:
            return g
        seed += 1000


def single_error_cases(k, genome, length, nreads, seed):
    """every read of both strands with one substitution at every position: (original, erroneous, position)"""
    rng = random.Random(seed)
    g = unique_genome(genome, k, seed)
    for i in range(nreads):
        at = rng.randrange(0, len(g) - length)
        s = g[at:at + length]
        if i % 2:
            s = revcomp(s)
        for p in range(length):
            yield g, s, sub(s, p, rng), p


# ---------------------------------------------------------------- command line
def cli_case():
    """(two FASTQ texts, the FASTA the table is built from, k, qb): reads of one genome with 1 % errors, some with an N,
    some shorter than k, some lower case, CRLF in a few records"""
    rng = random.Random(52)
    own = FC.dna(3000, 53)
    k = 21
    recs = []
    for i in range(1100):
        n = rng.randrange(15, 151)
        a = rng.randrange(0, len(own) - n)
        s = own[a:a + n]
        for p in range(n):
            if rng.random() < 0.01:
                s = sub(s, p, rng)
        if i % 23 == 4:
            s = s[:n // 2] + b"N" + s[n // 2 + 1:]
        if i % 11 == 3:
            s = s.lower()
        if i % 4 == 1:
            s = revcomp(s) if b"N" not in s and s.isupper() else s
        eol = b"\r\n" if i % 50 == 9 else b"\n"
        recs.append(b"@read_%d/1 lane=%d" % (i, i % 4) + eol + s + eol + b"+" + eol + b"I" * n + eol)
    return b"".join(recs[:800]), b"".join(recs[800:]),b">own\n" + FC.wrap(own, 70) + b">own again\n" + FC.wrap(own, 70), k, 14


def cli_expected(fq, fa, k, qb, min_count, check, max_edits, path):
    """(report, corrected text, table text, edits text) python -m shk.correct must produce, from the model alone"""
    from shk.correct import format_report
    uniq, cnt = np.unique(QC.text_keys(fa, k, qb + 8), return_counts=True)
    table = {int(a): int(b) for a, b in zip(uniq, cnt)}
    cs, rec, reads, eds = expect(fq, [0], [len(fq)], k, qb + 8, table, min_count, check, max_edits)
    lines = fq.split(b"\n")
    names = [lines[i].split()[0][1:].decode() for i in range(0, len(lines) - 1, 4)]
    assert len(names) == len(rec)
    tsv = "".join("%s\t%d\t%d\t%d\t%d\t%d\n" % ((nm, e[1]) + r) for nm, e, r in zip(names, reads, rec))
    log = []
    for nm, (o, n, _), e in zip(names, reads, eds):
        seq = bytearray(fq[o:o + n])
        for p, code in e:
            new = b"ACGT"[code] | (seq[p] & 0x20)
            log.append("%s\t%d\t%c\t%c\n" % (nm, p, seq[p], new))
            seq[p] = new
    return format_report(cs, k, min_count, check, max_edits, path), model_text(fq, reads, eds), tsv, "".join(log)
