"""FASTQ text shapes at the edges of the device front end (k_count_lines, k_emit_reads, k_count_keys, k_pack_reads, the
roll kernels, k_hash_reads), shared by the emulator tests and the GPU tests of tests/test_text_shapes.py and by the
oracle-vs-reference comparison of tests/test_oracle.py. The texts are built here with seeded `random`: reads up to the
65535 bases the library accepts, 'N's at the indices where the restart rule turns, neighbours of the sequence line that
look like bases, newlines and record starts, broken line structure, and chunk tables that do not tile the text.

A context factory `mk_ctx(**kw)` returns a shk.Context with two additions:
  ctx.read_words(dp, n)          -> list of the n key words at device pointer dp
  ctx.dev_text(data, offset=0)   -> pointer to a copy of `data` in memory the kernels may read as device text, `offset`
                                    bytes behind a 16-byte boundary, in an allocation that ends at the next multiple of 16
                                    behind the text (include/shk.h: what a caller must provide, and not a byte more --
                                    under AddressSanitizer the emulator build reports any read behind it)
"""
import contextlib
import os
import random

import cqflibs
from fastq_util import oracle_header, oracle_t1

ERR_ARG, ERR_FASTQ, ERR_BATCH = -1, -6, -7
MAX_CHUNKS = 4096
MAX_READ = 65535
LONG = [518, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 65471, 65472, 65473, 65534, 65535]


class Text:
    """one FASTQ text with its chunk table and the geometry it is counted at"""

    def __init__(self, name, k, qb, fq, offs, lens):
        self.name, self.k, self.qb, self.fq, self.offs, self.lens = name, k, qb, bytes(fq), list(offs), list(lens)
        self._exp = None

    def chunks(self):
        return [self.fq[a:a + n] for a, n in zip(self.offs, self.lens)]

    def ref_safe(self):
        """the reference's reads_to_kmers walks four memchr's per record without testing their result (CQF_mt.h:616-620,
        723-726): it only survives chunks made of whole groups of four lines"""
        return all(c.count(b"\n") % 4 == 0 and (not c or c.endswith(b"\n")) for c in self.chunks())

    def expected(self):
        """(key words in stream order, table bytes, header, nelts, ndistinct) by the oracle; computed once"""
        if self._exp is None:
            O = cqflibs.oracle()
            hb = self.qb + 8
            words = []
            for ci, c in enumerate(self.chunks()):
                words += [kk | (ci << hb) for kk in O.chunk_keys(c, self.k, hb)]
            q, _, _ = oracle_t1(self.fq, self.offs, self.lens, self.k, self.qb)
            assert not q.full(), self.name
            self._exp = (words, q.blocks(), oracle_header(q), q.nelts(), q.ndistinct())
            assert q.nelts() == len(words), self.name
            assert q.ndistinct() <= 0.5 * (1 << self.qb), (self.name, q.ndistinct())
            q.free()
        return self._exp


def _bases(rnd, n):
    return bytearray(rnd.choices(b"ACGT", k=n))


def _tile(recs, per):
    """chunk table over records laid end to end, `per` records per chunk"""
    offs, lens, pos = [], [], 0
    for i in range(0, len(recs), per):
        n = sum(len(r) for r in recs[i:i + per])
        offs.append(pos)
        lens.append(n)
        pos += n
    return offs, lens


def _rec(i, seq, qual=None, head=None, plus=b"+"):
    return (head if head is not None else b"@r%d" % i) + b"\n" + bytes(seq) + b"\n" + plus + b"\n" + \
        (qual if qual is not None else b"I" * len(seq)) + b"\n"


# ---------------------------------------------------------------------------------------------------- 1. long reads
def long_read_texts():
    """reads of 518 .. 65535 bases (up to 1024 of k_pack_reads' 64-base units; the wave-per-read kernel behind its
    256-base fast path; thousands of 16-byte units in k_count_keys) among ~100 reads of 30 .. 300, shuffled, 5 records
    per chunk. Variants: plain; an 'N' every ~700 bases (many restarts behind base 256); 'N' at k-1, k, len-k-1, len-k,
    len-1; a lower-case stretch and IUPAC bytes inside the 65535-base read."""
    out = []
    for k in (21, 47, 64, 65, 191):
        full = k == 47
        lens_ = LONG if full else [L for L in LONG if L <= 16385] + [65535]
        for vi, variant in enumerate(("plain", "n700", "nedges", "lower_iupac")):
            rnd = random.Random(10 * k + vi)
            reads = [_bases(rnd, L) for L in lens_] + [_bases(rnd, rnd.randrange(30, 301)) for _ in range(100)]
            for s in reads[:len(lens_)]:
                L = len(s)
                if variant == "n700":
                    for j, p in enumerate(range(350, L, 700)):
                        s[min(L - 1, p + j % 7)] = ord("N")
                elif variant == "nedges":
                    for p in (k - 1, k, L - k - 1, L - k, L - 1):
                        s[p] = ord("N")
                elif variant == "lower_iupac" and L == 65535:
                    s[30000:30400] = bytes(s[30000:30400]).lower()
                    for p, c in zip((3, 255, 256, 257, 4096, 40000, 65000, L - k - 1, L - 2), b"RYKSWDMnB"):
                        s[p] = c
            if variant == "nedges":
                # around the 256 bases the wave-per-read kernel holds in registers: an 'N' at the last index it sees there,
                # at the first it does not, and at the read's end
                for L in (255, 256, 257, 258, 320):
                    s = _bases(rnd, L)
                    for p in (255, 256, L - 1):
                        if k <= p < L:
                            s[p] = ord("N")
                    reads.append(s)
            recs = [_rec(i, s) for i, s in enumerate(reads)]
            rnd.shuffle(recs)
            offs, lens = _tile(recs, 5)
            out.append(Text("long-k%d-%s" % (k, variant), k, 20 if full else 19, b"".join(recs), offs, lens))
    return out


# ---------------------------------------------------------------------------------------------------- 2. 65535 / 65536
def too_long_batches(bad_len):
    """(k, qb, first batch, batch with one read of bad_len bases, the same with that read cut to 65535 bases)"""
    k, qb = 47, 18
    rnd = random.Random(bad_len)
    first = [_rec(i, _bases(rnd, rnd.randrange(40, 200))) for i in range(40)]
    reads = [_bases(rnd, rnd.randrange(30, 301)) for _ in range(30)]
    reads.insert(17, _bases(rnd, bad_len))
    bad = [_rec(100 + i, s) for i, s in enumerate(reads)]
    reads[17] = reads[17][:MAX_READ]
    good = [_rec(100 + i, s) for i, s in enumerate(reads)]
    mk = lambda name, recs: Text(name, k, qb, b"".join(recs), *_tile(recs, 5))      # noqa: E731
    return k, qb, mk("first", first), mk("bad-%d" % bad_len, bad), mk("cut-%d" % bad_len, good)


# ---------------------------------------------------------------------------------------------------- 3. neighbours
NEIGHBOURS = ("I", "qualN", "qualAt", "qualPlusAt", "qualSelf", "headNNNN", "plusHeadN")


def neighbour_texts(k):
    """{pattern: Text}: the same reads with the same 'N's, every line next to the sequence line filled with what the
    front end looks for elsewhere -- 'N' (k_count_keys' 16-byte SWAR search masked to [st + k, en)), '@' and '+', bases
    (the packer's and the roll kernels' 16-byte fetches reach into the neighbouring lines). Read lengths k, k+1, k+15,
    k+16, k+17 and 150; headers are padded so that the reads start on every residue mod 16, with every length."""
    rnd = random.Random(300 + k)
    reads = []
    for j in range(96):
        L = (k, k + 1, k + 15, k + 16, k + 17, 150)[j // 16]
        s = _bases(rnd, L)
        if j % 3 == 1:
            s[min(k, L - 1)] = ord("N")        # at index k: a restart right behind the un-inspected first window
        elif j % 3 == 2:
            s[L - 1] = ord("N")
        reads.append(s)
    out = {}
    for pat in NEIGHBOURS:
        recs, pos, residues = [], 0, set()
        for j, s in enumerate(reads):
            L = len(s)
            tail = b"NNNN" if pat in ("headNNNN", "plusHeadN") else b""
            head = b"@r%d" % j
            head += b"x" * ((j % 16 - (pos + len(head) + len(tail) + 1)) % 16) + tail
            qual = {"qualN": b"N" * L, "qualAt": b"@" * L, "qualPlusAt": (b"+@" if j % 2 else b"@+") + b"I" * (L - 2),
                    "qualSelf": bytes(s)}.get(pat, b"I" * L)
            r = _rec(j, s, qual, head, b"+" + head[1:] if pat == "plusHeadN" else b"+")
            residues.add((pos + len(head) + 1) % 16)
            assert (pos + len(head) + 1) % 16 == j % 16
            recs.append(r)
            pos += len(r)
        assert residues == set(range(16)), pat
        out[pat] = Text("beside-k%d-%s" % (k, pat), k, 14, b"".join(recs), *_tile(recs, 5))
    return out


# ---------------------------------------------------------------------------------------------------- 4. line structure
def line_texts():
    """texts whose line structure is not `four lines per record, '\\n' after each`. What the reference does with them
    (the oracle restates it, cqf/CQF_mt.h:610-731): the line behind the first '\\n' of a record is the read, whatever the
    lines hold; a chunk counts from its own first byte; the walk stops at the first memchr that finds no '\\n' -- a read
    whose own line has no '\\n' is dropped, one whose '+' or quality line is cut short is still counted (the reference
    itself dereferences the failed memchr there: CQF_mt.h:723-726; the oracle and the device stop instead). A '\\r' is a
    byte of the read like any other that is no base: a CRLF file gives every read one more (k-mer-bearing) position,
    seed 0 on the forward strand and seedTab['\\r' & 7] = 0 on the other (nthash.hpp:15,299)."""
    out = []
    rnd = random.Random(41)
    k, qb = 21, 13

    def recs(n, lo=21, hi=120):
        return [_rec(rnd.randrange(1000), _bases(rnd, rnd.randrange(lo, hi))) for _ in range(n)]

    def one(name, fq, k=k):
        out.append(Text("lines-" + name, k, qb, fq, [0], [len(fq)]))

    body = b"".join(recs(12))
    last = _rec(7, _bases(rnd, 60))
    one("no-final-newline", body + last[:-1])
    one("cut-inside-quality", body + last[:-20])
    one("stops-after-sequence-line", body + last[:last.index(b"\n+")+1])
    one("stops-inside-sequence-line", body + last[:last.index(b"\n+")])
    one("stops-after-plus-newline", body + last[:last.index(b"\n+") + 3])
    one("stops-after-plus", body + last[:last.index(b"\n+") + 2])
    one("stops-after-header", body + b"@h\n")
    one("empty-sequence-line", body + b"@e\n\n+\n\n" + b"".join(recs(5)))
    one("empty-header-and-quality", b"".join(b"\n" + bytes(_bases(rnd, 50 + i)) + b"\n+\n\n" for i in range(8)) + body)
    s = _bases(rnd, 90)
    s[40] = ord("\r")
    one("lone-cr-in-read", body + _rec(1, s) + _rec(2, _bases(rnd, 30) + b"\r" + _bases(rnd, 30)))
    # chunks of newlines only, and of one, two and three lines, among whole records
    parts = [b"".join(recs(3)), b"\n\n\n\n\n", b"".join(recs(2)), b"@x\n", b"@y\n" + bytes(_bases(rnd, 40)) + b"\n",
             b"@z\n" + bytes(_bases(rnd, 33)) + b"\n+\n", b"\n", b"".join(recs(2)), b"\n" * 37, last[:-1]]
    offs, lens, pos = [], [], 0
    for p in parts:
        offs.append(pos)
        lens.append(len(p))
        pos += len(p)
    out.append(Text("lines-newline-chunks-and-short-chunks", k, qb, b"".join(parts), offs, lens))
    # CRLF through the library: every line ends "\r\n"; chunks of 1, 4 and all records
    for kk in (21, 47):
        rs = [_rec(i, _bases(rnd, rnd.randrange(kk - 2, 160))).replace(b"\n", b"\r\n") for i in range(24)]
        for per in (1, 4, 24):
            out.append(Text("lines-crlf-k%d-per%d" % (kk, per), kk, qb, b"".join(rs), *_tile(rs, per)))
    return out


# ---------------------------------------------------------------------------------------------------- 5. chunk tables
def _tiny_records(rnd, n):
    """records of 17 .. 25 bytes: k = 5, reads of 5 .. 9 bases"""
    rs = []
    for i in range(n):
        s = _bases(rnd, rnd.randrange(5, 10))
        if i % 11 == 3 and len(s) > 5:
            s[5] = ord("N")
        rs.append(_rec(i, s, head=b"@" + bytes([97 + i % 26])))
    assert {len(r) for r in rs} <= set(range(17, 26))
    return rs


def chunk_table_texts():
    """chunk tables that do not tile the text in ascending 16-byte-or-longer pieces: the cases shk_unit_flags' byte masks
    (`wb + j < off || wb + j >= end`) exist for. k = 5, records of 17 .. 25 bytes."""
    out = []
    k, qb = 5, 12
    rnd = random.Random(51)
    rs = _tiny_records(rnd, 60)
    fq = b"".join(rs)
    offs, lens = _tile(rs, 1)
    out.append(Text("chunks-one-record-each", k, qb, fq, offs, lens))           # two chunks share a 16-byte unit
    out.append(Text("chunks-descending", k, qb, fq, offs[::-1], lens[::-1]))
    perm = list(range(len(offs)))
    rnd.shuffle(perm)
    out.append(Text("chunks-shuffled", k, qb, fq, [offs[i] for i in perm], [lens[i] for i in perm]))
    # gaps between the chunks: newlines, 'N's, whole records nobody asked for; bytes in front of the first chunk and
    # behind the last
    gaps = [b"\n\n\n", b"NNNNNNN", b"@f\nACGTACGT\n+\nIIIIIIII\n", b"N\nN\n", b"\n", b"@g\nTTTTTTT\n+\nIIIIIII\n@h\nGG", b"", b"NN\n\nNN"]
    text, goffs, glens = bytearray(b"@front\nACGTTGCA\n+\nIIIIIIII\n\nN"), [], []
    for i in range(0, len(rs), 3):
        piece = b"".join(rs[i:i + 3])
        goffs.append(len(text))
        glens.append(len(piece))
        text += piece + gaps[(i // 3) % len(gaps)]
    text += b"\n@back\nACGTACGTAC\n+\nIIIIIIIIII\nNNN"
    out.append(Text("chunks-with-gaps", k, qb, text, goffs, glens))
    # chunks of 1 .. 15 bytes (pieces of records: whatever lines they hold count from the piece's own first byte) and
    # zero-length chunks (allowed: no reads), between whole records
    soffs, slens, pos = [], [], 0
    for i, r in enumerate(rs):
        cut = 1 + (i * 7) % 15
        if i % 4 == 0:
            soffs += [pos, pos + cut, pos + cut]
            slens += [cut, 0, len(r) - cut]
        elif i % 4 == 1:
            soffs += [pos]
            slens += [len(r)]
        elif i % 4 == 2:
            soffs += [pos + len(r) - cut]          # only the record's last bytes: the rest lies in no chunk
            slens += [cut]
        else:
            soffs += [pos, pos]
            slens += [0, len(r)]
        pos += len(r)
    soffs.append(len(fq))
    slens.append(0)                                # a zero-length chunk at the very end of the text
    out.append(Text("chunks-of-1-to-15-bytes-and-empty", k, qb, fq, soffs, slens))
    big = _tiny_records(random.Random(52), MAX_CHUNKS)
    out.append(Text("chunks-4096", k, qb, b"".join(big), *_tile(big, 1)))
    return out


# ---------------------------------------------------------------------------------------------------- by name
LONG_NAMES = ["long-k%d-%s" % (k, v) for k in (21, 47, 64, 65, 191) for v in ("plain", "n700", "nedges", "lower_iupac")]
_groups = {}


def group(fn):
    """the texts of one generator, built once per process: {name: Text}"""
    if fn not in _groups:
        r = fn()
        _groups[fn] = r if isinstance(r, dict) else {T.name: T for T in r}
    return _groups[fn]


def all_texts():
    """every text of the cases above (the 65535 / 65536 batches that count included)"""
    out = list(group(long_read_texts).values())
    for k in (21, 47):
        out += list(neighbour_texts(k).values())
    out += list(group(line_texts).values()) + list(group(chunk_table_texts).values())
    for bad_len in (65536, 70000, 200000):
        out += too_long_batches(bad_len)[2::2]
    return out


# ---------------------------------------------------------------------------------------------------- the checks
@contextlib.contextmanager
def _pack(on):
    old = os.environ.pop("SHK_NO_PACK", None)
    if not on:
        os.environ["SHK_NO_PACK"] = "1"
    try:
        yield
    finally:
        os.environ.pop("SHK_NO_PACK", None)
        if old is not None:
            os.environ["SHK_NO_PACK"] = old


def _ctx_for(mk_ctx, T, largest=None):
    """a context sized for T's keys; `largest` = the largest text it will be handed (T's own when None)"""
    fq = T.fq if largest is None else largest
    nl = fq.count(b"\n")
    nk = len(T.expected()[0])
    return mk_ctx(qb=T.qb, k=T.k, max_batch_bytes=len(fq) + 16, max_batch_reads=nl + MAX_CHUNKS + 16,
                  max_batch_keys=max(1 << 14, nk + 64, 2 * (len(fq) // 64 + nl + MAX_CHUNKS + 8)))


def _state(ctx):
    t = ctx.totals()
    return ctx.blocks(), ctx.header(), t.nelts, t.ndistinct


def check(mk_ctx, T, short=False):
    """what every text goes through; returns the key words of shk_hash_chunks.
    shk_hash_chunks (device text, in an allocation without slack): exactly the oracle's keys per chunk, tagged with the
    chunk's index, in stream order. shk_hash_route_chunks(.., 1) with the 2-bit staging and without it (SHK_NO_PACK), both
    on that device text, and without it once more on host text: the same multiset and count. shk_count_chunks, and
    shk_prepare_chunks + shk_count_prepared on a second context: table bytes, header and totals of the oracle's t = 1
    build. (short: shk_hash_chunks on device text and shk_count_chunks alone -- for the one text whose 65536 workgroups
    per parse kernel cost the emulator a minute per pass; the GPU runs all of it.)"""
    exp, blocks, header, nelts, ndistinct = T.expected()
    ctx = _ctx_for(mk_ctx, T)
    ctx.profile(True)
    dtext = ctx.dev_text(T.fq)
    dp, nw = ctx.hash_chunks(dtext, T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
    words = ctx.read_words(dp, nw)
    assert nw == len(exp), T.name
    assert words == exp, T.name
    if short:
        st = ctx.count_chunks(T.fq, T.offs, T.lens)
        assert st["kmers"] == nelts and _state(ctx) == (blocks, header, nelts, ndistinct), T.name
        ctx.close()
        return words
    for pack, on_device in ((True, True), (False, True), (False, False)):
        with _pack(pack):
            ctx.profile_reset()
            if on_device:
                dp, counts, nw = ctx.hash_route_chunks(dtext, T.offs, T.lens, 1, on_device=True, text_bytes=len(T.fq))
            else:
                dp, counts, nw = ctx.hash_route_chunks(T.fq, T.offs, T.lens, 1)
            assert nw == len(exp) == counts[0], (T.name, pack, on_device)
            assert sorted(ctx.read_words(dp, nw)) == sorted(exp), (T.name, pack, on_device)
            prof = ctx.profile_get()
            assert ("k_pack_reads" in prof) == pack and "k_roll_scatter" in prof, (T.name, pack, on_device)
    st = ctx.count_chunks(T.fq, T.offs, T.lens)
    assert st["kmers"] == nelts and st["chunks"] == len(T.offs), T.name
    assert _state(ctx) == (blocks, header, nelts, ndistinct), T.name
    ctx.close()
    ctx = _ctx_for(mk_ctx, T)
    ctx.prepare_chunks(T.fq, T.offs, T.lens)
    st = ctx.count_prepared()
    assert st["kmers"] == nelts, T.name
    assert _state(ctx) == (blocks, header, nelts, ndistinct), T.name
    ctx.close()
    return words


def _raises(code, fn, what):
    try:
        fn()
    except Exception as e:        # shk.ShkError of whichever binding the factory uses
        assert getattr(e, "code", None) == code, (what, e)
        return
    raise AssertionError("%s: no error, expected code %d" % (what, code))


def _entry_points(ctx, text, offs, lens, on_device=False, text_bytes=None, reaches_kernels=False):
    """every call that takes FASTQ text, as {name: thunk}; the overlapped pair reports a front-end error from its second
    half. The two shk_hash_route_chunks thunks assert through the kernel times which path ran (the staging precedes the
    roll kernels, which find a read that is too long)."""
    kw = dict(on_device=on_device, text_bytes=text_bytes)

    def routed(pack, packs):
        with _pack(pack):
            ctx.profile(True)
            ctx.profile_reset()
            try:
                ctx.hash_route_chunks(text, offs, lens, 1, **kw)
            finally:
                if packs is not None:
                    assert ("k_pack_reads" in ctx.profile_get()) == packs, pack

    def prepared():
        ctx.prepare_chunks(text, offs, lens, **kw)
        ctx.count_prepared()
    reaches = None if not reaches_kernels else True
    return {"count_chunks": lambda: ctx.count_chunks(text, offs, lens, **kw),
            "hash_chunks": lambda: ctx.hash_chunks(text, offs, lens, **kw),
            "hash_route_chunks": lambda: routed(True, reaches),
            "hash_route_chunks/SHK_NO_PACK": lambda: routed(False, reaches and False),
            "prepare_chunks": lambda: ctx.prepare_chunks(text, offs, lens, **kw),
            "prepare_chunks + count_prepared": prepared}


IMMEDIATE = ("count_chunks", "hash_chunks", "hash_route_chunks", "hash_route_chunks/SHK_NO_PACK", "prepare_chunks")


def run_too_long(mk_ctx, bad_len):
    """a read of bad_len > 65535 bases: every entry point refuses the batch with SHK_ERR_FASTQ and leaves table, header
    and totals as they were; the same batch with that read cut to 65535 bases then counts on the same context"""
    k, qb, first, bad, good = too_long_batches(bad_len)
    both = Text("first+cut", k, qb, first.fq + good.fq, first.offs + [len(first.fq) + a for a in good.offs], first.lens + good.lens)
    exp, blocks, header, nelts, ndistinct = both.expected()
    ctx = _ctx_for(mk_ctx, both, largest=bad.fq)
    ctx.count_chunks(first.fq, first.offs, first.lens)
    before = _state(ctx)
    assert before[2] > 0
    E = _entry_points(ctx, bad.fq, bad.offs, bad.lens, reaches_kernels=True)
    for name in ("count_chunks", "hash_chunks", "hash_route_chunks", "hash_route_chunks/SHK_NO_PACK", "prepare_chunks + count_prepared"):
        _raises(ERR_FASTQ, E[name], (name, bad_len))
        assert _state(ctx) == before, (name, bad_len)
    dp, nw = ctx.hash_chunks(good.fq, good.offs, good.lens)
    assert ctx.read_words(dp, nw) == good.expected()[0]
    st = ctx.count_chunks(good.fq, good.offs, good.lens)
    assert st["kmers"] == good.expected()[3]
    assert _state(ctx) == (blocks, header, nelts, ndistinct), bad_len
    ctx.close()


def run_chunk_limit(mk_ctx, T):
    """T has SHK_MAX_CHUNKS = 4096 chunks (check() counts them in one call); one chunk more is SHK_ERR_BATCH"""
    assert len(T.offs) == MAX_CHUNKS
    ctx = _ctx_for(mk_ctx, T)
    before = _state(ctx)
    offs, lens = T.offs + [len(T.fq)], T.lens + [0]
    E = _entry_points(ctx, T.fq, offs, lens)
    for name in IMMEDIATE:
        _raises(ERR_BATCH, E[name], name)
    assert _state(ctx) == before
    ctx.close()


def run_alignment(mk_ctx, T):
    """device text must be 16-byte aligned (include/shk.h: the parse kernels and k_count_keys fetch aligned 16-byte units
    relative to the text's base): a pointer that is not is SHK_ERR_ARG from every entry point before anything runs; 16
    bytes into an allocation is fine"""
    exp, blocks, header, nelts, ndistinct = T.expected()
    ctx = _ctx_for(mk_ctx, T)
    before = _state(ctx)
    for off in (1, 8):
        p = ctx.dev_text(T.fq, off)
        assert p % 16 == off
        E = _entry_points(ctx, p, T.offs, T.lens, True, len(T.fq))
        for name in IMMEDIATE:
            _raises(ERR_ARG, E[name], (name, off))
        assert _state(ctx) == before
    p = ctx.dev_text(T.fq, 16)
    assert p % 16 == 0
    dp, nw = ctx.hash_chunks(p, T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
    assert ctx.read_words(dp, nw) == exp
    ctx.prepare_chunks(p, T.offs, T.lens, on_device=True, text_bytes=len(T.fq))
    ctx.count_prepared()
    assert _state(ctx) == (blocks, header, nelts, ndistinct)
    ctx.close()
