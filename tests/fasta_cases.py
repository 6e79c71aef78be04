"""Cases for shk_count_fasta (include/shk.h), shared by the emulator and the GPU tests of tests/test_fasta.py.

Expected values never come from the library: Reader below is a byte-by-byte Python reading of the grammar in shk.h, the
keys of its runs come from cqflibs.oracle().seq_keys (the oracle's reads_to_kmers, which on reads made of bases hashes
every k-mer), the table from the oracle's qf_new + qf_insert and, where oracle/_ref is built, the reference's as well."""
import contextlib
import os
import random

import numpy as np

import cqflibs

BASES = b"ACGTacgt"


class Reader:
    """the grammar, one byte at a time; keeps its state over feed() calls as a context does over pieces"""

    def __init__(self, k):
        self.k = k
        self.header, self.line_start = False, True
        self.run, self.runs = bytearray(), []

    def _break(self):
        if self.run:
            self.runs.append(bytes(self.run))
            self.run = bytearray()

    def feed(self, piece):
        st = {"records": 0, "bases": 0, "breaks": 0, "kmers": 0}
        for c in piece:
            if self.header:
                if c == 10:
                    self.header, self.line_start = False, True
                continue
            if self.line_start and c in b">;":
                self.header, self.line_start = True, False
                st["records"] += 1
                self._break()
                continue
            if c == 10:
                self.line_start = True
                continue
            self.line_start = False
            if c == 13:
                continue
            if c in BASES:
                self.run.append(c)
                st["bases"] += 1
                if len(self.run) >= self.k:
                    st["kmers"] += 1
            else:
                st["breaks"] += 1
                self._break()
        return st

    def all_runs(self):
        return self.runs + ([bytes(self.run)] if self.run else [])


def runs_of(text, k=1):
    r = Reader(k)
    r.feed(text)
    return r.all_runs()


def keys_of(text, k, hb):
    return cqflibs.oracle().seq_keys(runs_of(text, k), k, hb)


def dna(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


@contextlib.contextmanager
def segment(n):
    """SHK_FASTA_SEGMENT in the environment of the contexts created inside (None: the default)"""
    old = os.environ.pop("SHK_FASTA_SEGMENT", None)
    if n is not None:
        os.environ["SHK_FASTA_SEGMENT"] = str(n)
    try:
        yield
    finally:
        os.environ.pop("SHK_FASTA_SEGMENT", None)
        if old is not None:
            os.environ["SHK_FASTA_SEGMENT"] = old


class Expect:
    """the oracle's table (and the reference's) of everything fed so far"""

    def __init__(self, qb):
        self.qb = qb
        self.q = cqflibs.oracle().new(qb)
        self.r = cqflibs.ref().new(qb) if cqflibs.have_ref() else None

    def insert(self, keys):
        for x in keys.tolist():
            self.q.insert(x)
            if self.r is not None:
                self.r.insert(x)

    def check(self, ctx, what=""):
        want = self.q.blocks()
        if self.r is not None:
            assert self.r.blocks() == want, "oracle and reference disagree " + what
        assert ctx.blocks() == want, "table bytes differ " + what
        t = ctx.totals()
        assert (t.nelts, t.ndistinct) == (self.q.nelts(), self.q.ndistinct()), what

    def free(self):
        self.q.free()
        if self.r is not None:
            self.r.free()


def count_stream(ctx, exp, pieces, k, what=""):
    """the pieces of one stream into ctx (the first with first=True); statistics of every call against the Reader's,
    then the table against the oracle's"""
    rd = Reader(k)
    d0 = exp.q.ndistinct()
    newd = 0
    for i, p in enumerate(pieces):
        st, fs = ctx.count_fasta(p, first=(i == 0))
        want = rd.feed(p)
        assert fs == want, (what, i, fs, want)
        assert (st["kmers"], st["chunks"], st["denoise_rounds"]) == (want["kmers"], 1, 0), (what, i, st)
        newd += st["new_distinct"]
    exp.insert(cqflibs.oracle().seq_keys(rd.all_runs(), k, exp.qb + 8))
    exp.check(ctx, what)
    assert newd == exp.q.ndistinct() - d0, what


# ---------------------------------------------------------------- the texts
def grammar_texts():
    s = dna(300, 1)
    t = {
        "empty": b"",
        "header_only": b">only a header\n",
        "header_no_newline": b">ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT",
        "no_final_newline": b">r\n" + s[:90],
        "no_header": wrap(s[:130], 60),
        "gt_inside_line": b">r\n" + s[:40] + b">" + s[40:90] + b"\n" + s[90:130] + b" >x\n",
        "semicolon_lines": b";comment ACGTACGTACGTACGTACGTACGT\n>r\n" + s[:50] + b"\n;" + s[50:100] + b"\n" + s[100:160] + b"\n",
        "crlf": b">r\r\n" + wrap(s[:150], 60).replace(b"\n", b"\r\n"),
        "blank_lines": b">r\n" + s[:40] + b"\n\n\n" + s[40:90] + b"\n\r\n" + s[90:140] + b"\n",
        "lower_case": b">r\n" + wrap(s[:80].lower() + s[80:120] + s[120:200].lower(), 60),
        "n_runs": b">r\n" + wrap(s[:70] + b"N" * 45 + s[70:140] + b"n" + s[140:200] + b"NN" + s[200:210], 60),
        "iupac": b">r\n" + wrap(s[:50] + b"R" + s[50:100] + b"y" + s[100:150] + b"KMSWBDHVU" + s[150:200], 60),
        "odd_bytes": b">r\n" + s[:40] + b" " + s[40:80] + b"\t" + s[80:120] + b"*" + s[120:160] + b"\0" + s[160:200] + b"\xff" + s[200:240] + b"-\x80\x41\n",
        "consecutive_headers": b">a\n>b\n>c\n" + s[:60] + b"\n>d\n>e\n" + s[60:120] + b"\n",
        "header_full_of_bases": b">" + s[:200] + b"\n" + s[200:260] + b"\n>" + s[:200] + b"\n" + s[100:160] + b"\n",
        "header_over_one_tile": s[:45] + b"\n>" + b"ACGT" * 1300 + b"\n" + s[45:100] + b"\n",
        "header_over_two_tiles": s[:45] + b"\n>" + b"GATTACA" * 1400 + b"\n" + s[45:100] + b"\n",
        "header_holding_gt": b">a >b >c\n" + s[:60] + b"\n>>>\n" + s[60:110] + b"\n",
        "record_across_header": s[:30] + b"\n>h\n" + s[30:60] + b"\n",
    }
    for w in (1, 15, 16, 17, 60, 61):
        t["width_%d" % w] = b">w\n" + wrap(s[:150], w)
    return t


K_LIST = [1, 5, 31, 32, 33, 47, 64, 65, 100, 191]


def run_length_text(k, seg, seed):
    """runs of k-1, k, k+1, S+k-2, S+k-1, S+k and 2S+k-1 bases between breaks of several kinds"""
    lens = [k - 1, k, k + 1, seg + k - 2, seg + k - 1, seg + k, 2 * seg + k - 1]
    seps = [b"N", b"\n>h\n", b"NNN\n", b" ", b"\nn", b"*", b"\n;c\n"]
    s = dna(sum(lens), seed)
    out, at = [b">r\n"], 0
    for n, sep in zip(lens, seps):
        out.append(wrap(s[at:at + n], 70)[:-1] if n else b"")
        out.append(sep)
        at += n
    return b"".join(out)


def offsets_text(k, seed):
    """for every j in 0..63 a prefix run, a break, then a run of k + 70 bases that starts at an offset of j (mod 64) in
    the call's base stream; returns (text, the offsets reached)"""
    s, at, out, seen = dna(64 * (k + 70 + 64), seed), 0, [b">o\n"], []
    nbases = 0
    for j in range(64):
        p = (j - nbases) % 64
        out += [s[at:at + p], b"N", wrap(s[at + p:at + p + k + 70], 60), b"*"]
        seen.append((nbases + p) % 64)
        at += p + k + 70
        nbases += p + k + 70
    return b"".join(out), seen


# ---------------------------------------------------------------- runners (mk = context factory of the build under test)
def ctx_for(mk, qb, k, seg, text_cap=1 << 16, **kw):
    with segment(seg):
        return mk(qb=qb, k=k, max_batch_bytes=text_cap, max_batch_keys=text_cap, **kw)


def run_grammar(mk, k, seg, levels_bits=3):
    ctx, exp = ctx_for(mk, 13, k, seg, max_level_bits=levels_bits), Expect(13)
    for name, text in grammar_texts().items():
        count_stream(ctx, exp, [text], k, name)
    ctx.close()
    exp.free()


def run_run_lengths(mk, k, seg):
    ctx, exp = ctx_for(mk, 14, k, seg, max_level_bits=3), Expect(14)
    count_stream(ctx, exp, [run_length_text(k, seg, 100 + k)], k, "k=%d seg=%d" % (k, seg))
    ctx.close()
    exp.free()


def run_offsets(mk, k, seg):
    ctx, exp = ctx_for(mk, 15, k, seg, max_level_bits=3), Expect(15)
    text, seen = offsets_text(k, 200)
    assert seen == list(range(64))
    count_stream(ctx, exp, [text], k, "runs at every stream offset")
    ctx.close()
    exp.free()


def run_soup(mk, k, seg, ntexts=24):
    """texts drawn byte by byte from an alphabet heavy in line ends, header bytes and breaks, each fed in random pieces:
    every combination of neighbours the 16-byte masks can meet, at every alignment"""
    rng = random.Random(1234 + k)
    ctx, exp = ctx_for(mk, 13, k, seg, max_level_bits=3), Expect(13)
    for i in range(ntexts):
        alpha = b"ACGTacgt" * rng.choice([1, 4, 16]) + b"\n\n\r>;N \xc1"
        text = bytes(rng.choice(alpha) for _ in range(rng.randrange(1, 400)))
        cuts = sorted(rng.randrange(len(text) + 1) for _ in range(rng.randrange(0, 4)))
        pieces = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
        count_stream(ctx, exp, pieces, k, "soup %d %r" % (i, cuts))
    ctx.close()
    exp.free()


def run_long_runs(mk, k=5, seg=16):
    """runs of many segments: one of 40, then six of ten in a context whose small text capacity leaves room for fewer
    long-run records than that (the rest are written by their own workgroup)"""
    ctx, exp = ctx_for(mk, 14, k, seg, text_cap=2048, max_level_bits=3), Expect(14)
    count_stream(ctx, exp, [b">l\n" + wrap(dna(40 * seg + k - 1, 5), 60)], k, "one long run")
    count_stream(ctx, exp, [b"N".join(dna(10 * seg + k - 1, 60 + i) for i in range(6))], k, "six long runs")
    ctx.close()
    exp.free()


def run_default_segment(mk, k=47):
    import shk
    ctx, exp = ctx_for(mk, 13, k, None, max_level_bits=3), Expect(13)
    count_stream(ctx, exp, [b">one\n" + wrap(dna(shk.FASTA_SEGMENT + k, 7), 80)], k, "default segment")
    ctx.close()
    exp.free()


def stream_text(k):
    s = dna(330, 11)
    return (b">rec one\r\n" + s[:70] + b"\r\n" + s[70:118] + b"N" + s[118:121] + b"N" + s[121:250] + b"\n>two\n" + s[250:330] + b"\n", s)


def chosen_cuts(k, seg):
    text, s = stream_text(k)
    cuts = {
        "inside_header": 5,
        "behind_gt": 1,
        "between_cr_lf": text.index(b"\r\n") + 1,
        "few_bases_behind_break": text.index(b"N") + 2,
        "on_a_break": text.index(b"N"),
        "behind_a_break": text.index(b"N") + 1,
        "on_segment_end": text.index(b"\r\n") + 2 + seg + k - 1 + 2,      # (+2: the line end inside the run)
        "inside_second_header": text.index(b">two") + 2,
    }
    return text, cuts


def run_chosen_cut(mk, k, seg, name):
    text, cuts = chosen_cuts(k, seg)
    c = cuts[name]
    assert 0 < c < len(text)
    ctx, exp = ctx_for(mk, 12, k, seg, max_level_bits=2), Expect(12)
    count_stream(ctx, exp, [text[:c], text[c:]], k, "%s (cut at %d)" % (name, c))
    ctx.close()
    exp.free()


def run_every_cut(mk, k, seg):
    """every cut position of the text as two pieces into ONE context: after c cuts every count is c times the
    single-call count; a mismatch is run again cut by cut to name the position"""
    text, _ = stream_text(k)
    keys = keys_of(text, k, 12 + 8)
    uniq, cnt = np.unique(keys, return_counts=True)
    ctx = ctx_for(mk, 12, k, seg, max_level_bits=2)
    ncuts = len(text) - 1
    for c in range(1, len(text)):
        ctx.count_fasta(text[:c], first=True)
        ctx.count_fasta(text[c:], first=False)
    got = ctx.dump()
    ctx.close()
    want = [(int(a), int(b) * ncuts) for a, b in zip(uniq, cnt)]
    if got != want:
        for c in range(1, len(text)):
            one = ctx_for(mk, 12, k, seg, max_level_bits=2)
            one.count_fasta(text[:c], first=True)
            one.count_fasta(text[c:], first=False)
            d = one.dump()
            one.close()
            assert d == [(int(a), int(b)) for a, b in zip(uniq, cnt)], "cut at byte %d" % c
        assert got == want, "no single cut differs, the accumulated table does"


def run_byte_by_byte(mk, k, seg):
    text, _ = stream_text(k)
    ctx, exp = ctx_for(mk, 10, k, seg, max_level_bits=1), Expect(10)
    count_stream(ctx, exp, [text[i:i + 1] for i in range(len(text))], k, "one byte per call")
    ctx.close()
    exp.free()


def run_fastq_agreement(mk, k, seg):
    """base-only reads through shk_count_chunks and as FASTA records: byte-identical tables"""
    rng = random.Random(5)
    reads = [dna(rng.choice([k - 1, k, 90, 150, 151, 300]), 300 + i) for i in range(40)]
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    fa = b"".join(b">r%d\n%s" % (i, wrap(r, 60)) for i, r in enumerate(reads))
    a, b = ctx_for(mk, 14, k, seg, max_level_bits=3), ctx_for(mk, 14, k, seg, max_level_bits=3)
    st = a.count_chunks(fq, [0], [len(fq)])
    st2, fs = b.count_fasta(fa)
    assert st["kmers"] == st2["kmers"] == fs["kmers"] == sum(max(0, len(r) - k + 1) for r in reads)
    assert a.blocks() == b.blocks()
    a.close()
    b.close()


def run_trigger(mk, k, seg):
    """a context with rounds whose trigger the call reaches fires one round behind the call; one without fires none"""
    text = b">t\n" + wrap(dna(1500, 21), 60) + b">u\n" + wrap(dna(700, 21), 60)      # (the second record repeats the first's start)
    keys = keys_of(text, k, 13 + 8)
    ndist = len(set(keys.tolist()))
    ctx = ctx_for(mk, 13, k, seg, max_level_bits=3, trigger=ndist // 2, num_denoise=2, min_denoise_len=64)
    exp = Expect(13)
    st, fs = ctx.count_fasta(text)
    exp.insert(keys)
    removed = exp.q.denoise_round(64)
    assert (st["denoise_rounds"], st["removed"], st["kmers"]) == (1, removed, len(keys)), st
    assert removed > 0
    assert ctx.blocks() == exp.q.blocks()
    assert ctx.totals().rounds_left == 1
    ctx.close()
    exp.free()
    ctx = ctx_for(mk, 13, k, seg, max_level_bits=3, trigger=ndist // 2, num_denoise=0)
    exp = Expect(13)
    count_stream(ctx, exp, [text], k, "no rounds")
    ctx.close()
    exp.free()


GEOMETRIES = [(12, 0, 1), (12, 2, 2), (14, 2, 3)]       # qb, max_level_bits, partition levels


def run_geometry(mk, k, seg, qb, mlb):
    ctx, exp = ctx_for(mk, qb, k, seg, max_level_bits=mlb), Expect(qb)
    text, _ = stream_text(k)
    count_stream(ctx, exp, [run_length_text(k, seg, 31)], k, "geometry, one call")
    count_stream(ctx, exp, [text[:100], text[100:101], text[101:]], k, "geometry, pieces")
    ctx.close()
    exp.free()


def run_errors(mk, k, seg, dev_bytes):
    """every error of the contract; after each the table is unchanged and the stream goes on in smaller pieces.
    dev_bytes(b) -> (pointer the library can read, keep-alive)"""
    import shk
    text, _ = stream_text(k)
    nk = len(keys_of(text, k, 20))

    def expect_err(ctx, code, *a, **kw):
        before = ctx.blocks()
        try:
            ctx.count_fasta(*a, **kw)
        except shk.ShkError as e:
            assert e.code == code, (e.code, code)
        else:
            raise AssertionError("no error %d" % code)
        assert ctx.blocks() == before

    def finish(ctx, exp, first_piece):
        # the stream: first_piece went in before the failing call; the rest follows in pieces of 70 bytes
        rest = text[len(first_piece):]
        for i in range(0, len(rest), 70):
            ctx.count_fasta(rest[i:i + 70], first=False)
        exp.insert(keys_of(text, k, exp.qb + 8))
        exp.check(ctx, "stream continued behind an error")

    head = text[:90]
    # text_bytes > max_batch_bytes
    with segment(seg):
        ctx = mk(qb=12, k=k, max_batch_bytes=200, max_batch_keys=4096, max_level_bits=2)
    exp = Expect(12)
    ctx.count_fasta(head, first=True)
    expect_err(ctx, -7, text[90:], first=False)
    finish(ctx, exp, head)
    ctx.close()
    exp.free()
    # more k-mers than max_batch_keys
    with segment(seg):
        ctx = mk(qb=12, k=k, max_batch_bytes=4096, max_batch_keys=nk // 2, max_level_bits=2)
    exp = Expect(12)
    ctx.count_fasta(head, first=True)
    expect_err(ctx, -7, text[90:], first=False)
    finish(ctx, exp, head)
    ctx.close()
    exp.free()
    # more segments than max_batch_reads
    with segment(16):
        ctx = mk(qb=12, k=k, max_batch_bytes=4096, max_batch_keys=4096, max_batch_reads=8, max_level_bits=2)
    exp = Expect(12)
    ctx.count_fasta(head, first=True)
    expect_err(ctx, -7, text[90:], first=False)
    finish(ctx, exp, head)
    ctx.close()
    exp.free()
    # a device pointer that is not 16-byte aligned; a sharded context; batches prepared and not yet counted
    with segment(seg):
        ctx = mk(qb=12, k=k, max_batch_bytes=4096, max_batch_keys=4096, max_level_bits=2)
    exp = Expect(12)
    ctx.count_fasta(head, first=True)
    ptr, keep = dev_bytes(b"\n" * 16 + text[90:])
    expect_err(ctx, -1, ptr + 1, first=False, on_device=True, text_bytes=len(text) - 90)
    fq = b"@r\n%s\n+\n%s\n" % (dna(60, 1), b"I" * 60)
    ctx.prepare_chunks(fq, [0], [len(fq)])
    expect_err(ctx, -7, text[90:], first=False)
    ctx.count_prepared()
    exp.insert(cqflibs.oracle().seq_keys([dna(60, 1)], k, 20))
    st, fs = ctx.count_fasta(ptr + 16, first=False, on_device=True, text_bytes=len(text) - 90)      # (aligned device text works)
    exp.insert(keys_of(text, k, 20))
    exp.check(ctx, "device text")
    ctx.close()
    exp.free()
    with segment(seg):
        sh = mk(qb=12, k=k, max_batch_bytes=4096, max_batch_keys=4096, num_shards=2, shard_index=1)
    expect_err(sh, -1, text)
    sh.close()


def run_large(mk):
    """a 4 Mb multi-line genome with N blocks and one 1 Mb record, default segment, through dump() and numpy"""
    k, qb = 47, 22
    rng = np.random.default_rng(9)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4_000_000)]
    for at, n in ((300_000, 50_000), (1_234_567, 1), (2_000_000, 123_457), (3_900_000, 1000)):
        seq[at:at + n] = ord("N")
    seq[2_500_000:2_600_000] |= 0x20        # lower case
    recs = [(b">chr1 a 1 Mb record\n", seq[:1_000_000])]
    at = 1_000_000
    while at < len(seq):
        n = int(rng.integers(1000, 400_000))
        recs.append((b">contig_%d\n" % at, seq[at:at + n]))
        at += n
    parts = []
    for h, s in recs:
        parts.append(h)
        full = len(s) // 60 * 60
        lines = np.empty((full // 60, 61), dtype=np.uint8)
        lines[:, :60] = s[:full].reshape(-1, 60)
        lines[:, 60] = 10
        parts.append(lines.tobytes())
        if full < len(s):
            parts.append(s[full:].tobytes() + b"\n")
    text = b"".join(parts)
    # the runs by numpy (the Reader's byte loop would take a minute): records are runs' bounds, and so are the N blocks
    runs = []
    for _, s in recs:
        isb = s != ord("N")
        edges = np.flatnonzero(np.diff(np.concatenate(([0], isb.view(np.int8), [0]))))
        runs += [s[a:b].tobytes() for a, b in zip(edges[0::2], edges[1::2])]
    assert runs[0] == runs_of(text[:400_000])[0] and runs[-1] == runs_of(text[-120_000:])[-1]
    keys = cqflibs.oracle().seq_keys(runs, k, qb + 8)
    uniq, cnt = np.unique(keys, return_counts=True)
    ctx = mk(qb=qb, k=k, max_batch_bytes=len(text) + 64, max_batch_keys=len(text))
    st, fs = ctx.count_fasta(text)
    assert fs == {"records": len(recs), "bases": int((seq != ord("N")).sum()), "breaks": int((seq == ord("N")).sum()), "kmers": len(keys)}
    assert st["kmers"] == len(keys) and st["new_distinct"] == len(uniq)
    got = ctx.dump()
    ctx.close()
    assert len(got) == len(uniq)
    assert np.array_equal(np.array([g[0] for g in got], dtype=np.uint64), uniq)
    assert np.array_equal(np.array([g[1] for g in got], dtype=np.int64), cnt)


def run_own_output(mk, tmp_path):
    """unitigs written by shk_unitig_set_write, counted as FASTA: every k-mer of a unitig is solid in the reads filter"""
    import shk
    import synth
    from fastq_util import chunks_by_records
    k, qb, amin, smin = 31, 16, 2, 2
    fq = synth.make_fastq(synth.make_genome(6000, 3), 600, 100, 0.005, seed=4)
    offs, lens = chunks_by_records(fq, 200)
    reads = mk(qb=qb, k=k, max_batch_bytes=len(fq) + 1024, max_batch_keys=600 * 100)
    reads.count_chunks(fq, offs, lens)
    us = shk.UnitigSet(reads)
    us.add_reads(fq, offs, lens, k, amin, smin, 1000000, 45000)
    path = str(tmp_path / "unitigs.fa")
    ust = us.write(k, path)
    us.close()
    fa = open(path, "rb").read()
    seqs = [ln for ln in fa.split(b"\n") if ln and not ln.startswith(b">")]
    assert ust["unitigs"] == len(seqs) > 0
    own = mk(qb=qb, k=k, max_batch_bytes=len(fa) + 64, max_batch_keys=len(fa))
    st, fs = own.count_fasta(fa)
    assert fs["records"] == len(seqs) and fs["breaks"] == 0
    assert st["kmers"] == sum(len(s) - k + 1 for s in seqs)
    d = own.dump()
    counts, _ = reads.lookup([x for x, _ in d], mode=2)
    assert min(counts) >= min(amin, smin)
    own.close()
    reads.close()


# ---------------------------------------------------------------- command line
def report_case():
    fs = {"records": 3, "bases": 1000, "breaks": 12, "kmers": 900}
    against = {"path": "reads.cqf", "distinct": 850, "present": 800, "min_count": 3, "solid": 640, "inner_product": 12345}
    want = ("records\t3\nbases\t1000\nbreaks\t12\nk-mers\t900\ndistinct\t850\n"
            "against\treads.cqf\npresent\t800\t94.12%\ncount>=3\t640\t75.29%\ninner product\t12345\n")
    return fs, against, want
