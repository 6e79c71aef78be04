"""Cases for shk_query_fasta (include/shk.h), shared by the emulator and the GPU tests of tests/test_query.py.

Expected values never come from the library: Model below is fasta_cases.Reader's byte-by-byte reading of the grammar,
extended to give every base of a piece its ordinal, its record and the k-mer that ends there; the keys come from
cqflibs.oracle().seq_keys, the counts from a Python dict from hashed key to count that is filled next to the table
(Context.insert_counted) -- keyed by hashed key, so hash collisions are answered the way the filter answers them."""
import ctypes as C

import numpy as np

import cqflibs
import fasta_cases as FC

NONE = 0xFFFFFFFF
CAP = 0xFFFFFFFE
M64 = (1 << 64) - 1
SPECIAL_REMS = (0x00, 0x7f, 0x80, 0xff)
HARD_COUNTS = (1, 2, 3, 127, 128, 129, 1 << 14, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, 1 << 35)


class Model(FC.Reader):
    """the grammar, one byte at a time, with what a query needs: per base of the piece the k-mer whose last base it is (or
    None) and the record it belongs to (0 = the record open when the piece began, i = the i-th header line of the piece)"""

    def feed(self, piece):
        st = {"records": 0, "bases": 0, "breaks": 0, "kmers": 0}
        ends, recs = [], []
        for c in piece:
            if self.header:
                if c == 10:
                    self.header, self.line_start = False, True
                continue
            if self.line_start and c in b">;":
                self.header, self.line_start = True, False
                st["records"] += 1
                self.run = bytearray()
                continue
            if c == 10:
                self.line_start = True
                continue
            self.line_start = False
            if c == 13:
                continue
            if c in FC.BASES:
                self.run.append(c)
                del self.run[:-self.k]
                st["bases"] += 1
                full = len(self.run) >= self.k
                st["kmers"] += full
                ends.append(bytes(self.run) if full else None)
                recs.append(st["records"])
            else:
                st["breaks"] += 1
                self.run = bytearray()
        return st, ends, recs

    def expect(self, piece, table, hb, min_count):
        """(statistics, records, track) the call on this piece must answer"""
        st, ends, recs = self.feed(piece)
        kmers = [e for e in ends if e is not None]
        keys = cqflibs.oracle().seq_keys(kmers, self.k, hb) if kmers else []
        counts = iter(table.get(int(x), 0) for x in keys)
        rec = [[0, 0, 0, 0] for _ in range(1 + st["records"])]
        track = []
        for e, r in zip(ends, recs):
            if e is None:
                track.append(NONE)
                continue
            c = next(counts)
            track.append(min(c, CAP))
            rec[r][0] += 1
            rec[r][1] += c >= 1
            rec[r][2] += c >= min_count
            rec[r][3] = (rec[r][3] + c) & M64
        qs = dict(st, present=sum(r[1] for r in rec), solid=sum(r[2] for r in rec), sum=sum(r[3] for r in rec) & M64)
        return qs, np.array(rec, dtype=np.uint64).reshape(-1, 4), np.array(track, dtype=np.uint32)


def text_keys(text, k, hb):
    """the keys of a whole text's k-mers, in text order"""
    _, ends, _ = Model(k).feed(text)
    kmers = [e for e in ends if e is not None]
    return cqflibs.oracle().seq_keys(kmers, k, hb) if kmers else np.zeros(0, dtype=np.uint64)


def fill(ctx, table, pairs):
    """add (key, count) pairs to the table and to its dict"""
    pairs = [(int(a), int(b)) for a, b in pairs]
    if pairs:
        ctx.insert_counted([a for a, _ in pairs], [b for _, b in pairs])
    for a, b in pairs:
        table[a] = table.get(a, 0) + b


def half_of(keys):
    """every second distinct key, with counts 1 .. 5"""
    uniq = sorted(set(int(x) for x in keys))
    return [(x, 1 + i % 5) for i, x in enumerate(uniq[::2])]


def ask(ctx, model, piece, first, table, min_count=2, want_track=True, what=""):
    """one call against the model's answer; returns what the call answered"""
    hb = ctx.cfg.hb
    want_qs, want_rec, want_track_ = model.expect(piece, table, hb, min_count)
    qs, rec, track = ctx.query_fasta(piece, first=first, min_count=min_count, want_track=want_track)
    assert qs == want_qs, (what, qs, want_qs)
    assert rec.shape == want_rec.shape and np.array_equal(rec, want_rec), (what, rec.tolist(), want_rec.tolist())
    if want_track:
        assert track.dtype == np.uint32 and len(track) == len(want_track_), (what, len(track), len(want_track_))
        bad = np.flatnonzero(track != want_track_)
        assert len(bad) == 0, (what, "track differs first at base %d" % bad[0], int(track[bad[0]]), int(want_track_[bad[0]]))
    else:
        assert track is None
    return qs, rec, track


def merge_records(recs_of_pieces):
    """the rec[0] rule: a piece's record 0 continues the last record the caller already has"""
    out = recs_of_pieces[0].copy()
    for r in recs_of_pieces[1:]:
        out[-1] += r[0]
        out = np.concatenate([out, r[1:]])
    return out


def ctx_for(mk, qb, k, seg, text_cap=1 << 16, **kw):
    return FC.ctx_for(mk, qb, k, seg, text_cap=text_cap, **kw)


# ---------------------------------------------------------------- runners (mk = context factory of the build under test)
def run_grammar(mk, k, seg):
    """the header / break / CRLF / lower-case texts of the FASTA cases, each a stream of its own, about half of their
    k-mers in the table: the whole track with every SHK_QUERY_NONE, the record table, the statistics"""
    texts = FC.grammar_texts()
    ctx, table = ctx_for(mk, 11, k, seg, max_level_bits=3), {}
    fill(ctx, table, half_of(np.concatenate([text_keys(t, k, 19) for t in texts.values()])))
    seen = 0
    for name, text in texts.items():
        qs, _, _ = ask(ctx, Model(k), text, True, table, what=name)
        seen += qs["present"]
    assert seen > 0
    ctx.close()


def run_length_text(k, seg, seed):
    """fasta_cases.run_length_text (k-1, k, k+1, S+k-2, S+k-1, S+k, 2S+k-1 bases) and a record whose run of 9S+3 bases is
    long enough for k_fa_long_segments"""
    return FC.run_length_text(k, seg, seed) + b"\n>long one\n" + FC.wrap(FC.dna(9 * seg + 3, seed + 1), 70)


def run_run_lengths(mk, k, seg):
    text = run_length_text(k, seg, 100 + k)
    ctx, table = ctx_for(mk, 12, k, seg, max_level_bits=3), {}
    fill(ctx, table, half_of(text_keys(text, k, 20)))
    qs, rec, _ = ask(ctx, Model(k), text, True, table, what="k=%d seg=%d" % (k, seg))
    assert 9 * seg + 3 < k or rec[-1][0] == 9 * seg + 3 - k + 1
    ctx.close()


def hard_case(k, qb):
    """a text whose k-mers hit the remainders 0x00, 0x7f, 0x80, 0xff with each of HARD_COUNTS, and filler up to a load of
    about 0.9 of the slots; returns (text, pairs)"""
    O = cqflibs.oracle()
    hb = qb + 8
    pool = FC.dna(60000, 77)
    keys = O.seq_keys([pool], k, hb)
    want = [(r, c) for r in SPECIAL_REMS for c in HARD_COUNTS]
    pairs, parts, used = {}, [], 0
    at = 2
    for r, c in want:
        while int(keys[at]) & 0xff != r or int(keys[at]) in pairs:
            at += 1
        pairs[int(keys[at])] = c
        used += len(O.encode_counter(r, c))
        parts.append(pool[at - 2:at + k + 2])      # the k-mer and two neighbours on either side
        at += k + 4
    filler = FC.dna(2000, 78)
    fkeys = O.seq_keys([filler], k, hb)
    n = 0
    while used < 0.9 * (1 << qb):
        x = int(fkeys[n])
        n += 1
        if x in pairs:
            continue
        pairs[x] = 1 + n % 3
        used += len(O.encode_counter(x & 0xff, pairs[x]))
    text = b">special\n" + b"N".join(parts) + b"\n>filler\n" + FC.wrap(filler[:n + k + 10], 60)
    assert 0.88 * (1 << qb) <= used <= 0.95 * (1 << qb)
    return text, sorted(pairs.items())


def run_hard_table(mk, k=31, seg=50, qb=10):
    """the hard table. shk_insert_counted takes a count in passes of 2^22, a rebuild of the table each, which is 8192 of
    them for 2^35: the entries of 2^32 - 2 and more are put into the oracle's table and imported, everything else is
    inserted on top of them with insert_counted"""
    text, pairs = hard_case(k, qb)
    big = [p for p in pairs if p[1] >= 1 << 22]
    assert len(big) == 4 * len(SPECIAL_REMS)
    ctx, table = ctx_for(mk, qb, k, seg, max_level_bits=2), dict(big)
    q = cqflibs.oracle().new(qb)
    for key, c in big:
        q.insert(key, c)
    ctx.import_blocks(q.blocks(), q.nelts(), q.ndistinct())
    q.free()
    rest = [p for p in pairs if p[1] < 1 << 22]
    for i in range(0, len(rest), 97):
        fill(ctx, table, rest[i:i + 97])
    qs, rec, track = ask(ctx, Model(k), text, True, table, min_count=128, what="hard table")
    assert int((track == CAP).sum()) >= 4 * len(SPECIAL_REMS)      # 2^32 - 2 is the cap itself; 2^32 - 1, 2^32 and 2^35 are capped
    assert qs["sum"] >= len(SPECIAL_REMS) * (1 << 35)
    ctx.close()


def stream_text(k):
    """fasta_cases.stream_text, and behind it headers that follow each other with no bases between them"""
    text, s = FC.stream_text(k)
    return text + b">three\n>four\r\n>five" + b"\n" + s[10:10 + k + 30] + b"\n"


def run_pieces(mk, k, seg, cuts_list, qb=10):
    """every list of cut positions: the pieces against the model, the concatenated tracks and the merged records against
    the text in one call"""
    text = stream_text(k)
    ctx, table = ctx_for(mk, qb, k, seg, max_level_bits=2), {}
    fill(ctx, table, half_of(text_keys(text, k, qb + 8)))
    _, one_rec, one_track = ask(ctx, Model(k), text, True, table, what="one call")
    for cuts in cuts_list:
        m = Model(k)
        got = [ask(ctx, m, text[a:b], i == 0, table, what="cuts %r piece %d" % (cuts, i))
               for i, (a, b) in enumerate(zip([0] + list(cuts), list(cuts) + [len(text)]))]
        assert np.array_equal(np.concatenate([g[2] for g in got]), one_track), cuts
        assert np.array_equal(merge_records([g[1] for g in got]), one_rec), cuts
    ctx.close()


def every_cut(k):
    n = len(stream_text(k))
    return [(c,) for c in range(1, n)] + [(120, 120), (0, 0), (n, n)]


def chosen_cuts(k, seg, names):
    _, cuts = FC.chosen_cuts(k, seg)
    n = len(stream_text(k))
    return [(cuts[name],) for name in names] + [(120, 120), (n - 12, n - 12), (n - 9, n - 3)]


def run_reader_contract(mk, k=31, seg=50, qb=11):
    """a query directly behind count_fasta calls (the pending placement is launched); no byte of the table and no
    counter changes; the answers do not depend on traveled marks set by lookup(mode=1)"""
    reads = b">a\n" + FC.wrap(FC.dna(400, 5), 60) + b">b\n" + FC.wrap(FC.dna(400, 5)[100:350], 60)
    text = b">q1\n" + FC.wrap(FC.dna(400, 5)[50:300], 70) + b">q2\n" + FC.wrap(FC.dna(120, 6), 70)
    ctx = ctx_for(mk, qb, k, seg, max_level_bits=2)
    ctx.count_fasta(reads[:333], first=True)
    ctx.count_fasta(reads[333:], first=False)
    uniq, cnt = np.unique(text_keys(reads, k, qb + 8), return_counts=True)
    table = {int(a): int(b) for a, b in zip(uniq, cnt)}
    first = ask(ctx, Model(k), text, True, table, what="directly behind count_fasta")
    assert first[0]["present"] > 0 and first[0]["solid"] > 0
    before, tb = ctx.blocks(), ctx.totals()
    exp = FC.Expect(qb)
    exp.insert(text_keys(reads, k, qb + 8))
    exp.check(ctx, "the table the query read")
    exp.free()
    ctx.lookup([int(x) for x in uniq[::3]], mode=1)
    marked = ctx.blocks()
    assert marked != before
    again = ask(ctx, Model(k), text, True, table, what="behind lookup(mode=1)")
    assert np.array_equal(again[2], first[2]) and np.array_equal(again[1], first[1])
    assert ctx.blocks() == marked
    ta = ctx.totals()
    assert all(getattr(ta, f) == getattr(tb, f) for f, _ in ta._fields_)
    ctx.close()


def run_independent_streams(mk, k=31, seg=50, qb=11):
    """count and query calls on one context interleave without seeing each other's stream"""
    X = b">x\n" + FC.wrap(FC.dna(500, 8), 60)
    Y = b">y1\n" + FC.wrap(FC.dna(500, 8)[200:420], 50) + b">y2\n" + FC.wrap(FC.dna(90, 9), 50)
    cx, cy = 287, 133      # (both inside a run, more than k - 1 bases behind its start)
    plain = ctx_for(mk, qb, k, seg, max_level_bits=2)
    plain.count_fasta(X[:cx], first=True)
    plain.count_fasta(X[cx:], first=False)
    ctx = ctx_for(mk, qb, k, seg, max_level_bits=2)
    ctx.count_fasta(X[:cx], first=True)
    uniq, cnt = np.unique(text_keys(X[:cx], k, qb + 8), return_counts=True)
    table = {int(a): int(b) for a, b in zip(uniq, cnt)}
    my = Model(k)
    ask(ctx, my, Y[:cy], True, table, what="query between two count pieces")
    ctx.count_fasta(X[cx:], first=False)
    assert ctx.blocks() == plain.blocks(), "the count stream saw the query"
    uniq, cnt = np.unique(text_keys(X, k, qb + 8), return_counts=True)
    table = {int(a): int(b) for a, b in zip(uniq, cnt)}
    ask(ctx, my, Y[cy:], False, table, what="the query stream goes on behind a count piece")
    ctx.close()
    plain.close()


def run_without_track(mk, k=31, seg=50, qb=10):
    text = stream_text(k)
    ctx, table = ctx_for(mk, qb, k, seg, max_level_bits=2), {}
    fill(ctx, table, half_of(text_keys(text, k, qb + 8)))
    a = ask(ctx, Model(k), text, True, table, want_track=True)
    b = ask(ctx, Model(k), text, True, table, want_track=False)
    assert np.array_equal(a[1], b[1]) and a[0] == b[0]
    ctx.close()


def run_device_track(mk, dev_u32, k=31, seg=50, qb=10):
    """a track in device memory, at 64-byte alignment and 20 bytes off it (the kernel stores whole 64-byte groups where it
    can): the entries of the piece and nothing around them. dev_u32(n) -> (pointer to n words the library can write, read())"""
    text = stream_text(k)
    ctx, table = ctx_for(mk, qb, k, seg, max_level_bits=2), {}
    fill(ctx, table, half_of(text_keys(text, k, qb + 8)))
    want_qs, want_rec, want_track = Model(k).expect(text, table, qb + 8, 2)
    n = len(want_track)
    for off in (0, 5):
        ptr, read = dev_u32(n + 64)
        assert ptr % 64 == 0
        rc, nrec, qs, rec, _ = raw_query(ctx, text, True, 2, n, 64, dev_track=ptr + 4 * (16 + off))
        assert rc == 0 and qs == want_qs and np.array_equal(rec[:nrec], want_rec)
        got = read()
        assert np.array_equal(got[16 + off:16 + off + n], want_track), off
        assert not got[:16 + off].any() and not got[16 + off + n:].any(), off
    ctx.close()


def run_default_segment(mk, k=47, qb=12):
    """SHK_FASTA_SEGMENT unset, one run of 5 kb"""
    text = b">five kb\n" + FC.wrap(FC.dna(5000, 12), 80)
    ctx, table = ctx_for(mk, qb, k, None, max_level_bits=3), {}
    fill(ctx, table, half_of(text_keys(text, k, qb + 8)))
    ask(ctx, Model(k), text, True, table, what="default segment")
    ctx.close()


def raw_query(ctx, piece, first, min_count, track_cap, rec_cap, on_device=False, text_bytes=None, dev_track=None):
    """the C call itself with capacities of the caller's choosing; returns (rc, nrec, statistics, records, track).
    dev_track: a pointer the library writes the track through as device memory (the returned track is then untouched)"""
    import shk
    if on_device:
        ptr, n = C.c_void_p(int(piece)), int(text_bytes)
    else:
        buf = (C.c_char * max(len(piece), 1)).from_buffer_copy(bytes(piece) or b"\0")
        ptr, n = C.cast(buf, C.c_void_p), len(piece)
    track = np.full(max(track_cap, 1), 0x55555555, dtype=np.uint32)
    rec = np.zeros((max(rec_cap, 1), 4), dtype=np.uint64)
    nrec, qs = C.c_uint32(0), shk.QueryStats()
    rc = ctx.L.shk_query_fasta(ctx.h, ptr, 1 if on_device else 0, n, 1 if first else 0, min_count,
                               C.c_void_p(dev_track if dev_track is not None else track.ctypes.data), track_cap, 0 if dev_track is None else 1,
                               C.c_void_p(rec.ctypes.data), rec_cap, C.byref(nrec), C.byref(qs))
    return rc, nrec.value, qs.as_dict(), rec, track


def run_errors(mk, dev_bytes, k=31, seg=50, qb=10):
    """every error of the contract; behind each the query stream goes on from where it was.
    dev_bytes(b) -> (pointer the library can read, keep-alive)"""
    text = stream_text(k)
    nbases = Model(k).feed(text)[0]["bases"]
    nheaders = Model(k).feed(text)[0]["records"]
    keys = text_keys(text, k, qb + 8)
    head, rest = text[:100], text[100:]

    def case(**kw):
        ctx, table = ctx_for(mk, qb, k, seg, max_level_bits=2, **kw), {}
        fill(ctx, table, half_of(keys))
        m = Model(k)
        ask(ctx, m, head, True, table, what="the piece in front of the error")
        return ctx, table, m

    def goes_on(ctx, table, m, what):
        for i in range(0, len(rest), 70):
            ask(ctx, m, rest[i:i + 70], False, table, what=what)
        ctx.close()

    # text_bytes > max_batch_bytes
    ctx, table, m = case(text_cap=256)
    assert raw_query(ctx, rest, False, 2, len(rest), 64)[0] == -7
    goes_on(ctx, table, m, "behind text_bytes > max_batch_bytes")
    # a capacity limit of shk_count_fasta: more segments than max_batch_reads
    with FC.segment(16):
        ctx = mk(qb=qb, k=k, max_batch_bytes=4096, max_batch_keys=4096, max_batch_reads=8, max_level_bits=2)
    table, m = {}, Model(k)
    fill(ctx, table, half_of(keys))
    ask(ctx, m, head, True, table)
    assert raw_query(ctx, rest, False, 2, len(rest), 64)[0] == -7
    goes_on(ctx, table, m, "behind more segments than max_batch_reads")
    # ... more k-mers than max_batch_keys
    with FC.segment(seg):
        ctx = mk(qb=qb, k=k, max_batch_bytes=4096, max_batch_keys=len(keys) // 2, max_level_bits=2)
    table, m = {}, Model(k)
    fill(ctx, table, half_of(keys)[:len(keys) // 2 - 1])
    ask(ctx, m, head, True, table)
    assert raw_query(ctx, rest, False, 2, len(rest), 64)[0] == -7
    goes_on(ctx, table, m, "behind more k-mers than max_batch_keys")
    # track_cap smaller than the piece's bases; rec_cap < 1 + records: *nrec says how many, and the repeated call answers
    ctx, table, m = case()
    rest_bases = nbases - Model(k).feed(head)[0]["bases"]
    rc, _, _, _, track = raw_query(ctx, rest, False, 2, rest_bases - 1, 64)
    assert rc == -7 and int((track != 0x55555555).sum()) == 0
    rest_headers = nheaders - Model(k).feed(head)[0]["records"]
    assert rest_headers >= 3
    rc, nrec, _, _, _ = raw_query(ctx, rest, False, 2, rest_bases, rest_headers)
    assert (rc, nrec) == (-7, 1 + rest_headers)
    want_qs, want_rec, want_track = Model(k).expect(text, table, qb + 8, 2)      # (the whole text: head went in before)
    rc, nrec, qs, rec, track = raw_query(ctx, rest, False, 2, rest_bases, 1 + rest_headers)
    assert (rc, nrec) == (0, 1 + rest_headers)
    assert np.array_equal(track[:rest_bases], want_track[nbases - rest_bases:])
    assert np.array_equal(merge_records([ctx.query_fasta(head, first=True)[1], rec[:nrec]]), want_rec)
    fresh = ctx_for(mk, qb, k, seg, max_level_bits=2)
    fill(fresh, {}, half_of(keys))
    fresh.query_fasta(head, first=True)
    rc2, nrec2, qs2, rec2, track2 = raw_query(fresh, rest, False, 2, rest_bases, 1 + rest_headers)
    assert (rc2, nrec2, qs2) == (0, nrec, qs) and np.array_equal(rec2, rec) and np.array_equal(track2, track)
    fresh.close()
    ctx.close()
    # device text that is not 16-byte aligned (aligned device text works); batches prepared and not yet counted
    ctx, table, m = case(text_cap=4096)
    ptr, keep = dev_bytes(b"\n" * 16 + rest)
    assert raw_query(ctx, ptr + 1, False, 2, len(rest), 64, on_device=True, text_bytes=len(rest))[0] == -1
    fq = b"@r\n%s\n+\n%s\n" % (FC.dna(60, 1), b"I" * 60)
    ctx.prepare_chunks(fq, [0], [len(fq)])
    assert raw_query(ctx, rest, False, 2, len(rest), 64)[0] == -7
    ctx.count_prepared()
    for x in cqflibs.oracle().seq_keys([FC.dna(60, 1)], k, qb + 8).tolist():
        table[x] = table.get(x, 0) + 1
    want_qs, want_rec, want_track = m.expect(rest, table, qb + 8, 2)
    rc, nrec, qs, rec, track = raw_query(ctx, ptr + 16, False, 2, len(rest), 64, on_device=True, text_bytes=len(rest))
    assert rc == 0 and qs == want_qs and np.array_equal(rec[:nrec], want_rec) and np.array_equal(track[:qs["bases"]], want_track)
    ctx.close()
    # a sharded context
    with FC.segment(seg):
        sh = mk(qb=12, k=k, max_batch_bytes=4096, max_batch_keys=4096, num_shards=2, shard_index=1)
    assert raw_query(sh, text, True, 2, len(text), 64)[0] == -1
    sh.close()


# ---------------------------------------------------------------- command line
def cli_case():
    """(reads as FASTA, the queried file of three records, k, qb)"""
    g = FC.dna(900, 21)
    reads = b"".join(b">r%d\n%s" % (i, FC.wrap(g[a:a + 150], 60)) for i, a in enumerate(range(0, 700, 25)))
    fa = (b">contig_1 first of three\n" + FC.wrap(g[40:400], 70) + b">contig_2\tfrom the end\r\n" + FC.wrap(g[600:880], 70) +
          b">foreign\n" + FC.wrap(FC.dna(200, 22), 70))
    return reads, fa, 31, 12


def cli_expected(fa, reads, k, qb, smin, path):
    """(the report python -m shk.query --records must print, the track it must write)"""
    from shk.query import format_report
    uniq, cnt = np.unique(text_keys(reads, k, qb + 8), return_counts=True)
    table = {int(a): int(b) for a, b in zip(uniq, cnt)}
    qs, rec, track = Model(k).expect(fa, table, qb + 8, smin)
    names = ["contig_1", "contig_2", "foreign"]
    assert len(rec) == 4 and rec[0][0] == 0
    rows = [(n,) + tuple(int(x) for x in r) for n, r in zip(names, rec[1:])]
    return format_report(qs, k, smin, path, rows), track


def report_case():
    qs = {"records": 3, "bases": 1000, "breaks": 12, "kmers": 900, "present": 800, "solid": 640, "sum": 11106}
    rows = [("a", 500, 500, 400, 8000), ("b", 400, 300, 240, 3108), ("c", 0, 0, 0, 0), ("d", 10, 0, 0, 0)]
    want = ("records\t3\nbases\t1000\nk-mers\t900\nagainst\treads.cqf\npresent\t800\t88.89%\ncount>=3\t640\t71.11%\n"
            "mean count\t12.34\nQV\t24.21\n")
    want_rows = ("#name\tk-mers\tpresent\tsolid\tmean\tQV\na\t500\t500\t400\t16.00\tinf\nb\t400\t300\t240\t7.77\t20.34\n"
                 "c\t0\t0\t0\t0.00\tnan\nd\t10\t0\t0\t0.00\t0.00\n")
    return qs, rows, want, want_rows
