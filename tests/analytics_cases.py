"""Analytics on resident tables: shk_spectrum, shk_inner_product, shk_magnitude, shk_intersect. Shared by the emulator
tests and the GPU tests of tests/test_analytics.py.

mk_ctx(**kw) -> context. Every case checks against the DEFINITION, computed in Python from (key, count) lists (with
`ref` false that is all it does); with `ref` true it also compares with the compiled reference's qf_inner_product,
qf_magnitude and qf_intersect (oracle/_ref, gqf.c:2707-2763) on the same pairs. The reference iterates its SECOND operand
and looks the keys up in the first, and its iterator ends early inside the overflow tail (see shk_dump)."""
import collections
import ctypes as C
import io
import json
import math
import os
import random
import struct

import cqflibs
import f4_scenarios as F

K = 21
M64 = (1 << 64) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_ARG, ERR_CORRUPT = -1, -5
BINS = [1, 2, 7, 256, 300]           # 1 and 2 clamp; 300 crosses the border between the LDS bins and the global ones
_INTERSECT = "_Z12qf_intersectP15quotient_filterS0_S0_"     # gqf.h never declares it: it is exported under its C++ name


def _mk(mk_ctx, qb, **kw):
    return mk_ctx(qb=qb, k=K, max_batch_bytes=1 << 16, max_batch_keys=1 << 14, **kw)


def _load(mk_ctx, qb, kc):
    """a context holding exactly these pairs: the C restatement's canonical table, imported"""
    F.fits(qb, kc)
    q = F.build(cqflibs.oracle(), qb, kc)
    ctx = _mk(mk_ctx, qb)
    ctx.import_blocks(q.blocks(), q.nelts(), q.ndistinct())
    q.free()
    return ctx


def _spectrum_of(pairs, nbins):
    cnt = collections.Counter(c for _, c in pairs)
    hist = [0] * nbins
    for c, n in cnt.items():
        hist[min(c, nbins) - 1] += n
    cs = [c for _, c in pairs]
    return hist, {"distinct": len(cs), "total": sum(cs) & M64, "sumsq": sum(c * c for c in cs) & M64, "max_count": max(cs, default=0)}


def _check_spectrum(ctx, pairs=None):
    pairs = ctx.dump() if pairs is None else pairs
    for nb in BINS:
        assert ctx.spectrum(nb) == _spectrum_of(pairs, nb), nb
    assert ctx.spectrum(0) == ([], _spectrum_of(pairs, 1)[1])      # hist = NULL, nbins = 0: the totals only
    return _spectrum_of(pairs, 1)[1]


# ---------------------------------------------------------------- the tables
def t_plain(rng):
    return 12, F.pairs(rng, 12, 1000, 1 << 20)


def t_saturated(rng):
    return 12, F.pairs(rng, 12, 900, 1 << 16, cluster=(2000, 300))      # offsets saturate at 255: the big image


def t_tail(rng):
    return 10, F.pairs(rng, 10, 80, 300, cluster=(1000, 24))            # quotients 1000..1023: runs in the overflow tail


def t_wrap(rng):
    return 10, F.pairs(rng, 10, 40, 1 << 35)                            # sumsq wraps mod 2^64


def t_empty(rng):
    return 10, []


TABLES = [t_plain, t_saturated, t_tail, t_wrap, t_empty]


def run_spectrum(mk_ctx, table):
    """spectrum == a Counter over the dump, for every bin count; the dump == the pairs put in"""
    qb, kc = table(random.Random(41))
    ctx = _load(mk_ctx, qb, kc)
    d = ctx.dump()
    assert d == sorted(kc)
    tot = _check_spectrum(ctx, d)
    if table is t_wrap:
        assert sum(c * c for _, c in kc) > M64, "scenario must wrap"
    if table is t_tail:
        assert len(ctx.dump(ref_iterator_end=True)) < len(kc), "scenario must reach into the tail"
    assert tot["distinct"] == ctx.totals().ndistinct and tot["total"] == ctx.totals().nelts
    ctx.close()


def run_spectrum_device(mk_ctx):
    """on_device != 0: the histogram is built in the caller's device buffer (whatever it held before) and stays there;
    the words behind its nbins are not touched"""
    qb, kc = t_plain(random.Random(41))
    ctx = _load(mk_ctx, qb, kc)
    for nb in (7, 300):
        ptr, read = ctx.dev_u64([0xDEADBEEF] * (nb + 2))
        tot = ctx.spectrum_into(ptr, nb)
        got = read()
        assert (got[:nb], tot) == _spectrum_of(kc, nb) and got[nb:] == [0xDEADBEEF] * 2
    ctx.close()


def golden_build(i=0):
    """(cfg, text, chunk offsets, chunk lengths, path of the .cqf) of a FASTQ build of tests/golden/fastq_builds.json"""
    fx = json.load(open(os.path.join(GOLDEN, "fastq_builds.json")))
    b = fx["builds"][i]
    c = b["cfg"]
    text, offs, lens = b"", [], []
    for f in c["files"]:
        base = len(text)
        data = open(os.path.join(GOLDEN, f), "rb").read()
        text += data
        sizes = fx["chunks"].get("%s:%d:%d" % (f, c["ps"], c["ov"]))
        assert sizes or len(data) <= c["ps"]          # (not listed: a file of one part)
        for n in sizes or [len(data)]:
            offs.append(base)
            lens.append(n)
            base += n
        assert base == len(text)
    return c, text, offs, lens, os.path.join(GOLDEN, b["cqf"])


def run_spectrum_fresh(mk_ctx):
    """the spectrum as the FIRST reader of a freshly counted filter (its placement is still pending: the call launches
    it, once) == the Counter of the dump of the golden .cqf of the same build"""
    c, text, offs, lens, cqf = golden_build(4)
    assert c["nd"] == 0
    ctx = mk_ctx(qb=c["qb"], k=c["k"], max_batch_bytes=len(text) + 1024, max_batch_keys=1 << 14)
    ctx.profile(True)
    ctx.count_chunks(text, offs, lens)
    places = lambda: ctx.profile_get().get("k_region_place", (0, 0.0))[0]     # noqa: E731
    assert places() == 0
    gold = mk_ctx(qb=c["qb"], k=c["k"], max_batch_bytes=1 << 16, max_batch_keys=1 << 14)
    gold.import_cqf(cqf)
    want = gold.dump()
    assert ctx.spectrum(256) == _spectrum_of(want, 256)
    assert places() == 1
    assert ctx.spectrum(300) == _spectrum_of(want, 300)
    assert ctx.dump() == want and places() == 1
    assert (ctx.totals().nelts, ctx.totals().ndistinct) == cqf_header_counts(cqf)
    for x in (ctx, gold):
        x.close()


def run_shards(mk_ctx, nshards):
    """the shards' histograms, totals and inner products add up to the single table's (max_count: the maximum)"""
    qb = 12
    rng = random.Random(43 + nshards)
    a = F.pairs(rng, qb, 900, 1 << 12, cluster=(500, 3000))     # a cluster across the shard borders
    b = [(k, c + 2) for k, c in a[::3]] + F.pairs(rng, qb, 300, 1 << 12)
    b = list({k: c for k, c in b}.items())
    F.fits(qb, a)
    F.fits(qb, b)
    whole_a, whole_b = _load(mk_ctx, qb, a), _load(mk_ctx, qb, b)
    per = (1 << qb) // nshards
    hist, tot, dot = [0] * 300, collections.Counter(), 0
    for s in range(nshards):
        ca, cb = (_mk(mk_ctx, qb, shard_index=s, num_shards=nshards) for _ in range(2))
        for ctx, kc in ((ca, a), (cb, b)):
            mine = [(k, x) for k, x in kc if (k >> 8) // per == s]
            ctx.insert_counted([k for k, _ in mine], [x for _, x in mine])
        h, t = ca.spectrum(300)
        assert (h, t) == _spectrum_of(ca.dump(), 300)
        hist = [x + y for x, y in zip(hist, h)]
        for name in ("distinct", "total", "sumsq"):
            tot[name] = (tot[name] + t[name]) & M64
        tot["max_count"] = max(tot["max_count"], t["max_count"])
        dot = (dot + ca.inner_product(cb)) & M64
        assert ca.inner_product(ca) == t["sumsq"]
        ca.close()
        cb.close()
    assert (hist, dict(tot)) == whole_a.spectrum(300) == _spectrum_of(a, 300)
    assert dot == whole_a.inner_product(whole_b) == _dot(a, b)
    whole_a.close()
    whole_b.close()


# ---------------------------------------------------------------- two filters
def _dot(a, b):
    da = dict(a)
    return sum(da[k] * c for k, c in b if k in da) & M64


def _common(a, b):
    """{(key, count_b)}: what qf_intersect(a, b, .) inserts"""
    da = dict(a)
    return sorted((k, c) for k, c in b if k in da)


def _ref_handles(qb, *kcs):
    lib = cqflibs.ref()
    lib.L.qf_inner_product.restype = C.c_uint64
    lib.L.qf_inner_product.argtypes = [C.c_void_p, C.c_void_p]
    lib.L.qf_magnitude.restype = C.c_uint64
    lib.L.qf_magnitude.argtypes = [C.c_void_p]
    f = getattr(lib.L, _INTERSECT)
    f.restype, f.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p]
    return lib, [F.build(lib, qb, kc) for kc in kcs]      # (a RefQF* is a QF*: the QF is its first member)


def _ref_intersect(lib, qb, qa, qb_):
    r = lib.new(qb)
    getattr(lib.L, _INTERSECT)(qa.h, qb_.h, r.h)
    blocks = r.blocks()
    r.free()
    return blocks


def p_plain(rng):
    """the qb-12 pair: b = every second key of a with count + 3, plus fresh keys"""
    a = F.pairs(rng, 12, 600, 1 << 16)
    b = [(k, c + 3) for k, c in a[::2]] + F.pairs(rng, 12, 500, 1 << 16)
    return 12, a, list({k: c for k, c in b}.items())


def p_wrap(rng):
    a = F.pairs(rng, 10, 40, 1 << 35)
    return 10, a, [(k, c + 1) for k, c in a]


def p_tail(rng):
    a = F.pairs(rng, 10, 80, 300, cluster=(1000, 24))
    return 10, a, [(k, c + 1) for k, c in a]


def p_dense(rng):
    """one long cluster: the big LDS image (the pair of test_merge_matches_reference_qf_merge)"""
    a = F.pairs(rng, 14, 1500, 1 << 12, cluster=(3000, 4000))
    b = [(k, c + 3) for k, c in a[::2]] + F.pairs(rng, 14, 800, 1 << 12, cluster=(3500, 4000))
    return 14, a, list({k: c for k, c in b}.items())


def _visible(ctx):
    """the keys of ctx's table that the reference's iterator reaches (shk_dump is checked against it elsewhere)"""
    return ctx.dump(ref_iterator_end=True)


def run_inner_product(mk_ctx, pair, ref):
    qb, a, b = pair(random.Random(47))
    ca, cb = _load(mk_ctx, qb, a), _load(mk_ctx, qb, b)
    tail = pair is p_tail
    # the definition: both orders, every entry
    assert ca.inner_product(cb) == cb.inner_product(ca) == _dot(a, b)
    for ctx, kc in ((ca, a), (cb, b)):
        sq = sum(c * c for _, c in kc)
        assert ctx.inner_product(ctx) == ctx.spectrum(0)[1]["sumsq"] == sq & M64
        if not tail:
            assert ctx.magnitude() == int(math.sqrt(float(sq & M64)))
    if pair is p_wrap:
        assert sum(dict(a)[k] * c for k, c in b) > M64, "scenario must wrap"
    # the iterator's early end: entries of the ITERATED operand behind it do not contribute, the lookups see everything
    va, vb = _visible(ca), _visible(cb)
    assert (len(vb) < len(b)) == tail and (len(va) < len(a)) == tail
    assert ca.inner_product(cb, ref_iterator_end=True) == _dot(a, vb)
    assert cb.inner_product(ca, ref_iterator_end=True) == _dot(b, va)
    if tail:
        assert _dot(a, vb) != _dot(a, b), "scenario must make the two differ"
    if ref:
        lib, (qa, qb_) = _ref_handles(qb, a, b)
        assert ca.inner_product(cb, ref_iterator_end=True) == lib.L.qf_inner_product(qa.h, qb_.h)
        assert cb.inner_product(ca, ref_iterator_end=True) == lib.L.qf_inner_product(qb_.h, qa.h)
        assert ca.magnitude(ref_iterator_end=True) == lib.L.qf_magnitude(qa.h)
        assert cb.magnitude(ref_iterator_end=True) == lib.L.qf_magnitude(qb_.h)
        if not tail:
            assert ca.inner_product(cb) == lib.L.qf_inner_product(qa.h, qb_.h)
        qa.free()
        qb_.free()
    ca.close()
    cb.close()


def run_inner_product_edges(mk_ctx, ref):
    """each operand empty, both empty; mismatched qb"""
    qb, a, _ = p_plain(random.Random(47))
    ca, e1, e2 = _load(mk_ctx, qb, a), _mk(mk_ctx, qb), _mk(mk_ctx, qb)
    for end in (False, True):
        assert ca.inner_product(e1, end) == e1.inner_product(ca, end) == e1.inner_product(e2, end) == e1.inner_product(e1, end) == 0
        assert e1.magnitude(end) == 0
    other = _mk(mk_ctx, qb - 1)
    for f in (lambda: ca.inner_product(other), lambda: other.inner_product(ca), lambda: e1.intersect_from(ca, other),
              lambda: other.intersect_from(ca, e1)):
        try:
            f()
        except Exception as e:
            assert getattr(e, "code", None) == ERR_ARG
        else:
            raise AssertionError("mismatched qb accepted")
    if ref:
        lib, (qa, qe) = _ref_handles(qb, a, [])
        assert lib.L.qf_inner_product(qa.h, qe.h) == lib.L.qf_inner_product(qe.h, qa.h) == lib.L.qf_inner_product(qe.h, qe.h) == 0
        qa.free()
        qe.free()
    for x in (ca, e1, e2, other):
        x.close()


def run_intersect(mk_ctx, pair, ref):
    qb, a, b = pair(random.Random(47))
    ca, cb = _load(mk_ctx, qb, a), _load(mk_ctx, qb, b)
    tail = pair is p_tail
    dst = _load(mk_ctx, qb, F.pairs(random.Random(53), qb, 50, 300))      # a dst that held other entries before
    fresh = _mk(mk_ctx, qb)
    if ref:
        lib, (qa, qb_) = _ref_handles(qb, a, b)
    for x, y, kx, ky in ((ca, cb, a, b), (cb, ca, b, a)):
        # every entry: the definition, as the C restatement's table
        want = _common(kx, ky)
        st = dst.intersect_from(x, y)
        q = F.build(cqflibs.oracle(), qb, want)
        assert dst.blocks() == q.blocks()
        q.free()
        assert dst.dump() == want
        assert (st["new_distinct"], st["kmers"]) == (len(want), sum(c for _, c in want))
        t = dst.totals()
        assert (t.ndistinct, t.nelts) == (st["new_distinct"], st["kmers"])
        fresh.intersect_from(x, y)
        assert fresh.blocks() == dst.blocks()
        # the iterator's early end
        vis = _visible(y)
        assert (len(vis) < len(ky)) == tail
        st = dst.intersect_from(x, y, ref_iterator_end=True)
        assert dst.dump() == _common(kx, vis) and st["new_distinct"] == len(_common(kx, vis))
        if tail:
            assert _common(kx, vis) != want, "scenario must make the two differ"
        if ref:
            rx, ry = (qa, qb_) if x is ca else (qb_, qa)
            assert dst.blocks() == _ref_intersect(lib, qb, rx, ry)
    for f in (lambda: ca.intersect_from(ca, cb), lambda: cb.intersect_from(ca, cb)):
        try:
            f()
        except Exception as e:
            assert getattr(e, "code", None) == ERR_ARG
        else:
            raise AssertionError("dst is an operand: accepted")
    # an empty operand gives an empty table
    empty = _mk(mk_ctx, qb)
    for x, y in ((ca, empty), (empty, ca)):
        st = dst.intersect_from(x, y)
        assert dst.blocks() == empty.blocks() and (st["kmers"], st["new_distinct"]) == (0, 0)
    if ref:
        qa.free()
        qb_.free()
    for x in (ca, cb, dst, fresh, empty):
        x.close()


def run_corrupt(mk_ctx):
    """a table whose occupieds and runends disagree: SHK_ERR_CORRUPT from every call, and nothing written"""
    qb, a, b = p_plain(random.Random(47))
    F.fits(qb, a)
    q = F.build(cqflibs.oracle(), qb, a)
    blocks = bytearray(q.blocks())
    q.free()
    free_q = next(x for x in range(64) if not (blocks[1 + x // 8] >> (x % 8)) & 1)
    blocks[1 + free_q // 8] |= 1 << (free_q % 8)          # an occupied bit without a run
    bad, good, dst = _mk(mk_ctx, qb), _load(mk_ctx, qb, b), _load(mk_ctx, qb, b[:40])
    bad.import_blocks(bytes(blocks))
    before = dst.blocks()
    for f in (lambda: bad.spectrum(16), lambda: bad.inner_product(good), lambda: good.inner_product(bad),
              lambda: dst.intersect_from(bad, good), lambda: dst.intersect_from(good, bad)):
        try:
            f()
        except Exception as e:
            assert getattr(e, "code", None) == ERR_CORRUPT
        else:
            raise AssertionError("corrupt table accepted")
    assert dst.blocks() == before and dst.dump() == sorted(b[:40])
    for x in (bad, good, dst):
        x.close()


# ---------------------------------------------------------------- host pieces
def cqf_header_counts(path):
    with open(path, "rb") as f:
        hdr = f.read(128)
    return struct.unpack_from("<QQ", hdr, 88)      # nelts, ndistinct (gqf.h:62-77)


def run_cli(main, extra):
    """python -m shk.spectrum on a golden .cqf prints the F1 / F0 of that file's header"""
    _, _, _, _, cqf = golden_build(1)
    out = io.StringIO()
    assert main([cqf, "-k", "28", "--bins", "64"] + extra, out=out) == 0
    check_cli_output(out.getvalue(), cqf)


def check_cli_output(text, cqf):
    nelts, ndistinct = cqf_header_counts(cqf)
    lines = text.splitlines()
    assert lines[0] == "F1\t%d" % nelts and lines[1] == "F0\t%d" % ndistinct
    bins = [l.split("\t") for l in lines[2:-1]]
    assert bins and all(n.startswith("f") and int(v) > 0 for n, v in bins)
    assert sum(int(v) for _, v in bins) == ndistinct
    assert lines[-1].startswith("suggested: -N %d -n " % nelts)
