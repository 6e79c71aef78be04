"""What does a filter know about these reads, read by read -- and which of them to keep?

    python -m shk.reads (-i LIST -f {g,b,f} | FILE ...) -k K --against TABLE.cqf [--min-count C]
           [--min-solid F] [--max-solid F] [--min-present F] [--max-present F]
           [--min-median M] [--max-median M] [--min-kmers N] [--keep-short]
           [-o KEPT.fq] [--rejected REST.fq] [--table OUT.tsv] [--mask OUT.u8]
           [--parts-per-call P] [--part-size BYTES] [--lib PATH]

The reads go through the chunker a build uses (host/fastq_chunker.cpp: plain, gzip or bzip2, one file or a list) and
through shk_query_reads against a context that has imported TABLE.cqf; the filter stays untouched. Per read the device
answers the number of its k-mers, how many the table holds at all (present) and at least C times (solid), and the
smallest, largest and lower median count. TABLE.cqf built from a contaminant, host or organelle genome and
--max-present 0.2 is a decontamination filter (--min-present 0.5: a bait); the reads' own filter with --min-median 2
--max-median 500 drops reads that are mostly error or mostly repeat.

A read is kept when it passes every rule given; the fractions are solid / k-mers and present / k-mers. A read with fewer
than max(1, --min-kmers) k-mers passes no rule and is rejected, unless --keep-short keeps it. -o and --rejected receive
the records byte for byte as in the input, in the order the chunker hands out the parts (a single file: the file's order);
together they hold every input byte exactly once (bytes of a part in which the front end finds no read at all go to
--rejected). --table writes one line per read: name, sequence length, k-mers, present, solid, min, median, max, sum;
--mask one byte per read, 1 for kept, so that the mates of paired files can be combined outside."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

from . import QUERY_NONE, Context
from .count import _host
from .estimate import OVERHEAD, guess_format
from .spectrum import cqf_geometry

RULES = ("min_solid", "max_solid", "min_present", "max_present", "min_median", "max_median")


def select(rec, min_solid=None, max_solid=None, min_present=None, max_present=None, min_median=None, max_median=None,
           min_kmers=0, keep_short=False):
    """the reads to keep, as a boolean array: a function of the records (an array with shk_read_record's fields) and
    the rules alone. A rule that is None is not in force."""
    kmers = rec["kmers"].astype(np.float64)
    short = rec["kmers"] < max(1, int(min_kmers))
    with np.errstate(divide="ignore", invalid="ignore"):
        solid, present = rec["solid"] / kmers, rec["present"] / kmers
    keep = np.ones(len(rec), dtype=bool)
    if min_solid is not None:
        keep &= solid >= min_solid
    if max_solid is not None:
        keep &= solid <= max_solid
    if min_present is not None:
        keep &= present >= min_present
    if max_present is not None:
        keep &= present <= max_present
    if min_median is not None:
        keep &= rec["median"] >= min_median
    if max_median is not None:
        keep &= rec["median"] <= max_median
    return np.where(short, bool(keep_short), keep)


def rules_text(rules, min_kmers=0, keep_short=False):
    """the rules in force, one word each, in a fixed order"""
    words = ["%s=%g" % (name.replace("_", "-"), rules[name]) for name in RULES if rules.get(name) is not None]
    words.append("min-kmers=%d" % max(1, int(min_kmers)))
    if keep_short:
        words.append("keep-short")
    return " ".join(words)


def _pct(n, of):
    return 100.0 * n / of if of else 0.0


def format_report(stats, kept, k, min_count, path, rules, min_kmers=0, keep_short=False):
    """the report as text, a function of its numbers alone. stats: the summed shk_reads_stats of the calls"""
    n = stats["kmers"]
    lines = ["reads\t%d" % stats["reads"], "kept\t%d\t%.2f%%" % (kept, _pct(kept, stats["reads"])), "k-mers\t%d" % n,
             "against\t%s" % path, "present\t%d\t%.2f%%" % (stats["present"], _pct(stats["present"], n)),
             "count>=%d\t%d\t%.2f%%" % (min_count, stats["solid"], _pct(stats["solid"], n)),
             "rules\t%s" % rules_text(rules, min_kmers, keep_short)]
    return "\n".join(lines) + "\n"


def record_bounds(buf, ext, chunk_off, chunk_len):
    """[start, end) of every read's four-line record in the text: a record begins at its header line -- the first record
    of a chunk at the chunk's first byte -- and ends where the next record of its chunk begins, the last one at the
    chunk's end. From the newline positions and the extents of the sequence lines; nothing per read runs in Python."""
    n = len(ext)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    nl = np.flatnonzero(buf == 10)
    seq = ext["seq_off"].astype(np.int64)
    chunk = ext["chunk"].astype(np.int64)
    off, ln = np.asarray(chunk_off, dtype=np.int64), np.asarray(chunk_len, dtype=np.int64)
    # the header's line feed is the byte in front of the sequence line; the header begins behind the line feed before that
    at = np.searchsorted(nl, seq, side="left") - 2
    starts = np.where(at >= 0, nl[np.maximum(at, 0)] + 1, 0)
    first = np.ones(n, dtype=bool)
    first[1:] = chunk[1:] != chunk[:-1]
    starts = np.where(first, off[chunk], starts)
    ends = np.empty(n, dtype=np.int64)
    ends[:-1] = starts[1:]
    last = np.ones(n, dtype=bool)
    last[:-1] = first[1:]
    ends = np.where(last, off[chunk] + ln[chunk], ends)
    return starts, ends


def byte_mask(nbytes, starts, ends):
    """the bytes of the ranges [starts[i], ends[i]) as a boolean array (the ranges do not overlap)"""
    d = np.zeros(nbytes + 1, dtype=np.int32)
    np.add.at(d, starts, 1)
    np.add.at(d, ends, -1)
    return np.cumsum(d[:-1]) > 0


def names_of(buf, starts):
    """the first word behind the '@' of every record's header line"""
    out = []
    raw = buf.tobytes()
    for s in starts.tolist():
        e = s + 1
        while e < len(raw) and raw[e] not in b" \t\r\n":
            e += 1
        out.append(raw[s + 1:e].decode("latin-1"))
    return out


def parts_of(files, fmt, parts_per_call, part_size):
    """the files' parts as the chunker hands them out, `parts_per_call` per yield: (text, offsets, lengths)"""
    H = _host()
    arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
    bh = H.shkh_batch_open(arr, len(files), {"f": 0, "g": 1, "b": 2}[fmt], part_size, OVERHEAD)
    if not bh:
        raise IOError("cannot open the input files")
    try:
        done = False
        while not done:
            text, offs, lens = bytearray(), [], []
            while len(offs) < parts_per_call:
                p, n = C.c_void_p(), C.c_uint64()
                r = H.shkh_batch_next(bh, C.byref(p), C.byref(n))
                if r < 0:
                    raise IOError("Error: Wrong input file!")
                if r == 0:
                    done = True
                    break
                offs.append(len(text))
                lens.append(n.value)
                text += C.string_at(p.value, n.value)
                H.shkh_free(p)
            if offs:
                yield bytes(text), offs, lens
    finally:
        H.shkh_batch_close(bh)


def run(ctx, files, fmt, parts_per_call, part_size, min_count, rules, min_kmers, keep_short, median, kept_out=None,
        rest_out=None, table_out=None, mask_out=None):
    """every part through ctx; writes what is asked for and returns (summed statistics, reads kept)"""
    tot = {key: 0 for key in ("reads", "kmers", "present", "solid", "sum")}
    nkept = 0
    want_ext = any(o is not None for o in (kept_out, rest_out, table_out))
    for text, offs, lens in parts_of(files, fmt, parts_per_call, part_size):
        rs, rec, ext, _ = ctx.query_reads(text, offs, lens, min_count=min_count, median=median, want_extents=want_ext)
        for key in tot:
            tot[key] += rs[key]
        keep = select(rec, min_kmers=min_kmers, keep_short=keep_short, **rules)
        nkept += int(keep.sum())
        if mask_out is not None:
            mask_out.write(keep.astype(np.uint8).tobytes())
        if not want_ext:
            continue
        buf = np.frombuffer(text, dtype=np.uint8)
        starts, ends = record_bounds(buf, ext, offs, lens)
        if kept_out is not None or rest_out is not None:
            m = byte_mask(len(buf), starts[keep], ends[keep])
            if kept_out is not None:
                kept_out.write(buf[m].tobytes())
            if rest_out is not None:
                rest_out.write(buf[~m].tobytes())
        if table_out is not None:
            for name, e, r in zip(names_of(buf, starts), ext.tolist(), rec.tolist()):
                # (r: sum, kmers, present, solid, min, median, max)
                table_out.write("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, e[1], r[1], r[2], r[3], r[4], r[5], r[6], r[0]))
    tot["sum"] &= (1 << 64) - 1
    return tot, nkept


def main(argv=None, out=None):
    ap = argparse.ArgumentParser(prog="python -m shk.reads", description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="*", metavar="FILE", help="read files (format by suffix: .gz, .bz2, else plain FASTQ)")
    ap.add_argument("-k", type=int, required=True, help="k-mer size of the filter")
    ap.add_argument("-i", "--input", help="a file containing the list of read files (relative to its directory)")
    ap.add_argument("-f", "--format", choices=["g", "b", "f"], help="g(gzip); b(bzip2); f(plain fastq)")
    ap.add_argument("--against", metavar="TABLE.cqf", required=True, help="the filter the reads are asked against")
    ap.add_argument("--min-count", type=int, default=2, help="C: a k-mer the table holds at least C times is solid")
    for name in RULES:
        ap.add_argument("--" + name.replace("_", "-"), type=int if name.endswith("median") else float, default=None)
    ap.add_argument("--min-kmers", type=int, default=0, help="reads with fewer k-mers than max(1, N) pass no rule")
    ap.add_argument("--keep-short", action="store_true", help="... and are kept instead of rejected")
    ap.add_argument("-o", "--output", metavar="KEPT.fq", help="the records of the reads kept")
    ap.add_argument("--rejected", metavar="REST.fq", help="the records of all other reads")
    ap.add_argument("--table", metavar="OUT.tsv", help="one line per read: name, length, k-mers, present, solid, min, median, max, sum")
    ap.add_argument("--mask", metavar="OUT.u8", help="one byte per read, 1 for kept")
    ap.add_argument("--parts-per-call", type=int, default=16, help="parts per call")
    ap.add_argument("--part-size", type=int, default=1 << 23, help="bytes per part, as in a build")
    ap.add_argument("--lib", default=None, help="library to open instead of the in-tree libshk.so")
    a = ap.parse_args(argv)
    if bool(a.input) == bool(a.files):
        ap.error("give either -i LIST -f FORMAT or the read files themselves")
    if a.input:
        if not a.format:
            ap.error("-i needs -f")
        prefix = os.path.dirname(a.input)
        files = [os.path.join(prefix, ln.strip()) if prefix else ln.strip() for ln in open(a.input) if ln.strip()]
        fmt = a.format
    else:
        files = a.files
        fmt = a.format or guess_format(files[0])
        if not a.format and any(guess_format(f) != fmt for f in files):
            ap.error("files of several formats: run them one format at a time, or give -f")
    if a.parts_per_call < 1 or a.part_size < 1:
        ap.error("--parts-per-call and --part-size must be at least 1")
    if a.min_count < 0 or a.min_count >= 1 << 32:
        ap.error("--min-count must fit 32 bits")
    rules = {name: getattr(a, name) for name in RULES}
    median = a.table is not None or rules["min_median"] is not None or rules["max_median"] is not None
    parts = min(a.parts_per_call, 4096)
    cap_bytes = parts * (a.part_size + OVERHEAD + 64)
    qb = cqf_geometry(a.against)[0]
    # windows: a base needs a quality byte, so half the text bounds them; reads: a record is at least 8 bytes
    ctx = Context(qb=qb, k=a.k, max_batch_bytes=cap_bytes, max_batch_keys=cap_bytes // 2 + 256, max_batch_reads=cap_bytes // 8 + 1024,
                  lib_path=a.lib)
    outs = {"kept_out": (a.output, "wb"), "rest_out": (a.rejected, "wb"), "table_out": (a.table, "w"), "mask_out": (a.mask, "wb")}
    fh = {key: open(path, mode) if path else None for key, (path, mode) in outs.items()}
    try:
        ctx.import_cqf(a.against)
        tot, nkept = run(ctx, files, fmt, parts, a.part_size, a.min_count, rules, a.min_kmers, a.keep_short, median, **fh)
    finally:
        ctx.close()
        for f in fh.values():
            if f is not None:
                f.close()
    (out or sys.stdout).write(format_report(tot, nkept, a.k, a.min_count, a.against, rules, a.min_kmers, a.keep_short))
    return 0


if __name__ == "__main__":
    sys.exit(main())
