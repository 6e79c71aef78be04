"""Count the k-mers of a FASTA file on the device, and compare them with a filter built from reads:

    python -m shk.fasta FILE.fa[.gz] -k K (-q QB | --against READS.cqf) [-o OUT.cqf] [--min-count S] [--piece BYTES] [--lib PATH]

The file (a genome, somebody's assembly, this project's own unitigs.fa, long reads: records and lines of any length) is
streamed through shk_count_fasta in pieces cut at arbitrary byte positions -- nothing looks for record bounds, the
context carries the state of the stream from piece to piece. With --against the FASTA filter takes the reads filter's
geometry; its entries (shk_dump) are looked up in the reads filter (shk_lookup, counts only): how many of the FASTA's
distinct k-mers the reads hold at all, how many with count >= S, and the inner product of the two filters
(shk_inner_product)."""
import argparse
import gzip
import sys

from . import Context
from .spectrum import cqf_geometry


def format_report(fstats, distinct, against=None):
    """the report as text, a function of its numbers alone. fstats: records / bases / breaks / kmers summed over the
    pieces; against: dict(path, present, min_count, solid, inner_product) or None"""
    lines = ["records\t%d" % fstats["records"], "bases\t%d" % fstats["bases"], "breaks\t%d" % fstats["breaks"],
             "k-mers\t%d" % fstats["kmers"], "distinct\t%d" % distinct]
    if against is not None:
        pct = lambda n: 100.0 * n / distinct if distinct else 0.0      # noqa: E731
        lines += ["against\t%s" % against["path"],
                  "present\t%d\t%.2f%%" % (against["present"], pct(against["present"])),
                  "count>=%d\t%d\t%.2f%%" % (against["min_count"], against["solid"], pct(against["solid"])),
                  "inner product\t%d" % against["inner_product"]]
    return "\n".join(lines) + "\n"


def count_file(ctx, path, piece):
    """stream the file through ctx in pieces of `piece` bytes; returns the summed FASTA statistics"""
    tot = {"records": 0, "bases": 0, "breaks": 0, "kmers": 0}
    first = True
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        while True:
            buf = f.read(piece)
            if not buf and not first:
                break
            _, fs = ctx.count_fasta(buf, first=first)
            first = False
            for key in tot:
                tot[key] += fs[key]
            if not buf:
                break
    return tot


def main(argv=None, out=None):
    ap = argparse.ArgumentParser(prog="python -m shk.fasta", description=__doc__.split("\n\n")[0])
    ap.add_argument("fasta")
    ap.add_argument("-k", type=int, required=True, help="k-mer size (the reads filter's, with --against)")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("-q", type=int, help="log2 of the filter's slots")
    g.add_argument("--against", metavar="READS.cqf", help="a filter built from reads: take its geometry and compare")
    ap.add_argument("-o", metavar="OUT.cqf", help="write the FASTA's filter")
    ap.add_argument("--min-count", type=int, default=2, help="S: also report the k-mers the reads hold at least S times")
    ap.add_argument("--piece", type=int, default=1 << 24, help="bytes per call")
    ap.add_argument("--lib", default=None, help="library to open instead of the in-tree libshk.so")
    a = ap.parse_args(argv)
    if a.piece < 1:
        ap.error("--piece must be at least 1")
    qb = cqf_geometry(a.against)[0] if a.against else a.q
    ctx = Context(qb=qb, k=a.k, max_batch_bytes=a.piece, max_batch_keys=a.piece + 256, lib_path=a.lib)
    reads = None
    try:
        fstats = count_file(ctx, a.fasta, a.piece)
        distinct = ctx.totals().ndistinct
        against = None
        if a.against:
            reads = Context(qb=qb, k=a.k, max_batch_bytes=1 << 12, max_batch_keys=1 << 12, lib_path=a.lib)
            reads.import_cqf(a.against)
            entries = ctx.dump()
            counts, _ = reads.lookup([key for key, _ in entries], mode=2)
            against = {"path": a.against, "present": sum(1 for c in counts if c), "min_count": a.min_count,
                       "solid": sum(1 for c in counts if c >= a.min_count), "inner_product": ctx.inner_product(reads)}
        if a.o:
            ctx.export_cqf(a.o)
    finally:
        ctx.close()
        if reads is not None:
            reads.close()
    (out or sys.stdout).write(format_report(fstats, distinct, against))
    return 0


if __name__ == "__main__":
    sys.exit(main())
