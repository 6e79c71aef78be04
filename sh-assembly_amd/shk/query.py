"""How often do the reads hold the k-mers of this sequence, position by position and record by record?

    python -m shk.query FILE.fa[.gz] -k K --against READS.cqf [--min-count S] [--records] [--track OUT.u32] [--piece BYTES] [--lib PATH]

The file (a genome, somebody's assembly, this project's own unitigs.fa, long reads: records and lines of any length) is
streamed through shk_query_fasta in pieces cut at arbitrary byte positions, against a context that has imported READS.cqf;
the filter stays untouched and no second table is built. The report: records, bases, k-mers, how many of the k-mers the
reads hold at all and at least S times, their mean count, and the consensus quality that k-mer completeness implies,
QV = -10 log10(1 - (present / k-mers)^(1/k)). --records adds one line per record, --track writes the count of the k-mer
that ends at every base (little-endian uint32, 0xFFFFFFFF where none ends: the coverage track of an assembly)."""
import argparse
import gzip
import math
import sys

import numpy as np

from . import Context
from .spectrum import cqf_geometry

NO_HEADER = "(no header)"      # the name of sequence in front of the file's first header line


def qv(present, kmers, k):
    """-10 log10 of the per-base error rate at which a share present / kmers of the k-mers survives; inf when all do"""
    if not kmers:
        return float("nan")
    if present >= kmers:
        return float("inf")
    return -10.0 * math.log10(1.0 - (present / kmers) ** (1.0 / k)) + 0.0


def _pct(n, of):
    return 100.0 * n / of if of else 0.0


def _mean(total, kmers):
    return total / kmers if kmers else 0.0


def format_report(qstats, k, min_count, path, records=None):
    """the report as text, a function of its numbers alone. qstats: the summed statistics of the pieces; records: None or
    [(name, kmers, present, solid, sum)]"""
    n = qstats["kmers"]
    lines = ["records\t%d" % qstats["records"], "bases\t%d" % qstats["bases"], "k-mers\t%d" % n, "against\t%s" % path,
             "present\t%d\t%.2f%%" % (qstats["present"], _pct(qstats["present"], n)),
             "count>=%d\t%d\t%.2f%%" % (min_count, qstats["solid"], _pct(qstats["solid"], n)),
             "mean count\t%.2f" % _mean(qstats["sum"], n), "QV\t%.2f" % qv(qstats["present"], n, k)]
    if records is not None:
        lines.append("#name\tk-mers\tpresent\tsolid\tmean\tQV")
        lines += ["%s\t%d\t%d\t%d\t%.2f\t%.2f" % (name, m, p, s, _mean(t, m), qv(p, m, k)) for name, m, p, s, t in records]
    return "\n".join(lines) + "\n"


class Names:
    """the records' names, taken from the header lines on the host: what follows the '>' or ';' up to the first blank. Keeps
    the state of the line (at its start, inside a header, inside its name) over feed() calls, as the device keeps its own"""

    def __init__(self):
        self.names = []
        self.line_start, self.header, self.naming = True, False, False

    def feed(self, piece):
        for c in piece:
            if self.header:
                if c == 10:
                    self.header, self.naming, self.line_start = False, False, True
                elif self.naming:
                    if c in b" \t\r":
                        self.naming = False
                    else:
                        self.names[-1] += chr(c)
            elif self.line_start and c in b">;":
                self.header, self.naming, self.line_start = True, True, False
                self.names.append("")
            else:
                self.line_start = c == 10
        return self


def query_file(ctx, path, piece, min_count, track_out=None):
    """stream the file through ctx in pieces of `piece` bytes; returns (summed statistics, [[kmers, present, solid, sum]]
    per record -- entry 0 is the sequence in front of the first header --, the names of the header lines)"""
    tot = {key: 0 for key in ("records", "bases", "breaks", "kmers", "present", "solid", "sum")}
    recs = np.zeros((1, 4), dtype=np.uint64)
    names = Names()
    first = True
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        while True:
            buf = f.read(piece)
            if not buf and not first:
                break
            qs, rec, track = ctx.query_fasta(buf, first=first, min_count=min_count, want_track=track_out is not None)
            first = False
            for key in tot:
                tot[key] += qs[key]
            recs[-1] += rec[0]      # (the record that was open when the piece began)
            recs = np.concatenate([recs, rec[1:]])
            names.feed(buf)
            if track_out is not None:
                track_out.write(track.astype("<u4").tobytes())
            if not buf:
                break
    tot["sum"] &= (1 << 64) - 1
    return tot, recs, names.names


def main(argv=None, out=None):
    ap = argparse.ArgumentParser(prog="python -m shk.query", description=__doc__.split("\n\n")[0])
    ap.add_argument("fasta")
    ap.add_argument("-k", type=int, required=True, help="k-mer size of the reads filter")
    ap.add_argument("--against", metavar="READS.cqf", required=True, help="a filter built from reads")
    ap.add_argument("--min-count", type=int, default=2, help="S: a k-mer the reads hold at least S times is solid")
    ap.add_argument("--records", action="store_true", help="one line per record: name, k-mers, present, solid, mean count, QV")
    ap.add_argument("--track", metavar="OUT.u32", help="write the per-base counts, little-endian uint32")
    ap.add_argument("--piece", type=int, default=1 << 24, help="bytes per call")
    ap.add_argument("--lib", default=None, help="library to open instead of the in-tree libshk.so")
    a = ap.parse_args(argv)
    if a.piece < 1:
        ap.error("--piece must be at least 1")
    if a.min_count < 0 or a.min_count >= 1 << 32:
        ap.error("--min-count must fit 32 bits")
    qb = cqf_geometry(a.against)[0]
    ctx = Context(qb=qb, k=a.k, max_batch_bytes=a.piece, max_batch_keys=a.piece + 256, lib_path=a.lib)
    track_out = open(a.track, "wb") if a.track else None
    try:
        ctx.import_cqf(a.against)
        tot, recs, names = query_file(ctx, a.fasta, a.piece, a.min_count, track_out)
    finally:
        ctx.close()
        if track_out is not None:
            track_out.close()
    if len(names) != tot["records"] or len(recs) != 1 + tot["records"]:
        sys.stderr.write("shk.query: %d header lines read on the host, %d on the device\n" % (len(names), tot["records"]))
        return 1
    records = None
    if a.records:
        rows = [(name,) + tuple(int(x) for x in r) for name, r in zip([NO_HEADER] + names, recs)]
        records = rows[1:] if rows[0][1] == 0 else rows      # (sequence in front of the first header is listed when it has k-mers)
    (out or sys.stdout).write(format_report(tot, a.k, a.min_count, a.against, records))
    return 0


if __name__ == "__main__":
    sys.exit(main())
