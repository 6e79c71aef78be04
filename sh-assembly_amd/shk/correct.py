"""Repair the substitution errors of reads against a filter.

    python -m shk.correct (-i LIST -f {g,b,f} | FILE ...) -k K --against TABLE.cqf [--min-count C] [--check N]
           [--max-edits E] -o CORRECTED.fq [--table OUT.tsv] [--edits OUT.tsv]
           [--parts-per-call P] [--part-size BYTES] [--lib PATH]

The reads go through the chunker a build uses (host/fastq_chunker.cpp: plain, gzip or bzip2, one file or a list) and
through shk_correct_reads against a context that has imported TABLE.cqf; the filter stays untouched. A read whose k-mers
are solid (count >= C), then weak, then solid again holds a wrong base; where exactly one other base makes the next
N + 1 windows solid, that base is written (include/shk.h has the rule; a larger --check is more conservative, at most
--max-edits bases change per read). Reads with an N or any other byte that is no base, and reads shorter than k, are
left as they are.

-o receives every input byte exactly once, in the order the chunker hands out the parts (a single file: the file's
order): headers, '+' lines and quality lines byte for byte, sequence lines with the edits in them (a new letter takes the
case of the one it replaces); a part in which the front end finds no read is copied through. --table writes one line per
read: name, sequence length, edits, unfixable, ambiguous, flags (1 short, 2 holds a byte that is no base, 4 a suspect met
with the edits used up); --edits one line per edit: read name, 0-based position, old letter, new letter."""
import argparse
import os
import sys

import numpy as np

from . import Context
from .estimate import OVERHEAD, guess_format
from .reads import names_of, parts_of, record_bounds
from .spectrum import cqf_geometry

STATS = ("reads", "candidates", "edited_reads", "edits", "unfixable", "ambiguous", "capped")
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def edit_list(buf, ext, rec, edits):
    """the edits of a call one by one, in the order they were made: (read index, position in the sequence line, offset in
    the text, old byte, new byte) as arrays. The old byte of a position's second edit is the first one's new byte; a new
    byte takes the case of the text's. Nothing per read runs in Python."""
    buf = np.frombuffer(buf, dtype=np.uint8)
    edits = np.asarray(edits, dtype=np.uint32)
    edits = edits.reshape(len(rec), -1) if len(rec) else edits.reshape(0, 0)
    live = np.arange(edits.shape[1], dtype=np.uint32)[None, :] < np.asarray(rec["edits"], dtype=np.uint32)[:, None]
    r, e = np.nonzero(live)      # (row by row: the order of the edits of a read)
    word = edits[r, e]
    pos = (word & 0xFFFF).astype(np.int64)
    at = ext["seq_off"].astype(np.int64)[r] + pos
    was = buf[at]
    new = _LETTERS[(word >> 16) & 3] | (was & 0x20)
    old = was.copy()
    order = np.argsort(at, kind="stable")
    again = np.flatnonzero(at[order][1:] == at[order][:-1])
    old[order[again + 1]] = new[order[again]]
    return r, pos, at, old, new


def apply_edits(buf, ext, rec, edits):
    """the text with the edits of one shk_correct_reads call in it, as bytes: a function of its arguments alone. Only
    bytes of sequence lines change, a new letter takes the case of the byte it replaces, and of two edits of one position
    the later wins."""
    out = np.frombuffer(buf, dtype=np.uint8).copy()
    _, _, at, _, new = edit_list(buf, ext, rec, edits)
    if len(at):
        _, last = np.unique(at[::-1], return_index=True)      # (the first of the reversed list = the last made)
        last = len(at) - 1 - last
        out[at[last]] = new[last]
    return out.tobytes()


def _pct(n, of):
    return 100.0 * n / of if of else 0.0


def format_report(stats, k, min_count, check, max_edits, path):
    """the report as text, a function of its numbers alone. stats: the summed shk_correct_stats of the calls"""
    lines = ["reads\t%d" % stats["reads"],
             "candidates\t%d\t%.2f%%" % (stats["candidates"], _pct(stats["candidates"], stats["reads"])),
             "edited reads\t%d\t%.2f%%" % (stats["edited_reads"], _pct(stats["edited_reads"], stats["candidates"])),
             "edits\t%d" % stats["edits"], "unfixable\t%d" % stats["unfixable"], "ambiguous\t%d" % stats["ambiguous"],
             "capped\t%d" % stats["capped"], "against\t%s" % path,
             "parameters\tk=%d min-count=%d check=%d max-edits=%d" % (k, min_count, check, max_edits)]
    return "\n".join(lines) + "\n"


def run(ctx, files, fmt, parts_per_call, part_size, min_count, check, max_edits, out, table_out=None, edits_out=None):
    """every part through ctx; writes what is asked for and returns the summed statistics"""
    tot = {key: 0 for key in STATS}
    want_names = table_out is not None or edits_out is not None
    for text, offs, lens in parts_of(files, fmt, parts_per_call, part_size):
        cs, rec, ext, edits = ctx.correct_reads(text, offs, lens, min_count=min_count, check=check, max_edits=max_edits,
                                                want_extents=True)
        for key in tot:
            tot[key] += cs[key]
        out.write(apply_edits(text, ext, rec, edits))
        if not want_names:
            continue
        buf = np.frombuffer(text, dtype=np.uint8)
        names = names_of(buf, record_bounds(buf, ext, offs, lens)[0])
        if table_out is not None:
            for name, e, r in zip(names, ext.tolist(), rec.tolist()):
                table_out.write("%s\t%d\t%d\t%d\t%d\t%d\n" % (name, e[1], r[0], r[1], r[2], r[3]))
        if edits_out is not None:
            r, pos, _, old, new = edit_list(text, ext, rec, edits)
            for i, p, a, b in zip(r.tolist(), pos.tolist(), old.tolist(), new.tolist()):
                edits_out.write("%s\t%d\t%c\t%c\n" % (names[i], p, a, b))
    return tot


def main(argv=None, out=None):
    ap = argparse.ArgumentParser(prog="python -m shk.correct", description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="*", metavar="FILE", help="read files (format by suffix: .gz, .bz2, else plain FASTQ)")
    ap.add_argument("-k", type=int, required=True, help="k-mer size of the filter")
    ap.add_argument("-i", "--input", help="a file containing the list of read files (relative to its directory)")
    ap.add_argument("-f", "--format", choices=["g", "b", "f"], help="g(gzip); b(bzip2); f(plain fastq)")
    ap.add_argument("--against", metavar="TABLE.cqf", required=True, help="the filter the reads are repaired against")
    ap.add_argument("--min-count", type=int, default=2, help="C: a k-mer the table holds at least C times is solid")
    ap.add_argument("--check", type=int, default=4, help="N: a new base must make the suspect's window and the N behind it solid")
    ap.add_argument("--max-edits", type=int, default=8, help="E: at most E bases of a read change")
    ap.add_argument("-o", "--output", metavar="CORRECTED.fq", required=True, help="the input with the edits in it")
    ap.add_argument("--table", metavar="OUT.tsv", help="one line per read: name, length, edits, unfixable, ambiguous, flags")
    ap.add_argument("--edits", metavar="OUT.tsv", help="one line per edit: read name, position, old letter, new letter")
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
    if a.min_count < 1 or a.min_count >= 1 << 32:
        ap.error("--min-count must be at least 1 and fit 32 bits")
    if not 0 <= a.check <= 255:
        ap.error("--check must lie in 0 .. 255")
    if not 1 <= a.max_edits <= 16:
        ap.error("--max-edits must lie in 1 .. 16")
    parts = min(a.parts_per_call, 4096)
    cap_bytes = parts * (a.part_size + OVERHEAD + 64)
    qb = cqf_geometry(a.against)[0]
    # the 2-bit units: a quarter of max_batch_keys' bytes hold them (text / 64 + reads units of 16 bytes); reads: a record
    # is at least 8 bytes
    ctx = Context(qb=qb, k=a.k, max_batch_bytes=cap_bytes, max_batch_keys=cap_bytes // 2 + 256, max_batch_reads=cap_bytes // 8 + 1024,
                  lib_path=a.lib)
    outs = {"out": (a.output, "wb"), "table_out": (a.table, "w"), "edits_out": (a.edits, "w")}
    fh = {key: open(path, mode) if path else None for key, (path, mode) in outs.items()}
    try:
        ctx.import_cqf(a.against)
        tot = run(ctx, files, fmt, parts, a.part_size, a.min_count, a.check, a.max_edits, **fh)
    finally:
        ctx.close()
        for f in fh.values():
            if f is not None:
                f.close()
    (out or sys.stdout).write(format_report(tot, a.k, a.min_count, a.check, a.max_edits, a.against))
    return 0


if __name__ == "__main__":
    sys.exit(main())
