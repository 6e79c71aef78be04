"""The abundance spectrum of a built filter, computed on the device, in the layout of the ntCard excerpt of the
reference's README (README.md:78-86), and the -N -n -e that its recipe derives from it (README.md:88-93):

    python -m shk.spectrum FILE.cqf -k K [--bins B] [--false-max M] [--lib PATH]

The .cqf is imported into a context of its own geometry (shk_import_cqf) and read by shk_spectrum: no entry leaves the
device. The last bin holds every count >= B and is printed as `f>=B`."""
import argparse
import struct
import sys

from . import Context
from .plan import params_from_spectrum


def format_report(hist, totals, k, false_max=2):
    """the report as text, a function of (hist, totals, k) alone: F1, F0, then the non-zero bins, then the suggestion"""
    lines = ["F1\t%d" % totals["total"], "F0\t%d" % totals["distinct"]]
    nb = len(hist)
    for i, f in enumerate(hist):
        if f:
            lines.append(("f>=%d\t%d" if i == nb - 1 and totals["max_count"] > nb else "f%d\t%d") % (i + 1, f))
    if totals["total"] and false_max <= nb:
        N, n, e = params_from_spectrum(totals["distinct"], totals["total"], hist, k, false_max)
        lines.append("suggested: -N %d -n %d -e %.5f" % (N, n, e))
    else:
        lines.append("suggested: (none: %s)" % ("empty filter" if not totals["total"] else "fewer bins than --false-max"))
    return "\n".join(lines) + "\n"


def cqf_geometry(path):
    """(qb, hb) from the 128-byte header of a .cqf (quotient_filter_metadata, gqf.h:62-77)"""
    with open(path, "rb") as f:
        hdr = f.read(128)
    if len(hdr) != 128:
        raise ValueError("%s: no .cqf header" % path)
    nslots, = struct.unpack_from("<Q", hdr, 16)
    key_bits, = struct.unpack_from("<Q", hdr, 32)
    qb = nslots.bit_length() - 1
    if nslots != 1 << qb or key_bits != qb + 8:
        raise ValueError("%s: not a filter of 2^qb slots with 8-bit remainders" % path)
    return qb, key_bits


def main(argv=None, out=None):
    ap = argparse.ArgumentParser(prog="python -m shk.spectrum", description=__doc__.split("\n\n")[0])
    ap.add_argument("cqf")
    ap.add_argument("-k", type=int, required=True, help="k-mer size the filter was built with")
    ap.add_argument("--bins", type=int, default=256, help="histogram bins; the last takes every larger count")
    ap.add_argument("--false-max", type=int, default=2, help="k-mers with count <= this are taken as false (README.md:94)")
    ap.add_argument("--lib", default=None, help="library to open instead of the in-tree libshk.so")
    a = ap.parse_args(argv)
    if a.bins < 1:
        ap.error("--bins must be at least 1")
    qb, _ = cqf_geometry(a.cqf)
    ctx = Context(qb=qb, k=a.k, max_batch_bytes=1 << 12, max_batch_keys=1 << 12, lib_path=a.lib)
    try:
        ctx.import_cqf(a.cqf)
        hist, totals = ctx.spectrum(a.bins)
    finally:
        ctx.close()
    (out or sys.stdout).write(format_report(hist, totals, a.k, a.false_max))
    return 0


if __name__ == "__main__":
    sys.exit(main())
