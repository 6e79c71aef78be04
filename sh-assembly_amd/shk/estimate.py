"""-N -n -e for CQF-deNoise from the reads themselves: a hash-sampled k-mer spectrum, counted on the device.

    python -m shk.estimate -k K (-i LIST -f {g,b,f} | FILE ...) [-s S] [--qb QB] [--bins B] [--false-max M]
                           [--parts-per-call P] [--part-size BYTES] [--flags] [--lib PATH]

The reference's README sends the user to ntCard for these three numbers (README.md:74-94); its recipe is N = F1,
n = F0 - f1 - f2, e = 1 - ((F1 - f1 - 2 f2) / F1)^(1/k). Here the reads go through the chunker a build uses
(host/fastq_chunker.cpp: the same parts, so F1 is exactly the nelts a build without deNoise reports) and through
shk_sample_chunks, which counts -- exactly, in a small filter of 2^QB slots -- the k-mers whose canonical hash has S
chosen bits zero: a 2^-S sample of the DISTINCT k-mers with their true abundances. shk_spectrum of that filter, scaled
by 2^S, is the report; F1 is counted exactly on the way.

    bin/CQF-deNoise -k 47 $(python -m shk.estimate -k 47 -f f -i files.txt --flags) -f f -i files.txt -o k47.cqf

Without -s the sample is chosen so that the small filter stays at most half full even if every k-mer of the input were
distinct (default_sample_bits)."""
import argparse
import ctypes as C
import os
import sys

from . import Context, ShkError
from .count import _host
from .plan import params_from_spectrum
from .spectrum import format_report

OVERHEAD = 65535          # the chunker's allowance for the record a part ends in (cqf/CQF_mt.h:735-816), as in a build
MAX_SAMPLE_BITS = 24      # shk_sample_chunks (include/shk.h): sample_bits <= 24 and hb + sample_bits <= 56


def max_sample_bits(qb):
    return max(0, min(MAX_SAMPLE_BITS, 56 - (qb + 8)))


def input_bytes(sizes, fmt):
    """bytes of FASTQ text the files hold, as far as their sizes tell: compressed files count four times"""
    return sum(int(x) for x in sizes) * (4 if fmt in ("g", "b") else 1)


def default_sample_bits(sizes, fmt, qb):
    """the smallest s with (B_in / 2) * 2^-s <= 0.5 * 2^qb, capped by what shk_sample_chunks takes: a base needs a
    quality byte, so B_in / 2 bounds the k-mers, and the kept keys stay below half the slots even if all were distinct"""
    b_in, s = input_bytes(sizes, fmt), 0
    while s < max_sample_bits(qb) and b_in > (1 << (qb + s)):
        s += 1
    return s


def format_estimate(hist, totals, sstats_sum, s, k, false_max=2):
    """the report as text, a function of its arguments alone: hist, totals = shk_spectrum of the small filter,
    sstats_sum = the summed shk_sample_stats of the calls that filled it"""
    scaled = {"total": int(sstats_sum["kmers"]), "distinct": int(totals["distinct"]) << s, "max_count": int(totals["max_count"])}
    return "sampled\t1/2^%d\t%d\n" % (s, totals["distinct"]) + format_report([int(f) << s for f in hist], scaled, k, false_max)


def format_flags(hist, totals, sstats_sum, s, k, false_max=2):
    N, n, e = params_from_spectrum(int(totals["distinct"]) << s, int(sstats_sum["kmers"]), [int(f) << s for f in hist], k, false_max)
    return "-N %d -n %d -e %.5f\n" % (N, n, e)


def guess_format(path):
    return "g" if path.endswith(".gz") else "b" if path.endswith(".bz2") else "f"


def sample_files(ctx, files, fmt, s, parts_per_call, part_size):
    """the files' parts, `parts_per_call` per shk_sample_chunks call, into ctx; returns the summed sample statistics"""
    H = _host()
    arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
    bh = H.shkh_batch_open(arr, len(files), {"f": 0, "g": 1, "b": 2}[fmt], part_size, OVERHEAD)
    if not bh:
        raise IOError("cannot open the input files")
    total = {"kmers": 0, "kept": 0}
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
                _, ss = ctx.sample_chunks(bytes(text), offs, lens, s)
                for key in total:
                    total[key] += ss[key]
    finally:
        H.shkh_batch_close(bh)
    return total


def main(argv=None, out=None):
    ap = argparse.ArgumentParser(prog="python -m shk.estimate", description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="*", metavar="FILE", help="read files (format by suffix: .gz, .bz2, else plain FASTQ)")
    ap.add_argument("-k", type=int, required=True, help="k-mer size")
    ap.add_argument("-i", "--input", help="a file containing the list of read files (relative to its directory)")
    ap.add_argument("-f", "--format", choices=["g", "b", "f"], help="g(gzip); b(bzip2); f(plain fastq)")
    ap.add_argument("-s", type=int, default=None, help="sample 1 in 2^S distinct k-mers (default: from the input's size)")
    ap.add_argument("--qb", type=int, default=24, help="log2 of the small filter's slots")
    ap.add_argument("--bins", type=int, default=256, help="histogram bins; the last takes every larger count")
    ap.add_argument("--false-max", type=int, default=2, help="k-mers with count <= this are taken as false (README.md:94)")
    ap.add_argument("--parts-per-call", type=int, default=16, help="parts per call")
    ap.add_argument("--part-size", type=int, default=1 << 23, help="bytes per part, as in a build")
    ap.add_argument("--flags", action="store_true", help="print only `-N .. -n .. -e ..`")
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
    if a.bins < 1 or a.parts_per_call < 1 or a.part_size < 1:
        ap.error("--bins, --parts-per-call and --part-size must be at least 1")
    s = a.s if a.s is not None else default_sample_bits([os.path.getsize(f) for f in files], fmt, a.qb)
    if s < 0 or s > max_sample_bits(a.qb):
        ap.error("-s must lie in 0 .. %d for --qb %d" % (max_sample_bits(a.qb), a.qb))
    parts = min(a.parts_per_call, 4096)
    cap_bytes = parts * (a.part_size + OVERHEAD + 64)
    # keys: the 2-bit staging of 150-base reads needs about text / 27 words, the kept words at most text / 2^(s + 1)
    ctx = Context(qb=a.qb, k=a.k, num_denoise=0, max_batch_bytes=cap_bytes, max_batch_keys=max(cap_bytes // 16, cap_bytes >> (s + 1), 1 << 12),
                  max_batch_reads=cap_bytes // 16 + 1024, lib_path=a.lib)
    try:
        try:
            sstats = sample_files(ctx, files, fmt, s, parts, a.part_size)
        except ShkError as e:
            if e.code not in (-3, -4):      # SHK_ERR_TABLE_FULL, or SHK_ERR_REGION: how a table many times too small fails
                raise
            sys.stderr.write("%s\nthe sample does not fit a filter of 2^%d slots: raise -s (now %d) or --qb\n" % (e, a.qb, s))
            return 1
        hist, totals = ctx.spectrum(a.bins)
    finally:
        ctx.close()
    fmt_fn = format_flags if a.flags else format_estimate
    if a.flags and (not sstats["kmers"] or a.false_max > a.bins):
        sys.stderr.write("no parameters: %s\n" % ("no k-mers in the input" if not sstats["kmers"] else "fewer bins than --false-max"))
        return 1
    (out or sys.stdout).write(fmt_fn(hist, totals, sstats, s, a.k, a.false_max))
    return 0


if __name__ == "__main__":
    sys.exit(main())
