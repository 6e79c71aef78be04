#!/usr/bin/env python3
"""Side bench of shk_query_reads (not bench.py): reads drawn from a random genome, on the device as FASTQ text, asked
at k = 47, min_count 2, against tables of qb 24 (cache resident) and qb 29 (not) built from the genome by shk_count_fasta
(qb 24 is filled from as long a prefix as loads it to 0.7, so most queried k-mers are absent there). Shapes: 150-base
reads against both tables, and one long-read shape (lengths spread evenly over 5 .. 25 kb, about 15 kb on average)
against qb 24, where a wave runs at the pace of its longest read. Each shape runs without median or track, with the
median, and with a device track. Every configuration gets one untimed call of each kind and then --reps alternating turns.

Reported in k-mers per second: the whole call by the host's clock (it ends in the library's synchronise), and the
kernels alone by the library's HIP events (shk_profile_*): k_reads_query, k_reads_median, and the front end (parse,
pack, scans).

The yardstick is the route a user had before: the same reads written as two-line FASTA records, through shk_query_fasta
with records (k_roll_query plus its k_fa_* front end; no median, min or max), measured in the same run on the same
table, alternating with the new calls. Before anything is timed the records of one call are compared with the
yardstick's, read by read. Writes one JSON document (default profiles/reads_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sh-assembly_amd"))

FRONT = ("k_count_lines", "k_scan_chunks", "k_emit_reads", "k_pack_reads", "k_scan_*", "misc")
FA_FRONT = ("k_fa_maps", "k_fa_states", "k_fa_count", "k_fa_compact", "k_fa_segments+long+tail", "k_fa_pack", "k_scan_*", "k_fa_rec_starts")
K = 47
CHUNK = 1 << 20


def short_reads(seq, n, length, rng):
    """(FASTQ text, FASTA text, record ends of the FASTQ text) of n reads of `length` bases, fixed-width records"""
    at = rng.integers(0, len(seq) - length, n)
    bases = seq[at[:, None] + np.arange(length)[None, :]]
    names = np.frombuffer(b"".join(b"r%08d\n" % i for i in range(n)), dtype=np.uint8).reshape(n, 10)
    fq = np.full((n, 11 + length + 3 + length + 1), ord("I"), dtype=np.uint8)
    fq[:, 0] = ord("@")
    fq[:, 1:11] = names
    fq[:, 11:11 + length] = bases
    fq[:, 11 + length:11 + length + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    fq[:, -1] = 10
    fa = np.full((n, 11 + length + 1), 10, dtype=np.uint8)
    fa[:, 0] = ord(">")
    fa[:, 1:11] = names
    fa[:, 11:11 + length] = bases
    return fq.reshape(-1), fa.reshape(-1), np.arange(1, n + 1, dtype=np.int64) * fq.shape[1]


def long_reads(seq, total, rng):
    lens = []
    while sum(lens) < total:
        lens.append(int(rng.integers(5000, 25001)))
    fq, fa, ends, at = [], [], [], 0
    for i, n in enumerate(lens):
        a = int(rng.integers(0, len(seq) - n))
        s = seq[a:a + n].tobytes()
        fq.append(b"@r%08d\n%s\n+\n%s\n" % (i, s, b"I" * n))
        fa.append(b">r%08d\n%s\n" % (i, s))
        at += len(fq[-1])
        ends.append(at)
    return np.frombuffer(b"".join(fq), dtype=np.uint8), np.frombuffer(b"".join(fa), dtype=np.uint8), np.array(ends, dtype=np.int64)


def chunk_table(ends):
    """chunks of about CHUNK bytes that end where records end"""
    cuts = [0]
    for e in ends.tolist():
        if e - cuts[-1] >= CHUNK:
            cuts.append(e)
    if cuts[-1] != int(ends[-1]):
        cuts.append(int(ends[-1]))
    return cuts[:-1], [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def prof_ms(ctx, names):
    p = ctx.profile_get()
    return sum(p[n][1] for n in names if n in p)


def timed(torch, ctx, f, groups):
    ctx.profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, {g: prof_ms(ctx, names) for g, names in groups.items()}


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=30_000_000)
    ap.add_argument("--bases", type=int, default=60_000_000, help="bases of reads per shape")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qbs", default="24,29")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_bench.json"))
    a = ap.parse_args()
    import torch
    import shk
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    G = a.genome // 60 * 60
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, G)]
    lines = np.full((G // 60, 61), 10, dtype=np.uint8)
    lines[:, :60] = seq.reshape(-1, 60)
    genome_fa = np.concatenate([np.frombuffer(b">g\n", dtype=np.uint8), lines.reshape(-1)])
    del lines
    shapes = {"reads_150": short_reads(seq, a.bases // 150, 150, rng), "long_15kb": long_reads(seq, a.bases, rng)}
    res = {"metric": "shk_query_reads against the two-line-FASTA route through shk_query_fasta, k-mers per second", "k": K, "min_count": 2,
           "reps": a.reps, "genome": G, "tables": {}}
    for qb in [int(x) for x in a.qbs.split(",")]:
        fill_bases = min(G, int(0.7 * (1 << qb)) // 60 * 60)
        out = res["tables"][str(qb)] = {"filled_from_bases": fill_bases, "shapes": {}}
        for shape, (fq, fa, ends) in shapes.items():
            if shape == "long_15kb" and qb != 24:
                continue
            nreads, nbytes = len(ends), len(fq)
            offs, lens = chunk_table(ends)
            d_fq = torch.from_numpy(np.concatenate([fq, np.zeros(16, dtype=np.uint8)])).to(dev)
            d_fa = torch.from_numpy(np.concatenate([fa, np.zeros(16, dtype=np.uint8)])).to(dev)
            cap = max(nbytes, len(genome_fa)) + 64
            ctx = shk.Context(qb=qb, k=K, max_batch_bytes=cap, max_batch_keys=max(nbytes // 2, G) + 4096, max_batch_reads=max(nreads, cap // 16) + 1024)
            fill = torch.from_numpy(np.concatenate([genome_fa[:3 + fill_bases // 60 * 61], np.zeros(16, dtype=np.uint8)])).to(dev)
            ctx.count_fasta(fill.data_ptr(), first=True, on_device=True, text_bytes=fill.numel() - 16)
            del fill
            rec = np.zeros(nreads, dtype=shk._struct_dtype(shk.ReadRecord))
            frec = np.zeros((nreads + 1, 4), dtype=np.uint64)
            d_track = torch.zeros(nbytes // 2, dtype=torch.int32, device=dev)
            nr, nw, rs = C.c_uint64(), C.c_uint64(), shk.ReadsStats()
            nrec, qs = C.c_uint32(), shk.QueryStats()
            toff, tlen = ctx._tab(offs), ctx._tab(lens)

            def reads(median, track):
                ctx._chk(ctx.L.shk_query_reads(ctx.h, C.c_void_p(d_fq.data_ptr()), 1, nbytes, toff, tlen, len(offs), 2, 1 if median else 0,
                                               C.c_void_p(rec.ctypes.data), nreads, 0, C.byref(nr), None,
                                               C.c_void_p(d_track.data_ptr()) if track else None, d_track.numel() if track else 0, 1,
                                               C.byref(nw), C.byref(rs)))

            def fasta():
                ctx._chk(ctx.L.shk_query_fasta(ctx.h, C.c_void_p(d_fa.data_ptr()), 1, len(fa), 1, 2, None, 0, 1, C.c_void_p(frec.ctypes.data),
                                               len(frec), C.byref(nrec), C.byref(qs)))

            kinds = {"plain": (False, False), "median": (True, False), "track": (False, True)}
            # untimed: code objects load, buffers are allocated; and the two routes agree read by read
            for m, t in kinds.values():
                reads(m, t)
            fasta()
            torch.cuda.synchronize()
            assert nr.value == nreads and nrec.value == nreads + 1 and not frec[0].any(), (nr.value, nrec.value)
            for j, f in enumerate(("kmers", "present", "solid", "sum")):
                assert np.array_equal(rec[f].astype(np.uint64), frec[1:, j]), "the two routes disagree on " + f
            nk = rs.kmers
            assert nk == qs.kmers
            ctx.profile(True)
            new = {name: {"call_ms": [], "k_reads_query_ms": [], "k_reads_median_ms": [], "front_ms": []} for name in kinds}
            yard = {"call_ms": [], "k_roll_query_ms": [], "front_ms": []}
            for _ in range(a.reps):      # (alternating, one call of each kind per turn)
                for name, (m, t) in kinds.items():
                    w, g = timed(torch, ctx, lambda: reads(m, t), {"q": ("k_reads_query",), "m": ("k_reads_median",), "f": FRONT})
                    new[name]["call_ms"].append(w)
                    new[name]["k_reads_query_ms"].append(g["q"])
                    new[name]["k_reads_median_ms"].append(g["m"])
                    new[name]["front_ms"].append(g["f"])
                w, g = timed(torch, ctx, fasta, {"q": ("k_roll_query",), "f": FA_FRONT})
                yard["call_ms"].append(w)
                yard["k_roll_query_ms"].append(g["q"])
                yard["front_ms"].append(g["f"])
            ysum = [x + y for x, y in zip(yard["k_roll_query_ms"], yard["front_ms"])]
            r = {"reads": nreads, "text_bytes": nbytes, "fasta_bytes": len(fa), "chunks": len(offs), "windows": nw.value, "kmers": nk,
                 "present": rs.present, "yardstick": yard, "new": new}
            r["yardstick_ms"] = med(ysum)
            r["yardstick_spread_ms"] = max(ysum) - min(ysum)
            r["yardstick_kmers_per_s_call"] = nk / (med(yard["call_ms"]) * 1e-3)
            for name, f in new.items():
                dev_ms = [x + y + z for x, y, z in zip(f["k_reads_query_ms"], f["k_reads_median_ms"], f["front_ms"])]
                f["device_ms"] = med(dev_ms)
                f["device_spread_ms"] = max(dev_ms) - min(dev_ms)
                f["kmers_per_s_call"] = nk / (med(f["call_ms"]) * 1e-3)
                f["kmers_per_s_kernel"] = nk / (med(f["k_reads_query_ms"]) * 1e-3)
            r["plain_within_yardstick"] = new["plain"]["device_ms"] <= r["yardstick_ms"] + r["yardstick_spread_ms"]
            out["shapes"][shape] = r
            print(qb, shape, json.dumps({"reads": nreads, "kmers": nk, "yardstick_ms": round(r["yardstick_ms"], 3),
                                          "spread_ms": round(r["yardstick_spread_ms"], 3), "k_roll_query_ms": round(med(yard["k_roll_query_ms"]), 3),
                                          "yard_call_ms": round(med(yard["call_ms"]), 3),
                                          **{n: {"device_ms": round(f["device_ms"], 3), "k_reads_query_ms": round(med(f["k_reads_query_ms"]), 3),
                                                 "k_reads_median_ms": round(med(f["k_reads_median_ms"]), 3), "front_ms": round(med(f["front_ms"]), 3),
                                                 "call_ms": round(med(f["call_ms"]), 3)} for n, f in new.items()},
                                          "within": r["plain_within_yardstick"]}), flush=True)
            ctx.close()
            del d_fq, d_fa, d_track
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
