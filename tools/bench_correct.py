#!/usr/bin/env python3
"""Side bench of shk_correct_reads (not bench.py): tools/bench_reads.py's 150-base reads (same generator, same seed),
on the device as FASTQ text, against its tables of qb 24 (cache resident, filled from a prefix of the genome) and qb 29
(the whole genome) built from the genome by shk_count_fasta, at k = 47. Once as drawn -- every read is a piece of the
genome -- and once with 1 % of the bases substituted. The genome is counted once, so a k-mer of it has count 1:
min_count is 1 here (at bench_reads.py's 2 no window would be solid and no read would have a suspect); check and
max_edits are the defaults, 4 and 8. Records come back to the host, the edit lists stay on the device.

Reported per configuration: bases per second -- the whole call by the host's clock (it ends in the library's
synchronise), and k_reads_correct alone by the library's HIP events (shk_profile_*), with the front end (parse, pack,
scans) next to it -- and table lookups per window (shk_correct_lookups over the candidates' windows: 1 is a single
clean pass, 2 both passes without a suspect). Alongside, from the same run and alternating with the new calls, the
same texts through shk_query_reads without track and median. Every configuration gets one untimed call of each kind
and then --reps alternating turns. No threshold is set. Writes one JSON document (default profiles/correct_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sh-assembly_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_reads import FRONT, K, chunk_table, med, short_reads, timed  # noqa: E402

LENGTH = 150


def with_errors(fq, nreads, rate, rng):
    """a copy of short_reads' FASTQ text with `rate` of the bases replaced by one of the three others; (text, errors)"""
    out = fq.reshape(nreads, -1).copy()
    bases = out[:, 11:11 + LENGTH]
    code = ((bases >> 1) ^ (bases >> 2)) & 3
    hit = rng.random(bases.shape) < rate
    code = np.where(hit, (code + rng.integers(1, 4, bases.shape)) & 3, code)
    out[:, 11:11 + LENGTH] = np.frombuffer(b"ACGT", dtype=np.uint8)[code]
    return out.reshape(-1), int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=30_000_000)
    ap.add_argument("--bases", type=int, default=60_000_000, help="bases of reads")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qbs", default="24,29")
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_bench.json"))
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
    nreads = a.bases // LENGTH
    clean, _, ends = short_reads(seq, nreads, LENGTH, rng)
    noisy, nerr = with_errors(clean, nreads, a.rate, np.random.default_rng(4))
    texts = {"clean": clean, "errors": noisy}
    nbytes, nbases, nwin = len(clean), nreads * LENGTH, nreads * (LENGTH - K + 1)
    offs, lens = chunk_table(ends)
    res = {"metric": "shk_correct_reads, bases of reads per second, next to shk_query_reads (no track, no median) on the same texts",
           "k": K, "min_count": 1, "check": 4, "max_edits": 8, "reps": a.reps, "genome": G, "reads": nreads, "read_length": LENGTH,
           "bases": nbases, "windows": nwin, "text_bytes": nbytes, "chunks": len(offs), "substitution_rate": a.rate, "substitutions": nerr,
           "tables": {}}
    for qb in [int(x) for x in a.qbs.split(",")]:
        fill_bases = min(G, int(0.7 * (1 << qb)) // 60 * 60)
        cap = max(nbytes, len(genome_fa)) + 64
        ctx = shk.Context(qb=qb, k=K, max_batch_bytes=cap, max_batch_keys=max(nbytes // 2, G) + 4096, max_batch_reads=max(nreads, cap // 16) + 1024)
        fill = torch.from_numpy(np.concatenate([genome_fa[:3 + fill_bases // 60 * 61], np.zeros(16, dtype=np.uint8)])).to(dev)
        ctx.count_fasta(fill.data_ptr(), first=True, on_device=True, text_bytes=fill.numel() - 16)
        del fill
        d_text = {name: torch.from_numpy(np.concatenate([t, np.zeros(16, dtype=np.uint8)])).to(dev) for name, t in texts.items()}
        crec = np.zeros(nreads, dtype=shk._struct_dtype(shk.CorrectRecord))
        qrec = np.zeros(nreads, dtype=shk._struct_dtype(shk.ReadRecord))
        d_edits = torch.zeros(nreads * 8, dtype=torch.int32, device=dev)
        nr, nw, cs, rs = C.c_uint64(), C.c_uint64(), shk.CorrectStats(), shk.ReadsStats()
        toff, tlen = ctx._tab(offs), ctx._tab(lens)

        def correct(name):
            ctx._chk(ctx.L.shk_correct_reads(ctx.h, C.c_void_p(d_text[name].data_ptr()), 1, nbytes, toff, tlen, len(offs), 1, 4, 8,
                                             C.c_void_p(crec.ctypes.data), nreads, 0, C.byref(nr), None, C.c_void_p(d_edits.data_ptr()), 1,
                                             C.byref(cs)))

        def query(name):
            ctx._chk(ctx.L.shk_query_reads(ctx.h, C.c_void_p(d_text[name].data_ptr()), 1, nbytes, toff, tlen, len(offs), 1, 0,
                                           C.c_void_p(qrec.ctypes.data), nreads, 0, C.byref(nr), None, None, 0, 1, C.byref(nw), C.byref(rs)))

        out = res["tables"][str(qb)] = {"filled_from_bases": fill_bases, "texts": {}}
        # untimed: code objects load, buffers are allocated; and what the calls say about the texts
        facts = {}
        for name in texts:
            correct(name)
            query(name)
            torch.cuda.synchronize()
            assert nr.value == nreads and cs.candidates == nreads and nw.value == nwin, (nr.value, cs.candidates, nw.value)
            facts[name] = dict(cs.as_dict(), lookups=ctx.correct_lookups(), solid_windows=rs.solid)
        if fill_bases == G:      # (every k-mer of a clean read is in the table: one pass, nothing to repair)
            assert facts["clean"]["edits"] == 0 and facts["clean"]["lookups"] == nwin and facts["errors"]["edits"] > 0, facts
        ctx.profile(True)
        runs = {name: {"correct": {"call_ms": [], "kernel_ms": [], "front_ms": []}, "query": {"call_ms": [], "kernel_ms": [], "front_ms": []}}
                for name in texts}
        for _ in range(a.reps):      # (alternating, one call of each kind per turn)
            for name in texts:
                for kind, f, kernel in (("correct", correct, "k_reads_correct"), ("query", query, "k_reads_query")):
                    w, g = timed(torch, ctx, lambda: f(name), {"k": (kernel,), "f": FRONT})
                    runs[name][kind]["call_ms"].append(w)
                    runs[name][kind]["kernel_ms"].append(g["k"])
                    runs[name][kind]["front_ms"].append(g["f"])
        for name in texts:
            r = dict(facts[name], lookups_per_window=facts[name]["lookups"] / nwin)
            for kind, t in runs[name].items():
                r[kind] = dict(t, call_spread_ms=max(t["call_ms"]) - min(t["call_ms"]), kernel_spread_ms=max(t["kernel_ms"]) - min(t["kernel_ms"]),
                               bases_per_s_call=nbases / (med(t["call_ms"]) * 1e-3), bases_per_s_kernel=nbases / (med(t["kernel_ms"]) * 1e-3))
            r["correct_over_query_kernel"] = med(runs[name]["correct"]["kernel_ms"]) / med(runs[name]["query"]["kernel_ms"])
            r["correct_over_query_call"] = med(runs[name]["correct"]["call_ms"]) / med(runs[name]["query"]["call_ms"])
            out["texts"][name] = r
            print(qb, name, json.dumps({"edits": r["edits"], "edited_reads": r["edited_reads"], "unfixable": r["unfixable"],
                                        "lookups_per_window": round(r["lookups_per_window"], 3),
                                        **{kind: {"call_ms": round(med(t["call_ms"]), 3), "kernel_ms": round(med(t["kernel_ms"]), 3),
                                                  "front_ms": round(med(t["front_ms"]), 3), "Gbases_per_s_call": round(r[kind]["bases_per_s_call"] / 1e9, 3),
                                                  "Gbases_per_s_kernel": round(r[kind]["bases_per_s_kernel"] / 1e9, 3)} for kind, t in runs[name].items()},
                                        "kernel_ratio": round(r["correct_over_query_kernel"], 3)}), flush=True)
        ctx.close()
        del d_text, d_edits
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
