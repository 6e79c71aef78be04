#!/usr/bin/env python3
"""Side bench of shk_query_fasta (not bench.py): a random genome on the device, as one record of 60-column FASTA and as
records of 2 kb, queried at k = 47 against tables of qb 24 and qb 29 built from the genome itself by shk_count_fasta (qb 29
holds all of its k-mers; qb 24 has 2^24 slots, so it is filled from as long a prefix of the genome as loads it to 0.7, and
the rest of the queried k-mers are absent). Every configuration gets one untimed call of each kind and --reps timed ones.

Reported in k-mers per second: the whole call by the host's clock (it ends in the library's synchronise) and k_roll_query
alone by the library's HIP events (shk_profile_*), each with a device track and without one.

The yardstick is the unfused route made of kernels that were there before, timed in the same process and alternating
with the fused calls: shk_lookup(on_device, mode 2) over the same keys in text order (k_lookup), plus what shk_count_fasta
spends in its front end (k_fa_*, the scans) and its roll kernels (k_roll_hist, k_roll_scatter) on the same text, counted
into a qb-29 table of its own. The fused
kernel, k_roll_query plus the query's own front end, should cost no more than that sum; the margin is the spread
(max - min) of the yardstick over its own repeats. The track of the one-record form is compared with the yardstick's
counts entry by entry before anything is timed. Writes one JSON document (default profiles/query_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sh-assembly_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRONT = ("k_fa_maps", "k_fa_states", "k_fa_count", "k_fa_compact", "k_fa_segments+long+tail", "k_fa_pack", "k_scan_*", "k_fa_rec_starts")
ROLL = ("k_roll_hist", "k_roll_scatter")
K = 47


def one_record(seq):
    """'>g' and lines of 60 bases"""
    lines = np.full((len(seq) // 60, 61), 10, dtype=np.uint8)
    lines[:, :60] = seq.reshape(-1, 60)
    return np.concatenate([np.frombuffer(b">g\n", dtype=np.uint8), lines.reshape(-1)])


def records_2kb(seq):
    """'>r0000000' ... and 2000 bases each, as 33 lines of 60 and one of 20"""
    n = len(seq) // 2000
    rec = np.full((n, 10 + 33 * 61 + 21), 10, dtype=np.uint8)
    names = np.frombuffer(b"".join(b">r%07d\n" % i for i in range(n)), dtype=np.uint8).reshape(n, 10)
    rec[:, :10] = names
    s = seq[:n * 2000].reshape(n, 2000)
    rec[:, 10:10 + 33 * 61].reshape(n, 33, 61)[:, :, :60] = s[:, :1980].reshape(n, 33, 60)
    rec[:, 10 + 33 * 61:10 + 33 * 61 + 20] = s[:, 1980:]
    return rec.reshape(-1)


def prof_ms(ctx, names):
    p = ctx.profile_get()
    return sum(p[n][1] for n in names if n in p)


def timed(torch, ctx, f, groups, reps):
    """reps calls of f, each with the profile reset: ([call ms by the host's clock], {group: [ms per call]})"""
    wall, out = [], {g: [] for g in groups}
    for _ in range(reps):
        ctx.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        for g, names in groups.items():
            out[g].append(prof_ms(ctx, names))
    return wall, out


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=64_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qbs", default="24,29")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    a = ap.parse_args()
    import torch
    import cqflibs
    import shk
    dev = torch.device("cuda", 0)
    G = a.bases // 6000 * 6000
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(3).integers(0, 4, G)]
    forms = {"one_record": one_record(seq), "records_2kb": records_2kb(seq)}
    O = cqflibs.oracle()
    res = {"metric": "shk_query_fasta against the unfused route, k-mers per second", "bases": G, "k": K, "reps": a.reps, "tables": {}}
    for qb in [int(x) for x in a.qbs.split(",")]:
        hb = qb + 8
        fill_bases = min(G, int(0.7 * (1 << qb)) // 60 * 60)
        out = res["tables"][str(qb)] = {"filled_from_bases": fill_bases, "forms": {}}
        for form, text in forms.items():
            nbytes = len(text)
            d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).to(dev)
            runs = [seq.tobytes()] if form == "one_record" else [seq[i:i + 2000].tobytes() for i in range(0, G, 2000)]
            keys = O.seq_keys(runs, K, hb)
            del runs
            nk = len(keys)
            d_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
            d_counts = torch.zeros(nk, dtype=torch.int64, device=dev)
            d_track = torch.zeros(G, dtype=torch.int32, device=dev)
            ctx = shk.Context(qb=qb, k=K, max_batch_bytes=nbytes + 64, max_batch_keys=G + 4096)
            fill = torch.from_numpy(np.concatenate([forms["one_record"][:3 + fill_bases // 60 * 61], np.zeros(16, dtype=np.uint8)])).to(dev)
            ctx.count_fasta(fill.data_ptr(), first=True, on_device=True, text_bytes=fill.numel() - 16)
            del fill
            # (the yardstick's count goes into a table of its own that holds the whole genome, whatever the queried table's size)
            scratch = shk.Context(qb=max(qb, 29), k=K, max_batch_bytes=nbytes + 64, max_batch_keys=G + 4096)
            nrec, qs = C.c_uint32(), shk.QueryStats()
            rec = np.zeros((G // 2000 + 2, 4), dtype=np.uint64)

            def query(track):
                ctx._chk(ctx.L.shk_query_fasta(ctx.h, C.c_void_p(d_text.data_ptr()), 1, nbytes, 1, 2, C.c_void_p(d_track.data_ptr()) if track else None,
                                               G if track else 0, 1, C.c_void_p(rec.ctypes.data), len(rec), C.byref(nrec), C.byref(qs)))

            def lookup():
                ctx._chk(ctx.L.shk_lookup(ctx.h, C.c_void_p(d_keys.data_ptr()), nk, 1, 2, C.c_void_p(d_counts.data_ptr()), None))

            def count():
                scratch.count_fasta(d_text.data_ptr(), first=True, on_device=True, text_bytes=nbytes)

            # untimed: code objects load, buffers are allocated; and the answers agree
            query(True), query(False), lookup(), count()
            torch.cuda.synchronize()
            assert qs.kmers == nk, (qs.kmers, nk)
            if form == "one_record":
                assert torch.equal(d_track[K - 1:].long() & 0xFFFFFFFF, d_counts.clamp(max=0xFFFFFFFE)), "track and lookup disagree"
            assert qs.sum == int(d_counts.sum().item()) and qs.present == int((d_counts > 0).sum().item())
            ctx.profile(True)
            scratch.profile(True)
            r = {"text_bytes": nbytes, "kmers": nk, "records": qs.records, "present": qs.present}
            fused = {"track": {"call_ms": [], "k_roll_query_ms": [], "front_ms": []}, "no_track": {"call_ms": [], "k_roll_query_ms": [], "front_ms": []}}
            yard = {"k_lookup_ms": [], "count_front_ms": [], "count_roll_ms": []}
            for _ in range(a.reps):      # (alternating, one call of each kind per turn)
                for name, tr in (("track", True), ("no_track", False)):
                    w, g = timed(torch, ctx, lambda: query(tr), {"q": ("k_roll_query",), "f": FRONT}, 1)
                    fused[name]["call_ms"] += w
                    fused[name]["k_roll_query_ms"] += g["q"]
                    fused[name]["front_ms"] += g["f"]
                _, g = timed(torch, ctx, lookup, {"l": ("k_lookup",)}, 1)
                yard["k_lookup_ms"] += g["l"]
                _, g = timed(torch, scratch, count, {"f": FRONT, "r": ROLL}, 1)
                yard["count_front_ms"] += g["f"]
                yard["count_roll_ms"] += g["r"]
            ysum = [x + y + z for x, y, z in zip(yard["k_lookup_ms"], yard["count_front_ms"], yard["count_roll_ms"])]
            yard["sum_ms"] = ysum
            r["yardstick"] = yard
            r["fused"] = fused
            for name in fused:
                f = fused[name]
                f["kmers_per_s_call"] = nk / (med(f["call_ms"]) * 1e-3)
                f["kmers_per_s_kernel"] = nk / (med(f["k_roll_query_ms"]) * 1e-3)
                f["fused_ms"] = med([x + y for x, y in zip(f["k_roll_query_ms"], f["front_ms"])])
            r["yardstick_ms"] = med(ysum)
            r["yardstick_spread_ms"] = max(ysum) - min(ysum)
            r["fused_within_yardstick"] = all(fused[n]["fused_ms"] <= r["yardstick_ms"] + r["yardstick_spread_ms"] for n in fused)
            out["forms"][form] = r
            print(qb, form, json.dumps({"kmers": nk, "yardstick_ms": round(r["yardstick_ms"], 3), "spread_ms": round(r["yardstick_spread_ms"], 3),
                                         "k_lookup_ms": round(med(yard["k_lookup_ms"]), 3),
                                         **{n: {"fused_ms": round(fused[n]["fused_ms"], 3), "k_roll_query_ms": round(med(fused[n]["k_roll_query_ms"]), 3),
                                                "call_ms": round(med(fused[n]["call_ms"]), 3)} for n in fused},
                                         "within": r["fused_within_yardstick"]}), flush=True)
            ctx.close()
            scratch.close()
            del d_text, d_keys, d_counts, d_track
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
