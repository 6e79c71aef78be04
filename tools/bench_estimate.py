#!/usr/bin/env python3
"""Side bench of the sampling front end (not bench.py): shk_sample_chunks on batches of bench.py's generator.

Time, on ONE bench batch (8 M reads of 150 bases, 832 M k-mers at k = 47, text on the device): the device time of
k_roll_sample at s = 8 and s = 4 against k_roll_hist<10, 256> over the same batch staged the same way (k_pack_reads) in
the same process -- an existing kernel with the same arithmetic that writes nothing but its counters, reached through
shk_hash_route_chunks -- and the whole shk_sample_chunks call (parse + pack + sample + rebuild of the small table) by the
host's clock. Every configuration gets a context of its own, one untimed call and --reps timed ones.

Accuracy, over --batches batches: F0, f1, f2, n = F0 - f1 - f2 and e as python -m shk.estimate derives them from the
sampled table, against shk_spectrum of an exact build of the same text (no deNoise rounds, --exact-qb slots), with the
sampling standard deviation sqrt((2^s - 1) / X) of each quantity X next to its relative error.

Writes one JSON document (default profiles/estimate_bench.json)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sh-assembly_amd"))

FRONT = ("k_count_lines", "k_scan_chunks", "k_emit_reads", "k_pack_reads", "k_scan_*")


def timed(torch, ctx, call, reps):
    """one untimed call, then `reps` profiled ones: (mean kernel ms by name, sorted wall ms, last result)"""
    call()
    ctx.profile(True)
    ctx.profile_reset()
    wall, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    prof = {name: ms / reps for name, (n, ms) in ctx.profile_get().items() if n}
    ctx.profile(False)
    return prof, sorted(wall), out


def quantities(hist, distinct, total, k):
    from shk.plan import params_from_spectrum
    f1, f2 = int(hist[0]), int(hist[1])
    _, n, e = params_from_spectrum(distinct, total, hist, k, 2)
    return {"F0": int(distinct), "f1": f1, "f2": f2, "n": n, "e": e}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads-per-step", type=int, default=8_000_000)
    ap.add_argument("--genome", type=int, default=119_157_843)
    ap.add_argument("--batches", type=int, default=3, help="batches of the accuracy part")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="8:24,4:26", help="s:qb of the sampled contexts")
    ap.add_argument("--exact-qb", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_bench.json"))
    a = ap.parse_args()
    import torch
    import shk
    import bench
    dev = torch.device("cuda", 0)
    K, L, ERR = 47, 150, 0.00234
    R = a.reads_per_step
    rec = 2 * L + bench.NAME_W + 6
    offs, lens = bench.chunk_table(R, rec)
    text_bytes = R * rec
    nk = R * (L - K + 1)
    genome = torch.randint(0, 4, (a.genome,), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(2))
    texts = [torch.cat([bench.gen_batch_torch(torch, genome, R, L, ERR, s * R, 1000 + s, dev), torch.zeros(16, dtype=torch.uint8, device=dev)])
             for s in range(a.batches)]
    del genome
    torch.cuda.synchronize()
    configs = [tuple(int(x) for x in c.split(":")) for c in a.configs.split(",")]
    res = {"metric": "shk_sample_chunks on bench batches: kernel and call times in ms per batch, estimates against an exact build",
           "k": K, "reads_per_batch": R, "kmers_per_batch": nk, "text_bytes_per_batch": text_bytes, "chunks_per_batch": len(offs), "reps": a.reps,
           "time": {}, "accuracy": {}}

    def sample_ctx(s, qb):
        # the tool's capacities: keys = text / 16 (the 2-bit staging needs about text / 27), more for a small s
        return shk.Context(qb=qb, k=K, max_batch_bytes=64, max_batch_keys=max(text_bytes // 16, text_bytes >> (s + 1)), max_batch_reads=R + 1024)

    # ---- time
    ctx = shk.Context(qb=24, k=K, max_batch_bytes=64, max_batch_keys=nk + 4096, max_batch_reads=R + 1024)
    prof, wall, _ = timed(torch, ctx, lambda: ctx.hash_route_chunks(texts[0].data_ptr(), offs, lens, 1, on_device=True, text_bytes=text_bytes), a.reps)
    ctx.close()
    hist_ms = prof["k_roll_hist"]
    res["time"]["k_roll_hist<10,256>"] = {"kernel_ms": prof, "k_roll_hist_ms": hist_ms}
    for s, qb in configs:
        ctx = sample_ctx(s, qb)
        prof, wall, (st, ss) = timed(torch, ctx, lambda: ctx.sample_chunks(texts[0].data_ptr(), offs, lens, s, on_device=True, text_bytes=text_bytes), a.reps)
        ctx.close()
        assert 0 < ss["kmers"] <= nk, ss          # (reads that carry an N give fewer k-mers)
        front = sum(prof.get(n, 0.0) for n in FRONT)
        res["time"]["s=%d" % s] = {"qb": qb, "kept_per_batch": ss["kept"], "kmers": ss["kmers"], "kernel_ms": prof, "k_roll_sample_ms": prof["k_roll_sample"],
                                   "ratio_to_k_roll_hist": prof["k_roll_sample"] / hist_ms, "front_ms": front,
                                   "rest_ms": sum(prof.values()) - front - prof["k_roll_sample"], "call_ms": wall, "call_ms_median": wall[len(wall) // 2]}

    # ---- accuracy
    exact = shk.Context(qb=a.exact_qb, k=K, max_batch_bytes=64, max_batch_keys=nk + 4096, max_batch_reads=R + 1024)
    total = 0
    for t in texts:
        total += exact.count_chunks(t.data_ptr(), offs, lens, on_device=True, text_bytes=text_bytes)["kmers"]
    hist, tot = exact.spectrum(256)
    exact.close()
    assert tot["total"] == total
    want = quantities(hist, tot["distinct"], tot["total"], K)
    res["accuracy"]["exact"] = dict(want, F1=total, qb=a.exact_qb, batches=a.batches)
    for s, qb in configs:
        ctx = sample_ctx(s, qb)
        kmers = 0
        for t in texts:
            kmers += ctx.sample_chunks(t.data_ptr(), offs, lens, s, on_device=True, text_bytes=text_bytes)[1]["kmers"]
        h, tt = ctx.spectrum(256)
        ctx.close()
        got = quantities([int(f) << s for f in h], tt["distinct"] << s, kmers, K)
        row = {"qb": qb, "entries": tt["distinct"], "F1": kmers, "F1_exact": kmers == total}
        for key in ("F0", "f1", "f2", "n"):
            row[key] = {"estimate": got[key], "relative_error": (got[key] - want[key]) / want[key],
                        "sampling_sigma": math.sqrt(((1 << s) - 1) / want[key])}
        row["e"] = {"estimate": got["e"], "exact": want["e"], "relative_error": (got["e"] - want["e"]) / want["e"]}
        res["accuracy"]["s=%d" % s] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"k_roll_hist_ms": hist_ms, **{key: {"k_roll_sample_ms": v["k_roll_sample_ms"], "ratio": v["ratio_to_k_roll_hist"], "call_ms": v["call_ms_median"]}
                                                    for key, v in res["time"].items() if key.startswith("s=")}}))
    for key, v in res["accuracy"].items():
        print(key, json.dumps(v))


if __name__ == "__main__":
    main()
