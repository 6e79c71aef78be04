#!/usr/bin/env python3
"""Side bench of the FASTA front end (not bench.py): a synthetic genome as one record of 60-column FASTA, on the device,
counted by shk_count_fasta with SHK_FASTA_SEGMENT = 128, 256 (the default), 1024 and 4096; and, for comparison, the same bases
cut into 150-base reads and counted as FASTQ by shk_count_chunks (kernels this work does not touch). Every configuration
gets a context of its own, one untimed call (code objects load, buffers are allocated) and --reps timed ones into the same
table. Reported per 10^9 bases: the library's per-kernel HIP-event times (shk_profile_*) grouped as

  front   what turns text into the roll kernels' input: k_fa_* + the scans (FASTA); k_count_lines, k_scan_chunks,
          k_emit_reads, k_pack_reads + the scans (FASTQ)
  roll    k_roll_hist + k_roll_scatter (the FASTQ batch may run slotted, without k_roll_hist; the FASTA path never does)
  rest    partition and rebuild

and the whole call by the host's clock. The FASTQ text holds G / 150 * 104 k-mers at k = 47 against the FASTA's G - 46:
compare `front` and `roll` per base, not `rest`. Writes one JSON document (default profiles/fasta_bench.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sh-assembly_amd"))

FRONT = {"fasta": ("k_fa_maps", "k_fa_states", "k_fa_count", "k_fa_compact", "k_fa_segments+long+tail", "k_fa_pack", "k_scan_*"),
         "fastq": ("k_count_lines", "k_scan_chunks", "k_emit_reads", "k_pack_reads", "k_scan_*")}
ROLL = ("k_roll_hist", "k_roll_scatter")


def run(shk, torch, mk_ctx, do_call, reps, nbases, form):
    ctx = mk_ctx()
    do_call(ctx)
    ctx.profile(True)
    ctx.profile_reset()
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = do_call(ctx)
        wall.append((time.perf_counter() - t0) * 1e3)
    prof = {name: ms / reps for name, (n, ms) in ctx.profile_get().items() if n}
    ctx.profile(False)
    ctx.close()
    per = 1e9 / nbases
    front = sum(prof.get(n, 0.0) for n in FRONT[form])
    roll = sum(prof.get(n, 0.0) for n in ROLL)
    return {"kmers_per_call": st["kmers"], "kernel_ms_per_call": prof, "call_ms": sorted(wall),
            "front_ms_per_Gbase": front * per, "roll_ms_per_Gbase": roll * per,
            "rest_ms_per_Gbase": (sum(prof.values()) - front - roll) * per, "call_ms_per_Gbase": sorted(wall)[len(wall) // 2] * per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=64_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--qb", type=int, default=28)
    ap.add_argument("--segments", default="128,256,1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_bench.json"))
    a = ap.parse_args()
    import torch
    import shk
    dev = torch.device("cuda", 0)
    K, L = 47, 150
    G = a.bases // (60 * L) * (60 * L)
    code = torch.randint(0, 4, (G,), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(2))
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[code.long()]
    del code
    # FASTA: ">g\n" + lines of 60 bases; padded in front so that the text starts 16-byte aligned
    lines = torch.full((G // 60, 61), 10, dtype=torch.uint8, device=dev)
    lines[:, :60] = seq.view(-1, 60)
    fa = torch.cat([torch.tensor(list(b">g\n"), dtype=torch.uint8, device=dev), lines.view(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    del lines
    fa_bytes = fa.numel() - 16
    # FASTQ: records of "@\n" bases "\n+\n" qualities "\n"
    nreads = G // L
    rec = 2 * L + 6
    fq = torch.full((nreads, rec), ord("I"), dtype=torch.uint8, device=dev)
    fq[:, 0] = ord("@")
    fq[:, 1] = 10
    fq[:, 2:2 + L] = seq.view(-1, L)
    fq[:, 2 + L] = 10
    fq[:, 3 + L] = ord("+")
    fq[:, 4 + L] = 10
    fq[:, rec - 1] = 10
    fq = torch.cat([fq.view(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    fq_bytes = fq.numel() - 16
    del seq
    torch.cuda.synchronize()
    nchunks = 64
    per = (nreads + nchunks - 1) // nchunks
    offs = [i * per * rec for i in range(nchunks) if i * per < nreads]
    lens = [min(per, nreads - i * per) * rec for i in range(len(offs))]
    res = {"metric": "FASTA front end against the FASTQ one, ms per 10^9 bases", "bases": G, "k": K, "qb": a.qb, "reps": a.reps,
           "fasta_bytes": fa_bytes, "fastq_bytes": fq_bytes, "fasta": {}}
    for seg in [int(s) for s in a.segments.split(",")]:
        os.environ["SHK_FASTA_SEGMENT"] = str(seg)
        res["fasta"][str(seg)] = run(
            shk, torch, lambda: shk.Context(qb=a.qb, k=K, max_batch_bytes=fa_bytes + 64, max_batch_keys=G + 4096),
            lambda ctx: ctx.count_fasta(fa.data_ptr(), first=True, on_device=True, text_bytes=fa_bytes)[0], a.reps, G, "fasta")
    os.environ.pop("SHK_FASTA_SEGMENT", None)
    res["fastq_150"] = run(
        shk, torch, lambda: shk.Context(qb=a.qb, k=K, max_batch_bytes=64, max_batch_keys=nreads * (L - K + 1) + 4096, max_batch_reads=nreads + 1024),
        lambda ctx: ctx.count_chunks(fq.data_ptr(), offs, lens, on_device=True, text_bytes=fq_bytes), a.reps, G, "fastq")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("fasta", "fastq_150")}))
    for name, r in list(res["fasta"].items()) + [("fastq_150", res["fastq_150"])]:
        print(name, {k: round(v, 3) for k, v in r.items() if k.endswith("_per_Gbase")})


if __name__ == "__main__":
    main()
