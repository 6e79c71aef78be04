#!/usr/bin/env python3
"""Side bench of the read-side analytics (not bench.py): builds the filter bench.py --steps builds (same generator,
same sizing, serial counting), then times on it, with the library's own per-kernel HIP-event times (shk_profile_*):

  k_region_spectrum    shk_spectrum(nbins = 256)
  k_region_join        shk_inner_product(ctx, ctx)
  k_region_dump<0>     shk_dump in count-only mode (keys == NULL): the same staging and walk and nothing else -- the
                       yardstick. The spectrum should cost that plus its LDS atomics, the self inner product about twice
                       the staging. More than 1.5 x (spectrum vs the dump pass; inner product vs twice the dump pass)
                       would point at per-entry global atomics or a collapsed occupancy.

Prints one JSON line. The GB/s figures are table bytes staged over kernel time: one-wave workgroups that walk entries
lane by lane are latency-bound like the dump, so expect a small fraction of the HBM peak; this is not a roofline result."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sh-assembly_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reads-per-step", type=int, default=8_000_000)
    ap.add_argument("--genome", type=int, default=119_157_843)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import bench
    import shk
    from shk import plan
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K, L, ERR = 47, 150, 0.00234
    R = args.reads_per_step
    rec = 2 * L + bench.NAME_W + 6
    offs, lens = bench.chunk_table(R, rec)
    B = min(args.steps, bench.BUILD_STEPS)
    pl = plan.plan_build(K, args.genome, L, ERR, R * (L - K + 1) / len(offs), len(offs) * B)
    qb = pl["qb"]
    ctx = shk.Context(qb=qb, k=K, trigger=pl["trigger"], num_denoise=pl["rounds"], max_batch_bytes=64,
                      max_batch_keys=R * (L - K + 1) + 4096, max_batch_reads=R + 1024)
    genome = torch.randint(0, 4, (args.genome,), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(2))
    for s in range(B):
        t = bench.gen_batch_torch(torch, genome, R, L, ERR, s * R, 1000 + s, dev)
        torch.cuda.synchronize()
        ctx.count_chunks(t.data_ptr(), offs, lens, on_device=True, text_bytes=t.numel())
        del t
    tot = ctx.totals()

    def count_only_dump():
        n = C.c_uint64()
        ctx._chk(ctx.L.shk_dump(ctx.h, None, None, 0, 0, 0, C.byref(n)))
        return n.value

    # one untimed call each: the first reader launches the pending placement, and the code objects load
    entries = count_only_dump()
    hist, totals = ctx.spectrum(256)
    ip = ctx.inner_product(ctx)
    assert totals["distinct"] == entries == tot.ndistinct and totals["total"] == tot.nelts and ip == totals["sumsq"]
    assert sum(hist) == entries

    def timed(f, name):
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(args.reps):
            f()
        n, ms = ctx.profile_get()[name]
        ctx.profile(False)
        assert n == args.reps, (name, n)
        return ms / n

    dump_ms = timed(count_only_dump, "misc")
    spec_ms = timed(lambda: ctx.spectrum(256), "k_region_spectrum")
    join_ms = timed(lambda: ctx.inner_product(ctx), "k_region_join")
    gb = tot.table_bytes / 1e9
    print(json.dumps({"metric": "filter analytics, kernel ms on the built filter", "qb": qb, "steps": B, "table_GB": gb,
                      "entries": entries, "kmers": tot.nelts, "max_count": totals["max_count"], "free_pointer_frac": tot.free_pointer / tot.xnslots,
                      "dump_count_pass_ms": dump_ms, "spectrum_ms": spec_ms, "self_inner_product_ms": join_ms,
                      "spectrum_over_dump": spec_ms / dump_ms, "inner_product_over_2x_dump": join_ms / (2 * dump_ms),
                      "dump_GBps": gb / (dump_ms / 1e3), "spectrum_GBps": gb / (spec_ms / 1e3),
                      "inner_product_GBps_two_tables_staged": 2 * gb / (join_ms / 1e3), "reps": args.reps}))
    ctx.close()


if __name__ == "__main__":
    main()
