"""Contiger at 64 < k <= 191: the k-mer windows, map keys and contig ends of the device code in 4 or 6 64-bit words
(ShkKmer, sh-assembly_amd/csrc/shk_device.h). Held to what k <= 64 is held to: the whole pipeline against the sequential
restatement (oracle/contiger_pipeline.cpp), single unitigs against the oracle's get_unitig_forward, the closure, the
compacted-graph invariants, and the argument limits. The CPU part runs the emulator build (tests/emu); the GPU part
(-m gpu) the gfx950 library and the command lines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cqflibs
import synth
from fastq_util import chunks_by_records, oracle_t1
from test_emu_kernels import EMU, _ctx, _find_unitigs_case, _read_unitigs, _unitig_case, shk  # noqa: F401 (shk: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHK_ERR_ARG = -1


def _qb_for(G, nreads, L, err, k, lo):
    """a filter three times the distinct k-mers the reads can hold (genome + error k-mers), as tools/fuzz_contiger.py sizes it"""
    qb = lo
    while (1 << qb) < 3 * (G + nreads * L * err * k):
        qb += 1
    return qb


# ---------------------------------------------------------------- CPU: the emulator build

@pytest.mark.parametrize("k", [65, 96, 128, 129, 191])
@pytest.mark.parametrize("per_read", [True, False])
def test_wide_k_whole_pipeline_against_the_sequential_restatement(shk, tmp_path, k, per_read):
    """seeds from reads -> walks -> queued contigs -> duplicate removal -> numbering -> links -> unitigs.fa at wide k ==
    the sequential restatement: canonical sequences, links, and km / KC under the read-by-read schedule (admissible km
    when all chunks are one batch). A genome with two repeats, a plasmid longer than k, errors, N and lower case."""
    import contiger_cases as CC
    L, G = k + 70, 1500
    nreads = G * 24 // L
    fq = CC.reads(G=G, nreads=nreads, L=L, err=0.003, plasmid=k + 45, seed=100 + k)
    qb = _qb_for(G, nreads, L, 0.003, k, 13)
    r = CC.run_case(lambda **kw: _ctx(shk, **kw), shk.UnitigSet, tmp_path, k=k, qb=qb, fq=fq, chunk_reads=40,
                    per_read=per_read, max_len=16000)
    assert r["unitigs"] >= 3 and r["links"] >= 1, r


@pytest.mark.parametrize("k", [65, 127, 191])
def test_wide_k_unitigs_from_seeds_match_oracle(shk, k):
    """k_extend_forward<W> (one thread per open end, rolled hashes) against the oracle's restatement of
    get_unitig_forward (hashes from scratch): sequence, median abundance and both stop reasons per seed"""
    stops = _unitig_case(shk, lambda **kw: _ctx(shk, **kw), qb=14, k=k, G=700, nreads=40, L=k + 80, err=0.003, nseeds=12)
    assert stops


def test_wide_k_find_unitigs_matches_oracle_closure(shk, tmp_path, monkeypatch):
    """the unitig set (k_ug_walk<4>, queued branch neighbours, k_ug_check / emit / map2 / links) at k = 96 against an
    independent closure over the oracle's get_unitig_forward; walks continue over several launches"""
    monkeypatch.setenv("SHK_WALK_STEP", "23")
    g, got, st = _find_unitigs_case(lambda **kw: _ctx(shk, **kw), tmp_path, qb=14, k=96, G=700, nreads=60, L=170, err=0.004,
                                    repeat=130, seed_every=6)
    assert st["rounds"] >= 3 and len(got) >= 2


@pytest.mark.parametrize("mark", [0, 1])
def test_wide_k_unitig_set_invariants(shk, tmp_path, mark):
    """the output at k = 129 is the compacted graph of the solid k-mers (tests/unitig_invariants.py): a genome with a repeat
    longer than k and a plasmid that comes out as one pure circle; with and without the traveled-bit protocol"""
    import unitig_invariants as UI
    k, qb = 129, 14
    g = synth.make_genome(700, 17)
    g = np.concatenate([g[:420], g[100:250], g[420:]])
    plasmid = synth.make_genome(180, 19)
    fq = synth.make_fastq(g, 70, 200, 0.002, seed=19) + \
        synth.make_fastq(np.concatenate([plasmid, plasmid, plasmid[:90]]), 30, 180, 0.0, seed=23, name_prefix="p")
    offs, lens = chunks_by_records(fq, 40)
    q, _, _ = oracle_t1(fq, offs, lens, k, qb)
    assert not q.full()
    ctx = _ctx(shk, qb=qb, k=k, max_batch_bytes=len(fq) + 1024, max_batch_keys=1 << 15)
    ctx.count_chunks(fq, offs, lens)
    O = cqflibs.oracle()

    def count(km):
        fh, rh = O.nthash(km, k)
        return q.count(min(fh, rh) & ((1 << (qb + 8)) - 1))
    out = str(tmp_path / "u.fa")
    u = shk.UnitigSet(ctx)
    seeds = [ln[len(ln) // 2 - k // 2:][:k].upper() for ln in fq.split(b"\n")[1::4]]
    seeds = [s for s in seeds if len(s) == k and b"N" not in s and count(s) >= 2]
    if mark:
        assert u.add_reads(fq, offs, lens, k, 2, 2, 1000000, 8000) >= 3
    else:
        half = len(seeds) // 2
        u.add_seeds(seeds[:half], [count(s) for s in seeds[:half]], k, 2, 8000, mark_traveled=False)
        u.add_seeds(seeds[half:], [count(s) for s in seeds[half:]], k, 2, 8000, mark_traveled=False)
    st = u.write(k, out)
    u.close()
    got = _read_unitigs(out, k)
    seqs = [ln for ln in open(out, "rb").read().split(b"\n")[1::2] if ln]
    assert st["unitigs"] == len(seqs) == len(got) and st["truncated"] == 0
    UI.check(seqs, UI.Graph(count, k, 2), seeds=seeds)
    assert any(len(x) == 180 + k - 1 and x[-(k - 1):] == x[:k - 1] for x in seqs)      # the plasmid as one pure circle
    assert len(seqs) >= 3                                                               # the repeat cut the genome
    ctx.close()
    q.free()


def _select_seeds(L, ctx, text, k):
    L.shk_select_seeds.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.POINTER(C.c_uint32),
                                   C.c_uint32, C.POINTER(C.c_uint32)]
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(len(text))
    buf = C.create_string_buffer(text, len(text))
    seeds, counts, n = C.create_string_buffer(64 * 200), (C.c_uint32 * 64)(), C.c_uint32()
    return L.shk_select_seeds(ctx.h, C.cast(buf, C.c_void_p), 0, len(text), off, ln, 1, k, 2, 1000000, 0, seeds, counts, 64, C.byref(n))


def _extend_forward(L, ctx, km, k):
    n, max_ext = 1, 16
    ext, cnt, en, st = C.create_string_buffer(max_ext), (C.c_uint32 * max_ext)(), (C.c_uint32 * 1)(), (C.c_uint8 * 1)()
    return L.shk_extend_forward(ctx.h, km, km, n, k, 2, 0, max_ext, ext, cnt, en, st, None, None)


def test_wide_k_limits(shk):
    """k = 192 and k < 2 are refused with SHK_ERR_ARG by every Contiger entry point; k = 191 is accepted; a unitig set
    keeps the k of its first call"""
    fq = synth.make_fastq(synth.make_genome(600, 5), 12, 240, 0.0, seed=7)
    offs, lens = chunks_by_records(fq, 6)
    ctx = _ctx(shk, qb=12, k=191, max_batch_bytes=len(fq) + 1024, max_batch_keys=1 << 13)
    ctx.count_chunks(fq, offs, lens)
    L = ctx.L
    line = fq.split(b"\n")[1]
    for k in (192, 1, 0):
        km = (line * 2)[:max(k, 1)]
        assert _select_seeds(L, ctx, fq, k) == SHK_ERR_ARG
        assert _extend_forward(L, ctx, km, k) == SHK_ERR_ARG
        with pytest.raises(shk.ShkError) as e:
            ctx.unitigs_from_seeds([km], [3], k, 2, 4000)
        assert e.value.code == SHK_ERR_ARG
        with pytest.raises(shk.ShkError) as e:
            ctx.find_unitigs([km], [3], k, 2, 4000, os.devnull)
        assert e.value.code == SHK_ERR_ARG
        u = shk.UnitigSet(ctx)
        with pytest.raises(shk.ShkError) as e:
            u.add_seeds([km], [3], k, 2, 4000)
        assert e.value.code == SHK_ERR_ARG
        with pytest.raises(shk.ShkError) as e:
            u.add_reads(fq, offs, lens, k, 2, 2, 1000000, 4000)
        assert e.value.code == SHK_ERR_ARG
        u.close()
    # the top of the range works through every entry point
    k = 191
    assert _select_seeds(L, ctx, fq, k) == 0
    assert _extend_forward(L, ctx, line[:k], k) == 0
    assert len(ctx.unitigs_from_seeds([line[:k]], [3], k, 2, 4000)[0][0]) >= k
    u = shk.UnitigSet(ctx)
    u.add_reads(fq, offs, lens, k, 2, 2, 1000000, 4000)
    with pytest.raises(shk.ShkError) as e:          # one set, one k (and one W)
        u.add_seeds([line[:128]], [3], 128, 2, 4000)
    assert e.value.code == SHK_ERR_ARG
    u.close()
    ctx.close()


def test_wide_k_fuzz_on_the_emulator(shk):
    """tools/fuzz_contiger.py --wide on the emulator build: random genomes, k 65 .. 191, read lengths, thresholds and
    schedules; a case the library refuses counts as a failure there"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_contiger.py"), "--emu", "--wide", "--cases", "6", "--seed", "3"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "6 cases, 0 mismatches, 0 skipped" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]


# ---------------------------------------------------------------- GPU: the gfx950 library

def _gctx(**kw):
    import shk as m
    return m.Context(**kw)


@pytest.mark.gpu
@pytest.mark.parametrize("k,per_read", [(65, False), (95, True), (128, False), (191, True)])
def test_gpu_wide_k_whole_pipeline_against_the_sequential_restatement(tmp_path, k, per_read):
    """the whole of Contiger on the GPU at wide k against the sequential restatement (tests/contiger_cases.py): canonical
    sequences and links equal; km / KC equal under the read-by-read schedule, admissible otherwise. A genome with repeats,
    a plasmid (pure circles), errors, N and lower-case reads. k = 191 runs read by read: with 300-base reads the batched
    schedule seeds a few small components that the sequential one never seeds (their middle k-mers are marked traveled
    first), more than the batched comparison tolerates."""
    import shk
    import contiger_cases as CC
    L = min(250 if k < 128 else 300, k + 155)      # (run_case's key budget: 40 per FASTQ line)
    G, nreads = (24000, 2400) if not per_read else (6000, 600)
    fq = CC.reads(G=G, nreads=nreads, L=L, err=0.001, plasmid=700, seed=41)
    qb = _qb_for(G, nreads, L, 0.001, k, 17)
    r = CC.run_case(_gctx, shk.UnitigSet, tmp_path, k=k, qb=qb, fq=fq, chunk_reads=600, per_read=per_read, max_len=1 << 17)
    assert r["unitigs"] >= 8 and r["links"] >= 8, r


@pytest.mark.gpu
def test_gpu_wide_k_cli_from_gpu_built_cqf(tmp_path):
    """the README chain at k = 95: bin/CQF-deNoise -k 95 builds the .cqf on the GPU, bin/Contiger -k 95 loads it and writes
    unitigs.fa; the unitigs satisfy the compacted-graph invariants against the filter as the oracle reads it back"""
    import unitig_invariants as UI
    from test_gpu_parity import _fasta_seqs, _oracle_counter
    bind = os.path.join(ROOT, "sh-assembly_amd", "bin")
    k, G = 95, 30000
    g = synth.make_genome(G, 51)
    g = np.concatenate([g[:14000], g[5000:5500], g[14000:]])
    (tmp_path / "a.fq").write_bytes(synth.make_fastq(g, 1500, 250, 0.002, seed=53))
    (tmp_path / "b.fq").write_bytes(synth.make_fastq(g, 1500, 250, 0.002, seed=55, name_prefix="s"))
    (tmp_path / "files.txt").write_text("a.fq\nb.fq\n")
    cqf = str(tmp_path / "k95.cqf")
    r = subprocess.run([os.path.join(bind, "CQF-deNoise"), "-k", str(k), "-N", "800000", "-n", "30000", "-e", "0.002", "-f", "f",
                        "-i", str(tmp_path / "files.txt"), "-o", cqf, "--part-size", "100000", "--overhead", "4000"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = str(tmp_path / "unitigs.fa")
    r = subprocess.run([os.path.join(bind, "Contiger"), "-k", str(k), "-i", str(tmp_path / "files.txt"), "-c", cqf, "-o", out,
                        "--part-size", "100000", "--overhead", "4000", "--batch-chunks", "3"], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    import struct
    nslots = struct.unpack_from("<Q", open(cqf, "rb").read(128), 16)[0]
    qb = nslots.bit_length() - 1
    q = cqflibs.oracle().load(cqf)
    count = _oracle_counter(q, k, qb)
    seqs = _fasta_seqs(out)
    _read_unitigs(out, k)
    fq = (tmp_path / "a.fq").read_bytes() + (tmp_path / "b.fq").read_bytes()
    seeds = []
    for line in fq.split(b"\n")[1::4]:
        km = line[len(line) // 2 - k // 2:][:k]
        if len(km) == k and b"N" not in km and 2 <= count(km) <= 1000000:
            seeds.append(km)
    O = cqflibs.oracle()

    def key(km):
        fh, rh = O.nthash(km, k)
        return min(fh, rh) & ((1 << (qb + 8)) - 1)
    UI.check(seqs, UI.Graph(count, k, 2), seeds=seeds, key=key)
    assert len(seqs) >= 3 and "truncated: 0" in r.stderr
    # above the limit: one line naming it, non-zero exit
    r = subprocess.run([os.path.join(bind, "Contiger"), "-k", "192", "-i", str(tmp_path / "files.txt"), "-c", cqf, "-o", out],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode != 0 and "191" in r.stderr
    q.free()


@pytest.mark.gpu
def test_gpu_wide_k_randomised_against_the_sequential_restatement():
    """tools/fuzz_contiger.py --wide on the GPU: random genomes, k 65 .. 191, read lengths, thresholds, schedules"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_contiger.py"), "--wide", "--cases", "40", "--seed", "9",
                        "--scale", "8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "40 cases, 0 mismatches, 0 skipped" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]


@pytest.mark.gpu
def test_gpu_wide_k_larger_case_against_the_restatement(tmp_path):
    """k = 127 at a larger size: a 4 Mb genome, 1 M reads of 250 bases (text generated on the device, tools/bench_contiger.py),
    qb 24; the device's unitigs.fa against the sequential restatement over the same .cqf and chunks: canonical sequence
    and link sets equal up to the seeds whose filter key another k-mer shares (unitig_compare.explain_one_sided)"""
    import importlib.util
    import unitig_compare as UC
    import contiger_cases as CC
    spec = importlib.util.spec_from_file_location("bench_contiger", os.path.join(ROOT, "tools", "bench_contiger.py"))
    bc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bc)

    class A:
        genome, reads, read_len, err, k, qb, amin, xmin, max_len, batch_chunks = 4_000_000, 1_000_000, 250, 0.0002, 127, 24, 2, 2, 1 << 24, 16
    torch, shk, ctx, text, offs, lens, _ = bc.build(A)
    cqf = str(tmp_path / "k127.cqf")
    ctx.export_cqf(cqf)
    out = str(tmp_path / "unitigs.fa")
    nseeds, st, t_walk, t_write, walk_ms, prof = bc.walk(shk, ctx, text, offs, lens, A, out)
    assert st["truncated"] == 0
    host = text.cpu().numpy().tobytes()
    del text
    ctx.close()
    k = A.k
    q = cqflibs.oracle().load(cqf)
    orc_fa, ost = q.contiger(host, offs, lens, k, A.amin, A.xmin, 1000000, 1, True)
    q.free()
    dev = UC.canonical(UC.parse(open(out, "rb").read(), k), k)
    orc = UC.canonical(UC.parse(orc_fa, k), k, drop_invalid=True)
    assert dev[2] == 0
    one_sided = set(dev[0]) ^ set(orc[0])
    both = set(dev[0]) & set(orc[0])
    assert len(one_sided) <= max(4, len(both) // 500), (len(dev[0]), len(orc[0]), len(one_sided))
    UC.explain_one_sided(one_sided, both, k, A.qb + 8, CC.seed_kmers(host, k), cqflibs.oracle().seq_keys)
    dl = {l for l in dev[1] if l[0] in both and l[2] in both}
    ol = {l for l in orc[1] if l[0] in both and l[2] in both}
    assert dl == ol, (len(dl), len(ol), len(dl ^ ol))
    assert sum(len(c) - k + 1 for c in both) >= 0.95 * A.genome
    print("k127 unitigs", len(dev[0]), "links", len(dev[1]), "walk wall", t_walk, "walk kernel ms", walk_ms)
