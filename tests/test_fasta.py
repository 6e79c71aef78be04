"""shk_count_fasta (tests/fasta_cases.py): every case once on the CPU emulator build of the kernel sources (test_emu_*)
and once on the gfx950 library (test_gpu_*, -m gpu); the host pieces need neither. Most cases lower SHK_FASTA_SEGMENT to
50 (unaligned) and 64 (a whole unit), so that texts of a few hundred bytes cross segment and unit boundaries."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import cqflibs
import fasta_cases as FC
from test_emu_kernels import EMU, _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGS = [50, 64]
CUTS = ["inside_header", "behind_gt", "between_cr_lf", "few_bases_behind_break", "on_a_break", "behind_a_break", "on_segment_end",
        "inside_second_header"]


def _emu_factory(shk):     # noqa: F811
    return lambda **kw: _emu_ctx(shk, **kw)


def _emu_bytes(b):
    buf = (C.c_char * (len(b) + 32))()
    at = (-C.addressof(buf)) % 16
    C.memmove(C.addressof(buf) + at, b, len(b))
    return C.addressof(buf) + at, buf


def _gpu_factory():
    import shk as gshk
    return lambda **kw: gshk.Context(**kw)


def _gpu_bytes(b):
    import torch
    t = torch.frombuffer(bytearray(b + b"\0" * 16), dtype=torch.uint8).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t.data_ptr(), t


# ---------------------------------------------------------------- host pieces (no device)
def test_seq_keys_serves_as_reference():
    """what the expected values rest on: seq_keys takes a 200 kb run, agrees with itself on overlapping segments and
    treats case alike"""
    O = cqflibs.oracle()
    k, hb = 47, 30
    s = FC.dna(200_000, 3)
    whole = O.seq_keys([s], k, hb)
    assert len(whole) == len(s) - k + 1
    S = 1024
    segs = [s[i:i + S + k - 1] for i in range(0, len(s) - k + 1, S)]
    assert np.array_equal(np.concatenate([O.seq_keys([x], k, hb) for x in segs]), whole)
    assert np.array_equal(O.seq_keys([s[:5000].lower()], k, hb), whole[:5000 - k + 1])
    fh, rh = O.nthash(s[:k], k)
    assert int(whole[0]) == min(fh, rh) & ((1 << hb) - 1)


def test_reader_is_the_grammar():
    r = FC.Reader(3)
    st = r.feed(b"AC\nGT\r\n>ACGT\nacN-gt>a\n;x\n\nTTT")
    assert r.all_runs() == [b"ACGT", b"ac", b"gt", b"a", b"TTT"]
    assert st == {"records": 2, "bases": 12, "breaks": 3, "kmers": 3}


def test_report_format():
    from shk.fasta import format_report
    fs, against, want = FC.report_case()
    assert format_report(fs, against["distinct"], against) == want
    assert format_report(fs, 850) == "records\t3\nbases\t1000\nbreaks\t12\nk-mers\t900\ndistinct\t850\n"
    against = dict(against, distinct=0, present=0, solid=0)
    assert "present\t0\t0.00%" in format_report(fs, 0, against)


def test_binding_mirrors_the_header():
    import re
    import shk as m
    hdr = open(os.path.join(ROOT, "include", "shk.h")).read()
    assert int(re.search(r"#define SHK_FASTA_SEGMENT (\d+)", hdr).group(1)) == m.FASTA_SEGMENT
    assert "shk_count_fasta" in m.EXPORTS


# ---------------------------------------------------------------- CPU emulator
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", [5, 47])
def test_emu_grammar(shk, k, seg):     # noqa: F811
    FC.run_grammar(_emu_factory(shk), k, seg)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", FC.K_LIST)
def test_emu_run_lengths(shk, k, seg):     # noqa: F811
    FC.run_run_lengths(_emu_factory(shk), k, seg)


@pytest.mark.parametrize("seg", SEGS)
def test_emu_offsets(shk, seg):     # noqa: F811
    FC.run_offsets(_emu_factory(shk), 33, seg)


@pytest.mark.parametrize("k", [3, 21])
def test_emu_soup(shk, k):     # noqa: F811
    FC.run_soup(_emu_factory(shk), k, 16)


def test_emu_long_runs(shk):     # noqa: F811
    FC.run_long_runs(_emu_factory(shk))


def test_emu_default_segment(shk):     # noqa: F811
    FC.run_default_segment(_emu_factory(shk))


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("cut", CUTS)
def test_emu_chosen_cut(shk, cut, seg):     # noqa: F811
    FC.run_chosen_cut(_emu_factory(shk), 47, seg, cut)


def test_emu_byte_by_byte(shk):     # noqa: F811
    FC.run_byte_by_byte(_emu_factory(shk), 31, 50)


@pytest.mark.parametrize("seg", SEGS)
def test_emu_fastq_agreement(shk, seg):     # noqa: F811
    FC.run_fastq_agreement(_emu_factory(shk), 47, seg)


def test_emu_trigger(shk):     # noqa: F811
    FC.run_trigger(_emu_factory(shk), 31, 64)


@pytest.mark.parametrize("qb,mlb,levels", FC.GEOMETRIES)
def test_emu_geometry(shk, qb, mlb, levels):     # noqa: F811
    FC.run_geometry(_emu_factory(shk), 47, 50, qb, mlb)


def test_emu_errors(shk):     # noqa: F811
    FC.run_errors(_emu_factory(shk), 47, 50, _emu_bytes)


def test_emu_cli(shk, tmp_path):     # noqa: F811
    import io
    from shk.fasta import main

    def call(argv):
        out = io.StringIO()
        assert main(argv + ["--lib", EMU, "--piece", "1000"], out=out) == 0
        return out.getvalue()
    _run_cli(call, tmp_path)


# ---------------------------------------------------------------- gfx950
@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", [5, 47])
def test_gpu_grammar(k, seg):
    FC.run_grammar(_gpu_factory(), k, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", FC.K_LIST)
def test_gpu_run_lengths(k, seg):
    FC.run_run_lengths(_gpu_factory(), k, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
def test_gpu_offsets(seg):
    FC.run_offsets(_gpu_factory(), 33, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 21])
def test_gpu_soup(k):
    FC.run_soup(_gpu_factory(), k, 16)


@pytest.mark.gpu
def test_gpu_long_runs():
    FC.run_long_runs(_gpu_factory())


@pytest.mark.gpu
def test_gpu_default_segment():
    FC.run_default_segment(_gpu_factory())


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
def test_gpu_every_cut(seg):
    FC.run_every_cut(_gpu_factory(), 47, seg)


@pytest.mark.gpu
def test_gpu_byte_by_byte():
    FC.run_byte_by_byte(_gpu_factory(), 31, 50)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
def test_gpu_fastq_agreement(seg):
    FC.run_fastq_agreement(_gpu_factory(), 47, seg)


@pytest.mark.gpu
def test_gpu_trigger():
    FC.run_trigger(_gpu_factory(), 31, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("qb,mlb,levels", FC.GEOMETRIES)
def test_gpu_geometry(qb, mlb, levels):
    FC.run_geometry(_gpu_factory(), 47, 50, qb, mlb)


@pytest.mark.gpu
def test_gpu_errors():
    FC.run_errors(_gpu_factory(), 47, 50, _gpu_bytes)


@pytest.mark.gpu
def test_gpu_own_output(tmp_path):
    FC.run_own_output(_gpu_factory(), tmp_path)


@pytest.mark.gpu
def test_gpu_large():
    FC.run_large(_gpu_factory())


def _cli_inputs(tmp_path):
    """a .fa.gz made of reads of the golden build 1 (so that most of its k-mers are in that filter) and one foreign record"""
    fq = open(os.path.join(ROOT, "tests", "golden", "reads1.fq"), "rb").read().split(b"\n")
    reads = [r for r in fq[1::4] if r][:40]
    fa = b"".join(b">r%d\n%s" % (i, FC.wrap(r, 60)) for i, r in enumerate(reads)) + b">foreign\n" + FC.wrap(FC.dna(300, 77), 60)
    path = str(tmp_path / "some.fa.gz")
    with gzip.open(path, "wb") as f:
        f.write(fa)
    return path, fa, os.path.join(ROOT, "tests", "golden", "build1.cqf")


def _check_cli(text, fa, cqf, k, smin):
    from shk.fasta import format_report
    O = cqflibs.oracle()
    rd = FC.Reader(k)
    fs = rd.feed(fa)
    q = O.load(cqf)
    from shk.spectrum import cqf_geometry
    qb, hb = cqf_geometry(cqf)
    keys = O.seq_keys(rd.all_runs(), k, hb)
    uniq, cnt = np.unique(keys, return_counts=True)
    have = [q.count(int(x)) for x in uniq]
    q.free()
    against = {"path": cqf, "distinct": len(uniq), "present": sum(1 for h in have if h), "min_count": smin,
               "solid": sum(1 for h in have if h >= smin), "inner_product": sum(int(c) * h for c, h in zip(cnt, have))}
    assert against["present"] > 0
    assert text == format_report(fs, len(uniq), against)


def _run_cli(call, tmp_path):
    import json
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "fastq_builds.json")))["builds"][1]["cfg"]["k"]
    path, fa, cqf = _cli_inputs(tmp_path)
    ocqf = str(tmp_path / "fa.cqf")
    _check_cli(call([path, "-k", str(k), "--against", cqf, "--min-count", "3", "-o", ocqf]), fa, cqf, k, 3)
    assert os.path.getsize(ocqf) == os.path.getsize(cqf)


@pytest.mark.gpu
def test_gpu_cli(tmp_path):
    """the command line itself, as a process of its own"""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "sh-assembly_amd"))

    def call(argv):
        r = subprocess.run([sys.executable, "-m", "shk.fasta"] + argv, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    _run_cli(call, tmp_path)
