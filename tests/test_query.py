"""shk_query_fasta (tests/query_cases.py): every case once on the CPU emulator build of the kernel sources (test_emu_*)
and once on the gfx950 library (test_gpu_*, -m gpu); the host pieces need neither. Most cases lower SHK_FASTA_SEGMENT to
50 (unaligned) and 64 (a whole unit), so that texts of a few hundred bytes cross segment and unit boundaries."""
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fasta_cases as FC
import query_cases as QC
from test_emu_kernels import EMU, _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)
from test_fasta import CUTS, SEGS, _emu_bytes, _emu_factory, _gpu_bytes, _gpu_factory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emu_u32(n):
    a = np.zeros(n + 16, dtype=np.uint32)
    at = (-a.ctypes.data) % 64 // 4
    return a.ctypes.data + 4 * at, lambda: a[at:at + n]


def _gpu_u32(n):
    import torch
    t = torch.zeros(n, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t.data_ptr(), lambda: t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- host pieces (no device)
def test_model_is_the_grammar_with_ordinals_and_records():
    m = QC.Model(3)
    st, ends, recs = m.feed(b"AC\nGT\r\n>ACGT\nacN-gt>a\n;x\n\nTTT")
    assert st == {"records": 2, "bases": 12, "breaks": 3, "kmers": 3}
    assert ends == [None, None, b"ACG", b"CGT", None, None, None, None, None, None, None, b"TTT"]
    assert recs == [0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2]
    # the state goes over feed() calls: a run, a header and a line start cut anywhere
    m, got = QC.Model(3), []
    for piece in (b"A", b"C\nG", b"T\n>h", b"dr\nAC", b"G"):
        got += m.feed(piece)[1]
    assert got == [None, None, b"ACG", b"CGT", None, None, b"ACG"]


def test_qv_formula():
    from shk.query import qv
    assert qv(900, 900, 31) == math.inf
    assert qv(0, 900, 31) == 0
    assert math.isnan(qv(0, 0, 31))
    # one wrong base in a thousand: 1 - p = 1e-3, QV 30
    k = 21
    assert abs(qv(round(1e6 * (1 - 1e-3) ** k), 10 ** 6, k) - 30.0) < 0.01


def test_report_format():
    from shk.query import format_report
    qs, rows, want, want_rows = QC.report_case()
    assert format_report(qs, 31, 3, "reads.cqf") == want
    assert format_report(qs, 31, 3, "reads.cqf", rows) == want + want_rows
    empty = dict(qs, kmers=0, present=0, solid=0, sum=0)
    assert "present\t0\t0.00%" in format_report(empty, 31, 3, "reads.cqf") and "QV\tnan" in format_report(empty, 31, 3, "reads.cqf")


def test_names_across_piece_cuts():
    from shk.query import Names
    text = b"ACGT\n>one first\n>two\tsecond\r\nAC>GT\n;three\nAC\r>no\n>\n>five" + b"\n>>six six\nACGT"
    want = ["one", "two", "three", "", "five", ">six"]
    assert Names().feed(text).names == want
    assert len(want) == QC.Model(1).feed(text)[0]["records"]
    for c in range(len(text) + 1):
        assert Names().feed(text[:c]).feed(text[c:]).names == want, c
    n = Names()
    for i in range(len(text)):
        n.feed(text[i:i + 1])
    assert n.names == want


def test_binding_mirrors_the_header():
    import shk as m
    hdr = open(os.path.join(ROOT, "include", "shk.h")).read()
    assert int(re.search(r"#define SHK_QUERY_NONE (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == m.QUERY_NONE == QC.NONE
    assert "shk_query_fasta" in m.EXPORTS
    decl = re.search(r"typedef struct shk_query_stats\s+\{ uint64_t ([a-z, ]+); \} shk_query_stats;", hdr)
    assert [f for f, _ in m.QueryStats._fields_] == decl.group(1).split(", ")
    decl = re.search(r"typedef struct shk_query_record \{ uint64_t ([a-z, ]+); \} shk_query_record;", hdr)
    assert decl.group(1).split(", ") == ["kmers", "present", "solid", "sum"]


# ---------------------------------------------------------------- CPU emulator
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", [5, 47])
def test_emu_grammar(shk, k, seg):     # noqa: F811
    QC.run_grammar(_emu_factory(shk), k, seg)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", FC.K_LIST)
def test_emu_run_lengths(shk, k, seg):     # noqa: F811
    QC.run_run_lengths(_emu_factory(shk), k, seg)


def test_emu_hard_table(shk):     # noqa: F811
    QC.run_hard_table(_emu_factory(shk))


def test_emu_every_cut(shk):     # noqa: F811
    QC.run_pieces(_emu_factory(shk), 31, 50, QC.every_cut(31))


@pytest.mark.parametrize("seg", SEGS)
def test_emu_chosen_cuts(shk, seg):     # noqa: F811
    QC.run_pieces(_emu_factory(shk), 47, seg, QC.chosen_cuts(47, seg, CUTS))


def test_emu_reader_contract(shk):     # noqa: F811
    QC.run_reader_contract(_emu_factory(shk))


def test_emu_independent_streams(shk):     # noqa: F811
    QC.run_independent_streams(_emu_factory(shk))


def test_emu_without_track(shk):     # noqa: F811
    QC.run_without_track(_emu_factory(shk))


def test_emu_device_track(shk):     # noqa: F811
    QC.run_device_track(_emu_factory(shk), _emu_u32)


def test_emu_errors(shk):     # noqa: F811
    QC.run_errors(_emu_factory(shk), _emu_bytes)


def test_emu_default_segment(shk):     # noqa: F811
    QC.run_default_segment(_emu_factory(shk))


def test_emu_cli(shk, tmp_path):     # noqa: F811
    from shk.query import main

    def call(argv):
        out = io.StringIO()
        assert main(argv + ["--lib", EMU], out=out) == 0
        return out.getvalue()
    _run_cli(_emu_factory(shk), call, tmp_path)


# ---------------------------------------------------------------- gfx950
@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", [5, 47])
def test_gpu_grammar(k, seg):
    QC.run_grammar(_gpu_factory(), k, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("k", FC.K_LIST)
def test_gpu_run_lengths(k, seg):
    QC.run_run_lengths(_gpu_factory(), k, seg)


@pytest.mark.gpu
def test_gpu_hard_table():
    QC.run_hard_table(_gpu_factory())


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
def test_gpu_chosen_cuts(seg):
    QC.run_pieces(_gpu_factory(), 47, seg, QC.chosen_cuts(47, seg, CUTS))


@pytest.mark.gpu
def test_gpu_reader_contract():
    QC.run_reader_contract(_gpu_factory())


@pytest.mark.gpu
def test_gpu_independent_streams():
    QC.run_independent_streams(_gpu_factory())


@pytest.mark.gpu
def test_gpu_without_track():
    QC.run_without_track(_gpu_factory())


@pytest.mark.gpu
def test_gpu_device_track():
    QC.run_device_track(_gpu_factory(), _gpu_u32)


@pytest.mark.gpu
def test_gpu_errors():
    QC.run_errors(_gpu_factory(), _gpu_bytes)


@pytest.mark.gpu
def test_gpu_default_segment():
    QC.run_default_segment(_gpu_factory())


def _run_cli(mk, call, tmp_path):
    """a small .cqf built here, a file of three records cut into pieces of 100 bytes: the report with its record lines and
    the track against the model's"""
    reads, fa, k, qb = QC.cli_case()
    ctx = QC.ctx_for(mk, qb, k, None)
    ctx.count_fasta(reads)
    cqf = str(tmp_path / "reads.cqf")
    ctx.export_cqf(cqf)
    ctx.close()
    path, tpath = str(tmp_path / "three.fa"), str(tmp_path / "three.u32")
    with open(path, "wb") as f:
        f.write(fa)
    want_text, want_track = QC.cli_expected(fa, reads, k, qb, 3, cqf)
    text = call([path, "-k", str(k), "--against", cqf, "--min-count", "3", "--records", "--track", tpath, "--piece", "100"])
    assert text == want_text
    assert np.array_equal(np.fromfile(tpath, dtype="<u4"), want_track)
    assert "contig_1\t" in text and int((want_track != QC.NONE).sum()) > 0 and int((want_track == 0).sum()) > 0


@pytest.mark.gpu
def test_gpu_cli(tmp_path):
    """the command line itself, as a process of its own"""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "sh-assembly_amd"))

    def call(argv):
        r = subprocess.run([sys.executable, "-m", "shk.query"] + argv, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    _run_cli(_gpu_factory(), call, tmp_path)
