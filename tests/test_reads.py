"""shk_query_reads (tests/reads_cases.py): every device case once on the CPU emulator build of the kernel sources
(test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu); the host pieces need neither."""
import gzip
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import query_cases as QC
import reads_cases as RC
from test_emu_kernels import EMU, _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)
from test_fasta import _emu_bytes, _emu_factory, _gpu_bytes, _gpu_factory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LIST = [5, 16, 17, 31, 47, 64, 65, 191]


# ---------------------------------------------------------------- host pieces (no device)
def test_model_on_a_hand_written_text():
    #        0         1         2         3         4         5
    #        0123456789012345678901234567890123456789012345678901234567
    text = b"@a\nACGTN\n+\nIIIII\n@b x\nacgtac\r\n+\r\n@IIIII\r\n@c\nAC\n+\nII\n@d\nACG"
    assert RC.reads_of(text, [0], [len(text)]) == [(3, 5, 0), (22, 7, 0), (44, 2, 0)]      # (@d's line has no line feed)
    assert RC.reads_of(text, [42, 0, 17], [16, 17, 0]) == [(44, 2, 0), (3, 5, 1)]
    assert RC.windows(b"ACGTN", 3) == [b"ACG", b"CGT", None]
    assert RC.windows(b"acgtac\r", 3) == [b"acg", b"cgt", b"gta", b"tac", None]
    assert RC.windows(b"AC", 3) == [] and RC.windows(b"A.CGT-", 2) == [None, None, b"CG", b"GT", None]
    keys = [int(x) for x in RC.all_keys(text, [0], [len(text)], 3, 20)]
    assert len(keys) == 6 and keys[0] == keys[2] and keys[1] == keys[3]      # ACG = acg; CGT = cgt (and = ACG reversed: canonical)
    table = {keys[0]: 5, keys[4]: 1}      # ACG (= CGT, its reverse complement): 5; GTA (= TAC): 1
    assert keys[0] == keys[1] and keys[4] == keys[5]
    rs, rec, ext, track = RC.expect(text, [0], [len(text)], 3, 20, table, 2, True)
    assert rs == {"reads": 3, "kmers": 6, "present": 6, "solid": 4, "sum": 22}
    #              sum kmers present solid min median max
    assert rec == [(10, 2, 2, 2, 5, 5, 5), (12, 4, 4, 2, 1, 1, 5), (0, 0, 0, 0, 0, 0, 0)]
    assert ext == [(3, 5, 0), (22, 7, 0), (44, 2, 0)]
    assert track.tolist() == [5, 5, RC.NONE, 5, 5, 1, 1, RC.NONE]
    assert RC.expect(text, [0], [len(text)], 3, 20, table, 2, False)[1][1] == (12, 4, 4, 2, 1, RC.NONE, 5)


def test_binding_mirrors_the_header():
    import ctypes as C
    import shk as m
    hdr = open(os.path.join(ROOT, "include", "shk.h")).read()
    assert int(re.search(r"#define SHK_READS_MEDIAN (\d+)u", hdr).group(1)) == m.READS_MEDIAN == 1
    assert "shk_query_reads" in m.EXPORTS and re.search(r"\nint shk_query_reads\(shk_ctx \*ctx,", hdr)
    decl = re.search(r"typedef struct shk_read_record \{ uint64_t sum; uint32_t ([a-z, ]+); \} shk_read_record;", hdr)
    assert [f for f, _ in m.ReadRecord._fields_] == ["sum"] + decl.group(1).split(", ") == list(RC.REC_FIELDS)
    decl = re.search(r"typedef struct shk_read_extent \{ uint64_t seq_off; uint32_t ([a-z_, ]+); \} shk_read_extent;", hdr)
    assert [f for f, _ in m.ReadExtent._fields_] == ["seq_off"] + decl.group(1).split(", ")
    decl = re.search(r"typedef struct shk_reads_stats \{ uint64_t ([a-z, ]+); \} shk_reads_stats;", hdr)
    assert [f for f, _ in m.ReadsStats._fields_] == decl.group(1).split(", ")
    assert (C.sizeof(m.ReadRecord), C.sizeof(m.ReadExtent)) == (32, 16)
    assert (m._struct_dtype(m.ReadRecord).itemsize, m._struct_dtype(m.ReadExtent).itemsize) == (32, 16)


def _records(rows_):
    import shk as m
    a = np.zeros(len(rows_), dtype=m._struct_dtype(m.ReadRecord))
    for j, f in enumerate(("kmers", "present", "solid", "median")):
        a[f] = [r[j] for r in rows_]
    return a


def test_selection_rules():
    from shk.reads import select
    #               kmers present solid median
    rec = _records([(10, 10, 5, 3), (10, 9, 4, 2), (10, 3, 3, 0), (0, 0, 0, 0), (2, 2, 2, 900), (3, 1, 1, 0), (10, 1, 0, 0)])
    none = dict(min_solid=None, max_solid=None, min_present=None, max_present=None, min_median=None, max_median=None)
    # no rule: everything that has a k-mer; a read without k-mers passes no rule, --keep-short keeps it
    assert select(rec, **none).tolist() == [True, True, True, False, True, True, True]
    assert select(rec, keep_short=True, **none).tolist() == [True] * 7
    # --min-kmers: reads below it are short too
    assert select(rec, min_kmers=3, **none).tolist() == [True, True, True, False, False, True, True]
    assert select(rec, min_kmers=4, keep_short=True, **dict(none, min_solid=0.45)).tolist() == [True, False, False, True, True, True, False]
    # fractions exactly at a threshold pass, on either side
    assert select(rec, **dict(none, min_solid=0.5)).tolist() == [True, False, False, False, True, False, False]
    assert select(rec, **dict(none, max_solid=0.5)).tolist() == [True, True, True, False, False, True, True]
    assert select(rec, **dict(none, min_present=0.3, max_present=0.9)).tolist() == [False, True, True, False, False, True, False]
    assert select(rec, **dict(none, max_present=0.1)).tolist() == [False, False, False, False, False, False, True]
    assert select(rec, **dict(none, min_present=1 / 3)).tolist() == [True, True, False, False, True, True, False]
    # the median's bounds are inclusive; every rule given must pass
    assert select(rec, **dict(none, min_median=2, max_median=3)).tolist() == [True, True, False, False, False, False, False]
    assert select(rec, **dict(none, min_median=2, min_solid=0.5)).tolist() == [True, False, False, False, True, False, False]
    assert select(rec, **dict(none, max_median=0)).tolist() == [False, False, True, False, False, True, True]
    assert select(rec[:0], **none).tolist() == []


def test_report_format():
    from shk.reads import format_report
    stats, rules, want = RC.report_case()
    assert format_report(stats, 250, 31, 3, "host.cqf", rules, min_kmers=10, keep_short=True) == want
    empty = dict(stats, reads=0, kmers=0, present=0, solid=0, sum=0)
    text = format_report(empty, 0, 31, 3, "host.cqf", dict.fromkeys(rules))
    assert "kept\t0\t0.00%\n" in text and "present\t0\t0.00%\n" in text and text.endswith("rules\tmin-kmers=1\n")


def test_record_bounds_and_byte_mask():
    import shk as m
    from shk.reads import byte_mask, names_of, record_bounds
    recs = [b"@a 1\nACGT\n+\nIIII\n", b"@b\tx\r\nAC\r\n+\r\n@I\r\n", b"@c\n\n+\n\n", b"@d\nA\n+\n@"]
    text = b"".join(recs)
    offs, lens = [0, len(recs[0])], [len(recs[0]), len(text) - len(recs[0])]
    ext = np.zeros(4, dtype=m._struct_dtype(m.ReadExtent))
    for i, (o, n, c) in enumerate(RC.reads_of(text, offs, lens)):
        ext[i] = (o, n, c)
    buf = np.frombuffer(text, dtype=np.uint8)
    starts, ends = record_bounds(buf, ext, offs, lens)
    assert [text[a:b] for a, b in zip(starts.tolist(), ends.tolist())] == recs
    keep = np.array([True, False, True, False])
    mk = byte_mask(len(buf), starts[keep], ends[keep])
    assert buf[mk].tobytes() == recs[0] + recs[2] and buf[~mk].tobytes() == recs[1] + recs[3]
    assert names_of(buf, starts) == ["a", "b", "c", "d"]


# ---------------------------------------------------------------- the device cases
def _cases(mk, dev_bytes, many):
    return {
        "sources": lambda: RC.run_sources(mk),
        "chunks": lambda: RC.run_chunks(mk, dev_bytes),
        "hard_table": lambda: RC.run_hard_table(mk),
        "median": lambda: RC.run_median(mk),
        "longest": lambda: RC.run_longest(mk),
        "many": lambda: RC.run_many(mk, many),
        "against_fasta": lambda: RC.run_against_fasta(mk),
        "against_counting": lambda: RC.run_against_counting(mk),
        "reader_contract": lambda: RC.run_reader_contract(mk),
    }


CASES = sorted(_cases(None, None, 0))


@pytest.mark.parametrize("k", K_LIST)
def test_emu_shapes(shk, k):     # noqa: F811
    RC.run_shapes(_emu_factory(shk), k)


@pytest.mark.parametrize("case", CASES)
def test_emu_case(shk, case):     # noqa: F811
    _cases(_emu_factory(shk), _emu_bytes, 3001)[case]()


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_LIST)
def test_gpu_shapes(k):
    RC.run_shapes(_gpu_factory(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_case(case):
    _cases(_gpu_factory(), _gpu_bytes, 70001)[case]()


# ---------------------------------------------------------------- command line
def _run_cli(mk, call, tmp_path):
    """a small .cqf built here from a genome, a gzip file of 800 reads (three parts, two calls) of which a third come from it: the kept and the
    rejected records byte for byte, the table, the mask and the report against the model's"""
    fq, fa, k, qb = RC.cli_case()
    ctx = QC.ctx_for(mk, qb, k, None)
    ctx.count_fasta(fa)
    cqf = str(tmp_path / "own.cqf")
    ctx.export_cqf(cqf)
    ctx.close()
    path = str(tmp_path / "reads.fq.gz")
    with gzip.open(path, "wb") as f:
        f.write(fq)
    out = {name: str(tmp_path / name) for name in ("kept.fq", "rest.fq", "table.tsv", "mask.u8")}
    rules = {"min_solid": None, "max_solid": None, "min_present": 0.5, "max_present": None, "min_median": 1, "max_median": None}
    want = RC.cli_expected(fq, fa, k, qb, 1, rules, 5, False, cqf)
    text = call([path, "-k", str(k), "--against", cqf, "--min-count", "1", "--min-present", "0.5", "--min-median", "1", "--min-kmers", "5",
                 "-o", out["kept.fq"], "--rejected", out["rest.fq"], "--table", out["table.tsv"], "--mask", out["mask.u8"],
                 "--parts-per-call", "2", "--part-size", "66000"])
    assert text == want[0]
    got = [open(out["kept.fq"], "rb").read(), open(out["rest.fq"], "rb").read(), open(out["table.tsv"]).read()]
    assert got[0] == want[1] and got[1] == want[2] and got[2] == want[3]
    mask = np.fromfile(out["mask.u8"], dtype=np.uint8)
    assert np.array_equal(mask, want[4]) and len(mask) // 6 < int(mask.sum()) < len(mask) // 2
    assert len(got[0]) + len(got[1]) == len(fq) and b"\r\n" in got[0] + got[1]
    # --keep-short and no rule at all: every read is kept, the rejected file is empty
    text = call([path, "-k", str(k), "--against", cqf, "--keep-short", "-o", out["kept.fq"], "--rejected", out["rest.fq"],
                 "--part-size", "66000"])
    assert open(out["kept.fq"], "rb").read() == fq and open(out["rest.fq"], "rb").read() == b""
    assert text == RC.cli_expected(fq, fa, k, qb, 2, dict.fromkeys(rules), 0, True, cqf)[0]


def test_emu_cli(shk, tmp_path):     # noqa: F811
    from shk.reads import main

    def call(argv):
        out = io.StringIO()
        assert main(argv + ["--lib", EMU], out=out) == 0
        return out.getvalue()
    _run_cli(_emu_factory(shk), call, tmp_path)


@pytest.mark.gpu
def test_gpu_cli(tmp_path):
    """the command line itself, as a process of its own"""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "sh-assembly_amd"))

    def call(argv):
        r = subprocess.run([sys.executable, "-m", "shk.reads"] + argv, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    _run_cli(_gpu_factory(), call, tmp_path)
