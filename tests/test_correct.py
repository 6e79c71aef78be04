"""shk_correct_reads (tests/correct_cases.py): every device case once on the CPU emulator build of the kernel sources
(test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu); the rule's model and the host pieces need neither."""
import gzip
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import correct_cases as CC
import query_cases as QC
import reads_cases as RC
from test_emu_kernels import EMU, _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)
from test_fasta import _emu_bytes, _emu_factory, _gpu_bytes, _gpu_factory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LIST = [5, 21, 32, 33, 47, 64, 65, 191]


# ---------------------------------------------------------------- the rule and the host pieces (no device)
def test_model_on_a_hand_written_text():
    k = 4
    #      0         1
    #      01234567890123
    g = b"ACGGTCATTGCAAGC"
    solid_of = CC.solid_by_strings(set(CC.canonical_kmers(g, k)), k)
    assert solid_of(g) == [True] * 12 and solid_of(b"ACGGTCTTTG") == [True, True, True, False, False, False, False]
    # no error, an error in the middle (windows 3 .. 6 hold it; the forward pass meets it at window 3), at the last base
    # (window 11 alone, check shrinks to 0), at the first base (the backward pass alone meets it)
    assert CC.correct(g, solid_of, k) == ((0, 0, 0, 0), [])
    assert CC.correct(b"ACGGTCTTTGCAAGC", solid_of, k, check=2) == ((1, 0, 0, 0), [(6, 0)])
    assert CC.correct(b"ACGGTCATTGCAAGA", solid_of, k) == ((1, 0, 0, 0), [(14, 1)])
    assert CC.correct(b"TCGGTCATTGCAAGC", solid_of, k) == ((1, 0, 0, 0), [(0, 0)])
    # the reverse strand of the read with the error in the middle: the same base, in the read's own strand
    assert CC.correct(CC.revcomp(b"ACGGTCTTTGCAAGC"), solid_of, k, check=2) == ((1, 0, 0, 0), [(8, 3)])
    # lower case is read as upper case; the edits carry codes, the case is apply_edits' business
    assert CC.correct(b"acggtctttgcaagc", solid_of, k, check=2) == ((1, 0, 0, 0), [(6, 0)])
    assert CC.corrected(b"acggtcTttgcaagc", [(6, 0)]) == b"acggtcAttgcaagc" and CC.corrected(b"acggtctttg", [(6, 0)]) == b"acggtcattg"
    # two errors: the first (6) is repaired by the forward pass, the second (11) then by the forward pass too; with one
    # edit allowed the second is met with the budget used up (by the forward pass: it lies in the backward pass' head)
    assert CC.correct(b"ACGGTCTTTGCTAGC", solid_of, k, check=1) == ((2, 0, 0, 0), [(6, 0), (11, 0)])
    assert CC.correct(b"ACGGTCTTTGCTAGC", solid_of, k, check=1, max_edits=1) == ((1, 0, 0, CC.CAPPED), [(6, 0)])
    # ... and with check = 5 the windows behind the first suspect reach the second error: nothing can be repaired from the
    # left, and the backward pass repairs the second error first, then the first one
    assert CC.correct(b"ACGGTCTTTGCTAGC", solid_of, k, check=5) == ((2, 1, 0, 0), [(11, 0), (6, 0)])
    # reads that are left alone
    assert CC.correct(b"ACG", solid_of, k) == ((0, 0, 0, CC.SHORT), []) and CC.correct(b"", solid_of, k) == ((0, 0, 0, CC.SHORT), [])
    assert CC.correct(b"AN", solid_of, k) == ((0, 0, 0, CC.SHORT), [])
    for s in (b"ACGGTCNTTGC", b"ACGGTCnTTGC", b"ACGGTCRTTGC", b"ACGGTCATTGC\r"):
        assert CC.correct(s, solid_of, k) == ((0, 0, 0, CC.NONBASE), [])
    # ambiguous: both other bases at the suspect are solid
    more = CC.solid_by_strings(set(CC.canonical_kmers(g, k)) | set(CC.canonical_kmers(b"GTCGTTG", k)), k)
    assert CC.correct(b"ACGGTCTTTGCAAGC", more, k, check=3)[0] == (0, 0, 2, 0)      # (met from both sides)


@pytest.mark.parametrize("k,genome,length,nreads", [(21, 20000, 100, 30), (15, 3000, 40, 30)])
def test_single_error_property(k, genome, length, nreads):
    """len >= 2k: a read with one substitution, at whatever position and of whichever strand, comes back to the original
    with exactly one edit (the forward pass meets position p when p >= k - 1, the backward pass when p <= len - k)"""
    assert length >= 2 * k
    solid_of, of = None, None
    n = 0
    for g, s, bad, p in CC.single_error_cases(k, genome, length, nreads, 7 * k):
        if of is not g:
            solid_of, of = CC.solid_by_strings(set(CC.canonical_kmers(g, k)), k), g
        rec, edits = CC.correct(bad, solid_of, k)
        assert rec == (1, 0, 0, 0) and CC.corrected(bad, edits) == s and edits[0][0] == p, (p, rec, edits)
        n += 1
    assert n == nreads * length


def _arrays(ext_rows, rec_rows, edit_rows, width=4):
    import shk as m
    ext = np.zeros(len(ext_rows), dtype=m._struct_dtype(m.ReadExtent))
    rec = np.zeros(len(rec_rows), dtype=m._struct_dtype(m.CorrectRecord))
    edits = np.full((len(rec_rows), width), 0xFFFFFFFF, dtype=np.uint32)      # (entries behind rec.edits are unspecified)
    for i, (e, r, ed) in enumerate(zip(ext_rows, rec_rows, edit_rows)):
        ext[i] = e
        rec[i] = r
        edits[i, :len(ed)] = [p | c << 16 for p, c in ed]
    return ext, rec, edits


def test_apply_edits():
    from shk.correct import apply_edits, edit_list
    for eol in (b"\n", b"\r\n"):
        text = RC.fastq([b"ACGTACGT", b"acgtacgt", b"AcGtNNAC", b"", b"TTTT"], eol=eol)
        reads = RC.reads_of(text, [0], [len(text)])
        strip = len(eol) - 1      # (the '\r' belongs to the sequence line the front end reports)
        assert [text[o:o + n - strip] for o, n, _ in reads] == [b"ACGTACGT", b"acgtacgt", b"AcGtNNAC", b"", b"TTTT"]
        #         upper case; lower case kept; mixed, and a position twice (the later entry wins); none; first and last base
        plan = [[(0, 3), (7, 0)], [(2, 0)], [(1, 2), (3, 0), (1, 3)], [], [(0, 1), (3, 2)]]
        ext, rec, edits = _arrays(reads, [(len(e), 0, 0, 0) for e in plan], plan)
        got = apply_edits(text, ext, rec, edits)
        want = RC.fastq([b"TCGTACGA", b"acatacgt", b"AtGaNNAC", b"", b"CTTG"], eol=eol)
        assert isinstance(got, bytes) and got == want
        # only bytes of sequence lines have changed
        diff = [i for i in range(len(text)) if text[i] != got[i]]
        assert diff and all(any(o <= i < o + n for o, n, _ in reads) for i in diff)
        r, pos, at, old, new = edit_list(text, ext, rec, edits)
        assert r.tolist() == [0, 0, 1, 2, 2, 2, 4, 4] and pos.tolist() == [0, 7, 2, 1, 3, 1, 0, 3]
        assert bytes(old.tolist()) == b"ATgctgTT" and bytes(new.tolist()) == b"TAagatCG"
        # rec.edits = 0 everywhere: the text itself, whatever the edit array holds
        assert apply_edits(text, ext, np.zeros_like(rec), edits) == text
    none = _arrays([], [], [])
    assert apply_edits(b"@r\n", *none) == b"@r\n" and apply_edits(b"", *none) == b""


def test_report_format():
    from shk.correct import format_report
    stats = {"reads": 1000, "candidates": 900, "edited_reads": 90, "edits": 120, "unfixable": 7, "ambiguous": 3, "capped": 1}
    want = ("reads\t1000\ncandidates\t900\t90.00%\nedited reads\t90\t10.00%\nedits\t120\nunfixable\t7\nambiguous\t3\ncapped\t1\n"
            "against\town.cqf\nparameters\tk=31 min-count=2 check=4 max-edits=8\n")
    assert format_report(stats, 31, 2, 4, 8, "own.cqf") == want
    text = format_report(dict.fromkeys(stats, 0), 21, 3, 0, 1, "x.cqf")
    assert "candidates\t0\t0.00%\n" in text and "edited reads\t0\t0.00%\n" in text and text.endswith("k=21 min-count=3 check=0 max-edits=1\n")


def test_binding_mirrors_the_header():
    import ctypes as C
    import shk as m
    hdr = open(os.path.join(ROOT, "include", "shk.h")).read()
    for name, bit in (("SHORT", 1), ("NONBASE", 2), ("CAPPED", 4)):
        assert int(re.search(r"#define SHK_CORRECT_%s +(\d+)u" % name, hdr).group(1)) == getattr(m, "CORRECT_" + name) == getattr(CC, name) == bit
    assert "shk_correct_reads" in m.EXPORTS and re.search(r"\nint shk_correct_reads\(shk_ctx \*ctx,", hdr)
    decl = re.search(r"typedef struct shk_correct_record \{ uint32_t ([a-z, ]+); \} shk_correct_record;", hdr)
    assert [f for f, _ in m.CorrectRecord._fields_] == decl.group(1).split(", ") == list(CC.REC_FIELDS)
    decl = re.search(r"typedef struct shk_correct_stats \{ uint64_t ([a-z_, ]+); \} shk_correct_stats;", hdr)
    assert [f for f, _ in m.CorrectStats._fields_] == decl.group(1).split(", ") == list(CC.STAT_FIELDS)
    assert (C.sizeof(m.CorrectRecord), C.sizeof(m.CorrectStats), m._struct_dtype(m.CorrectRecord).itemsize) == (16, 56, 16)


# ---------------------------------------------------------------- the device cases
def _cases(mk, dev_bytes):
    return {
        "constructed": lambda: CC.run_constructed(mk),
        "batch": lambda: CC.run_batch(mk, dev_bytes),
        "reader_contract": lambda: CC.run_reader_contract(mk, dev_bytes),
        "errors": lambda: CC.run_errors(mk, dev_bytes),
    }


CASES = sorted(_cases(None, None))


@pytest.mark.parametrize("k", K_LIST)
def test_emu_shapes(shk, k):     # noqa: F811
    CC.run_shapes(_emu_factory(shk), k)


@pytest.mark.parametrize("case", CASES)
def test_emu_case(shk, case):     # noqa: F811
    _cases(_emu_factory(shk), _emu_bytes)[case]()


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_LIST)
def test_gpu_shapes(k):
    CC.run_shapes(_gpu_factory(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_case(case):
    _cases(_gpu_factory(), _gpu_bytes)[case]()


# ---------------------------------------------------------------- command line
def _run_cli(mk, call, tmp_path):
    """a small .cqf built here from a genome; a gzip file of 800 reads in three parts and two calls, then a list of two
    plain files: the corrected text, the table, the edit log and the report against the model's"""
    fq1, fq2, fa, k, qb = CC.cli_case()
    ctx = QC.ctx_for(mk, qb, k, None)
    ctx.count_fasta(fa)
    cqf = str(tmp_path / "own.cqf")
    ctx.export_cqf(cqf)
    ctx.close()
    path = str(tmp_path / "reads.fq.gz")
    with gzip.open(path, "wb") as f:
        f.write(fq1)
    out = {name: str(tmp_path / name) for name in ("fixed.fq", "table.tsv", "edits.tsv")}
    want = CC.cli_expected(fq1, fa, k, qb, 2, 3, 4, cqf)
    text = call([path, "-k", str(k), "--against", cqf, "--check", "3", "--max-edits", "4", "-o", out["fixed.fq"], "--table", out["table.tsv"],
                 "--edits", out["edits.tsv"], "--parts-per-call", "2", "--part-size", "66000"])
    assert text == want[0] and len(fq1) > 2 * 66000
    fixed = open(out["fixed.fq"], "rb").read()
    assert fixed == want[1] and fixed != fq1 and len(fixed) == len(fq1) and b"\r\n" in fixed
    # ... which differs from the input only inside sequence lines
    a, b = fq1.split(b"\n"), fixed.split(b"\n")
    assert len(a) == len(b) and all(x == y for i, (x, y) in enumerate(zip(a, b)) if i % 4 != 1)
    assert open(out["table.tsv"]).read() == want[2] and open(out["edits.tsv"]).read() == want[3] and want[3].count("\n") > 50
    # a list of two plain files, defaults: the chunker's order is the list's
    for name, body in (("a.fq", fq1), ("b.fq", fq2)):
        with open(str(tmp_path / name), "wb") as f:
            f.write(body)
    with open(str(tmp_path / "list.txt"), "w") as f:
        f.write("a.fq\nb.fq\n")
    # (the chunker goes round the files part by part, host/fastq_chunker.cpp: the text the model reads is what it hands out)
    from shk.reads import parts_of
    paths = [str(tmp_path / "a.fq"), str(tmp_path / "b.fq")]
    handed = b"".join(t for t, _, _ in parts_of(paths, "f", 1, 66000))
    assert len(handed) == len(fq1) + len(fq2) and handed != fq1 + fq2 and handed.startswith(fq1[:1000])
    want = CC.cli_expected(handed, fa, k, qb, 2, 4, 8, cqf)
    text = call(["-i", str(tmp_path / "list.txt"), "-f", "f", "-k", str(k), "--against", cqf, "-o", out["fixed.fq"], "--part-size", "66000"])
    assert text == want[0] and open(out["fixed.fq"], "rb").read() == want[1]


def test_emu_cli(shk, tmp_path):     # noqa: F811
    from shk.correct import main

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
        r = subprocess.run([sys.executable, "-m", "shk.correct"] + argv, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    _run_cli(_gpu_factory(), call, tmp_path)
