"""shk_sample_chunks and python -m shk.estimate (tests/sample_cases.py): every device case once on the CPU emulator build
of the kernel sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu); the host pieces need neither."""
import contextlib
import ctypes as C
import gzip
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cqflibs
import sample_cases as SC
import synth
from test_emu_kernels import EMU, _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


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


@contextlib.contextmanager
def _no_pack():
    """SHK_NO_PACK in the environment of the calls inside (pack_stage reads it call by call)"""
    old = os.environ.get("SHK_NO_PACK")
    os.environ["SHK_NO_PACK"] = "1"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SHK_NO_PACK", None)
        else:
            os.environ["SHK_NO_PACK"] = old


# ---------------------------------------------------------------- host pieces (no device)
def test_binding_mirrors_the_header():
    import shk as m
    hdr = open(os.path.join(ROOT, "include", "shk.h")).read()
    assert "shk_sample_chunks" in m.EXPORTS
    decl = re.search(r"typedef struct shk_sample_stats \{ uint64_t ([a-z, ]+); \} shk_sample_stats;", hdr)
    assert [x.strip() for x in decl.group(1).split(",")] == [n for n, _ in m.SampleStats._fields_]
    assert all(t is C.c_uint64 for _, t in m.SampleStats._fields_)
    proto = re.search(r"int shk_sample_chunks\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == 10
    from shk import estimate
    assert ("sample_bits > %d" % estimate.MAX_SAMPLE_BITS) in hdr and "hb + sample_bits > 56" in hdr
    assert estimate.max_sample_bits(24) == 24 and estimate.max_sample_bits(30) == 18


def test_constants_mirror_the_kernel():
    """the list capacity the flush cases are sized from, and the workgroup sizes the library launches"""
    src = open(os.path.join(ROOT, "sh-assembly_amd", "csrc", "roll_kernels.hip")).read()
    api = open(os.path.join(ROOT, "sh-assembly_amd", "csrc", "shk_api.hip")).read()
    assert int(re.search(r"#define SHK_ROLL_STEPS (\d+)", src).group(1)) == SC.ROLL_STEPS
    assert int(re.search(r"#define SHK_WAVE (\d+)", open(os.path.join(ROOT, "sh-assembly_amd", "csrc", "shk_device.h")).read()).group(1)) == SC.WAVE
    assert "WTILE = SHK_WAVE * SHK_ROLL_STEPS, WKEEP = WTILE / 4;" in src and "list[WAVES][WTILE + WKEEP]" in src
    assert "k_roll_sample<%d, 4>" % SC.GPU_THREADS in api and "k_roll_sample<%d, 4>" % SC.EMU_THREADS in api
    assert SC.LIST_CAPACITY == 1280


def test_format_estimate():
    from shk.estimate import format_estimate, format_flags
    hist, totals, sstats, s, k, fm, want = SC.format_case()
    assert format_estimate(hist, totals, sstats, s, k, fm) == want
    assert format_flags(hist, totals, sstats, s, k, fm) == want.split("suggested: ")[1]
    empty = format_estimate([0, 0], {"distinct": 0, "total": 0, "max_count": 0}, {"kmers": 0, "kept": 0}, 4, 31)
    assert empty == "sampled\t1/2^4\t0\nF1\t0\nF0\t0\nsuggested: (none: empty filter)\n"


def test_default_sample_bits():
    from shk.estimate import default_sample_bits, input_bytes
    # 3 GiB of plain FASTQ into 2^24 slots: 3 * 2^30 <= 2^(24 + s) first at s = 8
    assert default_sample_bits([1 << 31, 1 << 30], "f", 24) == 8
    # the same bytes gzipped count four times: 12 * 2^30 <= 2^(24 + s) first at s = 10
    assert input_bytes([1 << 31, 1 << 30], "g") == 12 << 30
    assert default_sample_bits([1 << 31, 1 << 30], "g", 24) == 10
    # exactly 2^24 bytes fit at s = 0, one byte more needs s = 1
    assert default_sample_bits([1 << 24], "f", 24) == 0
    assert default_sample_bits([(1 << 24) + 1], "f", 24) == 1
    # the cap: hb + s <= 56 leaves s <= 8 at qb = 40, and s <= 24 anywhere
    assert default_sample_bits([1 << 60], "f", 40) == 8
    assert default_sample_bits([1 << 60], "b", 20) == 24


def test_accuracy_of_the_sample_model():
    """case 9, oracle hashes and numpy only: 2^s times the kept distinct k-mers, per abundance class, against the exact
    values of F0, f1 and n = F0 - f1 - f2, within four standard deviations of an independent 2^-s sampling of X distinct
    k-mers plus X / 256 for the keys lost to hb-bit collisions. And the reason for the bit choice: the TOP s bits keep
    far more than their nominal share.
    Measured here, 436164 distinct 31-mers (the test prints the figures): F0 +0.18 %, -0.01 %, +0.84 % at s = 2, 3, 5
    against sigma 0.26 %, 0.40 %, 0.84 %; f1 +0.01 %, +0.25 %, +0.83 % against 0.29 %, 0.44 %, 0.92 %; n -0.28 %, -2.27 %,
    +1.47 % against 0.71 %, 1.08 %, 2.27 %; the top s bits keep 1.75, 1.89 and 1.98 times their nominal share."""
    O = cqflibs.oracle()
    k, hb = 31, 24
    fq = synth.make_fastq(synth.make_genome(60000, 3), 12000, 150, 0.01, seed=5, n_frac=0.02)
    h = np.array(O.chunk_keys(fq, k, 64), dtype=np.uint64)
    assert len(h) > 1_000_000
    uniq, cnt = np.unique(h, return_counts=True)

    def classes(c):
        f0, f1, f2 = len(c), int((c == 1).sum()), int((c == 2).sum())
        return {"F0": f0, "f1": f1, "n": f0 - f1 - f2}

    exact = classes(cnt)
    assert exact["n"] > 10000 and exact["f1"] > 100000
    for s in (2, 3, 5):
        keep = ((h >> np.uint64(hb)) & np.uint64((1 << s) - 1)) == 0
        _, c = np.unique(h[keep] & np.uint64((1 << hb) - 1), return_counts=True)
        est = {key: v << s for key, v in classes(c).items()}
        for key, X in exact.items():
            bound = 4 * np.sqrt(((1 << s) - 1) * X) + X / 256
            print("s=%d %s exact %d estimate %d error %+.3f%% sigma %.3f%%" % (s, key, X, est[key], 100.0 * (est[key] - X) / X,
                                                                               100.0 * np.sqrt(((1 << s) - 1) / X)))
            assert abs(est[key] - X) <= bound, (s, key, est[key], X, bound)
        top = int(((uniq >> np.uint64(64 - s)) == 0).sum())
        print("s=%d top bits keep %.2f times the nominal share" % (s, top * (1 << s) / len(uniq)))
        assert top * (1 << s) > 1.5 * len(uniq)


# ---------------------------------------------------------------- the tool
def _tool_inputs(tmp_path):
    k = json.load(open(os.path.join(GOLDEN, "fastq_builds.json")))["builds"][1]["cfg"]["k"]
    plain = os.path.join(GOLDEN, "reads1.fq")
    path = str(tmp_path / "reads1.fq.gz")
    with gzip.open(path, "wb") as f:
        f.write(open(plain, "rb").read())
    return k, plain, path


def _run_tool(call, tmp_path):
    from shk.estimate import OVERHEAD, format_estimate, format_flags
    k, plain, path = _tool_inputs(tmp_path)
    s, qb, part = 2, 14, 70000      # (a part is at least the chunker's overhead: two parts)
    hist, totals, sstats = SC.oracle_estimate(plain, k, qb, s, part, OVERHEAD, 256)
    argv = [path, "-k", str(k), "-s", str(s), "--qb", str(qb), "--part-size", str(part), "--parts-per-call", "1"]
    assert call(argv) == format_estimate(hist, totals, sstats, s, k)
    flags = call(argv + ["--flags"])
    assert flags == format_flags(hist, totals, sstats, s, k)
    assert re.fullmatch(r"-N \d+ -n \d+ -e 0\.\d{5}\n", flags)
    # the list form
    lst = tmp_path / "files.txt"
    lst.write_text("reads1.fq.gz\n")
    assert call(["-i", str(lst), "-f", "g"] + argv[1:]) == format_estimate(hist, totals, sstats, s, k)


def test_emu_tool(shk, tmp_path):     # noqa: F811
    from shk.estimate import main

    def call(argv):
        out = io.StringIO()
        assert main(argv + ["--lib", EMU], out=out) == 0
        return out.getvalue()
    _run_tool(call, tmp_path)


def test_emu_tool_names_the_way_out_of_a_full_table(shk, tmp_path, capsys):     # noqa: F811
    from shk.estimate import main
    k, plain, path = _tool_inputs(tmp_path)
    assert main([path, "-k", str(k), "-s", "0", "--qb", "14", "--part-size", "70000", "--lib", EMU], out=io.StringIO()) == 1
    err = capsys.readouterr().err
    assert "libshk error -3" in err and "-s" in err and "--qb" in err


@pytest.mark.gpu
def test_gpu_tool(tmp_path):
    """the command line itself, as a process of its own"""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "sh-assembly_amd"))

    def call(argv):
        r = subprocess.run([sys.executable, "-m", "shk.estimate"] + argv, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    _run_tool(call, tmp_path)


# ---------------------------------------------------------------- CPU emulator
@pytest.mark.parametrize("k", SC.K_LIST)
def test_emu_shapes(shk, k):     # noqa: F811
    SC.run_shapes(_emu_factory(shk), k, _no_pack)


def test_emu_anchor(shk):     # noqa: F811
    SC.run_anchor(_emu_factory(shk))


def test_emu_flush_full(shk):     # noqa: F811
    SC.run_flush_full(_emu_factory(shk), SC.EMU_THREADS)


def test_emu_flush_sparse(shk):     # noqa: F811
    SC.run_flush_sparse(_emu_factory(shk))


def test_emu_accumulate(shk):     # noqa: F811
    SC.run_accumulate(_emu_factory(shk))


@pytest.mark.parametrize("qb,mlb,levels", SC.GEOMETRIES)
def test_emu_geometry(shk, qb, mlb, levels):     # noqa: F811
    SC.run_geometry(_emu_factory(shk), qb, mlb)


def test_emu_trigger(shk):     # noqa: F811
    SC.run_trigger(_emu_factory(shk))


def test_emu_errors(shk):     # noqa: F811
    SC.run_errors(_emu_factory(shk), _emu_bytes)


# ---------------------------------------------------------------- gfx950
@pytest.mark.gpu
@pytest.mark.parametrize("k", SC.K_LIST)
def test_gpu_shapes(k):
    SC.run_shapes(_gpu_factory(), k, _no_pack)


@pytest.mark.gpu
def test_gpu_anchor():
    SC.run_anchor(_gpu_factory())


@pytest.mark.gpu
def test_gpu_flush_full():
    SC.run_flush_full(_gpu_factory(), SC.GPU_THREADS)


@pytest.mark.gpu
def test_gpu_flush_sparse():
    SC.run_flush_sparse(_gpu_factory())


@pytest.mark.gpu
def test_gpu_accumulate():
    SC.run_accumulate(_gpu_factory())


@pytest.mark.gpu
@pytest.mark.parametrize("qb,mlb,levels", SC.GEOMETRIES)
def test_gpu_geometry(qb, mlb, levels):
    SC.run_geometry(_gpu_factory(), qb, mlb)


@pytest.mark.gpu
def test_gpu_trigger():
    SC.run_trigger(_gpu_factory())


@pytest.mark.gpu
def test_gpu_errors():
    SC.run_errors(_gpu_factory(), _gpu_bytes)
