"""Filter analytics on the device (tests/analytics_cases.py): every case once on the CPU emulator build of the kernel
sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu); the host pieces need neither."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import analytics_cases as AC
import cqflibs
from test_emu_kernels import EMU, _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [AC.p_plain, AC.p_wrap, AC.p_tail]
CHECKERS = ["definition", "reference"]


def _emu_factory(shk):     # noqa: F811
    def mk(**kw):
        ctx = _emu_ctx(shk, **kw)

        def dev_u64(vals):      # -> (pointer the library can write, reader of the words)
            arr = (C.c_uint64 * len(vals))(*vals)
            return C.addressof(arr), lambda: list(arr)
        ctx.dev_u64 = dev_u64
        return ctx
    return mk


def _gpu_factory():
    import torch
    import shk as gshk

    def mk(**kw):
        ctx = gshk.Context(**kw)

        def dev_u64(vals):
            t = torch.tensor(vals, dtype=torch.int64).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            return t.data_ptr(), lambda: [x & ((1 << 64) - 1) for x in t.cpu().tolist()]
        ctx.dev_u64 = dev_u64
        return ctx
    return mk


def _ref(checker):
    if checker == "reference" and not cqflibs.have_ref():
        pytest.skip("needs oracle/_ref")
    return checker == "reference"


def _name(f):
    return f.__name__[2:]


# ---------------------------------------------------------------- host pieces (no device)
def test_params_from_spectrum_readme_figures():
    """the reference README's own example (README.md:78-93)"""
    from shk.plan import params_from_spectrum
    N, n, e = params_from_spectrum(1810841770, 16506371070, [1665561610, 26122317, 6172811], 47)
    assert N == 16506371070
    assert n == 119157843
    assert round(e, 5) == 0.00234
    # singletons only as false k-mers (README.md:94)
    N, n, e = params_from_spectrum(1810841770, 16506371070, [1665561610, 26122317, 6172811], 47, false_max=1)
    assert (N, n) == (16506371070, 1810841770 - 1665561610)
    assert e == 1 - ((16506371070 - 1665561610) / 16506371070) ** (1 / 47)
    with pytest.raises(ValueError):
        params_from_spectrum(5, 9, [1], 21)         # f2 is not in the histogram
    with pytest.raises(ValueError):
        params_from_spectrum(0, 0, [0, 0], 21)


def test_report_format():
    """F1, F0, the non-zero bins in the layout of the README's ntCard excerpt, then the suggestion"""
    from shk.spectrum import format_report
    hist = [5, 0, 2, 1]          # five singletons, two k-mers seen three times, one seen >= 4 times (9 times)
    totals = {"distinct": 8, "total": 5 + 6 + 9, "sumsq": 5 + 18 + 81, "max_count": 9}
    e = 1 - (15 / 20) ** (1 / 21)
    assert format_report(hist, totals, 21) == "F1\t20\nF0\t8\nf1\t5\nf3\t2\nf>=4\t1\nsuggested: -N 20 -n 3 -e %.5f\n" % e
    totals["max_count"] = 4      # the last bin holds exactly its own count: no ">="
    assert format_report(hist, totals, 21).splitlines()[4] == "f4\t1"
    assert format_report([0, 0], {"distinct": 0, "total": 0, "sumsq": 0, "max_count": 0}, 21) == "F1\t0\nF0\t0\nsuggested: (none: empty filter)\n"


# ---------------------------------------------------------------- CPU emulator
@pytest.mark.parametrize("table", AC.TABLES, ids=_name)
def test_emu_spectrum(shk, table):     # noqa: F811
    AC.run_spectrum(_emu_factory(shk), table)


def test_emu_spectrum_device(shk):     # noqa: F811
    AC.run_spectrum_device(_emu_factory(shk))


def test_emu_spectrum_fresh(shk):     # noqa: F811
    AC.run_spectrum_fresh(_emu_factory(shk))


@pytest.mark.parametrize("nshards", [2, 4])
def test_emu_shards(shk, nshards):     # noqa: F811
    AC.run_shards(_emu_factory(shk), nshards)


@pytest.mark.parametrize("checker", CHECKERS)
@pytest.mark.parametrize("pair", PAIRS, ids=_name)
def test_emu_inner_product(shk, pair, checker):     # noqa: F811
    AC.run_inner_product(_emu_factory(shk), pair, _ref(checker))


@pytest.mark.parametrize("checker", CHECKERS)
def test_emu_inner_product_edges(shk, checker):     # noqa: F811
    AC.run_inner_product_edges(_emu_factory(shk), _ref(checker))


@pytest.mark.parametrize("checker", CHECKERS)
@pytest.mark.parametrize("pair", PAIRS + [AC.p_dense], ids=_name)
def test_emu_intersect(shk, pair, checker):     # noqa: F811
    AC.run_intersect(_emu_factory(shk), pair, _ref(checker))


def test_emu_corrupt(shk):     # noqa: F811
    AC.run_corrupt(_emu_factory(shk))


def test_emu_cli(shk):     # noqa: F811
    from shk.spectrum import main
    AC.run_cli(main, ["--lib", EMU])


# ---------------------------------------------------------------- gfx950
@pytest.mark.gpu
@pytest.mark.parametrize("table", AC.TABLES, ids=_name)
def test_gpu_spectrum(table):
    AC.run_spectrum(_gpu_factory(), table)


@pytest.mark.gpu
def test_gpu_spectrum_device():
    AC.run_spectrum_device(_gpu_factory())


@pytest.mark.gpu
def test_gpu_spectrum_fresh():
    AC.run_spectrum_fresh(_gpu_factory())


@pytest.mark.gpu
@pytest.mark.parametrize("nshards", [2, 4])
def test_gpu_shards(nshards):
    AC.run_shards(_gpu_factory(), nshards)


@pytest.mark.gpu
@pytest.mark.parametrize("checker", CHECKERS)
@pytest.mark.parametrize("pair", PAIRS, ids=_name)
def test_gpu_inner_product(pair, checker):
    AC.run_inner_product(_gpu_factory(), pair, _ref(checker))


@pytest.mark.gpu
@pytest.mark.parametrize("checker", CHECKERS)
def test_gpu_inner_product_edges(checker):
    AC.run_inner_product_edges(_gpu_factory(), _ref(checker))


@pytest.mark.gpu
@pytest.mark.parametrize("checker", CHECKERS)
@pytest.mark.parametrize("pair", PAIRS + [AC.p_dense], ids=_name)
def test_gpu_intersect(pair, checker):
    AC.run_intersect(_gpu_factory(), pair, _ref(checker))


@pytest.mark.gpu
def test_gpu_corrupt():
    AC.run_corrupt(_gpu_factory())


@pytest.mark.gpu
def test_gpu_cli():
    """the command line itself, as a process of its own"""
    _, _, _, _, cqf = AC.golden_build(1)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "sh-assembly_amd"))
    r = subprocess.run([sys.executable, "-m", "shk.spectrum", cqf, "-k", "28", "--bins", "64"], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    AC.check_cli_output(r.stdout, cqf)
