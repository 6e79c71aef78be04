"""Lazy placement (tests/lazy_cases.py): every case once on the CPU emulator build of the kernel sources (test_emu_*) and
once on the gfx950 library (test_gpu_*, -m gpu)."""
import ctypes as C

import pytest

import lazy_cases as LC
from test_emu_kernels import _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _emu_factory(shk):     # noqa: F811
    def mk(**kw):
        ctx = _emu_ctx(shk, **kw)
        held = []

        def dev_words(ws):
            arr = (C.c_uint64 * max(len(ws), 1))(*ws)
            held.append(arr)
            return C.addressof(arr)
        ctx.dev_words = dev_words
        return ctx
    return mk


def _gpu_factory():
    import torch
    import shk as gshk
    dev = torch.device("cuda", 0)

    def mk(**kw):
        ctx = gshk.Context(**kw)
        held = []

        def dev_words(ws):
            t = torch.tensor(ws if ws else [0], dtype=torch.int64).to(dev)
            torch.cuda.synchronize()
            held.append(t)
            return t.data_ptr()
        ctx.dev_words = dev_words
        return ctx
    return mk


SIMPLE = [LC.run_chain, LC.run_alternating, LC.run_over_list, LC.run_failed_pass, LC.run_prepared, LC.run_partial_region, LC.run_sparse]
SCHEMES = ["fused", "two-pass", "guess"]


def test_point_reference_has_two_rounds():
    """the reads of the deNoise-point cases: the oracle alone takes at least two rounds and does not fill up"""
    from fastq_util import chunks_by_records, oracle_t1
    P = LC.POINT
    fq = LC.point_reads()
    offs, lens = chunks_by_records(fq, P["per"])
    q, orounds, _ = oracle_t1(fq, offs, lens, LC.K, P["qb"], P["trigger"], P["num_denoise"], False, P["ml"])
    assert not q.full() and orounds >= 2
    q.free()


@pytest.mark.parametrize("case", SIMPLE, ids=lambda f: f.__name__[4:])
def test_emu_lazy(shk, case):     # noqa: F811
    case(_emu_factory(shk))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_emu_lazy_points(shk, scheme):     # noqa: F811
    LC.run_points(_emu_factory(shk), scheme)


def test_emu_lazy_readers(shk, tmp_path):     # noqa: F811
    import shk as m
    LC.run_readers(_emu_factory(shk), m.UnitigSet, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SIMPLE, ids=lambda f: f.__name__[4:])
def test_gpu_lazy(case):
    case(_gpu_factory())


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_gpu_lazy_points(scheme):
    LC.run_points(_gpu_factory(), scheme)


@pytest.mark.gpu
def test_gpu_lazy_readers(tmp_path):
    import shk as m
    LC.run_readers(_gpu_factory(), m.UnitigSet, tmp_path)
