"""The partition plan (tests/partition_cases.py): every case once on the CPU emulator build of the kernel sources (test_emu_*)
and once on the gfx950 library (test_gpu_*, -m gpu)."""
import pytest

import partition_cases as PC
from test_emu_kernels import _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _factory(new_ctx, device):
    """contexts with the two things the cases add: where torch keeps the ranks' statistics, and copies of a words buffer"""
    from shk import dist as shkdist

    def mk(**kw):
        ctx = new_ctx(**kw)
        held = []

        def split(ptr, n, m):
            w = shkdist.wrap_words(ptr, n, device)
            a, b = w[:m].clone(), w[m:].clone()
            held.extend((a, b))
            return a.data_ptr(), m, b.data_ptr(), n - m
        ctx.split = split
        ctx.device = device
        return ctx
    return mk


def _emu_factory(shk):     # noqa: F811
    import torch
    return _factory(lambda **kw: _emu_ctx(shk, **kw), torch.device("cpu"))


def _gpu_factory():
    import torch
    import shk as gshk
    return _factory(gshk.Context, torch.device("cuda", 0))


def test_case_table_matches_the_geometry():
    """the levels the case table names are the ones create_init's rule gives"""
    for name, case in PC.CASES.items():
        assert PC.levels(case[0], case[1]) == case[2], name


@pytest.mark.parametrize("flow", PC.TEXT_FLOWS)
@pytest.mark.parametrize("name", PC.EMU_CASES)
def test_emu_partition_text(shk, name, flow):     # noqa: F811
    PC.run_text(_emu_factory(shk), name, (flow,))


@pytest.mark.parametrize("flow", PC.WORD_FLOWS)
@pytest.mark.parametrize("name", [n for n in PC.EMU_CASES if n >= "c"])
def test_emu_partition_words(shk, tmp_path, name, flow):     # noqa: F811
    PC.run_words(_emu_factory(shk), name, "gloo", tmp_path, (flow,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_gpu_partition_text(name):
    PC.run_text(_gpu_factory(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in sorted(PC.CASES) if n >= "c"])
def test_gpu_partition_words(tmp_path, name):
    PC.run_words(_gpu_factory(), name, "nccl", tmp_path)
