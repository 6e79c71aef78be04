"""The rebuild kernel's fold of batch words into the region's LDS hash (tests/fold_cases.py): every group of cases once on
the CPU emulator build of the kernel sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu), each in a
fresh child process."""
import os
import subprocess
import sys

import pytest

import fold_cases as FC
from test_emu_kernels import shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _child(backend, group):
    r = subprocess.run([sys.executable, os.path.join(FC.HERE, "fold_cases.py"), backend, group],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FOLD_GROUP_OK" in r.stdout, (group, r.stdout[-4000:])


def test_entries_follow_the_kernels_formula():
    """128 tags share each of the 512 entries; the chains the groups build are chains"""
    assert FC.entry(0) == 0 and FC.entry(1) == (40503 >> 7) and FC.entry(0xFFFF) == ((0xFFFF * 40503) & 0xFFFF) >> 7
    for e in (0, 150, 200, 505, 511):
        ts = FC.tags_of(e)
        assert len(ts) == 128 and all(FC.entry(t) == e for t in ts)
    assert FC.key(0x1234) >> 16 == FC.REGION and (FC.key(0x1234) >> 8) // 256 == FC.REGION


@pytest.mark.parametrize("group", FC.GROUPS)
def test_emu_fold(shk, group):     # noqa: F811
    _child("emu", group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", FC.GROUPS)
def test_gpu_fold(group):
    _child("gpu", group)
