"""The early loads of the record-sourced rebuild kernels (tests/prefetch_cases.py): every group of cases once on the CPU
emulator build of the kernel sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu), each in a fresh child
process."""
import os
import subprocess
import sys

import pytest

import prefetch_cases as PC
from test_emu_kernels import shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _child(backend, group):
    env = {k: v for k, v in os.environ.items() if k not in ("SHK_MERGE_PREFETCH", "SHK_SAMPLE_STRIDE", "SHK_DEBUG_FUSED")}
    r = subprocess.run([sys.executable, os.path.join(PC.HERE, "prefetch_cases.py"), backend, group], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "PREFETCH_GROUP_OK" in r.stdout, (group, r.stdout[-4000:])


def test_case_keys_have_the_sizes_they_claim():
    """n once-seen keys with remainders >= 2 are n distinct keys of one region, at most two to a quotient"""
    for n in (0, 1, 255, 256, 257, 511, 512):
        ks = PC.singles(3, n)
        assert len(ks) == n and all(k >> 16 == 3 and (k & 0xff) >= 2 for k in ks)
    assert not set(PC.singles(3, 4, first=257)) & set(PC.singles(3, 257))
    assert sum(PC.repeats(2, 1100, 60).values()) == 1100 and len(PC.repeats(2, 1100, 60)) <= 60


@pytest.mark.parametrize("group", PC.GROUPS)
def test_emu_prefetch(shk, group):     # noqa: F811
    _child("emu", group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", PC.GROUPS)
def test_gpu_prefetch(group):
    _child("gpu", group)
