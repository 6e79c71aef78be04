"""Slots above the last partition level (tests/roll_slots_cases.py): every group of cases once on the CPU emulator build of
the kernel sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu), each time in two fresh child
processes: as built, and with SHK_ROLL_SLOTS=0 (the variable is read when a context is created)."""
import json
import os
import subprocess
import sys

import pytest

import roll_slots_cases as RC
from test_emu_kernels import shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _child(backend, group, off):
    env = dict(os.environ)
    env.pop("SHK_ROLL_SLOTS", None)
    if off:
        env["SHK_ROLL_SLOTS"] = "0"
    r = subprocess.run([sys.executable, os.path.join(RC.HERE, "roll_slots_cases.py"), backend, group], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ROLL_SLOTS_GROUP_OK" in r.stdout, (group, off, r.stdout[-4000:])
    return r.stdout


def _both(backend, group):
    outs = [_child(backend, group, off) for off in (False, True)]
    if group == "shard":
        # the slotted path refuses the batch with the error the histogram path gives
        codes = [json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1])["code"] for o in outs]
        assert codes[0] == codes[1] == RC.ERR_CORRUPT, codes


def test_the_common_shape_meets_the_rule():
    """(3, 3, 2) at qb 16 and the shard's (3, 2, 2) as create_init splits them; a level-1 bucket's share of a full batch is
    at least 28,800 keys; the wide case's (5, 5, 5) likewise; the contexts of the older slot tests (65,536 keys) stay below"""
    import partition_cases as PC
    assert PC.levels(RC.QB, RC.MLB) == (3, 3, 2) and PC.levels(RC.QB - 1, RC.MLB) == (3, 2, 2) and PC.levels(23, 7) == (5, 5, 5)
    assert RC.MAX_KEYS // (1 << 6) >= 28800 and (1 << 25) // (1 << 10) >= 28800
    assert (1 << 16) // (1 << 6) < 28800 and (1 << 20) // (1 << 6) < 28800


@pytest.mark.parametrize("group", RC.EMU_GROUPS)
def test_emu_roll_slots(shk, group):     # noqa: F811
    _both("emu", group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", RC.GPU_GROUPS)
def test_gpu_roll_slots(group):
    _both("gpu", group)
