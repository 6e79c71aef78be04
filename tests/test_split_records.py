"""The split record between the roll kernels and the middle partition level (tests/split_cases.py): every group of cases
once on the CPU emulator build of the kernel sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu), each
time in two fresh child processes: as built, and with SHK_RP_SPLIT=0 (the variable is read when a context is created).

Which path ran is asserted in the child with Context.split_batches() (shk_split_batches): the profile keys are the same for
both forms and cannot tell."""
import json
import os
import subprocess
import sys

import pytest

import split_cases as SC
from test_emu_kernels import shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _child(backend, group, off):
    env = dict(os.environ)
    for v in ("SHK_RP_SPLIT", "SHK_RP_WORDS8", "SHK_ROLL_SLOTS"):
        env.pop(v, None)
    if off:
        env["SHK_RP_SPLIT"] = "0"
    r = subprocess.run([sys.executable, os.path.join(SC.HERE, "split_cases.py"), backend, group], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "SPLIT_GROUP_OK" in r.stdout, (group, off, r.stdout[-4000:])
    return r.stdout


def _both(backend, group):
    outs = [_child(backend, group, off) for off in (False, True)]
    if group == "rule":
        # a shard's context keeps 8-byte words and the middle level's range check with them: the same refusal either way
        codes = [json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1])["code"] for o in outs]
        assert codes[0] == codes[1] and codes[0] < 0, codes


def test_geometries_match_the_rule():
    """the levels the table names are the ones create_init's split gives; kb and cb as the record needs them; qb 33 is the
    last three-level geometry whose record fits 40 bits"""
    import partition_cases as PC
    for name in ("two", "three", "four", "edge"):
        qb, mlb, levels = SC.GEOM[name]
        assert PC.levels(qb, mlb) == levels, name
    assert PC.levels(14, 2) == (2, 2, 2) and PC.levels(SC.RC.QB, SC.RC.MLB) == (3, 3, 2)
    for qb, levels, total in ((16, (3, 3, 2), 35), (23, (5, 5, 5), 37), (14, (2, 2, 2), 34), (29, (7, 7, 7), 39)):
        assert SC.kb_of(qb, levels) + SC.NC.cb_of(levels) == total
    assert PC.levels(33, 10) == (9, 8, 8) and SC.kb_of(33, (9, 8, 8)) == 32 and SC.kb_of(33, (9, 8, 8)) + 8 == 40
    assert PC.levels(34, 10) == (9, 9, 8) and SC.kb_of(34, (9, 9, 8)) + 8 == 41


@pytest.mark.parametrize("group", SC.EMU_GROUPS)
def test_emu_split(shk, group):     # noqa: F811
    _both("emu", group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", SC.GPU_GROUPS)
def test_gpu_split(group):
    _both("gpu", group)
