"""The narrow record between the last two partition levels (tests/narrow_cases.py): every group of cases once on the CPU
emulator build of the kernel sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu), each time in two
fresh child processes: as built, and with SHK_RP_WORDS8=1 (the variable is read when a context is created)."""
import json
import os
import subprocess
import sys

import pytest

import narrow_cases as NC
from test_emu_kernels import shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _child(backend, group, tmp_path, words8):
    env = dict(os.environ)
    env.pop("SHK_RP_WORDS8", None)
    if words8:
        env["SHK_RP_WORDS8"] = "1"
    d = tmp_path / ("w8" if words8 else "built")
    d.mkdir()
    r = subprocess.run([sys.executable, os.path.join(NC.HERE, "narrow_cases.py"), backend, group, str(d)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "NARROW_GROUP_OK" in r.stdout, (group, words8, r.stdout[-4000:])
    return r.stdout


def _both(backend, group, tmp_path):
    outs = [_child(backend, group, tmp_path, w8) for w8 in (False, True)]
    if group == "corrupt":
        # the moved check: the narrow path refuses the batch with the error the 8-byte path gives
        codes = [json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1])["code"] for o in outs]
        assert codes[0] == codes[1] and codes[0] < 0, codes


def test_geometries_match_the_rule():
    """the levels the table names are the ones create_init's split gives; cb as the record needs it"""
    import partition_cases as PC
    for name, (qb, mlb, levels) in NC.GEOM.items():
        assert PC.levels(qb, mlb) == levels, name
    assert PC.levels(16 - 1, 3) == (3, 2, 2)      # the shard of the corrupt case: 2^15 quotients
    assert NC.cb_of(NC.GEOM["three"][2]) == 14 and NC.cb_of(NC.GEOM["edge"][2]) == 11


@pytest.mark.parametrize("group", NC.EMU_GROUPS)
def test_emu_narrow(shk, tmp_path, group):     # noqa: F811
    _both("emu", group, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("group", NC.GPU_GROUPS)
def test_gpu_narrow(tmp_path, group):
    _both("gpu", group, tmp_path)
