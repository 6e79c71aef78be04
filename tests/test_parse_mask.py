"""Newline flags kept between k_count_lines and k_emit_reads (tests/parse_mask_cases.py): every group of cases once on the
CPU emulator build of the kernel sources (test_emu_*) and once on the gfx950 library (test_gpu_*, -m gpu), each time in two
fresh child processes: as built, and with SHK_PARSE_MASK=0 (the variable is read when a context is created). Both runs give
the oracle's values (asserted in the child) and the same digest of words, tables and parse kernel names. The stand-alone
AddressSanitizer program of tests/emu/parse_mask_asan.cpp (the emulator sources, its own main) runs here on the CPU."""
import json
import os
import subprocess
import sys

import pytest

import parse_mask_cases as PC
from test_emu_kernels import shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _child(backend, group, off):
    env = dict(os.environ)
    env.pop("SHK_PARSE_MASK", None)
    if off:
        env["SHK_PARSE_MASK"] = "0"
    r = subprocess.run([sys.executable, os.path.join(PC.HERE, "parse_mask_cases.py"), backend, group], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "PARSE_MASK_GROUP_OK" in r.stdout, (group, off, r.stdout[-4000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["digest"]


def _both(backend, group):
    digests = [_child(backend, group, off) for off in (False, True)]
    assert digests[0] == digests[1], (group, digests)


def test_the_texts_hold_what_they_are_for():
    """the generators assert their own geometry (residues reached, shared units and groups, unit counts, capacities)"""
    PC.group_edge_text()
    PC.chunk_edge_text()
    for threads in (64, 512, 1024):
        PC.rounds_text(threads)
    PC.growth_texts()
    PC.stale_texts()


@pytest.mark.parametrize("group", PC.EMU_GROUPS)
def test_emu_parse_mask(shk, group):     # noqa: F811
    _both("emu", group)


@pytest.mark.gpu
@pytest.mark.parametrize("group", PC.GPU_GROUPS)
def test_gpu_parse_mask(group):
    _both("gpu", group)


def test_flags_buffer_under_address_sanitizer():
    """tests/emu/parse_mask_asan.cpp: shk_hash_chunks and shk_count_chunks of the emulator build, compiled with
    -fsanitize=address into a program of its own, on chunk-edge and growth texts in allocations that end at the next multiple
    of 16 behind the text; with the flags and with SHK_PARSE_MASK=0"""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a sanitizer build for the CPU: not built or run on a machine with a GPU")
    emu = os.path.join(PC.HERE, "emu")
    subprocess.check_call(["make", "-s", "-C", emu, "-f", "parse_mask_asan.mk"])
    for off in (False, True):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        env.pop("LD_PRELOAD", None)
        env.pop("SHK_PARSE_MASK", None)
        if off:
            env["SHK_PARSE_MASK"] = "0"
        r = subprocess.run([os.path.join(emu, "parse_mask_asan")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and "PARSE_MASK_ASAN_OK" in r.stdout, (off, r.stdout[-4000:])
