"""The device front end (newline counter, read-extent emitter, per-read key counter, 2-bit packer, thread-per-read roll
kernels, wave-per-read hash) over the FASTQ text shapes of tests/text_cases.py: once on the CPU emulator build of the
kernel sources (test_emu_*), once on the gfx950 library (test_gpu_*, -m gpu). Expected values are the oracle's;
tests/test_oracle.py holds the oracle to the compiled reference on the same texts."""
import ctypes as C

import pytest

import text_cases as TC
from test_emu_kernels import _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)

_libc = C.CDLL(None)
_libc.posix_memalign.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t]
_libc.free.argtypes = [C.c_void_p]


def _emu_factory(shk):     # noqa: F811
    """contexts on the emulator build; their "device" text is host memory of exactly the documented extent"""
    def mk(**kw):
        ctx = _emu_ctx(shk, **kw)
        ctx.read_words = lambda dp, n: list((C.c_uint64 * max(n, 1)).from_address(dp)[:n])
        held = []

        def dev_text(data, offset=0):
            p = C.c_void_p()
            assert _libc.posix_memalign(C.byref(p), 16, offset + ((len(data) + 15) & ~15)) == 0
            C.memmove(p.value + offset, data, len(data))
            held.append(p)
            return p.value + offset
        ctx.dev_text = dev_text
        close = ctx.close

        def close_and_free():
            close()
            while held:
                _libc.free(held.pop())
        ctx.close = close_and_free
        return ctx
    return mk


def _gpu_factory():
    import torch
    import shk as gshk
    from shk import dist as shkdist
    dev = torch.device("cuda", 0)

    def mk(**kw):
        ctx = gshk.Context(**kw)
        ctx.read_words = lambda dp, n: [x & 0xFFFFFFFFFFFFFFFF for x in shkdist.wrap_words(dp, n, dev).cpu().tolist()] if n else []
        held = []

        def dev_text(data, offset=0):
            t = torch.empty(offset + ((len(data) + 15) & ~15), dtype=torch.uint8, device=dev)
            t[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            torch.cuda.synchronize()
            held.append(t)
            assert t.data_ptr() % 16 == 0
            return t.data_ptr() + offset
        ctx.dev_text = dev_text
        return ctx
    return mk


LINE_NAMES = ["lines-" + n for n in (
    "no-final-newline", "cut-inside-quality", "stops-after-sequence-line", "stops-inside-sequence-line", "stops-after-plus-newline",
    "stops-after-plus", "stops-after-header", "empty-sequence-line", "empty-header-and-quality", "lone-cr-in-read",
    "newline-chunks-and-short-chunks", "crlf-k21-per1", "crlf-k21-per4", "crlf-k21-per24", "crlf-k47-per1", "crlf-k47-per4",
    "crlf-k47-per24")]
CHUNK_NAMES = ["chunks-" + n for n in ("one-record-each", "descending", "shuffled", "with-gaps", "of-1-to-15-bytes-and-empty", "4096")]


def test_case_lists_are_complete():
    """the names the tests below are parametrised with are all the texts the generators build"""
    assert list(TC.group(TC.long_read_texts)) == TC.LONG_NAMES
    assert list(TC.group(TC.line_texts)) == LINE_NAMES
    assert list(TC.group(TC.chunk_table_texts)) == CHUNK_NAMES


def _long(mk, name):
    TC.check(mk, TC.group(TC.long_read_texts)[name])


def _beside(mk, k):
    """bytes beside the read: every neighbour pattern gives the key words of plain 'I' qualities (and the oracle's)"""
    texts = TC.neighbour_texts(k)
    words = {pat: TC.check(mk, T) for pat, T in texts.items()}
    assert len(words["I"]) > 1000
    for pat in TC.NEIGHBOURS:
        assert words[pat] == words["I"], pat


def _chunks(mk, name, emu=False):
    G = TC.group(TC.chunk_table_texts)
    T = G[name]
    words = TC.check(mk, T, short=emu and name == "chunks-4096")
    if name == "chunks-shuffled":
        # shuffling the chunk table shuffles the chunk tags and nothing else
        base, hb = G["chunks-one-record-each"], T.qb + 8
        by_off = {}
        for w in base.expected()[0]:
            by_off.setdefault(base.offs[w >> hb], []).append(w & ((1 << hb) - 1))
        got = {}
        for w in words:
            got.setdefault(T.offs[w >> hb], []).append(w & ((1 << hb) - 1))
        assert got == by_off and sorted(T.offs) == base.offs and T.offs != base.offs
        assert T.expected()[1:] == base.expected()[1:]
    if name == "chunks-4096":
        TC.run_chunk_limit(mk, T)


# ---------------------------------------------------------------------------------------------------- emulator build
@pytest.mark.parametrize("name", TC.LONG_NAMES)
def test_emu_long_reads(shk, name):     # noqa: F811
    _long(_emu_factory(shk), name)


@pytest.mark.parametrize("bad_len", [65536, 70000, 200000])
def test_emu_read_longer_than_65535_is_refused_and_leaves_no_trace(shk, bad_len):     # noqa: F811
    TC.run_too_long(_emu_factory(shk), bad_len)


@pytest.mark.parametrize("k", [21, 47])
def test_emu_bytes_beside_the_read(shk, k):     # noqa: F811
    _beside(_emu_factory(shk), k)


@pytest.mark.parametrize("name", LINE_NAMES)
def test_emu_line_structure(shk, name):     # noqa: F811
    TC.check(_emu_factory(shk), TC.group(TC.line_texts)[name])


@pytest.mark.parametrize("name", CHUNK_NAMES)
def test_emu_chunk_tables(shk, name):     # noqa: F811
    _chunks(_emu_factory(shk), name, emu=True)


def test_emu_unaligned_device_text_is_refused(shk):     # noqa: F811
    TC.run_alignment(_emu_factory(shk), TC.neighbour_texts(21)["qualN"])


def test_emu_randomised_configurations_with_long_reads(shk):     # noqa: F811
    """tools/fuzz_gpu.py --long-reads on the emulator build: the random configurations of the default draw, on a filter of
    qb 17 so that two or three reads of 600 .. 20000 bases fit on top, quality lines of 'N' and '@'; table bytes, header, counters, rounds and removed counts
    equal the oracle's t = 1 build in every case"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_gpu.py"), "--emu", "--max-qb", "13", "--cases", "40", "--seed", "5",
                        "--long-reads"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    assert "fuzz: 40 cases (0 skipped" in r.stdout and ", 0 mismatches" in r.stdout, r.stdout[-500:]
    # the draw really holds what it is for: several long reads per case, some of them beyond 10000 bases
    import re
    m = re.search(r"long reads: (\d+) in (\d+) cases, (\d+) above 10000 bases, longest (\d+)", r.stdout)
    assert m, r.stdout[-500:]
    nlong, ncases, above, longest = map(int, m.groups())
    assert ncases == 40 and nlong >= 2 * ncases and above >= 10 and 10000 < longest <= 20000, m.group(0)


# ---------------------------------------------------------------------------------------------------- gfx950 library
@pytest.mark.gpu
@pytest.mark.parametrize("name", TC.LONG_NAMES)
def test_gpu_long_reads(name):
    _long(_gpu_factory(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("bad_len", [65536, 70000, 200000])
def test_gpu_read_longer_than_65535_is_refused_and_leaves_no_trace(bad_len):
    TC.run_too_long(_gpu_factory(), bad_len)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 47])
def test_gpu_bytes_beside_the_read(k):
    _beside(_gpu_factory(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LINE_NAMES)
def test_gpu_line_structure(name):
    TC.check(_gpu_factory(), TC.group(TC.line_texts)[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHUNK_NAMES)
def test_gpu_chunk_tables(name):
    _chunks(_gpu_factory(), name)


@pytest.mark.gpu
def test_gpu_unaligned_device_text_is_refused():
    """(the refusal is a test of the pointer's value on the host: no kernel ever sees the unaligned pointer)"""
    TC.run_alignment(_gpu_factory(), TC.neighbour_texts(21)["qualN"])
