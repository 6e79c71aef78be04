"""The read side (tests/read_cases.py): every case once on the CPU emulator build of the kernel sources (test_emu_*) and
once on the gfx950 library (test_gpu_*, -m gpu); the preconditions of the cases on the oracle alone."""
import ctypes as C

import pytest

import read_cases as RC
from test_emu_kernels import _ctx as _emu_ctx, shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)


def _emu_factory(shk):     # noqa: F811
    def mk(**kw):
        ctx = _emu_ctx(shk, **kw)
        held = []

        def dev_words(ws):
            arr = (C.c_uint64 * max(len(ws), 1))(*ws)
            held.append(arr)
            return C.addressof(arr)

        def dev_out(nbytes):
            buf = C.create_string_buffer(max(nbytes, 1))
            held.append(buf)
            return C.addressof(buf), lambda: buf.raw[:nbytes]
        ctx.dev_words, ctx.dev_out = dev_words, dev_out
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

        def dev_out(nbytes):
            t = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            held.append(t)
            return t.data_ptr(), lambda: t.cpu().numpy().tobytes()[:nbytes]
        ctx.dev_words, ctx.dev_out = dev_words, dev_out
        return ctx
    return mk


LOOKUPS = sorted(RC.TABLES)
WRITERS = ["count_words", "insert_counted", "merge"]
STAGED = ["try", "point"]


def test_denoise_reference_removes_marked_singletons():
    """the table of the marks-then-deNoise cases, on the oracle alone: the round removes at least 100 singletons, at
    least 20 of the keys the cases mark are singletons it removes, and at least one singleton survives it (the range
    walk's protected slot) -- so a round that honoured a reader's marks would be seen, and so would one that lost its own"""
    fq, offs, lens, q, marks = RC.denoise_table()
    before = dict(q.dump())
    removed = q.denoise_round(RC.DN["ml"])
    after = dict(q.dump())
    gone = set(before) - set(after)
    assert removed == len(gone) >= 100 and all(before[x] == 1 for x in gone)
    assert len(gone & set(marks)) >= 20
    assert sum(1 for c in after.values() if c == 1) >= 1
    q.free()


def test_denoise_inside_count_reference_fires_in_the_second_call():
    """the schedule of the round-inside-a-counting-call case, on the oracle alone: no round in the first three chunks, at
    least one behind them, and it removes something"""
    from fastq_util import oracle_t1
    fq, offs, lens, q, _ = RC.denoise_table()
    q.free()
    P = RC.DN_SCHED
    q1, r1, _ = oracle_t1(fq, offs[:3], lens[:3], RC.DN["k"], RC.DN["qb"], P["trigger"], P["num_denoise"], False, RC.DN["ml"])
    q2, r2, removed = oracle_t1(fq, offs, lens, RC.DN["k"], RC.DN["qb"], P["trigger"], P["num_denoise"], False, RC.DN["ml"])
    assert r1 == 0 and r2 >= 1 and removed >= 100 and not q2.full()
    q1.free()
    q2.free()


@pytest.mark.parametrize("table", LOOKUPS)
def test_emu_lookups(shk, table):     # noqa: F811
    RC.run_lookups(_emu_factory(shk), table, huge_by_import=True)


def test_emu_lookups_sharded(shk):     # noqa: F811
    RC.run_lookups_sharded(_emu_factory(shk))


def test_emu_denoise_after_lookup(shk):     # noqa: F811
    RC.run_denoise_after_lookup(_emu_factory(shk))


def test_emu_denoise_after_import(shk):     # noqa: F811
    RC.run_denoise_after_import(_emu_factory(shk))


@pytest.mark.parametrize("flow", sorted(RC.FLOWS))
def test_emu_denoise_inside_count(shk, flow):     # noqa: F811
    RC.run_denoise_inside_count(_emu_factory(shk), flow)


@pytest.mark.parametrize("path", STAGED)
def test_emu_denoise_staged(shk, path):     # noqa: F811
    RC.run_denoise_staged(_emu_factory(shk), path)


@pytest.mark.parametrize("writer", WRITERS)
def test_emu_writers_drop_marks(shk, writer):     # noqa: F811
    RC.run_writers_drop_marks(_emu_factory(shk), writer)


def test_emu_denoise_after_contiger(shk):     # noqa: F811
    RC.run_denoise_after_contiger(_emu_factory(shk), shk.UnitigSet)


@pytest.mark.gpu
@pytest.mark.parametrize("table", LOOKUPS)
def test_gpu_lookups(table):
    RC.run_lookups(_gpu_factory(), table)


@pytest.mark.gpu
def test_gpu_lookups_sharded():
    RC.run_lookups_sharded(_gpu_factory())


@pytest.mark.gpu
def test_gpu_denoise_after_lookup():
    RC.run_denoise_after_lookup(_gpu_factory())


@pytest.mark.gpu
def test_gpu_denoise_after_import():
    RC.run_denoise_after_import(_gpu_factory())


@pytest.mark.gpu
@pytest.mark.parametrize("flow", sorted(RC.FLOWS))
def test_gpu_denoise_inside_count(flow):
    RC.run_denoise_inside_count(_gpu_factory(), flow)


@pytest.mark.gpu
@pytest.mark.parametrize("path", STAGED)
def test_gpu_denoise_staged(path):
    RC.run_denoise_staged(_gpu_factory(), path)


@pytest.mark.gpu
@pytest.mark.parametrize("writer", WRITERS)
def test_gpu_writers_drop_marks(writer):
    RC.run_writers_drop_marks(_gpu_factory(), writer)


@pytest.mark.gpu
def test_gpu_denoise_after_contiger():
    import shk as m
    RC.run_denoise_after_contiger(_gpu_factory(), m.UnitigSet)


# ---------------------------------------------------------------- walks on low-complexity sequence
WALK_K = [21, 32, 66]


@pytest.mark.parametrize("k", WALK_K)
def test_emu_extend_forward_low_complexity(shk, k):     # noqa: F811
    RC.run_extend_forward(_emu_factory(shk), k)


@pytest.mark.parametrize("k", WALK_K)
def test_emu_unitigs_from_seeds_low_complexity(shk, k):     # noqa: F811
    RC.run_unitigs_from_seeds(_emu_factory(shk), k)


@pytest.mark.parametrize("k", WALK_K)
def test_emu_select_seeds_low_complexity(shk, k):     # noqa: F811
    RC.run_select_seeds(_emu_factory(shk), k)


@pytest.mark.parametrize("k", WALK_K)
def test_emu_pipeline_low_complexity(shk, tmp_path, k):     # noqa: F811
    RC.run_pipeline(_emu_factory(shk), shk.UnitigSet, tmp_path, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", WALK_K)
def test_gpu_extend_forward_low_complexity(k):
    RC.run_extend_forward(_gpu_factory(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", WALK_K)
def test_gpu_unitigs_from_seeds_low_complexity(k):
    RC.run_unitigs_from_seeds(_gpu_factory(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", WALK_K)
def test_gpu_select_seeds_low_complexity(k):
    RC.run_select_seeds(_gpu_factory(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", WALK_K)
def test_gpu_pipeline_low_complexity(tmp_path, k):
    import shk as m
    RC.run_pipeline(_gpu_factory(), m.UnitigSet, tmp_path, k)
