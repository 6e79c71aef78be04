"""The sharded build with all shards together in one process (tests/shard_cases.py): the ranks are threads of a loopback
group (tests/loopback_group.py) in place of torch.distributed, so shk/dist.py, the routing with more than one owner, the
staging of received words, the range walk continued from shard to shard and the stitch run on the CPU emulator build of
the kernel sources (test_emu_*) and on ONE gfx950 (test_gpu_*, -m gpu; the groups of shard_cases.EMU_GROUPS stay off it). Every group runs in a fresh child process and is
compared with the oracle's single filter byte for byte. tests/test_dist_gloo.py remains the check of the real
collectives' semantics (gloo processes); the RCCL transport between cards is not exercised here."""
import os
import subprocess
import sys
import threading

import pytest

import loopback_group
import shard_cases as SC
from test_emu_kernels import shk  # noqa: F401  (the fixture builds tests/emu/libshk_emu.so)

EMU_SECONDS, GPU_SECONDS = 300, 120      # limits of a child, not measurements (the slowest emulator group takes about 20 s)


@pytest.fixture(scope="module")
def hostlib():
    """libshkhost.so: the per-rank stitch of shk.dist.export_cqf"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(SC.ROOT, "sh-assembly_amd"), os.path.join(SC.ROOT, "sh-assembly_amd", "libshkhost.so")])


def _child(backend, group, seconds):
    r = subprocess.run([sys.executable, os.path.join(SC.HERE, "shard_cases.py"), backend, group],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=seconds)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SHARD_GROUP_OK %s %s" % (backend, group) in r.stdout, (group, r.stdout[-4000:])


@pytest.mark.parametrize("group", SC.GROUPS + SC.EMU_GROUPS)
def test_emu_shards(shk, hostlib, group):     # noqa: F811
    _child("emu", group, EMU_SECONDS)


@pytest.mark.gpu
@pytest.mark.parametrize("group", SC.GROUPS)
def test_gpu_shards(group):
    _child("gpu", group, GPU_SECONDS)


def test_groups_that_alter_kernel_inputs_stay_off_the_device():
    """the controls hand the walk kernel wrong arguments and `full` overfills a shard on purpose: emulator only (and so
    is `routing`, see its docstring)"""
    assert not set(SC.EMU_GROUPS) & set(SC.GROUPS) and set(SC.RUN) == set(SC.GROUPS + SC.EMU_GROUPS)
    with pytest.raises(AssertionError):
        SC.main(["shard_cases.py", "gpu", "controls"])


# ---------------------------------------------------------------------------------------------- the loopback group itself
def _t(*vals):
    import torch
    return torch.tensor(list(vals), dtype=torch.int64)


def test_loopback_collectives_move_what_the_real_ones_move():
    import torch
    g = loopback_group.Group(3, timeout=10.0)

    def rank_main(rank):
        assert (g.get_rank(), g.get_world_size()) == (rank, 3)
        s = _t(rank + 1, 10 * (rank + 1))
        g.all_reduce(s, op=g.ReduceOp.SUM)
        gathered = torch.empty(6, dtype=torch.int64)
        g.all_gather_into_tensor(gathered, _t(rank, rank * rank))
        # all_to_all: rank r sends r + 1 elements of value 100 r + p to every rank p
        ins = [torch.full((rank + 1,), 100 * rank + p, dtype=torch.int64) for p in range(3)]
        outs = [torch.zeros(p + 1, dtype=torch.int64) for p in range(3)]
        w = g.all_to_all(outs, ins, async_op=True)
        w.wait()
        single = torch.zeros(6, dtype=torch.int64)
        g.all_to_all_single(single, torch.cat(ins), output_split_sizes=[1, 2, 3], input_split_sizes=[rank + 1] * 3)
        token = torch.zeros(2, dtype=torch.int64)
        if rank > 0:
            g.recv(token, src=rank - 1)
        if rank + 1 < 3:
            g.send(token + _t(1, rank), dst=rank + 1)
        g.barrier()
        return s.tolist(), gathered.tolist(), [o.tolist() for o in outs], single.tolist(), token.tolist()

    res = g.run(rank_main)
    for rank, (s, gathered, outs, single, token) in enumerate(res):
        assert s == [6, 60] and gathered == [0, 0, 1, 1, 2, 4]
        assert outs == [[100 * p + rank] * (p + 1) for p in range(3)]
        assert single == [rank, 100 + rank, 100 + rank, 200 + rank, 200 + rank, 200 + rank]
        assert token == [[0, 0], [1, 0], [2, 1]][rank]


def test_loopback_runs_one_rank_at_a_time():
    """between two collectives no other rank's code runs: a counter only the running rank touches is never seen changed"""
    g = loopback_group.Group(4, timeout=10.0)
    running = []

    def rank_main(rank):
        for _ in range(20):
            running.append(rank)
            n = len(running)
            for _ in range(2000):
                assert len(running) == n and running[-1] == rank
            g.barrier()
        return True

    assert g.run(rank_main) == [True] * 4


def test_loopback_ranks_in_different_collectives_fail_at_once():
    g = loopback_group.Group(2, timeout=30.0)

    def rank_main(rank):
        if rank == 0:
            g.all_reduce(_t(1))
        else:
            g.barrier()

    with pytest.raises(AssertionError, match="is in"):
        g.run(rank_main)


def test_loopback_a_failed_rank_ends_the_run_with_its_own_exception():
    g = loopback_group.Group(3, timeout=30.0)

    def rank_main(rank):
        g.barrier()
        if rank == 1:
            raise ValueError("rank 1 broke")
        g.all_reduce(_t(rank))          # the others wait here; they are woken and leave
        g.barrier()

    with pytest.raises(ValueError, match="rank 1 broke"):
        g.run(rank_main)
    assert not [t for t in threading.enumerate() if t.name.startswith("rank")]


def test_loopback_a_wait_nobody_answers_times_out():
    """(a limit of zero seconds: the first look at the clock ends the wait, the test itself waits for nothing)"""
    g = loopback_group.Group(2, timeout=0.0)

    def rank_main(rank):
        if rank == 0:
            t = _t(0)
            g.recv(t, src=1)            # rank 1 never sends, and stays busy in a collective of its own
        else:
            g.barrier()

    with pytest.raises((TimeoutError, AssertionError)):
        g.run(rank_main)


def test_loopback_a_rank_that_returns_early_does_not_leave_the_others_waiting():
    g = loopback_group.Group(2, timeout=30.0)

    def rank_main(rank):
        if rank == 0:
            return "gone"
        g.barrier()

    with pytest.raises(TimeoutError, match="a rank has returned"):
        g.run(rank_main)
