"""A process group whose ranks are threads of one process, for running shk/dist.py with all shards of a filter on one
device (or on the emulator build) without a transport: install it with `shk.dist.dist = Group(world)` and start the ranks
with `Group.run(target)`. It has the surface of torch.distributed that shk/dist.py uses -- get_rank, get_world_size,
ReduceOp, all_reduce (SUM), all_gather_into_tensor, all_to_all, all_to_all_single, send, recv, barrier -- and nothing else.

Scheduling is cooperative: ONE lock (the group's condition variable) is held by whichever rank thread runs and is given
up only while that thread waits inside a collective or a recv. The library under the ranks is therefore never entered by
two threads at once, and a run is a fixed interleaving of the ranks' code.

A collective is a rendezvous: every rank leaves (name, payload) and waits for the others; the ranks must all have entered
the SAME collective, anything else fails the run at once. Data moves by copies between the ranks' own tensors, made by
the receiver after the first rendezvous; a second rendezvous behind the copies keeps every rank inside the call until all
peers have read what it offered (nobody reuses a send buffer a peer has not read yet).

A rank that raises ends the run: it sets the group's failure and wakes the others, whose waits then raise Aborted; every
wait also gives up after `timeout` seconds (a rank that returned early, a recv nobody sends to). run() raises the first
real exception."""
import collections
import threading
import time


class Aborted(RuntimeError):
    """raised in the ranks that were waiting when another rank failed (never the first cause)"""


class _ReduceOp:
    SUM = "sum"


class _Done:
    """the work object of an all_to_all(async_op=True): the copies were made inside the call"""

    def wait(self):
        return True


class Group:
    ReduceOp = _ReduceOp

    def __init__(self, world, timeout=60.0, device_sync=None, a2a_shift=0):
        """device_sync: called behind the copies of a collective (torch.cuda.synchronize on a GPU). a2a_shift: a fault to
        inject for the controls of the tests -- every rank is handed the bin meant for rank + a2a_shift."""
        self.world, self.timeout, self.device_sync, self.a2a_shift = world, timeout, device_sync, a2a_shift
        self.cond = threading.Condition()
        self._tls = threading.local()
        self.failure = None                 # the first real exception of any rank
        self._slots = [None] * world        # (name, payload) of the ranks waiting in the current rendezvous
        self._arrived = 0
        self._gen = 0
        self._result = None
        self._mail = collections.defaultdict(collections.deque)   # (src, dst) -> sent tensors
        self._returned = 0                  # ranks whose target has returned
        self.log = []                       # names of the completed rendezvous, in order

    # ------------------------------------------------------------------------------------------------ the surface
    def get_rank(self):
        return self._tls.rank

    def get_world_size(self):
        return self.world

    def is_initialized(self):
        return True

    def barrier(self):
        self._meet("barrier")

    def all_reduce(self, t, op=None):
        assert op in (None, _ReduceOp.SUM), op
        parts = self._meet("all_reduce", t)
        assert all(p.shape == t.shape and p.dtype == t.dtype for p in parts), "all_reduce: the ranks' tensors differ in shape"
        total = parts[0].clone()
        for p in parts[1:]:
            total += p
        self._sync()
        self._meet("all_reduce/read")
        t.copy_(total)
        self._sync()

    def all_gather_into_tensor(self, out, inp):
        parts = self._meet("all_gather_into_tensor", inp)
        n = inp.numel()
        assert out.numel() == n * self.world and all(p.numel() == n for p in parts), "all_gather: sizes differ"
        flat = out.view(-1)
        for p, src in enumerate(parts):
            flat[p * n:(p + 1) * n].copy_(src.view(-1))
        self._sync()
        self._meet("all_gather_into_tensor/read")

    def all_to_all(self, outs, ins, async_op=False):
        """outs[p] <- what rank p put into its ins[my rank], straight between the views"""
        assert len(outs) == len(ins) == self.world
        offered = self._meet("all_to_all", list(ins))
        me = (self.get_rank() + self.a2a_shift) % self.world
        for p in range(self.world):
            src = offered[p][me]
            if src.numel() != outs[p].numel():
                raise RuntimeError("all_to_all: rank %d sends %d elements to rank %d, which expects %d"
                                   % (p, src.numel(), self.get_rank(), outs[p].numel()))
            outs[p].copy_(src)
        self._sync()
        self._meet("all_to_all/read")
        return _Done() if async_op else None

    def all_to_all_single(self, output, input, output_split_sizes=None, input_split_sizes=None):
        w = self.world
        isz = list(input_split_sizes) if input_split_sizes is not None else [input.numel() // w] * w
        osz = list(output_split_sizes) if output_split_sizes is not None else [output.numel() // w] * w
        assert sum(isz) == input.numel() and sum(osz) == output.numel()
        ioff = [sum(isz[:p]) for p in range(w)]
        ins = [input[ioff[p]:ioff[p] + isz[p]] for p in range(w)]
        o, outs = 0, []
        for p in range(w):
            outs.append(output[o:o + osz[p]])
            o += osz[p]
        self.all_to_all(outs, ins)

    def send(self, t, dst):
        assert 0 <= dst < self.world and dst != self.get_rank()
        self._mail[(self.get_rank(), dst)].append(t.detach().clone())
        self._sync()
        self.cond.notify_all()

    def recv(self, t, src):
        assert 0 <= src < self.world and src != self.get_rank()
        box = self._mail[(src, self.get_rank())]
        self._wait(lambda: len(box) > 0, "recv from rank %d" % src)
        m = box.popleft()
        assert m.shape == t.shape and m.dtype == t.dtype, "recv: the message is not what the receiver expects"
        t.copy_(m)
        self._sync()

    # ------------------------------------------------------------------------------------------------ the machinery
    def _sync(self):
        if self.device_sync is not None:
            self.device_sync()

    def _fail(self, exc):
        if self.failure is None:
            self.failure = exc
        self.cond.notify_all()

    def _wait(self, ready, what):
        """give up the lock until ready(); raises when the run has failed or the time is up"""
        deadline = time.monotonic() + self.timeout
        while not ready():
            if self.failure is not None:
                raise Aborted("rank %d left %s: %r" % (self.get_rank(), what, self.failure))
            left = deadline - time.monotonic()
            if left <= 0 or self._returned:
                why = "a rank has returned" if self._returned else "no answer in %g s" % self.timeout
                e = TimeoutError("rank %d waits in %s: %s" % (self.get_rank(), what, why))
                self._fail(e)
                raise e
            self.cond.wait(min(left, 1.0))
        if self.failure is not None:
            raise Aborted("rank %d left %s: %r" % (self.get_rank(), what, self.failure))

    def _meet(self, name, payload=None):
        """rendezvous of all ranks in the collective `name`; returns the ranks' payloads by rank"""
        if self.failure is not None:
            raise Aborted("rank %d enters %s after %r" % (self.get_rank(), name, self.failure))
        r = self.get_rank()
        for p, s in enumerate(self._slots):
            if s is not None and s[0] != name:
                e = AssertionError("rank %d is in %s while rank %d is in %s" % (r, name, p, s[0]))
                self._fail(e)
                raise e
        assert self._slots[r] is None
        self._slots[r] = (name, payload)
        self._arrived += 1
        if self._arrived == self.world:
            self._result = [s[1] for s in self._slots]
            self._slots = [None] * self.world
            self._arrived = 0
            self._gen += 1
            self.log.append(name)
            self.cond.notify_all()
            return self._result
        gen = self._gen
        self._wait(lambda: self._gen != gen, name)
        # (the next rendezvous cannot complete before this rank has entered it: _result is still this one's)
        return self._result

    def run(self, target):
        """target(rank) on `world` threads, one running at a time; returns their results by rank, or raises the first
        real exception of any rank"""
        results = [None] * self.world

        def body(rank):
            with self.cond:
                self._tls.rank = rank
                try:
                    results[rank] = target(rank)
                except Aborted:
                    pass
                except BaseException as e:      # noqa: BLE001  (handed to the caller of run)
                    self._fail(e)
                finally:
                    self._returned += 1
                    self.cond.notify_all()

        threads = [threading.Thread(target=body, args=(r,), name="rank%d" % r) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if self.failure is not None:
            raise self.failure
        return results
