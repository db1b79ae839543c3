"""parallel._Coll's interface over the threads of ONE process: the merge's choreography runs for several ranks without process groups
(CPU tensors with the NumPy twin of the kernels, or device tensors with the HIP kernels on one GPU).

thread_groups() makes every parallel.* function accept such a stand-in as its `group`, so the directory and general plans
(plan_merge_directory, merge_raw_sharded, merge_accumulator_sharded, ...) run unchanged for several ranks of one process."""
import contextlib
import os
import queue
import threading


class _NoLock:
    wait_s, held = 0.0, False


_ABORT = object()       # what a failing rank leaves in every point-to-point queue: a rank blocked in recv raises instead of waiting


class ThreadWorld:
    def __init__(self, ws, exclusive=False):
        self.ws, self.barrier, self.slots = ws, threading.Barrier(ws), [None] * ws
        # exclusive: only ONE rank computes at a time (a lock taken at start, dropped inside every collective), and the time spent
        # inside collectives incl. waiting for the lock is booked to comm_s -- a rank's wall time minus comm_s is then what it computes
        # on a GPU of its own (tools/probe_merge2.py)
        self.lock = threading.Lock() if exclusive else None
        # point-to-point: one FIFO per ordered (source, destination) pair
        self.fifo = {(s, d): queue.SimpleQueue() for s in range(ws) for d in range(ws)}

    def abort(self):
        """a rank failed: nobody may stay inside a collective or a recv"""
        self.barrier.abort()
        for q in self.fifo.values():
            q.put(_ABORT)


class ThreadColl:
    """parallel._Coll's interface over threads of one process (device or CPU tensors)"""

    class _Dist:
        class ReduceOp:
            MIN, MAX, SUM = "min", "max", "sum"

        @staticmethod
        def get_backend(group):
            return "threads"

    def __init__(self, world, rank):
        self.w, self.rank, self.ws = world, rank, world.ws
        self.comm_s, self.bytes_out, self.calls, self.gpu_lock, self.dist, self.group = 0.0, 0, 0, _NoLock(), self._Dist, None

    def _sync(self, t):
        if getattr(t, "is_cuda", False):
            import torch
            torch.cuda.synchronize()

    def _round(self, mine, take):
        import time
        self._sync(mine[0] if isinstance(mine, tuple) else mine)
        t0 = time.perf_counter()
        if self.w.lock is not None:
            self.w.lock.release()
        self.w.slots[self.rank] = mine
        self.w.barrier.wait()
        res = take(self.w.slots)
        self._sync(res[0] if isinstance(res, list) else res)
        self.w.barrier.wait()
        if self.w.lock is not None:
            self.w.lock.acquire()
        self.comm_s += time.perf_counter() - t0
        self.calls += 1
        return res

    def all_gather(self, t):
        return self._round(t, lambda s: [x.clone() for x in s])

    def all_gather_into(self, out, chunk):
        n = chunk.numel()

        def take(s):
            for r, c in enumerate(s):
                if r != self.rank:
                    out[r * n:(r + 1) * n].copy_(c)
            return out
        return self._round(chunk, take)

    def all_to_all(self, inp, in_splits, out_splits):
        import torch

        def take(s):
            parts = []
            for p, (t, ins) in enumerate(s):
                o = sum(ins[:self.rank])
                assert ins[self.rank] == out_splits[p], (p, self.rank, ins, out_splits)
                parts.append(t[o:o + ins[self.rank]])
            return torch.cat(parts) if parts else inp[:0]
        self.bytes_out += 8 * (sum(in_splits) - in_splits[self.rank])
        return self._round((inp, list(in_splits)), take)

    def all_to_all_start(self, inp, in_splits, out_splits, overlap=True):
        return ("done", self.all_to_all(inp, in_splits, out_splits))

    def all_to_all_finish(self, handle):
        return handle[1]

    @staticmethod
    def _op_name(op):
        """"min" / "max" / "sum" from a member of _Dist.ReduceOp or of torch.distributed.ReduceOp"""
        if isinstance(op, str):
            name = op
        else:
            import torch.distributed as dist
            name = next((k.lower() for k in ("MIN", "MAX", "SUM") if op == getattr(dist.ReduceOp, k)), None)
        if name not in ("min", "max", "sum"):
            raise ValueError(f"ThreadColl: reduce op {op!r} is not MIN, MAX or SUM")
        return name

    @staticmethod
    def _reduced(parts, name):
        """the ranks' tensors folded in rank order into a NEW tensor (a sum of floats is then the same on every rank and in every run)"""
        import torch
        acc = parts[0].clone()
        for x in parts[1:]:
            acc = torch.minimum(acc, x) if name == "min" else torch.maximum(acc, x) if name == "max" else acc + x
        return acc

    def all_reduce(self, t, op):
        """in place, like parallel._Coll.all_reduce; returns t"""
        name = self._op_name(op)
        res = self._round(t, lambda s: self._reduced(s, name))      # (the peers read t until the round's second barrier: copy after it)
        t.copy_(res)
        return t

    def reduce(self, t, dst, op):
        """in place on rank dst; the other ranks' tensors stay as they are.  Returns t"""
        name = self._op_name(op)
        res = self._round(t, lambda s: self._reduced(s, name) if self.rank == dst else t)
        if self.rank == dst:
            t.copy_(res)
        else:
            self.bytes_out += t.numel() * t.element_size()
        return t

    def broadcast(self, t, src):
        res = self._round(t, lambda s: t if self.rank == src else s[src].clone())
        if self.rank == src:
            self.bytes_out += t.numel() * t.element_size()
        else:
            t.copy_(res)
        return t

    def send(self, t, dst):
        """a copy of t joins the FIFO of (this rank -> dst); does not wait for the receiver"""
        import time
        t0 = time.perf_counter()
        c = t.clone()
        self._sync(c)
        self.w.fifo[(self.rank, dst)].put(c)
        self.comm_s += time.perf_counter() - t0
        self.bytes_out += t.numel() * t.element_size()
        self.calls += 1

    def recv(self, t, src):
        """blocks until rank src's next send to this rank arrives and copies it INTO t (which may be a slice of a larger tensor)"""
        import time
        t0 = time.perf_counter()
        self._sync(t)
        if self.w.lock is not None:
            self.w.lock.release()
        q = self.w.fifo[(src, self.rank)]
        got = q.get()
        if self.w.lock is not None:
            self.w.lock.acquire()
        if got is _ABORT:
            q.put(_ABORT)                       # (for this rank's later recvs, should it catch the error and go on)
            raise threading.BrokenBarrierError(f"rank {self.rank}: recv from rank {src} -- another rank failed")
        assert got.shape == t.shape and got.dtype == t.dtype, (self.rank, src, tuple(got.shape), tuple(t.shape), got.dtype, t.dtype)
        t.copy_(got)
        self._sync(t)
        self.comm_s += time.perf_counter() - t0
        self.calls += 1
        return t


def run_ranks(ws, fn, exclusive=False):
    world = ThreadWorld(ws, exclusive)
    out, errs = [None] * ws, []

    def body(r):
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.set_device(0)
            if world.lock is not None:
                world.lock.acquire()
            try:
                out[r] = fn(r, ThreadColl(world, r))
            finally:
                if world.lock is not None and world.lock.locked():
                    try:
                        world.lock.release()
                    except RuntimeError:
                        pass
        except BaseException as e:      # noqa: BLE001 -- a failing rank must not leave the others in a barrier or a recv
            errs.append(e)
            world.abort()
    th = [threading.Thread(target=body, args=(r,)) for r in range(ws)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        # the rank that failed first, not one of those it released (they only report the broken barrier)
        first = [e for e in errs if not isinstance(e, threading.BrokenBarrierError)]
        raise (first or errs)[0]
    return out


@contextlib.contextmanager
def thread_groups(**env):
    """While this context is open, `group=<ThreadColl>` carries a rank's collectives into every avlmaps_amd.parallel function
    unchanged: parallel._Coll(group) hands the stand-in back and parallel._dist_on(group) is true for it (and false without a
    group, as in a process without torch.distributed).  Keyword arguments are environment variables of the merge
    (AVLMAPS_MERGE_PLAN="directory", AVLMAPS_MERGE_KERNELS="0", ...; None removes one): the threads of a world share the process
    environment, so they are set HERE, around run_ranks, never inside a rank, and put back on the way out.

        with thread_groups(AVLMAPS_MERGE_PLAN="directory"):
            outs = run_ranks(ws, lambda r, coll: parallel.merge_accumulator_sharded(shards[r], group=coll))"""
    from avlmaps_amd import parallel
    saved = parallel._Coll, parallel._dist_on
    old = {k: os.environ.get(k) for k in env}
    parallel._Coll = lambda g=None: g
    parallel._dist_on = lambda g=None: g is not None
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        parallel._Coll, parallel._dist_on = saved
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
