"""The two networks' HIP streams ("lanes") and every dependency between them and the caller's stream.

The two networks of a CPS pair are independent until the loss: each runs on its own stream, so that one network's small,
latency-bound kernels hide under the other's large ones.  `Lanes` owns those streams and the optional
weight-gradient side streams, and is the only place of the trainer that switches streams or orders one after another:
what crosses between the caller's stream and the lanes goes through one of the calls below, which names the edge.  With
the lanes off (a CPU device, CPSConfig.two_streams = False, VQSEG_TWO_STREAMS=0) every call does nothing and `on()` is a
null context: the same code then enqueues the same work, in the same order, on the caller's stream.
"""
import contextlib

import torch

from . import nnf


class Lanes:
    def __init__(self, device=None, n: int = 2, enabled: bool = False, wgrad_side: bool = False, prio: int = 0):
        """`prio` (A/B, py_stream_prio): 1 = the lanes above the weight-gradient side streams, 2 = the reverse."""
        self.enabled = enabled                  # assignable on a live object; streams are made only where it starts out True
        self.streams = [torch.cuda.Stream(device, priority=-1 if prio == 1 else 0) for _ in range(n)] if enabled else []
        # weight-gradient kernels (+ their slab sums) run on a side stream per network (nnf.WGRAD_SIDE_STREAMS): nothing later in
        # backward depends on them, so they fill the chip under the latency-bound links of the main chain.  They add into the
        # gradient buckets, so they are producer streams of the buckets and are waited for before the optimiser step.
        self.sides = [torch.cuda.Stream(device, priority=-1 if prio == 2 else 0) for _ in range(n)] if enabled and wgrad_side else []
        self._pending = set()                   # lanes holding work the caller's stream has not waited for yet

    def producers(self, k):
        """the streams that write network k's gradients (GradBuckets.producer_streams)"""
        return [s[k] for s in (self.streams, self.sides) if s]

    @contextlib.contextmanager
    def on(self, k, amp=None):
        """what runs inside goes to network k's lane, under autocast to `amp` if given"""
        with contextlib.ExitStack() as ctx:
            if self.enabled:
                ctx.enter_context(torch.cuda.stream(self.streams[k]))
            if amp is not None:
                ctx.enter_context(torch.autocast("cuda", dtype=amp))
            yield

    def fork(self, *ks, sides=False):
        """lanes `ks` (default: all) wait for what the caller's stream holds so far; `sides`: and for their weight-gradient
        side streams (after a backward pass)"""
        if not self.enabled:
            return
        main = torch.cuda.current_stream()
        for k in ks or range(len(self.streams)):
            self.streams[k].wait_stream(main)
            if sides and self.sides:
                self.streams[k].wait_stream(self.sides[k])
            self._pending.add(self.streams[k])

    def join(self, *ks, sides=False):
        """the caller's stream waits for everything queued on the lanes since they forked; `ks` / `sides`: and for whatever
        those lanes / all side streams hold (a backward pass ran there through autograd, without a fork())"""
        if self.enabled:
            self._pending.update(self.streams[k] for k in ks)
            self._pending.update(self.sides if sides else ())
        if self._pending:
            main = torch.cuda.current_stream()
            for s_ in self._pending:
                main.wait_stream(s_)
            self._pending.clear()

    def share(self, t):
        """`t` was made on the caller's stream and is read on every lane (ordered by a fork()): the allocator is told"""
        if self.enabled and t.is_cuda:
            for s_ in self.streams:
                t.record_stream(s_)

    def to_caller(self, *tensors):
        """these (tensors, or tuples of them) were made on a lane and are read on the caller's stream (ordered by a join())"""
        if not self.enabled:
            return
        main = torch.cuda.current_stream()
        for t in tensors:
            for x in (t if isinstance(t, (tuple, list)) else (t,)):
                if torch.is_tensor(x) and x.is_cuda:
                    x.record_stream(main)

    def mark(self):
        """an event on each lane, for an exchange() of what the lanes hold NOW that is carried out later"""
        return tuple(s_.record_event() for s_ in self.streams) if self.enabled else None

    def exchange(self, t_from_0, t_from_1, marks=None):
        """lane 0 may read t_from_1 (made on lane 1) and the reverse: one event each way, as of `marks` or of now"""
        if self.enabled:
            e0, e1 = marks or self.mark()
            self.streams[0].wait_event(e1)
            self.streams[1].wait_event(e0)
            t_from_1.record_stream(self.streams[0])
            t_from_0.record_stream(self.streams[1])

    def hold(self, k):
        """lane k waits for what the other lane holds so far (the VQ phases run one after the other)"""
        if self.enabled:
            self.streams[k].wait_event(self.streams[1 - k].record_event())

    def wgrad_sides(self, on: bool):
        """register / unregister the weight-gradient side streams with nnf for the duration of a backward pass"""
        for s_, w_ in zip(self.streams, self.sides):
            if on and self.enabled:
                nnf.WGRAD_SIDE_STREAMS[s_.cuda_stream] = w_
            else:
                nnf.WGRAD_SIDE_STREAMS.pop(s_.cuda_stream, None)


OFF = Lanes()                                   # no lanes: every call is a no-op (what runs "on" them runs on the caller's stream)
