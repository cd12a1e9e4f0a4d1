"""The host <-> device boundary of training: the data-parallel context, the double-buffered batch feeder of fit and the loss read
back one step late."""
import os

import numpy as np


class DistContext:
    """one process per GPU; collectives are RCCL (torch.distributed backend 'nccl') over xGMI.
    Gradient buckets are all-reduced on a side HIP stream so that they overlap the rest of backward."""

    def __init__(self, sync_bn=True, n_buckets=4):
        import torch.distributed as dist
        self.dist = dist
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.sync_bn = sync_bn
        self.n_buckets = n_buckets
        self._streams = {}
        self._bn_pg = None

    def all_reduce(self, t):
        """blocking (stream-ordered) sum all-reduce: SyncBatchNorm statistics of the forward pass"""
        self.dist.all_reduce(t, group=self._bn_group())

    def _bn_group(self):
        # SyncBatchNorm gets its own communicator (own RCCL stream): a statistics all-reduce never queues behind
        # a gradient bucket that is still on the wire.  DL3P_ONE_COMM=1 keeps everything on the default communicator
        # (one of the switches watchdog.FirstStepsGuard names when the first steps of a multi-rank job hang)
        if os.environ.get('DL3P_ONE_COMM', '0') not in ('', '0'):
            return None
        if self._bn_pg is None and self.dist.is_initialized() and self.dist.get_backend() == 'nccl':
            self._bn_pg = self.dist.new_group(backend='nccl')
        return self._bn_pg

    def broadcast(self, t, src=0):
        self.dist.broadcast(t, src)

    def _side(self, which):
        import torch
        if self._streams.get(which) is None:
            self._streams[which] = torch.cuda.Stream()
        return self._streams[which]

    def all_reduce_async(self, t):
        """sum all-reduce of a gradient bucket, ordered after everything already queued on the
        compute stream but running beside what is queued later"""
        import torch
        if not t.is_cuda:
            self.dist.all_reduce(t)
            return
        side = self._side('grad')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.dist.all_reduce(t)

    def wait_all(self):
        import torch
        if self._streams.get('grad') is not None:
            torch.cuda.current_stream().wait_stream(self._streams['grad'])

    def bn_all_reduce_begin(self, t):
        """SyncBatchNorm backward sums: start the all-reduce beside the compute stream (the deferred weight
        gradient of the previous layer runs meanwhile) ..."""
        import torch
        if not t.is_cuda:
            self.dist.all_reduce(t)
            return
        side = self._side('bn')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.dist.all_reduce(t, group=self._bn_group())

    def bn_all_reduce_end(self):
        """... and make the compute stream wait for it"""
        import torch
        if self._streams.get('bn') is not None:
            torch.cuda.current_stream().wait_stream(self._streams['bn'])


class StagedBatch:
    """a batch on its way to the device (BatchFeeder.put): device tensors with their host shapes, the staging slot they live in"""
    def __init__(self, slot, x, y, sample_weight):
        self.slot, self.x, self.y, self.sample_weight = slot, x, y, sample_weight


class BatchFeeder:
    """fit_generator's host -> device boundary (train.py:177-187 feeds numpy batches): TWO sets of pinned host buffers and device
    staging buffers and a copy stream, so that batch k + 1 crosses PCIe while the device runs step k.  put() copies the arrays into
    pinned memory (CPU) and starts the DMA on the copy stream; the consumer makes the compute stream wait for that DMA
    (consume), enqueues the step (whose first kernels read the staging buffers: uint8 -> float normalisation, label
    preparation) and releases the slot (release) -- the copy stream does not overwrite a slot before its last consumer ran."""
    def __init__(self, device='cuda'):
        import torch
        self.dev = device
        self.stream = torch.cuda.Stream()
        self.bufs = [{}, {}]
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]
        self.free = [None, None]
        self.k = 0

    def _move(self, slot, name, a):
        import torch
        t = torch.as_tensor(a)
        shape = tuple(t.shape)
        if t.dtype not in (torch.uint8, torch.float32):
            t = t.to(torch.float32)
        t = t.reshape(-1)
        pair = self.bufs[slot].get(name)
        if pair is None or pair[0].numel() != t.numel() or pair[0].dtype != t.dtype:
            pair = self.bufs[slot][name] = (torch.empty(t.numel(), dtype=t.dtype, pin_memory=True),
                                            torch.empty(t.numel(), dtype=t.dtype, device=self.dev))
        host, dev = pair
        # one thread's memcpy (0.5 ms for 12.6 MB).  Tensor.copy_ spreads it over every core of the host and the OpenMP workers then
        # spin for their block time: on the 256-thread GPU box that starved the HIP runtime's own thread and a staged step took
        # 35 ms instead of 12 (scripts/micro/feed_dbg.py)
        np.copyto(host.numpy(), t.numpy())
        with torch.cuda.stream(self.stream):
            dev.copy_(host, non_blocking=True)
        return dev.view(shape)

    def put(self, x, y=None, sample_weight=None):
        slot = self.k & 1
        self.k += 1
        if getattr(x, 'is_cuda', False):
            # a batch made on the device (data.SegmentationGenerator, output='device'): nothing crosses PCIe, no pinned copy; the step
            # waits for the work that built it, which is whatever the current stream holds now
            import torch
            self.ready[slot].record(torch.cuda.current_stream())
            return StagedBatch(slot, x, y, sample_weight)
        self.ready[slot].synchronize()          # (the DMA that last read this slot's pinned buffers; long done)
        if self.free[slot] is not None:
            self.stream.wait_event(self.free[slot])
        sw = sample_weight
        out = StagedBatch(slot, self._move(slot, 'x', x), None if y is None else self._move(slot, 'y', y),
                          sw if (sw is None or isinstance(sw, str)) else self._move(slot, 'sw', sw))
        self.ready[slot].record(self.stream)
        return out

    def consume(self, staged):
        import torch
        torch.cuda.current_stream().wait_event(self.ready[staged.slot])

    def release(self, staged):
        import torch
        ev = self.free[staged.slot] = self.free[staged.slot] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream())


class LateScalar:
    """a device scalar read back one step late: an asynchronous copy into pinned memory behind the step that produced it, the value
    taken when the NEXT step has been enqueued (fit's loss: the device never waits for the host to look at a number)"""
    def __init__(self):
        import torch
        self.host = [torch.zeros(1, dtype=torch.float32, pin_memory=True) for _ in range(2)]
        self.evt = [torch.cuda.Event(), torch.cuda.Event()]
        self.k = 0

    def post(self, dev_scalar):
        i = self.k & 1
        self.k += 1
        self.host[i].copy_(dev_scalar.reshape(-1)[:1], non_blocking=True)
        self.evt[i].record()
        return i

    def value(self, i):
        self.evt[i].synchronize()
        return float(self.host[i][0])
