"""hipGraph replay for launch-bound fixed-shape sub-networks (VAE decode, CLIP text encoder): ~100-250 launches of 5-30 us
kernels whose Python / ctypes launch cost (~10 us each) would otherwise exceed the kernel time. One captured graph per input
signature; inputs are copied into static buffers, the result is returned as a fresh tensor (the static output is overwritten by the
next replay). SPIDER_NO_GRAPHS=1 runs everything eagerly."""
from __future__ import annotations

import contextlib
import gc
import os
from typing import Callable, Dict, Tuple

import torch

_DISABLED = os.environ.get("SPIDER_NO_GRAPHS", "0") == "1"


@contextlib.contextmanager
def capture(graph: "torch.cuda.CUDAGraph", **kw):
    """`torch.cuda.graph(graph)` with Python's cyclic garbage collected first and the collector off while the stream captures.
    An engine dropped by its owner can wait for the collector (the GraphRunner lambdas of the CLIP / VAE engines close over their
    engine), and with it its captured graphs; torch.cuda.graph no longer collects on entry. A collection that starts inside a
    capture then destroys those graphs there, the ROCm build of torch synchronises the device in that destructor, a device
    synchronisation is illegal while a stream captures, and the error leaves a destructor: the process aborts."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            yield
    finally:
        if was_enabled:
            gc.enable()


class GraphRunner:
    def __init__(self, fn: Callable[..., torch.Tensor], max_entries: int = 8):
        self.fn, self.max_entries = fn, max_entries
        self.cache: Dict[Tuple, tuple] = {}

    def __call__(self, *tensors: torch.Tensor, key=()) -> torch.Tensor:
        if _DISABLED or not tensors[0].is_cuda or torch.cuda.is_current_stream_capturing():
            return self.fn(*tensors)
        k = (tuple((tuple(t.shape), t.dtype) for t in tensors), key)
        ent = self.cache.get(k)
        if ent is None:
            if len(self.cache) >= self.max_entries:
                self.cache.pop(next(iter(self.cache)))
            static_in = [t.clone() for t in tensors]
            dev = tensors[0].device
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                self.fn(*static_in)                      # warm-up outside capture (lazy allocations, first-use setup)
            torch.cuda.current_stream(dev).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with capture(g):
                out = self.fn(*static_in)
            ent = (g, static_in, out)
            self.cache[k] = ent
        g, static_in, out = ent
        for dst, src in zip(static_in, tensors):
            dst.copy_(src)
        g.replay()
        return out.clone() if torch.is_tensor(out) else tuple(o.clone() for o in out)      # a tuple of tensors: the safety checker
