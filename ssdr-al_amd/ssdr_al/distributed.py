"""Exchange steps of the sharded path.  Rooms/tiles are sharded across ranks (one process per
GPU); the data path has no collective until selection, where three small exchanges make the result identical to a
single-process run over the union of the rooms:
  1. all-reduce of the 64-bin dominant-class histogram (class balance, sampler2.py:262-266),
  2. all-gather of the per-superpoint region uncertainties (global top-`batch` cut, sampler2.py:640, :533-552),
  3. all-gather of the candidates' propagated features before the replicated global FPS (fps_gcn_cpu.py:169-170).
torch.distributed backend "nccl" (= RCCL over xGMI) on GPUs, "gloo" in the CPU tests.

The collectives run directly on the library's device buffers (``DevArray.__cuda_array_interface__`` -> zero-copy torch
views) and are ordered on the caller's HIP stream (``torch.cuda.ExternalStream``): RCCL's stream waits for what the stream
holds so far, and the stream continues after the collective.  Nothing is staged through the host and the host never waits."""
import contextlib

import numpy as np

from . import _lib


class RawView:
    """``count`` elements at a raw device pointer, not owned: what a callback of the library is handed (``Trainer``'s exchange callback gets
    ``const float* d_send, float* d_recv, size_t count``).  Everything ``Comm.view`` needs of a DevArray, so the collectives take either."""

    def __init__(self, ptr, count, dtype=np.float32):
        self.ptr, self.shape, self.dtype = int(ptr), (int(count),), np.dtype(dtype)
        self.nbytes = int(count) * self.dtype.itemsize

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2, "strides": None}

    def host_view(self):
        """CPU logic build only (device memory == host memory there)"""
        import ctypes as C
        return np.frombuffer((C.c_char * self.nbytes).from_address(self.ptr), self.dtype)


class Comm:
    def __init__(self, dist, device):
        import torch
        self.dist, self.device, self.torch = dist, device, torch
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.cuda = str(device).startswith("cuda")
        self._ext = {}
        self._raw = {}

    def view(self, arr):
        """torch tensor sharing the memory of a DevArray or a RawView (no copy); a tensor (``raw_view``'s) is returned as it is."""
        if isinstance(arr, self.torch.Tensor):
            return arr
        if self.cuda:
            return self.torch.as_tensor(arr, device=self.device)
        return self.torch.from_numpy(arr.host_view())              # CPU logic build: device memory is host memory

    def raw_view(self, ptr, count, dtype=np.float32):
        """Zero-copy torch tensor over ``count`` elements at the raw device pointer ``ptr`` (``__cuda_array_interface__`` on the GPU, host memory on
        the CPU logic build); ``allreduce_sum_`` and ``allgather_`` take it wherever they take a DevArray.  The same (ptr, count) gives the same
        tensor again: a training step asks for the same few buffers ninety times."""
        key = (int(ptr), int(count), np.dtype(dtype).str)
        t = self._raw.get(key)
        if t is None:
            if len(self._raw) > 4096:
                self._raw.clear()
            t = self._raw[key] = self.view(RawView(ptr, count, dtype))
        return t

    def on_stream(self, stream):
        """Context in which collectives are ordered on the library stream `stream` (None = the library's main stream)."""
        if not self.cuda:
            return contextlib.nullcontext()                         # CPU logic build: every launch has finished when it returns
        import ctypes as C
        if stream is None:
            p = C.c_void_p()
            _lib.check(_lib.lib().ssdr_main_stream(C.byref(p)))
            stream = p.value
        key = int(stream)
        if key not in self._ext:
            self._ext[key] = self.torch.cuda.ExternalStream(key)
        return self.torch.cuda.stream(self._ext[key])

    def allreduce_sum_(self, arr, stream=None):
        """In-place sum over ranks of a DevArray (or a ``raw_view``)."""
        with self.on_stream(stream):
            self.dist.all_reduce(self.view(arr))

    def allgather_(self, arr_in, arr_out, stream=None):
        """arr_out [world, *arr_in.shape] <- arr_in of every rank, in rank order (equal sizes: callers pad).  DevArrays or ``raw_view``s."""
        with self.on_stream(stream):
            self.dist.all_gather_into_tensor(self.view(arr_out).reshape(-1), self.view(arr_in).reshape(-1)) if self.cuda else \
                self.dist.all_gather(list(self.view(arr_out).reshape(self.world, -1).unbind(0)), self.view(arr_in).reshape(-1))

    def allgather_host(self, a):
        """Setup-time helper (untimed): equal-shaped NumPy arrays of every rank, stacked in rank order."""
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        out = [self.torch.zeros_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        return np.stack([o.cpu().numpy() for o in out])
