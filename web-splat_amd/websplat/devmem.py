"""Owners of the binding's device memory: DeviceArray (one allocation), ViewportPlanes (named planes of one viewport) and
staged() (a temporary device copy of a host array).  Pure Python + numpy: the device is reached only through a context's
malloc / free / upload / download / sync, so everything here runs on the CPU against a stand-in context."""
import contextlib

import numpy as np


class DeviceArray:
    """One device allocation of `shape` x `dtype`, never smaller than one element (a zero-sized viewport still reaches the
    library, which reports the state error).  free() is idempotent; as a context manager it frees on exit."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.pitch = int(np.prod(self.shape[1:], dtype=np.int64)) * self.dtype.itemsize  # bytes of one row
        self.ptr = ctx.malloc(max(self.nbytes, self.dtype.itemsize))

    @classmethod
    def from_host(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        d = cls(ctx, arr.shape, arr.dtype)
        try:
            d.upload(arr)
        except BaseException:
            d.free()
            raise
        return d

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError(f"DeviceArray.upload: {arr.nbytes} bytes into an allocation of {self.nbytes}")
        self.ctx.upload(self.ptr, arr, stream)

    def download(self):
        return self.ctx.download(self.ptr, self.shape, self.dtype)

    def free(self):
        ptr, self.ptr = self.ptr, None
        if ptr is not None:
            self.ctx.free(ptr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class ViewportPlanes:
    """Named DeviceArrays that all belong to one (w, h): allocated on first use, kept while the viewport stands, let go
    together when fit() sees another one.  A name is bound only to a live allocation, whatever raises in between."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.viewport = None
        self._planes = {}

    def fit(self, w, h):
        if self.viewport != (w, h):
            self.free()
            self.viewport = (w, h)

    def plane(self, name, dtype, channels=None):
        p = self._planes.get(name)
        if p is None:
            w, h = self.viewport
            p = DeviceArray(self.ctx, (h, w) if channels is None else (h, w, channels), dtype)
            self._planes[name] = p
        return p

    def get(self, name):
        return self._planes.get(name)

    def free(self):
        self.viewport = None
        while self._planes:
            self._planes.popitem()[1].free()


@contextlib.contextmanager
def staged(ctx, array, stream, min_bytes=4):
    """Yields the device pointer of a temporary copy of `array`; behind the body, also when it raises: wait for `stream`,
    free the copy.  array None: yields None, nothing is allocated or waited for."""
    if array is None:
        yield None
        return
    d = ctx.malloc(max(array.nbytes, min_bytes))
    try:
        ctx.upload(d, array)
        yield d
    finally:
        ctx.sync(stream)
        ctx.free(d)
