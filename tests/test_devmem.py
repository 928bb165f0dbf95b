"""websplat.devmem on the CPU: DeviceArray, ViewportPlanes and staged() against a stand-in context that keeps the books --
which blocks live, what was freed twice, what was waited for before what."""
import numpy as np
import pytest

from websplat import devmem
from websplat.devmem import DeviceArray, ViewportPlanes, staged


class FakeContext:
    """malloc hands out fresh integers, free refuses what is not live, upload / download keep the bytes, sync records the
    stream; fail_malloc(k) makes the k-th malloc from now raise, fail_upload() the next upload."""

    def __init__(self):
        self.live = {}      # ptr -> nbytes
        self.mem = {}       # ptr -> bytes
        self.log = []       # ("malloc", ptr) | ("free", ptr) | ("sync", stream) | ("upload", ptr, stream)
        self._next = 0x1000
        self._fail_in = 0
        self._fail_upload = False

    def fail_malloc(self, k=1):
        self._fail_in = k

    def fail_upload(self):
        self._fail_upload = True

    def mallocs(self):
        return sum(1 for e in self.log if e[0] == "malloc")

    def malloc(self, nbytes):
        if self._fail_in:
            self._fail_in -= 1
            if not self._fail_in:
                raise MemoryError("out of device memory")
        assert nbytes > 0
        self._next += 0x1000
        self.live[self._next] = int(nbytes)
        self.log.append(("malloc", self._next))
        return self._next

    def free(self, ptr):
        if ptr not in self.live:
            raise RuntimeError(f"free of {ptr!r}: unknown or already freed")
        del self.live[ptr]
        self.mem.pop(ptr, None)
        self.log.append(("free", ptr))

    def upload(self, ptr, arr, stream=None):
        if self._fail_upload:
            self._fail_upload = False
            raise RuntimeError("upload failed")
        raw = np.ascontiguousarray(arr).tobytes()
        assert len(raw) <= self.live[ptr]
        self.mem[ptr] = raw
        self.log.append(("upload", ptr, stream))

    def download(self, ptr, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.frombuffer(self.mem.get(ptr, bytes(self.live[ptr]))[:n], dtype=dtype).reshape(shape).copy()

    def sync(self, stream=None):
        self.log.append(("sync", stream))


@pytest.fixture
def fake():
    return FakeContext()


def test_module_is_pure_python():
    assert not {"ctypes", "C", "L", "lib", "_lib"} & set(vars(devmem))


# DeviceArray ---------------------------------------------------------------------------------------------------------------
def test_device_array_round_trip(fake):
    src = (np.arange(5 * 7 * 4, dtype=np.float32) * 0.5 - 3).reshape(5, 7, 4).astype(np.float16)
    d = DeviceArray.from_host(fake, src)
    assert d.shape == (5, 7, 4) and d.dtype == np.float16 and d.nbytes == src.nbytes and fake.live[d.ptr] == src.nbytes
    got = d.download()
    assert got.shape == src.shape and got.dtype == src.dtype and got.tobytes() == src.tobytes()
    d.free()
    assert not fake.live


def test_device_array_pitch(fake):
    assert DeviceArray(fake, (48, 64), np.float32).pitch == 64 * 4
    assert DeviceArray(fake, (48, 64, 4), np.float16).pitch == 64 * 4 * 2
    assert DeviceArray(fake, (48, 64, 4), np.uint8).pitch == 64 * 4
    assert DeviceArray(fake, (9,), np.uint32).pitch == 4


@pytest.mark.parametrize("shape, dtype", [((0, 0, 4), np.float32), ((0,), np.uint32), ((0, 5), np.float16)])
def test_device_array_zero_elements_still_allocates_one(fake, shape, dtype):
    d = DeviceArray(fake, shape, dtype)
    assert d.nbytes == 0 and d.ptr is not None and fake.live[d.ptr] == np.dtype(dtype).itemsize
    assert d.download().shape == shape


def test_device_array_free_is_idempotent(fake):
    d = DeviceArray(fake, (4, 4), np.float32)
    d.free()
    assert d.ptr is None
    d.free()  # (the stand-in raises on a second free of the pointer)
    assert [e[0] for e in fake.log] == ["malloc", "free"]


def test_device_array_with_block_frees_on_exception(fake):
    with pytest.raises(KeyError):
        with DeviceArray(fake, (4, 4), np.float32) as d:
            assert d.ptr in fake.live
            raise KeyError("body")
    assert d.ptr is None and not fake.live


def test_device_array_from_host_failed_upload_leaves_nothing(fake):
    fake.fail_upload()
    with pytest.raises(RuntimeError, match="upload failed"):
        DeviceArray.from_host(fake, np.zeros((3, 3), np.float32))
    assert not fake.live and fake.mallocs() == 1


def test_device_array_upload_goes_on_the_stream_and_fits(fake):
    d = DeviceArray(fake, (2, 3), np.float32)
    d.upload(np.ones((2, 3), np.float32), stream=77)
    assert fake.log[-1] == ("upload", d.ptr, 77)
    with pytest.raises(ValueError):
        d.upload(np.ones((2, 4), np.float32))


# ViewportPlanes ------------------------------------------------------------------------------------------------------------
def test_planes_same_viewport_same_name_same_pointer(fake):
    s = ViewportPlanes(fake)
    s.fit(64, 48)
    a = s.plane("depth", np.float32)
    assert a.shape == (48, 64) and s.get("depth") is a and s.get("alpha") is None
    s.fit(64, 48)
    assert s.plane("depth", np.float32) is a and a.ptr in fake.live and fake.mallocs() == 1


def test_planes_are_keyed_by_shape_not_size(fake):
    s = ViewportPlanes(fake)
    s.fit(64, 48)
    old = [s.plane("target", np.float32, 4), s.plane("depth", np.float32)]
    old_ptrs = [p.ptr for p in old]
    s.fit(48, 64)  # (the same byte counts)
    assert s.get("target") is None and s.get("depth") is None and not fake.live and all(p.ptr is None for p in old)
    new = s.plane("target", np.float32, 4)
    assert new.shape == (64, 48, 4) and new.nbytes == 64 * 48 * 16 and new.ptr not in old_ptrs


def test_planes_second_name_allocates_only_itself(fake):
    s = ViewportPlanes(fake)
    s.fit(64, 48)
    a = s.plane(0, np.float32)
    w = s.plane("winner", np.uint32)
    assert fake.mallocs() == 2 and w.dtype == np.uint32 and w.ptr != a.ptr and s.plane(0, np.float32) is a
    assert fake.mallocs() == 2


def test_planes_free_leaves_nothing(fake):
    s = ViewportPlanes(fake)
    s.fit(64, 48)
    for name in ("depth", "median_depth", "alpha"):
        s.plane(name, np.float32)
    assert len(fake.live) == 3
    s.free()
    assert not fake.live and s.viewport is None and s.get("depth") is None
    s.free()
    s.fit(64, 48)  # (a freed set fits again: fresh planes)
    s.plane("depth", np.float32)
    assert len(fake.live) == 1


def test_planes_failed_reallocation_leaves_no_dangling_target(fake):
    """The defect the three open-coded target blocks had: free, then a malloc that raises, kept the freed address under the
    old shape -- the next frame drew into it and close() freed it again."""
    s = ViewportPlanes(fake)
    s.fit(64, 48)
    s.plane("target", np.float32, 4)
    s.fit(96, 48)
    fake.fail_malloc()
    with pytest.raises(MemoryError):
        s.plane("target", np.float32, 4)
    assert s.get("target") is None and not fake.live
    t = s.plane("target", np.float32, 4)
    assert t.shape == (48, 96, 4) and list(fake.live) == [t.ptr]
    frees = sum(1 for e in fake.log if e[0] == "free")
    s.free()  # (the stand-in raises on a double free)
    assert sum(1 for e in fake.log if e[0] == "free") == frees + 1 and not fake.live


def test_planes_failed_allocation_keeps_the_others(fake):
    s = ViewportPlanes(fake)
    s.fit(64, 48)
    a = s.plane("depth", np.float32)
    fake.fail_malloc()
    with pytest.raises(MemoryError):
        s.plane("alpha", np.float32)
    assert s.get("alpha") is None and s.get("depth") is a and list(fake.live) == [a.ptr]
    s.free()
    assert not fake.live


# staged --------------------------------------------------------------------------------------------------------------------
def test_staged_syncs_the_stream_then_frees(fake):
    src = np.arange(6, dtype=np.float32)
    with staged(fake, src, 5) as d:
        assert fake.mem[d] == src.tobytes() and fake.live[d] == src.nbytes
    assert fake.log[-2:] == [("sync", 5), ("free", d)] and not fake.live


def test_staged_syncs_and_frees_when_the_body_raises(fake):
    with pytest.raises(KeyError):
        with staged(fake, np.zeros(3, np.float32), 9) as d:
            raise KeyError("body")
    assert fake.log[-2:] == [("sync", 9), ("free", d)] and not fake.live


def test_staged_min_bytes(fake):
    with staged(fake, np.zeros((0, 4), np.float32), None) as d:
        assert fake.live[d] == 4
    with staged(fake, np.zeros((0, 4), np.float32), None, min_bytes=16) as d:
        assert fake.live[d] == 16


def test_staged_none_does_nothing(fake):
    with staged(fake, None, 5) as d:
        assert d is None
    assert fake.log == []
