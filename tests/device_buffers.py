"""Device buffers and streams of a caller's own, for the tests that hand the library device pointers and a stream."""
import numpy as np


class Hip:
    """The few runtime calls a caller with buffers and a stream of its own makes (the runtime the library has loaded)."""
    H2D, D2H, D2D = 1, 2, 3

    def __init__(self):
        import ctypes as C

        self.C = C
        self.lib = C.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        self.lib.hipStreamDestroy.argtypes = [C.c_void_p]
        self.owned, self.streams = [], []

    def zeros(self, nbytes):
        p = self.C.c_void_p()
        assert self.lib.hipMalloc(self.C.byref(p), nbytes) == 0
        assert self.lib.hipMemset(p, 0, nbytes) == 0
        assert self.lib.hipDeviceSynchronize() == 0  # (the null stream's memset and the streams used below are not ordered)
        self.owned.append(p)
        return p.value

    def upload(self, a):
        """a buffer of its own holding the array `a`: in place when this returns"""
        a = np.ascontiguousarray(a)
        p = self.zeros(a.nbytes)
        assert self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, self.H2D) == 0
        assert self.lib.hipDeviceSynchronize() == 0
        return p

    def stream(self):
        s = self.C.c_void_p()
        assert self.lib.hipStreamCreateWithFlags(self.C.byref(s), 1) == 0  # hipStreamNonBlocking
        self.streams.append(s)
        return s.value

    def copy_on(self, stream, dst, src, nbytes):
        """device to device, enqueued on `stream`: no host sync"""
        assert self.lib.hipMemcpyAsync(dst, src, nbytes, self.D2D, stream) == 0

    def to_host(self, src, shape, dtype):
        a = np.zeros(shape, dtype=dtype)
        assert self.lib.hipMemcpy(a.ctypes.data, src, a.nbytes, self.D2H) == 0
        return a

    def close(self):
        for s in self.streams:
            self.lib.hipStreamDestroy(s)
        for p in self.owned:
            self.lib.hipFree(p)
