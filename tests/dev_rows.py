"""device-resident rows for the -m gpu tests: the HIP runtime through ctypes, and DevRows -- rows in device memory at any pitch and
pointer offset, generated on the device (tests/test_gpu_refdigest.py) or copied from a host array (tests/test_gpu_seams.py)."""
import ctypes as C

import numpy as np

D2D, H2D, D2H = 3, 1, 2


def hip_lib():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def dev_alloc(hip, nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0, "hipMalloc(%d)" % nbytes
    return p


class DevRows:
    """the first n reads of the entry's stream in device memory at `pitch`, the first row `offset` bytes into the allocation.
    Pitches that are multiples of 16 come from mk_synth_rows_device; the others (and the offset ones) are the pitch-160 rows moved
    by hipMemcpy2D into a zeroed buffer -- 150 bases, '\\n', zeros, the bytes mk_synth_rows_host writes at that pitch, which the
    first and last rows are compared with.  DevRows.from_host: any host rows instead, copied as they are and read back."""

    def __init__(self, capi, hip, x, pitch, offset=0, n=None):
        self.hip, self.bufs = hip, []
        n = x["reads"] if n is None else n
        self.n, self.pitch = n, pitch
        try:
            if pitch % 16 == 0 and offset == 0:
                p = self._alloc(n * pitch)
                capi.synth_rows_device(0, None, x["seed"], 0, n, x["read_len"], pitch, p.value)
                self.ptr = p.value
            else:
                src = self._alloc(n * 160)
                capi.synth_rows_device(0, None, x["seed"], 0, n, x["read_len"], 160, src.value)
                dst = self._alloc(n * pitch + 16)
                assert hip.hipMemset(dst, 0, n * pitch + 16) == 0
                assert hip.hipMemcpy2D(dst.value + offset, pitch, src, 160, min(pitch, 160), n, D2D) == 0
                assert hip.hipDeviceSynchronize() == 0
                hip.hipFree(src)
                self.bufs.remove(src)
                self.ptr = dst.value + offset
            assert hip.hipDeviceSynchronize() == 0
            for first in (0, max(0, n - 1024)):  # the test's own plumbing: these are the generator's rows at this pitch
                m = min(1024, n - first)
                back = np.zeros(m * pitch, np.uint8)
                assert hip.hipMemcpy(back.ctypes.data, self.ptr + first * pitch, back.size, D2H) == 0
                assert np.array_equal(back, capi.synth_rows_host(x["seed"], first, m, x["read_len"], pitch)), "rows at pitch %d" % pitch
        except BaseException:
            self.free()
            raise

    @classmethod
    def from_host(cls, hip, rows, pitch, offset=0):
        """`rows` (host uint8, a whole number of rows of `pitch` bytes) in a zeroed device buffer, the first row `offset` bytes in"""
        self = cls.__new__(cls)
        self.hip, self.bufs = hip, []
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.size and rows.size % pitch == 0
        self.n, self.pitch = rows.size // pitch, pitch
        try:
            dst = self._alloc(rows.size + offset + 16)
            assert hip.hipMemset(dst, 0, rows.size + offset + 16) == 0
            assert hip.hipMemcpy(dst.value + offset, rows.ctypes.data, rows.size, H2D) == 0
            assert hip.hipDeviceSynchronize() == 0
            self.ptr = dst.value + offset
            back = np.zeros(rows.size, np.uint8)
            assert hip.hipMemcpy(back.ctypes.data, self.ptr, back.size, D2H) == 0
            assert np.array_equal(back, rows), "rows at pitch %d, pointer + %d" % (pitch, offset)
        except BaseException:
            self.free()
            raise
        return self

    def _alloc(self, nbytes):
        p = dev_alloc(self.hip, nbytes)
        self.bufs.append(p)
        return p

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []
