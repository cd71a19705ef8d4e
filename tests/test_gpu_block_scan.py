"""uvc_launch_block_scan on its own: the one-block array scan behind the callable, MSI, read-profile and site reports (uvc_report_common.hip).  In place,
a[i] becomes the sum of a[0 .. i) and a[n], one element behind the input, the total.  The sizes cover a lane, a wave, a block of 1 024
threads and the carry between rounds; the values are signed (the read profile scans depth differences) and far from overflow.
The array lives in memory of the HIP runtime the library itself links, as in test_gpu_device_reads.py: torch's own copy of the runtime
finds no GPU once the library's has initialised it, so a torch tensor cannot be the buffer inside this suite."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 70001)
H2D, D2H = 1, 2


@pytest.fixture(scope="module")
def hip():
    dll = C.CDLL("libamdhip64.so")
    dll.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; dll.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; dll.hipFree.argtypes = [C.c_void_p]
    return dll


@pytest.mark.parametrize("n", SIZES)
def test_block_scan_is_numpys_exclusive_cumsum(gpu_lib, hip, n):
    fn = gpu_lib.dll.uvc_launch_block_scan
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_int, C.c_void_p]
    values = np.random.default_rng(n).integers(-1000, 1001, size=n).astype(np.int32)
    expected = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(values, out=expected[1:])
    host = np.append(values, np.int32(12345))   # (element n is an output: whatever it held must not show)
    got = np.empty(n + 1, dtype=np.int32)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), host.nbytes) == 0
    try:
        assert hip.hipMemcpy(p, host.ctypes.data, host.nbytes, H2D) == 0
        fn(p, n, None)   # the null stream: the copy back waits for it
        assert hip.hipMemcpy(got.ctypes.data, p, got.nbytes, D2H) == 0
    finally:
        hip.hipFree(p)
    assert np.array_equal(got.astype(np.int64), expected)
