"""The child process of tests/test_gpu_stream.py::test_bench_queue_count_in_a_fresh_process: the two passes of the pipelined stream
(tests/stream_tiles.py) under the GPU_MAX_HW_QUEUES its parent set, every tile's records and planes written to one .npz for the parent to
compare with the oracle.  No oracle here.  Usage: stream_worker.py OUT.npz"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np   # noqa: E402

from uvc_amd import region   # noqa: E402
import stream_tiles as st   # noqa: E402
from test_gpu_device_reads import DeviceColumns   # noqa: E402


def main():
    dst = sys.argv[1]
    os.environ.pop("UVCGPU_CHECK_PRESENCE", None)
    lib = region.gpu_lib()
    if lib.dll.uvcgpu_init(0) != 0:
        raise RuntimeError(lib.last_error())
    n = len(st.TILES)
    reads = [st.tile_reads(k) for k in range(n)]
    cols = [None if st.uses_host_reads(k) else DeviceColumns(reads[k]) for k in range(n)]
    t0 = time.perf_counter()
    out1 = st.run_stream(lib, reads, cols, release=True)
    out2 = st.run_stream(lib, reads, cols, release=False)
    dt = time.perf_counter() - t0
    for c in cols:
        if c is not None:
            c.free()
    z = dict(n_tiles=np.int64(n), queues=np.array(os.environ.get("GPU_MAX_HW_QUEUES", "")))
    for k in range(n):
        for f, v in out1[k]["records"].items():
            z["kept_%d_%s" % (k, f)] = v
        z["scored_%d" % k], z["cap_asked_%d" % k], z["enomem_%d" % k] = np.int64(out1[k]["scored"]), np.int64(out1[k]["cap_asked"]), np.bool_(out1[k]["enomem"])
        for f, v in out2[k]["records"].items():
            z["all_%d_%s" % (k, f)] = v
        for g, v in out2[k]["planes"].items():
            z["plane_%d_%s" % (k, g)] = v
        z["presence_%d" % k] = np.int64(out2[k]["presence"])
    np.savez(dst, **z)
    print("stream_worker: %d tiles twice in %.2f s" % (n, dt))


if __name__ == "__main__":
    main()
