"""The production schedule against the oracle.  Every other GPU test runs with the suite's validator switch (UVCGPU_CHECK_PRESENCE, set in
tests/conftest.py), which ends each accumulate with a host sync: every score there starts on an idle device.  bench.py and uvc1-mi355x
never sync between accumulate and score, so these tests turn the switch off for themselves and check what only that schedule does:

- the side-stream work of an accumulate (side / side3 and their events) still running when the next call on the handle or on another
  handle is enqueued -- A, C, D;
- the zero fill of release_state on the side stream under the D2H of the records, and the next accumulate's wait on it (e_join through
  state_zeroed) -- A (pass 1), B, C, D;
- the d_dirty memset of the zero fill against the marks k_enum sets -- A (pass 2: the selective fill in front of an accumulate), B;
- a release followed by a rebind to another length (configure_region's carry-over of the zeroed slab, or the full fill) -- A, B;
- bench.py's GPU_MAX_HW_QUEUES=16, where handles' streams run on queues of their own -- D.

Records are compared with the tolerance classes of tests/test_gpu_parity.py, planes bit for bit."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from uvc_amd import region, synth
from util import INT_GROUPS, kept_groups, presence_violations, run_region
from test_gpu_parity import compare_records
from test_gpu_device_reads import DeviceColumns
import stream_tiles as st

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GROW = dict(region_len=16385, depth=100, seed=611, indel_every=300, snv_every=200)   # longer than any tile of the set: the handle reallocates


@pytest.fixture(autouse=True)
def validator_off(monkeypatch):
    monkeypatch.delenv("UVCGPU_CHECK_PRESENCE", raising=False)   # region.py reads it on every accumulate


def _oracle_one(lib, reads):
    R = run_region(lib, reads)
    out = dict(full=R.score(), all=R.score(all_out=True), planes={g: R.fetch(g) for g in INT_GROUPS})
    R.close()
    return out


@pytest.fixture(scope="module")
def stream_data(oracle_lib):
    """The reads of every tile and the oracle's outputs for them (default-gate and all-out records, the 14 plane groups); one thread per
    tile, as the oracle_runs fixture of tests/test_gpu_large.py."""
    t0 = time.perf_counter()
    reads = [st.tile_reads(k) for k in range(len(st.TILES))] + [synth.generate_region(tid=19, beg=3_000_000, **GROW)]
    want, errs = [None] * len(reads), []

    def work(k):
        try:
            want[k] = _oracle_one(oracle_lib, reads[k])
        except Exception as e:   # noqa: BLE001
            errs.append((k, e))
    th = [threading.Thread(target=work, args=(k,)) for k in range(len(reads))]
    for t in th: t.start()
    for t in th: t.join()
    assert not errs, errs
    print("oracle of %d tiles: %.1f s" % (len(reads), time.perf_counter() - t0))
    return reads, want


def plane_diff(want, got):
    """{group: (n_mismatching_cells, first few (cell, oracle, gpu))} of the groups that differ (as util.diff_groups)."""
    bad = {}
    for g in INT_GROUPS:
        a, b = want[g], got[g]
        if not np.array_equal(a, b):
            idx = np.argwhere(a != b)
            bad[g] = (len(idx), [(tuple(int(v) for v in i), int(a[tuple(i)]), int(b[tuple(i)])) for i in idx[:8]])
    return bad


def assert_planes(want, got, what):
    bad = plane_diff(want, got)
    assert not bad, what + ": " + "\n".join("%s: %d cells differ, e.g. %s" % (g, v[0], v[1]) for g, v in bad.items())


def device_columns(reads):
    """Device columns of the tiles that do not come from the host, made before any stream starts (the copies in are synchronous)."""
    return [None if st.uses_host_reads(k) else DeviceColumns(reads[k]) for k in range(len(st.TILES))]


def check_kept_stream(out, want, label):
    """Pass 1 of a stream: every tile's kept-only records equal the oracle's default-gate records reduced to the kept groups.  -> (tiles that
    took the library's kept-only retry, tiles that took region.py's ENOMEM retry)."""
    dev_cap = [0] * st.N_HANDLES
    n_retry = n_enomem = 0
    for k, res in enumerate(out):
        full = want[k]["full"]
        _, expect = kept_groups(full)
        try:
            compare_records(expect, res["records"])
        except AssertionError as e:
            raise AssertionError("%s, tile %d (handle %d): %s" % (label, k, k % st.N_HANDLES, e)) from None
        assert res["scored"] == len(full["refpos"]), (label, k, res["scored"], len(full["refpos"]))
        retried, dev_cap[k % st.N_HANDLES] = st.library_retried(st.TILES[k]["region_len"] + 1, res["scored"], res["cap_asked"], dev_cap[k % st.N_HANDLES])
        n_retry += retried
        n_enomem += res["enomem"]
    return n_retry, n_enomem


def check_plane_stream(out, want, label):
    """Pass 2 of a stream: all-out records, the planes bit for bit, and no cell against the presence statement."""
    for k, res in enumerate(out):
        assert_planes(want[k]["planes"], res["planes"], "%s, tile %d (handle %d)" % (label, k, k % st.N_HANDLES))
        assert res["presence"] == 0, (label, k, res["presence"])
        try:
            compare_records(want[k]["all"], res["records"])
        except AssertionError as e:
            raise AssertionError("%s, tile %d (handle %d): %s" % (label, k, k % st.N_HANDLES, e)) from None


def test_bench_shaped_pipeline(stream_data, gpu_lib):
    """A: bench.py's stream (Leg.prepare / Leg.finish) over three handles, tiles prepared two ahead; then the same stream with all-out
    scoring that keeps the planes."""
    reads, want = stream_data
    n = len(st.TILES)
    cols = device_columns(reads)
    try:
        t0 = time.perf_counter()
        out1 = st.run_stream(gpu_lib, reads[:n], cols, release=True)
        out2 = st.run_stream(gpu_lib, reads[:n], cols, release=False)
        dt = time.perf_counter() - t0
    finally:
        for c in cols:
            if c is not None:
                c.free()
    n_retry, n_enomem = check_kept_stream(out1, want, "kept-only stream")
    check_plane_stream(out2, want, "all-out stream")
    print("stream A: %d tiles twice in %.2f s, %d kept-only retries in the library, %d ENOMEM retries in region.py" % (n, dt, n_retry, n_enomem))
    assert n_retry >= 2 and n_enomem >= 2     # both retry paths ran inside the stream


def test_release_then_rebind_to_other_lengths(stream_data, gpu_lib):
    """B: one handle walks every branch of configure_region / zero_state behind a release, starting from a large, variant-dense tile (a cell
    it leaves behind is non-zero).  Steps that release compare records (the planes are gone); the others planes and records."""
    reads, want = stream_data
    G = len(reads) - 1
    # (tile, release at its score, what the accumulate in front of the score does)
    steps = [(0, False, "first use: full fill"),
             (3, True, "shorter, no release before: full fill of the short layout only"),
             (6, False, "longer within the size after a release: state_bytes > zeroed_bytes, full fill"),
             (9, True, "equal length without release: selective fill"),
             (2, False, "shorter after a release: the zeroed slab is carried over"),
             (4, True, "equal length without release: selective fill"),
             (2, False, "equal length after a release: the zeroed slab is used as it is"),
             (G, True, "longer than the handle's size: reallocation"),
             (7, False, "shorter after a release into the new slab: carried over")]
    R = None
    for i, (k, release, what) in enumerate(steps):
        t = reads[k]
        if R is None:
            R = region.Region(gpu_lib, region.default_params(gpu_lib), t["tid"], t["beg"], t["end"], t["refseq"])
        else:
            R.reset(t["tid"], t["beg"], t["end"], t["refseq"])
        R.set_reads(t)
        R.accumulate()
        label = "step %d (tile %d, %d positions, %s)" % (i, k, R.npos, what)
        if release:
            rg = R.score(release_state=True)
            for call in (lambda: R.fetch("SEG32"), lambda: R.score()):
                with pytest.raises(region.UvcError) as e:
                    call()
                assert e.value.code == -5, label
        else:
            got = {g: R.fetch(g) for g in INT_GROUPS}
            assert_planes(want[k]["planes"], got, label)
            rg = R.score()
            assert presence_violations(R) == 0, label
        try:
            compare_records(want[k]["full"], rg)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (label, e)) from None
    R.close()


def test_host_threads_with_two_handles_each(stream_data, gpu_lib):
    """C: four host threads (UVC_BENCH_VALUE_THREADS, the CLI's workers), each with uvcgpu_init and two handles of its own, twelve tiles dealt
    across them; each thread prepares one tile ahead and scores with release_state + kept_only -- no sync but the scores."""
    reads, want = stream_data
    n_threads, n_tiles = 4, 12
    tiles = [k % len(st.TILES) for k in range(n_tiles)]
    cols = device_columns(reads)
    got, errs = {}, []
    params = region.default_params(gpu_lib)

    def work(i):
        try:
            assert gpu_lib.dll.uvcgpu_init(0) == 0, gpu_lib.last_error()
            mine = list(range(i, n_tiles, n_threads))
            Rs = [None, None]

            def prepare(j):
                k = tiles[mine[j]]
                t, h = reads[k], j % 2
                if Rs[h] is None:
                    Rs[h] = region.Region(gpu_lib, params, t["tid"], t["beg"], t["end"], t["refseq"])
                else:
                    Rs[h].reset(t["tid"], t["beg"], t["end"], t["refseq"])
                if cols[k] is None:
                    Rs[h].set_reads(t)
                else:
                    Rs[h].set_reads_device((cols[k].soa, cols[k]))
                Rs[h].accumulate()
            prepare(0)
            for j in range(len(mine)):
                if j + 1 < len(mine):
                    prepare(j + 1)
                got[mine[j]] = Rs[j % 2].score(release_state=True, kept_only=True, capacity=st.KEPT_CAP)
            for R in Rs:
                if R is not None:
                    R.close()
        except Exception as e:   # noqa: BLE001
            errs.append((i, e))
    try:
        th = [threading.Thread(target=work, args=(i,)) for i in range(n_threads)]
        for t in th: t.start()
        for t in th: t.join()
    finally:
        for c in cols:
            if c is not None:
                c.free()
    assert not errs, errs
    assert sorted(got) == list(range(n_tiles))
    for j in range(n_tiles):
        _, expect = kept_groups(want[tiles[j]]["full"])
        try:
            compare_records(expect, got[j])
        except AssertionError as e:
            raise AssertionError("tile %d (set tile %d, thread %d): %s" % (j, tiles[j], j % n_threads, e)) from None


def test_bench_queue_count_in_a_fresh_process(stream_data, tmp_path):
    """D: stream A in a child process with bench.py's GPU_MAX_HW_QUEUES=16 (read by the runtime when it starts: a fresh process), where the
    streams of different handles run on hardware queues of their own; its records and planes are compared here."""
    reads, want = stream_data
    dst = tmp_path / "stream.npz"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    env.pop("UVCGPU_CHECK_PRESENCE", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "stream_worker.py"), str(dst)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "stream_worker.py exited with %d:\n%s" % (p.returncode, p.stderr[-3000:])
    z = np.load(dst)
    n = len(st.TILES)
    assert int(z["n_tiles"]) == n and z["queues"].item() == "16"
    fields = [f for f in want[0]["full"]]
    out1 = [dict(records={f: z["kept_%d_%s" % (k, f)] for f in fields}, scored=int(z["scored_%d" % k]), cap_asked=int(z["cap_asked_%d" % k]), enomem=bool(z["enomem_%d" % k]))
            for k in range(n)]
    out2 = [dict(records={f: z["all_%d_%s" % (k, f)] for f in fields}, planes={g: z["plane_%d_%s" % (k, g)] for g in INT_GROUPS}, presence=int(z["presence_%d" % k]))
            for k in range(n)]
    n_retry, n_enomem = check_kept_stream(out1, want, "kept-only stream, 16 queues")
    check_plane_stream(out2, want, "all-out stream, 16 queues")
    print("stream D: %d kept-only retries, %d ENOMEM retries; child: %s" % (n_retry, n_enomem, p.stdout.strip()[-200:]))
